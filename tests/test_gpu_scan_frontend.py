"""The device-resident scan front end: vba_scan_decode against the numpy restatement of Features::process +
pcl_handler (tests/decode_oracle.py), bit for bit; vba_scan_prepare against the three stand-alone calls (equal) and against the C++
oracle stage by stage (the bars of tests/test_gpu_scan.py and tests/test_gpu_pipeline.py for the same kernels); the retry; the
consumers on the device pointers."""
import dataclasses

import numpy as np
import pytest

import decode_oracle as do

pytestmark = pytest.mark.gpu

BLIND2 = 1.0
DEPT_ERR, BEAM_ERR = 0.02, 0.05


@pytest.fixture(scope="module")
def env():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    opt = capi.options_from_workload(synth.CONFIGS["room20k_w4"])
    opt.deterministic = 1
    ctx = capi.Context(opt)
    frame = ctx.scan_frame()
    yield capi, ctx, frame
    frame.close()
    ctx.close()


def _layout(capi, name):
    if name == "step80":                     # the ouster fields, 80 bytes apart: the global-load path of the decode kernel
        l = capi.scan_layout("ouster"); l.point_step = 80
        return l
    return capi.scan_layout(name)


def _times(layout, n, rng, t_max=0.13):
    t = rng.uniform(0.0, t_max, n)
    if n >= 8:                               # >= 5 % duplicated times, far apart in the message
        k = max(1, n // 12)
        t[rng.choice(n, k, replace=False)] = t[rng.choice(n, k, replace=False)]
    if layout.time_type == do.TIME_U32_DIV1E9:
        return (t * 1e9).astype(np.uint32)
    if layout.time_type == do.TIME_F32:
        t = t.astype(np.float32); t[-1] = np.float32(0.1)      # FP:176: a usable time field
        return t
    if layout.time_type == do.TIME_F64_REL_FIRST:
        return 1.7e9 + t                                       # relative to record 0: both signs
    return None


def _message(layout, n, seed, t_max=0.13):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    if n >= 8:
        a = n // 4
        xyz[a:a + max(1, n // 10)] *= np.float32(0.01)         # a block of records inside the blind sphere
    if n > 12:
        xyz[12] = (0, 1, 0)                                    # exactly on it (a candidate for point_filter_num 1, 3 and 4)
    inten = rng.integers(0, 256, n) if layout.intensity_type == do.INTENSITY_U8 else rng.uniform(0, 255, n).astype(np.float32)
    return do.make_message(layout, xyz, inten, _times(layout, n, rng, t_max))


def _check_decode(frame, layout, msg, pfn, blind2=BLIND2):
    want = do.decode(layout, msg, pfn, blind2)
    n, last = frame.decode(layout, msg, pfn, blind2)
    assert n == want["n"]
    assert last == want["last_curvature"]
    got = frame.read(0)
    for k in ("pnt", "intensity", "curvature"):
        g32 = got[k].astype(np.float32)
        np.testing.assert_array_equal(g32.astype(got[k].dtype), got[k], err_msg=k)       # float values carried in doubles
        np.testing.assert_array_equal(g32, want[k], err_msg=k)
    return want


# ---------------------------------------------------------------- 1. decode, bit for bit

@pytest.mark.parametrize("pfn", [1, 3, 4])
@pytest.mark.parametrize("n_raw", [1, 63, 257, 4097, 65795])
@pytest.mark.parametrize("name", ["livox", "hesai", "velodyne", "ouster", "tartanair"])
def test_decode_bit_for_bit(env, name, n_raw, pfn):
    capi, ctx, frame = env
    layout = _layout(capi, name)
    want = _check_decode(frame, layout, _message(layout, n_raw, 1000 * n_raw + pfn), pfn)
    if n_raw >= 257 and layout.filter:
        kept_of = (n_raw + pfn - 1) // pfn
        assert 0 < want["n"] < kept_of                                   # the blind test and the cut both removed something
        if pfn == 1:
            assert len(np.unique(want["curvature"])) < want["n"]         # ties among the kept points


# ---------------------------------------------------------------- 2. edges

def test_everything_filtered_gives_two_points(env):
    capi, ctx, frame = env
    layout = _layout(capi, "livox")
    msg = do.make_message(layout, np.full((300, 3), 0.1, np.float32), np.arange(300) % 256, np.arange(300) * 1000)
    want = _check_decode(frame, layout, msg, 1)
    assert want["n"] == 2 and want["last_curvature"] == float(np.float32(0.09))
    _check_decode(frame, layout, np.zeros(0, np.uint8), 3)               # n_raw = 0


def test_every_time_beyond_the_cut_gives_no_point(env):
    capi, ctx, frame = env
    layout = _layout(capi, "livox")
    rng = np.random.default_rng(5)
    msg = do.make_message(layout, rng.uniform(2, 9, (500, 3)), np.zeros(500), rng.integers(111_000_000, 200_000_000, 500))
    n, last = frame.decode(layout, msg, 1, BLIND2)
    assert (n, last) == (0, 0.0)
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    m, dp, dv = frame.prepare(np.zeros((0, 22)), ext, ext, 0.1, DEPT_ERR, BEAM_ERR)
    assert m == 0


def test_hesai_negative_relative_times(env):
    capi, ctx, frame = env
    layout = _layout(capi, "hesai")
    rng = np.random.default_rng(6)
    n = 1000
    t = 1.7e9 + rng.uniform(0.0, 0.1, n); t[0] = 1.7e9 + 0.06              # more than half of the records are earlier than record 0
    msg = do.make_message(layout, rng.uniform(2, 9, (n, 3)), rng.uniform(0, 255, n), t)
    want = _check_decode(frame, layout, msg, 1)
    assert (want["curvature"] < 0).sum() > n // 3 and want["n"] == n


def test_signed_zero_times_keep_message_order(env):
    capi, ctx, frame = env
    layout = _layout(capi, "velodyne")
    n = 600
    t = np.zeros(n, np.float32); t[::2] = -0.0; t[1::2] = 0.0; t[-1] = 0.05
    t[100] = -0.001; t[200] = 1e-6
    xyz = np.stack([np.arange(n) + 2.0, np.zeros(n), np.zeros(n)], axis=1)
    want = _check_decode(frame, layout, do.make_message(layout, xyz, None, t), 1)
    x = want["pnt"][:, 0] - 2
    assert x[0] == 100 and x[-1] == n - 1 and x[-2] == 200 and (np.diff(x[1:-2]) > 0).all()   # the zeros of either sign in message order


def test_velodyne_without_a_usable_time_field_is_unsupported(env):
    capi, ctx, frame = env
    layout = _layout(capi, "velodyne")
    t = np.full(64, 0.05, np.float32); t[-1] = 0.5
    with pytest.raises(capi.VbaError) as e:
        frame.decode(layout, do.make_message(layout, np.full((64, 3), 3.0), None, t), 1, BLIND2)
    assert e.value.status == capi.ERR_UNSUPPORTED


def test_bad_arguments(env):
    capi, ctx, frame = env
    layout = _layout(capi, "livox")
    msg = _message(layout, 64, 1)
    for bad in (dict(point_filter_num=0), dict(n_raw=-1)):
        with pytest.raises(capi.VbaError) as e:
            frame.decode(layout, msg, **{"point_filter_num": 1, "blind2": BLIND2, **bad})
        assert e.value.status == capi.ERR_BAD_ARG
    layout.off_z = 18
    with pytest.raises(capi.VbaError) as e:
        frame.decode(layout, msg, 1, BLIND2)
    assert e.value.status == capi.ERR_BAD_ARG
    fresh = ctx.scan_frame()
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    with pytest.raises(capi.VbaError) as e:                               # not decoded
        fresh.prepare(np.zeros((0, 22)), ext, ext, 0.1, DEPT_ERR, BEAM_ERR)
    assert e.value.status == capi.ERR_BAD_ARG
    fresh.close()


@pytest.mark.parametrize("n_raw,pfn", [(257, 1), (4097, 3)])
def test_step_80_equals_step_48(env, n_raw, pfn):
    capi, ctx, frame = env
    l48, l80 = _layout(capi, "ouster"), _layout(capi, "step80")
    a = _check_decode(frame, l48, _message(l48, n_raw, 77), pfn)
    b = _check_decode(frame, l80, _message(l80, n_raw, 77), pfn)
    for k in ("pnt", "intensity", "curvature"):
        np.testing.assert_array_equal(a[k], b[k])


# ---------------------------------------------------------------- 3. / 4. prepare

def _scan_inputs(seed=41, n=30000):
    """The input distribution of tests/test_gpu_scan.py::test_undistort_parity (points in +-30 m, times in [0, 0.1]) plus the dense
    clump of test_down_sampling_voxel_parity, as a Livox message; 21 IMU poses."""
    from scipy.spatial.transform import Rotation
    from test_gpu_scan import _imu_poses
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-30, 30, (n, 3)).astype(np.float32)
    pts[: n // 3] = (pts[: n // 3] * 0.05).astype(np.float32)
    t = (rng.uniform(0.0, 0.1, n) * 1e9).astype(np.uint32)
    ip = _imu_poses(21, rng, 0.1)
    end = np.concatenate([Rotation.from_rotvec(rng.normal(0, 0.05, 3)).as_matrix().ravel(), rng.normal(0, 0.2, 3)])
    ext = np.concatenate([Rotation.from_rotvec(rng.normal(0, 0.3, 3)).as_matrix().ravel(), rng.normal(0, 0.1, 3)])
    return pts, t, rng.integers(0, 256, n), ip, end, ext


@pytest.fixture(scope="module")
def prepared(env):
    """One decoded and prepared scan of about 30 000 points, its stages read back once."""
    capi, ctx, _ = env
    frame = ctx.scan_frame()
    pts, t, refl, ip, end, ext = _scan_inputs()
    layout = capi.scan_layout("livox")
    n, last = frame.decode(layout, do.make_message(layout, pts, refl, t), 1, 1e-4)
    assert 29000 < n <= 30000
    m, dp, dv = frame.prepare(ip, end, ext, 0.1, DEPT_ERR, BEAM_ERR, min_points=500)
    st = [frame.read(k) for k in range(4)]
    assert m == len(st[2]["pnt"]) == len(st[3]["pnt"]) and dp and dv
    yield dict(frame=frame, ip=ip, end=end, ext=ext, n=n, m=m, st=st)
    frame.close()


def test_prepare_equals_the_staged_path(env, prepared):
    capi, ctx, _ = env
    p = prepared; s0, s1, s2, s3 = p["st"]
    und = ctx.undistort(s0["pnt"], s0["curvature"], p["ip"], p["end"], p["ext"])
    assert (und != s0["pnt"]).any()
    np.testing.assert_array_equal(s1["pnt"], und)
    np.testing.assert_array_equal(s1["curvature"], s0["curvature"])
    pd, cnt, first = ctx.down_sampling_voxel(und, 0.1)
    assert len(pd) == p["m"] and cnt.max() > 1
    np.testing.assert_array_equal(s2["pnt"], pd); np.testing.assert_array_equal(s2["count"], cnt); np.testing.assert_array_equal(s2["first"], first)
    po, var = ctx.var_init(pd, p["ext"], DEPT_ERR, BEAM_ERR)
    np.testing.assert_array_equal(s3["pnt"], po); np.testing.assert_array_equal(s3["var"], var)


def test_prepare_point_notime_skips_the_undistortion(env, prepared):
    capi, ctx, _ = env
    p = prepared; frame = p["frame"]
    m, dp, dv = frame.prepare(p["ip"], p["end"], p["ext"], 0.1, DEPT_ERR, BEAM_ERR, point_notime=True)
    np.testing.assert_array_equal(frame.read(1)["pnt"], p["st"][0]["pnt"])
    np.testing.assert_array_equal(frame.read(0)["pnt"], p["st"][0]["pnt"])
    pd, cnt, first = ctx.down_sampling_voxel(p["st"][0]["pnt"], 0.1)
    assert m == len(pd)
    np.testing.assert_array_equal(frame.read(2)["first"], first)
    # a size below 0.001 leaves the cloud as it is (TL:203)
    m, dp, dv = frame.prepare(p["ip"], p["end"], p["ext"], 0.0005, DEPT_ERR, BEAM_ERR, point_notime=True)
    s2 = frame.read(2)
    assert m == p["n"] and (s2["count"] == 0).all() and (s2["first"] == np.arange(m)).all()
    np.testing.assert_array_equal(s2["pnt"], p["st"][0]["pnt"])
    # and preparing again from the same decoded cloud gives the first result again
    m, dp, dv = frame.prepare(p["ip"], p["end"], p["ext"], 0.1, DEPT_ERR, BEAM_ERR, min_points=500)
    assert m == p["m"]
    np.testing.assert_array_equal(frame.read(3)["var"], p["st"][3]["var"])


def test_prepare_against_the_oracle_stage_by_stage(oracle, prepared):
    p = prepared; s0, s1, s2, s3 = p["st"]
    # undistortion: the bars of test_undistort_parity
    want = oracle.undistort(s0["pnt"], s0["curvature"], p["ip"], p["end"], p["ext"])
    untouched = s0["curvature"] <= p["ip"][0, 0]
    np.testing.assert_array_equal(s1["pnt"][untouched], s0["pnt"][untouched])
    np.testing.assert_allclose(s1["pnt"], want, rtol=0, atol=np.spacing(np.float32(np.abs(want).max())) * 1.01)
    assert np.mean(s1["pnt"] == want) > 0.99
    # down-sampling of the DEVICE's undistorted cloud: the bars of test_down_sampling_voxel_parity
    o_out, o_cnt, o_first = oracle.down_sampling_voxel(s1["pnt"], 0.1)
    np.testing.assert_array_equal(s2["first"], o_first)
    np.testing.assert_array_equal(s2["count"], o_cnt)
    assert s2["count"].sum() == p["n"]
    np.testing.assert_allclose(s2["pnt"], o_out, rtol=0, atol=2e-6 * max(1.0, float(s2["count"].max()) ** 0.5) * 20)
    single = s2["count"] == 1
    np.testing.assert_array_equal(s2["pnt"][single], o_out[single])
    # var_init of the DEVICE's down-sampled cloud: the bar of test_scan_pipeline_stage_parity
    o_pnt, o_var = oracle.var_init(s2["pnt"], p["ext"], DEPT_ERR, BEAM_ERR)
    np.testing.assert_allclose(s3["var"], o_var, rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(s3["pnt"], o_pnt, rtol=1e-9, atol=1e-15)


# ---------------------------------------------------------------- 5. the retry

def test_retry_runs_from_the_undistorted_cloud(oracle, prepared):
    p = prepared; frame = p["frame"]
    und = p["st"][1]["pnt"]
    size, min_points = 6.0, 2000
    o1 = oracle.down_sampling_voxel(und, size)
    o2 = oracle.down_sampling_voxel(und, size / 2)
    o3 = oracle.down_sampling_voxel(o1[0], size / 2)
    # the premises, on the oracle: the first pass falls short, the second does not, and re-sampling the FIRST RESULT would differ
    assert len(o1[0]) < min_points <= len(o2[0]) and len(o3[0]) != len(o2[0])
    args = (p["ip"], p["end"], p["ext"], size, DEPT_ERR, BEAM_ERR)
    m, dp, dv = frame.prepare(*args, min_points=min_points)
    s2 = frame.read(2)
    assert m == len(o2[0])
    np.testing.assert_array_equal(s2["first"], o2[2]); np.testing.assert_array_equal(s2["count"], o2[1])
    np.testing.assert_array_equal(frame.read(1)["pnt"], und)
    m, dp, dv = frame.prepare(*args, min_points=0)                      # VS:1470-1474: no retry
    assert m == len(o1[0])
    np.testing.assert_array_equal(frame.read(2)["first"], o1[2])
    m, dp, dv = frame.prepare(*args, min_points=len(o1[0]))             # "< min_points": an equal count does not retry
    assert m == len(o1[0])
    m, dp, dv = frame.prepare(*args, min_points=len(o1[0]) + 1)
    assert m == len(o2[0])
    m, dp, dv = frame.prepare(*args, min_points=10 ** 9)                # the second result is kept whatever its count
    assert m == len(o2[0])


# ---------------------------------------------------------------- 6. allocations, contexts, consumers

def test_no_allocation_inside_the_reservation(env):
    capi, ctx, _ = env
    frame = ctx.scan_frame()
    frame.reserve(70000, 48)
    a0 = frame.allocations()
    for name, n_raw in (("ouster", 70000), ("hesai", 4097), ("livox", 65795)):
        layout = _layout(capi, name)
        frame.decode(layout, _message(layout, n_raw, 3, t_max=0.1), 1, BLIND2)
        ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
        frame.prepare(np.zeros((0, 22)), ext, ext, 0.5, DEPT_ERR, BEAM_ERR)
    assert frame.allocations() == a0
    layout = _layout(capi, "tartanair")
    n, last = frame.decode(layout, _message(layout, 140001, 4), 1, BLIND2)      # outgrows it: the buffers double
    assert n == 140001
    a1 = frame.allocations()
    assert a1[0] > a0[0] and a1[1] > a0[1]
    frame.close()


def test_device_pointers_feed_the_map_and_another_context_prepares(env, prepared):
    capi, ctx, _ = env
    from voxel_slam_amd import synth
    p = prepared; frame = p["frame"]
    args = (p["ip"], p["end"], p["ext"], 0.1, DEPT_ERR, BEAM_ERR)
    opt = capi.options_from_workload(synth.CONFIGS["room20k_w4"]); opt.deterministic = 1
    other = capi.Context(opt)
    m, dp, dv = frame.prepare(*args, ctx=other)                         # decoded on ctx, prepared on another context of the device
    assert m == p["m"]
    s3 = frame.read(3)
    np.testing.assert_array_equal(s3["pnt"], p["st"][3]["pnt"]); np.testing.assert_array_equal(s3["var"], p["st"][3]["var"])
    pose = np.concatenate([np.eye(3).ravel(), np.zeros(3)]); cov = np.eye(15) * 1e-4
    other.pvec_update_cut_voxel_dev(0, m, dp, dv, pose, cov)            # in place, on the stream that prepared it
    host = capi.Context(opt)
    host.pvec_update_cut_voxel(0, s3["pnt"], s3["var"], pose, cov)
    a, b = other.dump_leaves(), host.dump_leaves()
    assert len(a) == len(b) > 100
    key = lambda d: d[np.lexsort(d[:, :5].T[::-1])]
    np.testing.assert_array_equal(key(a), key(b))
    other.synchronize()
    host.close(); other.close()


def test_device_pointers_feed_the_odometry(env):
    capi, ctx0, _ = env
    from voxel_slam_amd import synth
    from test_gpu_odom import _rand_var
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=4)
    W, nscan = wl.win_size, 6
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    ctx = capi.Context(capi.options_from_workload(wl))
    xs, win_count = [], 0
    for k in range(nscan - 1):                                          # local mapping on the true poses: builds and refreshes the planes
        xs.append(synth.poses_flat(s["R_gt"][k:k + 1], s["p_gt"][k:k + 1])[0])
        win_count += 1
        ctx.cut_voxel(win_count - 1, s["points"][k], xs[-1], var=_rand_var(len(s["points"][k]), 100 + k), multi=True)
        ctx.recut(win_count, np.array(xs), multi=True)
        if win_count >= W:
            ctx.margi(win_count, np.array(xs), jour=float(k))
            ctx.slide(1); xs = xs[1:]; win_count -= 1
    k = nscan - 1
    pts = s["points"][k].astype(np.float32)
    layout = capi.scan_layout("tartanair")
    frame = ctx.scan_frame()
    n, last = frame.decode(layout, do.make_message(layout, pts), 1, 0.0)
    assert n == len(pts) and last == 0.0
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    m, dp, dv = frame.prepare(None, None, ext, 0.05, DEPT_ERR, BEAM_ERR, point_notime=True)
    s3 = frame.read(3)
    state = np.zeros(25)
    state[1:10] = s["R_gt"][k].ravel(); state[10:13] = s["p_gt"][k] + 0.02
    state[13:16] = [1.0, 0.5, 0.0]; state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4; cov[9:, 9:] = np.eye(6) * 1e-5
    ok_d, st_d, cov_d = ctx.lio_state_estimation_dev(m, dp, dv, state, cov)
    ok_h, st_h, cov_h = ctx.lio_state_estimation(s3["pnt"], s3["var"], state, cov)
    assert ok_d == ok_h
    assert (st_d != state).any()
    np.testing.assert_array_equal(st_d, st_h)                           # the same kernels on the same values, sums by workgroup partials
    np.testing.assert_array_equal(cov_d, cov_h)
    frame.close(); ctx.close()
