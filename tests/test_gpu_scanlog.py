"""The scan log (vba_scanlog_*) on the MI355X: the capture of the map's scan ring, the keyframe build and the
loop update fed from the log, the export of pub_localmap, the ordering of a device-destination export against later pushes, and the
float form of a read.  Every comparison is np.array_equal, except the kept keyframe values in default (atomic) mode, which are held
against the CPU oracle's down_sampling_pvec with the one-float-spacing rule stated at _within_one_float_spacing."""
import numpy as np
import pytest

import export_oracle as eo
import kf_oracle as ko
import loop_oracle as lo

pytestmark = pytest.mark.gpu

VS10 = 0.5 / 10            # voxel_size / 10 of VS:2385 at Odometry/voxel_size 0.5
SENT = np.float32(-12345.5)


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


@pytest.fixture(scope="module")
def synth():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth as s
    return s


def _ctx(capi, **kw):
    o = capi.default_options()
    o.device = 0
    for k, v in kw.items():
        setattr(o, k, v)
    return capi.Context(o)


def _wl_ctx(capi, wl, **kw):
    o = capi.options_from_workload(wl)
    o.device = 0
    for k, v in kw.items():
        setattr(o, k, v)
    return capi.Context(o)


def _hip():
    """the HIP runtime libvoxelba.so has already loaded (for a device buffer of the test's own)"""
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _vars(rng, n):
    """n symmetric positive semi-definite 3x3 rows [n][9] of the size of a measurement covariance"""
    a = rng.normal(0, 1e-2, (n, 3, 3))
    return np.ascontiguousarray((a @ a.transpose(0, 2, 1)).reshape(n, 9))


def _poses(n, seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([Rotation.from_rotvec(rng.uniform(-1.2, 1.2, 3)).as_matrix().ravel(), rng.uniform(-40, 40, 3)]) for _ in range(n)])


def _check_live(log, want):
    """every live scan reads back as the arrays in want[seq], bit for bit; returns the live range"""
    first, end, sizes = log.range()
    assert end - first == len(sizes)
    for seq in range(first, end):
        pnt, var = log.read(seq)
        wp, wv = want[seq]
        assert sizes[seq - first] == len(wp) == len(pnt), seq
        assert np.array_equal(pnt, wp), seq
        assert np.array_equal(var, wv), seq
    return first, end


# ---------------------------------------------------------------- 1, 2: capture and its refusals
@pytest.mark.parametrize("with_var", [True, False])
def test_capture_from_the_ring(capi, synth, with_var):
    """Scans of 0, 1, 255, 256, 257 and 3000 points go through a window of W = 4 that slides twice (mp is rotated); at three moments
    every frame is pushed, in an order other than the frame order.  The log is reserved so that the last push of the second round
    skips the arena's tail (a wrap without growth: the allocation counter stands still) and the third round forces a growth."""
    wl = synth.CONFIGS["room20k_w4"]
    W = wl.win_size
    assert W == 4
    s = synth.make_scans(wl)
    poses_all = synth.poses_flat(s["R0"], s["p0"])
    rng = np.random.default_rng(7)
    sizes = [256, 0, 3000, 1, 255, 257]
    scans = []
    for i, n in enumerate(sizes):
        p = np.ascontiguousarray(s["points"][i % W][17 * i:17 * i + n])
        scans.append((p, _vars(rng, n) if with_var else np.zeros((n, 9)), poses_all[i % W]))
    ctx = _wl_ctx(capi, wl)
    log = ctx.scan_log()
    log.reserve(4000, 16)
    alloc0 = log.allocations()
    window = []                                   # scan index per frame

    def insert(frame, k):
        p, v, x = scans[k]
        ctx.cut_voxel(frame, p, x, var=v if with_var else None, multi=True)

    def poses():
        return np.ascontiguousarray(np.stack([scans[k][2] for k in window]))

    want = {}

    def push_all(order):
        for f in order:
            seq = log.push_window(f)
            want[seq] = scans[window[f]][:2]
            assert seq == len(want) - 1           # numbers go up by one per push

    def slide(k_new):
        ctx.evaluate_only_residual(poses())
        ctx.margi(len(window), poses(), jour=0.0)
        # after margi the outgoing slot's count is gone: the calling rule of vba_scanlog_push_window
        seq = log.push_window(0)
        want[seq] = (np.zeros((0, 3)), np.zeros((0, 9)))
        assert log.read(seq)[0].shape == (0, 3)
        ctx.slide(1)
        window.pop(0)
        insert(W - 1, k_new)
        window.append(k_new)
        ctx.recut(W, poses(), multi=True)

    for j in range(W):
        insert(j, j)
        window.append(j)
    ctx.recut(W, poses(), multi=True)
    push_all([2, 0, 3, 1])                        # 3000, 256, 1, 0 points: 3257 of 4000 rows
    assert _check_live(log, want) == (0, 4)
    assert log.allocations() == alloc0
    slide(4)                                      # frames now hold scans 1, 2, 3, 4 (0, 3000, 1, 255 points), slots rotated by one
    log.release(2)                                # the scans of 1 and 0 points and the empty one of the calling rule stay: rows [0, 3256) are free
    push_all([2, 0, 3, 1])                        # 1 | 0 | 255 behind the head; 3000 does not fit the 487-row tail: wrapped to row 0
    assert _check_live(log, want) == (2, 9)
    assert log.allocations() == alloc0            # a wrap, not a growth
    slide(5)                                      # frames hold scans 2, 3, 4, 5
    push_all([1, 3, 0, 2])                        # 1 | 257 (rows [3001, 3256) are too few: forces the growth) | 3000 | 255
    assert _check_live(log, want) == (2, 14)      # numbers and contents kept across the growth
    a1 = log.allocations()
    assert a1[0] == alloc0[0] + 1 and a1[1] > alloc0[1]
    # a frame outside the window; a sharded context
    for f in (-1, W):
        with pytest.raises(capi.VbaError) as e:
            log.push_window(f)
        assert e.value.status == capi.ERR_BAD_ARG
    ctx.set_shard(0, 2)
    with pytest.raises(capi.VbaError) as e:
        log.push_window(0)
    assert e.value.status == capi.ERR_UNSUPPORTED
    ctx.set_shard(0, 1)
    assert log.range()[1] == 14
    # 7: the float form is the doubles narrowed once
    for seq in (5, 8, 12):
        pnt, var, xyz = log.read(seq, xyz=True)
        assert xyz.dtype == np.float32 and np.array_equal(xyz, pnt.astype(np.float32)), seq
    with pytest.raises(capi.VbaError) as e:
        log.read(1)                               # released
    assert e.value.status == capi.ERR_BAD_ARG
    ctx.close()


# ---------------------------------------------------------------- 3: keyframes
def _within_one_float_spacing(got, want, what):
    """Both sides form a voxel's mean in double (relative error ~1e-13) and round it ONCE to float, so they can differ only where
    that rounding straddles the two double values: by one spacing of the float grid at the expected value, never more."""
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want)
    worst = float((err / bound).max()) if len(want) else 0.0
    print("%s: %d values, %d differ, largest difference %.3g float spacings" % (what, want.size, int((err > 0).sum()), worst))
    assert (err <= bound).all(), "%s: %d values further than one float spacing, worst %.3g spacings" % (what, int((err > bound).sum()), worst)


@pytest.fixture(scope="module")
def kf_scans(synth):
    """four scans of 3000 points on the keyframe path, with body covariances"""
    kf = synth.make_keyframe_path(n_kf=1, scans_per_kf=4, n_pts=3000, scan_step=0.02)[0]
    return kf


def _db(capi, ctx):
    db = ctx.btc_db(capi.btc_default_config(0))
    db.set_gen_config(capi.btc_default_gen_config(0))
    return db


@pytest.mark.parametrize("det", [1, 0])
def test_keyframes_from_the_log(capi, oracle, kf_scans, det):
    """vba_kf_build_from_log against vba_kf_build on the host arrays that read returns: k = 1, and k = 3 with an empty scan in the
    middle whose scans lie on both sides of the wrap (arena rows 3000.., 6000 (empty), 0..)."""
    P, V, X = kf_scans["points"], kf_scans["vars"], kf_scans["poses"]
    n = [len(p) for p in P]
    ctx = _ctx(capi, deterministic=det)
    sctx = _ctx(capi, deterministic=det)             # the stores hang off another context of the device
    log = ctx.scan_log()
    cap = n[0] + n[1] + 2000
    log.reserve(cap, 8)
    s_log, s_ref = sctx.kf_store(), sctx.kf_store()
    db_log, db_ref = _db(capi, sctx), _db(capi, sctx)
    for st in (s_log, s_ref):
        st.reserve(4 * sum(n), 8, 2 * sum(n))
    assert log.push_points(P[0], V[0]) == 0          # rows [0, n0): released below
    assert log.push_points(P[1], V[1]) == 1          # rows [n0, n0 + n1)
    assert log.push_points(np.zeros((0, 3))) == 2    # empty, at the head
    log.release(1)
    assert n[2] > 2000 and n[2] <= n[0]
    assert log.push_points(P[2], V[2]) == 3          # the tail of 2000 rows is too short: row 0
    a_log, a_st = log.allocations(), s_log.allocations()
    host = {q: log.read(q) for q in (1, 2, 3)}
    assert np.array_equal(host[1][0], P[1]) and np.array_equal(host[1][1], V[1]) and np.array_equal(host[3][0], P[2])
    builds = [([1], X[1:2]), ([1, 2, 3], np.stack([X[1], X[3], X[2]]))]           # (the empty scan's pose is anybody's)
    for kf_i, (seqs, poses) in enumerate(builds):
        got = s_log.build_from_log(log, seqs[0], poses, VS10, id=40 + kf_i, jour=1.5, db=db_log)
        ref = s_ref.build([host[q][0] for q in seqs], poses, VS10, id=40 + kf_i, jour=1.5, vars=[host[q][1] for q in seqs], db=db_ref)
        assert got[0] == ref[0] > 0
        assert np.array_equal(s_log.last_counts(), s_ref.last_counts())
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])                     # descriptor rows and bits
        assert np.array_equal(db_log.plane_cloud(kf_i), db_ref.plane_cloud(kf_i)) and len(db_ref.plane_cloud(kf_i)) > 0
        xyz, vd = s_log.read(kf_i)
        rxyz, rvd = s_ref.read(kf_i)
        if det:
            assert np.array_equal(xyz, rxyz) and np.array_equal(vd, rvd)
        else:
            merged = ko.merge([host[q][0] for q in seqs], poses)
            o_out, o_vd, o_cnt = oracle.down_sampling_pvec(merged, np.concatenate([host[q][1] for q in seqs]), VS10)
            assert np.array_equal(s_log.last_counts(), o_cnt)
            _within_one_float_spacing(xyz, o_out, "kept cloud from the log, k = %d" % len(seqs))
            _within_one_float_spacing(vd, o_vd, "covariance diagonals from the log, k = %d" % len(seqs))
        g = s_log.get(kf_i)
        assert np.array_equal(g["x0"], poses[-1]) and (g["id"], g["jour"], g["exist"], g["n_points"]) == (40 + kf_i, 1.5, 0, got[0])
    assert log.allocations() == a_log and s_log.allocations() == a_st       # reserved: neither counter moves
    # a range reaching past end, or before first after a release: refused, the store untouched
    for first, k in ((3, 2), (0, 2), (4, 1), (-1, 1)):
        with pytest.raises(capi.VbaError) as e:
            s_log.build_from_log(log, first, np.stack([X[0]] * k), VS10, id=99)
        assert e.value.status == capi.ERR_BAD_ARG
    assert s_log.size() == 2 and db_log.num_frames() == 2
    sctx.close(); ctx.close()


# ---------------------------------------------------------------- 4: loop update
@pytest.fixture(scope="module")
def ses(synth):
    return lo.make_session(synth, n_kf=5, k_bl=3, W=4, extra=1, n_pts=4000)


def _state(pose):
    s = np.zeros(25); s[1:10] = pose[:9]; s[10:13] = pose[9:]
    return s


def _history(capi, ses, ctx, log):
    """fill the window, then slide it k_bl times; every outgoing scan is pushed before its margi.  Covariances are formed on the
    device (pvec_update fused with the insertion).  Returns (window scan indices, marginalised scan indices)."""
    W, base = ses["W"], ses["n_kf"]
    window, bl = [], []

    def insert(slot, k):
        ctx.pvec_update_cut_voxel(slot, ses["points"][k], ses["vars"][k], ses["poses"][k], ses["cov"], multi=True)

    def poses():
        return np.ascontiguousarray(ses["poses"][window])

    for j in range(W):
        insert(j, base + j)
        window.append(base + j)
    ctx.recut(W, poses(), multi=True)
    nxt = base + W
    for step in range(ses["k_bl"]):
        ctx.evaluate_only_residual(poses())
        assert log.push_window(0) == step
        ctx.margi(len(window), poses(), jour=float(step))
        ctx.slide(1)
        bl.append(window.pop(0))
        insert(W - 1, nxt)
        window.append(nxt)
        nxt += 1
        ctx.recut(len(window), poses(), multi=True)
    return window, bl


def test_loop_update_from_the_log(capi, ses):
    """Context A: vba_loop_update with the buf_lba2loop scans as host arrays read back from its log.  Context B:
    vba_scanlog_loop_update.  deterministic = 1: the maps and the factor count are equal bit for bit."""
    wl, dx = ses["wl"], ses["dx"]
    out = []
    for from_log in (False, True):
        ctx = _wl_ctx(capi, wl, deterministic=1)
        log = ctx.scan_log()
        window, bl = _history(capi, ses, ctx, log)
        store = ctx.kf_store()
        for i in range(ses["n_kf"]):
            store.build([ses["points"][i]], ses["poses"][i][None, :], VS10, id=i, jour=0.5 * i, vars=[ses["vars"][i]])
        store.set_poses(0, np.array([lo.move_pose(ses["poses"][i], dx) for i in range(store.size())]))
        lm = ctx.loop_map()
        lm.build(store, 5, True)
        first, end, sizes = log.range()
        assert (first, end) == (0, len(bl)) and [int(x) for x in sizes] == [len(ses["points"][k]) for k in bl]
        bl_poses = np.array([lo.move_pose(ses["poses"][k], dx) for k in bl])
        win_poses = np.array([lo.move_pose(ses["poses"][k], dx) for k in window])
        if from_log:
            nf = ctx.scanlog_loop_update(lm, win_poses, log, 0, bl_poses, dx12=dx)
        else:
            rd = [log.read(q) for q in range(first, end)]
            for (p, v), k in zip(rd, bl):
                assert np.array_equal(p, ses["points"][k]) and v.any() and not np.array_equal(v, ses["vars"][k])   # world covariances
            nf = ctx.loop_update(lm, win_poses, [r[0] for r in rd], bl_poses, [r[1] for r in rd], dx12=dx)
        out.append((nf, ctx.num_roots(), ctx.dump_leaves(), ctx.dump_plane_var()))
        if from_log:
            with pytest.raises(capi.VbaError) as e:                      # a range that is not wholly live; the map stays
                ctx.scanlog_loop_update(lm, win_poses, log, 1, bl_poses, dx12=dx)
            assert e.value.status == capi.ERR_BAD_ARG
            assert np.array_equal(ctx.dump_leaves(), out[-1][2])
        ctx.close()
    a, b = out
    print("factors %d, roots %d, leaves %d" % (a[0], a[1], len(a[2])))
    assert a[0] == b[0] > 0 and a[1] == b[1] > 0
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---------------------------------------------------------------- 5, 6: export
EXPORT_SIZES = [6, 7, 8, 0, 601]      # size % 3 in {0, 1, 2}, an empty scan, more than two workgroups


def _export_log(capi, ctx, seed):
    rng = np.random.default_rng(seed)
    log = ctx.scan_log()
    clouds = [np.ascontiguousarray(rng.uniform(-30, 30, (n, 3))) for n in EXPORT_SIZES]
    for c in clouds:
        log.push_points(c)
    return log, clouds, _poses(len(clouds), seed + 1)


@pytest.mark.parametrize("stride", [1, 3])
def test_export_world(capi, stride):
    ctx = _ctx(capi)
    ectx = _ctx(capi)                                 # the export may run on another context of the device
    log, clouds, poses = _export_log(capi, ctx, 21)
    want = eo.points(clouds, poses, [4.0] * len(clouds), stride)
    assert len(want) == sum((n + stride - 1) // stride for n in EXPORT_SIZES)
    for c in (ctx, ectx):
        got = log.export_world(0, poses, stride, 4.0, ctx=c)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    # a window of the scans
    assert np.array_equal(log.export_world(1, poses[1:4], stride, 4.0), eo.points(clouds[1:4], poses[1:4], [4.0] * 3, stride))
    # a device destination
    C = capi.C
    hip = _hip()
    buf = np.full((len(want) + 8, 4), SENT, dtype=np.float32)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(buf.nbytes)) == 0
    assert hip.hipMemcpy(d, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice
    # a cap one record short: refused, the destination untouched (host and device)
    host = np.full((len(want), 4), SENT, dtype=np.float32)
    n_out = C.c_int64()
    args = (ectx.h, log.h, C.c_int64(0), C.c_int(len(poses)), capi._p(np.ascontiguousarray(poses)), C.c_int(stride), C.c_float(4.0), C.c_int64(len(want) - 1))
    assert ctx.lib.vba_scanlog_export_world(*args, host.ctypes.data_as(C.c_void_p), C.byref(n_out)) == capi.ERR_BAD_ARG
    assert n_out.value == len(want) and (host == SENT).all()
    assert ctx.lib.vba_scanlog_export_world(*args, d, C.byref(n_out)) == capi.ERR_BAD_ARG
    assert log.export_world(0, poses, stride, 4.0, ctx=ectx, out=d, cap=len(want)) == len(want)
    ectx.synchronize()
    assert hip.hipMemcpy(buf.ctypes.data_as(C.c_void_p), d, C.c_size_t(buf.nbytes), C.c_int(2)) == 0      # hipMemcpyDeviceToHost
    assert hip.hipFree(d) == 0
    assert np.array_equal(buf[:len(want)], want)
    assert (buf[len(want):] == SENT).all()
    # a range that is not live
    with pytest.raises(capi.VbaError) as e:
        log.export_world(3, poses[:3], stride, 4.0, cap=1000)
    assert e.value.status == capi.ERR_BAD_ARG
    ectx.close(); ctx.close()


def test_device_export_is_ordered_before_the_overwrite(capi):
    """An export into device memory on ANOTHER context's stream returns with the gather queued; the scans are then released and
    enough scans pushed to write over every row it reads (the arena is reserved, so nothing grows), and only then is anything
    synchronised.  The buffer holds the oracle's records: the pushes waited for the export's event on their own stream."""
    ctx, ectx = _ctx(capi), _ctx(capi)
    rng = np.random.default_rng(33)
    sizes = [50000, 50001, 49999]
    log = ctx.scan_log()
    log.reserve(sum(sizes), 16)
    clouds = [np.ascontiguousarray(rng.uniform(-30, 30, (n, 3))) for n in sizes]
    over = [np.ascontiguousarray(rng.uniform(100, 200, (n, 3))) for n in sizes]
    poses = _poses(3, 34)
    for c in clouds:
        log.push_points(c)
    a0 = log.allocations()
    want = eo.points(clouds, poses, [1.0] * 3, 1)
    C = capi.C
    hip = _hip()
    buf = np.zeros((len(want), 4), dtype=np.float32)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(buf.nbytes)) == 0
    assert log.export_world(0, poses, 1, 1.0, ctx=ectx, out=d, cap=len(want)) == len(want)
    log.release(3)
    for c in over:
        log.push_points(c)                            # rows 0 .. of the arena again
    assert log.allocations() == a0
    ectx.synchronize(); ctx.synchronize()
    assert hip.hipMemcpy(buf.ctypes.data_as(C.c_void_p), d, C.c_size_t(buf.nbytes), C.c_int(2)) == 0      # hipMemcpyDeviceToHost
    assert hip.hipFree(d) == 0
    assert np.array_equal(buf, want)
    assert np.array_equal(log.read(3)[0], over[0]) and np.array_equal(log.read(5)[0], over[2])
    ectx.close(); ctx.close()
