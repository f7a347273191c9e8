"""GPU tests of the odometry state resident in HBM: the IMU propagation on the device against the
high-precision reference and counted bars of tests/imu_ekf_ref.py, and the on-state calls (prepare, scan-to-map update, insertion)
against the host-fed calls they stand in for, BIT FOR BIT: the device builds the same image (P^-1 by inverse15_pplu, the restatement of
the host inverse) and the same kernels run on it.  The scene is that of test_gpu_odom_resident.py (room20k, W = 4), built without the
oracle: nothing here is compared with it."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import imu_ekf_ref as R

pytestmark = pytest.mark.gpu

EXT = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
DOWN_SIZE = 0.05


class Dev:
    """A scan's points and covariances as torch tensors on the context's device."""

    def __init__(self, pts, var):
        import torch
        self.n = len(pts)
        self.p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)).to("cuda:0")
        self.v = torch.from_numpy(np.ascontiguousarray(var, dtype=np.float64).reshape(-1, 9)).to("cuda:0")
        torch.cuda.synchronize()

    @property
    def args(self):
        return self.n, (self.p.data_ptr() if self.n else 0), (self.v.data_ptr() if self.n else 0)


def build_map(sc, ctx):
    """the local-mapping session of test_gpu_odom_resident.py's scene on GT poses; returns (win_count, window poses)"""
    from test_gpu_odom import _rand_var
    synth, s, W = sc["synth"], sc["scans"], sc["wl"].win_size
    xs, wc = [], 0
    for k in range(sc["nscan"] - 1):
        xs.append(synth.poses_flat(s["R_gt"][k:k + 1], s["p_gt"][k:k + 1])[0])
        wc += 1
        ctx.cut_voxel(wc - 1, s["points"][k], xs[-1], var=_rand_var(len(s["points"][k]), 100 + k), multi=True)
        ctx.recut(wc, np.array(xs), multi=True)
        if wc >= W:
            ctx.margi(wc, np.array(xs), jour=float(k))
            ctx.slide(1); xs = xs[1:]; wc -= 1
    return wc, xs


@pytest.fixture(scope="module")
def scene():
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")                   # torch's HIP runtime comes up first, as in bench.py: the library then shares it
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    from test_gpu_odom import _rand_var
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=4)
    nscan = 8
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    sc = dict(capi=capi, synth=synth, wl=wl, scans=s, nscan=nscan)
    ctx = capi.Context(capi.options_from_workload(wl))
    sc["win_count"], _ = build_map(sc, ctx)
    k = nscan - 1
    rng = np.random.default_rng(5)                    # the perturbed prediction of test_gpu_odom_resident.py
    state = np.zeros(25)
    state[1:10] = (s["R_gt"][k] @ synth.so3_exp(rng.normal(0, np.radians(0.2), 3))).ravel()
    state[10:13] = s["p_gt"][k] + rng.normal(0, 0.02, 3)
    state[13:16] = [1.0, 0.5, 0.0]; state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4
    cov[9:, 9:] = np.eye(6) * 1e-5
    pts = s["points"][k]
    var_b = _rand_var(len(pts), 999, scale=0.005)
    sc.update(ctx=ctx, pts=pts, var=var_b, state=state, cov=cov, dev=Dev(pts, var_b), st=ctx.odom_state())
    yield sc
    ctx.close()


@pytest.fixture(scope="module")
def corpus():
    c = R.corpus()
    return {k: (v, R.reference(v)) for k, v in c.items()}


def _propagate(st, case):
    st.set(case["state"], case["cov"])
    n = st.propagate(case["imu"], case["noise"], case["last_end"], case["beg"], case["end"], case["sg"])
    state, cov = st.get()
    poses, end = st.poses()
    return dict(n=n, state=state, cov=cov.ravel(), poses=poses, end_pose=end)


# ------------------------------------------------------------------------------------------------ propagation
@pytest.mark.parametrize("name", ("m6", "m21", "m64", "still", "repeat"))
def test_propagation_within_the_bars(scene, corpus, name):
    case, ref = corpus[name]
    st = scene["st"]
    got = _propagate(st, case)
    assert got["n"] == ref["n"] == len(got["poses"])               # the host's count is the device's
    q = R.ratios(ref, got)
    print("%-8s " % name + "  ".join("%s %.3g of its bar (k <= %d)" % (k, v[0], v[1]) for k, v in q.items()))
    assert all(v[0] <= 1.0 for v in q.values()), q
    assert got["state"][0] == case["end"] and np.array_equal(got["state"][16:25], case["state"][16:25])
    assert np.array_equal(got["end_pose"], got["state"][1:13])
    again = _propagate(st, case)
    for k in ("state", "cov", "poses", "end_pose"):
        assert np.array_equal(got[k], again[k]), k


def test_propagation_grows_its_table(scene, corpus):
    """129 IMU rows on an object created for 64: the table grows by doubling, the result is that of a fresh object"""
    capi, ctx = scene["capi"], scene["ctx"]
    case = dict(corpus["m64"][0])
    rng = np.random.default_rng(3)
    m = 129
    imu = np.zeros((m, 7)); imu[:, 0] = case["imu"][0, 0] + 0.0008 * np.arange(m); imu[:, 1:] = np.resize(case["imu"][:, 1:], (m, 6)) + rng.normal(0, 1e-3, (m, 6))
    case.update(m=m, imu=imu, end=float(imu[-1, 0] + 0.0003))
    small, big = ctx.odom_state(), ctx.odom_state()
    try:
        big.reserve(200)
        a0, b0 = small.allocations(), big.allocations()
        a, b = _propagate(small, case), _propagate(big, case)
        assert small.allocations()[0] > a0[0] and big.allocations() == b0
        want = capi.imu_ekf_propagate(case["imu"], case["noise"], case["last_end"], case["beg"], case["end"], case["state"], case["cov"], case["sg"])
        assert a["n"] == b["n"] == len(want[2]) > 64
        for k in ("state", "cov", "poses", "end_pose"):
            assert np.array_equal(a[k], b[k]), k
    finally:
        small.close(); big.close()


# ------------------------------------------------------------------------------------------------ inverse and loop
def _same_report(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def _on_state_equals_resident(sc, ctx, args, state, cov):
    st = sc["st"] if ctx is sc["ctx"] else ctx.odom_state()
    want = ctx.lio_state_estimation_resident(*args, state, cov)
    st.set(state, cov)
    ok, x, rep = st.lio_state_estimation(*args, ctx=ctx)
    x2, cov2 = st.get()
    assert ok == want[0] and np.array_equal(x, want[1]) and np.array_equal(x2, want[1])
    assert np.array_equal(cov2, want[2].reshape(15, 15))
    assert _same_report(rep, want[3]), (rep, want[3])
    return want


def test_update_is_the_resident_call_bit_for_bit(scene):
    sc = scene
    ok, x, cv, rep = _on_state_equals_resident(sc, sc["ctx"], sc["dev"].args, sc["state"], sc["cov"])
    print("iterations %d, match_num %s, ok %s" % (rep["iterations"], rep["match_num"], ok))
    assert rep["iterations"] >= 3 and rep["match_num"][0] > 2000 and (x != sc["state"]).any()
    # a covariance that is not a multiple of the identity: the inverse works for its result, and twice gives the same bits
    rng = np.random.default_rng(11)
    A = rng.normal(0, 1, (15, 15))
    cov = 1e-5 * (A @ A.T) / 15 + sc["cov"]
    a = _on_state_equals_resident(sc, sc["ctx"], sc["dev"].args, sc["state"], cov)
    b = _on_state_equals_resident(sc, sc["ctx"], sc["dev"].args, sc["state"], cov)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_update_in_deterministic_mode(scene):
    """with vba_options::deterministic the on-state update is the resident call's bits too, run to run"""
    sc = scene
    opt = sc["capi"].options_from_workload(sc["wl"])
    opt.deterministic = 1
    ctx = sc["capi"].Context(opt)
    try:
        build_map(sc, ctx)
        a = _on_state_equals_resident(sc, ctx, sc["dev"].args, sc["state"], sc["cov"])
        b = _on_state_equals_resident(sc, ctx, sc["dev"].args, sc["state"], sc["cov"])
        assert a[3]["iterations"] >= 3 and a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    finally:
        ctx.close()


def test_update_degenerate_forms(scene):
    """n = 0, and a context whose map was never allocated"""
    sc = scene
    ok, x, cv, rep = _on_state_equals_resident(sc, sc["ctx"], (0, 0, 0), sc["state"], sc["cov"])
    assert not ok and np.array_equal(x, sc["state"]) and rep["iterations"] == 2
    fresh = sc["capi"].Context(sc["capi"].options_from_workload(sc["wl"]))
    try:
        for args in (sc["dev"].args, (0, 0, 0)):
            ok, x, cv, rep = _on_state_equals_resident(sc, fresh, args, sc["state"], sc["cov"])
            assert not ok and np.array_equal(x, sc["state"]) and np.array_equal(cv, sc["cov"].reshape(cv.shape))
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ prepare, insertion, chain
def _message(sc, seed):
    import decode_oracle as do
    rng = np.random.default_rng(seed)
    layout = sc["capi"].scan_layout("hesai")
    pts = sc["pts"].astype(np.float32)
    return layout, do.make_message(layout, pts, rng.uniform(0, 255, len(pts)), 1.7e9 + np.sort(rng.uniform(0.0, 0.1, len(pts))))


def _imu_rows(sc, rng, t0, R_wb, m=21):
    """m rows at 200 Hz from t0: a sensor nearly at rest in attitude R_wb"""
    imu = np.zeros((m, 7))
    imu[:, 0] = t0 + 0.005 * np.arange(m)
    imu[:, 1:4] = rng.normal(0, 0.02, (m, 3))
    imu[:, 4:7] = R_wb.T @ np.array([0, 0, 9.8]) + rng.normal(0, 0.05, (m, 3))
    return imu


def test_prepare_on_state_is_prepare_on_the_table(scene):
    sc = scene
    ctx, st = sc["ctx"], sc["st"]
    layout, msg = _message(sc, 1)
    rng = np.random.default_rng(2)
    state = sc["state"].copy(); state[13:16] = [0.3, -0.2, 0.1]
    imu = _imu_rows(sc, rng, 50.0, state[1:10].reshape(3, 3))
    fa, fb = ctx.scan_frame(), ctx.scan_frame()
    try:
        for f in (fa, fb):
            n, _ = f.decode(layout, msg, 1, 0.0)
        st.set(state, sc["cov"])
        rows = st.propagate(imu, R.NOISE, 50.002, 50.003, 50.103)
        assert rows == 20
        na, dpa, dva = st.prepare(fa, EXT, DOWN_SIZE, sc["wl"].dept_err, sc["wl"].beam_err)
        poses, end = st.poses()
        assert len(poses) == rows and 0 < poses[-1, 0] < 0.1 and np.array_equal(end, st.get()[0][1:13])
        nb, dpb, dvb = fb.prepare(poses, end, EXT, DOWN_SIZE, sc["wl"].dept_err, sc["wl"].beam_err)
        assert na == nb and na > 2000
        a1, b1 = fa.read(1), fb.read(1)
        assert np.array_equal(a1["pnt"], b1["pnt"]) and (a1["pnt"] != fa.read(0)["pnt"]).any()       # stage 1, and it did move points
        a3, b3 = fa.read(3), fb.read(3)
        assert np.array_equal(a3["pnt"], b3["pnt"]) and np.array_equal(a3["var"], b3["var"])
        # without time stamps the table is left alone and the extrinsic still arrives
        na, _, _ = st.prepare(fa, EXT, DOWN_SIZE, sc["wl"].dept_err, sc["wl"].beam_err, point_notime=True)
        nb, _, _ = fb.prepare(None, None, EXT, DOWN_SIZE, sc["wl"].dept_err, sc["wl"].beam_err, point_notime=True)
        assert na == nb and np.array_equal(fa.read(3)["var"], fb.read(3)["var"]) and np.array_equal(st.poses()[0], poses)
    finally:
        fa.close(); fb.close()


def _by_key(rows):
    """a dump in the order of its leaf keys (kx, ky, kz, layer, path): the numbering of the leaves is not part of the map"""
    return rows[np.lexsort(rows[:, 4::-1].T)]


def _second_context(sc):
    ctx = sc["capi"].Context(sc["capi"].options_from_workload(sc["wl"]))
    wc, xs = build_map(sc, ctx)
    assert wc == sc["win_count"]
    ctx.window = xs
    return ctx


def test_insertion_on_state_is_the_host_fed_insertion(scene):
    sc = scene
    a, b = _second_context(sc), _second_context(sc)
    try:
        before = _by_key(a.dump_leaves())
        assert np.array_equal(before, _by_key(b.dump_leaves()))
        rng = np.random.default_rng(4)
        A = rng.normal(0, 1, (15, 15))
        cov = 1e-5 * (A @ A.T) / 15 + sc["cov"]
        st = a.odom_state()
        st.set(sc["state"], cov)
        x, cv = st.get()
        wc = sc["win_count"]
        st.pvec_update_cut_voxel(wc, *sc["dev"].args, multi=True)
        b.pvec_update_cut_voxel_dev(wc, *sc["dev"].args, np.concatenate([x[1:10], x[10:13]]), cv, multi=True)
        la, lb = _by_key(a.dump_leaves()), _by_key(b.dump_leaves())
        assert len(la) > 100 and np.array_equal(la, lb) and not np.array_equal(la, before)
        assert np.array_equal(_by_key(a.dump_plane_var()), _by_key(b.dump_plane_var()))
    finally:
        a.close(); b.close()


def test_chain_of_three_scans(scene):
    """propagate -> prepare -> update -> insert, three scans with no set between them, against the host-fed chain driven by the
    values read back at each step; no allocation after the reserves"""
    sc = scene
    wl = sc["wl"]
    a, b = _second_context(sc), _second_context(sc)
    try:
        st, fa, fb = a.odom_state(), a.scan_frame(), b.scan_frame()
        st.reserve(64); fa.reserve(len(sc["pts"]), 26)
        rng = np.random.default_rng(6)
        state = sc["state"].copy(); state[13:16] = 0.0; state[0] = 60.0
        st.set(state, sc["cov"])
        x, cv = st.get()
        wc, last_end, moved = sc["win_count"], 60.0, 0
        counters = (st.allocations(), fa.allocations())                        # after the reserves: they do not move again
        for scan in range(3):
            layout, msg = _message(sc, 10 + scan)
            for f in (fa, fb):
                f.decode(layout, msg, 1, 0.0)
            beg = last_end + 0.001
            imu = _imu_rows(sc, rng, beg - 0.004, x[1:10].reshape(3, 3))
            end_t = float(imu[-1, 0] + 0.002)
            rows = st.propagate(imu, R.NOISE, last_end, beg, end_t)
            na, dpa, dva = st.prepare(fa, EXT, DOWN_SIZE, wl.dept_err, wl.beam_err)
            xp, cp = st.get()                                               # the host-fed chain starts from the values read back
            poses, endp = st.poses()
            assert len(poses) == rows and xp[0] == end_t
            nb, dpb, dvb = fb.prepare(poses, endp, EXT, DOWN_SIZE, wl.dept_err, wl.beam_err)
            assert na == nb
            ok_a, xa, rep_a = st.lio_state_estimation(na, dpa, dva)
            ok_b, xb, cb, rep_b = b.lio_state_estimation_resident(nb, dpb, dvb, xp, cp)
            x, cv = st.get()
            assert ok_a == ok_b and np.array_equal(xa, xb) and np.array_equal(x, xb) and np.array_equal(cv, cb.reshape(15, 15))
            assert _same_report(rep_a, rep_b)
            moved += int((xb != xp).any())
            st.pvec_update_cut_voxel(wc, na, dpa, dva, multi=True)
            b.pvec_update_cut_voxel_dev(wc, nb, dpb, dvb, np.concatenate([xb[1:10], xb[10:13]]), cb, multi=True)
            for c in (a, b):                                               # the window moves on as in the local mapping
                xs = c.window + [np.concatenate([xb[1:10], xb[10:13]])]
                c.recut(wc + 1, np.array(xs), multi=True)
                c.margi(wc + 1, np.array(xs), jour=float(100 + scan))
                c.slide(1)
                c.window = xs[1:]
            last_end = end_t
            print("scan %d: %d rows, %d points, iterations %d, match_num %s, ok %s" % (scan, rows, na, rep_a["iterations"], rep_a["match_num"], ok_a))
        assert moved == 3
        assert (st.allocations(), fa.allocations()) == counters                # nothing allocated after the reserves
        assert np.array_equal(_by_key(a.dump_leaves()), _by_key(b.dump_leaves()))
        assert np.array_equal(_by_key(a.dump_plane_var()), _by_key(b.dump_plane_var()))
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_state_untouched(scene, corpus):
    sc = scene
    capi, ctx, st = sc["capi"], sc["ctx"], sc["st"]
    case = corpus["m21"][0]
    st.set(case["state"], case["cov"])
    before = st.get()
    rows_before = st.propagate(case["imu"], case["noise"], case["last_end"], case["beg"], case["end"], case["sg"])
    after_ok = st.get()
    st.set(case["state"], case["cov"])

    def refused(**over):
        c = dict(case); c.update(over)
        with pytest.raises(capi.VbaError) as e:
            st.propagate(c["imu"], c["noise"], c["last_end"], c["beg"], c["end"], c["sg"])
        assert e.value.status == capi.ERR_BAD_ARG, over.keys()
        now = st.get()
        assert np.array_equal(now[0], before[0]) and np.array_equal(now[1], before[1])

    refused(imu=case["imu"][:1])
    refused(last_end=case["imu"][-1, 0] + 1.0, beg=case["imu"][-1, 0] + 1.0)
    refused(beg=case["last_end"] - 0.011)
    bad = case["imu"].copy(); bad[7, 5] = np.inf
    refused(imu=bad)
    refused(end=np.nan)
    nz = case["noise"].copy(); nz[0] = np.nan
    refused(noise=nz)
    assert st.poses()[0].shape[0] == rows_before                            # the table of the last accepted call
    with pytest.raises(capi.VbaError) as e:
        bad_state = case["state"].copy(); bad_state[3] = np.nan
        st.set(bad_state, case["cov"])
    assert e.value.status == capi.ERR_BAD_ARG
    assert np.array_equal(st.get()[0], before[0]) and (after_ok[0] != before[0]).any()
    with pytest.raises(capi.VbaError) as e:
        st.lio_state_estimation(5, 0, 0)
    assert e.value.status == capi.ERR_BAD_ARG
    assert ctx.lib.vba_odom_lio_state_estimation_on_state(ctx.h, None, C.c_int(0), None, None, None, None, None) == capi.ERR_BAD_ARG
    sharded = capi.Context(capi.options_from_workload(sc["wl"]))
    try:
        sharded.set_shard(0, 2)
        for call in (lambda: st.lio_state_estimation(*sc["dev"].args, ctx=sharded),
                     lambda: st.pvec_update_cut_voxel(0, *sc["dev"].args, multi=True, ctx=sharded)):
            with pytest.raises(capi.VbaError) as e:
                call()
            assert e.value.status == capi.ERR_UNSUPPORTED
        assert np.array_equal(st.get()[0], before[0]) and np.array_equal(st.get()[1], before[1])
    finally:
        sharded.close()
