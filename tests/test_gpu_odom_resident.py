"""GPU tests of the device-resident scan-to-map EKF update (vba_odom_lio_state_estimation_resident) against the
CPU oracle of VOXEL_SLAM::lio_state_estimation (voxelslam.cpp:962-1098) and against the existing call on the same device pointers.
The existing call (vba_odom_lio_state_estimation) is a staging front end of the same loop: besides the bars, its ok, state and
covariance equal the resident call's bit for bit, from device pointers and from host arrays, and a sharded context accepts it.
The scene is that of test_gpu_odom.test_lio_state_estimation_parity and the bars are its bars (state 1e-7, covariance 1e-9 of its
largest entry); the step norms of the report are held to the oracle's trace at 1e-7.  match_num is printed, not compared: a point on
a float gate may fall either way."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE_BAR, COV_BAR, STEP_BAR = 1e-7, 1e-9, 1e-7


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


@pytest.fixture(scope="module")
def scene(oracle):
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")                   # torch's HIP runtime comes up first, as in bench.py: the library then shares it
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    from test_gpu_odom import _rand_var
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=4)
    W, nscan = wl.win_size, 8
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    ctx = capi.Context(capi.options_from_workload(wl))
    om = oracle.VoxelMap(W, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, 5)
    of = oracle.Factor(W)
    x_g, x_o, win_count = [], [], 0
    for k in range(nscan - 1):                       # local mapping on GT poses: builds + refreshes the planes
        pose = synth.poses_flat(s["R_gt"][k:k + 1], s["p_gt"][k:k + 1])[0]
        var = _rand_var(len(s["points"][k]), 100 + k)
        x_g.append(pose.copy()); x_o.append(pose.copy())
        win_count += 1
        ctx.cut_voxel(win_count - 1, s["points"][k], x_g[-1], var=var, multi=True)
        om.cut_voxel(win_count - 1, s["points"][k], x_o[-1], var=var, multi=True)
        ctx.recut(win_count, np.array(x_g), multi=True)
        om.recut(win_count, np.array(x_o), of, multi=True)
        if win_count >= W:
            ctx.margi(win_count, np.array(x_g), jour=float(k))
            om.margi(win_count, np.array(x_o), of)
            ctx.slide(1); om.slide(1)
            x_g = x_g[1:]; x_o = x_o[1:]
            win_count -= 1
    k = nscan - 1
    rng = np.random.default_rng(5)                    # the perturbed prediction of the existing test
    state = np.zeros(25)
    state[1:10] = (s["R_gt"][k] @ synth.so3_exp(rng.normal(0, np.radians(0.2), 3))).ravel()
    state[10:13] = s["p_gt"][k] + rng.normal(0, 0.02, 3)
    state[13:16] = [1.0, 0.5, 0.0]; state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4
    cov[9:, 9:] = np.eye(6) * 1e-5
    pts = s["points"][k]
    var_b = _rand_var(len(pts), 999, scale=0.005)
    sc = dict(capi=capi, synth=synth, wl=wl, ctx=ctx, om=om, pts=pts, var=var_b, state=state, cov=cov, dev=Dev(pts, var_b), gt=s["p_gt"][k])
    yield sc
    ctx.close()


def _parity(sc, pts, var, state, cov, dev=None):
    """New call vs oracle and vs the existing call on the same device pointers, at the bars, and bit for bit vs the existing call;
    returns the three results."""
    ctx, om = sc["ctx"], sc["om"]
    dev = dev or Dev(pts, var)
    ok_n, st_n, cov_n, rep = ctx.lio_state_estimation_resident(*dev.args, state, cov)
    ok_e, st_e, cov_e = ctx.lio_state_estimation_dev(*dev.args, state, cov)
    ok_o, st_o, cov_o, tr = om.lio_state_estimation(pts, var, state, cov)
    it = rep["iterations"]
    scale = np.abs(cov_o).max()
    print("n %d: iterations %d (oracle %d), match_num %s (oracle %s), ok %s/%s/%s" % (len(pts), it, len(tr), rep["match_num"][:it], tr[:, 0].astype(int), ok_n, ok_e, ok_o))
    print("  state: vs oracle %.3g, vs existing %.3g (bar %g); cov: %.3g, %.3g of max (bar %g)"
          % (np.abs(st_n - st_o).max(), np.abs(st_n - st_e).max(), STATE_BAR, np.abs(cov_n - cov_o).max() / scale, np.abs(cov_n - cov_e).max() / scale, COV_BAR))
    assert it == len(tr)
    print("  rot_add %s\n  tra_add %s\n  oracle  %s %s\n  nnt_eig_min %.6g" % (rep["rot_add"], rep["tra_add"], tr[:, 1], tr[:, 2], rep["nnt_eig_min"]))
    assert ok_n == ok_o and ok_n == ok_e
    assert np.abs(st_n - st_o).max() < STATE_BAR
    assert np.abs(st_n - st_e).max() < STATE_BAR
    assert np.abs(cov_n - cov_o).max() < COV_BAR * scale
    assert np.abs(cov_n - cov_e).max() < COV_BAR * scale
    assert np.abs(rep["rot_add"][:it] - tr[:, 1]).max() < STEP_BAR
    assert np.abs(rep["tra_add"][:it] - tr[:, 2]).max() < STEP_BAR
    assert np.all(rep["rot_add"][it:] == 0) and np.all(rep["tra_add"][it:] == 0) and np.all(rep["match_num"][it:] == 0)
    assert ok_n == (rep["nnt_eig_min"] >= 14)
    assert np.array_equal(st_e, st_n) and np.array_equal(cov_e, cov_n)   # the existing call runs the resident loop on a staged copy
    return (ok_n, st_n, cov_n, rep), (ok_e, st_e, cov_e), (ok_o, st_o, cov_o, tr)


def test_perturbed_prediction(scene):
    """Case 1: the state of the existing parity test; the loop runs past the first gate (at least three iterations)."""
    sc = scene
    new, _, (ok_o, st_o, cov_o, tr) = _parity(sc, sc["pts"], sc["var"], sc["state"], sc["cov"], sc["dev"])
    assert tr[0, 0] > 2000, "too few matches for a meaningful test: %s" % tr
    assert len(tr) >= 3
    assert new[0] and np.abs(new[1][10:13] - sc["gt"]).max() < np.abs(sc["state"][10:13] - sc["gt"]).max()


def _converged_start(sc):
    """A start at which the ORACLE converges at iterations 0 and 1: its own result chained as the next prediction (the covariance
    held at the first update's) until a pass takes two iterations, and once more for a margin to the thresholds of VS:1072."""
    om = sc["om"]
    _, st, cv, tr = om.lio_state_estimation(sc["pts"], sc["var"], sc["state"], sc["cov"])
    assert len(tr) >= 3
    twos = 0
    for _ in range(20):
        _, st_next, _, tr = om.lio_state_estimation(sc["pts"], sc["var"], st, cv)
        if len(tr) == 2:
            twos += 1
            if twos == 2:
                return st, cv
        st = st_next
    raise AssertionError("the oracle never converged in two iterations")


def test_converged_start_stops_at_the_first_gate(scene):
    """Case 2: from a converged state the oracle runs exactly two iterations: the launches of iterations 2 and 3 find the gate shut
    and must write nothing."""
    sc = scene
    st, cv = _converged_start(sc)
    _, _, _, tr = sc["om"].lio_state_estimation(sc["pts"], sc["var"], st, cv)
    assert len(tr) == 2 and tr[0, 0] > 2000, tr
    new, _, _ = _parity(sc, sc["pts"], sc["var"], st, cv, sc["dev"])
    assert new[3]["iterations"] == 2


@pytest.mark.parametrize("n", [255, 1001, 65537])
def test_sizes(scene, n):
    """Case 3: one partial; a ragged last workgroup; 257 partials, one more than the update kernel's workgroup has lanes."""
    sc = scene
    reps = (n + len(sc["pts"]) - 1) // len(sc["pts"])
    pts = np.concatenate([sc["pts"]] * reps)[:n]
    var = np.concatenate([sc["var"]] * reps)[:n]
    new, _, oracle_res = _parity(sc, pts, var, sc["state"], sc["cov"])
    if n < 2000:
        assert not new[0]                              # too few normals: the degenerate branch


def test_existing_call_on_host_arrays(scene):
    """The existing call on host arrays gives the resident call's bits."""
    sc = scene
    ok_n, st_n, cov_n, _ = sc["ctx"].lio_state_estimation_resident(*sc["dev"].args, sc["state"], sc["cov"])
    ok_h, st_h, cov_h = sc["ctx"].lio_state_estimation(sc["pts"], sc["var"], sc["state"], sc["cov"])
    assert (st_n != sc["state"]).any()
    assert ok_h == ok_n and np.array_equal(st_h, st_n) and np.array_equal(cov_h, cov_n)


def _assert_untouched(res, state, cov):
    ok, st, cv, rep = res
    assert np.array_equal(st, state) and np.array_equal(cv, cov)
    assert rep["iterations"] == 2
    assert not ok
    assert np.all(rep["match_num"] == 0) and np.all(rep["rot_add"] == 0) and np.all(rep["tra_add"] == 0)
    assert rep["nnt_eig_min"] == 0.0


def _assert_existing_untouched(res, state, cov):
    ok, st, cv = res
    assert np.array_equal(st, state) and np.array_equal(cv, cov)
    assert ok == 0


def test_no_point_matches(scene):
    """Case 4: the scan a kilometre away."""
    sc = scene
    dev = Dev(sc["pts"] + np.array([1000.0, 0.0, 0.0]), sc["var"])
    _assert_untouched(sc["ctx"].lio_state_estimation_resident(*dev.args, sc["state"], sc["cov"]), sc["state"], sc["cov"])


def test_empty_scan_and_empty_map(scene):
    """Case 5: n == 0, and a context whose map was never allocated; the existing call too returns its input and ok == 0."""
    sc = scene
    _assert_untouched(sc["ctx"].lio_state_estimation_resident(0, 0, 0, sc["state"], sc["cov"]), sc["state"], sc["cov"])
    fresh = sc["capi"].Context(sc["capi"].options_from_workload(sc["wl"]))
    try:
        _assert_untouched(fresh.lio_state_estimation_resident(*sc["dev"].args, sc["state"], sc["cov"]), sc["state"], sc["cov"])
        _assert_untouched(fresh.lio_state_estimation_resident(0, 0, 0, sc["state"], sc["cov"]), sc["state"], sc["cov"])
        _assert_existing_untouched(fresh.lio_state_estimation(sc["pts"], sc["var"], sc["state"], sc["cov"]), sc["state"], sc["cov"])
        _assert_existing_untouched(fresh.lio_state_estimation_dev(*sc["dev"].args, sc["state"], sc["cov"]), sc["state"], sc["cov"])
    finally:
        fresh.close()
    empty = np.zeros((0, 3)), np.zeros((0, 9))
    _assert_existing_untouched(sc["ctx"].lio_state_estimation(*empty, sc["state"], sc["cov"]), sc["state"], sc["cov"])
    _assert_existing_untouched(sc["ctx"].lio_state_estimation_dev(0, 0, 0, sc["state"], sc["cov"]), sc["state"], sc["cov"])


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_repeatable_and_reads_only(scene):
    """Case 6: two calls give the same bits; the existing call on the same context gives what it gave before them."""
    sc = scene
    ctx, dev = sc["ctx"], sc["dev"]
    before = ctx.lio_state_estimation_dev(*dev.args, sc["state"], sc["cov"])
    a = ctx.lio_state_estimation_resident(*dev.args, sc["state"], sc["cov"])
    b = ctx.lio_state_estimation_resident(*dev.args, sc["state"], sc["cov"])
    after = ctx.lio_state_estimation_dev(*dev.args, sc["state"], sc["cov"])
    assert a[0] == b[0] and _same(a[1:3], b[1:3])
    assert all(np.array_equal(np.asarray(a[3][k]), np.asarray(b[3][k])) for k in a[3])
    assert before[0] == after[0] and _same(before[1:], after[1:])
    assert np.array_equal(dev.p.cpu().numpy(), sc["pts"]) and np.array_equal(dev.v.cpu().numpy(), sc["var"])   # consumed in place, not written


def test_errors(scene):
    """Case 7: a sharded context is refused by the resident call (the existing call runs on the local map); null arrays with n > 0,
    null state, n < 0 are bad arguments."""
    sc = scene
    capi = sc["capi"]
    ctx = sc["ctx"]
    with pytest.raises(capi.VbaError) as e:
        ctx.lio_state_estimation_resident(5, 0, 0, sc["state"], sc["cov"])
    assert e.value.status == capi.ERR_BAD_ARG
    with pytest.raises(capi.VbaError) as e:
        ctx.lio_state_estimation_resident(5, sc["dev"].p.data_ptr(), 0, sc["state"], sc["cov"])
    assert e.value.status == capi.ERR_BAD_ARG
    with pytest.raises(capi.VbaError) as e:
        ctx.lio_state_estimation_resident(-1, sc["dev"].p.data_ptr(), sc["dev"].v.data_ptr(), sc["state"], sc["cov"])
    assert e.value.status == capi.ERR_BAD_ARG
    import ctypes as C
    n, dp, dv = sc["dev"].args
    assert ctx.lib.vba_odom_lio_state_estimation_resident(ctx.h, C.c_int(n), C.c_void_p(dp), C.c_void_p(dv), None, None, None, None) == capi.ERR_BAD_ARG
    sharded = capi.Context(capi.options_from_workload(sc["wl"]))
    try:
        sharded.set_shard(0, 2)
        with pytest.raises(capi.VbaError) as e:
            sharded.lio_state_estimation_resident(*sc["dev"].args, sc["state"], sc["cov"])
        assert e.value.status == capi.ERR_UNSUPPORTED
        n, dp, dv = sc["dev"].args
        st, cv, ok = sc["state"].copy(), sc["cov"].copy(), C.c_int(-1)
        assert sharded.lib.vba_odom_lio_state_estimation(sharded.h, C.c_int(n), C.c_void_p(dp), C.c_void_p(dv), capi._p(st), capi._p(cv), C.byref(ok)) == capi.OK
    finally:
        sharded.close()


def test_scan_frame_pointers(scene):
    """Case 8: the device arrays of ScanFrame.prepare, consumed in place: the existing call on the same addresses agrees."""
    import decode_oracle as do
    sc = scene
    capi, ctx = sc["capi"], sc["ctx"]
    layout = capi.scan_layout("tartanair")
    frame = ctx.scan_frame()
    try:
        pts = sc["pts"].astype(np.float32)
        n, _ = frame.decode(layout, do.make_message(layout, pts), 1, 0.0)
        assert n == len(pts)
        ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
        m, dp, dv = frame.prepare(None, None, ext, 0.05, 0.02, 0.05, point_notime=True)
        assert m > 2000
        s3 = frame.read(3)
        ok_n, st_n, cov_n, rep = ctx.lio_state_estimation_resident(m, dp, dv, sc["state"], sc["cov"])
        ok_e, st_e, cov_e = ctx.lio_state_estimation_dev(m, dp, dv, sc["state"], sc["cov"])
        print("prepared %d points: iterations %d, match_num %s, state %.3g, cov %.3g of max" % (m, rep["iterations"], rep["match_num"],
              np.abs(st_n - st_e).max(), np.abs(cov_n - cov_e).max() / np.abs(cov_e).max()))
        assert ok_n == ok_e
        assert (st_n != sc["state"]).any()
        assert np.abs(st_n - st_e).max() < STATE_BAR
        assert np.abs(cov_n - cov_e).max() < COV_BAR * np.abs(cov_e).max()
        after = frame.read(3)
        assert np.array_equal(after["pnt"], s3["pnt"]) and np.array_equal(after["var"], s3["var"])
    finally:
        frame.close()
