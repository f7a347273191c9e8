"""GPU tests of the device-resident kd-tree odometry (vba_odom_lio_state_estimation_kdtree_resident) against the
CPU oracle of VOXEL_SLAM::lio_state_estimation_kdtree (voxelslam.cpp:1102-1252) and against the existing call on the same device
pointer in a second context.  The scene, the predictions (rng seed 17) and the bars are those of
test_gpu_odom.test_lio_state_estimation_kdtree_parity: state 1e-5, covariance 1e-4 of its largest entry, map size within
max(2, len / 500) and 1e-4 on the points when the sizes agree.  match_num is printed, not compared: a point on the 0.1 gate may fall
either way.  The existing call is a staging front end of the same loop: in deterministic contexts it returns the resident call's bits
(without the mode the re-sampler's atomic insert promises no bits for the map, and the bars are the only assertion)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE_BAR, COV_BAR, TREE_BAR = 1e-5, 1e-4, 1e-4


class Dev:
    """A scan's points as a torch tensor on the context's device."""

    def __init__(self, pts):
        import torch
        self.host = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        self.n = len(self.host)
        self.p = torch.from_numpy(self.host).to("cuda:0")
        torch.cuda.synchronize()

    @property
    def args(self):
        return self.n, (self.p.data_ptr() if self.n else 0)

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.p.cpu().numpy(), self.host)


def _existing(ctx, n, ptr, state, cov):
    """vba_odom_lio_state_estimation_kdtree on a device pointer."""
    from voxel_slam_amd import capi
    st = np.ascontiguousarray(state, dtype=np.float64).copy(); cv = np.ascontiguousarray(cov, dtype=np.float64).copy(); it = C.c_int(0)
    ctx._chk(ctx.lib.vba_odom_lio_state_estimation_kdtree(ctx.h, C.c_int(n), C.c_void_p(ptr), capi._p(st), capi._p(cv), C.byref(it)))
    return it.value, st, cv


def _cov0():
    cov = np.eye(15) * 1e-4
    cov[9:, 9:] = np.eye(6) * 1e-5
    return cov


@pytest.fixture(scope="module")
def env(oracle):
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")                   # torch's HIP runtime comes up first, as in bench.py: the library then shares it
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=5)
    s = synth.make_scans(wl)
    rng = np.random.default_rng(17)
    pts, states = [], []
    for k in range(wl.win_size):
        pts.append(s["points"][k].astype(np.float32).astype(np.float64))      # PCL scan points are float
        state = np.zeros(25)
        dR = np.eye(3) if k == 0 else synth.so3_exp(rng.normal(0, np.radians(0.3), 3))
        state[1:10] = (s["R_gt"][k] @ dR).ravel()
        state[10:13] = s["p_gt"][k] + (0 if k == 0 else rng.normal(0, 0.03, 3))
        state[13:16] = [0.3, 0.1, 0.0]; state[22:25] = [0, 0, -9.8]
        states.append(state)
    e = dict(capi=capi, synth=synth, wl=wl, oracle=oracle, pts=pts, states=states, gt=s["p_gt"], ctxs=[], keep=[], cache={})
    yield e
    for c in e["ctxs"]:
        c.close()


def _ctx(env, deterministic=0):
    opt = env["capi"].options_from_workload(env["wl"])
    opt.deterministic = deterministic
    c = env["capi"].Context(opt)
    env["ctxs"].append(c)
    return c


def _dev(env, pts):
    d = Dev(pts)
    env["keep"].append(d)                             # a seeding call is stream-ordered: its tensor outlives the test
    return d


def _oracle_sequence(env, name, scans, empty=False):
    """The oracle over a sequence of (points, state) with the covariance chained, computed once per module: per call (iterations,
    state, cov, map size before the call, map after it).  With empty, an empty scan follows every estimation, from the state and
    covariance that the estimation returned."""
    if name not in env["cache"]:
        ko = env["oracle"].KdOdom()
        cov = _cov0(); out = []
        for p, state in scans:
            before = len(ko.tree())
            it, st, cv = ko.lio_state_estimation(p, state, cov)
            if it:
                cov = cv
            out.append((it, st, cv, before, ko.tree()))
            if empty and it:
                before = len(ko.tree())
                it0, st0, cv0 = ko.lio_state_estimation(np.zeros((0, 3)), st, cov)
                assert np.array_equal(st0, st) and np.array_equal(cv0, cov)
                out.append((it0, st0, cv0, before, ko.tree()))
        env["cache"][name] = out
    return env["cache"][name]


def _check_tree(tag, t, ref):
    assert abs(len(t) - len(ref)) <= max(2, len(ref) // 500), (tag, len(t), len(ref))   # a point within 1e-5 of a 0.5 m face may change cell
    if len(t) == len(ref):
        d = np.abs(t - ref).max()
        assert d < TREE_BAR, (tag, d)
        return d
    return float("nan")


def _step(tag, cn, ce, dev, state, cov_n, cov_e, orc=None):
    """One call of the new entry point on cn and of the existing one on ce, on the same device pointer; both against the oracle's
    result orc = (iterations, state, cov, -, map) when given, and against each other, at the bars.  Returns both results."""
    it_n, st_n, cv_n, rep = cn.lio_state_estimation_kdtree_resident(*dev.args, state, cov_n)
    it_e, st_e, cv_e = _existing(ce, *dev.args, state, cov_e)
    tn, te = cn.kdtree_points(), ce.kdtree_points()
    scale = np.abs(cv_e).max()
    print("%s: n %d, iterations %d (existing %d%s), valid %s, map %d (existing %d)" % (tag, dev.n, it_n, it_e, ", oracle %d" % orc[0] if orc else "",
                                                                                      rep["match_num"][:it_n], len(tn), len(te)))
    print("  new vs existing: state %.3g, cov %.3g of max" % (np.abs(st_n - st_e).max(), np.abs(cv_n - cv_e).max() / scale))
    assert it_n == it_e == rep["iterations"]
    assert np.abs(st_n - st_e).max() < STATE_BAR
    assert np.abs(cv_n - cv_e).max() < COV_BAR * scale
    d = _check_tree(tag + " map vs existing", tn, te)
    print("  map vs existing: %.3g" % d)
    assert rep["nnt_eig_min"] == 0.0
    assert np.all(rep["rot_add"][it_n:] == 0) and np.all(rep["tra_add"][it_n:] == 0) and np.all(rep["match_num"][it_n:] == 0)
    if orc is not None:
        it_o, st_o, cv_o, _, to = orc
        so = np.abs(cv_o).max()
        print("  new vs oracle: state %.3g, cov %.3g of max" % (np.abs(st_n - st_o).max(), np.abs(cv_n - cv_o).max() / so))
        assert it_n == it_o
        if it_o:
            assert np.abs(st_n - st_o).max() < STATE_BAR
            assert np.abs(cv_n - cv_o).max() < COV_BAR * so
        _check_tree(tag + " map vs oracle", tn, to)
    return (it_n, st_n, cv_n, rep, tn), (it_e, st_e, cv_e, te)


def _sequence(env, tag, cn, ce, scans, orc, empty=False):
    """The scans in turn with each runner's covariance chained; with empty, an empty scan after every estimation."""
    cov_n, cov_e = _cov0(), _cov0()
    out = []
    for k, (p, state) in enumerate(scans):
        dev = _dev(env, p)
        new, old = _step("%s scan %d" % (tag, k), cn, ce, dev, state, cov_n, cov_e, orc[len(out)] if orc else None)
        if new[0] == 0:
            np.testing.assert_array_equal(new[1], state); np.testing.assert_array_equal(new[2], cov_n)
        else:
            cov_n, cov_e = new[2], old[2]
        out.append(new)
        if empty and new[0]:
            it, st, cv, rep = cn.lio_state_estimation_kdtree_resident(0, 0, new[1], cov_n)
            it_e, _, _ = _existing(ce, 0, 0, new[1], cov_e)
            assert it == it_e == 2 and rep["iterations"] == 2 and np.all(rep["match_num"] == 0)
            np.testing.assert_array_equal(st, new[1]); np.testing.assert_array_equal(cv, cov_n)
            assert cn.kdtree_size() == ce.kdtree_size()
            tn = cn.kdtree_points()
            if orc:
                assert orc[len(out)][0] == 2                       # the oracle on zero sums: two iterations
                _check_tree("%s empty scan after %d" % (tag, k), tn, orc[len(out)][4])
            out.append((it, st, cv, rep, tn))
    return out


def _full(env):
    return list(zip(env["pts"], env["states"]))


def _every20(env):
    return [(p[::20], s) for p, s in zip(env["pts"], env["states"])]


def test_parity_sequence(env):
    """Case 1: the sequence of the existing parity test: a seed, three full loops and a stop after three iterations, whose four last
    launches find the flag; maps of 20 000 (unsampled) and ~950-990 points, no multiple of 256."""
    orc = _oracle_sequence(env, "full", _full(env))
    print("oracle: iterations %s, map sizes before the calls %s" % ([o[0] for o in orc], [o[3] for o in orc]))
    assert [o[0] for o in orc] == [0, 4, 4, 3, 4]
    sizes = [o[3] for o in orc]
    assert sizes[:2] == [0, 20000] and all(900 < m < 1100 and m % 256 for m in sizes[2:])     # what the docstring says of the maps
    out = _sequence(env, "full", _ctx(env), _ctx(env), _full(env), orc)
    for k in range(1, 5):
        assert np.linalg.norm(out[k][1][10:13] - env["gt"][k]) < np.linalg.norm(env["states"][k][10:13] - env["gt"][k])


def test_every_20th_point_and_empty_scans(env):
    """Case 2: n = 1000 (four workgroups, eight map slices of which four or more are empty on maps of 770-870 points), and an empty
    scan after every estimation: two iterations, state and covariance untouched, the map re-sampled as the existing call does."""
    orc = _oracle_sequence(env, "every20", _every20(env), empty=True)
    print("oracle: iterations %s, map sizes before the calls %s" % ([o[0] for o in orc], [o[3] for o in orc]))
    assert [o[0] for o in orc] == [0, 4, 2, 4, 2, 4, 2, 4, 2]
    _sequence(env, "every20", _ctx(env), _ctx(env), _every20(env), orc, empty=True)


def _dense(env, n):
    """n points in the frame of scan 1: its points repeated with 5 mm of jitter (float values)."""
    rng = np.random.default_rng(n)
    p = env["pts"][1]
    q = p[np.arange(n) % len(p)] + (rng.normal(0, 0.005, (n, 3)) if n > len(p) else 0.0)
    return q.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("n,with_oracle", [(255, True), (257, True), (32769, True), (130817, False)])
def test_partial_workgroups_and_slice_counts(env, n, with_oracle):
    """Case 3: one point short of and one past a workgroup (8 slices), the first size with 4 slices and the first with 1, against the
    unsampled 20 000-point map that the seed of case 1 leaves."""
    scans = [(env["pts"][0], env["states"][0]), (_dense(env, n), env["states"][1])]
    orc = _oracle_sequence(env, "dense%d" % n, scans) if with_oracle else None
    out = _sequence(env, "n=%d" % n, _ctx(env), _ctx(env), scans, orc)
    assert out[1][0] >= 2


def test_map_of_exactly_100_points(env):
    """Case 3, last item: the first map size at which the estimation runs."""
    scans = [(env["pts"][0][:100], env["states"][0]), (env["pts"][1][:300], env["states"][1])]
    orc = _oracle_sequence(env, "map100", scans)
    assert orc[1][3] == 100 and orc[1][0] >= 2
    _sequence(env, "map100", _ctx(env), _ctx(env), scans, orc)


def test_seeding(env):
    """Case 4: below 100 points the scan only seeds the map, in a stream-ordered call."""
    ctx = _ctx(env)
    state = np.zeros(25); state[1:10] = np.eye(3).ravel(); state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4
    pts = np.random.default_rng(0).uniform(-5, 5, (60, 3)).astype(np.float32).astype(np.float64)
    dev = _dev(env, pts)
    for size in (60, 120):
        it, st, cv, rep = ctx.lio_state_estimation_kdtree_resident(*dev.args, state, cov)
        assert it == 0 and rep["iterations"] == 0 and ctx.kdtree_size() == size
        np.testing.assert_array_equal(st, state); np.testing.assert_array_equal(cv, cov)
    np.testing.assert_array_equal(ctx.kdtree_points(), np.concatenate([pts, pts]))    # identity pose: the float points themselves
    ctx._chk(ctx.lib.vba_odom_kdtree_reset(ctx.h))
    assert ctx.kdtree_size() == 0
    it, _, _, _ = ctx.lio_state_estimation_kdtree_resident(0, 0, state, cov)           # an empty scan on an empty map
    assert it == 0 and ctx.kdtree_size() == 0


def test_repeatable_and_read_only(env):
    """Case 5: two deterministic contexts over the sequence of case 2 return the same bits; the scan tensors are not written."""
    runs = []
    first = len(env["keep"])
    for _ in range(2):
        cn = _ctx(env, deterministic=1)
        runs.append(_sequence(env, "det", cn, _ctx(env, deterministic=1), _every20(env), None, empty=True))
    assert len(runs[0]) == len(runs[1]) == 9
    for a, b in zip(*runs):
        assert a[0] == b[0]
        np.testing.assert_array_equal(a[1], b[1]); np.testing.assert_array_equal(a[2], b[2]); np.testing.assert_array_equal(a[4], b[4])
        for key in ("match_num", "rot_add", "tra_add"):
            np.testing.assert_array_equal(a[3][key], b[3][key])
    assert all(d.unchanged() for d in env["keep"][first:])


def _assert_same_bits(tag, a, b, ca, cb):
    """(iterations, state, cov) of two calls and the maps of their contexts, bit for bit."""
    assert a[0] == b[0], tag
    np.testing.assert_array_equal(a[1], b[1], err_msg=tag); np.testing.assert_array_equal(a[2], b[2], err_msg=tag)
    assert ca.kdtree_size() == cb.kdtree_size(), tag
    np.testing.assert_array_equal(ca.kdtree_points(), cb.kdtree_points(), err_msg=tag)


def test_existing_call_on_host_arrays_gives_the_same_bits(env):
    """The existing call is a staging front end of the resident loop: over the sequence of case 2 (a seed, then an empty scan after
    every estimation) in two deterministic contexts, the existing call on host arrays and the resident call on device pointers return
    the same iterations, state, covariance, map size and map points after every call."""
    ch, cd = _ctx(env, deterministic=1), _ctx(env, deterministic=1)
    cov_h, cov_d = _cov0(), _cov0()
    iters = []
    for k, (p, state) in enumerate(_every20(env)):
        dev = _dev(env, p)
        h = ch.lio_state_estimation_kdtree(p, state, cov_h)
        d = cd.lio_state_estimation_kdtree_resident(*dev.args, state, cov_d)[:3]
        _assert_same_bits("scan %d" % k, h, d, ch, cd)
        iters.append(h[0])
        if h[0]:
            cov_h, cov_d = h[2], d[2]
            h0 = ch.lio_state_estimation_kdtree(np.zeros((0, 3)), h[1], cov_h)
            d0 = cd.lio_state_estimation_kdtree_resident(0, 0, d[1], cov_d)[:3]
            _assert_same_bits("empty scan after %d" % k, h0, d0, ch, cd)
            iters.append(h0[0])
    assert iters[0] == 0 and len(iters) == 9 and all(i >= 2 for i in iters[1:])     # the first scan seeded, every other call estimated


def test_existing_call_keeps_its_stage_in_stream_order(env):
    """The existing call stages the scan in the context's staging buffer.  Other calls that stage there (a down-sampling, whose voxel
    table lands on the staged points, and a cut_voxel) between two existing calls change nothing: every result equals that of a
    context that made the kd calls alone."""
    ca, cb = _ctx(env, deterministic=1), _ctx(env, deterministic=1)
    scans = _every20(env)[:3]
    small = env["pts"][3][::100]
    pose = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    cov_a, cov_b = _cov0(), _cov0()
    for k, (p, state) in enumerate(scans):
        a = ca.lio_state_estimation_kdtree(p, state, cov_a)
        b = cb.lio_state_estimation_kdtree(p, state, cov_b)
        _assert_same_bits("scan %d" % k, a, b, ca, cb)
        assert a[0] == 0 if k == 0 else a[0] >= 2
        if a[0]:
            cov_a, cov_b = a[2], b[2]
        out, _, _ = ca.down_sampling_voxel(small, 0.5)
        assert 0 < len(out) <= len(small)
        ca.cut_voxel(0, small, pose)


def test_reservation(env):
    """Case 6: after the reservation the sequence of case 2 allocates nothing; a scan past it does, and is still right."""
    cn, ce = _ctx(env), _ctx(env)
    assert cn.kdtree_allocations() == (0, 0)
    cn.kdtree_reserve(4096, 1024)
    a0 = cn.kdtree_allocations()
    assert a0[0] > 0 and a0[1] > 0
    out = _sequence(env, "reserved", cn, ce, _every20(env), _oracle_sequence(env, "every20", _every20(env), empty=True), empty=True)
    assert cn.kdtree_allocations() == a0
    big = _dev(env, _dense(env, 32769))
    new, old = _step("past the reservation", cn, ce, big, env["states"][1], out[-1][2], out[-1][2])
    a1 = cn.kdtree_allocations()
    print("allocations %s -> %s" % (a0, a1))
    assert a1[0] > a0[0] and a1[1] > a0[1]
    assert new[0] >= 2


def test_errors(env):
    """Case 7."""
    capi = env["capi"]
    ctx = _ctx(env)
    state = env["states"][0].copy(); cov = _cov0()
    dev = _dev(env, env["pts"][0][:64])
    f = ctx.lib.vba_odom_lio_state_estimation_kdtree_resident
    it = C.c_int(0)
    assert f(ctx.h, C.c_int(64), C.c_void_p(dev.args[1]), None, capi._p(cov), C.byref(it), None) == capi.ERR_BAD_ARG
    assert f(ctx.h, C.c_int(64), C.c_void_p(dev.args[1]), capi._p(state), None, C.byref(it), None) == capi.ERR_BAD_ARG
    assert f(ctx.h, C.c_int(-1), C.c_void_p(dev.args[1]), capi._p(state), capi._p(cov), C.byref(it), None) == capi.ERR_BAD_ARG
    assert f(ctx.h, C.c_int(64), None, capi._p(state), capi._p(cov), C.byref(it), None) == capi.ERR_BAD_ARG
    assert ctx.kdtree_size() == 0
    assert f(ctx.h, C.c_int(64), C.c_void_p(dev.args[1]), capi._p(state), capi._p(cov), None, None) == capi.OK      # iterations may be NULL
    assert ctx.kdtree_size() == 64
    g = ctx.lib.vba_odom_lio_state_estimation_kdtree
    big = C.c_int((1 << 28) - 63)                     # map + scan past 2^28 points: refused by both calls before anything is read
    assert f(ctx.h, big, C.c_void_p(dev.args[1]), capi._p(state), capi._p(cov), C.byref(it), None) == capi.ERR_CAPACITY
    assert g(ctx.h, big, C.c_void_p(dev.args[1]), capi._p(state), capi._p(cov), C.byref(it)) == capi.ERR_CAPACITY
    assert ctx.kdtree_size() == 64
    assert ctx.lib.vba_odom_kdtree_reserve(ctx.h, C.c_int(-1), C.c_int(0)) == capi.ERR_BAD_ARG
    assert ctx.lib.vba_odom_kdtree_allocations(ctx.h, None, None) == capi.ERR_BAD_ARG


def test_frame_path(env):
    """Case 8: a prepared scan frame feeds the new call in place; the existing call takes the frame's stage-3 points from the host."""
    import decode_oracle as do
    capi = env["capi"]
    cn, ce = _ctx(env), _ctx(env)
    frame = cn.scan_frame()
    layout = capi.scan_layout("tartanair")
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    cov_n, cov_e = _cov0(), _cov0()
    ran = 0
    for k in range(3):
        n, _ = frame.decode(layout, do.make_message(layout, env["pts"][k]), 1, 1e-4)
        m, dp, dv = frame.prepare(None, ext, ext, 0.5, 0.02, 0.05, min_points=0, point_notime=True)
        host = frame.read(3)["pnt"]
        assert 100 < m == len(host) < n
        state = env["states"][k]
        it_n, st_n, cv_n, rep = cn.lio_state_estimation_kdtree_resident(m, dp, state, cov_n)
        it_e, st_e, cv_e = ce.lio_state_estimation_kdtree(host, state, cov_e)
        scale = np.abs(cv_e).max()
        print("frame scan %d: %d -> %d points, iterations %d (existing %d), valid %s; state %.3g, cov %.3g of max"
              % (k, n, m, it_n, it_e, rep["match_num"][:it_n], np.abs(st_n - st_e).max(), np.abs(cv_n - cv_e).max() / scale))
        assert it_n == it_e
        assert np.abs(st_n - st_e).max() < STATE_BAR
        assert np.abs(cv_n - cv_e).max() < COV_BAR * scale
        _check_tree("frame scan %d" % k, cn.kdtree_points(), ce.kdtree_points())
        if it_n:
            cov_n, cov_e = cv_n, cv_e
            ran += 1
    assert ran == 2
    frame.close()
