"""The LM linear solves on the device (k_lm_solve_m, k_li_solve, big_solve), driven through vba_debug_solve with systems of the test's
choosing and held to the bars of tests/solve_ref.py: backward error, forward error against an exact-residual reference, q1 against
its exact value at the returned dx, exact zeros on gauge and zero rows, the pivot-order probe.  Beside the bars: the masked LI
factorisation equals the dense one by value, every speculative candidate equals a one-candidate solve at its damping, and both
tile packings and both load orders of the lidar kernel give the same bits."""
import dataclasses
import os

import numpy as np
import pytest

import solve_ref as R

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    assert os.path.exists(m.LIB_PATH), "libvoxelba.so must be prebuilt in-tree (no fallback)"
    return m


def _ctx(capi, lm_spec):
    o = capi.default_options()
    o.win_size = 4
    o.lm_spec = lm_spec
    return capi.Context(o)


@pytest.fixture(scope="module")
def ctx4(capi):
    c = _ctx(capi, 4)
    yield c
    c.close()
    for k in sorted(WORST):
        print("worst ratio %-6s %-22s backward %.3g forward %.3g q1 %.3g" % (k + tuple(WORST[k][q] for q in ("bw", "fw", "q1"))))


@pytest.fixture(scope="module")
def ctx1(capi):
    c = _ctx(capi, 1)
    yield c
    c.close()


def _cls(label):
    return "probe" if label.startswith("probe") else label.split(" u=")[0]


def _check(kind, case, dx, q1, v):
    """bars for every candidate b (damping u_b of b consecutive rejections) and exact zeros on the gauge rows"""
    for b in range(len(q1)):
        ub = R.damping_of(case.u, v, b)
        r = R.check(case, dx[b], q1[b], u=ub)
        assert np.all(dx[b][:case.gauge] == 0.0), (kind, case.label, b)
        assert r["zeros"], (kind, case.label, b)
        assert r["bw"] <= 1 and r["fw"] <= 1 and r["q1"] <= 1, (kind, case.label, b, r)
        k = (kind, _cls(case.label))
        WORST[k] = {q: max(WORST.get(k, {}).get(q, 0.0), r[q]) for q in ("bw", "fw", "q1")}


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("W", list(range(2, 17)))
def test_lidar_solve(ctx4, ctx1, W):
    full = W in (2, 4, 10, 16)
    cases = R.lidar_cases(W, dampings=R.DAMPINGS if full else (1e-2,), kappas=R.KAPPAS if full else (1.0, 1e8))
    v = 2.0
    for i, case in enumerate(cases):
        out = ctx4.debug_solve("lidar", W, case.H, case.g, case.u, v)
        _check("lidar", case, out[0], out[1], v)
        if i % 3 == 0 or case.probe is not None:
            for fl in (dict(e_packed=True), dict(copy_raw=True), dict(copy_raw=True, from_raw=True), dict(e_packed=True, copy_raw=True)):
                assert _same(ctx4.debug_solve("lidar", W, case.H, case.g, case.u, v, **fl), out), (case.label, fl)
            for b in range(1, len(out[1])):
                one = ctx1.debug_solve("lidar", W, case.H, case.g, R.damping_of(case.u, v, b), v)
                assert np.array_equal(one[0][0], out[0][b]) and one[1][0] == out[1][b], (case.label, b)


@pytest.mark.parametrize("grav", [0, 1])
@pytest.mark.parametrize("W", list(range(2, 17)))
def test_li_solve(ctx4, ctx1, W, grav):
    full = W in (2, 5, 10, 11, 16)
    cases = R.li_cases(W, grav, dampings=(0.0, 1e-2, 1e3) if full else (1e-2,), kappas=R.KAPPAS if full else (1.0, 1e8))
    v = 2.0
    for i, case in enumerate(cases):
        out = ctx4.debug_solve("li", W, case.H, case.g, case.u, v, gravity=bool(grav))
        _check("li", case, out[0], out[1], v)
        dense = ctx4.debug_solve("li", W, case.H, case.g, case.u, v, gravity=bool(grav), dense_mask=True)
        assert _same(dense, out), (W, grav, case.label)             # (array_equal: the sign of a zero may differ)
        if i == 0:
            assert _same(ctx4.debug_solve("li", W, case.H, case.g, case.u, v, gravity=bool(grav), copy_raw=True), out)
            for b in range(1, len(out[1])):
                one = ctx1.debug_solve("li", W, case.H, case.g, R.damping_of(case.u, v, b), v, gravity=bool(grav))
                assert np.array_equal(one[0][0], out[0][b]) and one[1][0] == out[1][b], (case.label, b)


@pytest.mark.parametrize("W", [17, 21, 32, 43])
def test_dense_solve(ctx4, W):
    """n = 6W with n + 1 just below (W = 21: 127) and just above (W = 32: 193, W = 43: 259) a multiple of 64"""
    for case in R.lidar_cases(W, dampings=(0.0, 1e-2), kappas=(1.0, 1e4, 1e12)):
        dx, q1 = ctx4.debug_solve("dense", W, case.H, case.g, case.u)
        _check("dense", case, dx, q1, 2.0)


def test_realistic_systems(capi, ctx4):
    """the device's own Hessians (room20k at W = 4, 10, 16; the LI Hessian with and without gravity) with a chosen solution"""
    from voxel_slam_amd import synth
    rng = np.random.default_rng(77)
    for W in (4, 10, 16):
        wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="room_w%d" % W, win_size=W)
        s = synth.make_scans(wl)
        fac = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
        poses = synth.poses_flat(s["R0"], s["p0"])
        o = capi.default_options(); o.win_size = W; o.imu_coef = wl.imu_coef
        ctx = capi.Context(o); ctx.push_dict(fac)
        H, _, _ = ctx.acc_evaluate2(poses)
        H = 0.5 * (H + H.T)
        for u in (1e-2, 1e-6):
            x = R.xstar_like(rng, 6 * W) * 1e-2
            case = R.Case("realistic W=%d" % W, H, R.rhs_for(H, x, u, 6), u, 6)
            dx, q1 = ctx4.debug_solve("lidar", W, case.H, case.g, case.u, 2.0)
            _check("lidar", case, dx, q1, 2.0)
            dx, q1 = ctx4.debug_solve("dense", W, case.H, case.g, case.u)
            _check("dense", case, dx, q1, 2.0)
        if W == 4:
            imu_samples, vel, g = synth.make_imu(wl, gyr_sigma=1e-3, acc_sigma=1e-2)
            nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
            imus = np.stack([capi.imu_preintegrate(t, gy, ac, np.zeros(3), np.zeros(3), nm, nw) for (t, gy, ac) in imu_samples])
            states = np.zeros((W, 25))
            for i in range(W):
                states[i, 0] = 0.1 * i
                states[i, 1:10] = s["R0"][i].ravel(); states[i, 10:13] = s["p0"][i]; states[i, 13:16] = vel[i]; states[i, 22:25] = g
            for grav in (0, 1):
                ctx.evaluate_only_residual(poses)
                Hl = ctx.li_ba_damping_iter(states, imus, gravity=bool(grav), max_iter=1)["hess"]
                Hl = 0.5 * (Hl + Hl.T)
                Hl[~R.li_pattern(W, grav)] = 0.0
                n = 15 * W + 3 * grav
                case = R.Case("realistic-li W=%d g=%d" % (W, grav), Hl, R.rhs_for(Hl, R.xstar_like(rng, n, 15, 3) * 1e-2, 1e-2, 6 if grav else 15),
                              1e-2, 6 if grav else 15)
                dx, q1 = ctx4.debug_solve("li", W, case.H, case.g, case.u, 2.0, gravity=bool(grav))
                _check("li", case, dx, q1, 2.0)
        ctx.close()


def test_debug_solve_refuses(capi, ctx4):
    rng = np.random.default_rng(9)
    H = R.spd(rng, 24, 1e2); g = rng.standard_normal(24)
    for kind, W in (("lidar", 1), ("lidar", 17), ("li", 17), ("dense", 1)):
        n = 15 * W if kind == "li" else 6 * W
        with pytest.raises(capi.VbaError):
            ctx4.debug_solve(kind, W, np.eye(n), np.zeros(n), 1e-2)
    Hb = H.copy(); Hb[3, 7] += 1e-3                             # not symmetric
    Hn = H.copy(); Hn[5, 5] = np.nan
    for HH, gg, u in ((Hb, g, 1e-2), (Hn, g, 1e-2), (H, g, np.inf), (H, np.full(24, np.inf), 1e-2)):
        with pytest.raises(capi.VbaError):
            ctx4.debug_solve("lidar", 4, HH, gg, u)
    W = 4; n = 15 * W
    Hl = R.li_spd(rng, W, 0, 1e2)
    Hl[6, 15 * 2 + 7] = Hl[15 * 2 + 7, 6] = 1e-3                # v of frame 0 coupled with v of frame 2: outside the structure
    with pytest.raises(capi.VbaError):
        ctx4.debug_solve("li", W, Hl, np.zeros(n), 1e-2)
