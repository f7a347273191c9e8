"""The solve kernels end the factorisation with the panel of the last live pivot (k_lm_solve_m: the largest rank of a row k >= 6;
k_li_solve: column n of the structure order).  Single solves through vba_debug_solve, at every lidar window and at the LI windows
where the kernel changes form, on systems where the limit fires, where a live row ranks behind the gauge rows, where zero rows sit
behind them, on the pivot-order probe and on the device's own Hessians.  Every case is held to the bars of tests/solve_ref.py for
every damping candidate, to exact zeros on gauge and zero rows, and to equality by value (array_equal: the sign of a zero may
differ) with the launch that runs every panel (all_panels), with a one-candidate solve at each candidate's damping and with the
other forms of the kernel (tile packing, load order)."""
import dataclasses
import os

import numpy as np
import pytest

import solve_ref as R

pytestmark = pytest.mark.gpu

V = 2.0
PAIRS = ((1.0, 1e-2), (1e4, 0.0), (1e8, 1e-2), (1e4, 1e3))          # (kappa, u)


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


@pytest.fixture(scope="module")
def ctx1(capi):
    c = _ctx(capi, 1)
    yield c
    c.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _hold(ctx4, ctx1, kind, W, case, forms, **kw):
    """every check of the module on one case; `forms` = the flag sets whose launch must equal the default one"""
    out = ctx4.debug_solve(kind, W, case.H, case.g, case.u, V, **kw)
    dx, q1 = out
    assert len(q1) == 4
    for b in range(len(q1)):
        ub = R.damping_of(case.u, V, b)
        r = R.check(case, dx[b], q1[b], u=ub)
        assert np.all(dx[b][:case.gauge] == 0.0), (kind, W, case.label, b)
        assert r["zeros"], (kind, W, case.label, b)
        assert r["bw"] <= 1 and r["fw"] <= 1 and r["q1"] <= 1, (kind, W, case.label, b, r)
        one = ctx1.debug_solve(kind, W, case.H, case.g, ub, V, **kw)
        assert np.array_equal(one[0][0], dx[b]) and one[1][0] == q1[b], (kind, W, case.label, b)
    assert _same(ctx4.debug_solve(kind, W, case.H, case.g, case.u, V, all_panels=True, **kw), out), (kind, W, case.label, "all_panels")
    for fl in forms:
        assert _same(ctx4.debug_solve(kind, W, case.H, case.g, case.u, V, **fl, **kw), out), (kind, W, case.label, fl)
        assert _same(ctx4.debug_solve(kind, W, case.H, case.g, case.u, V, all_panels=True, **fl, **kw), out), (kind, W, case.label, fl, "all_panels")


LIDAR_FORMS = (dict(e_packed=True), dict(copy_raw=True), dict(copy_raw=True, from_raw=True), dict(e_packed=True, copy_raw=True))
LI_FORMS = (dict(copy_raw=True), dict(copy_raw=True, from_raw=True))


def lidar_tail_cases(W):
    """(a) every live diagonal > 1: the gauge rows take the last six ranks and the limit fires; (b) the same with one live diagonal
    scaled below 1 (row and column by 2^-8, exact): that row ranks behind the gauge rows and nothing or less is skipped;
    (c) solve_ref's zero frame / zero translation systems at u = 0: zero rows behind the gauge rows; (d) the pivot-order probe"""
    n = 6 * W
    out = []
    for kappa, u in PAIRS:
        rng = np.random.default_rng(7000 + 100 * W + int(np.log10(kappa)) + int(u > 1))
        H = R.spd(rng, n, kappa) * 1e3 + 10.0 * np.eye(n)
        assert np.diag(H)[6:].min() > 1.0
        out.append(R.Case("tail k=%g u=%g" % (kappa, u), H, R.rhs_for(H, R.xstar_like(rng, n), u, 6), u, 6))
        k = 6 + int(rng.integers(n - 6))
        s = np.ones(n); s[k] = 2.0 ** -8
        Hb = H * s[:, None] * s[None, :]
        assert Hb[k, k] < 1.0 and np.array_equal(Hb, Hb.T)
        out.append(R.Case("late row %d k=%g u=%g" % (k, kappa, u), Hb, R.rhs_for(Hb, R.xstar_like(rng, n), u, 6), u, 6))
    ref = R.lidar_cases(W, dampings=(1e-2,), kappas=(1.0,))
    out += [c for c in ref if c.label in ("zero frame u=0", "zero translation u=0") or c.probe is not None]
    assert len(out) == 11
    return out


@pytest.mark.parametrize("W", list(range(2, 17)))
def test_lidar_tail(ctx4, ctx1, W):
    for case in lidar_tail_cases(W):
        _hold(ctx4, ctx1, "lidar", W, case, LIDAR_FORMS)


@pytest.mark.parametrize("part", [0, 1, 2, 3])
@pytest.mark.parametrize("grav", [0, 1])
@pytest.mark.parametrize("W", [2, 5, 10, 11, 16])
def test_li_tail(ctx4, ctx1, W, grav, part):
    """li_cases(W, grav), three systems (one kappa at its three dampings) per test: the exact-residual reference at n = 243 takes a
    third of a second per candidate"""
    cases = R.li_cases(W, grav)
    assert len(cases) == 12
    for case in cases[3 * part:3 * part + 3]:
        _hold(ctx4, ctx1, "li", W, case, LI_FORMS, gravity=bool(grav))


def test_lidar_tail_device_hessian(capi, ctx4, ctx1):
    """(e) the device's own room Hessian at W = 4, 10, 16, as test_gpu_solve.test_realistic_systems builds it"""
    from voxel_slam_amd import synth
    rng = np.random.default_rng(78)
    for W in (4, 10, 16):
        wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="room_w%d" % W, win_size=W)
        s = synth.make_scans(wl)
        fac = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
        poses = synth.poses_flat(s["R0"], s["p0"])
        o = capi.default_options(); o.win_size = W; o.imu_coef = wl.imu_coef
        ctx = capi.Context(o); ctx.push_dict(fac)
        H, _, _ = ctx.acc_evaluate2(poses)
        ctx.close()
        H = 0.5 * (H + H.T)
        for u in (1e-2, 1e-6):
            x = R.xstar_like(rng, 6 * W) * 1e-2
            case = R.Case("realistic W=%d u=%g" % (W, u), H, R.rhs_for(H, x, u, 6), u, 6)
            _hold(ctx4, ctx1, "lidar", W, case, LIDAR_FORMS)
