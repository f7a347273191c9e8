"""Host-side checks of the device-resident kd-tree odometry: the kd mode of csrc/vba_odom_ekf.hpp (the step of
voxelslam.cpp:1206-1210 on the 28 sums of a point loop, the refind / rematch / stop rule of VS:1216-1233) compiled by g++ for one lane
against a numpy restatement, and the three new symbols through the C header, the ctypes table and the adapter."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from test_odom_ekf_cpu import _boxminus, _so3_exp, _so3_log, _spd, _state

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
SUMS_FN = C.CFUNCTYPE(None, C.c_int, DP, C.c_int, DP)
EPS = 2.0 ** -52


def _p(a):
    return a.ctypes.data_as(DP)


@pytest.fixture(scope="module")
def kd():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_kd_ekf_"), "libkdekfhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out, os.path.join(HERE, "host", "kd_ekf_host.cpp")])
    return C.CDLL(out)


def _pack28(HTH, HTz, valid=321):
    s = np.zeros(28)
    s[:21] = HTH[np.triu_indices(6)]
    s[21:27] = HTz
    s[27] = valid
    return s


def _unpack28(s28):
    HTH = np.zeros((6, 6)); i = 0
    for r in range(6):
        for c in range(r, 6):
            HTH[r, c] = HTH[c, r] = s28[i]; i += 1
    return HTH, s28[21:27].copy(), int(s28[27])


def _ref_step(s28, cov_inv, xp, xc):
    """VS:1206-1210: K_1 = (H_T_H + cov_inv / 1000)^-1, G(:,0:6) = K_1(:,0:6) HTH, solution = K_1(:,0:6) HTz + vec - G(:,0:6) vec(0:6)."""
    HTH, HTz, _ = _unpack28(s28)
    A = cov_inv / 1000; A[:6, :6] += HTH
    K1 = np.linalg.inv(A)
    G = np.zeros((15, 15)); G[:, :6] = K1[:, :6] @ HTH
    vec = _boxminus(xp, xc)
    return K1[:, :6] @ HTz + vec - G[:, :6] @ vec[:6], G, A


def _ref_loop(sums, state, cov):
    """VS:1135-1237 with the sums of each iteration's point loop handed in; sums(it, x_curr, refind)."""
    xp = state.copy(); xc = state.copy(); P = cov.copy()
    cov_inv = np.linalg.inv(P)
    rematch = 0; refind = True; converged_once = False
    trace = []; seen = []; after = []; rem = []; cov_iter = -1
    for it in range(4):
        seen.append(int(refind))
        s28 = sums(it, xc, int(refind))
        sol, G, _ = _ref_step(s28, cov_inv, xp, xc)
        xc = xc.copy()
        if np.linalg.norm(sol[:3]) >= 1e-11:
            xc[1:10] = (xc[1:10].reshape(3, 3) @ _so3_exp(sol[:3])).ravel()
        xc[10:22] += sol[3:]
        ra, ta = np.linalg.norm(sol[:3]), np.linalg.norm(sol[3:6])
        trace.append((_unpack28(s28)[2], ra, ta))
        refind = False                                                         # VS:1216-1227
        if ra * 57.3 < 0.01 and ta * 100 < 0.015:
            refind = True; converged_once = True; rematch += 1
        if it == 2 and not converged_once:
            refind = True
        after.append(int(refind)); rem.append(rematch)
        if rematch >= 2 or it == 3:                                            # VS:1229-1236
            P = (np.eye(15) - G) @ P
            cov_iter = it
            break
    return xc, P, np.array(trace), seen, after, rem, cov_iter


def _run_loop(kd, sums, state, cov):
    calls = []

    def cb(it, x25, refind, out28):
        x = np.ctypeslib.as_array(x25, shape=(25,)).copy()
        calls.append(it)
        np.ctypeslib.as_array(out28, shape=(28,))[:] = sums(it, x, refind)
    st = state.copy(); cv = np.ascontiguousarray(cov).copy(); tr = np.zeros(12)
    seen = np.zeros(4, np.int32); after = np.zeros(4, np.int32); rem = np.zeros(4, np.int32); ci = C.c_int(0); lr = C.c_int(0)
    n = kd.kd_ekf_loop_host(SUMS_FN(cb), _p(st), _p(cv), _p(tr), seen.ctypes.data_as(IP), after.ctypes.data_as(IP), rem.ctypes.data_as(IP),
                            C.byref(ci), C.byref(lr))
    return n, st, cv.reshape(15, 15), tr.reshape(4, 3), [int(v) for v in seen], [int(v) for v in after], [int(v) for v in rem], ci.value, lr.value, calls


# --------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("seed,plo,phi,jscale", [(0, 1e-3, 1e-1, 0.03), (1, 1e-4, 1e-1, 0.1), (2, 1e-5, 1e-2, 0.5), (3, 1e-4, 1e-4, 0.03)])
def test_one_step(kd, seed, plo, phi, jscale):
    """P SPD with eigenvalues in [plo, phi], HTH = J^T J of 300 rows.  A = HTH + P^-1 / 1000 has lambda_min >= 1 / (1000 phi) and
    lambda_max <= 1 / (1000 plo) + |J|_F^2 (Weyl), so kappa <= 1000 phi (1 / (1000 plo) + |J|_F^2) = phi / plo + 1000 phi |J|_F^2, which
    the parameters keep below 1e4.  Bar on the solution, relative to its max-norm: 100 kappa 15 eps (first-order forward bound, x100
    for the unmodelled constant), the bar of test_odom_ekf_cpu.py."""
    rng = np.random.default_rng(seed)
    P = _spd(rng, 15, plo, phi)
    cov_inv = np.linalg.inv(P)
    J = rng.normal(0, jscale, (300, 6))
    HTH = J.T @ J
    assert phi / plo + 1000 * phi * (J ** 2).sum() <= 1e4
    HTz = rng.normal(0, jscale * 3.0, 6)
    R = _so3_exp(rng.normal(0, 0.5, 3))
    xc = _state(R, rng.normal(0, 5, 3))
    xp = xc.copy()
    xp[1:10] = (R @ _so3_exp(rng.normal(0, 0.02, 3))).ravel()
    xp[10:22] += rng.normal(0, 0.02, 12)
    s28 = _pack28(HTH, HTz)
    sol = np.zeros(15); G = np.zeros(90); K = np.zeros(90)
    kd.kd_ekf_step_host(_p(s28), _p(np.ascontiguousarray(cov_inv / 1000)), _p(xp), _p(xc), _p(sol), _p(G), _p(K))
    ref, G_ref, A = _ref_step(s28, cov_inv, xp, xc)
    kappa = np.linalg.cond(A)
    bar = 100 * kappa * 15 * EPS
    err = np.abs(sol - ref).max() / np.abs(ref).max()
    print("seed %d: kappa %.4g, solution error %.3g of its max-norm, bar %.3g" % (seed, kappa, err, bar))
    assert kappa <= 1e4
    assert err <= bar
    assert np.abs(G.reshape(15, 6) - G_ref[:, :6]).max() <= bar * np.abs(G_ref).max()
    assert np.abs(K.reshape(15, 6) - np.linalg.inv(A)[:, :6]).max() <= bar * np.abs(np.linalg.inv(A)).max()


# --------------------------------------------------------------------------------------------- refind / rematch / stop
def _quadratic(H, targets):
    """Sums of the cost 1/2 d^T H d, d = x_curr - target(iter) in (rotation, position): HTH = H, HTz = -H d."""
    def sums(it, x, refind):
        Rt, pt = targets(it)
        d = np.concatenate([_so3_log(Rt.T @ x[1:10].reshape(3, 3)), x[10:13] - pt])
        return _pack28(H, -H @ d, valid=300 + it)
    return sums


def _setup(seed=11):
    rng = np.random.default_rng(seed)
    R0 = _so3_exp(rng.normal(0, 0.4, 3)); p0 = rng.normal(0, 3, 3)
    J = rng.normal(0, 1.0, (400, 6))
    cov = np.eye(15) * 1e-4; cov[9:, 9:] = np.eye(6) * 1e-5
    return rng, R0, p0, J.T @ J * 50.0, _state(R0, p0), cov


def _jump(rng, R0, p0):
    return R0 @ _so3_exp(rng.normal(0, 0.02, 3)), p0 + rng.normal(0, 0.1, 3)


def _compare(kd, sums, H, state, cov, iters, seen, after, rem):
    n, st, cv, tr, seen_h, after_h, rem_h, ci, lr, calls = _run_loop(kd, sums, state, cov)
    st_r, cv_r, tr_r, seen_r, after_r, rem_r, ci_r = _ref_loop(sums, state, cov)
    print("iterations %d (restatement %d), refind found %s, left %s, rematch_num %s, covariance written at %d\n%s"
          % (n, len(tr_r), seen_h, after_h, rem_h, ci, tr[:n]))
    assert n == len(tr_r) == iters
    assert lr == iters and calls == list(range(iters))            # the launches after the stop returned at the gate
    assert ci == ci_r == iters - 1
    pad = [-1] * (4 - iters)
    assert seen_h == seen_r + pad == seen + pad
    assert after_h == after_r + pad == after + pad
    assert rem_h == rem_r + pad == rem + pad
    # one step is good to 100 kappa 15 eps of a solution below 1 in max-norm (test_one_step), with kappa of H + P^-1 / 1000 as it is
    # here; up to four steps, on state entries up to ~10 whose rounding adds a few 1e-15
    A = np.linalg.inv(cov) / 1000; A[:6, :6] += H
    bar = 4 * 100 * np.linalg.cond(A) * 15 * EPS + 1e-14
    print("state difference %.3g, covariance %.3g of its largest entry, bar %.3g" % (np.abs(st - st_r).max(), np.abs(cv - cv_r).max() / np.abs(cv_r).max(), bar))
    assert np.abs(st - st_r).max() < bar
    assert np.abs(cv - cv_r).max() < bar * np.abs(cv_r).max()
    assert np.array_equal(tr[:n, 0], tr_r[:, 0])
    assert np.abs(tr[:n, 1:] - tr_r[:, 1:]).max() < bar
    assert np.all(tr[n:] == 0)
    return st, cv


def test_loop_converged_at_0_and_1(kd):
    """The target is the prediction: iterations 0 and 1 both converge and search again, the loop stops after two."""
    rng, R0, p0, H, state, cov = _setup()
    _compare(kd, _quadratic(H, lambda it: (R0, p0)), H, state, cov, 2, [1, 1], [1, 1], [1, 2])


def test_loop_never_converged(kd):
    """The target jumps before every iteration: no rematch is counted, iteration 2 forces the search of iteration 3, stop after four."""
    rng, R0, p0, H, state, cov = _setup()
    tg = [_jump(rng, R0, p0) for _ in range(4)]
    _, cv = _compare(kd, _quadratic(H, lambda it: tg[it]), H, state, cov, 4, [1, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 0])
    assert not np.array_equal(cv, cov)


def test_loop_converged_only_at_0(kd):
    """The prediction holds for iteration 0, then the target jumps before each of the others: one rematch, no forced search at
    iteration 2 (one iteration has converged), stop after four."""
    rng, R0, p0, H, state, cov = _setup()
    tg = [(R0, p0)] + [_jump(rng, R0, p0) for _ in range(3)]
    _compare(kd, _quadratic(H, lambda it: tg[it]), H, state, cov, 4, [1, 1, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1])


def test_loop_converged_only_at_2(kd):
    """The target jumps before iterations 0 and 1, holds for 2 and jumps again before 3: iteration 2 is the only rematch, stop after four."""
    rng, R0, p0, H, state, cov = _setup()
    a, b, c = (_jump(rng, R0, p0) for _ in range(3))
    tg = [a, b, b, c]
    _compare(kd, _quadratic(H, lambda it: tg[it]), H, state, cov, 4, [1, 0, 0, 1], [0, 0, 1, 0], [0, 0, 1, 1])


def test_loop_zero_sums(kd):
    """No valid point at all (an empty scan): the solution is exactly zero, two iterations, state and covariance bit-identical."""
    rng, R0, p0, H, state, cov = _setup()
    cov = _spd(rng, 15, 1e-5, 1e-3)
    n, st, cv, tr, seen, after, rem, ci, lr, calls = _run_loop(kd, lambda it, x, refind: np.zeros(28), state, cov)
    assert n == 2 and lr == 2 and ci == 1
    assert np.array_equal(st, state)
    assert np.array_equal(cv, cov)
    assert np.all(tr == 0)
    assert rem == [1, 2, -1, -1]


# --------------------------------------------------------------------------------------------- ABI
NEW = ["vba_odom_lio_state_estimation_kdtree_resident", "vba_odom_kdtree_reserve", "vba_odom_kdtree_allocations"]


def test_symbols_declared_and_listed():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    for s in NEW:
        assert re.search(r"^int %s\(vba_ctx \*ctx," % s, hdr, re.M), s
        assert s in capi.EXPORTS, s
    for m in ("lio_state_estimation_kdtree_resident", "kdtree_reserve", "kdtree_allocations"):
        assert callable(getattr(capi.Context, m))


def test_adapter_overload_compiles(tmp_path):
    src = tmp_path / "kd_adapter_check.cpp"
    src.write_text(r'''
#include "voxelba_adapter.hpp"
int (*on_frame)(vba::Context &, const vba::ScanView &, vba::IMUST &, vba_odom_report *) = &vba::lio_state_estimation_kdtree;
int (*on_host)(vba::Context &, const std::vector<vba::pointVar> &, vba::IMUST &) = &vba::lio_state_estimation_kdtree;
int use(vba::Context &c, const vba::ScanView &v, vba::IMUST &x) { vba_odom_report r; return vba::lio_state_estimation_kdtree(c, v, x) + vba::lio_state_estimation_kdtree(c, v, x, &r); }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
