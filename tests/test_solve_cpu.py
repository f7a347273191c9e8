"""Host-side checks of the LM linear solves against the exact-residual reference of tests/solve_ref.py: the reference itself (exact
on integer systems, residuals equal to `fractions`, x* equal to mpmath at 50 digits), the product's host solver
vbh::ldlt_solve_inplace and the oracle's LDLT on the corpus, the teeth of the bars (each must catch a planted defect) and the LI
structure mask of k_li_solve (csrc/vba_li_order.hpp, built here by g++) against the symbolic fill of the permuted system."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import solve_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def host():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_solve_"), "libsolvehost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out,
                           os.path.join(HERE, "host", "solve_host.cpp")])
    lib = C.CDLL(out)
    lib.li_live_host.restype = C.c_uint
    return lib


def host_solve(lib, A, b):
    A = np.ascontiguousarray(A, np.float64).copy(); b = np.ascontiguousarray(b, np.float64); x = np.zeros(len(b))
    lib.ldlt_solve_host(A.ctypes.data_as(_dp), b.ctypes.data_as(_dp), x.ctypes.data_as(_dp), C.c_int(len(b)))
    return x


def test_reference_exact_on_integer_systems():
    rng = np.random.default_rng(3)
    for n in (3, 6, 12, 24, 48):
        for _ in range(5):
            M = np.tril(rng.integers(-9, 10, (n, n)), -1)
            M = M + M.T
            A = (M + np.diag(np.abs(M).sum(axis=1) + rng.integers(1, 4, n))).astype(np.float64)    # integer, diagonally dominant
            x = rng.integers(-50, 51, n).astype(np.float64)
            b = A @ x
            assert np.abs(b).max() < 2.0 ** 52
            assert np.array_equal(R.ref_solve(A, b), x)
            assert np.all(R.residual(A, x, b) == 0.0)


def test_residual_matches_fractions():
    rng = np.random.default_rng(4)
    for n in (2, 5, 9, 16):
        for e in (0, 300, -300):
            A = rng.standard_normal((n, n)) * 2.0 ** e
            x = rng.standard_normal(n)
            b = A @ x * (1 + 1e-9 * rng.standard_normal(n))
            exact = [float(v) for v in R.residual_fractions(A, x, b)]           # float(Fraction) rounds correctly
            assert np.array_equal(R.residual(A, x, b), np.array(exact))


def test_reference_matches_mpmath():
    rng = np.random.default_rng(5)
    for n in (6, 24, 48):
        for kap in R.KAPPAS:
            A = R.spd(rng, n, kap)
            b = A @ R.xstar_like(rng, n)
            x, xm = R.ref_solve(A, b), R.ref_solve_mp(A, b)
            assert np.linalg.norm(x - xm) <= 4 * R.U * np.linalg.norm(xm), (n, kap)


def _corpus():
    out = []
    for W in (2, 4, 10, 16):
        out += [("lidar W=%d" % W, c) for c in R.lidar_cases(W)]
    for W in (2, 5):
        for grav in (0, 1):
            out += [("li W=%d grav=%d" % (W, grav), c) for c in R.li_cases(W, grav, dampings=(1e-2,))]
    return out


def test_host_solvers_meet_bars(host, oracle):
    """vbh::ldlt_solve_inplace (the host twin of the device solvers' pivoting) and the oracle's Eigen-LDLT restatement"""
    worst = {}
    for name, case in _corpus():
        A, b, _, _ = R.effective(case.H, case.g, case.u, case.gauge)
        for who, x in (("host", host_solve(host, A, b)), ("oracle", oracle.ldlt_solve(A, b))):
            r = R.check(case, x)
            assert r["zeros"], (who, name, case.label)
            assert r["bw"] <= 1 and r["fw"] <= 1, (who, name, case.label, r)
            k = (who, name.split()[0])
            worst[k] = {q: max(worst.get(k, {}).get(q, 0.0), r[q]) for q in ("bw", "fw")}
    for k, v in sorted(worst.items()):
        print("worst ratio %-8s %-6s backward %.3g forward %.3g" % (k[0], k[1], v["bw"], v["fw"]))


def test_teeth_skipped_tile_update():
    """the numpy model of ldlt_mfma meets the bars; with one tile's rank-8 update skipped it must fail them"""
    rng = np.random.default_rng(6)
    n = 60
    H = R.spd(rng, n, 1e4)
    case = R.Case("teeth", H, R.rhs_for(H, R.xstar_like(rng, n), 1e-2, 6), 1e-2, 6)
    A, b, _, _ = R.effective(case.H, case.g, case.u, case.gauge)
    good = R.check(case, R.blocked_ldlt_solve(A, b))
    assert good["bw"] <= 1 and good["fw"] <= 1, good
    for skip in ((0, 2, 1), (3, 3, 2), (5, 3, 3)):
        bad = R.check(case, R.blocked_ldlt_solve(A, b, skip=skip))
        assert bad["bw"] > 1 or bad["fw"] > 1, (skip, bad)


def test_teeth_moved_component():
    """one component of x moved by 100 C n u (relative) on a kappa = 1 system must fail a bar"""
    rng = np.random.default_rng(7)
    for n in (12, 60, 96):
        H = R.spd(rng, n, 1.0)
        case = R.Case("teeth", H, R.rhs_for(H, R.xstar_like(rng, n), 0.0, 6), 0.0, 6)
        A, b, _, _ = R.effective(case.H, case.g, case.u, case.gauge)
        x = R.ref_solve(A, b)
        assert R.check(case, x)["bw"] <= 1
        k = int(np.argmax(np.abs(x)))
        x[k] *= 1 + 100 * R.C_BAR * n * R.U
        bad = R.check(case, x)
        assert bad["bw"] > 1 or bad["fw"] > 1, bad


def test_teeth_probe_tie_other_way(host):
    """the pivot-order probe solved with 'last index wins ties' must fail; with the product's rule it passes"""
    rng = np.random.default_rng(8)
    for n in (12, 60):
        case = R.probe_case(rng, n, 6)
        A, b, _, _ = R.effective(case.H, case.g, case.u, case.gauge)
        assert R.check(case, host_solve(host, A, b))["zeros"]
        d = np.abs(np.diag(A))
        for last_wins in (False, True):
            order = sorted(range(n), key=lambda k: (-d[k], -k if last_wins else k))
            P = np.array(order)
            x = np.zeros(n)
            x[P] = R.blocked_ldlt_solve(A[np.ix_(P, P)], b[P])
            r = R.check(case, x)
            ok = r["zeros"] and r["bw"] <= 1 and r["fw"] <= 1
            assert ok != last_wins, (n, last_wins, r)


def _symbolic_fill(P):
    """lower-triangular non-zero structure of L for the pattern P eliminated in its given order"""
    S = np.tril(P).copy()
    n = len(P)
    for k in range(n):
        idx = np.nonzero(S[k + 1:, k])[0] + k + 1
        if len(idx):
            S[np.ix_(idx, idx)] |= np.tril(np.ones((len(idx), len(idx)), bool))
    return S


@pytest.mark.parametrize("grav", [0, 1])
def test_li_mask_covers_fill(host, grav):
    """for W = 2..16 the host build of li_live covers, in every panel, every 16-row block that holds a non-zero of L (the
    symbolic fill of the LI pattern in li_ord's order), the right-hand side row included"""
    for W in range(2, 17):
        n = 15 * W + 3 * grav
        NP = ((15 * W + 3 + 1 + 15) // 16) * 16
        order = [host.li_ord_host(k, W) for k in range(n)]
        assert sorted(order) == list(range(n))
        Pt = R.li_pattern(W, grav)
        Pp = np.zeros((n + 1, n + 1), bool)
        Pp[:n, :n] = Pt[np.ix_(order, order)]
        Pp[n, :] = True                                  # the right-hand side row (dense)
        S = _symbolic_fill(Pp)
        for kb in range((n + 7) // 8):
            live = host.li_live_host(kb, W, n, NP)
            for c in range(8 * kb, min(8 * kb + 8, n)):
                rows = np.nonzero(S[c + 1:, c])[0] + c + 1
                blocks = set(int(r) >> 4 for r in rows)
                missing = [b for b in blocks if not (live >> b) & 1]
                assert not missing, (W, grav, kb, c, missing)
