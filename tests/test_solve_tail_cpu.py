"""The claim behind the shortened lidar factorisation, in the numpy model of ldlt_mfma (solve_ref.blocked_ldlt_solve): the gauge rows
are identity rows with a zero right-hand side, decoupled from every other row.  Where Eigen's order ("largest |stored diagonal| first")
puts them behind every live row, the panels behind the one that holds the last live rank only factorise rows that cannot influence
anything: solving the leading 8 npan columns of the permuted system gives the same values as solving all of it, and the components
beyond are 0.

The model's two triangular solves are replaced by explicit loops in a fixed order: LAPACK changes its summation order with n, so
scipy's solve_triangular on systems of different n differs by a few ulp for reasons that have nothing to do with the claim."""
import types

import numpy as np
import pytest

import solve_ref as R

PAIRS = ((1.0, 1e-2), (1e4, 0.0), (1e8, 1e-2), (1e4, 1e3))          # (kappa, u)


def _solve_triangular_loops(T, b, lower=True, unit_diagonal=True, **_):
    """unit triangular solve, one scalar operation after the other: row i sums its terms in the order of the elimination"""
    assert unit_diagonal
    n = len(b)
    x = np.array(b, np.float64)
    if lower:
        for i in range(n):
            acc = x[i]
            for j in range(i):
                acc -= T[i, j] * x[j]
            x[i] = acc
    else:
        for i in range(n - 1, -1, -1):
            acc = x[i]
            for j in range(n - 1, i, -1):
                acc -= T[i, j] * x[j]
            x[i] = acc
    return x


@pytest.fixture()
def loops(monkeypatch):
    """solve_ref.blocked_ldlt_solve with explicit substitution loops (its module-level scipy handle swapped for the call)"""
    monkeypatch.setattr(R, "sla", types.SimpleNamespace(solve_triangular=_solve_triangular_loops))
    return R.blocked_ldlt_solve


def permuted_system(W, kappa, u, rng):
    """(A, b, live) of one case in Eigen's order: spd(kappa) 1e3 + 10 I so that every live diagonal exceeds 1, gauge 6"""
    n = 6 * W
    H = R.spd(rng, n, kappa) * 1e3 + 10.0 * np.eye(n)
    A, b, _, _ = R.effective(H, R.rhs_for(H, R.xstar_like(rng, n), u, 6), u, 6)
    d = np.abs(np.diag(A))
    P = np.array(sorted(range(n), key=lambda k: (-d[k], k)))           # first index wins ties
    return A[np.ix_(P, P)], b[P], P >= 6


def test_trailing_decoupled_panels_change_nothing(loops):
    lost = 0
    cases = 0
    for W in range(2, 17):
        for kappa, u in PAIRS:
            rng = np.random.default_rng(100 * W + int(np.log10(kappa)) + int(u > 1))
            A, b, live = permuted_system(W, kappa, u, rng)
            n = len(b)
            assert np.diag(A)[live].min() > abs(1.0 + u), "every live row ranks before the gauge rows"
            rmax = int(np.nonzero(live)[0].max())
            m = 8 * (rmax // 8 + 1)
            full = loops(A, b)
            assert np.all(full[~live] == 0.0), (W, kappa, u)
            m = min(m, n)
            short = loops(A[:m, :m], b[:m])
            assert np.array_equal(full[:m], short), (W, kappa, u)
            assert np.all(full[m:] == 0.0), (W, kappa, u)
            cases += 1
            lost += 1 if m < n else 0
    # (the test cannot pass without having exercised the shortened form)
    assert cases == 60 and lost == 44, (cases, lost)


def test_loops_solve_the_triangular_systems():
    """the explicit loops are a substitution: componentwise residual within the bound of one, |b - T x| <= gamma_n |T| |x|
    (gamma_n <= 2 n u here)"""
    rng = np.random.default_rng(11)
    for n in (8, 24, 60):
        L = np.tril(rng.standard_normal((n, n)), -1) * 0.1 + np.eye(n)
        b = rng.standard_normal(n)
        for T, lower in ((L, True), (L.T, False)):
            x = _solve_triangular_loops(T, b, lower=lower, unit_diagonal=True)
            r = np.array([abs(float(v)) for v in R.residual_fractions(T, x, b)])
            assert np.all(r <= 2 * n * R.U * (np.abs(T) @ np.abs(x))), (n, lower)
