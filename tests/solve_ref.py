"""Exact-residual reference, accuracy bars and a seeded corpus for the dense LDL^T solves of the LM loops: k_lm_solve_m (lidar,
n = 6W), k_li_solve (LI-BA, n = 15W (+3)) and big_solve (k_bigl_*, any window).  A helper module shared by tests/test_solve_cpu.py
(host solvers, mask, teeth) and tests/test_gpu_solve.py (the device kernels through vba_debug_solve).

The system a kernel factorises is formed here exactly as the kernel forms it (`effective`): gauge rows and columns -> identity with a
zero right-hand side, the damping a_ii + u a_ii in double precision.  For a returned x (x^) of A x = b:
  * r = b - A x^ exactly rounded: every product split error-free (Veltkamp/Dekker), each row summed by math.fsum;
  * x* = f64 LU with iterative refinement on those residuals (cross-checked against mpmath at 50 digits);
  * bars, u = 2^-53, C = 16:
      backward  |r|_inf / (|A|_inf |x^|_inf + |b|_inf) <= C n u
      forward   |x^ - x*|_2 / |x*|_2 <= C n u kappa_2(D^-1/2 A D^-1/2)   (van der Sluis scaling, D = diag(A))
      q1        |q1^ - q1(x^)| <= C n u sum_i |t_i|,  q1(x^) = sum_i t_i, t_i = 0.5 x^_i (u h_i x^_i - g_i), evaluated exactly.
    These are the bounds of a backward-stable symmetric solver, not tuned to any kernel.
Rows that are exactly zero in A and b (a frame without planes, translation rows without data) must come back exactly 0; the other
rows are held to the bars of the system without them."""
import math
from fractions import Fraction

import numpy as np
import scipy.linalg as sla

U = 2.0 ** -53
C_BAR = 16.0
KAPPAS = (1.0, 1e4, 1e8, 1e12)
DAMPINGS = (0.0, 1e-12, 1e-2, 1e3)


# ---------------------------------------------------------------- exact residual
def _split(a):
    c = 134217729.0 * a                       # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """a * b = p + e exactly (elementwise; no overflow or underflow at the magnitudes of the corpus)"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def residual(A, x, b):
    """b - A x, each row the correctly rounded value of the exact residual"""
    A = np.asarray(A, np.float64); x = np.asarray(x, np.float64); b = np.asarray(b, np.float64)
    P, E = two_prod(A, x[None, :])
    return np.array([math.fsum(np.concatenate(([b[i]], -P[i], -E[i]))) for i in range(len(b))])


def residual_fractions(A, x, b):
    """the same in exact rational arithmetic (slow: small n only)"""
    n = len(b)
    out = []
    for i in range(n):
        s = Fraction(float(b[i]))
        for j in range(n):
            s -= Fraction(float(A[i][j])) * Fraction(float(x[j]))
        out.append(s)
    return out


# ---------------------------------------------------------------- reference solution
def zero_rows(A, b):
    """rows that are exactly zero in A and in b"""
    return np.where(~np.any(A != 0, axis=1) & (b == 0))[0]


def ref_solve(A, b, iters=12):
    """x* of A x = b: LU (partial pivoting) + iterative refinement on exact residuals; exactly-zero rows give 0"""
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64)
    n = len(b)
    keep = np.setdiff1d(np.arange(n), zero_rows(A, b))
    Ak = A[np.ix_(keep, keep)]; bk = b[keep]
    lu = sla.lu_factor(Ak, check_finite=True)
    x = sla.lu_solve(lu, bk)
    for _ in range(iters):                           # until a correction no longer changes x
        xn = x + sla.lu_solve(lu, residual(Ak, x, bk))
        if np.array_equal(xn, x):
            break
        x = xn
    # a component the refinement leaves at a vanishing value next to an exact 0 (the correction of a correction): 0 where that is
    # at least as good in the exact residual
    r0 = np.abs(residual(Ak, x, bk)).max()
    for k in np.nonzero((x != 0) & (np.abs(x) < U * np.abs(x).max()))[0]:
        x2 = x.copy(); x2[k] = 0.0
        r2 = np.abs(residual(Ak, x2, bk)).max()
        if r2 <= r0:
            x, r0 = x2, r2
    out = np.zeros(n)
    out[keep] = x
    return out


def ref_solve_mp(A, b, dps=50):
    import mpmath
    with mpmath.workdps(dps):
        M = mpmath.matrix([[mpmath.mpf(float(v)) for v in row] for row in A])
        v = mpmath.matrix([mpmath.mpf(float(t)) for t in b])
        return np.array([float(t) for t in mpmath.lu_solve(M, v)])


# ---------------------------------------------------------------- the system a kernel factorises
def effective(H, g, u, gauge):
    """(A, b, h, gs): the gauged, damped matrix and right-hand side the solve kernels build (k_lm_solve_m, k_li_solve,
    k_bigl_setup), and the undamped gauged diagonal and gradient that q1 is formed from"""
    H = np.array(H, np.float64); g = np.array(g, np.float64)
    n = len(g)
    A = H.copy()
    A[:gauge, :] = 0.0; A[:, :gauge] = 0.0
    A[np.arange(gauge), np.arange(gauge)] = 1.0
    h = np.diag(A).copy()
    A[np.arange(n), np.arange(n)] = h + u * h
    gs = g.copy(); gs[:gauge] = 0.0
    return A, -gs, h, gs


def damping_of(u, v, b):
    """the damping of speculative candidate b: the f64 products b consecutive rejections form (u <- u v, v <- 2 v)"""
    for _ in range(b):
        u = u * v; v = 2 * v
    return u


# ---------------------------------------------------------------- bars
def kappa_scaled(A, keep=None):
    if keep is not None:
        A = A[np.ix_(keep, keep)]
    d = np.sqrt(np.abs(np.diag(A)))
    S = A / d[:, None] / d[None, :]
    w = np.abs(np.linalg.eigvalsh(S))
    return w.max() / w.min()


def ratios(A, b, x, xstar=None, kappa=None, gauge=0):
    """(backward ratio, forward ratio, exact-zero rows ok) of the returned x; a ratio <= 1 meets its bar.  The gauge rows (identity,
    zero right-hand side, decoupled) and the exactly-zero rows must come back exactly 0; the bars hold on the system of the others."""
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64); x = np.asarray(x, np.float64)
    n = len(b)
    z = np.union1d(zero_rows(A, b), np.arange(gauge))
    zeros_ok = bool(np.all(x[z] == 0.0))
    if not np.all(np.isfinite(x)):
        return math.inf, math.inf, zeros_ok
    keep = np.setdiff1d(np.arange(n), z)
    if len(keep) == 0:
        return 0.0, 0.0, zeros_ok
    if xstar is not None:
        xstar = xstar[keep]
    A = A[np.ix_(keep, keep)]; b = b[keep]; x = x[keep]
    n = len(b)
    bar = C_BAR * n * U
    r = residual(A, x, b)
    den = np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    bw = (np.abs(r).max() / den if den > 0 else (0.0 if np.abs(r).max() == 0 else math.inf)) / bar
    if xstar is None:
        xstar = ref_solve(A, b)
    if kappa is None:
        kappa = kappa_scaled(A)
    nx = np.linalg.norm(xstar)
    fw = (np.linalg.norm(x - xstar) / nx if nx > 0 else (0.0 if np.all(x == 0) else math.inf)) / (bar * kappa)
    return bw, fw, zeros_ok


def q1_ratio(q1, x, h, gs, u):
    """|q1 - sum t_i| / (C n u sum |t_i|), t_i = 0.5 x_i (u h_i x_i - g_i) in exact arithmetic"""
    F = Fraction
    fu = F(float(u))
    t = [F(1, 2) * F(float(x[i])) * (fu * F(float(h[i])) * F(float(x[i])) - F(float(gs[i]))) for i in range(len(x))]
    s = sum(t, F(0)); a = sum((abs(v) for v in t), F(0))
    err = abs(F(float(q1)) - s)
    if a == 0:
        return 0.0 if err == 0 else math.inf
    return float(err / (F(C_BAR) * len(x) * F(U) * a))


# ---------------------------------------------------------------- generators
def spd(rng, n, kappa):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, -np.log10(kappa), n) if kappa > 1 else np.ones(n)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def xstar_like(rng, n, stride=6, rot=3):
    """a solution with rotation components <= 0.5 (the first `rot` of every `stride`) and translations of a few metres"""
    x = rng.uniform(-2.0, 2.0, n)
    for k in range(0, n - n % stride, stride):
        x[k:k + rot] = rng.uniform(-0.5, 0.5, rot)
    return x


def rhs_for(H, x, u, gauge):
    """g such that the effective system at damping u has (about) the solution x: g = -(A x)"""
    A, _, _, _ = effective(H, np.zeros(len(x)), u, gauge)
    g = -(A @ x)
    g[:gauge] = 0.0
    return g


class Case:
    """one system: H, g (before the gauge), the damping, the gauge and a label; `probe` = (first twin, second twin) if any"""

    def __init__(self, label, H, g, u, gauge, probe=None):
        self.label, self.H, self.g, self.u, self.gauge, self.probe = label, np.asarray(H, np.float64), np.asarray(g, np.float64), float(u), gauge, probe


def lidar_cases(W, seed=0, dampings=DAMPINGS, kappas=KAPPAS):
    """the lidar classes at n = 6W: dense SPD at every kappa and damping, rotation rows scaled as at |p| up to 1e3 m, the whole
    system scaled by 2^+-400, semidefinite systems (a frame without data, zero translation rows) and the pivot-order probe"""
    rng = np.random.default_rng(1000 * W + seed)
    n = 6 * W
    out = []
    for kap in kappas:
        for u in dampings:
            H = spd(rng, n, kap)
            out.append(Case("spd k=%g u=%g" % (kap, u), H, rhs_for(H, xstar_like(rng, n), u, 6), u, 6))
    for pmax in (10.0, 1e3):           # rotation rows of a frame seen at |p|: J ~ [[p]x ; I], the rotation block ~ |p|^2
        s = np.ones(n)
        for f in range(W):
            s[6 * f:6 * f + 3] = rng.uniform(1.0, pmax)
        H = spd(rng, n, 1e4) * s[:, None] * s[None, :]
        H = 0.5 * (H + H.T)                             # (exactly symmetric again after the two roundings)
        out.append(Case("scaled-rot p=%g" % pmax, H, rhs_for(H, xstar_like(rng, n), 1e-2, 6), 1e-2, 6))
    for e in (400, -400):
        H = spd(rng, n, 1e4) * 2.0 ** e
        out.append(Case("scale 2^%d" % e, H, rhs_for(H, xstar_like(rng, n), 1e-2, 6), 1e-2, 6))
    if W >= 2:
        for u in (0.0, 1e-2):
            H = spd(rng, n, 1e4)
            f0 = 1 + int(rng.integers(W - 1))
            H[6 * f0:6 * f0 + 6, :] = 0.0; H[:, 6 * f0:6 * f0 + 6] = 0.0
            x = xstar_like(rng, n); x[6 * f0:6 * f0 + 6] = 0.0
            out.append(Case("zero frame u=%g" % u, H, rhs_for(H, x, u, 6), u, 6))
            H = spd(rng, n, 1e4)
            f1 = 1 + int(rng.integers(W - 1))
            z = np.arange(6 * f1 + 3, 6 * f1 + 6)
            H[z, :] = 0.0; H[:, z] = 0.0
            x = xstar_like(rng, n); x[z] = 0.0
            out.append(Case("zero translation u=%g" % u, H, rhs_for(H, x, u, 6), u, 6))
    out.append(probe_case(rng, n, 6))
    return out


def probe_case(rng, n, gauge, twins=None):
    """u = 0; two identical variables i < j whose shared diagonal is the largest power of two in the system.  After the first twin
    the second's row is exactly zero, so x comes out exactly 0 on the twin eliminated second: j, by 'first index wins ties'."""
    H = spd(rng, n, 1e2)
    H = H / np.abs(np.diag(H)).max()                  # diagonal <= 1 < 4
    if twins is None:
        i, j = sorted(rng.choice(np.arange(gauge, n), 2, replace=False))
    else:
        i, j = twins
    d = 4.0
    H[j, :] = H[i, :]; H[:, j] = H[:, i]
    H[i, i] = H[j, j] = H[i, j] = H[j, i] = d
    x = xstar_like(rng, n); x[j] = 0.0
    A, _, _, _ = effective(H, np.zeros(n), 0.0, gauge)
    g = -(A @ x); g[:gauge] = 0.0
    g[j] = g[i]                                        # identical rows, identical right-hand sides
    return Case("probe %d,%d" % (i, j), H, g, 0.0, gauge, probe=(int(i), int(j)))


def probe_reference(case):
    """x* of the probe: the system without the second twin, 0 there"""
    A, b, _, _ = effective(case.H, case.g, case.u, case.gauge)
    i, j = case.probe
    n = len(b)
    keep = np.array([k for k in range(n) if k != j])
    x = np.zeros(n)
    x[keep] = ref_solve(A[np.ix_(keep, keep)], b[keep])
    return x, kappa_scaled(A, keep)


def li_pattern(W, grav):
    """structurally allowed non-zeros of the LI system: 15 x 15 blocks (i, i) and (i, i +- 1), dense pose-pose coupling, gravity rows"""
    n = 15 * W + 3 * grav
    P = np.zeros((n, n), bool)
    for a in range(W):
        for b in range(max(0, a - 1), min(W, a + 2)):
            P[15 * a:15 * a + 15, 15 * b:15 * b + 15] = True
    pose = np.array([15 * f + k for f in range(W) for k in range(6)])
    P[np.ix_(pose, pose)] = True
    if grav:
        P[15 * W:, :] = True; P[:, 15 * W:] = True
    return P


def li_spd(rng, W, grav, kappa):
    """random SPD with every structurally allowed entry non-zero: IMU factors over (state i, state i+1, gravity) plus a dense
    pose-pose lidar part, each with eigenvalues spread over kappa"""
    n = 15 * W + 3 * grav
    H = np.zeros((n, n))
    pose = np.array([15 * f + k for f in range(W) for k in range(6)])
    H[np.ix_(pose, pose)] += spd(rng, 6 * W, kappa)
    for f in range(W - 1):
        idx = list(range(15 * f, 15 * f + 30)) + (list(range(15 * W, n)) if grav else [])
        H[np.ix_(idx, idx)] += spd(rng, len(idx), kappa)
    return 0.5 * (H + H.T)


def li_cases(W, grav, seed=0, dampings=(0.0, 1e-2, 1e3), kappas=KAPPAS):
    rng = np.random.default_rng(5000 + 100 * W + 10 * grav + seed)
    n = 15 * W + 3 * grav
    gauge = 6 if grav else 15
    out = []
    for kap in kappas:
        for u in dampings:
            H = li_spd(rng, W, grav, kap)
            out.append(Case("li k=%g u=%g" % (kap, u), H, rhs_for(H, xstar_like(rng, n, 15, 3), u, gauge), u, gauge))
    return out


def check(case, x, q1=None, u=None):
    """all ratios of one returned solution: dict(bw, fw, zeros[, q1]); zeros = exactly-zero rows (and the probe's second twin) are 0"""
    u = case.u if u is None else u
    A, b, h, gs = effective(case.H, case.g, u, case.gauge)
    if case.probe is not None and u == case.u:
        xs, kap = probe_reference(case)
        bw, fw, zok = ratios(A, b, x, xs, kap, gauge=case.gauge)
        zok = zok and x[case.probe[1]] == 0.0
    else:
        bw, fw, zok = ratios(A, b, x, gauge=case.gauge)
    out = dict(bw=bw, fw=fw, zeros=zok)
    if q1 is not None:
        out["q1"] = q1_ratio(q1, x, h, gs, u)
    return out


def worst(rows):
    """max of every ratio over a list of check() dicts"""
    return {k: max(r[k] for r in rows) for k in ("bw", "fw", "q1") if rows and k in rows[0]}


# ---------------------------------------------------------------- a numpy model of ldlt_mfma (for the teeth of the bars)
def blocked_ldlt_solve(A, b, skip=None):
    """LDL^T in ldlt_mfma's shape (panels of 8 columns, trailing update by 16 x 16 tiles) in the given order (no pivoting);
    skip = (panel, tile row, tile column) drops that tile's rank-8 update.  Zero pivots as the kernel: the column is left unscaled and
    a pivot |d| <= DBL_MIN gives a zero solution component."""
    A = np.array(A, np.float64); n = len(b)
    NP = (n + 15) // 16 * 16
    M = np.eye(NP); M[:n, :n] = np.tril(A)
    L = np.zeros((NP, NP)); d = np.zeros(NP)
    for kb in range(NP // 8):
        k0 = 8 * kb
        for c in range(k0, k0 + 8):                   # the panel, right-looking inside it
            dc = M[c, c]; d[c] = dc
            col = M[c + 1:, c].copy()
            L[c + 1:, c] = col / dc if dc != 0 else col
            T = col if dc != 0 else np.zeros_like(col)
            for cc in range(c + 1, k0 + 8):
                M[cc:, cc] -= L[cc:, c] * T[cc - c - 1]
        kn = k0 + 8
        if kn >= NP:
            break
        Lp = L[:, k0:kn]; Tp = Lp * np.where(d[k0:kn] != 0, d[k0:kn], 0.0)
        for ti in range(kn // 16, NP // 16):
            for tj in range(kn // 16, ti + 1):
                if skip is not None and skip == (kb, ti, tj):
                    continue
                r0, c0 = 16 * ti, 16 * tj
                upd = Lp[r0:r0 + 16] @ Tp[c0:c0 + 16].T
                R = np.arange(r0, r0 + 16)[:, None]; Cc = np.arange(c0, c0 + 16)[None, :]
                M[r0:r0 + 16, c0:c0 + 16] -= np.where((R >= Cc) & (Cc >= kn), upd, 0.0)
    Ln = L[:n, :n] + np.eye(n)
    z = sla.solve_triangular(Ln, b, lower=True, unit_diagonal=True)
    dd = d[:n]
    y = np.where(np.abs(dd) > np.finfo(float).tiny, z / np.where(dd != 0, dd, 1.0), 0.0)
    return sla.solve_triangular(Ln.T, y, lower=False, unit_diagonal=True)
