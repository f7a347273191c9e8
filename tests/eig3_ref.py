"""High-precision reference, corpus and accuracy bars for the symmetric 3x3 eigen-solver of the plane fit (csrc/vba_eig3.hpp with its
Jacobi fallback eig3_jacobi_dev in csrc/vba_kernels_factor.hpp).  A helper module shared by tests/test_eig3_cpu.py (host build of the
direct path) and tests/test_gpu_eig3.py (the device sites behind the C ABI).

Reference: mpmath.eigsy at 50 digits on the exact double matrix.  Bars, for a result (w, V) against (w*, V*), s = |A|_2:
  * every output finite, w ascending;
  * |w_i - w*_i| <= C eps s;
  * max|V^T V - I| <= 1e-14 and max|A V - V W| <= C eps s;
  * sin(v_i, v*_i) <= C eps s / gap_i wherever that bound is below 1 (gap_i = min_{j != i} |w*_i - w*_j|);
  * for a pair closer than 1e-8 s: |P - P*|_2 <= C eps s / (gap to the third eigenvalue), P the projector on the pair's span;
with C = 16.  These are the bounds of a backward-stable solver (Davis-Kahan); sign of each vector is free.  Absolute bars get a
further 2^-1074 (one unit of the subnormal grid: an output below 2^-1022 cannot be closer than that to anything)."""
import mpmath
import numpy as np

EPS = np.finfo(np.float64).eps
C_BAR = 16.0
PAIR_REL = 1e-8                      # a pair closer than PAIR_REL * s is checked as a subspace
TINY = 2.0 ** -1074
THRESH = 1e-10                       # the direct path's fallback test: (x_b - x_c)^2 = D > THRESH * c1
MP_DPS = 50


def tri(A):
    """symmetric 3x3 -> lower triangle a00 a10 a20 a11 a21 a22 (the order the solver and the cluster sums use)"""
    return np.array([A[0, 0], A[1, 0], A[2, 0], A[1, 1], A[2, 1], A[2, 2]], dtype=np.float64)


class Ref:
    """mpmath eigen-decomposition of one exact double matrix."""

    def __init__(self, A, M=None):
        """A: the double matrix; M (optional): the exact matrix as an mpmath matrix, when A is only its rounding"""
        A = np.asarray(A, dtype=np.float64)
        with mpmath.workdps(MP_DPS):
            if M is None:
                M = mpmath.matrix([[mpmath.mpf(float(A[i, j])) for j in range(3)] for i in range(3)])
            E, Q = mpmath.eigsy(M)
            order = sorted(range(3), key=lambda i: E[i])
            self.w_mp = [E[i] for i in order]
            self.V_mp = [[Q[r, i] for i in order] for r in range(3)]
            self.s_mp = max(abs(x) for x in self.w_mp)
            gaps = [min(abs(self.w_mp[i] - self.w_mp[j]) for j in range(3) if j != i) for i in range(3)]
        self.A = A
        self.w = np.array([float(x) for x in self.w_mp])
        self.V = np.array([[float(x) for x in row] for row in self.V_mp])
        self.s = float(self.s_mp)
        self.gap = np.array([float(g) for g in gaps])
        # clusters of eigenvalues closer than PAIR_REL * s (adjacent, ascending)
        d01 = abs(self.w[1] - self.w[0]) <= PAIR_REL * self.s
        d12 = abs(self.w[2] - self.w[1]) <= PAIR_REL * self.s
        self.pair = None                 # (i, j, gap to the third) for a close pair, not a triple
        if d01 and not d12:
            self.pair = (0, 1, float(self.w_mp[2] - self.w_mp[1]))
        elif d12 and not d01:
            self.pair = (1, 2, float(self.w_mp[1] - self.w_mp[0]))
        self.triple = d01 and d12
        if self.pair is not None:
            i, j, _ = self.pair
            self.P = np.outer(self.V[:, i], self.V[:, i]) + np.outer(self.V[:, j], self.V[:, j])

    def dc1(self):
        """(D / c1) of the direct path's fallback test, from the exact eigenvalues: D = (pair gap)^2, c1 = sum of squared gaps / 6"""
        w = [mpmath.mpf(x) for x in self.w_mp]
        c1 = ((w[0] - w[1]) ** 2 + (w[1] - w[2]) ** 2 + (w[0] - w[2]) ** 2) / 6
        if c1 == 0:
            return 0.0
        D = min((w[0] - w[1]) ** 2, (w[1] - w[2]) ** 2)
        return float(D / c1)


def ref_from_sums(pa):
    """Reference of cov = P/N - (v/N)(v/N)^T formed exactly from a cluster's sums (Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N, doubles), and the
    cancellation scale m2 = max|P/N| that bounds the rounding of the same cov formed in f64."""
    with mpmath.workdps(MP_DPS):
        N = mpmath.mpf(float(pa[9]))
        P = [mpmath.mpf(float(x)) / N for x in pa[:6]]
        c = [mpmath.mpf(float(x)) / N for x in pa[6:9]]
        a00, a10, a20, a11, a21, a22 = (P[0] - c[0] * c[0], P[1] - c[1] * c[0], P[2] - c[2] * c[0], P[3] - c[1] * c[1], P[4] - c[2] * c[1],
                                        P[5] - c[2] * c[2])
        M = mpmath.matrix([[a00, a10, a20], [a10, a11, a21], [a20, a21, a22]])
        A = np.array([[float(M[i, j]) for j in range(3)] for i in range(3)])
        m2 = float(max(abs(x) for x in P))
    return Ref(A, M), m2


def _sin(v, u):
    v = v / np.linalg.norm(v)
    return float(np.linalg.norm(v - (v @ u) * u))


def check(ref, w, V, scale=None, C=C_BAR):
    """Ratios (observed / bar) of every bar for one result; scale replaces s (the cancellation scale of a cov formed from sums).
    Returns a dict name -> ratio; a ratio above 1 is a failure.  Non-finite output or descending w gives inf."""
    w = np.asarray(w, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64).reshape(3, 3)
    s = ref.s if scale is None else max(scale, ref.s)
    out = {}
    if not (np.all(np.isfinite(w)) and np.all(np.isfinite(V))) or not (w[0] <= w[1] <= w[2]):
        return {"finite_ascending": np.inf}
    bar_abs = C * EPS * s + TINY
    with mpmath.workdps(MP_DPS):
        out["eigval"] = max(float(abs(mpmath.mpf(float(w[i])) - ref.w_mp[i])) for i in range(3)) / bar_abs
    out["orth"] = float(np.abs(V.T @ V - np.eye(3)).max()) / 1e-14
    # A V - V W in extended precision (the check's own rounding stays far below the bar)
    Al, Vl, wl = ref.A.astype(np.longdouble), V.astype(np.longdouble), w.astype(np.longdouble)
    out["resid"] = float(np.abs(Al @ Vl - Vl * wl).max()) / bar_abs
    vr = 0.0
    pair = ref.pair[:2] if ref.pair is not None else ()
    for i in range(3):
        if i in pair or ref.triple:
            continue
        if ref.gap[i] <= 0.0:
            continue
        bound = C * EPS * (s / ref.gap[i])          # (s / gap first: for a subnormal matrix eps * s underflows)
        if bound < 1.0:
            vr = max(vr, _sin(V[:, i], ref.V[:, i]) / bound)
    out["vec"] = vr
    if ref.pair is not None:
        i, j, g3 = ref.pair
        bound = C * EPS * (s / g3)
        if bound < 1.0:
            P = np.outer(V[:, i], V[:, i]) + np.outer(V[:, j], V[:, j])
            out["span"] = float(np.linalg.norm(P - ref.P, 2)) / bound
    return out


def worst(ratios):
    return max(ratios.values()) if ratios else 0.0


# ------------------------------------------------------------------------------------------------ corpus
G_LIST = (1e-2, 1e-3, 1e-4, 3e-5, 1.1e-5, 9e-6, 1e-6, 1e-9, 0.0)
SCALES = (-900, -500, -100, 100, 500, 900)


def _rot(rng):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.diag(R))


def _spec(Q, lam):
    A = (Q * np.asarray(lam, dtype=np.float64)) @ Q.T
    return 0.5 * (A + A.T)


def plane_patch(rng, m=None):
    """cov = P/N - c c^T of a noisy planar patch 10-100 m from the origin (the matrices K4 sees)."""
    n = rng.normal(size=3); n /= np.linalg.norm(n)
    t1 = np.cross(n, rng.normal(size=3)); t1 /= np.linalg.norm(t1); t2 = np.cross(n, t1)
    m = int(rng.integers(6, 400)) if m is None else m
    ext = rng.uniform(0.02, 0.3, 2)
    c0 = rng.normal(size=3); c0 *= rng.uniform(10, 100) / np.linalg.norm(c0)
    pts = c0 + np.outer(rng.uniform(-1, 1, m) * ext[0], t1) + np.outer(rng.uniform(-1, 1, m) * ext[1], t2) + np.outer(rng.normal(0, 0.01, m), n)
    c = pts.mean(0)
    return pts.T @ pts / m - np.outer(c, c)


def corpus(seed=20261015, n_plane=300, n_rot=64):
    """list of (class, 3x3 matrix).  Classes: a planar patches, b top near-double pairs, c bottom pairs (line-like) and rank 1,
    d exact rank 2 / qI / zero / diagonal / single off-diagonal, e = a-d scaled by 2^k, f subnormal."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_plane):
        out.append(("a", plane_patch(rng)))
    for g in G_LIST:
        for _ in range(n_rot):
            l1 = rng.uniform(0.5, 2.0)
            out.append(("b", _spec(_rot(rng), [1e-4 * l1, l1, l1 * (1.0 + g)])))
    for g in G_LIST:
        for _ in range(n_rot):
            l0 = rng.uniform(0.5, 2.0) * 1e-4
            out.append(("c", _spec(_rot(rng), [l0, l0 * (1.0 + g), 1.0])))
    for u in ((1.0, 2.0, 3.0), (0.0, 0.0, 1.0), (0.5, -0.25, 0.125), (3.0, 0.0, -4.0)):
        u = np.array(u)
        out.append(("c", np.outer(u, u)))                          # exact rank 1 (products of few-bit numbers are exact)
    for _ in range(8):
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        out.append(("c", np.outer(u, u) * rng.uniform(0.5, 2.0)))  # rank 1 up to rounding
    for u, v in (((1.0, 2.0, 3.0), (2.0, -1.0, 0.0)), ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.5, 0.5, 1.0), (-1.0, 1.0, 0.0))):
        u, v = np.array(u), np.array(v)
        out.append(("d", np.outer(u, u) + np.outer(v, v)))         # exact rank 2
    for q in (1.0, -2.5, 1e-3, 0.0):
        out.append(("d", q * np.eye(3)))
    for dg in ((3.0, 1.0, 2.0), (1.0, 1.0, 3.0), (2.0, 5.0, 5.0), (4.0, -1.0, 4.0), (0.0, 1e-4, 1.0), (-1.0, 0.0, 1.0)):
        for p in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            out.append(("d", np.diag([dg[p[0]], dg[p[1]], dg[p[2]]])))
    for (i, j) in ((0, 1), (0, 2), (1, 2)):
        A = np.zeros((3, 3)); A[i, j] = A[j, i] = 0.75
        out.append(("d", A))
        A = np.diag([1.0, 1.0, 1.0]); A[i, j] = A[j, i] = 1e-3
        out.append(("d", A))
    base = list(out)
    for k, (cls, A) in enumerate(base):
        if k % 3 == 0:
            for e in SCALES:
                out.append(("e", np.ldexp(A, e)))
    out.append(("f", np.array([[3e-310, 1e-310, 0.0], [1e-310, 2e-310, 0.0], [0.0, 0.0, 1e-311]])))
    out.append(("f", np.array([[2e-309, -1e-309, 5e-310], [-1e-309, 2e-309, 0.0], [5e-310, 0.0, 1e-309]])))
    return out


_REFS = {}


def refs(items):
    """References of a corpus (cached by the matrix bytes: the K4, host and GBA tests share them)."""
    out = []
    for _, A in items:
        key = np.ascontiguousarray(A).tobytes()
        r = _REFS.get(key)
        if r is None:
            r = _REFS[key] = Ref(A)
        out.append(r)
    return out


def plane_judge(w, min_eigen_value, plane_thre):
    """plane_judge (voxel_map.hpp): lambda0 < min_eigen_value and lambda0 / lambda2 < plane_thre"""
    return (w[0] < min_eigen_value) and (w[0] / w[2] < plane_thre)
