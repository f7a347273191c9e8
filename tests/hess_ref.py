"""High-precision reference, magnitude shadow, accuracy bars and corpus for the Hessian / gradient pass (k_hessian2<W>, k_hessian3<W>
with slot_terms, tl_fetch and k_reduce_partials: csrc/vba_kernels_factor.hpp, csrc/vba_kernels_h3.hpp).  A helper module shared by
tests/test_hess_cpu.py (the f64 oracle, the finite-difference cross-check, the teeth) and tests/test_gpu_hess.py (the device).  No GPU
code; nothing outside the repository is read.

Reference.  Inputs are the doubles the kernel reads: clusters[V,W,10] (Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N), coe[V], the stored
eig_val[V,3], eig_vec[V,9] (row-major, columns = eigenvectors), pcr_add[V,10], poses[W,12] (R row-major | p).  H (6W x 6W), g and r are
evaluated by the literal per-pair formula that oracle/ba_oracle.hpp::LidarFactor::acc_evaluate2 restates (one 6x6 block per occupied
frame and per occupied frame pair, slots with N == 0 skipped, the upper block triangle mirrored), NOT by the kernel's rank-3 identity
G^T C G + E.  The arithmetic is double-double (106 bits; numpy arrays over the voxels of a store) or, for small cases and for the
spot-check of the double-double code, mpmath numbers at any precision: the formula is written once over a value type with + - * /.
Every voxel's term is kept, so any range [head, end) or subset of a store is summed without evaluating again.  The stored eigen-data
is taken as given.

Magnitude shadow.  Every value carries M: the same expression with every input, product and quotient in absolute value and every
subtraction an addition, so no cancellation, inside a term or across voxels, shrinks it.  A divisor counts with its absolute VALUE
(NN, and l0 - l1 of the stored eigenvalues: a shadow of a divisor would shrink the scale instead of keeping it).

Rounding count.  Every value also carries k, the bound of its relative rounding count under the standard model
|fl(x) - x| <= k u M(x) + O(u^2), u = 2^-53:  inputs 0;  a +- b: max(ka, kb) + 1;  a * b and a / b: ka + kb + 1;  a product with an
exact zero (the hat matrices, the identity), a sum with one, a factor of +-2 or 1/2, a negation: no rounding.  d is the largest k of a
finished term (the block times coe), counted by this rule along the oracle's own order of operations.  By hand, for the rot-rot part
of a block:  RiTuk 3;  Ri Pi 3, ti_v = p - v/NN 2, ti_v vi^T 3, their sum 4, times hat(RiTuk) (two non-zeros per column) 4 + 3 + 1 + 1
= 9;  PiRiTuk 6, uk.ti_v 5, vihat (uk.ti_v) 6, combo1 7, Ri combo1 (two non-zeros per column) 7 + 1 + 1 = 9;  Arot 10, /NN 11 = Auk;
2/(l0 - li) 2, u u^T 1, their product 4, summed 5 = umumT;  Auk^T umumT 11 + 5 + 1 + 2 = 19;  times Auk 19 + 11 + 1 + 2 = 33;  plus the
remainder rr 34;  times coe 35.  For g: Auk^T uk 11 + 1 + 2 = 14, times coe 15.  For r: coe * l0, 1.  The count the code keeps is
asserted equal to these constants (tests/test_hess_cpu.py), so a change of the formula cannot leave them behind:
    D_H = 35,   D_G = 15,   D_R = 1.
They are counted, never tuned to a device.

Bars, per entry, over the voxels S of a range or subset:
    |H^ - H*|_ij <= (D_H + n_ij) u M_ij      n_ij = voxels of S that contribute to block (i, j) (both frames occupied)
    |g^ - g*|_i  <= (D_G + n_i)  u M_i       n_i  = voxels of S with frame i occupied
    |r^ - r*|    <= (D_R + |S|)  u sum |coe l0|
(recursive summation, in any order, of terms each within d u M: n - 1 additions of at most u times the running magnitude each).
Nothing is divided by max|H|.  H^ must equal its transpose exactly; an entry with M_ij exactly 0 (no voxel of S sees the frame pair)
must be exactly 0."""
import numpy as np

U = 2.0 ** -53
D_H, D_G, D_R = 35, 15, 1
CLASSES = ("plane", "fixed", "lonely", "neargap", "coe", "fixonly")


# ------------------------------------------------------------------------------------------------ value types
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    t = 134217729.0 * a
    h = t - (t - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class DD:
    """double-double numbers, elementwise over numpy arrays"""
    __slots__ = ("hi", "lo")

    def __init__(self, hi, lo=None):
        self.hi = hi
        self.lo = np.zeros_like(hi) if lo is None else lo

    @staticmethod
    def of(a):
        return DD(np.array(a, dtype=np.float64))

    def __add__(a, b):
        s, e = _two_sum(a.hi, b.hi)
        t, f = _two_sum(a.lo, b.lo)
        s, e = _fast_two_sum(s, e + t)
        return DD(*_fast_two_sum(s, e + f))

    def __neg__(a):
        return DD(-a.hi, -a.lo)

    def __sub__(a, b):
        return a + (-b)

    def __mul__(a, b):
        p, e = _two_prod(a.hi, b.hi)
        return DD(*_fast_two_sum(p, e + (a.hi * b.lo + a.lo * b.hi)))

    def __truediv__(a, b):
        q1 = a.hi / b.hi
        r = a - b * DD(q1)
        q2 = r.hi / b.hi
        r = r - b * DD(q2)
        q3 = r.hi / b.hi
        return DD(*_fast_two_sum(q1, q2)) + DD(q3)

    def times(a, c):
        """by an exact factor: a power of two or a 0 / 1 mask"""
        return DD(a.hi * c, a.lo * c)

    def absf(a):
        return np.abs(a.hi)

    def f64(a):
        return a.hi + a.lo

    def sum_last(a, idx):
        """sum over the chosen indices of the last axis"""
        acc = DD(np.zeros(a.hi.shape[:-1]))
        for v in idx:
            acc = acc + DD(a.hi[..., v], a.lo[..., v])
        return acc

    def err_to(a, x):
        """|x - a| for a double array x"""
        return np.abs((DD(np.asarray(x, dtype=np.float64)) - a).f64())

    @staticmethod
    def stack(items, shape):
        """items: dict index tuple -> DD vector (missing = 0) -> DD of shape + (V,)"""
        V = len(next(iter(items.values())).hi)
        hi = np.zeros(shape + (V,)); lo = np.zeros(shape + (V,))
        for k, x in items.items():
            hi[k] = x.hi; lo[k] = x.lo
        return DD(hi, lo)


class MP:
    """mpmath numbers in numpy object arrays (precision = the caller's mpmath context)"""
    __slots__ = ("a",)

    def __init__(self, a):
        self.a = a

    @staticmethod
    def of(a):
        import mpmath
        return MP(np.array([x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x)) for x in np.asarray(a, dtype=object).ravel()],
                           dtype=object))

    def __add__(a, b):
        return MP(a.a + b.a)

    def __neg__(a):
        return MP(-a.a)

    def __sub__(a, b):
        return MP(a.a - b.a)

    def __mul__(a, b):
        return MP(a.a * b.a)

    def __truediv__(a, b):
        return MP(a.a / b.a)

    def times(a, c):
        import mpmath
        c = np.broadcast_to(np.asarray(c, dtype=np.float64), a.a.shape)
        return MP(a.a * np.array([mpmath.mpf(float(x)) for x in c.ravel()], dtype=object).reshape(c.shape))

    def absf(a):
        return np.array([float(abs(x)) for x in a.a.ravel()]).reshape(a.a.shape)

    def f64(a):
        return np.array([float(x) for x in a.a.ravel()]).reshape(a.a.shape)

    def sum_last(a, idx):
        import mpmath
        out = np.empty(a.a.shape[:-1], dtype=object)
        for k in np.ndindex(*out.shape):
            out[k] = mpmath.fsum(a.a[k][v] for v in idx)
        return MP(out)

    def err_to(a, x):
        import mpmath
        x = np.asarray(x, dtype=np.float64)
        return np.array([float(abs(mpmath.mpf(float(p)) - q)) for p, q in zip(x.ravel(), a.a.ravel())]).reshape(x.shape)

    @staticmethod
    def stack(items, shape):
        import mpmath
        V = len(next(iter(items.values())).a)
        out = np.empty(shape + (V,), dtype=object)
        out[...] = mpmath.mpf(0)
        for k, x in items.items():
            out[k] = x.a
        return MP(out)


# ------------------------------------------------------------------------------------------------ tracked values
class Tr:
    """value v (DD or MP vector over the voxels; None = an exact zero), magnitude shadow m (f64), rounding count k"""
    __slots__ = ("v", "m", "k")

    def __init__(self, v, m, k):
        self.v, self.m, self.k = v, m, k


ZERO = Tr(None, None, 0)


def add(a, b):
    if a.v is None:
        return b
    if b.v is None:
        return a
    return Tr(a.v + b.v, a.m + b.m, max(a.k, b.k) + 1)


def neg(a):
    return a if a.v is None else Tr(-a.v, a.m, a.k)


def sub(a, b):
    if b.v is None:
        return a
    if a.v is None:
        return neg(b)
    return Tr(a.v - b.v, a.m + b.m, max(a.k, b.k) + 1)


def mul(a, b):
    if a.v is None or b.v is None:
        return ZERO
    return Tr(a.v * b.v, a.m * b.m, a.k + b.k + 1)


def div(a, b):
    """b counts with its absolute value (module docstring)"""
    if a.v is None:
        return ZERO
    return Tr(a.v / b.v, a.m / b.v.absf(), a.k + b.k + 1)


def sc(a, c):
    """times an exact +-2^e (or a 0 / 1 mask): no rounding"""
    return a if a.v is None else Tr(a.v.times(c), a.m * np.abs(c), a.k)


def dot(x, y):
    s = ZERO
    for a, b in zip(x, y):
        s = add(s, mul(a, b))
    return s


def matmul(A, B):
    return [[dot(A[r], [B[k][c] for k in range(len(B))]) for c in range(len(B[0]))] for r in range(len(A))]


def matvec(A, x):
    return [dot(row, x) for row in A]


def tr_(A):
    return [[A[r][c] for r in range(len(A))] for c in range(len(A[0]))]


def hat(v):
    return [[ZERO, neg(v[2]), v[1]], [v[2], ZERO, neg(v[0])], [neg(v[1]), v[0], ZERO]]


def outer(x, y):
    return [[mul(a, b) for b in y] for a in x]


def madd(A, B):
    return [[add(a, b) for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def msub(A, B):
    return [[sub(a, b) for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def mscale(A, s):
    return [[mul(a, s) for a in row] for row in A]


def mdiv(A, s):
    return [[div(a, s) for a in row] for row in A]


def add_block(H, r0, c0, B):
    for r in range(len(B)):
        for c in range(len(B[0])):
            H[r0 + r][c0 + c] = add(H[r0 + r][c0 + c], B[r][c])


# ------------------------------------------------------------------------------------------------ the reference
class Ref:
    """Per-voxel terms of H, g, r of one store at one set of poses.  T = DD (default) or MP.  eig_val / eig_vec / pcr_add / poses may be
    given as T values already (the finite-difference check passes eigen-data of its own precision); clusters and coe are doubles."""

    def __init__(self, clusters, coe, eig_val, eig_vec, pcr_add, poses, T=DD):
        clusters = np.asarray(clusters, dtype=np.float64)
        V, W = clusters.shape[:2]
        self.V, self.W, self.T = V, W, T
        self.occ = clusters[:, :, 9] != 0.0

        def inp(a):                                 # one input vector over the voxels
            v = a if isinstance(a, T) else T.of(a)
            return Tr(v, v.absf(), 0)

        def const(x):
            return inp(np.full(V, float(x)))

        def col(a, k):                              # column k of [V, n] doubles or a list of T vectors
            return inp(a[k]) if isinstance(a, (list, tuple)) else inp(np.asarray(a, dtype=np.float64)[:, k])

        coe_t = inp(np.asarray(coe, dtype=np.float64))
        lm = [col(eig_val, k) for k in range(3)]
        Um = [[col(eig_vec, 3 * r + c) for c in range(3)] for r in range(3)]
        NN = col(pcr_add, 9)
        vBar = [div(col(pcr_add, 6 + k), NN) for k in range(3)]
        if isinstance(poses, (list, tuple)):
            pose = [[inp(x) for x in row] for row in poses]
        else:
            pose = [[const(x) for x in row] for row in np.asarray(poses, dtype=np.float64).reshape(W, 12)]
        ONE, TWO = const(1.0), const(2.0)
        I3 = [[ONE if r == c else ZERO for c in range(3)] for r in range(3)]

        u = [[Um[r][c] for r in range(3)] for c in range(3)]            # u[m] = column m
        uk = u[0]
        ukukT = outer(uk, uk)
        umumT = [[ZERO] * 3 for _ in range(3)]
        for m in (1, 2):
            umumT = madd(umumT, mscale(outer(u[m], u[m]), div(TWO, sub(lm[0], lm[m]))))
        inv2NN = div(TWO, NN)                                           # 2.0 / NN
        inv2NN2 = div(inv2NN, NN)                                       # 2.0 / NN / NN

        n6 = 6 * W
        Hd, gd = {}, {}
        Auk, AukT_um, viRiTuk, viRiTukukT, nis = [None] * W, [None] * W, [None] * W, [None] * W, [None] * W
        self.g_slot = np.zeros((V, W, 6))                               # coe * jjt per slot, in f64 (for the teeth)
        for i in range(W):
            if not self.occ[:, i].any():
                continue
            gate = self.occ[:, i].astype(np.float64)
            c = [inp(clusters[:, i, k]) for k in range(10)]
            Pi = [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]
            vi = c[6:9]
            ni = c[9]
            Ri = [pose[i][0:3], pose[i][3:6], pose[i][6:9]]
            pi = pose[i][9:12]
            vihat = hat(vi)
            RiTuk = matvec(tr_(Ri), uk)
            RiTukhat = hat(RiTuk)
            PiRiTuk = matvec(Pi, RiTuk)
            viRiTuk[i] = matvec(vihat, RiTuk)
            viRiTukukT[i] = outer(viRiTuk[i], uk)
            ti_v = [sub(pi[k], vBar[k]) for k in range(3)]
            ukTti_v = dot(uk, ti_v)
            combo1 = madd(hat(PiRiTuk), mscale(vihat, ukTti_v))
            Rivi = matvec(Ri, vi)
            combo2 = [add(Rivi[k], mul(ti_v[k], ni)) for k in range(3)]
            Arot = msub(matmul(madd(matmul(Ri, Pi), outer(ti_v, vi)), RiTukhat), matmul(Ri, combo1))
            Atr = madd(outer(combo2, uk), mscale(I3, dot(combo2, uk)))
            A = mdiv([Arot[r] + Atr[r] for r in range(3)], NN)          # 3 x 6
            Auk[i] = A
            nis[i] = ni
            AT = tr_(A)                                                 # 6 x 3
            jjt = matvec(AT, uk)
            for k in range(6):
                t = sc(mul(jjt[k], coe_t), gate)
                gd[(6 * i + k,)] = t
                self.g_slot[:, i, k] = t.v.f64()
            HRt = mscale(viRiTukukT[i], mul(inv2NN, sub(ONE, div(ni, NN))))
            AukT_um[i] = matmul(AT, umumT)                              # 6 x 3
            Hb = matmul(AukT_um[i], A)
            jr3 = hat(jjt[0:3])
            rr = msub(msub(mscale(matmul(msub(combo1, matmul(RiTukhat, Pi)), RiTukhat), inv2NN),
                           mscale(outer(viRiTuk[i], viRiTuk[i]), inv2NN2)),
                      [[sc(x, 0.5) for x in row] for row in jr3])
            add_block(Hb, 0, 0, rr)
            add_block(Hb, 0, 3, HRt)
            add_block(Hb, 3, 0, tr_(HRt))
            add_block(Hb, 3, 3, mscale(ukukT, mul(inv2NN, sub(ni, div(mul(ni, ni), NN)))))
            for r in range(6):
                for cc in range(6):
                    Hd[(6 * i + r, 6 * i + cc)] = sc(mul(Hb[r][cc], coe_t), gate)
        for i in range(W - 1):
            for j in range(i + 1, W):
                both = self.occ[:, i] & self.occ[:, j]
                if not both.any():
                    continue
                gate = both.astype(np.float64)
                Hb = matmul(AukT_um[i], Auk[j])
                add_block(Hb, 0, 0, mscale(outer(viRiTuk[i], viRiTuk[j]), neg(inv2NN2)))
                add_block(Hb, 0, 3, mscale(viRiTukukT[i], div(div(sc(nis[j], -2.0), NN), NN)))
                add_block(Hb, 3, 0, mscale(tr_(viRiTukukT[j]), div(div(sc(nis[i], -2.0), NN), NN)))
                add_block(Hb, 3, 3, mscale(ukukT, div(div(mul(sc(nis[i], -2.0), nis[j]), NN), NN)))
                for r in range(6):
                    for cc in range(6):
                        t = sc(mul(Hb[r][cc], coe_t), gate)
                        Hd[(6 * i + r, 6 * j + cc)] = t
                        Hd[(6 * j + cc, 6 * i + r)] = t                 # the mirror
        rt = mul(coe_t, lm[0])
        self.dH = max([t.k for t in Hd.values() if t.v is not None], default=0)
        self.dG = max([t.k for t in gd.values() if t.v is not None], default=0)
        self.dR = rt.k
        live = lambda d: {k: t for k, t in d.items() if t.v is not None}
        self.Ht = T.stack({k: t.v for k, t in live(Hd).items()}, (n6, n6)) if live(Hd) else T.stack({(0, 0): coe_t.v.times(0.0)}, (n6, n6))
        self.gt = T.stack({k: t.v for k, t in live(gd).items()}, (n6,)) if live(gd) else T.stack({(0,): coe_t.v.times(0.0)}, (n6,))
        self.HM = np.zeros((n6, n6, V)); self.gM = np.zeros((n6, V))
        for k, t in live(Hd).items():
            self.HM[k] = t.m
        for k, t in live(gd).items():
            self.gM[k] = t.m
        self.rt = T.stack({(0,): rt.v}, (1,))
        self.rM = rt.m

    def sums(self, idx):
        """(H*, g*, r*) as T values and the bars (barH, barG, barR) over the voxels idx"""
        idx = np.asarray(idx, dtype=np.int64)
        W = self.W
        occ = self.occ[idx].astype(np.float64)                          # [n, W]
        nf = occ.sum(0)
        npair = occ.T @ occ                                             # voxels with both frames
        barH = (D_H + np.kron(npair, np.ones((6, 6)))) * U * self.HM[:, :, idx].sum(-1)
        barG = (D_G + np.repeat(nf, 6)) * U * self.gM[:, idx].sum(-1)
        barR = (D_R + len(idx)) * U * float(self.rM[idx].sum())
        return (self.Ht.sum_last(idx), self.gt.sum_last(idx), self.rt.sum_last(idx)), (barH, barG, barR)

    def check(self, H, g, r, idx, sym=True):
        """ratios observed / bar of one result over the voxels idx: dict with H, g, r (largest entry ratio), zero and sym (0 or inf).
        sym=False leaves the exact-symmetry bar out: the oracle forms both halves of a diagonal block, each within the bars."""
        (Hs, gs, rs), (barH, barG, barR) = self.sums(idx)
        H = np.asarray(H, dtype=np.float64); g = np.asarray(g, dtype=np.float64)
        out = {}
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and np.isfinite(r)):
            return {"finite": np.inf}

        def ratio(err, bar, got):
            z = bar == 0.0
            out["zero"] = max(out.get("zero", 0.0), np.inf if np.any(got[z] != 0.0) else 0.0)
            return float((err[~z] / bar[~z]).max()) if np.any(~z) else 0.0

        out["H"] = ratio(Hs.err_to(H), barH, H)
        out["g"] = ratio(gs.err_to(g), barG, g)
        er = float(rs.err_to(np.array([r]))[0])
        out["r"] = (er / barR) if barR > 0.0 else (0.0 if er == 0.0 else np.inf)
        if sym:
            out["sym"] = 0.0 if np.array_equal(H, H.T) else np.inf
        return out


def worst(q):
    return max(q.values()) if q else 0.0


# ------------------------------------------------------------------------------------------------ corpus
def hess2_tv(W):
    """voxels per tile of k_hessian2<W> (csrc/vba_kernels_factor.hpp hess2_tv)"""
    return {2: 128, 3: 80, 4: 64, 5: 48, 6: 40, 7: 32, 8: 32, 9: 24, 10: 24}.get(W, 16)


def cluster(pts):
    P = pts.T @ pts
    v = pts.sum(0)
    return np.array([P[0, 0], P[1, 0], P[2, 0], P[1, 1], P[2, 1], P[2, 2], v[0], v[1], v[2], float(len(pts))])


def transform(c, pose):
    """cluster c under pose [R | p] (the exact-order sums the host pushes: R P R^T + Rv p^T + p (Rv)^T + N p p^T)"""
    R = pose[:9].reshape(3, 3); p = pose[9:]
    P = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
    Rv = R @ c[6:9]
    rp = np.outer(Rv, p)
    Pw = R @ P @ R.T + rp + rp.T + c[9] * np.outer(p, p)
    v = Rv + c[9] * p
    return np.array([Pw[0, 0], Pw[1, 0], Pw[2, 0], Pw[1, 1], Pw[2, 1], Pw[2, 2], v[0], v[1], v[2], c[9]])


def host_eigen(clusters, fix, poses):
    """eig_val, eig_vec (row-major, columns = eigenvectors), pcr_add of every voxel: numpy eigh of the cluster sums"""
    V, W = clusters.shape[:2]
    ev = np.zeros((V, 3)); evec = np.zeros((V, 9)); pa = np.zeros((V, 10))
    for a in range(V):
        s = fix[a].copy()
        for i in range(W):
            if clusters[a, i, 9] != 0.0:
                s = s + transform(clusters[a, i], poses[i])
        c = s[6:9] / s[9]
        P = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]]) / s[9]
        w, Q = np.linalg.eigh(P - np.outer(c, c))
        ev[a] = w; evec[a] = Q.ravel(); pa[a] = s
    return ev, evec, pa


def _rot(rng):
    """a rotation of any angle"""
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))
    return Q if np.linalg.det(Q) > 0 else -Q


def _small_rot(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + K if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _frame(rng):
    n = rng.normal(size=3); n /= np.linalg.norm(n)
    t1 = np.cross(n, rng.normal(size=3)); t1 /= np.linalg.norm(t1)
    return n, t1, np.cross(n, t1)


def _body(q, pose):
    return (q - pose[9:]) @ pose[:9].reshape(3, 3)                      # R^T (q - p)


GAPS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)
_CYCLE = ("plane", "fixed", "lonely", "neargap", "coe", "fixed", "plane", "fixonly")
COE_VALUES = (0.0, 1e-3, 1e3)


def _mask(rng, W, kind):
    m = np.zeros(W, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[W - 1] = True
    elif kind == "two":                         # two non-adjacent frames (W = 2 has none: both)
        a = int(rng.integers(0, max(W - 2, 1)))
        b = int(rng.integers(a + 2, W)) if W > 2 else 1
        m[a] = m[b] = True
    elif kind == "one":
        m[int(rng.integers(0, W))] = True
    else:                                       # random, at least two frames
        m = rng.uniform(size=W) < rng.uniform(0.2, 0.9)
        while m.sum() < min(2, W):
            m[int(rng.integers(0, W))] = True
    return m


def _rod(c0, axis, n1, n2, gap, frames, a_=0.03):
    """World points per frame of a rod along `axis` through c0 with a designed cross-section: the even frames of `frames` see pairs
    at +-a n1, the odd ones pairs at +-b n2, the same number of points in all on either side, so the sums give lambda0 = a^2/2,
    lambda1 = b^2/2 with (lambda1 - lambda0) / lambda1 = gap exactly as designed (the caller keeps the frames consistent with the
    evaluation poses), while every frame alone is as anisotropic in the (u0, u1) plane as can be: the rows Auk^T u1 that
    2 / (lambda0 - lambda1) multiplies are of full size, and H grows with 1 / gap as the Hessian of a nearly double eigenvalue does."""
    b_ = a_ / np.sqrt(1.0 - gap)
    ev, od = frames[0::2], frames[1::2]
    out = []
    for grp, other, d, w in ((ev, od, n1, a_), (od, ev, n2, b_)):
        npos = 3 * max(len(other), 1)                                    # len(ev) * 3 len(od) = len(od) * 3 len(ev) positions a side
        s = (np.arange(npos * len(grp)) - (npos * len(grp) - 1) / 2) * (0.6 / (npos * max(len(grp), 1)))
        for j, i in enumerate(grp):
            sj = s[j::len(grp)]
            out.append((i, np.concatenate([c0 + np.outer(sj, axis) + sg * w * d for sg in (1.0, -1.0)])))
    return out


def corpus(W, seed=20261017, extra_run=0):
    """One seeded store of V = 3 TV(W) + 5 voxels (four tiles of k_hessian2<W>, the last with 5) whose classes cycle so that every tile
    holds a mixture, plus extra_run voxels of one mask (frame 0 and a fixed cluster).  Returns a dict: clusters, fix, coe, eig_val,
    eig_vec, pcr_add (what vba_factor_push_voxels takes), poses [W,12], cls (class name per voxel)."""
    rng = np.random.default_rng(seed + W)
    TV = hess2_tv(W)
    V = 3 * TV + 5 + extra_run
    true = np.zeros((W, 12)); poses = np.zeros((W, 12))
    for i in range(W):
        R = _rot(rng); p = rng.uniform(-3, 3, 3)
        true[i, :9] = R.ravel(); true[i, 9:] = p
        poses[i, :9] = (R @ _small_rot(rng.normal(0, 0.01, 3))).ravel(); poses[i, 9:] = p + rng.normal(0, 0.02, 3)
    clusters = np.zeros((V, W, 10)); fix = np.zeros((V, 10)); coe = rng.uniform(0.5, 2.0, V)
    cls = []
    count = {k: 0 for k in CLASSES}
    for a in range(V):
        kind = _CYCLE[a % len(_CYCLE)] if a < V - extra_run else "run"
        k = count.get(kind, 0)
        if kind in count:
            count[kind] += 1
        n, t1, t2 = _frame(rng)
        c0 = rng.normal(size=3); c0 *= 10.0 ** rng.uniform(0, 2) / np.linalg.norm(c0)     # 1 to 100 m from the origin
        ext = rng.uniform(0.05, 0.5, 2)

        def patch(m):                           # m noisy points of a window of the patch (each frame sees its own part)
            o = rng.uniform(-0.5, 0.5, 2) * ext
            return (c0 + np.outer(o[0] + rng.uniform(-0.5, 0.5, m) * ext[0], t1) + np.outer(o[1] + rng.uniform(-0.5, 0.5, m) * ext[1], t2)
                    + np.outer(rng.normal(0, 0.01, m), n))

        def npts():
            return int(round(10.0 ** rng.uniform(np.log10(6), 4)))                         # 6 to 1e4 points per slot

        if kind in ("plane", "coe"):
            mask = _mask(rng, W, ("all", "two", "random")[k % 3])
        elif kind == "fixed":
            mask = _mask(rng, W, ("all", "first", "last", "two", "random")[k % 5])
        elif kind == "lonely":
            mask = _mask(rng, W, ("first", "last", "one")[k % 3])
        elif kind == "run":
            mask = _mask(rng, W, "first")
        elif kind == "neargap":
            mask = _mask(rng, W, ("all", "random")[k % 2])                          # (at least two frames: one for either side of the rod)
        else:
            mask = np.zeros(W, dtype=bool)
        if kind == "neargap":
            c0 = c0 / np.linalg.norm(c0) * rng.uniform(3, 30)
            for i, q in _rod(c0, n, t1, t2, GAPS[k % len(GAPS)], np.flatnonzero(mask)):
                clusters[a, i] = cluster(_body(q, poses[i]))
        else:
            for i in np.flatnonzero(mask):
                clusters[a, i] = cluster(_body(patch(npts()), true[i]))
        if kind in ("fixed", "fixonly", "run"):
            fix[a] = cluster(patch(npts() if kind != "run" else 8))
        if kind == "coe":
            coe[a] = COE_VALUES[k % 3]
        cls.append(kind)
    ev, evec, pa = host_eigen(clusters, fix, poses)
    return dict(clusters=clusters, fix=fix, coe=coe, eig_val=ev, eig_vec=evec, pcr_add=pa, poses=poses, cls=np.array(cls), W=W, TV=TV,
                true_poses=true)


def origin_store(W, seed=20261018):
    """Ten voxels within 0.3 m of the world origin, seen from poses within centimetres of it (rotations of any angle): nothing in the
    literal formula cancels against metres of lever arm, so the shadow M is within 1e2 of the terms themselves and the bars are at their
    tightest: the store where a relative error of 2^-40 in 2 / (l0 - l1) shows.  Four `plane` patches (each frame sees its own half
    along the shorter side, so the frames pull against each other along u1; voxel 0 is seen by every frame) and six rods (_rod), one
    per gap of GAPS, where 2 / (l0 - l1) is the largest factor of H."""
    rng = np.random.default_rng(seed + W)
    V = 4 + len(GAPS)
    poses = np.zeros((W, 12))
    for i in range(W):
        poses[i, :9] = _rot(rng).ravel(); poses[i, 9:] = rng.normal(0, 0.05, 3)
    clusters = np.zeros((V, W, 10)); fix = np.zeros((V, 10)); coe = rng.uniform(0.5, 2.0, V)
    cls = []
    for a in range(V):
        n, t1, t2 = _frame(rng)
        c0 = rng.uniform(0.0, 0.3) * n
        mask = _mask(rng, W, "all" if a in (0, 4) else "random")
        if a >= 4:
            for i, q in _rod(c0, n, t1, t2, GAPS[a - 4], np.flatnonzero(mask)):
                clusters[a, i] = cluster(_body(q, poses[i]))
            cls.append("rod")
            continue
        for j, i in enumerate(np.flatnonzero(mask)):
            m = int(rng.integers(50, 400))
            sg = -1.0 if j % 2 == 0 else 1.0
            q = c0 + np.outer(rng.uniform(-0.5, 0.5, m), t1) + np.outer(sg * rng.uniform(0, 0.25, m), t2) + np.outer(rng.normal(0, 0.01, m), n)
            clusters[a, i] = cluster(_body(q, poses[i]))
        cls.append("plane")
    ev, evec, pa = host_eigen(clusters, fix, poses)
    return dict(clusters=clusters, fix=fix, coe=coe, eig_val=ev, eig_vec=evec, pcr_add=pa, poses=poses, cls=np.array(cls), W=W,
                TV=hess2_tv(W))


def occupancy_masks(st):
    occ = st["clusters"][:, :, 9] != 0.0
    return (occ * (1 << np.arange(occ.shape[1]))).sum(1).astype(np.int64)


def reorder(st, perm):
    out = dict(st)
    for k in ("clusters", "fix", "coe", "eig_val", "eig_vec", "pcr_add", "cls"):
        out[k] = st[k][perm]
    return out


def order_popcount(st):
    """popcount-descending, equal masks together (what the map's extraction produces)"""
    m = occupancy_masks(st)
    pc = np.array([bin(int(x)).count("1") for x in m])
    return np.lexsort((m, -pc))


def order_shuffled(st, seed=5):
    return np.random.default_rng(seed).permutation(len(st["coe"]))


def ranges(st):
    """the sub-ranges every store is checked on: whole store, [3, V-2), [TV-1, TV+1) (straddles a tile boundary), [TV, 2 TV) (one whole tile)"""
    V, TV = len(st["coe"]), st["TV"]
    return ((0, V), (3, V - 2), (TV - 1, TV + 1), (TV, 2 * TV))


_REFS = {}


def ref_of(st, key):
    """reference of a store (cached per module run under key)"""
    if key not in _REFS:
        _REFS[key] = Ref(st["clusters"], st["coe"], st["eig_val"], st["eig_vec"], st["pcr_add"], st["poses"])
    return _REFS[key]


_STORES = {}


def store(W, extra_run=0):
    if (W, extra_run) not in _STORES:
        _STORES[(W, extra_run)] = corpus(W, extra_run=extra_run)
    return _STORES[(W, extra_run)]
