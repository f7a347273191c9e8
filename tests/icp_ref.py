"""High-precision reference, magnitude shadow, decision margins, accuracy bars and corpus for ONE pass of icp_normal
(loop_refine.hpp:77-134): the 1-NN launch, the gate-and-accumulate launch and the step launch of vba_btc_icp_normal
(k_btc_icp_nn, k_btc_icp_accum, k_btc_icp_step; the arithmetic in csrc/vba_icp_math.hpp).  A helper shared by
tests/test_icp_ref_cpu.py (the g++ build of the shared header, the teeth) and tests/test_gpu_icp_passes.py (the device, through
vba_debug_btc_icp_pass).  No GPU code; nothing outside the repository is read.

1-NN, exact by contract.  The query is float(((R0 x + R1 y) + R2 z) + t) with every operation rounded to double once (numpy's
elementwise operations); the distance is dx dx, += dy dy, += dz dz with every operation rounded to float32; the answer is the lowest
index among the minima, by brute force over the whole target.  key = distance bits << 32 | index, ~0 for an empty target.  Compared
bit for bit.

Value type.  That of tests/hess_ref.py and tests/odom_ref.py: Tr(v, m, k) with v double-double over the points, m the magnitude shadow
and k the counted roundings (inputs 0; a +- b: max + 1; a * b: ka + kb + 1; products and sums with an exact zero, a pose entry that
is exactly 1.0 or 0.0, negations and the factor 1/2: none).  The clouds are floats, so the inputs are exact.  Along the reference's
order, at a general pose:
    pi = R plocal + t        4        ni = R n                3        dv = pi - tpi        5
    rr = tni . dv            8        |ni -+ tni|^2           11       |dv|^2               13
    jac.head = (hat(plocal) R^T) tni  5   (hat(plocal) R^T: two non-zeros per row, 2; times tni 3, 4, 5)      jac.tail = tni  0
    Hess: head x head 11, head x tail 6, tail x tail 1;   JacT: head 14, tail 9;   resi = 0.5 rr rr  17;   match_num 0;   mat_norm 1
(K_PI .. D_* below; tests/test_icp_ref_cpu.py asserts them against the counts the code keeps.)  Counted, never tuned.

Decisions.  The three norms are compared squared, |x|^2 against paras^2 (both in double-double), which decides the same as
sqrt(fl(|x|^2)) < paras up to the roundings of |x|^2 and one of the square root (two more on the square); rr is compared as it is.  A
point is UNCLEAR when any of the four quantities lies within (counted roundings) u (its shadow) of its threshold, u = 2^-53; on
such a point the gate byte under test is taken as given.  The share of unclear points of a corpus class is capped at 2 %
(UNCLEAR_CAP).  The class "threshold" is decided apart: its quantities are exact doubles by construction (exact_gate evaluates them
in rational arithmetic), its pairs sit on a threshold or one float ulp inside it, and every one of its decisions is compared.

Bars on the sums, per entry over the points S that entered a workgroup's partial or the pass's sums:
    |s^ - s*| <= (D + L) u sum_S M        L = 6 (wave) + 2 (waves) for a partial, + nb (partials in workgroup order) for the sums
An entry whose shadow is exactly 0 must be exactly 0; match_num is exact; sums is the host's sum of partial in workgroup order, bit
for bit.  The step is held to the backward and forward bars of tests/solve_ref.py (C = 16, n = 6) on the system of the sums under
test, the pose update to K_ROT / K_TRA counted roundings, the state table exactly (every corpus case keeps both step norms more than
their 8 roundings away from 1e-3, asserted)."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np

import solve_ref as sr
from hess_ref import DD, Tr, ZERO, U, add, dot, mul, neg, sub  # noqa: F401
from odom_ref import cdot, const, inp

NPART = 35
K_PI, K_NI, K_DV, K_RR, K_NORMAL2, K_P2P2, K_JAC = 4, 3, 5, 8, 11, 13, 5
K_SQRT = 2                        # one rounding of the square root, on the square
D_HH, D_HT, D_TT, D_GH, D_GT, D_RESI, D_MATCH, D_MAT = 11, 6, 1, 14, 9, 17, 0, 1
L_PART = 8
UNCLEAR_CAP = 0.02
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)
PARAS1 = (0.2, 0.2, 0.5, 3.0)
PARAS2 = (0.1, 0.1, 0.1, 1.0)
ITER_CAP = 20


def d_vector():
    """the counted D of each of the 35 columns"""
    d = []
    for r in range(6):
        for c in range(r, 6):
            d.append(D_HH if c < 3 else (D_HT if r < 3 else D_TT))
    d += [D_GH] * 3 + [D_GT] * 3 + [D_RESI, D_MATCH] + [D_MAT] * 6
    return np.array(d, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ 1-NN
def query(R, t, src):
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    p = np.asarray(src, np.float32).reshape(-1, 6)[:, 0:3].astype(np.float64)
    return np.stack([(((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r]) for r in range(3)], axis=1).astype(np.float32)


def nn_keys(R, t, src, tar, chunk=1 << 22):
    """key [ns] (uint64) by brute force over the whole target"""
    q = query(R, t, src); ns = len(q)
    c = np.asarray(tar, np.float32).reshape(-1, 6)[:, 0:3]
    nt = len(c)
    if nt == 0:
        return np.full(ns, NOKEY, dtype=np.uint64)
    out = np.empty(ns, dtype=np.uint64)
    step = max(1, chunk // nt)
    for a in range(0, ns, step):
        qq = q[a:a + step]
        d = qq[:, None, 0] - c[None, :, 0]
        dd = d * d
        d = qq[:, None, 1] - c[None, :, 1]
        dd = dd + d * d
        d = qq[:, None, 2] - c[None, :, 2]
        dd = dd + d * d
        assert dd.dtype == np.float32
        idx = dd.argmin(axis=1)                                   # the first of equal minima
        bits = dd[np.arange(len(qq)), idx].view(np.uint32).astype(np.uint64)
        out[a:a + step] = (bits << np.uint64(32)) | idx.astype(np.uint64)
    return out


def key_index(key):
    return (np.asarray(key, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ gates and terms
class PassRef:
    """One pass at (R, t, paras): per point the reference's own 1-NN, the four gate quantities with their margins and the 35 terms
    in double-double with shadows; sums over any subset without evaluating again."""

    def __init__(self, R, t, paras, src, tar, T=DD):
        self.R = np.asarray(R, np.float64).reshape(3, 3); self.t = np.asarray(t, np.float64).reshape(3)
        self.paras = np.asarray(paras, np.float64).reshape(4)
        self.src = np.asarray(src, np.float32).reshape(-1, 6); self.tar = np.asarray(tar, np.float32).reshape(-1, 6)
        self.ns = ns = len(self.src)
        self.nb = max((ns + 255) // 256, 1)
        self.key = nn_keys(self.R, self.t, self.src, self.tar)
        self.has = self.key != NOKEY
        self.counts = {}
        self.hi = np.zeros((NPART, ns)); self.lo = np.zeros((NPART, ns)); self.M = np.zeros((NPART, ns))
        self.accept = np.zeros(ns, dtype=bool); self.unclear = np.zeros(ns, dtype=bool)
        sel = np.nonzero(self.has)[0]
        if len(sel) == 0:
            return
        n = len(sel)
        s = self.src[sel].astype(np.float64); g = self.tar[key_index(self.key[sel])].astype(np.float64)
        Rc = [[const(T, self.R[r, c], n) for c in range(3)] for r in range(3)]
        tc = [const(T, self.t[r], n) for r in range(3)]
        pl = [inp(T, s[:, k]) for k in range(3)]; nl = [inp(T, s[:, 3 + k]) for k in range(3)]
        tp = [inp(T, g[:, k]) for k in range(3)]; tn = [inp(T, g[:, 3 + k]) for k in range(3)]
        pi = [add(cdot(Rc[r], pl), tc[r]) for r in range(3)]
        ni = [cdot(Rc[r], nl) for r in range(3)]
        dv = [sub(pi[r], tp[r]) for r in range(3)]
        rr = dot(tn, dv)
        dinc = [sub(ni[r], tn[r]) for r in range(3)]; dadd = [add(ni[r], tn[r]) for r in range(3)]
        ninc2 = dot(dinc, dinc); nadd2 = dot(dadd, dadd); p2p2 = dot(dv, dv)
        # hat(plocal) R^T, then times tni (Eigen evaluates the product left to right)
        hp = [[ZERO, neg(pl[2]), pl[1]], [pl[2], ZERO, neg(pl[0])], [neg(pl[1]), pl[0], ZERO]]
        HR = [[_cdot_r(hp[r], [Rc[c][k] for k in range(3)]) for c in range(3)] for r in range(3)]
        jac = [dot(HR[r], tn) for r in range(3)] + tn
        terms = []
        for r in range(6):
            for c in range(r, 6):
                terms.append(mul(jac[r], jac[c]))
        gk = [mul(jac[r], rr) for r in range(6)]
        terms += gk
        resi = mul(rr, rr)
        terms.append(Tr(resi.v.times(0.5), resi.m * 0.5, resi.k) if resi.v is not None else ZERO)
        one = Tr(T.of(np.ones(n)), np.ones(n), 0)
        terms.append(one)
        for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            terms.append(mul(tn[a], tn[b]))
        self.counts = dict(pi=_k(pi), ni=_k(ni), dv=_k(dv), rr=rr.k, ninc=ninc2.k, nadd=nadd2.k, p2p=p2p2.k, jac=_k(jac[:3]),
                           terms=[x.k for x in terms])
        for j, x in enumerate(terms):
            if x.v is not None:
                self.hi[j, sel] = x.v.hi; self.lo[j, sel] = x.v.lo; self.M[j, sel] = x.m
        pa = [T.of(np.full(n, p)) for p in self.paras]
        pa2 = [p * p for p in pa]
        zero = T.of(np.zeros(n))

        def below(q, thr, extra=0):
            """(q < thr, |q - thr| within the margin)"""
            v = q.v if q.v is not None else zero
            m = q.m if q.v is not None else np.zeros(n)
            d = (v - thr).f64()
            return d < 0, np.abs(d) <= (q.k + extra) * U * m
        a_inc, u_inc = below(ninc2, pa2[0], K_SQRT)
        a_add, u_add = below(nadd2, pa2[1], K_SQRT)
        a_p2p, u_p2p = below(p2p2, pa2[3], K_SQRT)
        rv = rr.v if rr.v is not None else zero
        rm = rr.m if rr.v is not None else np.zeros(n)
        rabs = np.abs(rv.f64())
        a_rr = (DD(np.where(rv.hi < 0, -rv.hi, rv.hi), np.where(rv.hi < 0, -rv.lo, rv.lo)) - pa[2]).f64() < 0
        u_rr = np.abs(rabs - self.paras[2]) <= rr.k * U * rm
        self.accept[sel] = (a_inc | a_add) & a_rr & a_p2p
        self.unclear[sel] = u_inc | u_add | u_rr | u_p2p
        self.quant = dict(sel=sel, ninc2=ninc2, nadd2=nadd2, p2p2=p2p2, rr=rr)

    def gate(self, given):
        """the gate the sums are formed with: the reference's decision, the byte under test on unclear points"""
        g = self.accept.copy()
        g[self.unclear] = np.asarray(given, bool)[self.unclear]
        return g

    def sum_err(self, gate, idx, dev):
        """(|dev - s*|, sum of the shadows) per column over the accepted points among idx"""
        idx = np.asarray(idx, np.int64)
        idx = idx[np.asarray(gate, bool)[idx]]
        err = np.array([abs(math.fsum(np.concatenate((self.hi[j, idx], self.lo[j, idx], [-float(dev[j])])))) for j in range(NPART)])
        return err, self.M[:, idx].sum(axis=1), len(idx)

    def check_pass(self, out):
        """out: key, gate, partial [nb][35], sums [35] of a pass under test -> dict of findings; ratio <= 1 meets its bar"""
        f = dict(key_equal=bool(np.array_equal(np.asarray(out["key"], np.uint64), self.key)))
        given = np.asarray(out["gate"]).astype(bool)
        clear = ~self.unclear
        f["decisions_equal"] = bool(np.array_equal(given[clear], self.accept[clear]))
        f["unclear"] = int(self.unclear.sum())
        f["gate_without_key"] = bool(np.any(given & ~self.has))
        g = self.gate(given)
        D = d_vector()
        worst, zeros_ok, match_ok = 0.0, True, True
        partial = np.asarray(out["partial"], np.float64).reshape(self.nb, NPART)
        for b in range(self.nb):
            idx = np.arange(b * 256, min((b + 1) * 256, self.ns))
            err, M, cnt = self.sum_err(g, idx, partial[b])
            worst = max(worst, _ratio(err, (D + L_PART) * U * M))
            zeros_ok &= bool(np.all(partial[b][M == 0] == 0.0))
            match_ok &= partial[b][28] == cnt
        f["partial_ratio"] = worst
        sums = np.asarray(out["sums"], np.float64)
        err, M, cnt = self.sum_err(g, np.arange(self.ns), sums)
        f["sums_ratio"] = _ratio(err, (D + L_PART + self.nb) * U * M)
        zeros_ok &= bool(np.all(sums[M == 0] == 0.0))
        match_ok &= sums[28] == cnt
        f["zeros_exact"] = zeros_ok; f["match_exact"] = bool(match_ok)
        acc = np.zeros(NPART)
        for b in range(self.nb):
            acc = acc + partial[b]
        f["sums_is_ordered_sum"] = bool(np.array_equal(acc, sums))
        return f


def _cdot_r(xs, cs):
    """sum of value times pose entry (the pose entry on the right)"""
    return cdot(cs, xs)


def _k(vec):
    return max(x.k for x in vec)


def _ratio(err, bar):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if len(r) else 0.0


def passed(f, need_keys=True):
    return ((f["key_equal"] or not need_keys) and f["decisions_equal"] and not f["gate_without_key"] and f["partial_ratio"] <= 1.0
            and f["sums_ratio"] <= 1.0 and f["zeros_exact"] and f["match_exact"] and f["sums_is_ordered_sum"])


def exact_gate(paras, src, tar, key):
    """the gate at the identity pose in rational arithmetic (class "threshold"): squares of the norms against squares of paras"""
    F = Fraction
    out = np.zeros(len(src), dtype=bool)
    pa = [F(float(p)) for p in paras]
    for i in range(len(src)):
        if key[i] == NOKEY:
            continue
        s = [F(float(v)) for v in src[i]]; g = [F(float(v)) for v in tar[int(key_index(key[i]))]]
        dv = [s[k] - g[k] for k in range(3)]
        ninc2 = sum((s[3 + k] - g[3 + k]) ** 2 for k in range(3)); nadd2 = sum((s[3 + k] + g[3 + k]) ** 2 for k in range(3))
        rr = sum(g[3 + k] * dv[k] for k in range(3)); p2p2 = sum(d * d for d in dv)
        out[i] = (ninc2 < pa[0] ** 2 or nadd2 < pa[1] ** 2) and abs(rr) < pa[2] and p2p2 < pa[3] ** 2
    return out


# ------------------------------------------------------------------------------------------------ the step
def transition(dx, paras, is_conv, done, iters):
    """loop_refine.hpp:69, 121-130 -> (paras, is_conv, done, iters) after the step"""
    paras = tuple(float(p) for p in paras)
    iters += 1
    if np.linalg.norm(dx[0:3]) < 1e-3 and np.linalg.norm(dx[3:6]) < 1e-3:
        if is_conv:
            done = 1
        else:
            paras = PARAS2; is_conv = 1
    if iters >= ITER_CAP:
        done = 1
    return paras, is_conv, done, iters


def transition_clear(dx):
    """the two norms are away from 1e-3 by more than their roundings (4 each)"""
    return all(abs(np.linalg.norm(v) - 1e-3) > 8 * U * 1e-3 for v in (dx[0:3], dx[3:6]))


def system_of(sums):
    H = np.zeros((6, 6)); k = 0
    for r in range(6):
        for c in range(r, 6):
            H[r, c] = H[c, r] = sums[k]; k += 1
    return H, -np.asarray(sums[21:27], np.float64)


K_ROT, K_TRA = 40, 1


def pose_update_ratio(R, t, dx, Rn, tn):
    """R Exp(dx[0:3]) and t + dx[3:6] in mpmath against the values under test.  Counted along Exp (tools.hpp:51-66): the norm 4, the
    axis 5, K K 11, sin and 1 - cos (argument error 4 at |x| <= pi, the function 1, the difference 1) 6, s K + c1 K^2 19, + I 20; the
    product with R 3 x (20 + 1) -> K_ROT = 40 on the shadow |R| (I + |sin| |K| + (1 + |cos|) |K|^2) (the difference 1 - cos counts
    with the sum of its operands, as every subtraction does; a bound, not a tight count);
    t + dx: K_TRA = 1."""
    import mpmath
    with mpmath.workdps(50):
        w = [mpmath.mpf(float(v)) for v in dx[0:3]]
        n = mpmath.sqrt(sum(v * v for v in w))
        E = mpmath.eye(3)
        Es = mpmath.eye(3)
        if float(n) >= 1e-11:
            a = [v / n for v in w]
            K = mpmath.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            Ka = mpmath.matrix(3, 3)
            for i in range(3):
                for j in range(3):
                    Ka[i, j] = abs(K[i, j])
            E = mpmath.eye(3) + mpmath.sin(n) * K + (1 - mpmath.cos(n)) * (K * K)
            Es = mpmath.eye(3) + abs(mpmath.sin(n)) * Ka + (1 + abs(mpmath.cos(n))) * (Ka * Ka)
        Rm = mpmath.matrix(np.asarray(R, np.float64).reshape(3, 3).tolist())
        Ra = mpmath.matrix(np.abs(np.asarray(R, np.float64)).reshape(3, 3).tolist())
        P = Rm * E; S = Ra * Es
        worst = 0.0
        Rn = np.asarray(Rn, np.float64).reshape(3, 3)
        for i in range(3):
            for j in range(3):
                e = abs(mpmath.mpf(float(Rn[i, j])) - P[i, j]); bar = K_ROT * mpmath.mpf(U) * S[i, j]
                worst = max(worst, float(e / bar) if bar > 0 else (0.0 if e == 0 else math.inf))
        for k in range(3):
            e = abs(mpmath.mpf(float(tn[k])) - (mpmath.mpf(float(t[k])) + mpmath.mpf(float(dx[3 + k]))))
            bar = K_TRA * mpmath.mpf(U) * (abs(mpmath.mpf(float(t[k]))) + abs(mpmath.mpf(float(dx[3 + k]))))
            worst = max(worst, float(e / bar) if bar > 0 else (0.0 if e == 0 else math.inf))
    return worst


def check_step(state0, out):
    """state0: dict(R, t, paras, is_conv, done, iters); out: sums, dx and dict state after -> findings"""
    f = {}
    sums = np.asarray(out["sums"], np.float64); dx = np.asarray(out["dx"], np.float64)
    H, b = system_of(sums)
    s1 = out["state"]
    if not np.any(H) and not np.any(b):
        f["dx_ratio"] = 0.0 if np.array_equal(dx, host_ldlt_inplace(H, b), equal_nan=True) else math.inf
    else:
        keep = np.setdiff1d(np.arange(6), sr.zero_rows(H, b))
        with np.errstate(all="ignore"):
            kap = sr.kappa_scaled(H, keep)
        if kap < 1e15:
            bw, fw, zeros_ok = sr.ratios(H, b, dx, kappa=kap)
            f["dx_ratio"] = max(bw, fw); f["dx_zero_rows"] = zeros_ok
        else:
            # rank-deficient beyond its zero rows (fewer than three matched directions): no bar of a stable solver applies; the
            # step is then DEFINED as what the unpivoted-tail LDL^T of the host twin returns, operation for operation
            f["dx_ratio"] = 0.0 if np.array_equal(dx, host_ldlt_inplace(H, b), equal_nan=True) else math.inf
        f["kappa"] = float(kap)
    f["pose_ratio"] = pose_update_ratio(state0["R"], state0["t"], dx, s1["R"], s1["t"]) if np.all(np.isfinite(dx)) else math.inf
    want = transition(dx, state0["paras"], state0["is_conv"], state0["done"], state0["iters"])
    got = (tuple(float(p) for p in s1["paras"]), s1["is_conv"], s1["done"], s1["iters"])
    f["table_clear"] = transition_clear(dx)                    # a corpus property, required: no case may sit on the 1e-3 edge
    f["table_equal"] = want == got
    f["mat_equal"] = bool(np.array_equal(np.asarray(s1["mat"]), sums[29:35]))
    return f


def step_passed(f):
    return (f["dx_ratio"] <= 1.0 and f.get("dx_zero_rows", True) and f["pose_ratio"] <= 1.0 and f["table_clear"] and f["table_equal"]
            and f["mat_equal"])


def eig_ratio(mat6, eig):
    """the eigenvalues of mat_norm against tests/eig3_ref.py's bars (values only)"""
    import eig3_ref as er
    import mpmath
    m = np.asarray(mat6, np.float64)
    ref = er.Ref(np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]]))
    w = np.asarray(eig, np.float64)
    if not np.all(np.isfinite(w)) or not (w[0] <= w[1] <= w[2]):
        return math.inf
    with mpmath.workdps(er.MP_DPS):
        return max(float(abs(mpmath.mpf(float(w[i])) - ref.w_mp[i])) for i in range(3)) / (er.C_BAR * er.EPS * ref.s + er.TINY)


# ------------------------------------------------------------------------------------------------ the g++ build
_LIB = None


class State(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("paras", C.c_double * 4), ("is_conv", C.c_int), ("done", C.c_int),
                ("iters", C.c_int), ("pad", C.c_int), ("mat", C.c_double * 6), ("eig", C.c_double * 3)]


def make_state(R, t, paras=PARAS1, is_conv=0, done=0, iters=0, cls=State):
    s = cls()
    s.R[:] = [float(x) for x in np.reshape(R, 9)]; s.t[:] = [float(x) for x in np.reshape(t, 3)]
    s.paras[:] = [float(x) for x in paras]
    s.is_conv, s.done, s.iters = int(is_conv), int(done), int(iters)
    return s


def state_dict(s):
    return dict(R=np.array(s.R[:]).reshape(3, 3), t=np.array(s.t[:]), paras=np.array(s.paras[:]), is_conv=s.is_conv, done=s.done,
                iters=s.iters, mat=np.array(s.mat[:]), eig=np.array(s.eig[:]))


def host_lib():
    """tests/host/icp_host.cpp built by g++ -O2 -ffp-contract=off over csrc/vba_icp_math.hpp (once per process)"""
    global _LIB
    if _LIB is None:
        import subprocess
        import tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = os.path.join(tempfile.mkdtemp(prefix="icp_host_"), "libicp_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(root, "tests", "host", "icp_host.cpp"),
                               "-o", out])
        _LIB = C.CDLL(out)
        _LIB.icp_host_pass.restype = C.c_int
        _LIB.icp_host_point.restype = C.c_int
    return _LIB


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_ldlt_inplace(H, b):
    A = np.ascontiguousarray(H, np.float64).copy(); bb = np.ascontiguousarray(b, np.float64); x = np.zeros(6)
    host_lib().icp_host_ldlt_inplace(_vp(A), _vp(bb), _vp(x))
    return x


def host_pass(src, tar, state, slices=1):
    """vba_debug_btc_icp_pass's outputs by the g++ build; state: a State (left as given)"""
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 6); tar = np.ascontiguousarray(tar, np.float32).reshape(-1, 6)
    ns, nt = len(src), len(tar); nb = max((ns + 255) // 256, 1)
    st = State.from_buffer_copy(state)
    key = np.zeros(max(ns, 1), np.uint64); gate = np.full(max(ns, 1), 255, np.uint8)
    partial = np.full((nb, NPART), np.nan); sums = np.full(NPART, np.nan); dx = np.full(6, np.nan)
    rc = host_lib().icp_host_pass(ns, _vp(src), nt, _vp(tar), C.byref(st), int(slices), _vp(key), _vp(gate), _vp(partial), _vp(sums), _vp(dx))
    return dict(rc=rc, state=state_dict(st), key=key[:ns], gate=gate[:ns], partial=partial, sums=sums, dx=dx, slices=slices)


def own_slices(ns, nt):
    """the slice count vba_btc_icp_normal takes (restated for the plans of the corpus)"""
    nb = max((ns + 255) // 256, 1); ntile = (nt + 255) // 256
    s = 1
    while s < ntile and nb * s * 2 <= 1024:
        s *= 2
    if s > ntile and ntile > 0:
        s = ntile
    return s


# ------------------------------------------------------------------------------------------------ numpy restatement with teeth
TEETH = ("R_for_RT", "hat_world", "swap_normal_thresholds", "le_ninc", "le_nadd", "le_rr", "le_p2p", "no_half", "tie_high", "dist_double",
         "no_rebase", "rebase_nokey", "drop_last_point", "drop_wave", "drop_last_partial", "switch_and_done", "cap_21")


def restate_keys(R, t, src, tar, slices, tooth=None):
    q = query(R, t, src); ns = len(q)
    c = np.asarray(tar, np.float32).reshape(-1, 6)[:, 0:3]; nt = len(c)
    ntile = (nt + 255) // 256; per = (ntile + slices - 1) // slices
    best = np.full(ns, NOKEY, dtype=np.uint64)
    for sl in range(slices):
        lo = sl * per * 256; hi = min(lo + per * 256, nt)
        k = np.full(ns, NOKEY, dtype=np.uint64)
        if min(lo, nt) < hi and ns:
            cc = c[lo:hi]
            if tooth == "dist_double":
                d = q[:, None, :].astype(np.float64) - cc[None].astype(np.float64)
                dd = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
                idx = dd.argmin(axis=1)
                dd = dd.astype(np.float32)
            else:
                d = q[:, None, :] - cc[None]
                dd = d[..., 0] * d[..., 0]; dd = dd + d[..., 1] * d[..., 1]; dd = dd + d[..., 2] * d[..., 2]
                idx = dd.argmin(axis=1)
                if tooth == "tie_high":
                    idx = (dd.shape[1] - 1) - dd[:, ::-1].argmin(axis=1)
            bits = dd[np.arange(ns), idx].view(np.uint32).astype(np.uint64)
            k = (bits << np.uint64(32)) | idx.astype(np.uint64)
            if tooth != "no_rebase":
                k = k + np.uint64(lo)
        elif tooth == "rebase_nokey":
            k = k + np.uint64(lo)                                # wraps, as the unsigned word does
        best = np.minimum(best, k)
    return best


def restate_pass(state, src, tar, slices=1, tooth=None):
    """one pass in numpy float64 (the oracle's formulas, the kernels' partition into workgroups), with one defect switched on"""
    src = np.asarray(src, np.float32).reshape(-1, 6); tar = np.asarray(tar, np.float32).reshape(-1, 6)
    R = np.asarray(state["R"], np.float64).reshape(3, 3); t = np.asarray(state["t"], np.float64); pa = np.asarray(state["paras"], np.float64)
    ns = len(src); nb = max((ns + 255) // 256, 1)
    with np.errstate(over="ignore"):
        key = restate_keys(R, t, src, tar, slices, tooth)
    has = key != NOKEY
    idx = np.where(has, key_index(key), 0)
    idx = np.where(idx < len(tar), idx, 0)
    T = np.zeros((ns, NPART)); gate = np.zeros(ns, dtype=bool)
    if ns and len(tar):
        p = src[:, 0:3].astype(np.float64); n = src[:, 3:6].astype(np.float64)
        pi = np.stack([(((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r]) for r in range(3)], axis=1)
        ni = np.stack([((R[r, 0] * n[:, 0] + R[r, 1] * n[:, 1]) + R[r, 2] * n[:, 2]) for r in range(3)], axis=1)
        tp = tar[idx, 0:3].astype(np.float64); tn = tar[idx, 3:6].astype(np.float64)
        d = pi - tp
        nrm = lambda v: np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        ninc, nadd, p2p = nrm(ni - tn), nrm(ni + tn), nrm(d)
        rr = (tn[:, 0] * d[:, 0] + tn[:, 1] * d[:, 1]) + tn[:, 2] * d[:, 2]
        lt = lambda a, b, name: (a <= b) if tooth == name else (a < b)
        p0, p1 = (pa[1], pa[0]) if tooth == "swap_normal_thresholds" else (pa[0], pa[1])
        gate = has & (lt(ninc, p0, "le_ninc") | lt(nadd, p1, "le_nadd")) & lt(np.abs(rr), pa[2], "le_rr") & lt(p2p, pa[3], "le_p2p")
        RtN = tn @ (R.T if tooth == "R_for_RT" else R)
        jh = np.cross(pi if tooth == "hat_world" else p, RtN)
        jac = np.concatenate([jh, tn], axis=1)
        k = 0
        for r in range(6):
            for c in range(r, 6):
                T[:, k] = jac[:, r] * jac[:, c]; k += 1
        for r in range(6):
            T[:, 21 + r] = jac[:, r] * rr
        T[:, 27] = (1.0 if tooth == "no_half" else 0.5) * rr * rr
        T[:, 28] = 1.0
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            T[:, 29 + k] = tn[:, a] * tn[:, b]
    T[~gate] = 0.0
    use = gate.copy()
    if tooth == "drop_last_point" and ns % 256:
        use[ns - 1] = False
    if tooth == "drop_wave":
        use[np.arange(ns) % 256 // 64 == 1] = False
    partial = np.zeros((nb, NPART))
    for b in range(nb):
        sl = slice(b * 256, min((b + 1) * 256, ns))
        X = np.zeros((256, NPART)); X[:sl.stop - sl.start] = T[sl] * use[sl][:, None]
        X = X.reshape(4, 64, NPART)
        for h in (32, 16, 8, 4, 2, 1):                           # lane 0 of the xor butterfly
            X = X[:, :h] + X[:, h:2 * h]
        partial[b] = (X[0, 0] + X[1, 0]) + (X[2, 0] + X[3, 0])
    sums = np.zeros(NPART)
    for b in range(nb - 1 if (tooth == "drop_last_partial" and nb > 1) else nb):
        sums = sums + partial[b]
    H, g = system_of(sums)
    dx = host_ldlt_inplace(H, g)
    from btc_oracle import so3_exp
    Rn = R @ so3_exp(dx[0:3]); tn_ = t + dx[3:6]
    paras, is_conv, done, iters = tuple(pa), state["is_conv"], state["done"], state["iters"]
    iters += 1
    if np.linalg.norm(dx[0:3]) < 1e-3 and np.linalg.norm(dx[3:6]) < 1e-3:
        if is_conv:
            done = 1
        else:
            paras = PARAS2; is_conv = 1
            if tooth == "switch_and_done":
                done = 1
    if iters >= (21 if tooth == "cap_21" else ITER_CAP):
        done = 1
    m = sums[29:35]
    eig = np.linalg.eigvalsh(np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])) if done else np.zeros(3)
    st = dict(R=Rn, t=tn_, paras=np.array(paras), is_conv=is_conv, done=done, iters=iters, mat=m.copy(), eig=eig)
    return dict(state=st, key=key, gate=gate.astype(np.uint8), partial=partial, sums=sums, dx=dx, slices=slices)


# ------------------------------------------------------------------------------------------------ corpus
SIZES = (1, 63, 64, 65, 255, 256, 257, 700)


def _so3(w):
    from btc_oracle import so3_exp
    return so3_exp(np.asarray(w, np.float64))


def plane_cloud(n, seed):
    """voxel_slam_amd.synth.btc_plane_cloud restated (five planes, 5 mm noise): the corpus must not need the package"""
    rng = np.random.default_rng(seed)
    normals = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [0.6, 0.8, 0], [0, 0.6, 0.8]], dtype=np.float64)
    ds = np.array([0.0, 8.0, -6.0, 4.0, 3.0])
    k = rng.integers(0, 5, n)
    nrm = normals[k]
    u = np.cross(nrm, [0.3, 0.5, 0.81]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(nrm, u)
    a, b = rng.uniform(-10, 10, (2, n))
    pts = nrm * ds[k][:, None] + a[:, None] * u + b[:, None] * v + rng.normal(0, 0.005, (n, 3))
    return np.column_stack([pts, nrm]).astype(np.float32)


RT_OFFSET = ([0.02, -0.03, 0.05], [0.3, -0.2, 0.1])        # the scene of tests/test_gpu_btc.py::test_icp_matches_oracle


def scene_pair(ns, nt, Rt, tt, seed=1):
    """(src, tar): tar = the first nt points of a plane cloud, src = its first ns points moved by (Rt, tt)^-1 (tar = Rt src + tt)"""
    full = plane_cloud(max(ns, nt, 1), seed)
    tar = full[:nt]
    src = full[:ns].copy()
    if not (np.array_equal(Rt, np.eye(3)) and not np.any(tt)):
        src[:, 0:3] = ((full[:ns, 0:3].astype(np.float64) - tt) @ Rt).astype(np.float32)
        src[:, 3:6] = (full[:ns, 3:6].astype(np.float64) @ Rt).astype(np.float32)
    return src, tar


def scene_poses():
    """name -> (Rt, tt, R, t, paras, is_conv): the scene's own placement (Rt, tt) and the pose the pass starts from.  identity: the
    clouds coincide; offset: the existing scene from the identity; oblique: 0.5 rad about an oblique axis from the identity;
    first_set: a few mrad and mm off the solution, where the first parameter set still holds; converged: at the solution under the
    second parameter set"""
    Rt = _so3(RT_OFFSET[0]); tt = np.array(RT_OFFSET[1])
    ax = np.array([1.0, 2.0, -2.0]) / 3.0
    I, z = np.eye(3), np.zeros(3)
    return dict(identity=(I, z, I, z, PARAS1, 0),
                offset=(Rt, tt, I, z, PARAS1, 0),
                oblique=(_so3(0.5 * ax), np.array([0.1, 0.2, -0.1]), I, z, PARAS1, 0),
                first_set=(Rt, tt, Rt @ _so3([2e-3, -1e-3, 1.5e-3]), tt + np.array([4e-3, -3e-3, 2e-3]), PARAS1, 0),
                converged=(Rt, tt, Rt @ _so3([1e-5, 2e-5, -1e-5]), tt + np.array([1e-5, -2e-5, 1e-5]), PARAS2, 1))


def _case(name, src, tar, R, t, paras=PARAS1, is_conv=0, done=0, iters=0, slices=(0,), exact=None):
    return dict(name=name, src=np.ascontiguousarray(src, np.float32).reshape(-1, 6), tar=np.ascontiguousarray(tar, np.float32).reshape(-1, 6),
                R=np.asarray(R, np.float64).reshape(3, 3), t=np.asarray(t, np.float64).reshape(3), paras=tuple(float(p) for p in paras),
                is_conv=is_conv, done=done, iters=iters, slices=tuple(slices), exact=exact)


CLASSES = ("scene", "slices", "ties", "threshold", "state", "degenerate")
_CASES = {}


def cases(cls):
    """the corpus of one class: a list of cases (name, src, tar, the state the pass starts from, the slice counts to run; 0 = the
    call's own).  Built once per process."""
    if cls in _CASES:
        return _CASES[cls]
    out = []
    P = scene_poses()
    if cls == "scene":
        names = list(P); k = 0
        sizes = [(a, b) for a in SIZES for b in SIZES] + [(0, 257), (257, 0), (0, 0)]
        for ns, nt in sizes:
            Rt, tt, R, t, pa, ic = P[names[k % 5]]
            src, tar = scene_pair(ns, nt, Rt, tt)
            out.append(_case("scene_%s_%d_%d" % (names[k % 5], ns, nt), src, tar, R, t, pa, ic)); k += 1
        for nm in names:                                           # every pose at the largest size too
            Rt, tt, R, t, pa, ic = P[nm]
            src, tar = scene_pair(700, 700, Rt, tt)
            out.append(_case("scene_%s_full" % nm, src, tar, R, t, pa, ic))
    elif cls == "slices":
        Rt, tt, R, t, pa, ic = P["first_set"]
        src, tar = scene_pair(700, 2200, Rt, tt)
        out.append(_case("slices_700_2200", src, tar, R, t, pa, ic, slices=(1, 2, 4, 8, 9)))
        src, tar = scene_pair(17000, 2200, Rt, tt)
        out.append(_case("slices_17000_2200", src, tar, R, t, pa, ic, slices=(0,)))
        src, tar = scene_pair(200, 2200, Rt, tt)
        out.append(_case("slices_200_2200", src, tar, R, t, pa, ic, slices=(0, 1)))
    elif cls == "ties":
        src, tar = ties_cloud()
        out.append(_case("ties_near", src, tar, np.eye(3), np.zeros(3), slices=(0, 1, 3)))
        src, tar = ties_cloud(far=1000.0)
        out.append(_case("ties_far", src, tar, np.eye(3), np.array([1e-5, 0.0, 0.0]), slices=(0, 1, 3)))
    elif cls == "threshold":
        for k, pa in enumerate(THRESHOLD_PARAS):
            src, tar, want = threshold_pairs(pa)
            out.append(_case("threshold_%d" % k, src, tar, np.eye(3), np.zeros(3), pa, exact=want))
    elif cls == "state":
        Rt, tt = P["offset"][0:2]
        src, tar = scene_pair(700, 700, Rt, tt)
        for nm, (wr, wt) in dict(small=(1e-5, 1e-5), rot=(2e-3, 1e-5), tra=(1e-5, 2e-3), both=(2e-3, 2e-3)).items():
            R = Rt @ _so3(np.array([0.6, -0.48, 0.64]) * wr); t = tt + np.array([0.48, 0.64, -0.6]) * wt
            for ic in (0, 1):
                out.append(_case("state_%s_conv%d" % (nm, ic), src, tar, R, t, PARAS2 if ic else PARAS1, ic))
            if nm in ("small", "both"):
                out.append(_case("state_%s_iters19" % nm, src, tar, R, t, PARAS1, 0, 0, 19))
        out.append(_case("state_done", src, tar, Rt, tt, PARAS2, 1, 1, 7))
    elif cls == "degenerate":
        for nm, (src, tar) in degenerate_clouds().items():
            out.append(_case("degenerate_%s" % nm, src, tar, np.eye(3), np.zeros(3)))
        # the same parallel normals on the twentieth pass: `done` is set in this pass, so the eigenvalues of mat_norm = diag(0, 0, n),
        # which the direct solver declines, come from the Jacobi fallback and meet eig3_ref's bar here
        src, tar = degenerate_clouds()["parallel"]
        out.append(_case("degenerate_parallel_iters19", src, tar, np.eye(3), np.zeros(3), iters=19))
    else:
        raise KeyError(cls)
    _CASES[cls] = out
    return out


def start_state(case, cls=State):
    return make_state(case["R"], case["t"], case["paras"], case["is_conv"], case["done"], case["iters"], cls)


_REFS = {}


def ref_of(case):
    if case["name"] not in _REFS:
        _REFS[case["name"]] = PassRef(case["R"], case["t"], case["paras"], case["src"], case["tar"])
    return _REFS[case["name"]]


def check_case(case, out, slices):
    """every finding of one pass under test on one case: (pass findings, step findings, ok)"""
    ref = ref_of(case)
    if case["done"]:
        return {}, {}, True
    f = ref.check_pass(out)
    ok = passed(f)
    if case["exact"] is not None:
        f["exact_equal"] = bool(np.array_equal(np.asarray(out["gate"]).astype(bool), case["exact"]))
        f["exact_is_rational"] = bool(np.array_equal(exact_gate(case["paras"], case["src"], case["tar"], ref.key), case["exact"]))
        ok = ok and f["exact_equal"] and f["exact_is_rational"]
    s0 = dict(R=case["R"], t=case["t"], paras=case["paras"], is_conv=case["is_conv"], done=case["done"], iters=case["iters"])
    g = check_step(s0, out)
    ok = ok and step_passed(g)
    s1 = out["state"]
    if s1["done"] and "eig_ratio" not in g and out.get("rc", 0) != 2:
        g["eig_ratio"] = eig_ratio(s1["mat"], s1["eig"])
        ok = ok and g["eig_ratio"] <= 1.0
    elif not s1["done"]:
        g["eig_untouched"] = bool(np.array_equal(s1["eig"], np.zeros(3)))
        ok = ok and g["eig_untouched"]
    return f, g, ok


def worst_ratios(f, g):
    return {k: v for k, v in list(f.items()) + list(g.items()) if k.endswith("_ratio")}


COINCIDENT = (200, 201, 300, 520, 800, 1000, 1030, 1300, 1540, 1600, 1800, 1831)     # twelve indices over six tiles and three slices


def ties_cloud(per=3, far=0.0):
    """a target on a 2^-3 m lattice whose points repeat at index distances 1, 256 and per * 256, twelve coincident points, and queries
    on lattice points, midway between two and midway between four; far: an offset of the whole scene along x"""
    g = np.arange(8) * 0.125
    base = np.array([[x, y, 0.0] for x in g for y in g], dtype=np.float64)       # 64 lattice points
    nt = (2 * per + 1) * 256 + 40
    pts = np.zeros((nt, 3)); pts[:] = [50.0, 50.0, 50.0]                        # filler far from every query
    pts += (np.arange(nt) % 97)[:, None] * np.array([0.25, 0.0, 0.0])
    for j, b in enumerate(base[:40]):
        pts[3 * j] = b; pts[3 * j + 1] = b                                       # index distance 1
    for j, b in enumerate(base[40:52]):
        pts[130 + j] = b; pts[130 + j + 256] = b                                 # next tile
    for j, b in enumerate(base[52:64]):
        pts[150 + j] = b; pts[150 + j + per * 256] = b                           # next slice
    co = np.array([2.0, 2.0, 0.0])
    assert per == 3 and nt == 1832
    for j in COINCIDENT:
        pts[j] = co
    pts[:, 0] += far
    nrm = np.tile([0.0, 0.0, 1.0], (nt, 1))
    tar = np.column_stack([pts, nrm]).astype(np.float32)
    q = [b for b in base] + [b + [0.0625, 0, 0] for b in base[:48]] + [b + [0.0625, 0.0625, 0] for b in base[:48]] + [co, co + [0.01, 0, 0]]
    q = np.array(q, dtype=np.float64); q[:, 0] += far
    q[:, 2] += 0.03125
    src = np.column_stack([q, np.tile([0.0, 0.0, 1.0], (len(q), 1))]).astype(np.float32)
    return src, tar


def _f32_below(x):
    """the largest float32 below x, the smallest float32 not below x"""
    f = np.float32(x)
    if float(f) >= x:
        return np.nextafter(f, np.float32(-np.inf)), f
    return f, np.nextafter(f, np.float32(np.inf))


def threshold_pairs(paras):
    """isolated source / target pairs 16 m apart at the identity pose, target normals (1, 0, 0), coordinates on a 2^-10 grid but for
    the one float that carries the tested difference; every gate quantity is an exact double.  Per gate one pair on the threshold
    (the smallest float not below it: rejected) and one the float below (accepted); the other gates hold well inside.  Plus a pair that passes by
    ninc only and one by nadd only.  Returns (src, tar, expected gate)."""
    pa = [float(p) for p in paras]
    src, tar, want = [], [], []

    def pair(dn, sign, dpx, dpy, ok):
        """source normal = sign * (1, 0, 0) + (0, dn, 0); source point = target point + (dpx, dpy, 0)"""
        k = len(src)
        base = np.array([0.0, 0.0, 16.0 * (k + 1) + 2.0 ** -10 * k])           # the tested axes start at 0: base + v is the float v
        tar.append(np.concatenate([base, [1.0, 0.0, 0.0]]))
        src.append(np.concatenate([base + [dpx, dpy, 0.0], [sign * 1.0, dn, 0.0]]))
        want.append(ok)
    small = 2.0 ** -6
    for gate in range(4):
        lo, hi = _f32_below(pa[gate])
        for val, ok in ((hi, False), (lo, True)):
            v = float(val)
            if gate == 0:
                pair(v, 1.0, 0.0, small, ok)             # ninc = v, nadd > 2
            elif gate == 1:
                pair(v, -1.0, 0.0, small, ok)            # nadd = v, ninc > 2
            elif gate == 2:
                pair(0.0, 1.0, v, 0.0, ok)               # rr = v = p2p (p2p's threshold is the larger)
            else:
                pair(0.0, 1.0, 0.0, v, ok)               # rr = 0, p2p = v
    mid = lambda a, b: float(np.float32(0.5 * (a + b)))
    if pa[0] != pa[1]:
        m = mid(pa[0], pa[1])                            # between the two normal thresholds
        pair(m, 1.0, 0.0, small, pa[0] > m)              # ninc = m: passes only where paras[0] is the larger
        pair(m, -1.0, 0.0, small, pa[1] > m)             # nadd = m
    pair(float(_f32_below(pa[0])[0]), 1.0, 0.0, small, True)     # by ninc only
    pair(float(_f32_below(pa[1])[0]), -1.0, 0.0, small, True)    # by nadd only
    s = np.array(src).astype(np.float32); t = np.array(tar).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), np.array(src)) and np.array_equal(t.astype(np.float64), np.array(tar))
    return s, t, np.array(want, dtype=bool)


THRESHOLD_PARAS = ((0.125, 0.25, 0.5, 2.0), (0.25, 0.125, 0.5, 2.0), PARAS1, PARAS2)


def degenerate_clouds():
    """name -> (src, tar): all target normals parallel; every point gated out; one lone match in a tail workgroup"""
    rng = np.random.default_rng(20261020)
    n = 300
    xy = rng.uniform(-5, 5, (n, 2))
    flat = np.column_stack([xy, rng.normal(0, 0.005, n), np.zeros((n, 2)), np.ones(n)]).astype(np.float32)
    src_flat = flat.copy(); src_flat[:, 0] += np.float32(0.01); src_flat[:, 2] += np.float32(0.02)
    far = flat.copy(); far[:, 0:3] += np.float32(40.0)
    lone_src = far.copy(); lone_src[299, 0:3] = flat[7, 0:3] + np.float32(0.01)
    return dict(parallel=(src_flat, flat), gated_out=(far, flat), lone=(lone_src, flat))
