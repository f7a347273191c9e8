"""High-precision reference, magnitude shadow, decision margins and accuracy bars for ONE point loop of the two resident odometry
updates: the scan-to-map loop on the voxel map (odom_match_body, csrc/vba_kernels_map.hpp) and the loop on a point-cloud map
(kd_match_body, kd_fit_body, kd_accum_body, csrc/vba_kernels_kd.hpp), with the fixed-order reduction of their workgroup partials
(odom_sum_partials, csrc/vba_kernels_odom.hpp).  A helper shared by tests/test_odom_sums_cpu.py (f64 restatements, caps, teeth) and
tests/test_gpu_odom_sums.py (the device, through vba_debug_odom_sums).  No GPU code; nothing outside the repository is read.

Value type.  That of tests/hess_ref.py: a value is Tr(v, m, k) with v a double-double (or mpmath) vector over the points, m the magnitude
shadow (the same expression with every input, product and quotient in absolute value and every subtraction an addition) and k the counted
relative roundings under |fl(x) - x| <= k u m, u = 2^-53: inputs 0; a +- b: max + 1; a * b: ka + kb + 1; products and sums with an
exact zero, negations: none.  Two rules are added here.  A factor that is exactly 1.0 or 0.0 in a pose (the identity pose) is an exact
one / zero: no rounding.  A quotient a / b counts ka + kb + 1 on the shadow ma mb / b^2: the divisor 0.0005 + sigma_l carries roundings of
its own, and mb / |b| >= 1 is their amplification (hess_ref divides by stored data only and needs no such factor).

Voxel path.  The plane data (centre, normal, radius, plane_var of every leaf; key, layer and path of the leaves) are the map's own dump
and are taken as given; voxel centres follow from key, path and the voxel size by the reference's formula (exact for a binary voxel
size).  Per point the reference evaluates, by the literal formulas of oracle/map_oracle.hpp::lio_state_estimation / match:
  w = R b + t                                   k 4   (products 1, three additions)
  root key: float(w / vs), -1 if negative, truncation; out of range beyond +-2^20; descent by w > centre per axis
  d = w - c  5;  resi = n . d  8;  dd = d . d  13
  range gate   dd - resi^2 <= 9 float(radius)   in float: the conversions of |resi| and dd (1 each), the square (3), the difference (4);
                                                the right side one float product
  var_world = (R var) R^T + (hat(b) rot_var) hat(b)^T + tsl_var     R var 3, (R var) R^T 6, hat(b) rot_var 2, times hat(b)^T 4, sum 7, 8
  sigma_l = J plane_var J^T + n^T var_world n,  J = [d, -n]         plane_var J 11, times J 17, summed 22; var_world n 11, n . 14; sum 25
  sigma gate   float(|resi|) < 3 sqrt(sigma_l)
  R_inv = 1 / (0.0005 + sigma_l)  27;   jac = [b x (R^T n); n]      R^T n 3, cross product 5
  HTH = (R_inv jac_r) jac_c  39;  HTz = -(R_inv jac_r) resi  42;  nnt = n_r n_c  1;  match_num  0
so D_HTH = 39, D_HTZ = 42, D_NNT = 1 at a general pose; the code's own count is asserted equal to these (tests/test_odom_sums_cpu.py).
Margins: a decision is UNCLEAR when the compared quantity lies within (counted roundings) x (2^-24 for a float temporary, 2^-53
otherwise) x (its shadow) of the threshold: every voxel face (float(w / vs) against the integers: one float rounding of |w / vs| plus the
5 roundings of w / vs), every octant plane of the descent (4 roundings of w), the range gate (4 + 1 float roundings on dd + resi^2 +
9 radius, plus the double roundings of dd - resi^2), the sigma gate (one float rounding of |resi|, the 8 of resi, and 3 d(sqrt) of
sigma_l: (25 u M_sigma) / (2 sqrt(sigma_l)) + 2 u sqrt(sigma_l)).  `<` against a margin is strict, so a comparison of exact zeros with
zero shadows is clear.

kd path.  The selection is a discrete function, defined exactly: float32 query q = float(R b + t) and map points, distance
((dx dx) + dy dy) + dz dz with dx = q - p and every operation rounded to float32, strict `<` with the earlier index winning a tie (the
order of the words distance bits << 32 | index), five per slice with the kernel's slice bounds, then merged.  kd_candidates restates it
in numpy float32; kd_dist_exact evaluates one distance in exact rational arithmetic, rounding where the unfused or the fused (one
rounding per multiply-add) evaluation rounds.  The plane fit is the least-squares solution of the 5 x 3 problem A x = -1 in
double-double (normal equations: 106 bits against kappa^2 <= 1e12).  Its bar is the first-order perturbation bound of the problem,
    |x^ - x|_2 <= 100 * 5 u * (kappa |x|_2 + kappa^2 |r|_2 / |A|_2)        (kappa, r of the reference; 100 = the unmodelled constant)
carried to (n, d) = (x / |x|, 1 / |x|): |n^ - n| <= 2 bar / |x| + 4 u, |d^ - d| <= d (bar / |x| + 3 u).  The 0.1 gate on |x . a_k + 1|
gets the margin |a_k|_2 bar + 5 u (|x| . |a_k| + 1); a point with any of its five inside it is unclear.  The 28 sums are evaluated from
the device's own planes, taken as given:  w 4;  pd2 = n . w + d  8;  R^T n 3, cross product 5;  HTH = jac_r jac_c  11;  HTz = -pd2 jac_r  14:
D_KD_HTH = 11, D_KD_HTZ = 14.

Bars on sums, per entry over the matched points S of a workgroup or a scan:  |s^ - s*| <= (D + |S|) u sum_S M  (any summation order of
terms each within D u M).  An entry whose shadow is exactly 0 must be exactly 0; the match count must be exact.  Nothing here is tuned
to a device."""
from fractions import Fraction

import numpy as np

from hess_ref import DD, MP, Tr, ZERO, U, add, dot, mul, neg, sub  # noqa: F401

UF = 2.0 ** -24
KEY_OFF = 1 << 20
D_HTH, D_HTZ, D_NNT = 39, 42, 1
D_KD_HTH, D_KD_HTZ = 11, 14
K_W, K_RESI, K_SIGMA = 4, 8, 25
REASONS = ("match", "no_root", "key_range", "no_plane", "untouched", "range_gate", "sigma_gate")
MATCH, NO_ROOT, KEY_RANGE, NO_PLANE, UNTOUCHED, RANGE_GATE, SIGMA_GATE = range(7)
RED_LANES = 7 * 34
UNFILLED = np.uint64((int(np.float32(3.4e38).view(np.uint32)) << 32) | 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ tracked values over the points
def divs(a, b):
    """a / b with the divisor's own roundings amplified by mb / |b| (module docstring)"""
    if a.v is None:
        return ZERO
    bb = b.v.absf()
    return Tr(a.v / b.v, a.m * b.m / (bb * bb), a.k + b.k + 1)


def const(T, x, n):
    """a pose entry: exact zero, or an input broadcast over the n points"""
    return ZERO if x == 0.0 else Tr(T.of(np.full(n, float(x))), np.full(n, abs(float(x))), 0)


def inp(T, a):
    a = np.asarray(a, dtype=np.float64)
    return Tr(T.of(a), np.abs(a), 0)


def cmul(c, x):
    """pose entry times a value: an exact 1.0 or 0.0 does not round"""
    if c.v is None or x.v is None:
        return ZERO
    if np.all(c.m == 1.0):
        return x if np.all(c.v.f64() == 1.0) else neg(x)
    return mul(c, x)


def cdot(cs, xs):
    s = ZERO
    for c, x in zip(cs, xs):
        s = add(s, cmul(c, x))
    return s


def f64(a, n):
    return np.zeros(n) if a.v is None else a.v.f64()


def shadow(a, n):
    return np.zeros(n) if a.v is None else a.m


# ------------------------------------------------------------------------------------------------ the voxel map as dumped
class LeafMap:
    """Leaves [L][39] (vba_map_dump_leaves rows) and plane_var [L][36] in the same order; voxel centres by the reference's formula."""

    def __init__(self, leaves, plane_var, voxel_size, max_layer):
        self.vs, self.max_layer = float(voxel_size), int(max_layer)
        self.leaves, self.pv = np.asarray(leaves), np.asarray(plane_var)
        assert len(self.leaves) == len(self.pv)
        self.leaf, self.internal = {}, set()
        for i, o in enumerate(self.leaves):
            k = (int(o[0]), int(o[1]), int(o[2])); L = int(o[3]); p = int(o[4])
            assert (k, L, p) not in self.leaf
            self.leaf[(k, L, p)] = i
            q = p
            for l in range(L - 1, -1, -1):
                q >>= 3
                self.internal.add((k, l, q))
        self.roots = {k for (k, L, p) in self.leaf} | {k for (k, L, p) in self.internal}

    @staticmethod
    def from_device(leaves39, pv86, voxel_size, max_layer):
        """match the rows of the two device dumps by (key, layer, path)"""
        idx = {tuple(r[:5].astype(np.int64)): i for i, r in enumerate(pv86)}
        order = [idx[tuple(r[:5].astype(np.int64))] for r in leaves39]
        return LeafMap(leaves39, pv86[order, 5:41], voxel_size, max_layer)

    def centre(self, k, L, p):
        """centre and half length of node (key, layer, path): (0.5 + k) vs, then +- the quarter length (a float) per level"""
        c = (0.5 + np.array(k, dtype=np.float64)) * self.vs
        ql = np.float32(self.vs / 4)
        for l in range(1, L + 1):
            o = (p >> (3 * (L - l))) & 7
            c = c + (2.0 * np.array([(o >> 2) & 1, (o >> 1) & 1, o & 1]) - 1.0) * float(ql)
            ql = np.float32(ql / np.float32(2))
        return c, 2.0 * float(ql)

    def keys(self, w):
        loc = (w / self.vs).astype(np.float32)
        return np.where(loc < 0, loc - np.float32(1.0), loc).astype(np.float32).astype(np.int64)

    def descend(self, w, M_w, le=False):
        """w [N][3] (f64 of the reference's value), its shadow -> (leaf row or -1, reason, slack).  slack: the smallest |distance to a
        threshold| / margin over the faces and octant planes the point was compared with (inf: margin 0 and distance 0 included, a
        comparison of exact zeros); < 1 is unclear."""
        N = len(w)
        leaf = np.full(N, -1); reason = np.full(N, NO_ROOT)
        loc = w / self.vs
        slack = _ratio(np.abs(loc - np.rint(loc)), (K_W + 1) * U * M_w / self.vs + UF * np.abs(loc)).min(axis=1)
        key = self.keys(w)
        for i in range(N):
            k = tuple(int(x) for x in key[i])
            if min(k) < -KEY_OFF or max(k) >= KEY_OFF:
                reason[i] = KEY_RANGE
                continue
            if k not in self.roots:
                continue
            L, p = 0, 0
            while True:
                if (k, L, p) in self.leaf:
                    r = self.leaf[(k, L, p)]
                    leaf[i] = r
                    reason[i] = MATCH if self.leaves[r, 7] != 0 else NO_PLANE
                    break
                if (k, L, p) not in self.internal:
                    reason[i] = UNTOUCHED
                    break
                c, _ = self.centre(k, L, p)
                slack[i] = min(slack[i], _ratio(np.abs(w[i] - c), K_W * U * M_w[i]).min())
                o = 4 * int(w[i, 0] > c[0]) + 2 * int(w[i, 1] > c[1]) + int(w[i, 2] > c[2])
                L, p = L + 1, (p * 8 + o if L > 0 else o)
        return leaf, reason, slack


def _ratio(dist, margin):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(margin > 0, dist / np.where(margin > 0, margin, 1.0), np.inf)


# ------------------------------------------------------------------------------------------------ the voxel reference
class Pose:
    def __init__(self, state25, cov225):
        s = np.asarray(state25, dtype=np.float64); P = np.asarray(cov225, dtype=np.float64).reshape(15, 15)
        self.R = s[1:10].reshape(3, 3).copy(); self.t = s[10:13].copy()
        self.rot_var = P[0:3, 0:3].copy(); self.tsl_var = P[3:6, 3:6].copy()


def world(T, pose, b):
    """w = R b + t as tracked values, b = list of 3 inputs"""
    n = len(b[0].m)
    R = [[const(T, pose.R[r, c], n) for c in range(3)] for r in range(3)]
    return [add(cdot(R[r], b), const(T, pose.t[r], n)) for r in range(3)], R


class VoxelRef:
    """Per-point terms [34] of one point loop, decisions and margins.  T = DD (default) or MP."""

    def __init__(self, lm, pose, pts, var, T=DD):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3); var = np.asarray(var, dtype=np.float64).reshape(-1, 9)
        N = self.N = len(pts)
        b = [inp(T, pts[:, k]) for k in range(3)]
        w, R = world(T, pose, b)
        wf = np.stack([f64(x, N) for x in w], axis=1); Mw = np.stack([shadow(x, N) for x in w], axis=1)
        self.k_w = max(x.k for x in w)
        self.leaf, self.reason, slack = lm.descend(wf, Mw)
        self.layer = np.where(self.leaf >= 0, lm.leaves[np.maximum(self.leaf, 0), 3], -1).astype(int)
        has = self.reason == MATCH                                   # a leaf with a plane: the gates decide
        row = np.maximum(self.leaf, 0)
        L = lm.leaves[row]; L = np.where(has[:, None], L, 0.0); PV = np.where(has[:, None], lm.pv[row], 0.0)
        c = [inp(T, L[:, 32 + k]) for k in range(3)]; nv = [inp(T, L[:, 35 + k]) for k in range(3)]
        r32 = L[:, 38].astype(np.float32).astype(np.float64)
        d = [sub(w[k], c[k]) for k in range(3)]
        resi = dot(nv, d); dd = dot(d, d)
        self.k_resi, self.k_dd = resi.k, dd.k
        lhs = sub(dd, mul(resi, resi))
        lf, rf = f64(lhs, N), 9.0 * r32
        m_range = UF * (4 * (shadow(dd, N) + shadow(resi, N) ** 2) + rf) + U * lhs.k * shadow(lhs, N)
        range_ok = lf <= rf
        slack = np.where(has, np.minimum(slack, _ratio(np.abs(lf - rf), m_range)), slack)
        # var_world
        v = [[inp(T, var[:, 3 * r + k]) for k in range(3)] for r in range(3)]
        RV = [[cdot(R[r], [v[0][k], v[1][k], v[2][k]]) for k in range(3)] for r in range(3)]
        RVRt = [[cdot(R[k], RV[r]) for k in range(3)] for r in range(3)]
        ph = [[ZERO, neg(b[2]), b[1]], [b[2], ZERO, neg(b[0])], [neg(b[1]), b[0], ZERO]]
        rv = [[const(T, pose.rot_var[r, k], N) for k in range(3)] for r in range(3)]
        tv = [[const(T, pose.tsl_var[r, k], N) for k in range(3)] for r in range(3)]
        PR = [[dot(ph[r], [rv[0][k], rv[1][k], rv[2][k]]) for k in range(3)] for r in range(3)]
        PRPt = [[dot(PR[r], ph[k]) for k in range(3)] for r in range(3)]
        vw = [[add(add(RVRt[r][k], PRPt[r][k]), tv[r][k]) for k in range(3)] for r in range(3)]
        J = d + [neg(x) for x in nv]
        pv = [[inp(T, PV[:, 6 * r + k]) for k in range(6)] for r in range(6)]
        sigma = ZERO
        for r in range(6):
            sigma = add(sigma, mul(J[r], dot(pv[r], J)))
        for r in range(3):
            sigma = add(sigma, mul(nv[r], dot(vw[r], nv)))
        self.k_sigma = sigma.k
        sg = f64(sigma, N); sq = np.sqrt(np.maximum(sg, 0.0))
        dtp = np.abs(f64(resi, N))
        with np.errstate(divide="ignore", invalid="ignore"):
            m_sigma = UF * dtp + U * resi.k * shadow(resi, N) + 3 * (np.where(sq > 0, sigma.k * U * shadow(sigma, N) / (2 * sq), np.sqrt(sigma.k * U * shadow(sigma, N))) + 2 * U * sq)
        sigma_ok = dtp.astype(np.float32).astype(np.float64) < 3 * sq
        slack = np.where(has & range_ok, np.minimum(slack, _ratio(np.abs(dtp - 3 * sq), m_sigma)), slack)
        self.slack, self.unclear = slack, slack < 1
        self.reason = np.where(has & ~range_ok, RANGE_GATE, np.where(has & range_ok & ~sigma_ok, SIGMA_GATE, self.reason))
        self.match = self.reason == MATCH
        self.sigma = sg
        # the 34 terms (of every point with a plane; the caller masks by self.match)
        half = inp(T, np.full(N, 0.0005))
        one = inp(T, np.ones(N))
        sig_safe = sigma if sigma.v is not None else half
        Rinv = divs(one, add(half, sig_safe))
        a = [cdot([R[0][k], R[1][k], R[2][k]], nv) for k in range(3)]
        jac = [sub(mul(b[1], a[2]), mul(b[2], a[1])), sub(mul(b[2], a[0]), mul(b[0], a[2])), sub(mul(b[0], a[1]), mul(b[1], a[0]))] + nv
        t = []
        for r in range(6):
            for cc in range(r, 6):
                t.append(mul(mul(Rinv, jac[r]), jac[cc]))
        for r in range(6):
            t.append(neg(mul(mul(Rinv, jac[r]), resi)))
        for r, cc in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            t.append(mul(nv[r], nv[cc]))
        t.append(one)
        self.t = t
        self._stk = None
        self.k = [x.k for x in t]
        self.T = T

    def sums(self, idx):
        """(value f64-able T, shadow, d, count) of the 34 sums over the MATCHED points among idx"""
        if self._stk is None:
            self._stk = stack_terms(self.t, self.N)
        return sum_terms(self._stk, [i for i in idx if self.match[i]], [D_HTH] * 21 + [D_HTZ] * 6 + [D_NNT] * 6 + [0])


def stack_terms(t, N):
    """the double-double terms as arrays [len(t)][N] (hi, lo, shadow); an exact zero is a zero row"""
    hi = np.zeros((len(t), N)); lo = np.zeros((len(t), N)); M = np.zeros((len(t), N))
    for j, x in enumerate(t):
        if x.v is not None:
            hi[j], lo[j], M[j] = x.v.hi, x.v.lo, x.m
    return hi, lo, M


def sum_terms(stk, idx, d):
    """double-double sums of the chosen points (pairwise), their shadows, bars (d + |idx|) u M and the count"""
    hi, lo, M = stk
    idx = np.asarray(idx, dtype=np.int64)
    a = DD(hi[:, idx], lo[:, idx])
    while a.hi.shape[1] > 1:
        n = a.hi.shape[1]; h = n // 2
        b = DD(a.hi[:, :h], a.lo[:, :h]) + DD(a.hi[:, h:2 * h], a.lo[:, h:2 * h])
        a = b if n == 2 * h else DD(np.concatenate([b.hi, a.hi[:, -1:]], axis=1), np.concatenate([b.lo, a.lo[:, -1:]], axis=1))
    val = DD(a.hi[:, 0], a.lo[:, 0]) if len(idx) else DD(np.zeros(len(hi)))
    Ms = M[:, idx].sum(axis=1)
    return val, Ms, (np.asarray(d) + len(idx)) * U * Ms, len(idx)


def check_sums(dev, ref):
    """dev [34] against (value, M, bar, count): the worst |error| / bar over the entries; raises on an entry outside its bar.  The count
    (last entry) must be exact; an entry with shadow 0 must be exactly 0."""
    val, M, bar, cnt = ref
    dev = np.asarray(dev, dtype=np.float64)
    assert dev[-1] == cnt, "match count %r, reference %d" % (dev[-1], cnt)
    err = val.err_to(dev)
    zero = M == 0.0
    assert (dev[zero] == 0.0).all(), "entries %s: %r where the reference is an exact zero" % (np.nonzero(zero & (dev != 0))[0], dev[zero & (dev != 0)])
    bad = ~zero & ~(err <= bar)
    bad[-1] = False
    assert not bad.any(), "entry %d: error %.3g, bar %.3g (device %r)" % (np.nonzero(bad)[0][0], err[bad][0], bar[bad][0], dev[bad][0])
    live = ~zero
    live[-1] = False
    return float((err[live] / bar[live]).max()) if live.any() else 0.0


# ------------------------------------------------------------------------------------------------ f64 restatements (numpy)
def voxel_restate(lm, pose, pts, var, defect=None):
    """The point loop of odom_match_body in plain f64, literally; returns terms [N][34] (zero rows for unmatched points)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3); var = np.asarray(var, dtype=np.float64).reshape(-1, 9)
    N = len(pts)
    R, t = pose.R, pose.t
    w = pts @ R.T + t
    leaf, reason, _ = lm.descend(w, np.abs(pts) @ np.abs(R).T + np.abs(t))
    out = np.zeros((N, 34))
    for i in np.nonzero(reason == MATCH)[0]:
        L = lm.leaves[leaf[i]]; c, n, radius = L[32:35], L[35:38], np.float32(L[38])
        b = pts[i]; d = w[i] - c
        resi = n @ d
        dtp = np.float32(abs(resi)); dtc = np.float32(d @ d)
        if not (np.float32(dtc - np.float32(dtp * dtp)) <= np.float32(9.0) * radius):
            continue
        ph = np.array([[0, -b[2], b[1]], [b[2], 0, -b[0]], [-b[1], b[0], 0]])
        vw = R @ var[i].reshape(3, 3) @ R.T
        if defect != "no_rot_var":
            vw = vw + ph @ pose.rot_var @ ph.T
        if defect != "no_tsl_var":
            vw = vw + pose.tsl_var
        J = np.concatenate([d, -n])
        sigma = J @ lm.pv[leaf[i]].reshape(6, 6) @ J + n @ vw @ n
        if defect == "sigma_float":
            sigma = float(np.float32(sigma))
        thr = 3.0 * np.sqrt(sigma)
        if not (float(dtp) <= thr if defect == "le_gate" else float(dtp) < thr):
            continue
        Rinv = 1.0 / ((0.0004 if defect == "0.0004" else 0.0005) + sigma)
        jac = np.concatenate([np.cross(b, (R if defect == "R_for_Rt" else R.T) @ n), n])
        k = 0
        for r in range(6):
            for cc in range(r, 6):
                out[i, k] = Rinv * jac[r] * jac[cc]; k += 1
        out[i, 21:27] = -Rinv * jac * resi
        out[i, 27:33] = [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2]]
        out[i, 33] = 1.0
    return out


def wg_partials(terms, defect=None):
    """[nb][34]: the sums of each workgroup's 256 points (lanes in a xor butterfly of 64, then (w0 + w1) + (w2 + w3))"""
    N = len(terms); nb = (N + 255) // 256
    pad = np.zeros((nb * 256, terms.shape[1])); pad[:N] = terms
    if defect == "drop_tail" and N % 256:
        pad[N - 1] = 0.0
    x = pad.reshape(nb, 4, 64, -1)
    for s in (32, 16, 8, 4, 2, 1):
        x = x + x[:, :, np.arange(64) ^ s, :]
    x = x[:, :, 0, :]
    return (x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])


def reduce_partials(partial, defect=None):
    """The documented order of odom_sum_partials: lane t adds the elements t, t + 238, ... of the flat array, then lane c adds the seven
    group sums c + 34 g in group order."""
    flat = np.asarray(partial, dtype=np.float64).reshape(-1)
    rd = np.zeros(RED_LANES)
    for t in range(RED_LANES):
        s = 0.0
        for x in flat[t::RED_LANES]:
            s += x
        rd[t] = s
    out = np.zeros(34)
    for c in range(34):
        s = rd[c]
        for g in range(1, 6 if defect == "drop_group" else 7):
            s += rd[c + 34 * g]
        out[c] = s
    return out


# ------------------------------------------------------------------------------------------------ kd: the selection, exactly
def kd_slice_bounds(m, slices):
    ntile = (m + 255) // 256; per = (ntile + slices - 1) // slices
    return [(min(s * per * 256, m), min(s * per * 256 + per * 256, m)) for s in range(slices)]


def kd_query(pose, pts):
    """float(R b + t) with every f64 operation rounded, in the kernel's order"""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3); R, t = pose.R, pose.t
    return np.stack([((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)], axis=1).astype(np.float32)


def kd_dist(q, tree, mode="unfused"):
    """[n][m] distances; unfused: every float32 operation rounded (FLANN L2_Simple).  fused: one rounding per multiply-add, emulated in
    f64 (exact products; the double rounding of the sum is rare and is what kd_dist_exact rules out on the near-tie corpus).  double:
    the f64 distance."""
    q = np.asarray(q, dtype=np.float32); tr = np.asarray(tree, dtype=np.float32)
    dx = q[:, None, 0] - tr[None, :, 0]; dy = q[:, None, 1] - tr[None, :, 1]; dz = q[:, None, 2] - tr[None, :, 2]
    if mode == "unfused":
        return (dx * dx + dy * dy) + dz * dz
    if mode == "double":
        dx, dy, dz = dx.astype(np.float64), dy.astype(np.float64), dz.astype(np.float64)
        return (dx * dx + dy * dy) + dz * dz
    d = (dx * dx).astype(np.float64)
    d = (dy.astype(np.float64) * dy.astype(np.float64) + d).astype(np.float32).astype(np.float64)
    return (dz.astype(np.float64) * dz.astype(np.float64) + d).astype(np.float32)


def _rn32(x):
    """a positive rational rounded to the nearest float32 (ties to even), as a rational; normal range"""
    if x == 0:
        return x
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    return round(x / ulp) * ulp


def kd_dist_exact(q, p, fused):
    """one float distance in exact rational arithmetic -> the float32 result"""
    dl = [_rn32(abs(Fraction(float(a)) - Fraction(float(b)))) for a, b in zip(q, p)]
    if fused:
        d = _rn32(dl[0] * dl[0]); d = _rn32(dl[1] * dl[1] + d); d = _rn32(dl[2] * dl[2] + d)
    else:
        d = _rn32(_rn32(dl[0] * dl[0]) + _rn32(dl[1] * dl[1])); d = _rn32(d + _rn32(dl[2] * dl[2]))
    return np.float32(float(d))


def kd_keys(D, lo, later_wins=False):
    """distance matrix of map points lo.. -> the five smallest words (distance bits << 32 | index) per query, sorted, padded"""
    n, m = D.shape
    idx = np.arange(lo, lo + m, dtype=np.uint64)
    if D.dtype == np.float64:
        order = np.argsort(D, axis=1, kind="stable")[:, :5]
        key = (np.take_along_axis(D, order, axis=1).astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[order]
    else:
        bits = D.view(np.uint32).astype(np.uint64) << np.uint64(32)
        key = bits | (np.uint64(0xFFFFFFFF) - idx if later_wins else idx)[None, :]
        key = np.sort(key, axis=1)[:, :5]
        if later_wins:
            key = (key & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF)))
    out = np.full((n, 5), UNFILLED, dtype=np.uint64)
    out[:, :key.shape[1]] = key
    return out


def kd_candidates(q, tree, slices, mode="unfused", later_wins=False):
    """cand [slices][n][5] as kd_match_body leaves them"""
    q = np.asarray(q, dtype=np.float32); tree = np.asarray(tree, dtype=np.float32)
    out = np.full((slices, len(q), 5), UNFILLED, dtype=np.uint64)
    for s, (lo, hi) in enumerate(kd_slice_bounds(len(tree), slices)):
        if hi > lo:
            out[s] = kd_keys(kd_dist(q, tree[lo:hi], mode), lo, later_wins)
    return out


def kd_merge(cand, first_slice_only=False):
    """the five smallest filled words over the slices (kd_fit_body); UNFILLED-index words are skipped; ~0 pads"""
    c = cand[:1] if first_slice_only else cand
    c = np.transpose(c, (1, 0, 2)).reshape(c.shape[1], -1).copy()
    c[(c & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return np.sort(c, axis=1)[:, :5]


# ------------------------------------------------------------------------------------------------ kd: the plane fit
def _dd(x):
    return DD(np.array(x, dtype=np.float64))


def kd_fit_ref(tree, best):
    """best [n][5] merged words -> dict(x [n][3] DD-evaluated f64, n4 [n][4] planes, bar_n, bar_d, reject, unclear, kappa)"""
    tree = np.asarray(tree, dtype=np.float32).astype(np.float64)
    n = len(best)
    full = best[:, 4] != np.uint64(0xFFFFFFFFFFFFFFFF)
    ids = np.where(best == np.uint64(0xFFFFFFFFFFFFFFFF), 0, best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    A = tree[ids]                                                    # [n][5][3]
    # normal equations in double-double: (A^T A) x = -A^T 1, solved by the adjugate
    a = [[_dd(A[:, k, c]) for c in range(3)] for k in range(5)]
    G = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(r, 3):
            s = a[0][r] * a[0][c]
            for k in range(1, 5):
                s = s + a[k][r] * a[k][c]
            G[r][c] = G[c][r] = s
    g = []
    for r in range(3):
        s = a[0][r]
        for k in range(1, 5):
            s = s + a[k][r]
        g.append(-s)
    cof = lambda i, j, k, l: G[i][j] * G[k][l] - G[i][l] * G[k][j]          # noqa: E731
    adj = [[cof(1, 1, 2, 2), -cof(0, 1, 2, 2), cof(0, 1, 1, 2)], [None, cof(0, 0, 2, 2), -cof(0, 0, 1, 2)], [None, None, cof(0, 0, 1, 1)]]
    adj[1][0], adj[2][0], adj[2][1] = adj[0][1], adj[0][2], adj[1][2]
    det = G[0][0] * adj[0][0] + G[0][1] * adj[1][0] + G[0][2] * adj[2][0]
    with np.errstate(all="ignore"):
        x = [((adj[r][0] * g[0] + adj[r][1] * g[1] + adj[r][2] * g[2]) / det) for r in range(3)]
        xf = np.stack([v.f64() for v in x], axis=1)
        res = np.stack([(a[k][0] * x[0] + a[k][1] * x[1] + a[k][2] * x[2] + _dd(np.ones(n))).f64() for k in range(5)], axis=1)   # A x + 1
        sv = np.linalg.svd(A, compute_uv=False)
        kappa = sv[:, 0] / sv[:, 2]
        xn = np.linalg.norm(xf, axis=1)
        bar = 100 * 5 * U * (kappa * xn + kappa ** 2 * np.linalg.norm(res, axis=1) / sv[:, 0])
        margin = np.linalg.norm(A, axis=2) * bar[:, None] + 5 * U * ((np.abs(A) * np.abs(xf)[:, None, :]).sum(axis=2) + 1)
        reject = (np.abs(res) > 0.1).any(axis=1) | ~full | ~np.isfinite(xf).all(axis=1)
        unclear = full & ((np.abs(np.abs(res) - 0.1) < margin).any(axis=1) | ~np.isfinite(bar) | (bar >= 0.01 * xn))
        d = 1.0 / xn
        planes = np.concatenate([xf * d[:, None], d[:, None]], axis=1)
    planes[reject] = (0.0, 0.0, 0.0, -1.0)
    return dict(planes=planes, bar_n=2 * bar / xn + 4 * U, bar_d=d * (bar / xn + 3 * U), reject=reject, unclear=unclear, kappa=kappa, full=full)


def kd_fit_restate(tree, best):
    """f64 restatement of kd_fit_body: the least-squares solution of the 5 x 3 problem (LAPACK), the 0.1 gate, normalisation"""
    tree = np.asarray(tree, dtype=np.float32).astype(np.float64)
    out = np.zeros((len(best), 4)); out[:, 3] = -1.0
    for i, bk in enumerate(best):
        if bk[4] == np.uint64(0xFFFFFFFFFFFFFFFF):
            continue
        A = tree[(bk & np.uint64(0xFFFFFFFF)).astype(np.int64)]
        x = np.linalg.lstsq(A, -np.ones(5), rcond=None)[0]
        if (np.abs(A @ x + 1.0) > 0.1).any() or not np.isfinite(x).all():
            continue
        d = 1.0 / np.sqrt(x @ x)
        out[i] = [x[0] * d, x[1] * d, x[2] * d, d]
    return out


# ------------------------------------------------------------------------------------------------ kd: the 28 sums from given planes
class KdSumsRef:
    def __init__(self, pose, pts, planes, T=DD):
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3); planes = np.asarray(planes, dtype=np.float64)
        N = self.N = len(pts)
        self.match = planes[:, 3] >= 0
        b = [inp(T, pts[:, k]) for k in range(3)]
        w, R = world(T, pose, b)
        nv = [inp(T, planes[:, k]) for k in range(3)]; dist = inp(T, planes[:, 3])
        pd2 = add(dot(nv, w), dist)
        a = [cdot([R[0][k], R[1][k], R[2][k]], nv) for k in range(3)]
        jac = [sub(mul(b[1], a[2]), mul(b[2], a[1])), sub(mul(b[2], a[0]), mul(b[0], a[2])), sub(mul(b[0], a[1]), mul(b[1], a[0]))] + nv
        t = []
        for r in range(6):
            for cc in range(r, 6):
                t.append(mul(jac[r], jac[cc]))
        for r in range(6):
            t.append(neg(mul(pd2, jac[r])))
        t += [ZERO] * 6 + [inp(T, np.ones(N))]
        self.t = t
        self._stk = None
        self.k = [x.k for x in t]

    def sums(self, idx):
        if self._stk is None:
            self._stk = stack_terms(self.t, self.N)
        return sum_terms(self._stk, [i for i in idx if self.match[i]], [D_KD_HTH] * 21 + [D_KD_HTZ] * 6 + [0] * 6 + [0])


def kd_accum_restate(pose, pts, planes):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3); R, t = pose.R, pose.t
    out = np.zeros((len(pts), 34))
    for i in np.nonzero(planes[:, 3] >= 0)[0]:
        n, b = planes[i, :3], pts[i]
        w = R @ b + t
        pd2 = n @ w + planes[i, 3]
        jac = np.concatenate([np.cross(b, R.T @ n), n])
        k = 0
        for r in range(6):
            for cc in range(r, 6):
                out[i, k] = jac[r] * jac[cc]; k += 1
        out[i, 21:27] = -pd2 * jac
        out[i, 33] = 1.0
    return out


# ------------------------------------------------------------------------------------------------ kd corpora
def lattice_corpus(m, n):
    """an integer lattice offset from the origin (m points, x fastest) and n queries at half-integers inside it: every float operation
    exact, ties everywhere"""
    side = int(np.ceil(m ** (1 / 3))) + 1
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]
    tree = (g[:m] + np.array([3.0, -2.0, 1.0])).astype(np.float64)
    rng = np.random.default_rng(20261019)
    q = rng.integers(0, side - 1, (n, 3)) + 0.5 + np.array([3.0, -2.0, 1.0])
    return tree, q.astype(np.float64)


def near_tie_corpus(want=64, seed=20261020, max_trials=20000):
    """Clusters of seven map points 16 apart and one query each, kept when exact-arithmetic emulation of the fused and of the unfused
    float distance puts the query's neighbours in different orders (two of them sit at mirrored offsets, equidistant in exact
    arithmetic before the coordinates are rounded).  Returns (tree [7 k][3], queries [k][3]) as float-representable doubles."""
    rng = np.random.default_rng(seed)
    tree, qs = [], []
    for trial in range(max_trials):
        if len(qs) >= want:
            break
        base = np.array([16.0 * len(qs), 5.0, -7.0])
        q = (base + rng.uniform(-1, 1, 3)).astype(np.float32)
        v = rng.uniform(0.2, 0.9, 3) * rng.choice([-1, 1], 3)
        perm = rng.permutation(3)
        while (perm == np.arange(3)).all():
            perm = rng.permutation(3)
        pts = [q + v, q + v[perm]] + [q + rng.normal(0, 1, 3) * s for s in (0.2, 0.4, 1.3, 1.7, 2.2)]
        pts = np.array(pts).astype(np.float32)
        order = rng.permutation(7)
        pts = pts[order]
        du = [kd_dist_exact(q, p, False) for p in pts]; df = [kd_dist_exact(q, p, True) for p in pts]
        ku = sorted(range(7), key=lambda j: (du[j], j))[:5]; kf = sorted(range(7), key=lambda j: (df[j], j))[:5]
        if ku != kf:
            tree.append(pts); qs.append(q)
    assert len(qs) >= want, "near-tie search found %d of %d" % (len(qs), want)
    return np.concatenate(tree).astype(np.float64), np.array(qs).astype(np.float64)


def room_corpus(m, n, seed=20261021):
    """plane-like random points: four walls with 5 mm noise, map and queries drawn alike; float-representable"""
    rng = np.random.default_rng(seed)

    def draw(k):
        u = rng.uniform(0, 4, (k, 2)); e = rng.normal(0, 0.005, k); w = rng.integers(0, 4, k)
        p = np.zeros((k, 3))
        p[w == 0] = np.stack([u[:, 0], u[:, 1], e], axis=1)[w == 0]
        p[w == 1] = np.stack([u[:, 0], e, u[:, 1]], axis=1)[w == 1]
        p[w == 2] = np.stack([e, u[:, 0], u[:, 1]], axis=1)[w == 2]
        p[w == 3] = np.stack([u[:, 0], 4 + e, u[:, 1] * 0.5 + u[:, 0] * 0.1], axis=1)[w == 3]
        return (p + np.array([0.5, -0.375, 0.25])).astype(np.float32).astype(np.float64)
    tree, q = draw(m), draw(n)
    for a in (tree, q):                                                 # a tenth of each off the walls: clutter, and rejected fits
        loose = rng.random(len(a)) < 0.1
        a[loose] = (a[loose] + rng.normal(0, 0.3, (int(loose.sum()), 3))).astype(np.float32).astype(np.float64)
    return tree, q


def state_of(R, t):
    s = np.zeros(25); s[1:10] = np.asarray(R).ravel(); s[10:13] = t; s[22:25] = [0, 0, -9.8]
    return s


def general_pose():
    a = np.array([0.02, -0.03, 0.05]); th = np.linalg.norm(a); k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K, np.array([0.011, -0.007, 0.004])


def fused_query_differs(pose, pts):
    """queries whose float rounding differs between a fused and an unfused evaluation of R b + t: any coordinate whose f64 value lies
    within 8 u of its shadow from a float rounding boundary"""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    w = p @ pose.R.T + pose.t; M = np.abs(p) @ np.abs(pose.R).T + np.abs(pose.t)
    f = w.astype(np.float32).astype(np.float64)
    nxt = np.nextafter(w.astype(np.float32), np.where(w > f, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    mid = 0.5 * (f + nxt)
    return (np.abs(w - mid) <= 8 * U * M).any(axis=1)


# ------------------------------------------------------------------------------------------------ voxel corpus
VOXEL_CLASSES = ("random", "no_root", "key_range", "no_plane", "untouched", "max_layer", "range_gate", "sigma_gate")
_EXPECT = dict(no_root=NO_ROOT, key_range=KEY_RANGE, no_plane=NO_PLANE, untouched=UNTOUCHED, max_layer=MATCH, range_gate=RANGE_GATE,
               sigma_gate=SIGMA_GATE)
BATCHES = (63, 64, 65, 255, 256, 257, 1791, 1792, 1793, 3585)


def rand_var(n, seed, scale=0.005):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, scale, (n, 3, 3))
    return np.ascontiguousarray((A @ A.transpose(0, 2, 1) + 1e-6 * np.eye(3)).reshape(n, 9))


def full_cov(seed=7):
    """a full SPD covariance of the size of the diagonal one of the state-level tests (1e-4 pose, 1e-5 biases)"""
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 1, (15, 15))
    Q, _ = np.linalg.qr(A)
    d = np.concatenate([rng.uniform(0.5e-4, 2e-4, 9), rng.uniform(0.5e-5, 2e-5, 6)])
    B = np.eye(15) + 0.3 * (Q - np.eye(15))
    return B @ np.diag(d) @ B.T


def voxel_candidates(lm, scan_world, seed, per_class=400):
    """World points by class (before the reference has judged them): the scan jittered by 5 mm, and points placed in the map's own
    leaves where each class lives."""
    rng = np.random.default_rng(seed)
    out = {}
    sw = np.asarray(scan_world)
    out["random"] = sw[rng.permutation(len(sw))[:2600]] + rng.normal(0, 0.005, (min(2600, len(sw)), 3))
    out["no_root"] = sw[:per_class] + np.array([1000.0, 0.0, 0.0])
    far = (KEY_OFF + rng.integers(10, 5000, (per_class, 3)) + 0.5) * lm.vs * rng.choice([-1.0, 1.0], (per_class, 3))
    out["key_range"] = np.where(rng.integers(0, 3, (per_class, 1)) == np.arange(3)[None, :], far, sw[:per_class])
    noplane, untouched, deep, rng_gate, sig_gate = [], [], [], [], []
    for (k, L, p), r in lm.leaf.items():
        c, half = lm.centre(k, L, p)
        row = lm.leaves[r]
        if row[7] == 0:
            noplane.append(c + rng.uniform(-0.4, 0.4, 3) * half)
            continue
        pc, pn, rad = row[32:35], row[35:38], row[38]
        inside = lambda x: (np.abs(x - c) < 0.9 * half).all()            # noqa: E731
        if L == lm.max_layer and inside(pc):
            deep.append(pc + np.cross(pn, rng.normal(0, 1, 3)) * 0.02 * half)
        corners = c + 0.85 * half * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
        dcs = corners - pc
        inpl = (dcs ** 2).sum(axis=1) - (dcs @ pn) ** 2
        rng_gate += list(corners[inpl > 18 * rad])
        for sgn in (1.0, -1.0):
            x = pc + sgn * pn * 0.12
            if inside(x):
                sig_gate.append(x)
                break
    for (k, L, p) in lm.internal:
        for o in range(8):
            ch = (k, L + 1, p * 8 + o if L > 0 else o)
            if ch not in lm.leaf and ch not in lm.internal:
                c, half = lm.centre(*ch)
                untouched.append(c + rng.uniform(-0.4, 0.4, 3) * half)
    for name, lst in (("no_plane", noplane), ("untouched", untouched), ("max_layer", deep), ("range_gate", rng_gate), ("sigma_gate", sig_gate)):
        a = np.array(lst).reshape(-1, 3)
        out[name] = a[rng.permutation(len(a))[:per_class]]
    return out


def voxel_corpus(lm, pose, scan_world, seed, total=3600):
    """Body points, covariances and classes of one (pose, covariance): every point clear by the reference; the constructed classes at
    least twice their margin from every gate and judged as their class says.  Ordered so that the first 300 hold every class and every
    prefix of BATCHES ends in a match.  Returns dict(pts, var, cls, ref, dropped_random, n_random)."""
    cand = voxel_candidates(lm, scan_world, seed)
    names, world = [], []
    for c in VOXEL_CLASSES:
        names += [c] * len(cand[c]); world.append(cand[c])
    world = np.concatenate(world); names = np.array(names)
    pts = (world - pose.t) @ pose.R                                    # R^T (w - t), row form
    var = rand_var(len(pts), seed + 1)
    ref = VoxelRef(lm, pose, pts, var)
    is_rand = names == "random"
    keep = np.where(is_rand, ~ref.unclear, ref.slack >= 2)
    for c, e in _EXPECT.items():
        keep &= (names != c) | (ref.reason == e)
    keep &= (names != "max_layer") | (ref.layer == lm.max_layer)
    n_random, dropped = int(is_rand.sum()), int((is_rand & ref.unclear).sum())
    idx = np.nonzero(keep)[0]
    rng = np.random.default_rng(seed + 2)
    idx = idx[rng.permutation(len(idx))]
    # at most `total`, the constructed classes first in line for their places
    order = np.argsort(np.where(names[idx] == "random", 1, 0), kind="stable")
    idx = idx[order][:total]
    idx = idx[rng.permutation(len(idx))]
    cls = names[idx]
    for c in VOXEL_CLASSES[1:]:                                        # at least five of every class among the first 300
        have = int((cls[:300] == c).sum())
        back = [j for j in range(300, len(idx)) if cls[j] == c]
        front = [j for j in range(300) if cls[j] == "random"]
        for _ in range(max(0, min(5 - have, len(back)))):
            a, b = front.pop(), back.pop()
            idx[a], idx[b] = idx[b], idx[a]
            cls[a], cls[b] = cls[b], cls[a]
    m = ref.reason[idx] == MATCH
    idx = list(idx)
    spare = [j for j in range(len(idx) - 1, -1, -1) if m[j] and (j + 1) not in BATCHES]
    for n in BATCHES:
        if n <= len(idx) and not m[n - 1]:
            j = spare.pop()
            while j < 300:                                            # (leave the first 300 as drawn)
                j = spare.pop()
            idx[n - 1], idx[j] = idx[j], idx[n - 1]
            m[n - 1], m[j] = m[j], m[n - 1]
    idx = np.array(idx)
    ref = VoxelRef(lm, pose, pts[idx], var[idx])
    assert not ref.unclear.any()
    return dict(pts=pts[idx], var=var[idx], cls=names[idx], ref=ref, dropped_random=dropped, n_random=n_random)


def scene_poses(s, k, synth):
    """the two poses of the voxel cases: the ground truth of scan k and the perturbed prediction of test_gpu_odom_resident.py"""
    rng = np.random.default_rng(5)
    Rp = s["R_gt"][k] @ synth.so3_exp(rng.normal(0, np.radians(0.2), 3))
    return {"gt": (s["R_gt"][k], s["p_gt"][k]), "perturbed": (Rp, s["p_gt"][k] + rng.normal(0, 0.02, 3))}


def scene_covs():
    diag = np.eye(15) * 1e-4
    diag[9:, 9:] = np.eye(6) * 1e-5
    return {"diag": diag, "full": full_cov()}
