"""High-precision references, magnitude shadows, counted accuracy bars and corpora for the chain that produces the plane data of a
leaf and the covariance of a point: plane_update_dev (csrc/vba_kernels_map.hpp, run from margi_leaf_body), k_var_init
(csrc/vba_kernels_scan.hpp) and k_scan_to_soa_pvec_update with the Bf_var terms of ord_terms (csrc/vba_kernels_map.hpp).  A helper
shared by tests/test_plane_cpu.py (f64 restatements, the C++ oracle, caps, teeth) and tests/test_gpu_plane.py (the device, through
vba_debug_plane_update, vba_scan_var_init and vba_map_pvec_update_cut_voxel).  No GPU code; nothing outside the repository is read.

Value type.  That of tests/hess_ref.py and tests/odom_ref.py: Tr(v, m, k) with v a double-double (or mpmath) vector over the leaves or
points, m the magnitude shadow and k the counted relative roundings under |fl(x) - x| <= k u m, u = 2^-53: inputs 0; a +- b: max + 1;
a * b: ka + kb + 1; a factor that is an exact power of two, a product or sum with an exact zero, a negation: none; a / b by the
quotient rule odom_ref.divs (ka + kb + 1 on ma mb / b^2); an exact 1.0 or 0.0 of a pose does not round (odom_ref.cmul).  A zero INPUT
of one leaf or point (an axis-aligned eigenvector, a centre on an axis, a point at the origin) has shadow 0, and so has every product
with it: an entry whose shadow is exactly 0 must be exactly 0.  An entry with k = 0 and a non-zero shadow must be bit-exact.  Two rules
are added here, both next to their use below:
  sqrt   a correctly rounded square root of a value with count ka on shadow ma: the error ka u ma / (2 sqrt a) of the argument plus one
         rounding, k = ceil(ka / 2) + 1 on the shadow ma / sqrt a  (= sqrt a for a sum of squares, where ma = a)
  sin    the ONE sine, of the constant fl(degree_inc * 0.017453293): the argument's rounding (condition x cot x <= 1: one) plus a library
         sine within 4 ulp (the bound of the OpenCL C specification for double, which the device library is written to; glibc
         states less than 1 ulp), 4 ulp <= 8 u |sin|: k = 9
Bars are per entry (and per leaf, per point) on that entry's own shadow; nothing is divided by a maximum; nothing is tuned to a device.

plane_update_ref follows OctoTree::plane_update (oracle/map_oracle.hpp:202-226) at l = 0, the eigen-pairs taken as given:
  nv = 1 / N  1;  c = v nv  2;  ukl = u_k u_0^T  1;  fkl[0..5]  1 or 2;  u_k . c  5;  tail = -(u_0 (u_k . c) + u_k (u_0 . c))  7;
  s_k = nv / (ev0 - evk)  3 on the shadow nv (|ev0| + |evk|) / (ev0 - evk)^2: the gap's amplification enters through the quotient rule;
  u_c = sum_k (u_k fkl) s_k  columns 0..5: 6 or 7, summed 7 or 8; columns 6..8: 12, summed 13;  Jc = u_c cov_add: products 8, 9, 9, 8, 9,
  8, 14, 14, 14, summed in that order (max + 1 per addition) 17;  Jc u_c^T: products 25 or 26 and 31, summed 34;
  Jc_N = nv Jc[:, 6:9]  19;  nv^2 cov_add[6:9, 6:9]  4;  normal = u_0  0;  radius = (double)(float)ev2  0:
    K_CENTRE = 2, K_NN = 34, K_CROSS = 19, K_CC = 4.
var_init_ref follows calcBodyVar + var_init (oracle/map_oracle.hpp:79-103):
  z == 0 -> 0.0001;  s = x x + y y + z z  3;  nrm = sqrt s  3;  range = (float) nrm: a DISCRETE decision: a point whose exact root lies
  within 3 u nrm of the midpoint of two neighbouring floats is UNCLEAR and is left out, every other point's range is an exact input;
  range_var = (float)(range_inc range_inc) in float  0;  sn = sin(...)  9, dv = sn sn  19;  d = p / nrm  4;  b1z = -(d0 + d1) / d2  10;
  n1 = sqrt(2 + b1z b1z)  12;  b1 = (1, 1, b1z) / n1  13, 13, 23;  b2 = b1 x d  29;  n2  32;  b2 / n2  62;
  a1 = range (d x b1)  30;  a2 = range (d x b2)  69;  var = (d_i rv) d_j + ((a1_i dv) a1_j + (a2_i dv) a2_j)  10, 81, 159 -> 161;
  extrinsic  pnt = R p + t  4;  R var  164;  (R var) R^T  167  (identity: 0 and 161):
    K_PNT = 4, K_VAR = 167.
pvec_update_ref: var_world = ((R var) R^T + (hat(p) rot_var) hat(p)^T) + tsl_var  8 (R var 3, times R^T 6, hat(p) rot_var 2, times
hat(p)^T 4, sums 7, 8), pw = R p + t  4; bf_var_ref: the 45 upper-triangle entries of Bf_var (oracle/map_oracle.hpp:62-75) of tracked
var_world and pw: Bi var  14, (Bi var) Bi^T  20, the rest as they come:  K_VW = 8, K_PW = 4, K_BF = 20.
The counts the code keeps are asserted equal to these constants (tests/test_plane_cpu.py)."""
from fractions import Fraction

import numpy as np

from hess_ref import DD, MP, Tr, ZERO, U, add, dot, mul, neg, sc, sub  # noqa: F401
from odom_ref import cdot, const, divs, inp

K_CENTRE, K_NN, K_CROSS, K_CC = 2, 34, 19, 4
K_PNT, K_VAR = 4, 167
K_VW, K_PW, K_BF = 8, 4, 20
DEG2RAD = 0.017453293                                       # PCL's macro, as the reference compiles it
PLANE_CLASSES = ("wall", "line3", "line6", "line9", "axis", "bigN", "neg", "far")
N_LEAVES = 257
PREFIXES = (63, 64, 65, 256, 257)


def ci(r, c):
    """index of (r, c) in the row-by-row upper triangle of a symmetric 9 x 9"""
    rr, cc = (r, c) if r <= c else (c, r)
    return rr * 9 - rr * (rr - 1) // 2 + (cc - rr)


# ------------------------------------------------------------------------------------------------ packed results and the check
class Out:
    """E entries over L leaves / points: v (value type, [E][L]), m [E][L], k [E]"""

    def __init__(self, items, L, T=DD):
        self.L, self.k = L, np.array([x.k for x in items])
        self.m = np.stack([np.zeros(L) if x.v is None else np.broadcast_to(x.m, (L,)) for x in items])
        self.v = T.stack({(j,): x.v for j, x in enumerate(items) if x.v is not None} or {(0,): T.of(np.zeros(L))}, (len(items),))

    def f64(self):
        return self.v.f64().T

    def take(self, entries):
        """the chosen entries as an Out of their own"""
        o = object.__new__(Out)
        e = np.asarray(entries)
        o.L, o.k, o.m = self.L, self.k[e], self.m[e]
        o.v = DD(self.v.hi[e], self.v.lo[e]) if isinstance(self.v, DD) else MP(self.v.a[e])
        return o

    def rows(self, idx):
        """the chosen leaves / points as an Out of their own"""
        o = object.__new__(Out)
        i = np.asarray(idx)
        o.L, o.k, o.m = len(i), self.k, self.m[:, i]
        o.v = DD(self.v.hi[:, i], self.v.lo[:, i]) if isinstance(self.v, DD) else MP(self.v.a[:, i])
        return o


def judge(dev, ref):
    """dev [L][E] against an Out -> (bad [L][E], ratio [L][E]): error over bar where a bar exists, 0 for exact entries"""
    d = np.asarray(dev, dtype=np.float64).reshape(ref.L, -1).T
    err = ref.v.err_to(d)
    bar = ref.k[:, None] * U * ref.m
    zero = ref.m == 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = np.where(zero, d != 0.0, ~(err <= bar))
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)
    return bad.T, ratio.T


def check(dev, ref, what="", names=None):
    """raises on an entry outside its bar (or a non-zero where the shadow is 0, a non-exact where the count is 0); returns the worst ratio"""
    bad, ratio = judge(dev, ref)
    if bad.any():
        i, e = np.argwhere(bad)[0]
        raise AssertionError("%s row %d%s entry %d: device %r, reference %r, shadow %.3g, count %d (%d entries outside)" % (
            what, i, "" if names is None else " (%s)" % (names[i],), e, np.asarray(dev).reshape(ref.L, -1)[i, e], ref.f64()[i, e], ref.m[e, i], ref.k[e], bad.sum()))
    return float(ratio.max()) if ratio.size else 0.0


def sqrt_t(v):
    if isinstance(v, DD):
        s = np.sqrt(v.hi)
        safe = np.where(s > 0, s, 1.0)
        r = v - DD(s) * DD(s)
        return DD(s) + DD(np.where(s > 0, r.hi / (2.0 * safe), 0.0))
    import mpmath
    return MP(np.array([mpmath.sqrt(x) for x in v.a], dtype=object))


def sqrts(a):
    """the sqrt rule of the module docstring"""
    r = sqrt_t(a.v)
    return Tr(r, a.m / r.absf(), (a.k + 1) // 2 + 1)


# ------------------------------------------------------------------------------------------------ plane_update
def plane_update_ref(pcr, ev, Um, cov45, T=DD):
    """pcr [L][10], ev [L][3], Um [L][9] (row-major, columns = eigenvectors), cov45 [L][45] -> Out of 43 entries per leaf:
    centre(3) | normal(3) | radius | plane_var(36 row-major)"""
    pcr = np.atleast_2d(np.asarray(pcr, dtype=np.float64)); ev = np.atleast_2d(np.asarray(ev, dtype=np.float64))
    Um = np.atleast_2d(np.asarray(Um, dtype=np.float64)); cov45 = np.atleast_2d(np.asarray(cov45, dtype=np.float64))
    L = len(pcr)
    one = inp(T, np.ones(L))
    nv = divs(one, inp(T, pcr[:, 9]))
    c = [mul(inp(T, pcr[:, 6 + j]), nv) for j in range(3)]
    u = [[inp(T, Um[:, 3 * r + k]) for r in range(3)] for k in range(3)]      # u[k] = column k
    lam = [inp(T, ev[:, k]) for k in range(3)]
    cv = [[inp(T, cov45[:, ci(r, cc)]) for cc in range(9)] for r in range(9)]
    uc = [[ZERO] * 9 for _ in range(3)]
    for k in (1, 2):
        a, b = u[k], u[0]
        fkl = [mul(a[0], b[0]), add(mul(a[1], b[0]), mul(a[0], b[1])), add(mul(a[2], b[0]), mul(a[0], b[2])),
               mul(a[1], b[1]), add(mul(a[1], b[2]), mul(a[2], b[1])), mul(a[2], b[2])]
        ac, bc = dot(a, c), dot(b, c)
        fkl += [neg(add(mul(b[j], ac), mul(a[j], bc))) for j in range(3)]
        s = divs(nv, sub(lam[0], lam[k]))                  # the shadow of the gap is |ev0| + |evk|
        for r in range(3):
            for j in range(9):
                uc[r][j] = add(uc[r][j], mul(mul(a[r], fkl[j]), s))
    Jc = [[dot(uc[r], [cv[q][j] for q in range(9)]) for j in range(9)] for r in range(3)]
    pv = [[None] * 6 for _ in range(6)]
    nv2 = mul(nv, nv)
    for r in range(3):
        for cc in range(3):
            pv[r][cc] = dot(Jc[r], uc[cc])
            pv[r][3 + cc] = pv[3 + cc][r] = mul(Jc[r][6 + cc], nv)
            pv[3 + r][3 + cc] = mul(cv[6 + r][6 + cc], nv2)
    radius = inp(T, ev[:, 2].astype(np.float32).astype(np.float64))
    out = Out(c + u[0] + [radius] + [pv[r][cc] for r in range(6) for cc in range(6)], L, T)
    out.k_uc, out.k_jc = max(x.k for row in uc for x in row), max(x.k for row in Jc for x in row)
    return out


def _fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def plane_restate(pcr, ev, Um, cov9, fused=False, defect=None):
    """plane_update_dev in plain f64, from the kernel text, one leaf: -> 43 doubles.  cov9: a full 9 x 9 of which the code reads the
    UPPER triangle.  fused: every multiply-add the compiler may contract (x += a * b; a * b + c * d) rounds once."""
    fm = _fma_exact if fused else (lambda a, b, c: a * b + c)
    pcr = [float(x) for x in pcr]; ev = [float(x) for x in ev]; Um = [float(x) for x in Um]
    cov9 = np.asarray(cov9, dtype=np.float64)

    def cvv(r, c):
        rr, cc = (r, c) if r <= c else (c, r)
        return float(cov9[cc, rr] if defect == "lower" else cov9[rr, cc])
    nv = 1.0 / pcr[9]
    src = 0 if defect == "centre_from_P" else 6
    c = [pcr[src] * nv, pcr[src + 1] * nv, pcr[src + 2] * nv]
    u = [[Um[0], Um[3], Um[6]], [Um[1], Um[4], Um[7]], [Um[2], Um[5], Um[8]]]
    uc = [[0.0] * 9 for _ in range(3)]
    for k in (1, 2):
        a, b = u[k], u[0]
        fkl = [a[0] * b[0], a[1] * b[0] if defect == "fkl1_half" else fm(a[1], b[0], a[0] * b[1]), fm(a[2], b[0], a[0] * b[2]),
               a[1] * b[1], fm(a[1], b[2], a[2] * b[1]), a[2] * b[2]]
        ac = fm(a[2], c[2], fm(a[1], c[1], a[0] * c[0])); bc = fm(b[2], c[2], fm(b[1], c[1], b[0] * c[0]))
        for j in range(3):
            t = fm(ac, b[j], bc * a[j])
            fkl.append(t if defect == "tail_sign" else -t)
        s = nv / (ev[0] - ev[1 if defect == "gap01" else k])
        for r in range(3):
            for j in range(9):
                uc[r][j] = fm(s * a[r], fkl[j], uc[r][j])
    Jc = [[0.0] * 9 for _ in range(3)]
    for r in range(3):
        for j in range(9):
            s = 0.0
            for k in range(9):
                s = fm(uc[r][k], cvv(k, j), s)
            Jc[r][j] = s
    pv = [0.0] * 36
    for r in range(3):
        for cidx in range(3):
            s = 0.0
            for k in range(9):
                s = fm(Jc[r][k], uc[cidx][k], s)
            pv[r * 6 + cidx] = s
            jn = (1.0 if defect == "no_nv_cross" else nv) * (Jc[cidx][6 + r] if defect == "cross_T" else Jc[r][6 + cidx])
            pv[r * 6 + 3 + cidx] = jn; pv[(3 + cidx) * 6 + r] = jn
            pv[(3 + r) * 6 + 3 + cidx] = (nv if defect == "nv_centre" else nv * nv) * cvv(6 + r, 6 + cidx)
    radius = ev[2] if defect == "radius_double" else float(np.float32(ev[2]))
    return np.array(c + u[0] + [radius] + pv)


PLANE_DEFECTS = ("nv_centre", "no_nv_cross", "cross_T", "fkl1_half", "tail_sign", "gap01", "lower", "radius_double", "centre_from_P")


def cov9_of(cov45, lower=None):
    """the symmetric 9 x 9 of 45 upper-triangle entries; lower: a factor on the strict lower triangle (the asymmetric probe)"""
    M = np.zeros((9, 9))
    for r in range(9):
        for c in range(9):
            M[r, c] = cov45[ci(r, c)] * (lower if (lower is not None and r > c) else 1.0)
    return M


# ------------------------------------------------------------------------------------------------ var_init
def _sin_exact(x):
    """sin of a double as a rational, by the Taylor series in exact arithmetic to below 1e-40 (|x| < 1)"""
    x = Fraction(x)
    assert abs(x) < 1
    term, s, n = x, Fraction(0), 1
    while abs(term) > Fraction(1, 10 ** 45):
        s += term
        term = -term * x * x / ((n + 1) * (n + 2))
        n += 2
    return s


def _dd_of_fraction(q, L, T):
    hi = float(q); lo = float(q - Fraction(hi))
    if T is DD:
        return DD(np.full(L, hi), np.full(L, lo))
    import mpmath
    return MP(np.array([mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator)] * L, dtype=object))


def var_init_ref(points, ext, dept_err, beam_err, T=DD):
    """points [n][3], ext [12] (R row-major | t) -> dict(pnt Out 3, var Out 9, unclear [n], range [n] float32)"""
    p = np.array(points, dtype=np.float64).reshape(-1, 3)
    ext = np.asarray(ext, dtype=np.float64)
    n = len(p)
    p[:, 2] = np.where(p[:, 2] == 0, 0.0001, p[:, 2])
    x = [inp(T, p[:, k]) for k in range(3)]
    s = dot(x, x)                                                        # 3
    nrm = sqrts(s)                                                       # sqrt rule: ceil(3 / 2) + 1 = 3
    # range = (float) nrm: unclear within the counted roundings of nrm of a float rounding boundary
    nf = nrm.v.f64()
    rng = nf.astype(np.float32)
    other = np.nextafter(rng, np.where(nf > rng.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    mid = 0.5 * (rng.astype(np.float64) + other.astype(np.float64))     # exact: two neighbouring floats
    unclear = np.abs((nrm.v - T.of(mid)).f64()) <= nrm.k * U * nrm.m
    rg = inp(T, rng.astype(np.float64))
    ri = np.float32(dept_err)
    rv = inp(T, np.full(n, float(np.float32(ri * ri))))                  # range_var: a float product, then an exact input
    arg = float(np.float32(beam_err)) * DEG2RAD
    sq = _sin_exact(Fraction(float(np.float32(beam_err))) * Fraction(DEG2RAD))
    sn = Tr(_dd_of_fraction(sq, n, T), np.full(n, abs(float(sq))), 9)    # sin rule: 1 (argument) + 8 (4 ulp)
    assert abs(arg) < 0.5
    dv = mul(sn, sn)                                                     # 19
    d = [divs(x[k], nrm) for k in range(3)]                              # 4
    b1z = neg(divs(add(d[0], d[1]), d[2]))                               # 10
    n1 = sqrts(add(inp(T, np.full(n, 2.0)), mul(b1z, b1z)))              # 1 * 1 + 1 * 1 = 2 exactly; 22 -> 12
    one = inp(T, np.ones(n))
    b1 = [divs(one, n1), divs(one, n1), divs(b1z, n1)]                   # 13, 13, 23
    cross = lambda a, b: [sub(mul(a[1], b[2]), mul(a[2], b[1])), sub(mul(a[2], b[0]), mul(a[0], b[2])), sub(mul(a[0], b[1]), mul(a[1], b[0]))]  # noqa: E731
    b2 = cross(b1, d)                                                    # 29
    n2 = sqrts(dot(b2, b2))                                              # 61 -> 32
    b2 = [divs(b2[k], n2) for k in range(3)]                             # 62
    a1 = [mul(rg, t) for t in cross(d, b1)]                              # 30
    a2 = [mul(rg, t) for t in cross(d, b2)]                              # 69
    vb = [[add(mul(mul(d[i], rv), d[j]), add(mul(mul(a1[i], dv), a1[j]), mul(mul(a2[i], dv), a2[j]))) for j in range(3)] for i in range(3)]
    R = [[const(T, ext[3 * r + c], n) for c in range(3)] for r in range(3)]
    pnt = [add(cdot(R[r], x), const(T, ext[9 + r], n)) for r in range(3)]
    RV = [[cdot(R[i], [vb[0][j], vb[1][j], vb[2][j]]) for j in range(3)] for i in range(3)]
    var = [[cdot(R[j], RV[i]) for j in range(3)] for i in range(3)]
    return dict(pnt=Out(pnt, n, T), var=Out([var[i][j] for i in range(3) for j in range(3)], n, T), unclear=unclear, range=rng,
                k_body=max(t.k for row in vb for t in row))


def var_init_restate(points, ext, dept_err, beam_err, defect=None):
    """k_var_init in plain f64 numpy, from the kernel text -> (pnt [n][3], var [n][9])"""
    p = np.array(points, dtype=np.float64).reshape(-1, 3); R = np.asarray(ext, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], np.where(p[:, 2] == 0, 0.0001, p[:, 2])
    rng = np.sqrt(x * x + y * y + z * z).astype(np.float32)
    ri = np.float32(dept_err)
    rv = float(ri) * float(ri) if defect == "rv_wide" else float(np.float32(ri * ri))
    sn = np.sin(float(np.float32(beam_err)) * DEG2RAD); dv = sn if defect == "dv_nosq" else sn * sn
    nrm = np.sqrt(x * x + y * y + z * z)
    d0, d1, d2 = x / nrm, y / nrm, z / nrm
    b1x, b1y, b1z = np.ones_like(x), np.ones_like(x), -(d0 + d1) / d2
    n1 = np.sqrt(b1x * b1x + b1y * b1y + b1z * b1z)
    b1x, b1y, b1z = b1x / n1, b1y / n1, b1z / n1
    b2x, b2y, b2z = b1y * d2 - b1z * d1, b1z * d0 - b1x * d2, b1x * d1 - b1y * d0
    n2 = np.sqrt(b2x * b2x + b2y * b2y + b2z * b2z)
    b2x, b2y, b2z = b2x / n2, b2y / n2, b2z / n2
    r = rng.astype(np.float64)
    a1 = [r * (d1 * b1z - d2 * b1y), r * (d2 * b1x - d0 * b1z), r * (d0 * b1y - d1 * b1x)]
    a2 = [r * (d1 * b2z - d2 * b2y), r * (d2 * b2x - d0 * b2z), r * (d0 * b2y - d1 * b2x)]
    d = [d0, d1, d2]
    vb = [[d[i] * rv * d[j] + (a1[i] * dv * a1[j] + a2[i] * dv * a2[j]) for j in range(3)] for i in range(3)]
    pnt = np.stack([R[3 * k] * x + R[3 * k + 1] * y + R[3 * k + 2] * z + R[9 + k] for k in range(3)], axis=1)
    RV = [[R[3 * i] * vb[0][j] + R[3 * i + 1] * vb[1][j] + R[3 * i + 2] * vb[2][j] for j in range(3)] for i in range(3)]
    if defect == "RvR":
        var = [[RV[i][0] * R[j] + RV[i][1] * R[3 + j] + RV[i][2] * R[6 + j] for j in range(3)] for i in range(3)]
    else:
        var = [[RV[i][0] * R[3 * j] + RV[i][1] * R[3 * j + 1] + RV[i][2] * R[3 * j + 2] for j in range(3)] for i in range(3)]
    return pnt, np.stack([var[i][j] for i in range(3) for j in range(3)], axis=1)


VAR_DEFECTS = ("rv_wide", "dv_nosq", "RvR")


# ------------------------------------------------------------------------------------------------ pvec_update and Bf_var
def _pvec_tr(p, var, R, t, rot_var, tsl_var, T):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3); var = np.asarray(var, dtype=np.float64).reshape(-1, 9)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3); t = np.asarray(t, dtype=np.float64)
    rot_var = np.asarray(rot_var, dtype=np.float64).reshape(3, 3); tsl_var = np.asarray(tsl_var, dtype=np.float64).reshape(3, 3)
    n = len(p)
    b = [inp(T, p[:, k]) for k in range(3)]
    Rt = [[const(T, R[r, c], n) for c in range(3)] for r in range(3)]
    v = [[inp(T, var[:, 3 * r + k]) for k in range(3)] for r in range(3)]
    RV = [[cdot(Rt[r], [v[0][k], v[1][k], v[2][k]]) for k in range(3)] for r in range(3)]
    RVRt = [[cdot(Rt[k], RV[r]) for k in range(3)] for r in range(3)]
    ph = [[ZERO, neg(b[2]), b[1]], [b[2], ZERO, neg(b[0])], [neg(b[1]), b[0], ZERO]]
    rv = [[const(T, rot_var[r, k], n) for k in range(3)] for r in range(3)]
    tv = [[const(T, tsl_var[r, k], n) for k in range(3)] for r in range(3)]
    PR = [[dot(ph[r], [rv[0][k], rv[1][k], rv[2][k]]) for k in range(3)] for r in range(3)]
    PRPt = [[dot(PR[r], ph[k]) for k in range(3)] for r in range(3)]
    vw = [[add(add(RVRt[r][k], PRPt[r][k]), tv[r][k]) for k in range(3)] for r in range(3)]
    pw = [add(cdot(Rt[r], b), const(T, t[r], n)) for r in range(3)]
    return vw, pw, n


def _bf_tr(vw, pw):
    two = lambda a: sc(a, 2.0)                                           # noqa: E731
    Bi = [[two(pw[0]), ZERO, ZERO], [pw[1], pw[0], ZERO], [pw[2], ZERO, pw[0]], [ZERO, two(pw[1]), ZERO], [ZERO, pw[2], pw[1]], [ZERO, ZERO, two(pw[2])]]
    Bu = [[dot(Bi[r], [vw[0][c], vw[1][c], vw[2][c]]) for c in range(3)] for r in range(6)]
    out = []
    for r in range(9):
        for c in range(r, 9):
            out.append(dot(Bu[r], Bi[c]) if c < 6 else Bu[r][c - 6] if r < 6 else vw[r - 6][c - 6])
    return out


def pvec_update_ref(p, var, R, t, rot_var, tsl_var, T=DD):
    """-> dict(var_world Out 9, pw Out 3, bf Out 45 = bf_var_ref of the two): per point"""
    vw, pw, n = _pvec_tr(p, var, R, t, rot_var, tsl_var, T)
    return dict(var_world=Out([vw[r][c] for r in range(3) for c in range(3)], n, T), pw=Out(pw, n, T), bf=Out(_bf_tr(vw, pw), n, T))


def bf_var_ref(var_world, pw, T=DD):
    """the 45 upper-triangle entries of Bf_var of GIVEN var_world [n][9] and pw [n][3] (inputs, count 0)"""
    vwa = np.asarray(var_world, dtype=np.float64).reshape(-1, 9); pwa = np.asarray(pw, dtype=np.float64).reshape(-1, 3)
    vw = [[inp(T, vwa[:, 3 * r + c]) for c in range(3)] for r in range(3)]
    return Out(_bf_tr(vw, [inp(T, pwa[:, k]) for k in range(3)]), len(vwa), T)


def hat(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])


def pvec_restate(p, var, R, t, rot_var, tsl_var, defect=None):
    """k_scan_to_soa_pvec_update, world_point and the Bf_var terms of ord_terms in plain f64 -> (var_world [n][9], pw [n][3], bf [n][45])"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3); var = np.asarray(var, dtype=np.float64).reshape(-1, 3, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3); t = np.asarray(t, dtype=np.float64)
    rot_var = np.asarray(rot_var, dtype=np.float64).reshape(3, 3); tsl_var = np.asarray(tsl_var, dtype=np.float64).reshape(3, 3)
    if defect == "tsl_from_rot":
        tsl_var = rot_var
    n = len(p)
    vw = np.zeros((n, 3, 3)); pw = np.zeros((n, 3)); bf = np.zeros((n, 45))
    for i in range(n):
        ph = hat(p[i])
        RV = np.array([[(R[r, 0] * var[i, 0, c] + R[r, 1] * var[i, 1, c]) + R[r, 2] * var[i, 2, c] for c in range(3)] for r in range(3)])
        PR = np.array([[(ph[r, 0] * rot_var[0, c] + ph[r, 1] * rot_var[1, c]) + ph[r, 2] * rot_var[2, c] for c in range(3)] for r in range(3)])
        pt = ph.T if defect == "no_hatT" else ph                      # (the kernel indexes ph[3 c + k]: rows of ph = columns of ph^T)
        for r in range(3):
            for c in range(3):
                vw[i, r, c] = (((RV[r, 0] * R[c, 0] + RV[r, 1] * R[c, 1]) + RV[r, 2] * R[c, 2]) +
                               ((PR[r, 0] * pt[c, 0] + PR[r, 1] * pt[c, 1]) + PR[r, 2] * pt[c, 2])) + tsl_var[r, c]
        x, y, z = [((R[r, 0] * p[i, 0] + R[r, 1] * p[i, 1]) + R[r, 2] * p[i, 2]) + t[r] for r in range(3)]
        pw[i] = (x, y, z)
        Bi = np.array([[2 * x, 0, 0], [y, x, 0], [z, 0, x], [0, 2 * y, 0], [0, z, y], [0, 0, 2 * z]])
        Bu = np.array([[(Bi[r, 0] * vw[i, 0, c] + Bi[r, 1] * vw[i, 1, c]) + Bi[r, 2] * vw[i, 2, c] for c in range(3)] for r in range(6)])
        k = 0
        for r in range(9):
            for c in range(r, 9):
                bf[i, k] = ((Bu[r, 0] * Bi[c, 0] + Bu[r, 1] * Bi[c, 1]) + Bu[r, 2] * Bi[c, 2]) if c < 6 else Bu[r, c - 6] if r < 6 else vw[i, r - 6, c - 6]
                k += 1
    return vw.reshape(n, 9), pw, bf


PVEC_DEFECTS = ("no_hatT", "tsl_from_rot")


# ------------------------------------------------------------------------------------------------ corpora
def rand_spd(n, rng, lo=-6.0, hi=-3.0):
    """n random SPD 3 x 3 of size 1e-6 .. 1e-3"""
    A = rng.normal(0, 1, (n, 3, 3))
    return (A @ A.transpose(0, 2, 1) / 3.0 + 0.1 * np.eye(3)) * (10.0 ** rng.uniform(lo, hi, (n, 1, 1)))


def bf_sum(pw, var):
    """f64 Bf_var sums of points pw [N][3] with covariances var [N][3][3]: the 45 upper-triangle entries of cov_add"""
    N = len(pw)
    Bi = np.zeros((N, 6, 3))
    Bi[:, 0, 0] = 2 * pw[:, 0]; Bi[:, 1, 0] = pw[:, 1]; Bi[:, 1, 1] = pw[:, 0]; Bi[:, 2, 0] = pw[:, 2]; Bi[:, 2, 2] = pw[:, 0]
    Bi[:, 3, 1] = 2 * pw[:, 1]; Bi[:, 4, 1] = pw[:, 2]; Bi[:, 4, 2] = pw[:, 1]; Bi[:, 5, 2] = 2 * pw[:, 2]
    Bu = Bi @ var
    M = np.zeros((9, 9))
    M[:6, :6] = (Bu @ Bi.transpose(0, 2, 1)).sum(axis=0); M[:6, 6:] = Bu.sum(axis=0); M[6:, 6:] = var.sum(axis=0)
    return np.array([M[r, c] for r in range(9) for c in range(r, 9)])


def _rot(rng):
    Q = np.linalg.qr(rng.normal(0, 1, (3, 3)))[0]
    return Q * np.sign(np.linalg.det(Q))


def plane_corpus(seed=20261101, min_point=5):
    """257 leaves cycling through PLANE_CLASSES -> dict(rows [257][67] = add10 | ev3 | U9 | cov45, cls [257]).  ev and U are
    numpy.linalg.eigh of the cluster's covariance; cov_add are f64 Bf_var sums over the cluster's points."""
    rng = np.random.default_rng(seed)
    rows, cls = [], []
    for i in range(N_LEAVES):
        c = PLANE_CLASSES[i % len(PLANE_CLASSES)]
        N = int(rng.integers(min_point + 1, 200)) if i >= 16 else min_point + 1 + i // 8 * 193      # the smallest and the largest N early
        if c == "bigN":
            N = 100000
        Q = _rot(rng)
        ext = rng.uniform(0.1, 0.5)
        sig = np.array([rng.uniform(0.002, 0.02), ext * rng.uniform(0.3, 1.0), ext])        # normal, in-plane, in-plane
        dist = rng.uniform(5.0, 40.0)
        if c == "far":
            dist = rng.uniform(800.0, 1500.0)
        if c.startswith("line"):
            sig[1] = sig[0]
        if c == "neg":
            sig[0] = 0.0
        centre = _rot(rng)[:, 0] * dist
        if c == "axis":
            Q = np.eye(3)[:, rng.permutation(3)]
            centre = np.eye(3)[int(rng.integers(0, 3))] * dist
        pts = (rng.normal(0, 1, (N, 3)) * sig) @ Q.T
        if c == "axis":
            pts -= pts.mean(axis=0)                         # (the centre then comes from the sums below, set exactly)
        pts = pts + centre
        P = pts.T @ pts
        v = pts.sum(axis=0)
        if c == "axis":
            v = centre * N                                  # a centre on an axis: exact zeros
        cm = v / N
        C = P / N - np.outer(cm, cm)
        if c == "axis":                                     # axis-aligned eigenvectors: an exactly diagonal covariance
            C = np.diag(np.diag(C))
        w, V = np.linalg.eigh((C + C.T) / 2)
        if c.startswith("line"):                            # the wanted gap (ev1 - ev0) / ev2, then the eigen-pairs of THAT matrix
            w[1] = w[0] + float("1e-" + c[4:]) * w[2]
            w, V = np.linalg.eigh((V * w) @ V.T)
        if c == "neg":
            w[0] = -1e-18                                   # what an eigen-solver returns for a flat cluster
        if c == "axis":
            assert set(np.abs(V).ravel()) <= {0.0, 1.0}
        add10 = np.array([P[0, 0], P[0, 1], P[0, 2], P[1, 1], P[1, 2], P[2, 2], v[0], v[1], v[2], float(N)])
        rows.append(np.concatenate([add10, w, V.ravel(), bf_sum(pts, rand_spd(N, rng))]))
        cls.append(c)
    return dict(rows=np.array(rows), cls=np.array(cls))


def split67(rows):
    rows = np.asarray(rows).reshape(-1, 67)
    return rows[:, :10], rows[:, 10:13], rows[:, 13:22], rows[:, 22:]


def plane_ref_of_rows(rows, T=DD):
    return plane_update_ref(*split67(rows), T=T)


POINT_CLASSES = ("random", "z0", "z1e-12", "z1e-9", "z1e-6", "x=-y", "axis", "midpoint")


def point_corpus(n=320, seed=20261102):
    """Body points for var_init: ranges 0.3 .. 100 m in all eight octants, z == 0, |z| of 1e-12, 1e-9, 1e-6 of the range, x == -y, points
    on the axes, and ONE point on the z axis at the midpoint of two floats (unclear by construction).  The special classes come first,
    so every tested prefix holds them.  -> dict(pts [n][3], cls [n])"""
    rng = np.random.default_rng(seed)
    pts, cls = [], []
    r_of = lambda: 10.0 ** rng.uniform(np.log10(0.3), 2.0)             # noqa: E731
    for o in range(8):                                                  # every octant, per class
        sgn = np.array([1.0 if o & 4 else -1.0, 1.0 if o & 2 else -1.0, 1.0 if o & 1 else -1.0])
        for c in POINT_CLASSES[1:6]:
            r = r_of()
            q = np.abs(rng.normal(0, 1, 3)); q = q / np.linalg.norm(q) * r * sgn
            if c == "z0":
                q[2] = 0.0
            elif c.startswith("z1e"):
                q[2] = sgn[2] * float(c[1:]) * r
            else:
                q[1] = -q[0]
            q[:2] *= np.sqrt(max(r * r - q[2] * q[2], 0.0)) / np.linalg.norm(q[:2])      # back to the range r (x == -y survives a common factor)
            pts.append(q); cls.append(c)
    for k in range(3):
        for s in (1.0, -1.0):
            q = np.zeros(3); q[k] = s * r_of()
            pts.append(q); cls.append("axis")
    f = np.float32(7.3)
    pts.append(np.array([0.0, 0.0, 0.5 * (float(f) + float(np.nextafter(f, np.float32(np.inf))))])); cls.append("midpoint")
    while len(pts) < n:
        r = r_of()
        q = rng.normal(0, 1, 3)
        pts.append(q / np.linalg.norm(q) * r); cls.append("random")
    return dict(pts=np.array(pts), cls=np.array(cls))


def general_ext():
    """a general extrinsic (12: R row-major | t)"""
    a = np.array([0.3, -0.2, 0.5]); th = np.linalg.norm(a); k = a / th
    K = hat(k)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    return np.concatenate([R.ravel(), [0.04, -0.02, 0.11]])


IDENT_EXT = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
DEPT_ERR, BEAM_ERR = 0.02, 0.05


def lattice_points(n, voxel_size, R, t, seed=20261103, origin=False):
    """n body points whose world images R p + t sit one per voxel: the sites 2 vs (i, j, k), i, j, k >= 1, plus half a voxel, with jitter
    below 0.4 vs.  origin: point 0 is the body origin itself (its voxel, that of t, must be free: t has a non-positive voxel index).
    -> (pts [n][3], keys [n][3] voxel keys of the world points)"""
    rng = np.random.default_rng(seed)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3); t = np.asarray(t, dtype=np.float64)
    side = int(np.ceil(n ** (1 / 3))) + 1
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 3)[:n] + 1
    w = (2.0 * g + 0.5 + rng.uniform(-0.39, 0.39, (n, 3))) * voxel_size
    pts = (w - t) @ R
    if origin:
        pts[0] = 0.0
    w = pts @ R.T + t
    loc = (w / voxel_size).astype(np.float32)
    keys = np.where(loc < 0, loc - np.float32(1.0), loc).astype(np.float32).astype(np.int64)
    assert len({tuple(k) for k in keys}) == n
    return pts, keys


# ------------------------------------------------------------------------------------------------ in situ: the marginalisation's own dumps
def insitu_workload(synth, n_pts=4000):
    """room20k_w4 cut to n_pts points per scan, W = 4, random point covariances -> (wl, scans, poses [W][12], vars)"""
    import dataclasses
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], n_pts=n_pts, win_size=4)
    s = synth.make_scans(wl)
    poses = synth.poses_flat(s["R0"], s["p0"])
    rng = np.random.default_rng(20261104)
    return wl, s, poses, [np.ascontiguousarray(rand_spd(len(p), rng).reshape(-1, 9)) for p in s["points"]]


def insitu_session(wl, s, poses, var, cut, recut, evaluate, margi, slide, dump):
    """cut_voxel(multi) x W, recut, evaluate_only_residual, margi, dump, slide(1), margi again with no recut in between, dump.
    The callables hide which side runs (the device context, or the oracle with its factor store); dump() -> (leaves [L][39],
    plane_var [L][36], cov_add [L][45]) in one row order.  -> (first, second), each a dict keyed by (kx, ky, kz, layer, path) of
    (leaf row, plane_var row, cov_add row)."""
    W = wl.win_size
    for i in range(W):
        cut(i, s["points"][i], poses[i], var[i])
    recut(W, poses)
    evaluate(poses)
    margi(W, poses)
    first = _table(*dump())
    slide(1)
    margi(W - 1, poses[1:])
    return first, _table(*dump())


def _table(leaves, pv, cov):
    assert len(leaves) == len(pv) == len(cov)
    return {tuple(int(v) for v in r[:5]): (r, p, c) for r, p, c in zip(leaves, pv, cov)}


def device_dump(ctx):
    """the two dumps of a context joined by key -> (leaves, plane_var, cov_add)"""
    lv, pv = ctx.dump_leaves(), ctx.dump_plane_var()
    idx = {tuple(r[:5].astype(np.int64)): i for i, r in enumerate(pv)}
    order = [idx[tuple(r[:5].astype(np.int64))] for r in lv]
    return lv, pv[order, 5:41], pv[order, 41:86]


def written(tab):
    """keys of the leaves with is_plane and a written normal"""
    return [k for k, (r, p, c) in tab.items() if r[7] != 0 and np.abs(r[35:38]).max() > 0]


def dump_consistency(tab, keys, what=""):
    """plane_update_ref of the dump's own (pcr_add, eig_value, eig_vector, cov_add) against the dump's centre, normal, radius and
    plane_var, for the chosen leaves -> worst ratio to bar"""
    got, ref = dump_pairs(tab, keys)
    return check(got, ref, what, names=keys)


def dump_pairs(tab, keys):
    """-> (the dumped 43 plane doubles [len(keys)][43], plane_update_ref of the same rows' inputs)"""
    rows = np.array([np.concatenate([tab[k][0][22:32], tab[k][0][10:22], tab[k][2]]) for k in keys])
    return np.array([np.concatenate([tab[k][0][32:39], tab[k][1]]) for k in keys]), plane_ref_of_rows(rows)


def predict_second_pass(first, second, max_points):
    """which leaves the second marginalisation (no new points, no recut) updates, by the reference's gate
    `N - last_num >= 5 || last_num <= 10` with last_num from the first pass (the N it wrote the plane at, 0 if it wrote none), among
    the leaves it visits at all: those that still exist after the first pass, are planes and hold fewer than max_points fixed points.
    -> (firing keys, non-firing keys: leaves with a written plane in the first dump that are not predicted to fire)"""
    fire, keep = [], []
    w1 = set(written(first))
    for k, (r2, p2, c2) in second.items():
        if k not in first:
            continue
        r1 = first[k][0]
        last = int(r1[5]) if k in w1 else 0
        visited = r1[8] != 0 and r1[7] != 0 and r1[6] < max_points
        if visited and (int(r2[5]) - last >= 5 or last <= 10):
            fire.append(k)
        elif k in w1:
            keep.append(k)
    return fire, keep
