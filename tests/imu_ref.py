"""High-precision reference, magnitude shadow, rounding counts, bars and corpus for the IMU factor pass of LI-BA (li_imu_body and the
trial-state residual of k_li_update in csrc/vba_kernels_li.hpp, over vbh::imu_residual_jacobian of csrc/vba_hostmath.hpp).  A helper
shared by tests/test_imu_cpu.py (the g++ build of the very header: calibration, host model of the window assembly, teeth) and
tests/test_gpu_imu.py (the device, through vba_debug_li_imu).  No GPU code; nothing outside the repository is read.

Reference.  The literal formulas of IMU_PRE::give_evaluate(_g) (preintegration.hpp:137-294) and the window assembly of divide_thread
(voxel_map.hpp:551-567 / 783-801), on the doubles the kernel reads: states[W][25], imus[W-1][304] and cov^-1 AS HANDED BACK by the hook
(inverse_pplu's result is not symmetric in its bits, and neither side is asked for a symmetric matrix).  The branches of the reference
project are kept: so3_exp at 1e-11, so3_log's tr > 3 - 1e-6 and |theta| < 0.001 -> f = 1/2 (so at 5e-4 rad the reference reproduces
the project's own theta^2/6 approximation error), jr at 1e-9, jr_inv (through Eigen's matrix -> quaternion -> angle/axis, both of its
branches) at 1e-9.  The mathematically ideal log map is NOT the reference.
Arithmetic: sqrt, sin, cos, acos, atan2, tan and the quotients theta / sin theta, (a/2) / tan(a/2) are evaluated by mpmath at 200 bits
on the exact value of their double-double argument; everything polynomial (rotation products, the 15 x 33 Jacobian, cov^-1 J,
J^T (cov^-1 J), J^T (cov^-1 r), r^T cov^-1 r, the sums over the <= 2 (corner: F) factors of an entry in ascending order) runs in the
double-double arithmetic of tests/hess_ref.py (DD, reused, vectorised over all factors of the corpus at once); MP (mpmath throughout)
is the same code over the other value type and spot-checks the double-double path on a W = 3 window.  The gravity columns 30..32 are
the only difference between the two modes, so one evaluation with nb = 33 serves both (the 30 x 30 part is the same sums in the same
order).

Magnitude shadow M.  hess_ref's rule for sums (absolute values, subtractions as additions) and for inputs.  For a product, a quotient
and a function value the shadow is the first-order CONDITIONED one, which is a bound where hess_ref's plain product of shadows is a
bound too, but does not multiply the cancellation of one factor into the cancellation of the next (the axis q / |q| of a 0.01 rad
rotation has M / |value| ~ 1e2; under M_a M_b the term (1 - ctt) a_r a_c of jr_inv would carry M ~ 2e4 for a value of 1e-5, the block
joca(0,9) a bar of 1e9 times its value, and no defect of the rotation blocks could be seen):
  * a * b:  M = max(|a| M_b, |b| M_a)          (k u M bounds k_a u |b| M_a + k_b u |a| M_b + u |a b|, since M >= |value| always);
  * a / b:  M = max(M_a / |b|, |a| M_b / b^2)  (hess_ref's M_a / |b| when the divisor carries no cancellation);
  * x * x (the norms):  M = max(x^2, 2 |x| M_x), one rounding;
  * y = f(x):  M = max(|y|, |f'(x)| M_x):  the conditioning of acos (1 / sin theta) and of theta / sin theta is in the shadow, as the
    rounding of (tr - 1) / 2 is amplified by ~1e3 just above theta = 1e-3 (atan2: both partials).
For an exact factor (an input, cov^-1) this is hess_ref's rule unchanged.
Rounding count k (standard model, u = 2^-53): hess_ref's rule; sqrt and the division are correctly rounded (1); an exact zero, the
identity, +-1, +-2 and 1/2 are free.
LIBM_ULP = 4: the assumed error bound, in ulp, of the device's f64 sin, cos, acos, atan2 and tan.  The ROCm release the project
builds with ships no accuracy statement for the device library's f64 functions (its rocm-device-libs documentation directory holds the
licence only), so the bound is the stated fallback "assume 4 ulp each", not a documented figure; each call counts as LIBM_ULP roundings.
No other free constant enters a bar.

Bars, per entry:  |x^ - x*| <= k u M, with k the count of the entry including the additions over its factors (k = d + terms, d the
count of one factor's term).  The largest d per quantity over the corpus is pinned below and asserted equal to what the code keeps
(tests/test_imu_cpu.py):
    D_RR = 108 (residual), D_JOC = 633 (Jacobian), D_CJ = 643 (cov^-1 J), D_HF = 1286 (one factor's J^T cov^-1 J entry),
    D_GF = 766 (gradient term), D_QF = 246 (r^T cov^-1 r).
Where they come from, along vba_hostmath.hpp with every branch general (dbg != 0, residual rotation away from 0; a product adds the
counts of its factors + 1):  rb = R_bg dbg 3;  Exp(rb) 38;  Rc = R_delta Exp 41;  res_r = Rc^T (R1^T R2) 47;  the log: acos 54,
theta / (2 sin theta) 59, times (m21 - m12) 48 -> rr[0:3] 108.  The quaternion of res_r: |q_xyz| 105, angle = 2 atan2 109, axis =
q / |q| 207;  (a/2) / tan(a/2) 114, (1 - ctt) a_r a_c 530, JRi 532;  joca(0,0) = -JRi R2^T R1 538;  jr(rb) 45;  joca(0,9) =
-((JRi res_r^T) jr(rb)) R_bg 633.  The other rows are short: hat(exp_t) 6, -dt R1^T 1, -dt^2/2 R1^T 2, rr[3:6] 7, rr[9:15] 1.
cov^-1 J adds 1 + 9 (a rotation column of J holds 10 non-zeros), J^T (cov^-1 J) adds the two and 10 more.
With dbg = 0 (Exp = I exactly) the same chain gives res_r 6, JRi 122, joca(0,9) 128, rr[0:3] 26: the bars follow the branch taken.
The counts are large because the standard model adds the RELATIVE errors of the factors of every product (the axis q / |q| is a
quotient of a 100- and a 105-rounding value and enters JRi squared); they are what the code counts, asserted equal to the constants
above, never tuned to a device.
Nothing is divided by the largest entry.  Entries outside the block-tridiagonal (+ gravity border) pattern must be exactly 0, and so
must an entry whose M is 0 (rr[0:3] of a factor whose residual rotation is the identity by construction)."""
import dataclasses

import mpmath
import numpy as np

import hess_ref as hr
from hess_ref import DD, MP, Tr, ZERO, U, add, neg, sc, sub

LIBM_ULP = 4
D_RR, D_JOC, D_CJ, D_HF, D_GF, D_QF = 108, 633, 643, 1286, 766, 246
MARGIN = 1e-3
CLASSES = ("consistent", "offset", "bigangle", "smallangle", "far", "mixed")
WS = list(range(2, 17))
_PREC = 200


# ------------------------------------------------------------------------------------------------ tracked scalars (vectors over factors)
class _One(Tr):
    """the exact 1 of an identity matrix: a product with it is free"""


def _mul(a, b):
    if a.v is None or b.v is None:
        return ZERO
    if isinstance(a, _One):
        return b
    if isinstance(b, _One):
        return a
    return Tr(a.v * b.v, np.maximum(a.v.absf() * b.m, b.v.absf() * a.m), a.k + b.k + 1)


def _cdiv(a, b):
    """a / b with the divisor's own uncertainty (module docstring)"""
    if a.v is None:
        return ZERO
    ab = b.v.absf()
    return Tr(a.v / b.v, np.maximum(a.m / ab, a.v.absf() * b.m / ab ** 2), a.k + b.k + 1)


def _dot(x, y):
    s = ZERO
    for a, b in zip(x, y):
        s = add(s, _mul(a, b))
    return s


def _matmul(A, B):
    return [[_dot(A[r], [B[k][c] for k in range(len(B))]) for c in range(len(B[0]))] for r in range(len(A))]


def _matvec(A, x):
    return [_dot(row, x) for row in A]


def _tr(A):
    return [[A[r][c] for r in range(len(A))] for c in range(len(A[0]))]


def _hat(v):
    return [[ZERO, neg(v[2]), v[1]], [v[2], ZERO, neg(v[0])], [neg(v[1]), v[0], ZERO]]


def _mp_of(v):
    if isinstance(v, DD):
        return [mpmath.mpf(float(h)) + mpmath.mpf(float(l)) for h, l in zip(np.ravel(v.hi), np.ravel(v.lo))]
    return list(np.ravel(v.a))


def _mp_to(ys, T):
    if T is DD:
        hi = np.array([float(y) for y in ys])
        lo = np.array([float(y - mpmath.mpf(float(h))) for y, h in zip(ys, hi)])
        return DD(hi, lo)
    return MP(np.array(ys, dtype=object))


def _safe(df, a):
    try:
        return float(abs(df(*a)))
    except ZeroDivisionError:
        return np.inf


def _fn(xs, f, dfs, c):
    """y = f(x_0, ..) by mpmath on the exact arguments; M_y = max(|y|, sum |df/dx_i| M_i); k = max k_i + c"""
    T = type(xs[0].v)
    with mpmath.workprec(_PREC):
        args = list(zip(*[_mp_of(x.v) for x in xs]))
        ys = [f(*a) for a in args]
        cond = np.zeros(len(ys))
        for x, df in zip(xs, dfs):
            d = np.array([_safe(df, a) for a in args])
            cond = cond + np.where(x.m == 0.0, 0.0, d * np.where(x.m == 0.0, 1.0, x.m))   # (an exact argument has no conditioning)
        v = _mp_to(ys, T)
    return Tr(v, np.maximum(v.absf(), cond), max(x.k for x in xs) + c)


def _sqrt(x):
    return _fn([x], mpmath.sqrt, [lambda t: 1 / (2 * mpmath.sqrt(t))], 1)


def _sin(x):
    return _fn([x], mpmath.sin, [mpmath.cos], LIBM_ULP)


def _cos(x):
    return _fn([x], mpmath.cos, [mpmath.sin], LIBM_ULP)


# ------------------------------------------------------------------------------------------------ the so(3) functions of vba_hostmath.hpp
class _Ctx:
    """constants over V factors of value type T, and the branch variables met on the way"""

    def __init__(self, V, T):
        self.V, self.T = V, T
        self.ONE = _One(self.arr(np.ones(V)), np.ones(V), 0)
        self.one = self.inp(np.ones(V))                                    # the literal 1.0 of a sum
        self.half = self.inp(np.full(V, 0.5))
        self.branch = []                                                  # (name, kind, Tr value, threshold)

    def arr(self, a):
        return self.T.of(np.asarray(a, dtype=np.float64))

    def inp(self, a):
        a = np.asarray(a, dtype=np.float64)
        return Tr(self.arr(a), np.abs(a), 0)

    def eye(self):
        return [[self.ONE if r == c else ZERO for c in range(3)] for r in range(3)]

    def note(self, name, kind, value, thr):
        self.branch.append((name, kind, value, thr))


def _sq(x):
    """x * x as a function of ONE value: M = max(x^2, 2 |x| M_x), one more rounding (a product's rule M_x^2 forgets that both
    factors err together, and would hide a small norm behind the cancellation its components came from)"""
    if x.v is None:
        return ZERO
    a = x.v.absf()
    return Tr(x.v * x.v, np.maximum(a * a, 2 * a * x.m), x.k + 1)


def _norm3(w):
    s = ZERO
    for x in w:
        s = add(s, _sq(x))
    return _sqrt(s)


def _so3_exp(C, w, general):
    n = _norm3(w)
    C.note("so3_exp |w|", "ge", n, 1e-11)
    if not general:
        return C.eye()
    ax = [_cdiv(x, n) for x in w]
    K = _hat(ax)
    K2 = _matmul(K, K)
    s, c1 = _sin(n), sub(C.one, _cos(n))
    R = [[add(_mul(s, K[r][c]), _mul(c1, K2[r][c])) for c in range(3)] for r in range(3)]
    for i in range(3):
        R[i][i] = add(R[i][i], C.one)
    return R


def _so3_log(C, R, branch):
    tr = add(add(R[0][0], R[1][1]), R[2][2])
    C.note("so3_log 3 - tr", "gt_rev", sub(C.inp(np.full(C.V, 3.0)), tr), 1e-6)      # tr > 3 - 1e-6  <=>  3 - tr < 1e-6
    K = [sub(R[2][1], R[1][2]), sub(R[0][2], R[2][0]), sub(R[1][0], R[0][1])]
    if branch == "one":
        return [sc(k, 0.5) for k in K]
    x = sc(sub(tr, C.one), 0.5)
    th = _fn([x], mpmath.acos, [lambda t: 1 / mpmath.sqrt(1 - t * t)], LIBM_ULP)
    C.note("so3_log theta", "lt", th, 0.001)
    if branch == "half":
        return [sc(k, 0.5) for k in K]
    f = _fn([th], lambda t: t / (2 * mpmath.sin(t)), [lambda t: (mpmath.sin(t) - t * mpmath.cos(t)) / (2 * mpmath.sin(t) ** 2)],
            LIBM_ULP + 1)
    return [_mul(f, k) for k in K]


def _so3_jr(C, vec, general):
    ang = _norm3(vec)
    C.note("so3_jr |v|", "lt", ang, 1e-9)
    if not general:
        return C.eye()
    a = [_cdiv(x, ang) for x in vec]
    ra = _cdiv(_sin(ang), ang)
    k = _cdiv(sub(C.one, _cos(ang)), ang)
    H = _hat(a)
    om = sub(C.one, ra)
    return [[sub(add(ra if r == c else ZERO, _mul(_mul(om, a[r]), a[c])), _mul(k, H[r][c])) for c in range(3)] for r in range(3)]


def _angle_axis(C, m, quat, q0neg, nonzero):
    """Eigen::AngleAxisd(Matrix3d).  quat: 'pos' (trace > 0) or the index i of the largest diagonal entry"""
    t0 = add(add(m[0][0], m[1][1]), m[2][2])
    C.note("angle_axis trace", "sign", t0, 0.0)
    q = [None] * 4
    if quat == "pos":
        t = _sqrt(add(t0, C.one))
        q[0] = sc(t, 0.5)
        t2 = _cdiv(C.half, t)
        q[1] = _mul(sub(m[2][1], m[1][2]), t2); q[2] = _mul(sub(m[0][2], m[2][0]), t2); q[3] = _mul(sub(m[1][0], m[0][1]), t2)
    else:
        i = int(quat)
        C.note("angle_axis m11 - m00", "sign", sub(m[1][1], m[0][0]), 0.0)
        i1 = 1 if i == 1 else (0 if i == 0 else None)
        if i1 is None:                                                    # i == 2: the second comparison is against the first's winner
            C.note("angle_axis m22 - m00", "sign", sub(m[2][2], m[0][0]), 0.0)
            C.note("angle_axis m22 - m11", "sign", sub(m[2][2], m[1][1]), 0.0)
        else:
            C.note("angle_axis m22 - mii", "sign", sub(m[2][2], m[i1][i1]), 0.0)
        j, k = (i + 1) % 3, (i + 2) % 3
        t = _sqrt(add(sub(sub(m[i][i], m[j][j]), m[k][k]), C.one))
        q[1 + i] = sc(t, 0.5)
        t2 = _cdiv(C.half, t)
        q[0] = _mul(sub(m[k][j], m[j][k]), t2)
        q[1 + j] = _mul(add(m[j][i], m[i][j]), t2)
        q[1 + k] = _mul(add(m[k][i], m[i][k]), t2)
        C.note("angle_axis q0", "sign", q[0], 0.0)
    n = _norm3(q[1:])
    if not nonzero:
        return None, None, n
    aq0 = q[0] if not q0neg else neg(q[0])
    ang = sc(_fn([n, aq0], mpmath.atan2, [lambda y, x: x / (x * x + y * y), lambda y, x: y / (x * x + y * y)], LIBM_ULP), 2.0)
    ns = neg(n) if q0neg else n
    return ang, [_cdiv(x, ns) for x in q[1:]], n


def _so3_jr_inv(C, R, sig):
    quat, q0neg, mode = sig                                               # mode: 'n0' (|q_xyz| == 0), 'small' (< 1e-9), 'gen'
    ang, a, n = _angle_axis(C, R, quat, q0neg, mode != "n0")
    C.note("angle_axis |q_xyz| != 0", "zero" if mode == "n0" else "nonzero", n, 0.0)
    if mode == "n0":
        return C.eye()
    C.note("so3_jr_inv angle", "lt", ang, 1e-9)
    if mode == "small":
        return C.eye()
    ctt = _fn([ang], lambda t: (t / 2) / mpmath.tan(t / 2), [lambda t: (1 / mpmath.tan(t / 2) - (t / 2) / mpmath.sin(t / 2) ** 2) / 2],
              LIBM_ULP + 1)
    H = _hat(a)
    om, h2 = sub(C.one, ctt), sc(ang, 0.5)
    return [[add(add(ctt if r == c else ZERO, _mul(_mul(om, a[r]), a[c])), _mul(h2, H[r][c])) for c in range(3)] for r in range(3)]


# ------------------------------------------------------------------------------------------------ one factor: rr[15], joc[15][33]
O_RD, O_PD, O_VD, O_RBG, O_PBG, O_PBA, O_VBG, O_VBA, O_DT, O_DBG, O_DBA, O_COV = 0, 9, 12, 21, 30, 39, 48, 57, 66, 67, 70, 79


def factor_terms(imu, s1, s2, sig, T=DD):
    """rr [15] and joc [15][33] (Tr, vectors over the V factors given, which all take the branches `sig`) and the branch variables"""
    imu, s1, s2 = (np.asarray(a, dtype=np.float64) for a in (imu, s1, s2))
    V = len(imu)
    C = _Ctx(V, T)
    m3 = lambda a, o: [[C.inp(a[:, o + 3 * r + c]) for c in range(3)] for r in range(3)]
    v3 = lambda a, o: [C.inp(a[:, o + k]) for k in range(3)]
    Rd, Rbg, pbg, pba, vbg, vba = (m3(imu, o) for o in (O_RD, O_RBG, O_PBG, O_PBA, O_VBG, O_VBA))
    pd, vd, dbg, dba = v3(imu, O_PD), v3(imu, O_VD), v3(imu, O_DBG), v3(imu, O_DBA)
    dt = C.inp(imu[:, O_DT])
    R1, R2 = m3(s1, 1), m3(s2, 1)
    p1, v1, bg1, ba1, g1 = (v3(s1, o) for o in (10, 13, 16, 19, 22))
    p2, v2, bg2, ba2 = (v3(s2, o) for o in (10, 13, 16, 19))

    rb = _matvec(Rbg, dbg)
    Eb = _so3_exp(C, rb, sig["exp"])
    Rc = _matmul(Rd, Eb)
    a3, b3 = _matvec(pbg, dbg), _matvec(pba, dba)
    tc = [add(add(pd[i], a3[i]), b3[i]) for i in range(3)]
    a3, b3 = _matvec(vbg, dbg), _matvec(vba, dba)
    vc = [add(add(vd[i], a3[i]), b3[i]) for i in range(3)]
    res_r = _matmul(_tr(Rc), _matmul(_tr(R1), R2))
    hdt2 = _mul(sc(dt, 0.5), dt)                                          # 0.5 * dt * dt
    dv = [sub(sub(v2[i], v1[i]), _mul(dt, g1[i])) for i in range(3)]
    dp = [sub(sub(sub(p2[i], p1[i]), _mul(v1[i], dt)), _mul(hdt2, g1[i])) for i in range(3)]
    R1t = _tr(R1)
    exp_v, exp_t = _matvec(R1t, dv), _matvec(R1t, dp)
    lr = _so3_log(C, res_r, sig["log"])
    rr = lr + [sub(exp_t[i], tc[i]) for i in range(3)] + [sub(exp_v[i], vc[i]) for i in range(3)] \
        + [sub(bg2[i], bg1[i]) for i in range(3)] + [sub(ba2[i], ba1[i]) for i in range(3)]

    joc = [[ZERO] * 33 for _ in range(15)]

    def block(r0, c0, B, f=lambda x: x):
        for r in range(3):
            for c in range(3):
                joc[r0 + r][c0 + c] = f(B[r][c])

    JRi = _so3_jr_inv(C, res_r, sig["jrinv"])
    block(0, 0, _matmul(JRi, _matmul(_tr(R2), R1)), neg)
    block(0, 15, JRi)
    jrb = _so3_jr(C, rb, sig["jr"])
    block(0, 9, _matmul(_matmul(_matmul(JRi, _tr(res_r)), jrb), Rbg), neg)
    block(3, 0, _hat(exp_t))
    block(3, 3, R1t, neg)
    block(3, 6, R1t, lambda x: neg(_mul(dt, x)))
    block(3, 9, pbg, neg); block(3, 12, pba, neg)
    block(3, 18, R1t)
    block(6, 0, _hat(exp_v))
    block(6, 6, R1t, neg)
    block(6, 9, vbg, neg); block(6, 12, vba, neg)
    block(6, 21, R1t)
    I3 = C.eye()
    block(9, 9, I3, neg); block(12, 12, I3, neg); block(9, 24, I3); block(12, 27, I3)
    block(3, 30, R1t, lambda x: neg(_mul(hdt2, x)))
    block(6, 30, R1t, lambda x: neg(_mul(dt, x)))
    return rr, joc, C.branch


# ------------------------------------------------------------------------------------------------ branch signature in plain f64
def _np_hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def np_exp(w):
    n = np.linalg.norm(w)
    if n < 1e-11:
        return np.eye(3)
    K = _np_hat(w / n)
    return np.eye(3) + np.sin(n) * K + (1 - np.cos(n)) * K @ K


def np_jr(v):
    ang = np.linalg.norm(v)
    if ang < 1e-9:
        return np.eye(3)
    a = v / ang
    ra = np.sin(ang) / ang
    return ra * np.eye(3) + (1 - ra) * np.outer(a, a) - (1 - np.cos(ang)) / ang * _np_hat(a)


def np_res_r(imu, s1, s2):
    Rd, Rbg = imu[O_RD:O_RD + 9].reshape(3, 3), imu[O_RBG:O_RBG + 9].reshape(3, 3)
    rb = Rbg @ imu[O_DBG:O_DBG + 3]
    return (Rd @ np_exp(rb)).T @ (s1[1:10].reshape(3, 3).T @ s2[1:10].reshape(3, 3)), rb


def signature(imu, s1, s2):
    """the branches one factor takes, from a plain f64 evaluation (the margins asserted on the reference make it the reference's)"""
    m, rb = np_res_r(imu, s1, s2)
    nrb = np.linalg.norm(rb)
    tr = np.trace(m)
    if tr > 3.0 - 1e-6:
        lg = "one"
    else:
        lg = "half" if abs(np.arccos(0.5 * (tr - 1))) < 0.001 else "gen"
    if tr > 0:
        quat = "pos"
        qv = np.array([m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]]) * (0.5 / np.sqrt(tr + 1))
        q0 = 0.5 * np.sqrt(tr + 1)
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        qv = np.zeros(3)
        qv[i] = 0.5 * t
        q0 = (m[k, j] - m[j, k]) * (0.5 / t)
        qv[j] = (m[j, i] + m[i, j]) * (0.5 / t); qv[k] = (m[k, i] + m[i, k]) * (0.5 / t)
        quat = str(i)
    n = np.linalg.norm(qv)
    mode = "n0" if n == 0.0 else ("small" if 2 * np.arctan2(n, abs(q0)) < 1e-9 else "gen")
    return (bool(nrb >= 1e-11), lg, bool(nrb >= 1e-9), quat, bool(q0 < 0), mode)


def _sig_dict(s):
    return {"exp": s[0], "log": s[1], "jr": s[2], "jrinv": (s[3], s[4], s[5])}


# ------------------------------------------------------------------------------------------------ tracked arrays
class TA:
    """arrays of tracked values: v (DD or MP), shadow m, count k (int), exact-zero mask z"""
    __slots__ = ("v", "m", "k", "z")

    def __init__(self, v, m, k, z):
        self.v, self.m, self.k, self.z = v, m, k, z

    def __getitem__(self, ix):
        return TA(_vix(self.v, ix), self.m[ix], self.k[ix], self.z[ix])

    @property
    def shape(self):
        return self.m.shape

    def bar(self):
        return np.where(self.z, 0.0, self.k * U * self.m)


def _vix(v, ix):
    return DD(v.hi[ix], v.lo[ix]) if isinstance(v, DD) else MP(v.a[ix])


def _vzeros(T, shape):
    if T is DD:
        return DD(np.zeros(shape))
    a = np.empty(shape, dtype=object)
    a[...] = mpmath.mpf(0)
    return MP(a)


def _vset(v, ix, x):
    if isinstance(v, DD):
        v.hi[ix] = x.hi; v.lo[ix] = x.lo
    else:
        v.a[ix] = x.a


def ta_zero(T, shape):
    return TA(_vzeros(T, shape), np.zeros(shape), np.zeros(shape, dtype=np.int64), np.ones(shape, dtype=bool))


def ta_input(T, a):
    a = np.asarray(a, dtype=np.float64)
    if T is DD:
        v = DD(a.copy())
    else:
        with mpmath.workprec(_PREC):
            v = MP(np.array([mpmath.mpf(float(x)) for x in a.ravel()], dtype=object).reshape(a.shape))
    return TA(v, np.abs(a), np.zeros(a.shape, dtype=np.int64), np.zeros(a.shape, dtype=bool))


def ta_mul(a, b):
    z = a.z | b.z
    return TA(a.v * b.v, np.maximum(a.v.absf() * b.m, b.v.absf() * a.m), np.where(z, 0, a.k + b.k + 1), z)


def ta_add(a, b):
    k = np.where(a.z, b.k, np.where(b.z, a.k, np.maximum(a.k, b.k) + 1))
    return TA(a.v + b.v, a.m + b.m, k, a.z & b.z)


def _bc(a, shape):
    """a TA broadcast to `shape` (views)"""
    f = lambda x: np.broadcast_to(x, shape)
    v = DD(f(a.v.hi), f(a.v.lo)) if isinstance(a.v, DD) else MP(f(a.v.a))
    return TA(v, f(a.m), f(a.k), f(a.z))


def ta_contract(A, B, ka, kb):
    """sum over the paired axes ka of A and kb of B in ascending order, the other axes broadcast (both come with singleton axes in place)"""
    n = A.shape[ka]
    acc = None
    for i in range(n):
        ia = tuple(slice(i, i + 1) if d == ka else slice(None) for d in range(A.m.ndim))
        ib = tuple(slice(i, i + 1) if d == kb else slice(None) for d in range(B.m.ndim))
        t = ta_mul(A[ia], B[ib])
        acc = t if acc is None else ta_add(acc, t)
    return acc


# ------------------------------------------------------------------------------------------------ the reference over a set of windows
class Ref:
    """Reference of a list of windows [(states [W,25], imus [W-1,304], covinv [W-1,15,15])].  All factors are evaluated at once (grouped
    by the branches they take); window(i, gravity) assembles H, g, rimu of one window with their bars."""

    def __init__(self, windows, T=DD):
        self.T = T
        self.windows = windows
        self.off = np.concatenate([[0], np.cumsum([len(w[1]) for w in windows])]).astype(int)
        imu = np.concatenate([np.asarray(w[1], dtype=np.float64).reshape(-1, 304) for w in windows])
        s1 = np.concatenate([np.asarray(w[0], dtype=np.float64)[:-1] for w in windows])
        s2 = np.concatenate([np.asarray(w[0], dtype=np.float64)[1:] for w in windows])
        cinv = np.concatenate([np.asarray(w[2], dtype=np.float64).reshape(-1, 15, 15) for w in windows])
        NF = len(imu)
        self.NF = NF
        sigs = [signature(imu[f], s1[f], s2[f]) for f in range(NF)]
        self.sigs = sigs
        rr = ta_zero(T, (15, NF)); joc = ta_zero(T, (15, 33, NF))
        self.branch = []                                                  # (factor, name, kind, value f64, shadow bar, threshold)
        for sg in sorted(set(sigs)):
            idx = np.flatnonzero([s == sg for s in sigs])
            r_, j_, br = factor_terms(imu[idx], s1[idx], s2[idx], _sig_dict(sg), T)
            for k in range(15):
                self._put(rr, (k,), idx, r_[k])
                for c in range(33):
                    self._put(joc, (k, c), idx, j_[k][c])
            for name, kind, val, thr in br:
                x = val.v.f64() if val.v is not None else np.zeros(len(idx))
                for e, f in enumerate(idx):
                    self.branch.append((int(f), name, kind, float(x[e]), float(val.k * U * val.m[e]) if val.v is not None else 0.0, thr))
        self.rr, self.joc = rr, joc
        ci = ta_input(T, np.moveaxis(cinv, 0, -1))                        # [15, 15, NF]
        # cj[r, c] = sum_k2 cinv[r, k2] joc[k2, c];  cr[r] = sum_k2 cinv[r, k2] rr[k2]
        self.cj = ta_contract(self._ax(ci, (0, 1, None)), self._ax(joc, (None, 0, 1)), 1, 1)[:, 0]
        self.cr = ta_contract(ci, self._ax(rr, (None, 0)), 1, 1)[:, 0]
        self.q = ta_contract(rr, self.cr, 0, 0)[0]
        # jtj[lr, lc] = sum_k joc[k, lr] cj[k, lc];  gg[lr] = sum_k joc[k, lr] cr[k]
        self.jtj = ta_contract(self._ax(joc, (0, 1, None)), self._ax(self.cj, (0, None, 1)), 0, 0)[0]
        self.gg = ta_contract(joc, self._ax(self.cr, (0, None)), 0, 0)[0]

    @staticmethod
    def _ax(a, spec):
        """insert singleton axes: spec lists, per output axis, the source axis or None; the factor axis stays last"""
        ix = tuple(slice(None) if s is not None else None for s in spec) + (slice(None),)
        f = lambda x: x[ix]
        v = DD(f(a.v.hi), f(a.v.lo)) if isinstance(a.v, DD) else MP(f(a.v.a))
        return TA(v, f(a.m), f(a.k), f(a.z))

    def _put(self, dst, pos, idx, t):
        if t.v is None:
            return
        ix = pos + (idx,)
        _vset(dst.v, ix, t.v)
        dst.m[ix] = t.m; dst.k[ix] = t.k; dst.z[ix] = False

    # ---- what the code keeps
    def counts(self):
        mx = lambda a: int(a.k[~a.z].max()) if (~a.z).any() else 0
        return dict(D_RR=mx(self.rr), D_JOC=mx(self.joc), D_CJ=mx(self.cj), D_HF=mx(self.jtj), D_GF=mx(self.gg), D_QF=mx(self.q))

    def margins(self):
        """violations of the corpus condition: every branch variable a factor 1 +- MARGIN (absolute MARGIN for a sign test, and for the
        sums it is formed from) away from its threshold, with the value's own error bar far inside that margin"""
        bad = []
        for f, name, kind, x, bar, thr in self.branch:
            if kind in ("ge", "lt", "gt_rev"):
                ok = not (thr * (1 - MARGIN) <= x <= thr * (1 + MARGIN)) and bar < 1e-3 * abs(x - thr)
            elif kind == "sign":
                ok = abs(x) > MARGIN and bar < 1e-3 * abs(x)
            elif kind == "zero":
                ok = x == 0.0 and bar == 0.0
            else:                                                         # (n != 0.0: any non-zero value is a factor away from 0)
                ok = abs(x) > 0.0
            if not ok:
                bad.append((f, name, x, bar, thr))
        return bad

    def branch_consistent(self):
        """the f64 signature is the one the reference's own branch variables select"""
        bad = []
        for f, name, kind, x, bar, thr in self.branch:
            s = self.sigs[f]
            want = None
            if name == "so3_exp |w|":
                want, got = s[0], x >= thr
            elif name == "so3_jr |v|":
                want, got = s[2], not (x < thr)
            elif name == "so3_log 3 - tr":
                want, got = s[1] == "one", x < thr
            elif name == "so3_log theta":
                want, got = s[1] == "half", abs(x) < thr
            elif name == "angle_axis trace":
                want, got = s[3] == "pos", x > 0
            elif name == "so3_jr_inv angle":
                want, got = s[5] == "small", x < thr
            if want is not None and want != got:
                bad.append((f, name, x, s))
        return bad

    # ---- per factor
    def factor(self, f, gravity):
        nb = 33 if gravity else 30
        return dict(rr=self.rr[:, f], joc=self.joc[:, :nb, f], jtj=self.jtj[:nb, :nb, f], gg=self.gg[:nb, f], q=self.q[f])

    # ---- per window
    def window(self, i, gravity):
        """(H, g, rimu) as TA of shapes [n, n], [n], [] for window i"""
        states = self.windows[i][0]
        W = len(states)
        f0 = self.off[i]
        F = W - 1
        n = 15 * W + (3 if gravity else 0)
        H = ta_zero(self.T, (n, n)); g = ta_zero(self.T, (n,))

        def put(dst, ix, src):
            _vset(dst.v, ix, src.v); dst.m[ix] = src.m; dst.k[ix] = src.k; dst.z[ix] = src.z

        def blk(f, r0, c0, nr, nc):
            return self.jtj[r0:r0 + nr, c0:c0 + nc, f0 + f]

        def sum_f(terms):
            acc = None
            for t in terms:
                acc = t if acc is None else ta_add(acc, t)
            return acc

        for a in range(W):
            fs = [(f, 15 if f == a - 1 else 0) for f in (a - 1, a) if 0 <= f < F]
            put(H, (slice(15 * a, 15 * a + 15), slice(15 * a, 15 * a + 15)), sum_f([blk(f, o, o, 15, 15) for f, o in fs]))
            put(g, (slice(15 * a, 15 * a + 15),), sum_f([self.gg[o:o + 15, f0 + f] for f, o in fs]))
            if a + 1 < W:
                put(H, (slice(15 * a, 15 * a + 15), slice(15 * a + 15, 15 * a + 30)), blk(a, 0, 15, 15, 15))
                put(H, (slice(15 * a + 15, 15 * a + 30), slice(15 * a, 15 * a + 15)), blk(a, 15, 0, 15, 15))
            if gravity:
                put(H, (slice(15 * a, 15 * a + 15), slice(15 * W, n)), sum_f([blk(f, o, 30, 15, 3) for f, o in fs]))
                put(H, (slice(15 * W, n), slice(15 * a, 15 * a + 15)), sum_f([blk(f, 30, o, 3, 15) for f, o in fs]))
        if gravity:
            put(H, (slice(15 * W, n), slice(15 * W, n)), sum_f([blk(f, 30, 30, 3, 3) for f in range(F)]))
            put(g, (slice(15 * W, n),), sum_f([self.gg[30:33, f0 + f] for f in range(F)]))
        rimu = sum_f([self.q[f0 + f] for f in range(F)])
        return H, g, rimu


def ratio(ref, got):
    """largest |got - ref| / bar of a TA against doubles, and inf where an exact-zero entry (bar 0) is not 0 / anything is not finite"""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return np.inf
    bar = ref.bar()
    err = ref.v.err_to(got)
    z = bar == 0.0
    if np.any(err[z] != 0.0):
        return np.inf
    return float((err[~z] / bar[~z]).max()) if np.any(~z) else 0.0


def check(Ht, gt, rt, H, g, rimu0, rimu1=None):
    out = {"H": ratio(Ht, H), "g": ratio(gt, g), "rimu0": ratio(rt, np.float64(rimu0))}
    if rimu1 is not None:
        out["rimu1"] = ratio(rt, np.float64(rimu1))
    return out


def pattern_mask(W, gravity):
    """True where the dense matrix may be non-zero"""
    n = 15 * W + (3 if gravity else 0)
    a = np.arange(n) // 15
    m = np.abs(a[:, None] - a[None, :]) <= 1
    if gravity:
        m[15 * W:, :] = True; m[:, 15 * W:] = True
    return m


# ------------------------------------------------------------------------------------------------ corpus
NM = np.array([0.01] * 3 + [1.0] * 3)
NW = np.array([1e-4] * 6)
DTS = (0.1, 0.01, 1.0)
G = np.array([0.0, 0.0, -9.8])
SMALL = (1e-10, 1e-7, 5e-4, 2e-3, 0.0)                                    # 0.0: exactly the identity, by construction
BIG = (1.0, 1.7, 2.5, 2.9, 2.2)
_MIX = ("consistent", "offset", "bigangle", "smallangle", "far")
_PERM = (np.array([[0., -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[1., 0, 0], [0, 0, -1], [0, 1, 0]]),
         np.array([[0., 0, 1], [0, 1, 0], [-1, 0, 0]]))


def _unit(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def make_window(cls, W, seed=20261019):
    """states [W,25], imus [W-1,304] of one window of class `cls`: consistent (residual at noise level), offset (rotation 0.01..0.3 rad, 0.1 m,
    0.1 m/s, biases and dbg / dba at 1e-3..1e-2, so Exp(R_bg dbg), jr(rb) and the R_bg / p_bg / v_bg columns are live), bigangle (residual
    rotation BIG, below 3 rad: the axis formula degrades at pi by design), smallangle (SMALL; 0.0 = the identity in every bit, from signed
    permutation matrices), far (|p| = 1e3 m, |v| = 30 m/s: the cancellation in dp), mixed (each factor from another class).  dtime cycles
    over DTS inside a window."""
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    rng = np.random.default_rng(seed + 1000 * CLASSES.index(cls) + W)
    F = W - 1
    states = np.zeros((W, 25)); imus = np.zeros((F, 304))
    far = cls == "far"
    R = hr._rot(rng)
    p = _unit(rng) * (1e3 if far else 3.0)
    v = _unit(rng) * (30.0 if far else 1.0)
    bias = lambda: rng.uniform(1e-3, 1e-2, 3) * rng.choice([-1.0, 1.0], 3)
    bg, ba = (bias(), bias()) if cls in ("offset", "mixed") else (np.zeros(3), np.zeros(3))
    t = 0.0
    states[0] = np.concatenate([[t], R.ravel(), p, v, bg, ba, G])
    for f in range(F):
        kind = _MIX[f % 5] if cls == "mixed" else cls
        dt = DTS[(f + W) % 3]
        wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=F + 1, seed=seed + 31 * W + f)
        ts, gy, ac = synth.make_imu(wl, scan_dt=dt, gyr_sigma=1e-3, acc_sigma=1e-2)[0][f]
        im = capi.imu_preintegrate(ts, gy, ac, bg, ba, NM, NW)
        live = kind == "offset"
        if live:
            im[O_DBG:O_DBG + 3] = bias(); im[O_DBA:O_DBA + 3] = bias()
        var = (f + W) % 5
        exact = kind == "smallangle" and SMALL[var] == 0.0
        if exact:                                                         # exactly representable rotations: res_r = I in every bit
            P = _PERM[(f + W) % 3]
            im[O_RD:O_RD + 9] = P.ravel()
            R = _PERM[(f + W + 1) % 3].copy()
            states[f, 1:10] = R.ravel()
        Rc = im[O_RD:O_RD + 9].reshape(3, 3) @ np_exp(im[O_RBG:O_RBG + 9].reshape(3, 3) @ im[O_DBG:O_DBG + 3])
        tc = im[O_PD:O_PD + 3] + im[O_PBG:O_PBG + 9].reshape(3, 3) @ im[O_DBG:O_DBG + 3] + im[O_PBA:O_PBA + 9].reshape(3, 3) @ im[O_DBA:O_DBA + 3]
        vc = im[O_VD:O_VD + 3] + im[O_VBG:O_VBG + 9].reshape(3, 3) @ im[O_DBG:O_DBG + 3] + im[O_VBA:O_VBA + 9].reshape(3, 3) @ im[O_DBA:O_DBA + 3]
        if kind == "offset":
            ang, dpn, dvn = rng.uniform(0.01, 0.3), 0.1, 0.1
        elif kind == "bigangle":
            ang, dpn, dvn = BIG[var], 0.01, 0.01
        elif kind == "smallangle":
            ang, dpn, dvn = SMALL[var], 1e-3, 1e-3
        else:
            ang, dpn, dvn = 3e-3, 1e-3, 1e-3
        R2 = R @ Rc if exact else R @ Rc @ np_exp(ang * _unit(rng))
        p2 = p + v * dt + 0.5 * dt * dt * G + R @ (tc + dpn * _unit(rng))
        v2 = v + dt * G + R @ (vc + dvn * _unit(rng))
        if kind == "offset" or cls == "mixed":
            bg, ba = bias(), bias()
        t += dt
        states[f + 1] = np.concatenate([[t], R2.ravel(), p2, v2, bg, ba, G])
        imus[f] = im
        R, p, v = R2, p2, v2
    return states, imus


def host_covinv(imus):
    """cov^-1 of every factor as the host inverts it (inverse_pplu through the g++ build of the header: tests/host/imu_host.cpp)"""
    lib = host_lib()
    out = np.zeros((len(imus), 15, 15))
    for f in range(len(imus)):
        lib.imu_host_covinv(_p(np.ascontiguousarray(imus[f])), _p(out[f]))
    return out


_LIB = None


def _p(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_double))


def host_lib():
    """tests/host/imu_host.cpp built by g++ -O2 -ffp-contract=off over csrc/vba_hostmath.hpp (cached per process, rebuilt when older)"""
    global _LIB
    if _LIB is None:
        import ctypes as C
        import os
        import subprocess
        import tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        src = os.path.join(root, "tests", "host", "imu_host.cpp")
        out = os.path.join(tempfile.mkdtemp(prefix="imu_host_"), "libimu_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(root, "voxel-slam_amd", "csrc"),
                               src, "-o", out])
        _LIB = C.CDLL(out)
    return _LIB


_IN, _WIN, _REF = {}, {}, {}


def inputs(cls, W):
    """states, imus of the corpus window (cls, W)"""
    if (cls, W) not in _IN:
        _IN[(cls, W)] = make_window(cls, W)
    return _IN[(cls, W)]


def window(cls, W):
    """states, imus, cov^-1 by the g++ build (the CPU companion; the device test takes cov^-1 from the hook)"""
    if (cls, W) not in _WIN:
        st, im = inputs(cls, W)
        _WIN[(cls, W)] = (st, im, host_covinv(im))
    return _WIN[(cls, W)]


def corpus_ref(ws=WS, classes=CLASSES):
    """one reference over every (class, W) window of the corpus; index(cls, W) finds a window in it"""
    key = (tuple(ws), tuple(classes))
    if key not in _REF:
        keys = [(c, W) for c in classes for W in ws]
        _REF[key] = (Ref([window(c, W) for c, W in keys]), {k: i for i, k in enumerate(keys)})
    return _REF[key]


# ------------------------------------------------------------------------------------------------ host evaluation and the model of the kernel's assembly
def host_factor(imu, s1, s2, cinv, gravity):
    """rr, joc, jtj, gg, q of one factor by the g++ build of the header"""
    import ctypes as C
    lib = host_lib()
    lib.imu_host_eval.restype = C.c_double
    nb = 33 if gravity else 30
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (imu, s1, s2, cinv)]
    rr = np.zeros(15); joc = np.zeros((15, nb)); jtj = np.zeros((nb, nb)); gg = np.zeros(nb)
    lib.imu_host_rj(_p(a[0]), _p(a[1]), _p(a[2]), int(gravity), _p(rr), _p(joc))
    q = lib.imu_host_eval(_p(a[0]), _p(a[1]), _p(a[2]), int(gravity), _p(a[3]), _p(jtj), _p(gg))
    return dict(rr=rr, joc=joc, jtj=jtj, gg=gg, q=q)


def np_factor(joc, rr, cinv):
    """jtj, gg, q from a (possibly altered) Jacobian in plain numpy f64 (the teeth: the order of the sums is numpy's)"""
    cj = cinv @ joc
    cr = cinv @ rr
    return dict(rr=rr, joc=joc, jtj=joc.T @ cj, gg=joc.T @ cr, q=float(rr @ cr))


def tile_block(joc_flat, cj_flat, f, nb, ro, co, poison=None):
    """numpy model of the matrix-core loop of li_imu_body for one factor of one block: 64 lanes (m = lane & 15, kq = lane >> 4), four
    16 x 16 x 4 steps over k = 0..15 with the 16th k padded with zeros; lane 15 of a row reads a neighbour (its products only reach the
    discarded row / column 15).  joc_flat / cj_flat: the LDS images [F][15][nb] (+ slack).  poison = (m0, n0): the padded k-slice holds
    1.0 at row m0 of the first operand and column n0 of the second.  Returns the 15 x 15 block."""
    acc = np.zeros((16, 16))
    jf = f * 15 * nb + ro
    cf = f * 15 * nb + co
    m = np.arange(16)
    for k0 in range(0, 16, 4):
        for kq in range(4):
            k = k0 + kq
            av = joc_flat[jf + k * nb + m] if k < 15 else np.zeros(16)
            bv = cj_flat[cf + k * nb + m] if k < 15 else np.zeros(16)
            if k == 15 and poison is not None:
                av = av.copy(); bv = bv.copy()
                av[poison[0]] = 1.0; bv[poison[1]] = 1.0
            acc = acc + np.outer(av, bv)
    return acc[:15, :15]


def model_assemble(W, gravity, facs, tooth=None):
    """The window assembly of li_imu_body over per-factor results facs[f] = dict(jtj, gg, q), in the kernel's order: the block pairs pr
    -> (a, b) with the <= 2 factors of a diagonal block in passes 0 / 1, the gravity border u1 / u2 and the corner over all factors,
    the gradient, rimu; written into the compact image and read back through li_hb_get (the g++ build).  tooth: one of the defects of
    tests/test_imu_cpu.py.  Returns dense H [n, n], g [n], rimu."""
    F = W - 1
    n = 15 * W + (3 if gravity else 0)
    lib = host_lib()
    hb = np.zeros(lib.li_hb_size_host(W, 1))
    ne1 = lib.li_hb_ne1_host(W)
    jt = lambda f: facs[f]["jtj"]
    for pr in range(3 * W - 2):
        a = (pr + 1) // 3
        b = a + ((pr + 1) % 3) - 1
        acc = np.zeros((15, 15))
        for ps in range(2):
            if b == a:
                f, ro, co = (a - 1, 15, 15) if ps == 0 else (a, 0, 0)
                if ps == 1 and tooth == "drop_second_factor":
                    continue
            elif b == a + 1:
                if ps:
                    continue
                f, ro, co = a, 0, 15
            else:
                if ps:
                    continue
                f, ro, co = b, 15, 0
            if f < 0 or f >= F:
                continue
            acc = acc + jt(f)[ro:ro + 15, co:co + 15]
        o = lib.li_hb_pair_host(a, b)
        hb[o:o + 225] = acc.ravel()
    if tooth == "swap_offdiag":
        for a in range(W - 1):
            o1, o2 = lib.li_hb_pair_host(a, a + 1), lib.li_hb_pair_host(a + 1, a)
            t = hb[o1:o1 + 225].copy(); hb[o1:o1 + 225] = hb[o2:o2 + 225]; hb[o2:o2 + 225] = t
    g = np.zeros(n)
    if gravity:
        for R in range(15 * W):
            a, r = divmod(R, 15)
            for k in range(3):
                u1 = u2 = 0.0
                if a >= 1:
                    u1 += jt(a - 1)[15 + r, 30 + k]; u2 += jt(a - 1)[30 + k, 15 + r]
                if a <= W - 2:
                    u1 += jt(a)[r, 30 + k]; u2 += jt(a)[30 + k, r]
                if tooth == "swap_u1_u2":
                    u1, u2 = u2, u1
                hb[ne1 + R * 3 + k] = u1
                hb[ne1 + 45 * W + (R * 3 + k if tooth == "u2_in_u1_layout" else k * 15 * W + R)] = u2
        for r in range(3):
            for k in range(3):
                acc = 0.0
                for f in range(F - 1 if tooth == "corner_misses_last" else F):
                    acc += jt(f)[30 + r, 30 + k]
                hb[ne1 + 90 * W + 3 * r + k] = acc
    for t in range(n):
        acc = 0.0
        if t < 15 * W:
            a, r = divmod(t, 15)
            if a >= 1:
                acc += facs[a - 1]["gg"][15 + r]
            if a <= W - 2 and not (tooth == "drop_gradient" and a == 0):
                acc += facs[a]["gg"][r]
        else:
            for f in range(F):
                acc += facs[f]["gg"][30 + (t - 15 * W)]
        g[t] = acc
    rimu = 0.0
    for f in range(F):
        rimu += facs[f]["q"]
    H = np.zeros((n, n))
    lib.li_hb_dense_host(_p(hb), W, n, _p(H))
    return H, g, rimu
