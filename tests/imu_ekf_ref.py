"""High-precision reference, magnitude shadow, rounding counts, bars, corpus and f64 model for the IMU forward propagation
(vbh::imu_ekf_propagate of csrc/vba_imu_ekf.hpp: IMUEKF::motion_blur, ekf_imu.hpp:54-123, "EK").  A helper shared by
tests/test_imu_ekf_cpu.py (the g++ build of the very header, the teeth) and tests/test_gpu_odom_state.py (the device, through
vba_odom_state_propagate).  No GPU code; nothing outside the repository is read.

Reference.  The literal formulas of EK:54-123 on the doubles the code reads, in the order the header states them (F_x by its five
blocks: the dense product without its exact zeros), with the branches of the reference project kept: Exp(w, dt) is the identity when
|w| <= 1e-7 (TL:68-84), the interval is skipped when its tail lies before last_pcl_end_time, cur_time is clamped, note = +-1.  Every
value is an mpmath number at 200 bits; sqrt, sin and cos are evaluated by mpmath on the exact value of their argument.

Magnitude shadow M and rounding count k (u = 2^-53), the rules of tests/imu_ref.py on scalars:
  * an input: M = |x|, k = 0;
  * a + b:  M = M_a + M_b, k = max(k_a, k_b) + 1.  When BOTH operands are exact (k = 0: two time stamps) the sum is one correctly
    rounded operation on exact numbers: M = |a + b|, k = 1, and k = 0 when the sum is a double itself (dt = tail - cur_time between
    neighbouring stamps: checked, not assumed);
  * a * b:  M = max(|a| M_b, |b| M_a), k = k_a + k_b + 1;  a / b:  M = max(M_a / |b|, |a| M_b / b^2), k = k_a + k_b + 1;
  * x * x:  M = max(x^2, 2 |x| M_x), k = k_x + 1;
  * y = f(x):  M = max(|y|, |f'(x)| M_x), k = k_x + c, with c = 1 for sqrt and c = LIBM_ULP = 4 for sin and cos (imu_ref's stated
    fallback for the two math libraries, the host's and the device's);
  * an exact +-1, 0.5, a sign change: free.
Bar of an output entry:  |x^ - x*| <= k u M (1 + MARGIN), MARGIN = 1e-3 for the f64 arithmetic of the shadow itself.  An entry with
M = 0 must be exactly 0.  Every bound is counted; nothing is tuned to a measured value.  The counts grow with the recursion (the
rotation gains one Exp and one 3 x 3 product per interval, P two sparse products): the largest per quantity over the corpus are
printed by the tests, not pinned.

What cannot be counted: a branch.  The stamps' comparisons are exact.  The one computed branch variable is the gyro norm against
1e-7; the reference REFUSES a case whose norm lies within its own bar of the threshold (assert), so no case of the corpus has an
unclear branch and nothing is excluded from the comparison (excluded share 0)."""
import mpmath
import numpy as np

U = 2.0 ** -53
LIBM_ULP = 4
MARGIN = 1e-3
_PREC = 200
mpf = mpmath.mpf


class X:
    """value v (mpf), magnitude shadow m (float), rounding count k"""
    __slots__ = ("v", "m", "k")

    def __init__(self, v, m, k):
        self.v, self.m, self.k = v, m, k

    def __add__(a, b):
        v = a.v + b.v
        if a.k == 0 and b.k == 0:
            f = float(v)
            return X(v, abs(f), 0 if mpf(f) == v else 1)
        return X(v, a.m + b.m, max(a.k, b.k) + 1)

    def __sub__(a, b):
        return a + (-b)

    def __neg__(a):
        return X(-a.v, a.m, a.k)

    def __mul__(a, b):
        return X(a.v * b.v, max(abs(float(a.v)) * b.m, abs(float(b.v)) * a.m), a.k + b.k + 1)

    def __truediv__(a, b):
        ab = abs(float(b.v))
        return X(a.v / b.v, max(a.m / ab, abs(float(a.v)) * b.m / ab ** 2), a.k + b.k + 1)

    def half(a):
        return X(a.v / 2, a.m / 2, a.k)

    def sq(a):
        f = abs(float(a.v))
        return X(a.v * a.v, max(f * f, 2 * f * a.m), a.k + 1)

    def fn(a, f, df, c):
        y = f(a.v)
        return X(y, max(abs(float(y)), abs(float(df(a.v))) * a.m), a.k + c)

    @property
    def bar(a):
        return a.k * U * a.m * (1 + MARGIN)


def inp(x):
    return X(mpf(float(x)), abs(float(x)), 0)


def _vec(a):
    return [inp(x) for x in np.ravel(a)]


def _mat3(a):
    a = np.reshape(a, (3, 3))
    return [[inp(a[r, c]) for c in range(3)] for r in range(3)]


def _dot3(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def _mm(A, B):
    return [[_dot3(A[r], [B[0][c], B[1][c], B[2][c]]) for c in range(3)] for r in range(3)]


def _mv(A, x):
    return [_dot3(A[r], x) for r in range(3)]


ONE, ZERO = inp(1.0), inp(0.0)


def _hat(v):
    return [[ZERO, -v[2], v[1]], [v[2], ZERO, -v[0]], [-v[1], v[0], ZERO]]


def _exp_dt(w, dt):
    """so3_exp_dt of vba_hostmath.hpp (TL:68-84): identity unless |w| > 1e-7; None stands for the exact identity"""
    n = (w[0].sq() + w[1].sq() + w[2].sq()).fn(mpmath.sqrt, lambda t: 1 / (2 * mpmath.sqrt(t)) if t else mpf(0), 1)
    assert abs(float(n.v) - 1e-7) > n.bar, "gyro norm within its bar of the 1e-7 branch: the case has no reference"
    if not float(n.v) > 1e-7:
        return None
    ax = [x / n for x in w]
    th = n * dt
    K = _hat(ax)
    K2 = _mm(K, K)
    s = th.fn(mpmath.sin, mpmath.cos, LIBM_ULP)
    c1 = ONE - th.fn(mpmath.cos, mpmath.sin, LIBM_ULP)
    R = [[s * K[r][c] + c1 * K2[r][c] for c in range(3)] for r in range(3)]
    for r in range(3):
        R[r][r] = R[r][r] + ONE
    return R


def reference(case):
    """dict of object arrays of X: state [25], cov [225], poses [n][22], end_pose [12]; and n"""
    with mpmath.workprec(_PREC):
        return _reference(case)


def _reference(case):
    m, imu = case["m"], np.asarray(case["imu"], dtype=np.float64).reshape(-1, 7)
    last_end, beg, end = (inp(case[k]) for k in ("last_end", "beg", "end"))
    sg = inp(case["sg"])
    noise = _vec(case["noise"])
    cov_gyr, cov_acc, cov_bg, cov_ba = noise[0:3], noise[3:6], noise[6:9], noise[9:12]
    st = np.asarray(case["state"], dtype=np.float64)
    R, p, v = _mat3(st[1:10]), _vec(st[10:13]), _vec(st[13:16])
    bg, ba, g = _vec(st[16:19]), _vec(st[19:22]), _vec(st[22:25])
    P = [_vec(row) for row in np.reshape(case["cov"], (15, 15))]
    rows = []
    wv = acc = None
    for j in range(m - 1):
        head, tail = _vec(imu[j]), _vec(imu[j + 1])
        if imu[j + 1, 0] < case["last_end"]:
            continue
        wv = [(head[1 + k] + tail[1 + k]).half() - bg[k] for k in range(3)]
        av = [(head[4 + k] + tail[4 + k]).half() * sg - ba[k] for k in range(3)]
        cur = head[0] if not imu[j, 0] < case["last_end"] else last_end
        dt = tail[0] - cur
        Ef, Em = _exp_dt(wv, dt), _exp_dt(wv, -dt)
        acc = [a + b for a, b in zip(_mv(R, av), g)]
        rows.append([cur - beg] + [R[r][c] for r in range(3) for c in range(3)] + p + v + wv + acc)
        # F_x blocks and P <- F P F^T + cov_w
        H = _hat(av)
        nR = [[-R[r][c] for c in range(3)] for r in range(3)]
        A = [[x * dt for x in row] for row in _mm(nR, H)]
        B = [[x * dt for x in row] for row in nR]
        Emm = Em if Em is not None else [[ONE if r == c else ZERO for c in range(3)] for r in range(3)]
        ndt = -dt
        T = [[None] * 15 for _ in range(15)]
        for i in range(15):
            for c in range(15):
                if i < 3:
                    s = Emm[i][0] * P[0][c] + Emm[i][1] * P[1][c] + Emm[i][2] * P[2][c] + ndt * P[9 + i][c]
                elif i < 6:
                    s = P[i][c] + dt * P[i + 3][c]
                elif i < 9:
                    a_, b_ = A[i - 6], B[i - 6]
                    s = a_[0] * P[0][c] + a_[1] * P[1][c] + a_[2] * P[2][c] + P[i][c]
                    s = s + b_[0] * P[12][c] + b_[1] * P[13][c] + b_[2] * P[14][c]
                else:
                    s = P[i][c]
                T[i][c] = s
        Pn = [[None] * 15 for _ in range(15)]
        for i in range(15):
            t = T[i]
            for c in range(15):
                if c < 3:
                    s = t[0] * Emm[c][0] + t[1] * Emm[c][1] + t[2] * Emm[c][2] + t[9 + c] * ndt
                elif c < 6:
                    s = t[c] + t[c + 3] * dt
                elif c < 9:
                    a_, b_ = A[c - 6], B[c - 6]
                    s = t[0] * a_[0] + t[1] * a_[1] + t[2] * a_[2] + t[c]
                    s = s + t[12] * b_[0] + t[13] * b_[1] + t[14] * b_[2]
                else:
                    s = t[c]
                if i < 3 and c == i:
                    s = s + cov_gyr[i] * dt * dt
                elif 6 <= i < 9 and 6 <= c < 9:
                    a6, b6 = i - 6, c - 6
                    s = s + (R[a6][0] * cov_acc[0] * R[b6][0] + R[a6][1] * cov_acc[1] * R[b6][1] + R[a6][2] * cov_acc[2] * R[b6][2]) * dt * dt
                elif i >= 9 and c == i:
                    s = s + (cov_bg[i - 9] if i < 12 else cov_ba[i - 12]) * dt * dt
                Pn[i][c] = s
        P = Pn
        # position, velocity, rotation (EK:108-110)
        p = [p[k] + v[k] * dt + acc[k].half() * dt * dt for k in range(3)]
        v = [v[k] + acc[k] * dt for k in range(3)]
        if Ef is not None:
            R = _mm(R, Ef)
    assert rows, "no interval left: the call refuses this case"
    imu_end = inp(imu[m - 1, 0])
    pos = case["end"] > imu[m - 1, 0]
    dt = (end - imu_end) if pos else -(end - imu_end)
    sgn = (lambda x: x) if pos else (lambda x: -x)
    E = _exp_dt([sgn(x) for x in wv], dt)
    Re = _mm(R, E) if E is not None else R
    ve = [v[k] + sgn(acc[k]) * dt for k in range(3)]
    pe = [p[k] + sgn(v[k]) * dt + sgn(acc[k].half()) * dt * dt for k in range(3)]
    Rf = [Re[r][c] for r in range(3) for c in range(3)]
    state = [end] + Rf + pe + ve + bg + ba + g
    return dict(n=len(rows), state=state, cov=[x for row in P for x in row], poses=rows, end_pose=Rf + pe)


def ratios(ref, got):
    """worst |got - ref| / bar per quantity (inf when an entry with bar 0 differs), with the largest k met"""
    out = {}
    with mpmath.workprec(_PREC):
        for name in ("state", "cov", "poses", "end_pose"):
            r = ref[name] if name != "poses" else [x for row in ref["poses"] for x in row]
            a = np.ravel(np.asarray(got[name], dtype=np.float64))[:len(r)]
            worst, kmax = 0.0, 0
            for x, y in zip(r, a):
                err = abs(float(mpf(float(y)) - x.v))
                bar = x.bar
                q = (0.0 if err == 0.0 else np.inf) if bar == 0.0 else err / bar
                if not np.isfinite(y):
                    q = np.inf
                worst, kmax = max(worst, q), max(kmax, x.k)
            out[name] = (worst, kmax)
    return out


# ------------------------------------------------------------------------------------------------ corpus
NOISE = np.array([0.01] * 3 + [0.1] * 3 + [1e-4] * 3 + [1e-4] * 3)


def _so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _case(rng, m, t, last_end, end, sg=1.0, gyro=0.3, zero_bias=False):
    imu = np.zeros((m, 7))
    imu[:, 0] = t
    imu[:, 1:4] = rng.normal(0, gyro, (m, 3))
    imu[:, 4:7] = (rng.normal(0, 0.5, (m, 3)) + np.array([0.2, -0.1, 9.8])) / (9.8 if sg != 1.0 else 1.0)
    st = np.zeros(25)
    st[0] = last_end
    st[1:10] = _so3(rng.normal(0, 0.4, 3)).ravel()
    st[10:13] = rng.normal(0, 2, 3); st[13:16] = rng.normal(0, 1, 3)
    st[16:19] = 0 if zero_bias else rng.normal(0, 0.01, 3)
    st[19:22] = rng.normal(0, 0.05, 3); st[22:25] = [0.05, -0.02, -9.8]
    A = rng.normal(0, 1, (15, 15))
    cov = 1e-5 * (A @ A.T) / 15 + np.diag([1e-4] * 9 + [1e-5] * 6)
    return dict(m=m, imu=imu, last_end=float(last_end), beg=float(last_end) + 0.0004, end=float(end), noise=NOISE.copy(), sg=float(sg), state=st,
                cov=cov.ravel())


def corpus():
    """name -> case.  m = 6 (the fewest rows sync_packages lets through, plus last_imu), 21 and 64; an interval straddling
    last_pcl_end_time in every case, intervals wholly before it (m21, m64); pcl_end_time beyond (m6, m64, still) and before (m21,
    repeat) the last stamp; a gyro norm below 1e-7 (still); a repeated stamp (repeat); scale_gravity 9.8 (m21)."""
    rng = np.random.default_rng(20)
    c = {}
    t = 10.0 + 0.005 * np.arange(6)
    c["m6"] = _case(rng, 6, t, 10.002, t[-1] + 0.003)
    t = 20.0 + 0.005 * np.arange(21)
    c["m21"] = _case(rng, 21, t, t[3] + 0.001, t[-1] - 0.002, sg=9.8)
    t = 30.0 + 0.0016 * np.arange(64)
    c["m64"] = _case(rng, 64, t, t[2] + 0.0007, t[-1] + 0.0011)
    t = 40.0 + 0.005 * np.arange(6)
    c["still"] = _case(rng, 6, t, 40.001, t[-1] + 0.002, gyro=0.0, zero_bias=True)
    c["still"]["imu"][:, 1:4] = rng.normal(0, 2e-9, (6, 3))
    t = 50.0 + 0.005 * np.arange(8); t[4] = t[3]
    c["repeat"] = _case(rng, 8, t, 50.003, t[-1] - 0.001)
    return c


# ------------------------------------------------------------------------------------------------ f64 model (the teeth)
TEETH = ("fx60_sign", "covw_dt", "rotation_first", "no_clamp", "note_ignored")


def _exp_f64(w, dt):
    n = np.linalg.norm(w)
    if not n > 1e-7:
        return np.eye(3)
    return _so3(w / n * (n * dt))


def model(case, tooth=None):
    """EK:54-123 in numpy f64 with dense 15 x 15 products; tooth: one defect of TEETH"""
    m, imu = case["m"], np.asarray(case["imu"]).reshape(-1, 7)
    last_end, beg, end, sg = case["last_end"], case["beg"], case["end"], case["sg"]
    cg, ca, cbg, cba = np.split(np.asarray(case["noise"]), 4)
    st = np.array(case["state"], dtype=np.float64)
    R, p, v = st[1:10].reshape(3, 3).copy(), st[10:13].copy(), st[13:16].copy()
    bg, ba, g = st[16:19], st[19:22], st[22:25]
    P = np.array(case["cov"], dtype=np.float64).reshape(15, 15)
    rows = []
    for j in range(m - 1):
        head, tail = imu[j], imu[j + 1]
        if tail[0] < last_end:
            continue
        w = 0.5 * (head[1:4] + tail[1:4]) - bg
        a = 0.5 * (head[4:7] + tail[4:7]) * sg - ba
        acc = R @ a + g
        cur = head[0]
        if cur < last_end and tooth != "no_clamp":
            cur = last_end
        dt = tail[0] - cur
        rows.append(np.concatenate([[cur - beg], R.ravel(), p, v, w, acc]))
        H = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        F, W = np.eye(15), np.zeros((15, 15))
        F[0:3, 0:3] = _exp_f64(w, -dt)
        F[0:3, 9:12] = -np.eye(3) * dt
        F[3:6, 6:9] = np.eye(3) * dt
        F[6:9, 0:3] = (1 if tooth == "fx60_sign" else -1) * R @ H * dt
        F[6:9, 12:15] = -R * dt
        d2 = dt if tooth == "covw_dt" else dt * dt
        W[0:3, 0:3] = np.diag(cg * d2); W[6:9, 6:9] = R @ np.diag(ca) @ R.T * d2
        W[9:12, 9:12] = np.diag(cbg * d2); W[12:15, 12:15] = np.diag(cba * d2)
        P = F @ P @ F.T + W
        if tooth == "rotation_first":
            R = R @ _exp_f64(w, dt)
            acc = R @ a + g
        p = p + v * dt + 0.5 * acc * dt * dt
        v = v + acc * dt
        if tooth != "rotation_first":
            R = R @ _exp_f64(w, dt)
    imu_end = imu[m - 1, 0]
    note = 1.0 if (end > imu_end or tooth == "note_ignored") else -1.0
    dt = note * (end - imu_end)
    out = st.copy()
    out[0] = end
    Re = R @ _exp_f64(note * w, dt)
    out[1:10] = Re.ravel()
    out[13:16] = v + note * acc * dt
    out[10:13] = p + note * v * dt + note * 0.5 * acc * dt * dt
    return dict(n=len(rows), state=out, cov=P.ravel(), poses=np.array(rows), end_pose=np.concatenate([Re.ravel(), out[10:13]]))
