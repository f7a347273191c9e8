"""The numpy restatement of the published scan (tests/scan_export_ref.py), which tests/test_gpu_kd_on_state.py holds
vba_odom_state_export_scan to bit for bit, pinned before a GPU is involved: against x.R * p + x.p in exact rational arithmetic
(fractions) at the counted bound, and against the stated order evaluated one correctly rounded operation at a time.

The bound.  A coordinate is ((a + b) + c) + t with a, b, c products: the first two products pass through one rounding of their own and
three sums, the third through one and two, t through one sum, so with u = 2^-53 every term carries at most (1 + u)^4 - 1 and
|d - v| <= ((1 + u)^4 - 1) * (|a| + |b| + |c| + |t|) for the exact products a, b, c.  The narrowing adds at most 2^-24 |d| (the values
here are far from the float subnormals and from overflow).  Nothing is measured: the bound is the count.

The transform on the device is vba::kf_apply (csrc/vba_common.hpp), a __device__ function of a header that includes the HIP runtime:
it is not a host/device shared header, so there is no g++ build of it here; the GPU test compares the kernel itself."""
from fractions import Fraction

import numpy as np

from scan_export_ref import checksum, export_restated

U = Fraction(1, 2 ** 53)
E4 = (1 + U) ** 4 - 1
NARROW = Fraction(1, 2 ** 24)


def _so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _state(rng, scale=30.0):
    s = np.zeros(25)
    s[1:10] = _so3(rng.normal(0, 0.8, 3)).ravel()
    s[10:13] = rng.normal(0, scale, 3)
    return s


def _points(rng, n):
    p = rng.normal(0, 20.0, (n, 3)).astype(np.float32).astype(np.float64)      # scan points are floats
    p[0] = [-0.0, 0.0, -0.0]
    p[1] = [-0.0, 3.5, 0.0]
    p[2] = [1e-3, -1e-3, 0.0]
    return p


def _rounded_steps(state, p):
    """the stated order with every operation exact and then rounded to the nearest double (float(Fraction) rounds correctly)"""
    R = state[1:10].reshape(3, 3); t = state[10:13]
    F = Fraction
    out = []
    for r in range(3):
        a = float(F(R[r, 0]) * F(p[0])); b = float(F(R[r, 1]) * F(p[1])); c = float(F(R[r, 2]) * F(p[2]))
        s = float(F(a) + F(b)); s = float(F(s) + F(c)); s = float(F(s) + F(t[r]))
        out.append(s)
    return out


def test_restatement_within_the_counted_bound_of_exact_arithmetic():
    rng = np.random.default_rng(22)
    worst = Fraction(0)
    for trial in range(4):
        state = _state(rng)
        pts = _points(rng, 300)
        got = export_restated(state, pts, 2.0)
        assert got.dtype == np.float32 and got.shape == (300, 4) and np.all(got[:, 3] == np.float32(2.0))
        R = [[Fraction(v) for v in row] for row in state[1:10].reshape(3, 3)]
        t = [Fraction(v) for v in state[10:13]]
        for i, p in enumerate(pts):
            x = [Fraction(v) for v in p]
            for r in range(3):
                terms = [R[r][k] * x[k] for k in range(3)] + [t[r]]
                v = sum(terms)
                S = sum(abs(q) for q in terms)
                bound = E4 * S + NARROW * (abs(v) + E4 * S)
                err = abs(Fraction(float(got[i, r])) - v)
                assert err <= bound, (trial, i, r, float(err), float(bound))
                if bound:
                    worst = max(worst, err / bound)
    print("largest error: %.3f of its bound" % float(worst))
    assert worst > Fraction(1, 100)                  # (the bound is not loose by orders of magnitude: the narrowing is really there)


def test_restatement_is_the_stated_order_operation_by_operation():
    """bit equality with the order evaluated in exact arithmetic rounded after every operation, then narrowed once: numpy fused and
    reordered nothing.  Includes negative zeros and results within a few double ulps of a float rounding tie."""
    rng = np.random.default_rng(23)
    state = _state(rng)
    pts = _points(rng, 400)
    # ties: with R = I and p = 0 the result is the point itself; midpoints of adjacent floats are doubles, and so are their neighbours
    tie_state = np.zeros(25); tie_state[1:10] = np.eye(3).ravel()
    f = rng.normal(0, 20.0, 60).astype(np.float32)
    mid = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    ties = np.concatenate([mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf)]).reshape(-1, 3)
    for st, P in ((state, pts), (tie_state, ties)):
        got = export_restated(st, P, 0.0)
        want = np.array([_rounded_steps(st, p) for p in P]).astype(np.float32)
        assert np.array_equal(got[:, :3], want)
    # a tie itself goes to the even neighbour, one double above it goes up
    got = export_restated(tie_state, ties, 0.0)[:, :3].ravel()
    lo = f; hi = np.nextafter(f, np.float32(np.inf))
    even = np.where(lo.view(np.uint32) % 2 == 0, lo, hi)
    assert np.array_equal(got[:60], even) and np.array_equal(got[60:120], hi) and np.array_equal(got[120:], lo)
    # negative zeros in, zeros of either sign out: R * (-0, 0, -0) + p = p
    z = export_restated(state, np.array([[-0.0, 0.0, -0.0]]), 0.0)
    assert np.array_equal(z[0, :3], state[10:13].astype(np.float32))


def test_checksum_is_the_sum_of_the_float_bits():
    a = np.array([[1.0, -2.0, 0.5, 0.0]], dtype=np.float32)
    assert checksum(a) == 0x3F800000 + 0xC0000000 + 0x3F000000
    assert checksum(np.zeros((0, 4), dtype=np.float32)) == 0
