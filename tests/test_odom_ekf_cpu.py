"""Host-side check of the EKF algebra of the resident odometry loop (csrc/vba_odom_ekf.hpp: the step of voxelslam.cpp:1053-1062 on the
34 sums of a point loop, the stop rule of VS:1072-1086) against a numpy restatement with np.linalg.inv and synth.so3_exp.  The same
header is compiled for the device by hipcc, where one workgroup's lanes share the work; here g++ builds it for one lane."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DP = C.POINTER(C.c_double)
SUMS_FN = C.CFUNCTYPE(None, C.c_int, DP, DP)
EPS = 2.0 ** -52


def _p(a):
    return a.ctypes.data_as(DP)


@pytest.fixture(scope="module")
def ekf():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_odom_ekf_"), "libodomekfhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out, os.path.join(HERE, "host", "odom_ekf_host.cpp")])
    lib = C.CDLL(out)
    lib.odom_nnt_eig_min_host.restype = C.c_double
    return lib


def _so3_exp(w):
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth
    return synth.so3_exp(np.asarray(w, dtype=np.float64))


def _so3_log(R):                                                  # tools.hpp:86-91
    tr = np.trace(R)
    theta = 0.0 if tr > 3.0 - 1e-6 else np.arccos(0.5 * (tr - 1))
    K = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return (0.5 if abs(theta) < 0.001 else 0.5 * theta / np.sin(theta)) * K


def _state(R, p, v=(0.3, -0.2, 0.1), bg=(0.01, 0.02, -0.01), ba=(0.05, -0.03, 0.02)):
    s = np.zeros(25)
    s[0] = 12.5; s[1:10] = np.asarray(R).ravel(); s[10:13] = p; s[13:16] = v; s[16:19] = bg; s[19:22] = ba; s[22:25] = [0, 0, -9.8]
    return s


def _boxminus(xp, xc):                                            # x_prop - x_curr, tools.hpp:164-173
    Rp, Rc = xp[1:10].reshape(3, 3), xc[1:10].reshape(3, 3)
    return np.concatenate([_so3_log(Rc.T @ Rp), xp[10:22] - xc[10:22]])


def _unpack(s34):
    HTH = np.zeros((6, 6)); i = 0
    for r in range(6):
        for c in range(r, 6):
            HTH[r, c] = HTH[c, r] = s34[i]; i += 1
    n = s34[27:33]
    nnt = np.array([[n[0], n[1], n[2]], [n[1], n[3], n[4]], [n[2], n[4], n[5]]])
    return HTH, s34[21:27].copy(), nnt, int(s34[33])


def _pack(HTH, HTz, nnt=np.diag([30.0, 40.0, 50.0]), match=1234):
    s = np.zeros(34)
    s[:21] = HTH[np.triu_indices(6)]
    s[21:27] = HTz
    s[27:33] = nnt[np.triu_indices(3)]
    s[33] = match
    return s


def _ref_step(s34, cov_inv, xp, xc):
    HTH, HTz, _, _ = _unpack(s34)
    A = cov_inv.copy(); A[:6, :6] += HTH
    K1 = np.linalg.inv(A)
    G = np.zeros((15, 15)); G[:, :6] = K1[:, :6] @ HTH
    vec = _boxminus(xp, xc)
    return K1[:, :6] @ HTz + vec - G[:, :6] @ vec[:6], G, A


def _ref_loop(sums, state, cov):
    """VS:987-1087 with the sums of each iteration's point loop handed in."""
    xp = state.copy(); xc = state.copy(); P = cov.copy()
    cov_inv = np.linalg.inv(P)
    rematch = 0; trace = []; cov_iter = -1; nnt = None
    for it in range(4):
        s34 = sums(it, xc)
        sol, G, _ = _ref_step(s34, cov_inv, xp, xc)
        _, _, nnt, match = _unpack(s34)
        xc = xc.copy()
        xc[1:10] = (xc[1:10].reshape(3, 3) @ _so3_exp(sol[:3])).ravel() if np.linalg.norm(sol[:3]) >= 1e-11 else xc[1:10]
        xc[10:22] += sol[3:]
        ra, ta = np.linalg.norm(sol[:3]), np.linalg.norm(sol[3:6])
        trace.append((match, ra, ta))
        conv = ra * 57.3 < 0.01 and ta * 100 < 0.015
        if conv or (rematch == 0 and it == 2):
            rematch += 1
        if rematch >= 2 or it == 3:
            P = (np.eye(15) - G) @ P
            cov_iter = it
            break
    return xc, P, np.array(trace), cov_iter, nnt


def _spd(rng, n, lo, hi):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    w = np.exp(rng.uniform(np.log(lo), np.log(hi), n)); w[0] = lo; w[-1] = hi
    M = Q @ np.diag(w) @ Q.T
    return 0.5 * (M + M.T)


def _run_loop(ekf, sums, state, cov):
    calls = []

    def cb(it, x25, out34):
        x = np.ctypeslib.as_array(x25, shape=(25,)).copy()
        calls.append(it)
        np.ctypeslib.as_array(out34, shape=(34,))[:] = sums(it, x)
    st = state.copy(); cv = np.ascontiguousarray(cov).copy(); tr = np.zeros(12); ci = C.c_int(0); lr = C.c_int(0); nnt = np.zeros(9)
    n = ekf.odom_ekf_loop_host(SUMS_FN(cb), _p(st), _p(cv), _p(tr), C.byref(ci), C.byref(lr), _p(nnt))
    return n, st, cv.reshape(15, 15), tr.reshape(4, 3), ci.value, lr.value, nnt.reshape(3, 3), calls


# --------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("seed,plo,phi,jscale", [(0, 1e-3, 1e-1, 1.0), (1, 1e-4, 1e-1, 3.0), (2, 1e-5, 1e-2, 15.0), (3, 1e-4, 1e-4, 1.0)])
def test_one_step(ekf, seed, plo, phi, jscale):
    """P SPD with eigenvalues in [plo, phi], HTH = J^T J of 300 rows: lambda_min(HTH + P^-1) >= 1 / phi and lambda_max <= 1 / plo +
    |J|_F^2 (Weyl), so kappa <= phi (1 / plo + |J|_F^2), which the parameters keep below 1e4.  Bar on the solution, relative to its
    max-norm: 100 kappa 15 eps (first-order forward bound, x100 for the unmodelled constant)."""
    rng = np.random.default_rng(seed)
    P = _spd(rng, 15, plo, phi)
    cov_inv = np.linalg.inv(P)
    J = rng.normal(0, jscale, (300, 6))
    HTH = J.T @ J
    assert phi * (1 / plo + (J ** 2).sum()) <= 1e4
    HTz = rng.normal(0, jscale * 3.0, 6)
    R = _so3_exp(rng.normal(0, 0.5, 3))
    xc = _state(R, rng.normal(0, 5, 3))
    xp = xc.copy()
    xp[1:10] = (R @ _so3_exp(rng.normal(0, 0.02, 3))).ravel()
    xp[10:22] += rng.normal(0, 0.02, 12)
    s34 = _pack(HTH, HTz)
    sol = np.zeros(15); G = np.zeros(90); K = np.zeros(90)
    ekf.odom_ekf_step_host(_p(s34), _p(np.ascontiguousarray(cov_inv)), _p(xp), _p(xc), _p(sol), _p(G), _p(K))
    ref, G_ref, A = _ref_step(s34, cov_inv, xp, xc)
    kappa = np.linalg.cond(A)
    bar = 100 * kappa * 15 * EPS
    err = np.abs(sol - ref).max() / np.abs(ref).max()
    print("seed %d: kappa %.4g, solution error %.3g of its max-norm, bar %.3g" % (seed, kappa, err, bar))
    assert kappa <= 1e4
    assert err <= bar
    assert np.abs(G.reshape(15, 6) - G_ref[:, :6]).max() <= bar * np.abs(G_ref).max()
    assert np.abs(K.reshape(15, 6) - np.linalg.inv(A)[:, :6]).max() <= bar * np.abs(np.linalg.inv(A)).max()


# --------------------------------------------------------------------------------------------- whole loop
def _quadratic(H, targets):
    """Sums of the cost 1/2 d^T H d, d = x_curr - target(iter) in (rotation, position): HTH = H, HTz = -H d."""
    def sums(it, x):
        Rt, pt = targets(it)
        d = np.concatenate([_so3_log(Rt.T @ x[1:10].reshape(3, 3)), x[10:13] - pt])
        return _pack(H, -H @ d)
    return sums


def _setup(seed=7):
    rng = np.random.default_rng(seed)
    R0 = _so3_exp(rng.normal(0, 0.4, 3)); p0 = rng.normal(0, 3, 3)
    J = rng.normal(0, 1.0, (400, 6))
    cov = np.eye(15) * 1e-4; cov[9:, 9:] = np.eye(6) * 1e-5
    return rng, R0, p0, J.T @ J * 50.0, _state(R0, p0), cov


def _compare(ekf, sums, state, cov, iters, cov_iter):
    n, st, cv, tr, ci, lr, nnt, calls = _run_loop(ekf, sums, state, cov)
    st_r, cv_r, tr_r, ci_r, nnt_r = _ref_loop(sums, state, cov)
    print("iterations %d (reference %d), covariance written at %d, trace\n%s" % (n, len(tr_r), ci, tr[:n]))
    assert n == len(tr_r) == iters
    assert lr == iters and calls == list(range(iters))            # the launches after the stop returned at the gate
    assert ci == ci_r == cov_iter
    # kappa(HTH + P^-1) < 100 in these cases (P^-1 = diag 1e4 / 1e5, HTH ~ 2e4), so one step is good to 100 kappa 15 eps < 4e-11 of
    # steps below 1; up to four steps, on state entries up to ~10 whose rounding adds a few 1e-15
    assert np.abs(st - st_r).max() < 1e-10
    assert np.abs(cv - cv_r).max() < 1e-10 * np.abs(cv_r).max()
    assert np.array_equal(tr[:n, 0], tr_r[:, 0])
    assert np.abs(tr[:n, 1:] - tr_r[:, 1:]).max() < 1e-10
    assert np.all(tr[n:] == 0)
    assert np.array_equal(nnt, nnt_r)
    return st, cv


def test_loop_converged_at_once(ekf):
    """The target is the prediction: iterations 0 and 1 both converge, the loop stops after two."""
    rng, R0, p0, H, state, cov = _setup()
    _compare(ekf, _quadratic(H, lambda it: (R0, p0)), state, cov, 2, 1)


def test_loop_never_converged(ekf):
    """The target jumps before every iteration: four iterations, the covariance updated once, at iteration 3."""
    rng, R0, p0, H, state, cov = _setup()
    tg = [(R0 @ _so3_exp(rng.normal(0, 0.02, 3)), p0 + rng.normal(0, 0.1, 3)) for _ in range(4)]
    _, cv = _compare(ekf, _quadratic(H, lambda it: tg[it]), state, cov, 4, 3)
    assert not np.array_equal(cv, cov)


def test_loop_first_converged_at_iteration_2(ekf):
    """The target moves before iterations 0 and 1, then holds: iteration 2 is the first rematch, the stop comes at iteration 3."""
    rng, R0, p0, H, state, cov = _setup()
    tg = [(R0 @ _so3_exp(rng.normal(0, 0.02, 3)), p0 + rng.normal(0, 0.1, 3)) for _ in range(2)]
    _compare(ekf, _quadratic(H, lambda it: tg[min(it, 1)]), state, cov, 4, 3)


def test_loop_converged_at_1_and_2(ekf):
    """A fixed target away from the prediction: iteration 0 moves, 1 and 2 converge, three iterations."""
    rng, R0, p0, H, state, cov = _setup()
    tg = (R0 @ _so3_exp(rng.normal(0, 0.01, 3)), p0 + rng.normal(0, 0.05, 3))
    st, _ = _compare(ekf, _quadratic(H, lambda it: tg), state, cov, 3, 2)
    assert np.abs(st[10:13] - tg[1]).max() < np.abs(state[10:13] - tg[1]).max()


def test_loop_zero_sums(ekf):
    """No match at all is a legal input: the solution is exactly zero, two iterations, state and covariance bit-identical."""
    rng, R0, p0, H, state, cov = _setup()
    cov = _spd(rng, 15, 1e-5, 1e-3)
    n, st, cv, tr, ci, lr, nnt, calls = _run_loop(ekf, lambda it, x: np.zeros(34), state, cov)
    assert n == 2 and lr == 2 and ci == 1
    assert np.array_equal(st, state)
    assert np.array_equal(cv, cov)
    assert np.all(tr == 0) and np.all(nnt == 0)
    assert ekf.odom_nnt_eig_min_host(_p(np.zeros(9))) == 0.0


def test_nnt_eig_min(ekf):
    rng = np.random.default_rng(3)
    for _ in range(200):
        A = rng.normal(size=(50, 3)); A = A.T @ A
        e = ekf.odom_nnt_eig_min_host(_p(np.ascontiguousarray(A)))
        assert abs(e - np.linalg.eigvalsh(A)[0]) < 1e-12 * np.abs(A).max()
