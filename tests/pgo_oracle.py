"""numpy / scipy restatement of vba_pgo_optimize: the pose-graph optimisation that build_graph (VS:2078-2156)
hands to gtsam::ISAM2 {relinearizeThreshold, relinearizeSkip 1} with update(graph, initial) + (U - 1) x update() +
calculateEstimate() (VS:2550-2561, VS:2769-2777).

Poses are flat [R(9) row-major, p(3)]; tangents are xi = [omega; v] (GTSAM Pose3 order); retraction X (+) xi = X Exp(xi).
Every update linearises all factors at theta and solves the FULL 6N system with scipy.sparse (no segment elimination, so the
device's chain elimination is checked independently)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

SMALL = 0.2      # below this rotation angle the trigonometric coefficients come from their Taylor series (no cancellation)


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _coeffs(phi):
    """A = sin/phi, B = (1 - cos)/phi^2, C = (phi - sin)/phi^3, D = 1/phi^2 - (1 + cos)/(2 phi sin),
    E = (1 - phi^2/2 - cos)/phi^4, F = (phi - sin - phi^3/6)/phi^5."""
    t = phi * phi
    if phi < SMALL:
        A = 1 - t / 6 * (1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110))))
        B = 0.5 * (1 - t / 12 * (1 - t / 30 * (1 - t / 56 * (1 - t / 90 * (1 - t / 132)))))
        C = (1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110 * (1 - t / 156))))) / 6
        D = 1 / 12 + t * (1 / 720 + t * (1 / 30240 + t * (1 / 1209600 + t * (1 / 47900160))))
        E = -(1 - t / 30 * (1 - t / 56 * (1 - t / 90 * (1 - t / 132 * (1 - t / 182))))) / 24
        F = -(1 - t / 42 * (1 - t / 72 * (1 - t / 110 * (1 - t / 156 * (1 - t / 210))))) / 120
    else:
        s, c = np.sin(phi), np.cos(phi)
        A = s / phi
        B = (1 - c) / t
        C = (phi - s) / (t * phi)
        D = 1 / t - (1 + c) / (2 * phi * s)
        E = (1 - t / 2 - c) / (t * t)
        F = (phi - s - t * phi / 6) / (t * t * phi)
    return A, B, C, D, E, F


def so3_exp(w):
    W = hat(w)
    A, B = _coeffs(np.linalg.norm(w))[:2]
    return np.eye(3) + A * W + B * (W @ W)


def so3_log(R):
    """omega with Exp(omega) = R, |omega| < pi (angle from atan2: accurate at small and large angles)."""
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])    # 2 sin(phi) u
    s2 = np.linalg.norm(a)
    phi = np.arctan2(0.5 * s2, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))
    t = phi * phi
    f = 1 + t / 6 * (1 + 7 * t / 60) if phi < 1e-4 else phi / np.sin(phi)     # (no cancellation: the series only avoids 0 / 0)
    return 0.5 * f * a


def exp6(xi):
    """SE(3) exponential of xi = [omega; v] -> flat pose."""
    w, v = xi[:3], xi[3:]
    W = hat(w)
    A, B, C = _coeffs(np.linalg.norm(w))[:3]
    WW = W @ W
    R = np.eye(3) + A * W + B * WW
    V = np.eye(3) + B * W + C * WW
    return np.concatenate([R.ravel(), V @ v])


def log6(X):
    R = X[:9].reshape(3, 3)
    w = so3_log(R)
    W = hat(w)
    D = _coeffs(np.linalg.norm(w))[3]
    Vinv = np.eye(3) - 0.5 * W + D * (W @ W)
    return np.concatenate([w, Vinv @ X[9:12]])


def compose(X, Y):
    R1, R2 = X[:9].reshape(3, 3), Y[:9].reshape(3, 3)
    return np.concatenate([(R1 @ R2).ravel(), R1 @ Y[9:12] + X[9:12]])


def inverse(X):
    R = X[:9].reshape(3, 3)
    return np.concatenate([R.T.ravel(), -R.T @ X[9:12]])


def retract(X, xi):
    return compose(X, exp6(xi))


def adjoint(X):
    """Ad(X) in [omega; v] order: [[R, 0], [p^ R, R]]."""
    R = X[:9].reshape(3, 3)
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(X[9:12]) @ R
    return A


def jr_inv(xi):
    """Inverse right Jacobian of SE(3) at xi = [omega; v] (GTSAM's Pose3::LogmapDerivative): [[J^-1, 0], [-J^-1 Q J^-1, J^-1]],
    J = right Jacobian of SO(3), Q = Barfoot's coupling block with the odd terms negated (right form)."""
    w, v = xi[:3], xi[3:]
    W, V = hat(w), hat(v)
    _, _, C, D, E, F = _coeffs(np.linalg.norm(w))
    WW = W @ W
    Ji = np.eye(3) + 0.5 * W + D * WW
    WV, VW, WVW = W @ V, V @ W, W @ V @ W
    Q = -0.5 * V + C * (WV + VW - WVW) + E * (W @ WV + VW @ W - 3 * WVW) - 0.5 * (E - 3 * F) * (WVW @ W + W @ WVW)
    out = np.zeros((6, 6))
    out[:3, :3] = Ji
    out[3:, 3:] = Ji
    out[3:, :3] = -Ji @ Q @ Ji
    return out


def between_error(Xi, Xj, Z):
    return log6(compose(inverse(Z), compose(inverse(Xi), Xj)))


def between_jacobians(Xi, Xj, Z):
    """e = Log(Z^-1 Xi^-1 Xj); de/dxi_j = Jr^-1(e), de/dxi_i = -Jr^-1(e) Ad(Xj^-1 Xi)."""
    e = between_error(Xi, Xj, Z)
    Jj = jr_inv(e)
    Ji = -Jj @ adjoint(compose(inverse(Xj), Xi))
    return e, Ji, Jj


def prior_error(X, P):
    return log6(compose(inverse(P), X))


def prior_jacobian(X, P):
    e = prior_error(X, P)
    return e, jr_inv(e)


def _edge(row):
    row = np.asarray(row, float)
    return int(row[0]), int(row[1]), np.concatenate([row[2:11], row[11:14]]), row[14:20]


def _prior(row):
    row = np.asarray(row, float)
    return int(row[0]), row[1:13].copy(), row[13:19]


def cost(poses, edges, priors):
    c = 0.0
    for row in edges:
        i, j, Z, var = _edge(row)
        e = between_error(poses[i], poses[j], Z)
        c += 0.5 * np.sum(e * e / var)
    for row in priors:
        k, P, var = _prior(row)
        e = prior_error(poses[k], P)
        c += 0.5 * np.sum(e * e / var)
    return c


def linearize(poses, edges, priors):
    """H (sparse 6N x 6N), g = J^T Lambda e, cost at poses."""
    n = len(poses)
    rows, cols, vals = [], [], []
    g = np.zeros(6 * n)
    c = 0.0
    idx = np.arange(6)

    def put(a, b, M):
        r, cc = np.meshgrid(6 * a + idx, 6 * b + idx, indexing="ij")
        rows.append(r.ravel()); cols.append(cc.ravel()); vals.append(M.ravel())

    for row in edges:
        i, j, Z, var = _edge(row)
        e, Ji, Jj = between_jacobians(poses[i], poses[j], Z)
        lam = 1.0 / var
        c += 0.5 * np.sum(e * e * lam)
        LJi, LJj = lam[:, None] * Ji, lam[:, None] * Jj
        put(i, i, Ji.T @ LJi); put(j, j, Jj.T @ LJj); put(i, j, Ji.T @ LJj); put(j, i, Jj.T @ LJi)
        g[6 * i:6 * i + 6] += Ji.T @ (lam * e)
        g[6 * j:6 * j + 6] += Jj.T @ (lam * e)
    for row in priors:
        k, P, var = _prior(row)
        e, J = prior_jacobian(poses[k], P)
        lam = 1.0 / var
        c += 0.5 * np.sum(e * e * lam)
        put(k, k, J.T @ (lam[:, None] * J))
        g[6 * k:6 * k + 6] += J.T @ (lam * e)
    if rows:
        H = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n)).tocsc()
    else:
        H = sp.csc_matrix((6 * n, 6 * n))
    return H, g, c


def solve(H, b, refine=3):
    """H x = b by SuperLU plus fixed-precision iterative refinement.  A chain pinned by a 1e-9 prior is badly conditioned: one
    LU solve leaves the later costs (at the relinearised theta) uncertain to ~5e-9 relative, and the refinement steps make the
    oracle the accurate side of a device comparison."""
    lu = spla.splu(sp.csc_matrix(H))
    x = lu.solve(b)
    for _ in range(refine):
        x = x + lu.solve(b - H @ x)
    return x


def optimize(poses, edges, priors, n_updates=6, relin_threshold=0.01):
    """The schedule of DESIGN.md §12: returns (poses [n][12], stats [U][3] = relinearised nodes, cost at theta, max |delta|_inf,
    deltas [U][n][6])."""
    theta = np.array(poses, float).reshape(-1, 12).copy()
    edges = np.asarray(edges, float).reshape(-1, 20)
    priors = np.asarray(priors, float).reshape(-1, 19)
    n = len(theta)
    stats = np.zeros((n_updates, 3))
    deltas = []
    delta = None
    for u in range(n_updates):
        cnt = 0
        if u > 0:
            for k in range(n):
                if np.abs(delta[k]).max() >= relin_threshold:
                    theta[k] = retract(theta[k], delta[k])
                    cnt += 1
        H, g, c = linearize(theta, edges, priors)
        delta = solve(H, -g).reshape(n, 6)
        stats[u] = (cnt, c, np.abs(delta).max() if n else 0.0)
        deltas.append(delta.copy())
    out = np.array([retract(theta[k], delta[k]) for k in range(n)])
    return out, stats, np.array(deltas)


def relin_margin(deltas, relin_threshold=0.01):
    """Smallest distance of any |delta_k|_inf that feeds a relinearisation decision from the threshold."""
    if len(deltas) < 2:
        return np.inf
    m = np.abs(deltas[:-1]).max(axis=2)
    return np.abs(m - relin_threshold).min()


# ---------------------------------------------------------------- graph builders shared by the tests
def rand_rot(rng, scale=np.pi):
    w = rng.normal(size=3)
    w *= rng.uniform(0, scale) / np.linalg.norm(w)
    return so3_exp(w)


def relative(Xi, Xj):
    """The row body of add_edge(pos1, pos2, x1, x2) (LR:147-153): rot = R1^T R2, tra = R1^T (p2 - p1)."""
    Z = compose(inverse(Xi), Xj)
    return Z[:9], Z[9:12]


def edge_row(i, j, Xi, Xj, var, noise=None):
    rot, tra = relative(Xi, Xj)
    if noise is not None:
        Z = retract(np.concatenate([rot, tra]), noise)
        rot, tra = Z[:9], Z[9:]
    return np.concatenate([[i, j], rot, tra, var])


def prior_row(k, P, var):
    return np.concatenate([[k], P, var])


def trajectory(rng, n, step=1.0):
    """A smooth ground-truth trajectory of n poses."""
    X = np.zeros((n, 12))
    X[0] = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    for k in range(1, n):
        d = np.concatenate([rng.normal(0, 0.05, 3), [step, 0.0, 0.0] + rng.normal(0, 0.1, 3)])
        X[k] = retract(X[k - 1], d)
    return X


def drift(rng, X, rot=2e-3, tra=2e-2):
    """An initial state with accumulated drift: every step's relative pose is perturbed and the chain re-integrated."""
    Y = X.copy()
    for k in range(1, len(X)):
        rel = compose(inverse(X[k - 1]), X[k])
        rel = retract(rel, np.concatenate([rng.normal(0, rot, 3), rng.normal(0, tra, 3)]))
        Y[k] = compose(Y[k - 1], rel)
    return Y


def reference_session(rng, n=400, win=10, kf_win=10, kf_stride=5, n_loops=3, noise=True):
    """Edges shaped like build_graph + topDownProcess (VS:2078-2156, VS:2717-2812) over one session: chain odometry with v6 in
    1e-6 .. 1e-3, a keyframe every win scans, HBA bottom edges between all keyframe pairs of windows of kf_win keyframes every
    kf_stride keyframes, a 1e-9 prior on node 0 and loop edges at 1e-4.  Returns (truth, initial, edges, priors)."""
    X = trajectory(rng, n)
    Y = drift(rng, X)
    ed = []
    nz = (lambda s: np.concatenate([rng.normal(0, s, 3), rng.normal(0, 3 * s, 3)])) if noise else (lambda s: None)
    for k in range(1, n):
        v6 = 10.0 ** rng.uniform(-6, -3, 6)
        ed.append(edge_row(k - 1, k, X[k - 1], X[k], v6, nz(1e-4)))
    kfs = list(range(0, n, win))
    seen = set()
    for s in range(0, max(len(kfs) - kf_win, 0) + 1, kf_stride):
        w = kfs[s:s + kf_win]
        for a in range(len(w)):
            for b in range(a + 1, len(w)):
                if (w[a], w[b]) in seen:
                    continue
                seen.add((w[a], w[b]))
                ed.append(edge_row(w[a], w[b], X[w[a]], X[w[b]], 10.0 ** rng.uniform(-6, -4, 6), nz(1e-4)))
    for _ in range(n_loops):
        a, b = sorted(rng.choice(kfs, 2, replace=False))
        ed.append(edge_row(b, a, X[b], X[a], np.full(6, 1e-4), nz(1e-3)))
    pr = [prior_row(0, Y[0], np.full(6, 1e-9))]
    return X, Y, np.array(ed), np.array(pr)
