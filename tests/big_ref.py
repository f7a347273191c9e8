"""Corpus, conversions and references for the any-window path (csrc/vba_kernels_big.hpp: k_big_slot, k_big_syrk, k_big_diag,
k_big_blockdiag, k_big_residual, k_big_eidx) on its sparse store.  A helper module shared by tests/test_big_cpu.py (the f64 oracle, the
teeth) and tests/test_gpu_big.py (the device through vba_debug_big_*).  No GPU code; nothing outside the repository is read.

Store.  CSR over voxels: vptr[V + 1], efr[E] (the frame of every entry, increasing within a voxel), ecl[E][10] (the body cluster sums
Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N), and per voxel eig_val[V][3], eig_vec[V][9], pcr_add[V][10].  The path has no fixed cluster and no
coefficient: fix = 0, coe = 1.  to_csr / to_dense convert to and from the dense [V][W][10] form hess_ref works on; a slot with N == 0 is
absent.

Hessian pass.  The reference and the bars are hess_ref.Ref and Ref.check(..., sym=False), unchanged: the literal per-pair formula in
double-double, D_H = 35, D_G = 15, D_R = 1, per entry, exact zeros where no voxel of the subset sees the frame pair.  sym=False is
deliberate: k_big_syrk forms entry (r, c) of a diagonal tile as (w g_r) g_c and entry (c, r) as (w g_c) g_r, and the voxel slices reach the
two mirrors in different atomic order, so H is not its transpose bit for bit and each half has to meet the bar on its own.  Both halves
are read: k_bigl_setup (the solve) takes the lower half, k_big_blockdiag (the edge weights of HBA_add_edge) the upper.

Residual pass.  k_big_residual sums the entries of a voxel after PointCluster::transform, P' = R P R^T + (R v) p^T + p (R v)^T + N p p^T,
v' = R v + N p, fits the plane and stores eig_val, eig_vec, pcr_add.  transform_ref writes that formula once over hess_ref's counted value
type (Tr over DD), so its rounding count and its magnitude shadow M come from the code.  By hand, by the rule of hess_ref's docstring:
R P 3 (a dot product of three: 1, 2, 3); (R P) R^T 3 + 0 + 1 = 4, summed 6; R v 3; (R v) p^T 4; N p 1, (N p) p^T 2; the four terms added
from the left max(6, 4) + 1 = 7, 8, 9.  v' = R v + N p: max(3, 1) + 1 = 4.  So
    D_T = 9
(asserted equal to the count the code keeps, tests/test_big_cpu.py).  A voxel of n_v entries adds n_v terms, each within D_T u M:
    |pcr_add^[v][k] - pcr_add*[v][k]| <= (D_T + n_v) u M[v][k]        k = 0..8;      N (k = 9) is exact.
The eigen-data is compared as tests/test_gpu_eig3.py compares K4's: against eig3_ref.Ref of the covariance formed exactly from the sums the
device itself returned, bars scaled by m2 = max|P/N|.  r is compared with the double-double sum of the eig_val[:, 0] the device itself
returned, within (1 + V) u sum |l0|: the reduction is kept apart from the eigen-solver.

Corpus.  store(W): hess_ref.corpus(W) with fix = 0 and coe = 1, voxels left without a frame dropped (class fixonly), eigen-data
recomputed by hess_ref.host_eigen, class labels kept (`fixed` and `coe` are then further planar classes, `lonely` a one-entry voxel),
padded with planar voxels (`pad`) to a multiple of 16 = one chunk of k_big_syrk, then three runs that each start at a chunk boundary:
    skip      32 voxels that see frames 0 and 1 only: for W > 8 two whole chunks without an entry in the later tiles (the chunk skip);
    straddle  16 voxels that see frames 7 and 8 only (frame W - 1 and one other when W <= 8): pairs across a tile boundary;
    full      5 voxels that see every frame, so V is not a multiple of 16.
At W = 41 the voxels hess_ref gave a "random" mask are rebuilt on bands of at most 4 consecutive frames, the occupancy of a top-level
window.  origin(W): hess_ref.origin_store(W) with coe = 1, where the bars are tightest."""
import numpy as np

import hess_ref as R
from hess_ref import DD, Tr, U, add, mul, matmul, matvec, outer, tr_, madd

D_T = 9
VC = 16                                 # voxels per chunk of k_big_syrk (BIG_VC)
TF = 8                                  # frames per tile (BIG_TF)
CLASSES = ("plane", "fixed", "lonely", "neargap", "coe", "pad", "skip", "straddle", "full")


# ------------------------------------------------------------------------------------------------ conversions
def to_csr(clusters):
    """[V][W][10] -> vptr [V+1], efr [E], ecl [E][10]: entries in frame order, a slot with N == 0 absent"""
    clusters = np.asarray(clusters, dtype=np.float64)
    occ = clusters[:, :, 9] != 0.0
    vptr = np.zeros(len(clusters) + 1, dtype=np.int32)
    vptr[1:] = np.cumsum(occ.sum(1))
    v, f = np.nonzero(occ)                                              # row-major: voxel by voxel, frames increasing
    return vptr, f.astype(np.int32), clusters[v, f].copy()


def to_dense(vptr, efr, ecl, W):
    V = len(vptr) - 1
    out = np.zeros((V, W, 10))
    evox = np.repeat(np.arange(V), np.diff(vptr))
    out[evox, np.asarray(efr)] = np.asarray(ecl, dtype=np.float64).reshape(-1, 10)
    return out


# ------------------------------------------------------------------------------------------------ corpus
def _patch_voxel(rng, W, frames, true, lo=6, hi=300):
    """one planar voxel seen by `frames`: every frame sees its own noisy window of a patch 1 to 100 m out (as hess_ref.corpus's patch)"""
    n, t1, t2 = R._frame(rng)
    c0 = rng.normal(size=3); c0 *= 10.0 ** rng.uniform(0, 2) / np.linalg.norm(c0)
    ext = rng.uniform(0.05, 0.5, 2)
    out = np.zeros((W, 10))
    for i in frames:
        m = int(round(10.0 ** rng.uniform(np.log10(lo), np.log10(hi))))
        o = rng.uniform(-0.5, 0.5, 2) * ext
        q = (c0 + np.outer(o[0] + rng.uniform(-0.5, 0.5, m) * ext[0], t1) + np.outer(o[1] + rng.uniform(-0.5, 0.5, m) * ext[1], t2)
             + np.outer(rng.normal(0, 0.01, m), n))
        out[i] = R.cluster(R._body(q, true[i]))
    return out


def _rod_voxel(rng, W, frames, poses, gap):
    n, t1, t2 = R._frame(rng)
    c0 = n * rng.uniform(3, 30)
    out = np.zeros((W, 10))
    for i, q in R._rod(c0, n, t1, t2, gap, np.asarray(frames)):
        out[i] = R.cluster(R._body(q, poses[i]))
    return out


def _band(rng, W):
    k = int(rng.integers(2, 5))                                         # 2 to 4 consecutive frames
    a = int(rng.integers(0, W - k + 1))
    return list(range(a, a + k))


def _random_mask_kinds(cls):
    """which voxels of hess_ref.corpus drew a "random" mask (the cycle of mask kinds per class in corpus())"""
    count, out = {}, []
    for c in cls:
        k = count.get(c, 0); count[c] = k + 1
        out.append((c in ("plane", "coe") and k % 3 == 2) or (c == "fixed" and k % 5 == 4) or (c == "neargap" and k % 2 == 1))
    return np.array(out)


def _build(W, seed=20261019):
    base = R.store(W)
    rng = np.random.default_rng(seed + W)
    poses, true = base["poses"], base["true_poses"]
    clusters = base["clusters"].copy(); cls = list(base["cls"])
    if W == 41:                                                         # bands instead of the random masks
        gaps = 0
        for a in np.flatnonzero(_random_mask_kinds(cls)):
            if cls[a] == "neargap":
                clusters[a] = _rod_voxel(rng, W, _band(rng, W), poses, R.GAPS[gaps % len(R.GAPS)]); gaps += 1
            else:
                clusters[a] = _patch_voxel(rng, W, _band(rng, W), true)
    keep = np.flatnonzero((clusters[:, :, 9] != 0.0).any(1))            # fix = 0: a voxel with no frame is no voxel
    clusters = clusters[keep]; cls = [cls[a] for a in keep]
    more, mcls = [], []
    for _ in range(-len(cls) % VC):
        fr = _band(rng, W) if W == 41 else np.flatnonzero(R._mask(rng, W, "random"))
        more.append(_patch_voxel(rng, W, fr, true)); mcls.append("pad")
    for _ in range(2 * VC):
        more.append(_patch_voxel(rng, W, (0, 1), true)); mcls.append("skip")
    pair = (TF - 1, TF) if W > TF else (W - 1, int(rng.integers(0, W - 1)))
    for _ in range(VC):
        more.append(_patch_voxel(rng, W, pair, true)); mcls.append("straddle")
    for _ in range(5):
        more.append(_patch_voxel(rng, W, range(W), true, hi=60)); mcls.append("full")
    clusters = np.concatenate([clusters, np.array(more)]); cls = np.array(cls + mcls)
    V = len(cls)
    fix = np.zeros((V, 10)); coe = np.ones(V)
    ev, evec, pa = R.host_eigen(clusters, fix, poses)
    return dict(clusters=clusters, fix=fix, coe=coe, eig_val=ev, eig_vec=evec, pcr_add=pa, poses=poses, true_poses=true, cls=cls, W=W)


_STORES, _REFS = {}, {}


def store(W):
    if ("store", W) not in _STORES:
        _STORES[("store", W)] = _build(W)
    return _STORES[("store", W)]


def origin(W):
    if ("origin", W) not in _STORES:
        st = dict(R.origin_store(W))
        V = len(st["coe"])
        st["coe"] = np.ones(V); st["fix"] = np.zeros((V, 10))
        st["eig_val"], st["eig_vec"], st["pcr_add"] = R.host_eigen(st["clusters"], st["fix"], st["poses"])
        _STORES[("origin", W)] = st
    return _STORES[("origin", W)]


def subset(st, idx):
    out = dict(st)
    for k in ("clusters", "fix", "coe", "eig_val", "eig_vec", "pcr_add", "cls"):
        out[k] = st[k][idx]
    return out


def ref_of(st, key, poses=None, eigen=None):
    """hess_ref.Ref of a store (cached under key); eigen = (eig_val, eig_vec, pcr_add) replaces the stored eigen-data"""
    if key not in _REFS:
        ev, evec, pa = eigen if eigen is not None else (st["eig_val"], st["eig_vec"], st["pcr_add"])
        _REFS[key] = R.Ref(st["clusters"], st["coe"], ev, evec, pa, st["poses"] if poses is None else poses)
    return _REFS[key]


def nchunk(V):
    return (V + VC - 1) // VC


# ------------------------------------------------------------------------------------------------ the kernel's split, for the teeth
def slot_terms(st, v, i):
    """The split k_big_slot makes of one entry (voxel v, frame i), in plain f64: G [3][6] (g1, g2, h), the weights c [3] of k_big_syrk,
    the diagonal-block remainder E [6][6] and the gradient [6].  The voxel's Hessian is sum_ij G_i^T diag(c) G_j + blockdiag(E_i); the
    teeth of tests/test_big_cpu.py take single pieces out of the oracle's result (after checking this sum against the bars)."""
    c = st["clusters"][v, i]; X = st["poses"][i]
    Rm, p = X[:9].reshape(3, 3), X[9:]
    P = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]); vv = c[6:9]; n = c[9]
    Um = st["eig_vec"][v].reshape(3, 3); lam = st["eig_val"][v]; pa = st["pcr_add"][v]
    NN = pa[9]; inn = 1.0 / NN
    u = [Um[:, m] for m in range(3)]
    a = [Rm.T @ u[m] for m in range(3)]
    t = p - pa[6:9] * inn
    s = [u[m] @ t for m in range(3)]
    w = P @ a[0] + s[0] * vv
    c2 = Rm @ vv + n * t
    q = np.cross(vv, a[0])
    d = [c2 @ u[m] for m in range(3)]
    grad = 2.0 * inn * np.concatenate([np.cross(w, a[0]), d[0] * u[0]])
    G = np.zeros((3, 6))
    for m in (1, 2):
        bm = P @ a[m] + s[m] * vv
        G[m - 1, :3] = (-np.cross(a[0], bm) + np.cross(w, a[m])) * inn
        G[m - 1, 3:] = (u[0] * d[m] + d[0] * u[m]) * inn
    G[2, :3] = q; G[2, 3:] = n * u[0]
    cw = np.array([2.0 / (lam[0] - lam[1]), 2.0 / (lam[0] - lam[2]), -2.0 * inn * inn])
    T = np.cross(a[0], P.T).T                                           # column c of T = a0 x (column c of P)
    S = np.cross(T, a[0])                                               # row r of S = (row r of T) x a0
    S = np.triu(S) + np.triu(S, 1).T
    E = np.zeros((6, 6)); e2 = 2.0 * inn
    E[:3, :3] = e2 * (0.5 * (np.outer(a[0], w) + np.outer(w, a[0])) - (w @ a[0]) * np.eye(3) - S)
    E[:3, 3:] = e2 * np.outer(q, u[0]); E[3:, :3] = E[:3, 3:].T
    E[3:, 3:] = e2 * n * np.outer(u[0], u[0])
    return G, cw, E, grad


# ------------------------------------------------------------------------------------------------ residual pass
def transform_ref(ecl, pose_of_entry):
    """PointCluster::transform of every entry, over Tr(DD): (list of 9 Tr vectors over the entries, the largest rounding count)"""
    ecl = np.asarray(ecl, dtype=np.float64); X = np.asarray(pose_of_entry, dtype=np.float64)

    def inp(a):
        v = DD.of(a)
        return Tr(v, v.absf(), 0)

    c = [inp(ecl[:, k]) for k in range(10)]
    P = [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]
    v, N = c[6:9], c[9]
    Rm = [[inp(X[:, 3 * r + k]) for k in range(3)] for r in range(3)]
    p = [inp(X[:, 9 + k]) for k in range(3)]
    Rv = matvec(Rm, v)
    rp = outer(Rv, p)
    Np = [mul(N, x) for x in p]
    Pw = madd(madd(madd(matmul(matmul(Rm, P), tr_(Rm)), rp), tr_(rp)), outer(Np, p))
    vw = [add(a, b) for a, b in zip(Rv, Np)]
    out = [Pw[0][0], Pw[1][0], Pw[2][0], Pw[1][1], Pw[2][1], Pw[2][2], vw[0], vw[1], vw[2]]
    return out, max(t.k for t in out)


def residual_ref(vptr, efr, ecl, poses):
    """sums of the transformed entries per voxel: (DD of shape [9][V], bar [V][9], N [V])"""
    vptr = np.asarray(vptr); V = len(vptr) - 1
    terms, d = transform_ref(ecl, np.asarray(poses, dtype=np.float64).reshape(-1, 12)[np.asarray(efr)])
    assert d == D_T
    hi = np.zeros((9, V)); lo = np.zeros((9, V)); M = np.zeros((V, 9)); N = np.zeros(V)
    ecl = np.asarray(ecl, dtype=np.float64)
    for a in range(V):
        e0, e1 = int(vptr[a]), int(vptr[a + 1])
        for k in range(9):
            s = DD(np.zeros(1))
            for e in range(e0, e1):
                s = s + DD(terms[k].v.hi[e:e + 1], terms[k].v.lo[e:e + 1])
            hi[k, a] = s.hi[0]; lo[k, a] = s.lo[0]
            M[a, k] = terms[k].m[e0:e1].sum()
        N[a] = ecl[e0:e1, 9].sum()                                      # point counts: small integers, exact in any order
    n_v = np.diff(vptr).astype(np.float64)
    return DD(hi, lo), (D_T + n_v)[:, None] * U * M, N


def check_sums(vptr, efr, ecl, poses, pcr_add):
    """ratios of the device's pcr_add to the bars: dict with sums (largest ratio), zero, N (0 or inf)"""
    s, bar, N = residual_ref(vptr, efr, ecl, poses)
    pa = np.asarray(pcr_add, dtype=np.float64)
    if not np.all(np.isfinite(pa)):
        return {"finite": np.inf}
    err = s.err_to(pa[:, :9].T).T
    z = bar == 0.0
    return {"sums": float((err[~z] / bar[~z]).max()) if np.any(~z) else 0.0, "zero": np.inf if np.any(err[z] != 0.0) else 0.0,
            "N": 0.0 if np.array_equal(pa[:, 9], N) else np.inf}


def check_r(r, l0):
    """ratio of |r - sum l0| to (1 + V) u sum |l0|, the sum in double-double over the device's own eigenvalues"""
    l0 = np.asarray(l0, dtype=np.float64)
    if len(l0) == 0:
        return 0.0 if r == 0.0 else np.inf
    s = DD(l0[None, :]).sum_last(range(len(l0)))
    bar = (1 + len(l0)) * U * float(np.abs(l0).sum())
    err = float(s.err_to(np.array([r]))[0])
    return err / bar if bar > 0.0 else (0.0 if err == 0.0 else np.inf)
