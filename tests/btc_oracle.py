"""numpy restatement of the loop retrieval of the loop-closure thread for the tests of vba_btc_*: STDescManager::AddSTDescs /
SearchLoop (BTC.cpp:205-277) with candidate_selector, candidate_verify, triangle_solver and plane_geometric_verify
(BTC.cpp:1128-1479), and icp_normal (loop_refine.hpp:47-139).  TEST INFRASTRUCTURE only.

Descriptor rows use the layout of include/voxelba.h (VBA_BTC_ROW_LEN = 19):
  [triangle(3) center(3) frame A.loc(3) B.loc(3) C.loc(3) A.summary B.summary C.summary], occupancy as uint64 [n][3].
Nearest neighbours are exact (squared L2 in float32, x then y then z, the earlier index wins a tie: the conventions of
pcl::KdTreeFLANN with eps = 0 as the device restates them).
"""
import math

import numpy as np
from scipy.spatial import cKDTree

ROUND = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]   # voxel_round, BTC.cpp:1135-1143


def config_dict(cfg):
    """vba_btc_config (ctypes) or dict -> dict of Python floats / ints (float fields keep their float32 values)."""
    keys = ("skip_near_num", "candidate_num", "rough_dis_threshold", "similarity_threshold", "icp_threshold", "normal_threshold",
            "dis_threshold", "occupy_len")
    if isinstance(cfg, dict):
        return {k: cfg[k] for k in keys}
    return {k: getattr(cfg, k) for k in keys}


def read_parameters(is_high_fly):
    """BTC.cpp:3-68, retrieval fields, as float32 values."""
    f = lambda v: float(np.float32(v))
    return dict(skip_near_num=30, candidate_num=100 if is_high_fly else 20, rough_dis_threshold=f(0.01),
                similarity_threshold=f(0.5 if is_high_fly else 0.7), icp_threshold=f(0.15), normal_threshold=f(0.2),
                dis_threshold=f(0.5), occupy_len=50)


def popcount64(a):
    return np.bitwise_count(np.asarray(a, dtype=np.uint64)).astype(np.int64)


def binary_similarity(a, b, sa, sb):
    """BTC.cpp:70-80: 2 popcount(a & b) / (sa + sb); 0 / 0 is NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * popcount64(np.bitwise_and(a, b)).astype(np.float64) / (np.asarray(sa, np.int64) + np.asarray(sb, np.int64)).astype(np.float64)


def norm3(v):
    v = np.asarray(v, dtype=np.float64)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def triangle_solver(src_loc, src_cen, ref_loc, ref_cen):
    """BTC.cpp:1398-1420, batched: loc [k][3][3] (rows A, B, C), cen [k][3] -> R [k][3][3], t [k][3]."""
    src = np.swapaxes(src_loc - src_cen[:, None, :], 1, 2)       # columns A, B, C minus the centre
    ref = np.swapaxes(ref_loc - ref_cen[:, None, :], 1, 2)
    cov = src @ np.swapaxes(ref, 1, 2)
    U, S, Vt = np.linalg.svd(cov)
    V = np.swapaxes(Vt, 1, 2)
    R = V @ np.swapaxes(U, 1, 2)
    neg = np.linalg.det(R) < 0
    if neg.any():
        K = np.diag([1.0, 1.0, -1.0])
        R[neg] = V[neg] @ K @ np.swapaxes(U[neg], 1, 2)
    t = -np.einsum("kij,kj->ki", R, src_cen) + ref_cen
    return R, t


def nn_float(query_f32, cloud_f32):
    """exact 1-NN in float32 (x then y then z, earlier index wins a tie): index per query, -1 for an empty cloud."""
    q = np.asarray(query_f32, np.float32).reshape(-1, 3)
    c = np.asarray(cloud_f32, np.float32).reshape(-1, 3)
    if len(c) == 0:
        return np.full(len(q), -1, dtype=np.int64)
    return _nn_tree(cKDTree(c.astype(np.float64)), q, c)


class BtcDb:
    """STDescManager's database half: descriptors in cells keyed by STD_LOC, in insertion order; plane clouds."""

    def __init__(self, cfg):
        self.cfg = config_dict(cfg)
        self.rows = np.zeros((0, 19))
        self.bits = np.zeros((0, 3), dtype=np.uint64)
        self.cells = {}
        self.clouds = []
        self.seq = []

    def push_plane_cloud(self, xyz_normal, seq):
        self.clouds.append(np.asarray(xyz_normal, np.float32).reshape(-1, 6).copy())
        self.seq.append(seq)

    def add_stds(self, rows, bits):
        """BTC.cpp:258-277: STD_LOC = (int)(triangle_ + 0.5), C truncation."""
        rows = np.asarray(rows, np.float64).reshape(-1, 19)
        bits = np.asarray(bits, np.uint64).reshape(-1, 3)
        base = len(self.rows)
        for i, r in enumerate(rows):
            assert 0 <= r[6] < len(self.clouds)
            key = (int(r[0] + 0.5), int(r[1] + 0.5), int(r[2] + 0.5))
            self.cells.setdefault(key, []).append(base + i)
        self.rows = np.concatenate([self.rows, rows])
        self.bits = np.concatenate([self.bits, bits])

    # --- candidate_selector (BTC.cpp:1128-1279)
    def match_list(self, rows, bits):
        """the match list in the reference's order: (query i, database row) pairs, and the per-frame votes"""
        cfg = self.cfg
        rows = np.asarray(rows, np.float64).reshape(-1, 19)
        bits = np.asarray(bits, np.uint64).reshape(-1, 3)
        qi, dj = [], []
        for i, r in enumerate(rows):
            tri = r[0:3]
            for inc in ROUND:
                pos = (int(tri[0] + inc[0]), int(tri[1] + inc[1]), int(tri[2] + inc[2]))
                cen = np.array(pos, dtype=np.float64) + 0.5
                if not norm3(tri - cen) < 1.5:
                    continue
                lst = self.cells.get(pos)
                if lst is None:
                    continue
                qi.append(np.full(len(lst), i, dtype=np.int64))
                dj.append(np.asarray(lst, dtype=np.int64))
        if not qi:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        qi = np.concatenate(qi); dj = np.concatenate(dj)
        q, d = rows[qi], self.rows[dj]
        ok = (q[:, 6].astype(np.int64) - d[:, 6].astype(np.int64)) > cfg["skip_near_num"]
        thr = norm3(q[:, 0:3]) * cfg["rough_dis_threshold"]
        ok &= norm3(q[:, 0:3] - d[:, 0:3]) < thr
        sim = (binary_similarity(bits[qi, 0], self.bits[dj, 0], q[:, 16], d[:, 16]) +
               binary_similarity(bits[qi, 1], self.bits[dj, 1], q[:, 17], d[:, 17]) +
               binary_similarity(bits[qi, 2], self.bits[dj, 2], q[:, 18], d[:, 18])) / 3
        with np.errstate(invalid="ignore"):
            ok &= sim > cfg["similarity_threshold"]
        return qi[ok], dj[ok]

    def candidates(self, mframes):
        """repeated max_element over match_array (BTC.cpp:1239-1277): [(frame, votes)]"""
        nf = len(self.clouds)
        votes = np.bincount(mframes, minlength=nf).astype(np.int64) if nf else np.zeros(0, np.int64)
        out = []
        for _ in range(self.cfg["candidate_num"]):
            if nf == 0:
                break
            f = int(np.argmax(votes))
            v = int(votes[f])
            if v < 5:
                break
            votes[f] = 0
            out.append((f, v))
        return out

    # --- candidate_verify + plane_geometric_verify (BTC.cpp:1281-1479)
    def verify(self, rows, qi, dj, pl_cur):
        size = len(qi)
        skip = size // 50 + 1
        use = size // skip
        s_idx = np.arange(use) * skip
        q = np.asarray(rows, np.float64).reshape(-1, 19)
        qloc = q[qi][:, 7:16].reshape(-1, 3, 3); qcen = q[qi][:, 3:6]
        dloc = self.rows[dj][:, 7:16].reshape(-1, 3, 3); dcen = self.rows[dj][:, 3:6]
        R, t = triangle_solver(qloc[s_idx], qcen[s_idx], dloc[s_idx], dcen[s_idx])
        votes = np.zeros(use, dtype=np.int64)
        for s in range(use):
            tr = np.einsum("ij,kvj->kvi", R[s], qloc) + t[s]
            ok = np.all(norm3(tr - dloc) < 3.0, axis=1)
            votes[s] = int(ok.sum())
        max_vote, max_idx = 0, 0
        for s in range(use):
            if max_vote < votes[s]:
                max_vote, max_idx = int(votes[s]), s
        if max_vote < 4:
            return dict(max_vote=max_vote, max_vote_index=max_idx, score=-1.0, R=None, t=None)
        return dict(max_vote=max_vote, max_vote_index=max_idx, R=R[max_idx], t=t[max_idx])

    def plane_geometric_verify(self, src, tar, R, t):
        src = np.asarray(src, np.float32).reshape(-1, 6)
        tar = np.asarray(tar, np.float32).reshape(-1, 6)
        p = src[:, 0:3].astype(np.float64); n = src[:, 3:6].astype(np.float64)
        pi = p @ R.T + t
        ni = n @ R.T
        idx = nn_float(pi.astype(np.float32), tar[:, 0:3])
        useful = 0
        if len(tar):
            tp = tar[idx, 0:3].astype(np.float64); tn = tar[idx, 3:6].astype(np.float64)
            ninc = norm3(ni - tn); nadd = norm3(ni + tn)
            d = pi - tp
            p2p = np.abs((tn[:, 0] * d[:, 0] + tn[:, 1] * d[:, 1]) + tn[:, 2] * d[:, 2])
            useful = int((((ninc < self.cfg["normal_threshold"]) | (nadd < self.cfg["normal_threshold"])) & (p2p < self.cfg["dis_threshold"])).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.float64(useful) / np.float64(len(src))

    def search_loop(self, rows, bits, pl_cur):
        """SearchLoop (BTC.cpp:205-256): (result dict, candidate list)."""
        rows = np.asarray(rows, np.float64).reshape(-1, 19)
        if len(rows) == 0:
            return dict(loop_id=-1, score=0.0, t=None, R=None), []
        qi, dj = self.match_list(rows, bits)
        mframes = self.rows[dj][:, 6].astype(np.int64)
        cands = []
        best, best_c = 0.0, -1
        for f, v in self.candidates(mframes):
            sel = mframes == f
            r = self.verify(rows, qi[sel], dj[sel], pl_cur)
            if r["R"] is not None:
                r["score"] = self.plane_geometric_verify(pl_cur, self.clouds[f], r["R"], r["t"])
            r.update(frame=f, votes=v, match_len=int(sel.sum()))
            cands.append(r)
            if r["score"] > best:
                best, best_c = r["score"], len(cands) - 1
        if best_c >= 0 and best > self.cfg["icp_threshold"]:
            c = cands[best_c]
            return dict(loop_id=c["frame"], score=best, t=c["t"], R=c["R"]), cands
        return dict(loop_id=-1, score=0.0, t=None, R=None), cands


# --- icp_normal (loop_refine.hpp:47-139)
def so3_exp(w):
    """tools.hpp:51-66."""
    n = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if n < 1e-11:
        return np.eye(3)
    a = np.asarray(w) / n
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(n) * K + (1.0 - math.cos(n)) * (K @ K)


def ldlt_solve(A, b):
    """vbh::ldlt_solve_inplace (Eigen's LDLT with diagonal pivoting), restated."""
    A = np.array(A, dtype=np.float64)
    n = len(b)
    tr = list(range(n))
    for k in range(n):
        piv = k
        big = abs(A[k, k])
        for i in range(k + 1, n):
            if abs(A[i, i]) > big:
                big, piv = abs(A[i, i]), i
        tr[k] = piv
        if piv != k:
            for j in range(k):
                A[k, j], A[piv, j] = A[piv, j], A[k, j]
            for i in range(piv + 1, n):
                A[i, k], A[i, piv] = A[i, piv], A[i, k]
            A[k, k], A[piv, piv] = A[piv, piv], A[k, k]
            for i in range(k + 1, piv):
                A[i, k], A[piv, i] = A[piv, i], A[i, k]
        if k > 0:
            tmp = [A[j, j] * A[k, j] for j in range(k)]
            s = 0.0
            for j in range(k):
                s += A[k, j] * tmp[j]
            A[k, k] -= s
            for i in range(k + 1, n):
                tt = 0.0
                for j in range(k):
                    tt += A[i, j] * tmp[j]
                A[i, k] -= tt
        akk = A[k, k]
        if k == 0 and not abs(akk) > 0.0:
            tr = list(range(n))
            break
        if abs(akk) > 0.0:
            for i in range(k + 1, n):
                A[i, k] /= akk
    x = [float(v) for v in b]
    for k in range(n):
        if tr[k] != k:
            x[k], x[tr[k]] = x[tr[k]], x[k]
    for i in range(n):
        s = x[i]
        for j in range(i):
            s -= A[i, j] * x[j]
        x[i] = s
    for i in range(n):
        d = A[i, i]
        x[i] = x[i] / d if abs(d) > 2.2250738585072014e-308 else 0.0
    for i in range(n - 1, -1, -1):
        s = x[i]
        for j in range(i + 1, n):
            s -= A[j, i] * x[j]
        x[i] = s
    for k in range(n - 1, -1, -1):
        if tr[k] != k:
            x[k], x[tr[k]] = x[tr[k]], x[k]
    return np.array(x)


def icp_normal(src, tar, t, R, icp_eigval):
    """loop_refine.hpp:47-139 -> dict(ok, t, R, eig, iters, paras_switched)."""
    src = np.asarray(src, np.float32).reshape(-1, 6)
    tar = np.asarray(tar, np.float32).reshape(-1, 6)
    t = np.array(t, np.float64).reshape(3); R = np.array(R, np.float64).reshape(3, 3)
    paras = [0.2, 0.2, 0.5, 3.0]
    is_conv = 0
    p = src[:, 0:3].astype(np.float64); n = src[:, 3:6].astype(np.float64)
    tree = cKDTree(tar[:, 0:3].astype(np.float64)) if len(tar) else None
    mat_norm = np.zeros((3, 3))
    iters = 0
    for _ in range(20):
        iters += 1
        pi = p @ R.T + t
        ni = n @ R.T
        Hess = np.zeros((6, 6)); JacT = np.zeros(6); mat_norm = np.zeros((3, 3))
        if len(tar) and len(src):
            idx = _nn_tree(tree, pi.astype(np.float32), tar[:, 0:3])
            tp = tar[idx, 0:3].astype(np.float64); tn = tar[idx, 3:6].astype(np.float64)
            d = pi - tp
            ninc = norm3(ni - tn); nadd = norm3(ni + tn)
            p2p = norm3(d)
            rr = (tn[:, 0] * d[:, 0] + tn[:, 1] * d[:, 1]) + tn[:, 2] * d[:, 2]
            ok = ((ninc < paras[0]) | (nadd < paras[1])) & (np.abs(rr) < paras[2]) & (p2p < paras[3])
            pl, tnk, rk = p[ok], tn[ok], rr[ok]
            RtN = tnk @ R                                          # R^T tni, per row
            jh = np.cross(pl, RtN)                                 # hat(plocal) R^T tni
            jac = np.concatenate([jh, tnk], axis=1)
            Hess = jac.T @ jac
            JacT = jac.T @ rk
            mat_norm = tnk.T @ tnk
        dxi = ldlt_solve(Hess, -JacT)
        R = R @ so3_exp(dxi[0:3])
        t = t + dxi[3:6]
        if np.linalg.norm(dxi[0:3]) < 1e-3 and np.linalg.norm(dxi[3:6]) < 1e-3:
            if is_conv:
                break
            paras = [0.1, 0.1, 0.1, 1.0]
            is_conv = 1
    eig = np.linalg.eigvalsh(mat_norm)
    return dict(ok=int(eig[0] > icp_eigval and is_conv == 1), t=t, R=R, eig=eig, iters=iters, is_converge=is_conv)


def _nn_tree(tree, q32, cloud32):
    q = np.asarray(q32, np.float32).reshape(-1, 3)
    c = np.asarray(cloud32, np.float32).reshape(-1, 3)
    k = min(8, len(c))
    _, cand = tree.query(q.astype(np.float64), k=k)
    cand = np.asarray(cand).reshape(len(q), k)
    d = q[:, None, :] - c[cand]
    dd = d[..., 0] * d[..., 0]
    dd = dd + d[..., 1] * d[..., 1]
    dd = dd + d[..., 2] * d[..., 2]
    m = dd.min(axis=1, keepdims=True)
    out = np.where(dd == m, cand, np.iinfo(np.int64).max).min(axis=1)
    # k candidates do not answer a query whose last candidate (the farthest in double) still ties the minimum in float (nine or more coincident or
    # equidistant points, or a float rounding that promotes a farther double-neighbour): those rows by brute force, lowest index
    if k < len(c):
        for i in np.nonzero(dd[:, -1] == m[:, 0])[0]:
            e = q[i][None, :] - c
            ee = e[:, 0] * e[:, 0]
            ee = ee + e[:, 1] * e[:, 1]
            ee = ee + e[:, 2] * e[:, 2]
            out[i] = int(np.argmin(ee))
    return out
