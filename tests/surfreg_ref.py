"""Plain numpy restatement of the surfel map and of the registration against it (vba_surfel_map_build, vba_surfel_register,
include/voxelba.h) on top of tests/surfel_ref.py and tests/export_voxel_ref.py: the map from (records, cov),
one pass (cell, gate, the 29 terms of every point in the operation order of csrc/vba_surfreg_math.hpp, the sums as a chain), the
loop, the exact sums at 60 digits with a bar valid for any order of the additions, the check of W and of the step by residual, the
scans and starts of the tests, and the driver of tests/host/surfreg_host.cpp.  TEST INFRASTRUCTURE only.

numpy's elementwise operations round every product and sum on its own (nothing is fused), which is what the contract needs."""
import os
import struct
import subprocess

import mpmath
import numpy as np

import export_voxel_ref as ev
import kf_oracle as ko
import solve_ref
import surfel_ref as sr

U = 2.0 ** -53
MP_DPS = 60
PART = 29
ORDER = ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))     # own, -x, +x, -y, +y, -z, +z
TERM_ROUNDINGS = 10          # the deepest path of one term from (A, W, d): W A (5 roundings), A^T (W A) (5); d^T (W d) likewise


# ------------------------------------------------------------------------------------------------ the map
def axis_keys(pts, voxel):
    """int64 [n][3] of float coordinates: the down-samplers' per-axis index with both quirks"""
    return ko.voxel_keys(np.asarray(pts, dtype=np.float32), voxel, pvec=False)


def pack(k3):
    k = np.asarray(k3, dtype=np.int64) & 0x1FFFFF
    return (k[..., 0].astype(np.uint64) << np.uint64(42)) | (k[..., 1].astype(np.uint64) << np.uint64(21)) | k[..., 2].astype(np.uint64)


def weight(C, sigma, with_sigma=True):
    """W [n][6] = (C + sigma^2 I)^-1 in the operation order of sreg_weight.  with_sigma False is the mutation W = C^-1."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 6)
    s2 = np.float64(sigma) * np.float64(sigma) if with_sigma else 0.0
    a, b, c, d, e, f = C[:, 0] + s2, C[:, 1], C[:, 2], C[:, 3] + s2, C[:, 4], C[:, 5] + s2
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = (a * c00 + b * c01) + c * c02
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        return np.stack([c00 * inv, c01 * inv, c02 * inv, c11 * inv, c12 * inv, c22 * inv], axis=1)


def weight_check(C, sigma, W):
    """max over the entries of |W (C + sigma^2 I) - I| / bar, the product formed at 60 digits.  The bar counts the roundings of
    sreg_weight (u = 2^-53): a cofactor is two products and a difference, |e_ik| <= 3 u cabs_ik with cabs the cofactor of the
    absolute values; the determinant along the first row adds three products and two sums on those, |det^ - det| <= 6 u dabs,
    dabs = sum_k |a_0k| cabs_0k; the reciprocal and the product 2 u.  With adj A = det I:
      |W A - I|_ij <= u (delta_ij (6 dabs / |det| + 2) + 3 sum_k cabs_ik |A_kj| / |det|), and 5 % for the second order."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 6); W = np.asarray(W, dtype=np.float64).reshape(-1, 6)
    worst = 0.0
    idx = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
    with mpmath.workdps(MP_DPS):
        s2 = mpmath.mpf(float(sigma)) ** 2
        for n in range(len(C)):
            A = [[mpmath.mpf(float(C[n, idx[i][j]])) + (s2 if i == j else 0) for j in range(3)] for i in range(3)]
            Wm = [[mpmath.mpf(float(W[n, idx[i][j]])) for j in range(3)] for i in range(3)]
            Aa = np.array([[float(abs(A[i][j])) for j in range(3)] for i in range(3)])
            a, b, c, d, e, f = Aa[0, 0], Aa[0, 1], Aa[0, 2], Aa[1, 1], Aa[1, 2], Aa[2, 2]
            cabs = np.array([[d * f + e * e, c * e + b * f, b * e + c * d], [c * e + b * f, a * f + c * c, b * c + a * e],
                             [b * e + c * d, b * c + a * e, a * d + b * b]])
            det = float(abs(mpmath.det(mpmath.matrix(A))))
            dabs = a * cabs[0, 0] + b * cabs[0, 1] + c * cabs[0, 2]
            for i in range(3):
                for j in range(3):
                    r = float(abs(mpmath.fsum(Wm[i][k] * A[k][j] for k in range(3)) - (1 if i == j else 0)))
                    bar = 1.05 * U * ((6.0 * dabs / det + 2.0) * (i == j) + 3.0 * float(cabs[i] @ Aa[:, j]) / det)
                    worst = max(worst, r / bar)
    return worst


class Map:
    """cells of the records with [11] >= min_count: sorted packed keys for the lookup, the row of each, c as doubles of the floats,
    W.  dup: two records met in one key.  Mutations: with_sigma False, ignore_min_count True."""

    def __init__(self, rec, cov, voxel, sigma, min_count, with_sigma=True, ignore_min_count=False):
        rec = np.asarray(rec, dtype=np.float32).reshape(-1, 12)
        self.voxel, self.sigma = float(voxel), float(sigma)
        keep = np.ones(len(rec), bool) if ignore_min_count else rec[:, 11] >= np.float32(min_count)
        self.rows = np.nonzero(keep)[0]
        self.keys = pack(axis_keys(rec[self.rows, :3], voxel))
        self.dup = len(np.unique(self.keys)) != len(self.keys)
        order = np.argsort(self.keys, kind="stable")
        self.skeys, self.srows = self.keys[order], self.rows[order]
        self.c = rec[:, :3].astype(np.float64)
        self.W = weight(cov, sigma, with_sigma)
        self.n_cells = len(self.rows)

    def lookup(self, keys):
        """row of every key, -1 where the map has no such cell"""
        if len(self.skeys) == 0:
            return np.full(len(keys), -1, np.int64)
        pos = np.minimum(np.searchsorted(self.skeys, keys), len(self.skeys) - 1)
        return np.where(self.skeys[pos] == keys, self.srows[pos], -1)


# ------------------------------------------------------------------------------------------------ one pass
def query(R, t, p):
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    return np.stack([((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)], axis=1)


def maha(W, d):
    Wd = np.stack([(W[:, 0] * d[:, 0] + W[:, 1] * d[:, 1]) + W[:, 2] * d[:, 2],
                   (W[:, 1] * d[:, 0] + W[:, 3] * d[:, 1]) + W[:, 4] * d[:, 2],
                   (W[:, 2] * d[:, 0] + W[:, 4] * d[:, 1]) + W[:, 5] * d[:, 2]], axis=1)
    return (d[:, 0] * Wd[:, 0] + d[:, 1] * Wd[:, 1]) + d[:, 2] * Wd[:, 2], Wd


def jac_rot(R, p, sign=-1.0):
    """A [n][9] = -R hat(p) in the order of sreg_terms; sign +1 is the mutation J = [+R hat(p) | I]"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    cols = []
    for r in range(3):
        cols += [R[r, 2] * y - R[r, 1] * z, R[r, 0] * z - R[r, 2] * x, R[r, 1] * x - R[r, 0] * y]
    A = np.stack(cols, axis=1)
    return A if sign < 0 else -A


def terms_of(A, W, Wd, m):
    """[n][29] in the operation order of sreg_terms"""
    Wm = [W[:, 0], W[:, 1], W[:, 2], W[:, 1], W[:, 3], W[:, 4], W[:, 2], W[:, 4], W[:, 5]]
    WA = [None] * 9
    for r in range(3):
        for c in range(3):
            WA[3 * r + c] = (Wm[3 * r] * A[:, c] + Wm[3 * r + 1] * A[:, 3 + c]) + Wm[3 * r + 2] * A[:, 6 + c]

    def ata(r, c):
        return (A[:, r] * WA[c] + A[:, 3 + r] * WA[3 + c]) + A[:, 6 + r] * WA[6 + c]

    def atv(r):
        return (A[:, r] * Wd[:, 0] + A[:, 3 + r] * Wd[:, 1]) + A[:, 6 + r] * Wd[:, 2]

    out = [ata(0, 0), ata(0, 1), ata(0, 2), WA[0], WA[3], WA[6], ata(1, 1), ata(1, 2), WA[1], WA[4], WA[7], ata(2, 2), WA[2], WA[5], WA[8],
           W[:, 0], W[:, 1], W[:, 2], W[:, 3], W[:, 4], W[:, 5], atv(0), atv(1), atv(2), Wd[:, 0], Wd[:, 1], Wd[:, 2], 0.5 * m, np.ones(len(m))]
    return np.stack(out, axis=1)


def one_pass(mp, pnt, R, t, gate=3.0, neighbors=7, jsign=-1.0, gate_squared=True, tie="earlier", order=ORDER):
    """dict(cell int64 [n] row or -1, gate bool [n], terms [n][29] (zero rows where the gate is shut), sums [29] the chain in point
    order, ties: points with two candidates of equal m at the minimum, d, W, A of the chosen cells).  Mutations: jsign +1,
    gate_squared False (m < gate), tie "later", another candidate order."""
    pnt = np.asarray(pnt, dtype=np.float64).reshape(-1, 3); t = np.asarray(t, dtype=np.float64).reshape(3)
    n = len(pnt)
    q = query(R, t, pnt)
    k3 = axis_keys(q, mp.voxel)
    best = np.full(n, -1, np.int64); bm = np.full(n, np.inf); bd = np.zeros((n, 3)); bWd = np.zeros((n, 3)); ties = np.zeros(n, bool)
    for off in order[:neighbors]:
        row = mp.lookup(pack(k3 + np.array(off, dtype=np.int64)))
        ok = row >= 0
        rr = np.where(ok, row, 0)
        d = q - mp.c[rr]
        m, Wd = maha(mp.W[rr], d)
        ties |= ok & (best >= 0) & (m == bm)
        take = ok & ((best < 0) | ((m <= bm) if tie == "later" else (m < bm)))
        best = np.where(take, row, best); bm = np.where(take, m, bm)
        bd[take] = d[take]; bWd[take] = Wd[take]
    lim = gate * gate if gate_squared else gate
    g = (best >= 0) & (bm < lim)
    rr = np.where(best >= 0, best, 0)
    A = jac_rot(R, pnt, jsign)
    T = terms_of(A, mp.W[rr], bWd, np.where(best >= 0, bm, 0.0))
    T[~g] = 0.0
    sums = np.zeros(PART)
    for k in range(PART):
        sums[k] = np.add.accumulate(T[g, k])[-1] if g.any() else 0.0          # the chain ((0 + t_0) + t_1) + ...
    return dict(cell=best, gate=g, terms=T, sums=sums, ties=ties, d=bd, W=mp.W[rr], A=A, Wd=bWd, m=bm)


def unpack_H(s):
    H = np.zeros((6, 6)); k = 0
    for r in range(6):
        for c in range(r, 6):
            H[r, c] = H[c, r] = s[k]; k += 1
    return H


def so3_exp(w):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(w, dtype=np.float64)).as_matrix()


def loop(mp, pnt, R, t, gate=3.0, neighbors=7, max_iter=30, min_matches=50, eps_rot=1e-5, eps_tra=1e-5, **mut):
    """the stop rules of sreg_step around one_pass, the solve by numpy (not bit for bit: the fixtures keep their iteration
    counts away from a last-bit decision) -> dict(iters, converged, lost, singular, matches, cost, step_rot, step_tra, R, t, H, g)"""
    R = np.array(R, dtype=np.float64).reshape(3, 3); t = np.array(t, dtype=np.float64).reshape(3)
    out = dict(iters=0, converged=0, lost=0, singular=0, matches=[], cost=[], step_rot=[], step_tra=[])
    for _ in range(max_iter):
        ps = one_pass(mp, pnt, R, t, gate, neighbors, **mut)
        s = ps["sums"]
        out["iters"] += 1; out["matches"].append(int(s[28])); out["cost"].append(float(s[27]))
        out["H"], out["g"] = unpack_H(s), s[21:27].copy()
        if int(s[28]) < min_matches:
            out["lost"] = 1; out["step_rot"].append(0.0); out["step_tra"].append(0.0); break
        try:
            dx = np.linalg.solve(out["H"], -out["g"])
        except np.linalg.LinAlgError:
            dx = np.full(6, np.nan)
        if not np.all(np.isfinite(dx)):
            out["singular"] = 1; out["step_rot"].append(0.0); out["step_tra"].append(0.0); break
        R = R @ so3_exp(dx[:3]); t = t + dx[3:]
        out["step_rot"].append(float(np.linalg.norm(dx[:3]))); out["step_tra"].append(float(np.linalg.norm(dx[3:])))
        if out["step_rot"][-1] < eps_rot and out["step_tra"][-1] < eps_tra:
            out["converged"] = 1; break
    out["R"], out["t"] = R, t
    return out


# ------------------------------------------------------------------------------------------------ the exact sums and the bar
def exact_sums(ps):
    """(sums [29], sum of |term| [29]) of the gated points of a pass, every term formed at 60 digits from the doubles the pass
    hands to sreg_terms (A = -R hat(p), W, d as rounded: the rounding of d = q - c, about u |q|, is the estimator's input and is
    held bit for bit by the per-point comparison, not by this bar) and summed exactly."""
    g = np.nonzero(ps["gate"])[0]
    tot = [mpmath.mpf(0)] * PART; ab = [mpmath.mpf(0)] * PART
    with mpmath.workdps(MP_DPS):
        tot = [mpmath.mpf(0) for _ in range(PART)]; ab = [mpmath.mpf(0) for _ in range(PART)]
        for i in g:
            A = [[mpmath.mpf(float(ps["A"][i, 3 * r + c])) for c in range(3)] for r in range(3)]
            w = [mpmath.mpf(float(x)) for x in ps["W"][i]]
            Wm = [[w[0], w[1], w[2]], [w[1], w[3], w[4]], [w[2], w[4], w[5]]]
            d = [mpmath.mpf(float(x)) for x in ps["d"][i]]
            WA = [[mpmath.fsum(Wm[r][k] * A[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
            Wd = [mpmath.fsum(Wm[r][k] * d[k] for k in range(3)) for r in range(3)]
            H = [[mpmath.mpf(0)] * 6 for _ in range(6)]
            for r in range(3):
                for c in range(3):
                    H[r][c] = mpmath.fsum(A[k][r] * WA[k][c] for k in range(3))
                    H[r][3 + c] = WA[c][r]
                    H[3 + r][3 + c] = Wm[r][c]
            gr = [mpmath.fsum(A[k][r] * Wd[k] for k in range(3)) for r in range(3)] + Wd
            m = mpmath.fsum(d[k] * Wd[k] for k in range(3))
            term = [H[r][c] for r in range(6) for c in range(r, 6)] + gr + [m / 2, mpmath.mpf(1)]
            for k in range(PART):
                tot[k] += term[k]; ab[k] += abs(term[k])
        return np.array([float(x) for x in tot]), np.array([float(x) for x in ab])


def sums_bar(matched, abs_sum):
    """|sum - exact| for additions in ANY order: a sum of N terms carries at most (N - 1) u sum |t| whatever the tree, each term its
    own TERM_ROUNDINGS roundings: (N + TERM_ROUNDINGS) u sum |t|, and 1 % for the second order.  The count (term 28) is exact."""
    bar = 1.01 * (matched + TERM_ROUNDINGS) * U * np.asarray(abs_sum, dtype=np.float64)
    bar[28] = 0.0
    return bar


def step_check(sums, dx):
    """(backward ratio, forward ratio) of H dx = -g by the exact residual, the method and bars of tests/solve_ref.py"""
    bw, fw, _ = solve_ref.ratios(unpack_H(sums), -np.asarray(sums[21:27]), np.asarray(dx, dtype=np.float64))
    return bw, fw


# ------------------------------------------------------------------------------------------------ scenes, scans, starts
VOXELS = (0.5, 1.0)
SIGMA = 0.02
MIN_COUNT = 5
GEN_SEED = 11
STARTS = {"small": (0.05, 0.5, 4), "large": (0.2, 2.0, 7)}          # name -> (metres, degrees, seed): seeds that meet the fixture conditions


def world(name):
    """(sessions, S) of the scene of surfel_ref: near, or far (shifted by about 1000 m)"""
    clouds, poses = sr.scene()
    P = poses if name == "near" else sr.shifted(poses)
    sessions = [(clouds, P, 2.0)]
    S, _ = ev.sequence(sessions, 1)
    return sessions, S


def scan_of(S, name):
    """(body points [1564][3], the generating pose R, t): every third record of S seen from a known pose"""
    rng = np.random.default_rng(GEN_SEED)
    Rg = so3_exp(rng.uniform(-0.3, 0.3, 3)); tg = rng.uniform(-1.0, 1.0, 3)
    if name == "far":
        tg = tg + sr.SHIFT
    w = S[::3, :3].astype(np.float64)
    return (w - tg) @ Rg, Rg, tg                             # R^T (w - t)


def start_of(Rg, tg, which):
    metres, degrees, seed = STARTS[which]
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3); a *= np.deg2rad(degrees) / np.linalg.norm(a)
    b = rng.normal(size=3); b *= metres / np.linalg.norm(b)
    return Rg @ so3_exp(a), tg + b


def pose_distance(R, t, Rg, tg):
    """(metres, radians) between two poses"""
    from scipy.spatial.transform import Rotation
    return float(np.linalg.norm(t - tg)), float(np.linalg.norm(Rotation.from_matrix(Rg.T @ np.asarray(R).reshape(3, 3)).as_rotvec()))


def records_of(S, voxel):
    """(records float32 [m][12], cov [m][6]) of every voxel of S in the export's order, with the fields the map reads: [0..2] the
    narrowed mean, [11] the count (the eigen fields of a real export stay zero: the map does not read them)"""
    mo = sr.moments(S, voxel)
    rec = np.zeros((len(mo["cnt"]), 12), np.float32)
    rec[:, :3] = mo["c"].astype(np.float32); rec[:, 11] = mo["cnt"]
    return rec, mo["C"]


def tie_case():
    """two cells of equal isotropic weight either side of the face x = 0.5 and a point on the face: own (row 1) and -x (row 0)
    give the same m exactly"""
    rec = np.zeros((2, 12), np.float32); rec[0, :3] = (0.25, 0.25, 0.25); rec[1, :3] = (0.75, 0.25, 0.25); rec[:, 11] = 10
    cov = np.tile(np.array([0.01, 0, 0, 0.01, 0, 0.01]), (2, 1))
    return rec, cov, np.array([[0.5, 0.25, 0.25]]), np.eye(3), np.zeros(3)


LOOP_CASES = [(scene, which, nb) for scene in ("near", "far") for which in ("small", "large") for nb in (1, 7)]
LOOP_VOXEL = {"small": 0.5, "large": 1.0}


def measure_spread(mp, pnt, R0, t0, nb, seed=99, count=16, size=1e-12):
    """(largest spread of a final R entry, of a final t component, of a cost[] slot relative to its size) of the restatement's loop
    from `count` starts that differ from (R0, t0) by +-size in each of the six pose components; the iteration counts and matches[]
    must not move"""
    rng = np.random.default_rng(seed)
    Rs, ts, cs, its = [], [], [], set()
    for _ in range(count):
        sg = rng.choice([-1.0, 1.0], 6) * size
        lp = loop(mp, pnt, R0 @ so3_exp(sg[:3]), t0 + sg[3:], neighbors=nb)
        Rs.append(lp["R"].ravel()); ts.append(lp["t"]); cs.append(lp["cost"]); its.add((lp["iters"], tuple(lp["matches"])))
    assert len(its) == 1, its
    Rs, ts, cs = np.array(Rs), np.array(ts), np.array(cs)
    return (float((Rs.max(0) - Rs.min(0)).max()), float((ts.max(0) - ts.min(0)).max()),
            float(((cs.max(0) - cs.min(0)) / np.abs(cs).max(0)).max()))


# measure_spread of every loop case, as measured: the final pose is a fixed point the iteration contracts
# to, so a 1e-12 change of the start moves it by rounding only; cost[0] moves by g . delta
SPREAD = {("near", "small", 1): (4.44e-16, 2.11e-15, 7.55e-11), ("near", "small", 7): (3.33e-16, 1.33e-15, 7.94e-11),
          ("near", "large", 1): (5.55e-16, 2.78e-15, 1.05e-10), ("near", "large", 7): (3.33e-16, 2.22e-15, 1.06e-10),
          ("far", "small", 1): (5.00e-16, 0.0, 7.61e-11), ("far", "small", 7): (5.27e-16, 0.0, 8.00e-11),
          ("far", "large", 1): (9.44e-16, 0.0, 1.20e-10), ("far", "large", 7): (8.33e-16, 0.0, 1.19e-10)}


def pose_bars(case, t):
    """(bar on |R - R'| per entry, on |t - t'| per component, on |cost - cost'| / |cost| per slot): 4 x the measured spread (the
    sample is small), and never below 4 units in the last place of the compared numbers (1 for R, max |t| for t): two libraries'
    sin and cos may round differently, and no comparison of doubles can ask for less than their spacing"""
    sR, sT, sC = SPREAD[case]
    return 4.0 * max(sR, 2.0 ** -52), 4.0 * max(sT, float(np.spacing(np.abs(t).max()))), 4.0 * sC


# ------------------------------------------------------------------------------------------------ the host program
def build_host(workdir, sanitize=False):
    """compile tests/host/surfreg_host.cpp without contraction; returns the program's path"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "surfreg_host_san" if sanitize else "surfreg_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + flags +
                          [os.path.join(root, "tests", "host", "surfreg_host.cpp"), "-o", exe])
    return exe


def build_adapter(workdir, lib_path):
    """compile tests/host/surfreg_adapter_host.cpp against libvoxelba.so, as the surfel export's adapter program is built"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "surfreg_adapter_host")
    libdir = os.path.dirname(lib_path)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "surfreg_adapter_host.cpp"), "-o", exe, "-L", libdir, "-lvoxelba",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def host_run(exe, workdir, rec, cov, pnt, R, t, voxel, sigma=SIGMA, min_count=MIN_COUNT, gate=3.0, neighbors=7, max_iter=1, min_matches=50,
             eps_rot=1e-5, eps_tra=1e-5, tag="run"):
    """the program's output as a dict: n_cells, slots, dup, eig_ok, key [n_rec], W [n_rec][6], the taps of iteration 0 (cell, gate,
    terms, sums, dx) and the state after the loop (R, t, done, iters, converged, lost, singular, matches, cost, step_rot, step_tra, H,
    g, eig_tt)"""
    rec = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 12); cov = np.ascontiguousarray(cov, dtype=np.float64).reshape(-1, 6)
    pnt = np.ascontiguousarray(pnt, dtype=np.float64).reshape(-1, 3)
    nr, npnt = len(rec), len(pnt)
    fin, fout = os.path.join(str(workdir), tag + "_in.bin"), os.path.join(str(workdir), tag + "_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qq5d4i", nr, npnt, voxel, sigma, gate, eps_rot, eps_tra, min_count, neighbors, max_iter, min_matches))
        f.write(np.ascontiguousarray(R, dtype=np.float64).reshape(9).tobytes()); f.write(np.ascontiguousarray(t, dtype=np.float64).reshape(3).tobytes())
        f.write(rec.tobytes()); f.write(cov.tobytes()); f.write(pnt.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    raw = open(fout, "rb").read()
    o = [0]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=o[0]).copy()
        o[0] += a.nbytes
        return a

    head = take(np.int64, 4)
    out = dict(n_cells=int(head[0]), slots=int(head[1]), dup=int(head[2]), eig_ok=int(head[3]))
    out["key"] = take(np.uint64, nr); out["W"] = take(np.float64, 6 * nr).reshape(nr, 6)
    out["cell"] = take(np.int32, npnt); out["gate"] = take(np.uint8, npnt); out["terms"] = take(np.float64, PART * npnt).reshape(npnt, PART)
    out["sums"] = take(np.float64, PART); out["dx"] = take(np.float64, 6)
    out["R"] = take(np.float64, 9).reshape(3, 3); out["t"] = take(np.float64, 3)
    take(np.float64, 3)                                       # gate2, eps_rot, eps_tra
    ints = take(np.int32, 4); out["done"] = int(ints[3])
    rep = take(np.int32, 4)
    out["iters"], out["converged"], out["lost"], out["singular"] = (int(x) for x in rep)
    out["matches"] = take(np.int32, 32); out["cost"] = take(np.float64, 32); out["step_rot"] = take(np.float64, 32); out["step_tra"] = take(np.float64, 32)
    out["H"] = take(np.float64, 21); out["g"] = take(np.float64, 6); out["eig_tt"] = take(np.float64, 3)
    assert o[0] == len(raw), (o[0], len(raw))
    return out
