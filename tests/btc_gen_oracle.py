"""numpy restatement of BTC descriptor generation for the tests of vba_btc_generate_stds: GenerateSTDescs (BTC.cpp:156-203) with
init_voxel_map, get_plane, get_project_plane, merge_plane, binary_extractor / extract_binary, non_maxi_suppression and
generate_std (BTC.cpp:279-1126), under the order contract of include/voxelba.h and DESIGN.md §11.  TEST INFRASTRUCTURE only.

Plane fits come from a host build of the solver code the kernels call (tests/host/btcgen_host.cpp, compiled with
-ffp-contract=off).  Every other floating-point expression is written in the reference's evaluation order; per-group sums are
sequential in input order (np.add.at), so the results are the device's bits.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KEY_OFF = 1 << 20
F32 = np.float32

_lib = None


def host_lib():
    """g++ build of tests/host/btcgen_host.cpp (the plane fit of vba_btcgen_fit.hpp)"""
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vba_btcg_"), "libbtcghost.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out,
                               os.path.join(HERE, "host", "btcgen_host.cpp")])
        _lib = C.CDLL(out)
    return _lib


def plane_eig(cov6):
    """cov6 [n][6] (a00 a10 a20 a11 a21 a22) -> (smallest eigenvalue [n], sign-ruled normal [n][3], direct-path flag [n])"""
    cov6 = np.ascontiguousarray(np.reshape(cov6, (-1, 6)), dtype=np.float64)
    n = len(cov6)
    w = np.zeros(n); nv = np.zeros((n, 3)); d = np.zeros(n, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    host_lib().btcg_plane_eig_host(C.c_int(n), cov6.ctypes.data_as(dp), w.ctypes.data_as(dp), nv.ctypes.data_as(dp),
                                   d.ctypes.data_as(C.POINTER(C.c_int)))
    return w, nv, d


def f(v):
    return float(np.float32(v))


def read_parameters(is_high_fly):
    """BTC.cpp:3-68, generation fields, float fields as float32 values"""
    h = bool(is_high_fly)
    return dict(useful_corner_num=200 if h else 100, plane_merge_normal_thre=f(0.3 if h else 0.1),
                plane_merge_dis_thre=f(0.6 if h else 0.3), plane_detection_thre=f(0.05 if h else 0.01), voxel_size=f(2 if h else 1),
                voxel_init_num=10, proj_plane_num=1 if h else 2, proj_image_resolution=f(0.5), proj_image_high_inc=f(0.2 if h else 0.1),
                proj_dis_min=f(0), proj_dis_max=f(10 if h else 5), summary_min_thre=f(6 if h else 10), line_filter_enable=0 if h else 1,
                touch_filter_enable=0, descriptor_near_num=f(15), descriptor_min_len=f(3 if h else 2), descriptor_max_len=f(50),
                non_max_suppression_radius=f(3 if h else 2), std_side_resolution=f(0.2))


def config_dict(cfg):
    if isinstance(cfg, dict):
        return dict(cfg)
    return {k: getattr(cfg, k) for k, _ in cfg._fields_}


def cut_num(cfg):
    return int((cfg["proj_dis_max"] - cfg["proj_dis_min"]) / cfg["proj_image_high_inc"])


def norm3(x, y, z):
    return np.sqrt(x * x + y * y + z * z)


class Plane:
    __slots__ = ("c", "n", "cov", "N", "d")

    def __init__(self, c, n, cov, N, d):
        self.c, self.n, self.cov, self.N, self.d = c, n, cov, N, d


def plane_d(n, c):
    return float(np.float32(-(n[0] * c[0] + n[1] * c[1] + n[2] * c[2])))


# ------------------------------------------------------------------------------------------------ voxels and planes
def voxel_keys(xyz, cfg):
    """init_voxel_map's grouping: (key [n][3] int64 per point, voxel ordinal per point, points per voxel).  The key is
    (int64_t)(p / voxel_size - (p / voxel_size < 0 ? 1 : 0)) in double; voxels are ordered by their first point"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    l = p.astype(np.float64) / float(cfg["voxel_size"])
    l = np.where(l < 0, l - 1.0, l)
    kk = l.astype(np.int64)
    k = kk + KEY_OFF
    key = (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    uniq, first, inv, cnt = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")          # voxel ordinal = rank of the first point
    rank = np.empty(len(uniq), np.int64); rank[order] = np.arange(len(uniq))
    return kk, rank[inv.reshape(-1)], cnt[order]


def voxel_planes(xyz, cfg):
    """init_voxel_map + init_plane + get_plane: list of Plane in voxel order (first-point order), planar voxels only"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    _, vox, counts = voxel_keys(p, cfg)
    V = len(counts)
    cand = counts > int(cfg["voxel_init_num"])
    d = p.astype(np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    S = np.zeros((V, 9))
    for j, v in enumerate((x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
        np.add.at(S[:, j], vox, v)                    # sequential in input order
    idx = np.flatnonzero(cand)
    S = S[idx]; N = counts[idx].astype(np.float64)
    c = S[:, 6:9] / N[:, None]
    cov = np.stack([S[:, 0] / N - c[:, 0] * c[:, 0], S[:, 1] / N - c[:, 1] * c[:, 0], S[:, 2] / N - c[:, 2] * c[:, 0],
                    S[:, 3] / N - c[:, 1] * c[:, 1], S[:, 4] / N - c[:, 2] * c[:, 1], S[:, 5] / N - c[:, 2] * c[:, 2]], axis=1)
    w, nv, _ = plane_eig(cov)
    ok = w < float(cfg["plane_detection_thre"])
    out = []
    for t in np.flatnonzero(ok):
        out.append(Plane(c[t].copy(), nv[t].copy(), cov[t].copy(), int(counts[idx[t]]), plane_d(nv[t], c[t])))
    return out


def plane_cloud(planes):
    a = np.zeros((len(planes), 6), np.float32)
    for i, q in enumerate(planes):
        a[i, :3] = q.c; a[i, 3:] = q.n
    return a


def greedy_ids(L, cfg):
    """the id assignment of get_project_plane / merge_plane (iter descending, iter2 ascending)"""
    m = len(L)
    ids = np.zeros(m, np.int64)
    if m < 2:
        return ids
    thn, thd = float(cfg["plane_merge_normal_thre"]), float(cfg["plane_merge_dis_thre"])
    n = np.array([q.n for q in L]); c = np.array([q.c for q in L]); d = np.array([q.d for q in L], np.float64)
    cur = 1
    for r in range(m - 1, 0, -1):
        nr, cr = n[r], c[r]
        nj, cj = n[:r], c[:r]
        nd = norm3(nr[0] - nj[:, 0], nr[1] - nj[:, 1], nr[2] - nj[:, 2])
        na = norm3(nr[0] + nj[:, 0], nr[1] + nj[:, 1], nr[2] + nj[:, 2])
        d1 = np.abs(nr[0] * cj[:, 0] + nr[1] * cj[:, 1] + nr[2] * cj[:, 2] + d[r])
        d2 = np.abs(nj[:, 0] * cr[0] + nj[:, 1] * cr[1] + nj[:, 2] * cr[2] + d[:r])
        ps = ((nd < thn) | (na < thn)) & ((d1 < thd) & (d2 < thd))
        for j in np.flatnonzero(ps):
            if ids[r] == 0 and ids[j] == 0:
                ids[r] = cur; ids[j] = cur; cur += 1
            elif ids[r] == 0 and ids[j] != 0:
                ids[r] = ids[j]
            elif ids[r] != 0 and ids[j] == 0:
                ids[j] = ids[r]
    return ids


RR = (0, 1, 2, 1, 2, 2)
CC = (0, 0, 0, 1, 1, 2)


def fold(L, ids, i):
    """BTC.cpp:382-402: members in ascending index from the first, then the eigen-solve"""
    a_c = L[i].c.copy(); a_cov = L[i].cov.copy(); a_N = L[i].N
    for j in range(i + 1, len(L)):
        if ids[j] != ids[i]:
            continue
        b = L[j]
        n1, n2, nt = float(a_N), float(b.N), float(a_N + b.N)
        P1 = np.array([(a_cov[k] + a_c[RR[k]] * a_c[CC[k]]) * n1 for k in range(6)])
        P2 = np.array([(b.cov[k] + b.c[RR[k]] * b.c[CC[k]]) * n2 for k in range(6)])
        mc = np.array([(a_c[k] * n1 + b.c[k] * n2) / nt for k in range(3)])
        a_cov = np.array([(P1[k] + P2[k]) / nt - mc[RR[k]] * mc[CC[k]] for k in range(6)])
        a_c = mc; a_N = a_N + b.N
    _, nv, _ = plane_eig(a_cov)
    return Plane(a_c, nv[0], a_cov, a_N, plane_d(nv[0], a_c))


def groups(L, ids, keep_singles):
    out, seen = [], set()
    for i in range(len(L)):
        if ids[i] in seen:
            continue
        if ids[i] == 0:
            if keep_singles:
                out.append(L[i])
            continue
        seen.add(ids[i])
        out.append(fold(L, ids, i))
    return out


def stable_sort_planes(L):
    return sorted(L, key=lambda q: -q.N)               # Python's sort is stable


def projection_planes(planes, xyz0, cfg):
    """get_project_plane, sort, merge_plane, sort; single_plane when nothing merged: list of (center, normal)"""
    G = groups(planes, greedy_ids(planes, cfg), False)
    if not G:
        return [(np.array([float(xyz0[0]), float(xyz0[1]), float(xyz0[2])]), np.array([0.0, 0.0, 1.0]))], 0
    srt = stable_sort_planes(G)
    if len(srt) == 1:
        E = srt
    else:
        E = stable_sort_planes(groups(srt, greedy_ids(srt, cfg), True))
    return [(q.c, q.n) for q in E], len(G)


# ------------------------------------------------------------------------------------------------ extract_binary
def axes(c, n):
    A, B, Cn = n
    D = -(A * c[0] + B * c[1] + Cn * c[2])
    x = [1.0, 1.0, 0.0]
    if Cn != 0:
        x[2] = -(A + B) / Cn
    elif B != 0:
        x[1] = -A / B
    else:
        x[0] = 0.0; x[1] = 1.0
    z = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
    if z > 0:
        q = float(np.sqrt(z)); x = [x[0] / q, x[1] / q, x[2] / q]
    y = [n[1] * x[2] - n[2] * x[1], n[2] * x[0] - n[0] * x[2], n[0] * x[1] - n[1] * x[0]]
    z = y[0] * y[0] + y[1] * y[1] + y[2] * y[2]
    if z > 0:
        q = float(np.sqrt(z)); y = [y[0] / q, y[1] / q, y[2] / q]
    dx = -(x[0] * c[0] + x[1] * c[1] + x[2] * c[2])
    dy = -(y[0] * c[0] + y[1] * c[1] + y[2] * c[2])
    return A, B, Cn, D, x, y, dx, dy


def extract_binary(c, n, xyz, cfg):
    """corners of one projection plane: list of (loc [3], summary, bits)"""
    A, B, Cn, D, xa, ya, dx, dy = axes(c, n)
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    dmin, dmax, res, hinc = float(cfg["proj_dis_min"]), float(cfg["proj_dis_max"]), float(cfg["proj_image_resolution"]), float(cfg["proj_image_high_inc"])
    dis = np.abs(x * A + y * B + z * Cn + D)
    keep = ~((dis < dmin) | (dis > dmax))
    x, y, z, dis = x[keep], y[keep], z[keep], dis[keep]
    if len(x) <= 5:
        return []
    den = A * A + B * B + Cn * Cn
    p0 = (-A * (B * y + Cn * z + D) + x * (B * B + Cn * Cn)) / den
    p1 = (-B * (A * x + Cn * z + D) + y * (A * A + Cn * Cn)) / den
    p2 = (-Cn * (A * x + B * y + D) + z * (A * A + B * B)) / den
    X = p0 * ya[0] + p1 * ya[1] + p2 * ya[2] + dy
    Y = p0 * xa[0] + p1 * xa[1] + p2 * xa[2] + dx
    minx, maxx = min(10.0, float(X.min())), max(-10.0, float(X.max()))
    miny, maxy = min(10.0, float(Y.min())), max(-10.0, float(Y.max()))
    seg = 5 * res
    xseg, yseg = int((maxx - minx) / seg + 1), int((maxy - miny) / seg + 1)
    xlen, ylen = int((maxx - minx) / res + 5), int((maxy - miny) / res + 5)
    xi = ((X - minx) / res).astype(np.int64); yi = ((Y - miny) / res).astype(np.int64)
    cell = xi * ylen + yi
    uc, inv = np.unique(cell, return_inverse=True)
    inv = inv.reshape(-1)
    sx = np.zeros(len(uc)); sy = np.zeros(len(uc)); cnt = np.zeros(len(uc), np.int64)
    np.add.at(sx, inv, X); np.add.at(sy, inv, Y); np.add.at(cnt, inv, 1)
    cn = cut_num(cfg)
    ci = ((dis - dmin) / hinc).astype(np.int64)
    bits = np.zeros(len(uc), np.uint64)
    ok = ci < cn
    np.bitwise_or.at(bits, inv[ok], np.left_shift(np.uint64(1), ci[ok].astype(np.uint64)))
    summ = np.bitwise_count(bits).astype(np.int64)
    img = np.zeros((max(xlen, xseg * 5), max(ylen, yseg * 5)), np.int64)
    img[uc // ylen, uc % ylen] = summ
    pos = {int(u): k for k, u in enumerate(uc)}
    out = []
    smin = float(cfg["summary_min_thre"])
    for xs in range(xseg):
        for ys in range(yseg):
            blk = img[xs * 5:xs * 5 + 5, ys * 5:ys * 5 + 5].reshape(-1)
            t = int(np.argmax(blk))                     # first maximum in x-then-y order
            md = float(blk[t])
            if not (md > 0):
                continue                                # nothing beat 0: (-10, -10) fails the bound test
            bx, by = xs * 5 + t // 5, ys * 5 + t % 5
            if not (md >= smin):
                continue
            if bx <= 0 or bx >= xlen - 1 or by <= 0 or by >= ylen - 1:
                continue
            k = pos[bx * ylen + by]
            if cfg["touch_filter_enable"] and (int(bits[k]) & 0xF) == 0:
                continue
            add = True
            if cfg["line_filter_enable"]:
                v = float(img[bx, by])
                for ddx, ddy in ((0, 1), (1, 0), (1, 1), (1, -1)):
                    v1, v2 = float(img[bx + ddx, by + ddy]), float(img[bx - ddx, by - ddy])
                    thr = v - 3
                    if v1 >= thr and v2 >= 0.5 * v: add = False
                    if v2 >= thr and v1 >= 0.5 * v: add = False
                    if v1 >= thr and v2 >= thr: add = False
            if not add:
                continue
            cnv = float(cnt[k])
            px, py = sx[k] / cnv, sy[k] / cnv
            loc = np.array([py * xa[j] + px * ya[j] + c[j] for j in range(3)])
            out.append((loc, int(summ[k]), int(bits[k])))
    return out


def binary_extractor(proj, xyz, cfg):
    temp = []
    last = np.zeros(3)
    used = 0
    for c, n in proj:
        n = np.asarray(n, np.float64)
        if norm3(*(n - last)) < 0.3 or norm3(*(n + last)) > 0.3:
            last = n; used += 1
            temp += extract_binary(c, n, xyz, cfg)
            if used == cfg["proj_plane_num"]:
                break
    return select_corners(temp, cfg)


def select_corners(temp, cfg):
    """binary_extractor's tail: non_maxi_suppression, then (useful_corner_num <= size) the stable sort by summary and the first
    useful_corner_num; useful_corner_num > size keeps the list as it is"""
    temp = nms(temp, cfg)
    if cfg["useful_corner_num"] > len(temp):
        return temp
    order = sorted(range(len(temp)), key=lambda i: -temp[i][1])   # stable
    return [temp[i] for i in order[:cfg["useful_corner_num"]]]


def pairwise_d2(P):
    P = np.asarray(P, np.float32)
    dx = P[:, None, 0] - P[None, :, 0]; dy = P[:, None, 1] - P[None, :, 1]; dz = P[:, None, 2] - P[None, :, 2]
    return dx * dx + dy * dy + dz * dz


def nms(temp, cfg):
    if not temp:
        return temp
    r = float(cfg["non_max_suppression_radius"])
    r2 = np.float32(r * r)
    P = np.array([t[0] for t in temp]).astype(np.float32)
    s = np.array([t[1] for t in temp])
    d2 = pairwise_d2(P)
    near = d2 < r2
    np.fill_diagonal(near, False)
    drop = (near & (s[:, None] <= s[None, :])).any(axis=1)
    return [t for t, dr in zip(temp, drop) if not dr]


# ------------------------------------------------------------------------------------------------ generate_std
def generate_std(corners, frame_id, cfg, stats=None):
    """rows [n][19] and masks [n][3] in emission order (first key wins); stats["dupes"] = triangles dropped as repeated keys"""
    N = len(corners)
    K = int(cfg["descriptor_near_num"])
    Kf = min(K, N)
    scale = 1.0 / float(cfg["std_side_resolution"])
    mn, mx = float(cfg["descriptor_min_len"]), float(cfg["descriptor_max_len"])
    rows, bits, seen = [], [], set()
    if N == 0:
        return np.zeros((0, 19)), np.zeros((0, 3), np.uint64)
    P = np.array([t[0] for t in corners]).astype(np.float32)
    d2 = pairwise_d2(P)
    ar = np.arange(N)
    for i in range(N):
        nb = np.lexsort((ar, d2[i]))[:Kf]
        for m in range(1, Kf - 1):
            for nn in range(m + 1, Kf):
                ci = [i, int(nb[m]), int(nb[nn])]
                p1, p2, p3 = P[ci[0]], P[ci[1]], P[ci[2]]
                da, db_, dc = p1 - p2, p1 - p3, p3 - p2          # float32 differences
                a = float(np.sqrt(float(da[0]) * float(da[0]) + float(da[1]) * float(da[1]) + float(da[2]) * float(da[2])))
                b = float(np.sqrt(float(db_[0]) * float(db_[0]) + float(db_[1]) * float(db_[1]) + float(db_[2]) * float(db_[2])))
                c = float(np.sqrt(float(dc[0]) * float(dc[0]) + float(dc[1]) * float(dc[1]) + float(dc[2]) * float(dc[2])))
                if a > mx or b > mx or c > mx or a < mn or b < mn or c < mn:
                    continue
                l1, l2, l3 = [1, 2, 0], [1, 0, 3], [0, 2, 3]
                if a > b:
                    a, b = b, a; l1, l2 = l2, l1
                if b > c:
                    b, c = c, b; l2, l3 = l3, l2
                if a > b:
                    a, b = b, a; l1, l2 = l2, l1
                if abs(c - (a + b)) < 0.2:
                    continue
                key = (int(np.float32(a * 1000)), int(np.float32(b * 1000)), int(np.float32(c * 1000)))
                if key in seen:
                    if stats is not None:
                        stats["dupes"] = stats.get("dupes", 0) + 1
                    continue
                seen.add(key)
                va = 0 if l1[0] == l2[0] else (1 if l1[1] == l2[1] else 2)
                vb = 0 if l1[0] == l3[0] else (1 if l1[1] == l3[1] else 2)
                vc = 0 if l2[0] == l3[0] else (1 if l2[1] == l3[1] else 2)
                V = [ci[va], ci[vb], ci[vc]]
                cen = [(float(P[V[0], k]) + float(P[V[1], k]) + float(P[V[2], k])) / 3 for k in range(3)]
                row = [scale * a, scale * b, scale * c] + cen + [float(frame_id)]
                for v in V:
                    row += [float(q) for q in corners[v][0]]
                row += [float(corners[v][1]) for v in V]
                rows.append(row)
                bits.append([corners[v][2] for v in V])
    return np.array(rows, np.float64).reshape(-1, 19), np.array(bits, np.uint64).reshape(-1, 3)


def generate_stds(xyz, frame_id, cfg):
    """GenerateSTDescs: dict(planes [p][6] float32, corners (loc [n][3], summ [n], bits [n]), rows, bits, groups)"""
    cfg = config_dict(cfg)
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    if len(p) == 0:
        return dict(planes=np.zeros((0, 6), np.float32), corners=(np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(0, np.uint64)),
                    rows=np.zeros((0, 19)), bits=np.zeros((0, 3), np.uint64), groups=0, dupes=0)
    planes = voxel_planes(p, cfg)
    proj, G = projection_planes(planes, p[0], cfg)
    corners = binary_extractor(proj, p, cfg)
    st = {}
    rows, bits = generate_std(corners, frame_id, cfg, st)
    cl = np.array([t[0] for t in corners]).reshape(-1, 3)
    return dict(planes=plane_cloud(planes), corners=(cl, np.array([t[1] for t in corners], np.int64),
                                                      np.array([t[2] for t in corners], np.uint64)),
                rows=rows, bits=bits, groups=G, dupes=st.get("dupes", 0))
