"""Restatement of the local-map display export (vba_map_display) in numpy, from (a) the CPU oracle's leaf dump,
(b) the window's scans and (c) one pose per scan.  A helper module shared by tests/test_map_display_cpu.py (the restatement against
the oracle's own point counts) and tests/test_gpu_map_display.py (the device against the restatement).

The leaf of a window point is found by geometric descent: root key VM:1907-1918, root centre (0.5 + k) voxel_size with
quater_length = voxel_size / 4 (a float), octant 4 [x > cx] + 2 [y > cy] + [z > cz] (VM:1315-1320), child centre and size VM:1328-1332,
path = octant at layer 1, then 8 path + octant (oracle/map_oracle.hpp:555-573); the descent stops at the first (key, layer, path) of
the dump.  This is exact only when every scan keeps ONE pose from insertion to display: the sessions below insert, recut, marginalise
and display with the scans' R0/p0 poses and run no LM step (evaluate_only_residual before a marginalisation moves no pose)."""
import dataclasses

import numpy as np

import eig3_ref


def world(pnt, pose12):
    """x_buf[i].R pnt + x_buf[i].p in the uncontracted order ((R0 x + R1 y) + R2 z) + p, doubles"""
    T = np.asarray(pose12, dtype=np.float64)
    p = np.asarray(pnt, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[3 * r] * x + T[3 * r + 1] * y) + T[3 * r + 2] * z) + T[9 + r] for r in range(3)], axis=1)


def root_keys(pw, voxel_size):
    """VM:1907-1918: narrowed to float, -1 if negative, truncated toward zero"""
    loc = (pw / voxel_size).astype(np.float32)
    loc = np.where(loc < 0, loc - np.float32(1.0), loc).astype(np.float32)
    return np.trunc(loc).astype(np.int64)


def leaf_table(dump):
    """(kx, ky, kz, layer, path) -> row of the dump"""
    return {tuple(int(v) for v in r[:5]): i for i, r in enumerate(dump)}


def assign(pw, table, voxel_size, max_layer):
    """row of the dump that holds each world point, -1 when the descent finds no leaf"""
    n = len(pw)
    key = root_keys(pw, voxel_size)
    c = (0.5 + key) * voxel_size
    ql = np.float32(voxel_size / 4.0)
    path = np.zeros(n, dtype=np.int64)
    out = np.full(n, -1, dtype=np.int64)
    kl = key.tolist()
    for layer in range(max_layer + 1):
        pl = path.tolist()
        for j in np.flatnonzero(out < 0).tolist():
            out[j] = table.get((kl[j][0], kl[j][1], kl[j][2], layer, pl[j]), -1)
        if layer == max_layer:
            break
        b = (pw > c).astype(np.int64)
        octant = 4 * b[:, 0] + 2 * b[:, 1] + b[:, 2]
        c = c + (2 * b - 1).astype(np.float32) * ql         # an int times a float is a float (exact), added to the double centre
        ql = np.float32(ql / np.float32(2.0))
        path = octant if layer == 0 else 8 * path + octant
    return out


def leaf_geometry(key5, voxel_size):
    """(voxel_center double [3], half edge float) of the leaf (kx, ky, kz, layer, path)"""
    kx, ky, kz, layer, path = (int(v) for v in key5)
    c = (0.5 + np.array([kx, ky, kz], dtype=np.float64)) * voxel_size
    ql = np.float32(voxel_size / 4.0)
    octs = []
    for _ in range(layer):
        octs.append(path & 7); path >>= 3
    for o in reversed(octs):
        b = np.array([(o >> 2) & 1, (o >> 1) & 1, o & 1])
        c = c + (2 * b - 1).astype(np.float32) * ql
        ql = np.float32(ql / np.float32(2.0))
    return c, np.float32(2.0) * ql


_EIG = {}


def plane_eig(row):
    """high-precision eigen-data of the leaf's cov, cached by the sums' bytes (the sessions revisit most leaves unchanged)"""
    k = row[22:32].tobytes()
    if k not in _EIG:
        _EIG[k] = eig3_ref.ref_from_sums(row[22:32])
    return _EIG[k]


def plane_exact(row, voxel_size):
    """the floats of a plane record that are bit for bit: 0..3, 7, 11..15 (the others stay NaN)"""
    rec = np.full(16, np.nan, dtype=np.float32)
    N = row[31]
    rec[0:3] = (row[28:31] / N).astype(np.float32)
    vc, half = leaf_geometry(row[:5], voxel_size)
    rec[3] = half
    rec[7] = np.float32(row[3])
    rec[11] = np.float32(N)
    rec[12:15] = vc.astype(np.float32)
    rec[15] = np.float32(N - row[6])
    return rec


def place(dump, scans, poses, voxel_size, max_layer):
    """per frame (world points, row of the dump that holds each): the descent, done once for both forms of display()"""
    table = leaf_table(dump)
    out = []
    for pnt, T in zip(scans, poses):
        pw = world(pnt, T)
        out.append((pw, assign(pw, table, voxel_size, max_layer) if len(pw) else np.zeros(0, dtype=np.int64)))
    return out


def display(dump, scans, poses, voxel_size, max_layer, all_points=False, placed=None):
    """What vba_map_display returns, up to the order of the planes: per frame the records (xyzi float32 [m][4]), the key of each record's
    leaf (int64 [m][5]) and whether that leaf is planar; the planar leaves' keys; frame_begin; and the per-leaf point counts of the
    WHOLE window with the number of points the descent could not place.  placed = place(...) of the same arguments, when at hand."""
    planar = dump[:, 7] != 0 if len(dump) else np.zeros(0, dtype=bool)
    keys = dump[:, :5].astype(np.int64) if len(dump) else np.zeros((0, 5), dtype=np.int64)
    counts = np.zeros(len(dump), dtype=np.int64)
    frames, unassigned = [], 0
    fb = [0]
    for i, (pw, leaf) in enumerate(placed if placed is not None else place(dump, scans, poses, voxel_size, max_layer)):
        unassigned += int((leaf < 0).sum())
        np.add.at(counts, leaf[leaf >= 0], 1)
        in_plane = planar[np.maximum(leaf, 0)] if len(dump) else np.zeros(len(leaf), dtype=bool)
        keep = (leaf >= 0) & (True if all_points else in_plane)
        xyzi = np.concatenate([pw[keep].astype(np.float32), np.full((int(keep.sum()), 1), np.float32(i), dtype=np.float32)], axis=1)
        frames.append({"xyzi": xyzi, "key": keys[leaf[keep]], "planar": planar[leaf[keep]]})
        fb.append(fb[-1] + len(xyzi))
    return {"frames": frames, "frame_begin": np.array(fb, dtype=np.int64), "plane_keys": keys[planar], "plane_rows": np.flatnonzero(planar),
            "counts": counts, "unassigned": unassigned}


def sorted_records(xyzi, key):
    """the records of one frame with their leaf keys appended, sorted by bytes: [m] rows of 16 + 40 bytes"""
    a = np.concatenate([np.ascontiguousarray(xyzi, dtype=np.float32).view(np.uint8).reshape(len(xyzi), 16),
                        np.ascontiguousarray(key, dtype=np.int64).view(np.uint8).reshape(len(key), 40)], axis=1)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


# ---------------------------------------------------------------- the sessions
def make_session(synth, n_pts, nscan, W=4):
    """room20k_w4 cut to n_pts rays per scan: (workload with win_size W, scans, poses [nscan][12] = R0 / p0)"""
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=W, n_pts=n_pts)
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    return wl, s["points"], synth.poses_flat(s["R0"], s["p0"])


def run_session(sides, scans, poses, W, on_state, multi=True):
    """The steady-state loop of local mapping without its LM step on every side of `sides` (objects with cut_voxel / recut / margi /
    slide / evaluate_only_residual taking the arguments of capi.Context): per scan insert and recut, with a full window evaluate,
    marginalise and slide.  on_state(kind, win) is called after every recut and every margi + slide, win = the scans in the window."""
    win = []
    for k in range(len(scans)):
        win.append(k)
        for s in sides:
            s.cut_voxel(len(win) - 1, scans[k], poses[k], multi=multi)
            s.recut(len(win), poses[win], multi=multi)
        on_state("recut", list(win))
        if len(win) >= W:
            for s in sides:
                s.evaluate_only_residual(poses[win])
                s.margi(len(win), poses[win], jour=float(k))
                s.slide(1)
            win = win[1:]
            on_state("margi", list(win))


class OracleSide:
    """oracle_api.VoxelMap + Factor behind the call shapes of capi.Context"""

    def __init__(self, oracle, wl, thread_num=5):
        self.m = oracle.VoxelMap(wl.win_size, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, thread_num)
        self.f = oracle.Factor(wl.win_size)

    def cut_voxel(self, win_count, pnt, pose, multi=False):
        self.m.cut_voxel(win_count, pnt, pose, multi=multi)

    def recut(self, win_count, poses, multi=False):
        self.m.recut(win_count, poses, self.f, multi=multi)

    def evaluate_only_residual(self, poses):
        self.f.evaluate_only_residual(poses)

    def margi(self, win_count, poses, jour=0.0):
        self.m.margi(win_count, poses, self.f, jour=jour)

    def slide(self, n):
        self.m.slide(n)

    def dump_leaves(self):
        return self.m.dump_leaves()
