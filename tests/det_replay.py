"""Host replay of the canonical numbering and order of deterministic mode (vba_options::deterministic).

The device contract, restated in numpy so that the GPU tests can check it on real dumps:
  - new roots of one insertion are ranked by the smallest index of an input point in their voxel; the r-th new root takes the
    r-th id of [free root ids ascending..., CNT_NODES, CNT_NODES + 1, ...];
  - the leaves a recut level splits are taken in ascending node id; the r-th takes the r-th block of [free blocks ascending...,
    fresh storage in steps of 8];
  - the factor store is ordered by (mask_bucket(occupancy mask), node id); dumps list leaves in ascending node id;
  - down-sampling adds each voxel's points in input order, then divides and rounds like k_ds_emit.
"""
import numpy as np


def world_points(pts, pose12):
    """world_point() of csrc/vba_kernels_map.hpp: ((R0 x + R1 y) + R2 z) + t, every operation rounded on its own."""
    R, t = pose12[:9], pose12[9:12]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + t[r] for r in range(3)], 1)


def key_axis(pw, voxel_size):
    """The reference's key quirk VM:1907-1918: float narrowing, -1 if negative, truncation toward zero."""
    loc = (pw / voxel_size).astype(np.float32)
    loc = np.where(loc < 0, loc - np.float32(1.0), loc).astype(np.float32)
    return np.trunc(loc).astype(np.int64)


def voxel_keys(world, voxel_size):
    return np.stack([key_axis(world[:, k], voxel_size) for k in range(3)], 1)


def first_touch_order(keys):
    """Distinct rows of `keys` in the order of their first occurrence."""
    _, first = np.unique(keys, axis=0, return_index=True)
    return keys[np.sort(first)]


class RootNumbering:
    """Node ids of roots as deterministic mode hands them out (free ids kept ascending, fresh ids counted up)."""

    def __init__(self):
        self.ids = {}            # voxel key -> node id
        self.free = []           # free root ids, ascending
        self.nodes = 0           # CNT_NODES

    def insert(self, keys):
        """One insertion call: returns the ids of the roots it creates, in rank order."""
        new = [tuple(int(v) for v in k) for k in first_touch_order(keys) if tuple(int(v) for v in k) not in self.ids]
        out = []
        for r, k in enumerate(new):
            if r < len(self.free):
                i = self.free[r]
            else:
                i = self.nodes + (r - len(self.free))
            self.ids[k] = i
            out.append(i)
        take = min(len(new), len(self.free))
        self.nodes += len(new) - take
        self.free = self.free[take:]
        return out

    def prune(self, dead_keys):
        for k in dead_keys:
            self.free.append(self.ids.pop(tuple(int(v) for v in k)))
        self.free.sort()

    def live_in_id_order(self):
        return np.array([k for k, _ in sorted(self.ids.items(), key=lambda kv: kv[1])], dtype=np.int64).reshape(-1, 3)


def allocate_blocks(split_ids, free_blocks, nodes):
    """Rule 2: the split leaves of one level (any order in) are taken in ascending id.  Returns ({leaf: base}, free, nodes)."""
    split = sorted(split_ids)
    free = sorted(free_blocks)
    out = {}
    for r, leaf in enumerate(split):
        out[leaf] = free[r] if r < len(free) else nodes + 8 * (r - len(free))
    take = min(len(split), len(free))
    return out, free[take:], nodes + 8 * (len(split) - take)


_BINOM = [[1 if k == 0 or k == n else 0 for k in range(11)] for n in range(11)]
for _n in range(2, 11):
    for _k in range(1, _n):
        _BINOM[_n][_k] = _BINOM[_n - 1][_k - 1] + _BINOM[_n - 1][_k]


def mask_bucket(m, nb):
    """csrc/vba_kernels_factor.hpp mask_bucket: popcount descending, then the combinatorial rank of the mask among the masks
    with that popcount."""
    m = int(m)
    p = sum((m >> b) & 1 for b in range(nb))
    off = sum(_BINOM[nb][q] for q in range(nb, p, -1))
    r = k = 0
    for b in range(nb):
        if (m >> b) & 1:
            k += 1
            r += _BINOM[b][k]
    return off + r


def store_order(masks, ids, W):
    """Rule 4: store positions of factors with occupancy masks `masks` and node ids `ids` (any order in): the index array that
    sorts them by (bucket, id)."""
    nb = min(W, 10)
    b = np.array([mask_bucket(int(m) & ((1 << nb) - 1), nb) for m in masks], dtype=np.int64)
    return np.lexsort((np.asarray(ids), b))


def _ds_axis(v, voxel_size, dbl):
    loc = ((v if dbl else v.astype(np.float32).astype(np.float64)) / voxel_size).astype(np.float32)
    loc = np.where(loc < 0, (loc.astype(np.float64) - 1.0).astype(np.float32), loc)
    return np.trunc(loc).astype(np.int64)


def down_sampling(pnt, voxel_size, var=None):
    """k_ds_* in deterministic mode: voxels in first-occurrence order, sums added in input order from 0.0, centroid
    (double)(float)(sum * (1.0 / cnt)).  Returns (centroids, vardiag or None, counts, first indices)."""
    dbl = var is not None
    keys = np.stack([_ds_axis(pnt[:, k], voxel_size, dbl) & 0x1FFFFF for k in range(3)], 1)
    _, first, inv, cnt = np.unique(keys, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")           # output row of each unique voxel
    vals = pnt if dbl else pnt.astype(np.float32).astype(np.float64)
    s = np.zeros((len(first), 3))
    np.add.at(s, inv, vals)                              # ufunc.at applies the additions in index order
    scale = 1.0 / cnt.astype(np.float64)
    cen = (s * scale[:, None]).astype(np.float32).astype(np.float64)[order]
    vd = None
    if dbl:
        v = np.zeros((len(first), 3))
        np.add.at(v, inv, var.reshape(-1, 9)[:, [0, 4, 8]])
        vd = (v * scale[:, None]).astype(np.float32).astype(np.float64)[order]
    return cen, vd, cnt[order].astype(np.int32), first[order].astype(np.int32)
