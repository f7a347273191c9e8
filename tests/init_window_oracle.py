"""numpy restatement of the pl_origs half of initialization() (voxelslam.cpp:1499-1511): what one scan contributes to the window.

    pl_down = orig; down_sampling_close(pl_down, down_size)
    if pl_down.size() < 1000: pl_down = orig; down_sampling_close(pl_down, down_size / 2)
    sort(pl_down, curvature <)

``orig`` is the decoded cloud, already sorted by curvature with a STABLE sort (the contract of vba_scan_decode), so the cloud the
reference's sort leaves, with ties resolved the same way (message order), is the kept subset in ascending index order: ``push``
returns those indices.  ``close(points, voxel_size)`` is any down_sampling_close that returns the kept indices (the C++ oracle's, or
the device's), in whatever order."""
import numpy as np


def push(points, curv, down_size, min_points, close):
    """Returns (indices ascending, retried).  points [n][3], curv [n] ascending."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(points)
    assert len(np.ravel(curv)) == n

    def keep(vs):
        if vs < 0.001:                                   # tools.hpp:242: the cloud is left as it is
            return np.arange(n, dtype=np.int64)
        return np.asarray(close(points, vs), dtype=np.int64)

    idx = keep(down_size)
    retried = False
    if min_points > 0 and len(idx) < min_points:         # VS:1503, strict
        idx = keep(down_size / 2)                        # from the full cloud, kept whatever its count
        retried = True
    return np.sort(idx), retried


def sorted_by_curvature(idx, curv):
    """The reference's own order: the kept indices (in the order down_sampling_close emits them) sorted by curvature, ties resolved in
    message order (a stable sort of the index-ordered subset)."""
    idx = np.sort(np.asarray(idx, dtype=np.int64))
    return idx[np.argsort(np.asarray(curv)[idx], kind="stable")]


def grid_cloud(n_voxels, per_voxel=3, voxel=0.5):
    """n_voxels voxels in a row along x, per_voxel distinct points inside each (no point on a voxel face): down_sampling_close at
    `voxel` keeps exactly n_voxels points, at voxel / 2 it keeps more.  float32 values; curvature ascending."""
    k = np.arange(n_voxels, dtype=np.float64)
    frac = 0.1 + 0.8 * (np.arange(per_voxel) + 0.5) / per_voxel        # spread over both halves of the voxel
    x = (k[:, None] + frac[None, :]) * voxel
    pts = np.stack([x.ravel(), np.full(x.size, 0.1 * voxel), np.full(x.size, 0.1 * voxel)], axis=1).astype(np.float32).astype(np.float64)
    curv = (np.arange(len(pts)) * (0.1 / len(pts))).astype(np.float32).astype(np.float64)
    return pts, curv
