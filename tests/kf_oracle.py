"""numpy restatement of the keyframe store for the tests of vba_kf_*: the merge of K clouds into the frame of the last one's pose
(voxelslam.cpp:2354-2371, 348-372, 384-398), the float narrowing of the merged cloud (VS:2390-2397), the voxel key of the two
down-samplers (voxel_map.hpp:45-51, tools.hpp:210-217), the keyframe -> world transform of keyframe_loading (VS:1418-1427), the
history bookkeeping (VS:2628-2647) and the nearby selection (VS:1379-1438).  TEST INFRASTRUCTURE only.

The order of operations is the one include/voxelba.h states.  numpy's elementwise operations round every product and sum on
its own (nothing is fused), which is what that contract needs.  Poses are flat [R(9) row-major, p(3)].
"""
import numpy as np


def delta(xc, x):
    """(dR, dp) of a cloud at pose x into the frame of pose xc: dR = xc.R^T x.R, dp = xc.R^T (x.p - xc.p)."""
    xc = np.asarray(xc, dtype=np.float64); x = np.asarray(x, dtype=np.float64)
    A = xc[:9].reshape(3, 3); B = x[:9].reshape(3, 3)
    dR = (A[0][:, None] * B[0][None, :] + A[1][:, None] * B[1][None, :]) + A[2][:, None] * B[2][None, :]
    d = x[9:12] - xc[9:12]
    dp = (A[0] * d[0] + A[1] * d[1]) + A[2] * d[2]
    return dR, dp


def apply(dR, dp, pts):
    """q[r] = ((dR[r][0] x + dR[r][1] y) + dR[r][2] z) + dp[r] per point"""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((dR[r, 0] * x + dR[r, 1] * y) + dR[r, 2] * z) + dp[r] for r in range(3)], axis=1)


def merge(clouds, poses):
    """clouds i = 0..k-1 concatenated in the frame of poses[k-1], in doubles"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    assert len(clouds) == len(poses) and len(clouds) >= 1
    out = [apply(*delta(poses[-1], poses[i]), clouds[i]) for i in range(len(clouds))]
    return np.concatenate(out) if out else np.zeros((0, 3))


def merge_float(clouds, poses):
    """the cloud handed to GenerateSTDescs: PointXYZI x, y, z = the merged doubles narrowed to float"""
    return merge(clouds, poses).astype(np.float32)


def world(x0, pts):
    """keyframe_loading: world = x0.R p + x0.p in the same operation order"""
    x0 = np.asarray(x0, dtype=np.float64)
    return apply(x0[:9].reshape(3, 3), x0[9:12], pts)


def voxel_keys(pts, voxel_size, pvec):
    """int64 [n][3]: loc = (float)(p / voxel_size), loc -= 1 below zero (in float), truncated.  pvec: the coordinate is the double
    (voxel_map.hpp:45-51); otherwise it is first narrowed to float, the PCL point of tools.hpp:210-217."""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    if not pvec:
        p = p.astype(np.float32).astype(np.float64)
    loc = (p / float(voxel_size)).astype(np.float32)
    loc = np.where(loc < 0, (loc.astype(np.float64) - 1.0).astype(np.float32), loc)
    return loc.astype(np.int64)


def voxel_groups(pts, voxel_size, pvec):
    """(first index of every voxel in first-occurrence order, counts in that order, voxel index of every point)"""
    keys = voxel_keys(pts, voxel_size, pvec)
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, inv, cnt = np.unique(keys, axis=0, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64); rank[order] = np.arange(len(order))
    return first[order], cnt[order], rank[np.ravel(inv)]


class History:
    """exist flags, pl_kdmap and history_kfsize of one session (VS:2628-2647, VS:1379-1438)"""

    def __init__(self, positions):
        self.p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)      # x0.p of every keyframe
        self.exist = np.zeros(len(self.p), dtype=np.int64)
        self.size = 0
        self.snap = np.zeros((0, 3), np.float32)

    def set_history(self, n):
        self.exist[:] = 0
        self.exist[:n] = 1
        self.snap = self.p[:n].astype(np.float32)
        self.size = n

    def candidates(self, p3, radius):
        """(indices inside the sphere, nearest first, lower index on a tie; their float squared distances)"""
        q = np.asarray(p3, dtype=np.float64).astype(np.float32)
        d2 = np.zeros(len(self.snap), np.float32)
        for j in range(3):
            t = self.snap[:, j] - q[j]
            d2 = d2 + t * t
        idx = np.nonzero(d2 < np.float32(float(radius) * float(radius)))[0]
        idx = idx[np.lexsort((idx, d2[idx]))]
        return idx, d2[idx]

    def load_nearby(self, p3, radius):
        """index of the keyframe keyframe_loading loads around p3, -1 = none"""
        if self.size <= 0:
            return -1
        for i in self.candidates(p3, radius)[0]:
            if self.exist[i]:
                self.exist[i] = 0
                self.size -= 1
                return int(i)
        return -1
