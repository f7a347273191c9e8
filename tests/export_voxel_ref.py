"""Plain numpy restatement of vba_kf_voxel_export (include/voxelba.h): the sequence S of export_oracle.points,
the voxel of kf_oracle.voxel_groups on the float coordinates, the sums as chains in sequence order, the min_count filter.  TEST
INFRASTRUCTURE only.

A session is (clouds, poses, intensity): the kept clouds of its keyframes, their x0, the float of its store."""
import numpy as np

import export_oracle as eo
import kf_oracle as ko


def sequence(sessions, jump):
    """S, float32 [n][4]: the records vba_kf_export_world writes for the stores in order, and the keyframe (counted over all
    sessions) of every record"""
    recs, kf, k = [], [], 0
    for clouds, poses, intensity in sessions:
        for c, x in zip(clouds, poses):
            r = eo.points([c], [x], [intensity], jump)
            recs.append(r); kf.append(np.full(len(r), k, np.int64)); k += 1
    if not recs:
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
    return np.concatenate(recs), np.concatenate(kf)


def centroids(S, voxel_size):
    """(first, cnt, vox, xyz float32, f64 sums): one row per voxel in first-occurrence order.  np.add.at adds unbuffered, one
    index after the other, so each sum is the chain ((0 + a_0) + a_1) + ... in the order of S."""
    first, cnt, vox = ko.voxel_groups(S[:, :3], voxel_size, pvec=False)
    sums = np.zeros((len(first), 3))
    np.add.at(sums, vox, S[:, :3].astype(np.float64))
    inv = 1.0 / cnt.astype(np.float64)
    return first, cnt, vox, (sums * inv[:, None]).astype(np.float32), sums


def export_voxel(sessions, jump, voxel_size, min_count=1):
    """(xyzi float32 [m][4], counts int32 [m], first int64 [m]) of the kept voxels"""
    S, _ = sequence(sessions, jump)
    first, cnt, _, xyz, _ = centroids(S, voxel_size)
    keep = cnt >= min_count
    xyzi = np.concatenate([xyz, S[first, 3:4]], axis=1)[keep] if len(first) else np.zeros((0, 4), np.float32)
    return np.ascontiguousarray(xyzi, dtype=np.float32), cnt[keep].astype(np.int32), first[keep]


def voxel_census(sessions, jump, voxel_size):
    """(voxels, voxels of more than one record, voxels whose records come from more than one keyframe, the largest count)"""
    S, kf = sequence(sessions, jump)
    first, cnt, vox, _, _ = centroids(S, voxel_size)
    lo = np.full(len(first), np.iinfo(np.int64).max); hi = np.full(len(first), -1)
    np.minimum.at(lo, vox, kf); np.maximum.at(hi, vox, kf)
    return len(first), int((cnt > 1).sum()), int((hi > lo).sum()), int(cnt.max())


def message_ends(n, interval_size):
    """vba::voxel_message_ends: full messages while more than interval_size records remain, then the final one"""
    ends, b = [], 0
    while n - b > interval_size:
        b += interval_size
        ends.append(b)
    return ends + [n]


# ---- the stores of the tests: the edge store of tests/test_gpu_export.py (sizes, lattice, rotations), with its translations of
# +-40 m and with translations within +-2 m, where the keyframes overlap
EDGE_SIZES = [0, 1, 2, 3, 255, 256, 257, 1000]


def edge_poses(n, seed, spread):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):                                        # the draws of test_gpu_export._poses, the translation rescaled
        R = Rotation.from_rotvec(rng.uniform(-1.2, 1.2, 3)).as_matrix().ravel()
        out.append(np.concatenate([R, rng.uniform(-40, 40, 3) * (spread / 40.0)]))
    return np.stack(out)


def lattice(n, seed):
    rng = np.random.default_rng(seed)
    idx = rng.permutation(16 ** 3)[:n]
    return np.stack([idx % 16, (idx // 16) % 16, idx // 256], axis=1).astype(np.float64) - 7.75


def edge_clouds(seed=5):
    return [lattice(n, seed + 100 + k) for k, n in enumerate(EDGE_SIZES)]


def boundary_grid():
    """2500 points: x, y in {-3, -2.75, ..., 3}, z in {-1, -0.0, 0, 0.5}; every coordinate is a float"""
    a = np.arange(-12, 13) * 0.25
    z = np.array([-1.0, -0.0, 0.0, 0.5])
    g = np.stack(np.meshgrid(a, a, z, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g)


IDENTITY = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
