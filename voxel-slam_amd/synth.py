"""Deterministic synthetic workloads for the local-mapping hot path.

Workload synthesis only: scenes, scan patterns, ray casting, ground-truth / perturbed poses and
IMU samples.  Nothing here evaluates the BA; the shipped compute path is the HIP library.

Scenes are axis-aligned rooms (6 walls) plus optional interior rectangular partitions; scans are
ray-cast from the sensor pose with Gaussian range noise along the ray.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List, Tuple

import numpy as np

SEED_BASE = 20241008  # seed = 20241008 + config index


@dataclasses.dataclass
class Workload:
    name: str
    win_size: int
    voxel_size: float
    n_pts: int
    pattern: str            # "spin32" | "avia"
    room: Tuple[float, float, float]   # extents (x, y, z); room spans [-x/2,x/2]x[-y/2,y/2]x[0,z]
    partitions: int
    seed: int
    max_layer: int = 2
    min_eigen_value: float = 0.0025          # config/avia.yaml:32 (LocalBA/min_eigen_value)
    plane_thre: Tuple[float, ...] = (0.25, 0.25, 0.25, 0.25)   # 1/4, stored inverted (VS:930-931)
    min_point: Tuple[float, ...] = (5, 5, 5, 5)                 # VS:917
    max_points: int = 100                     # VM:101
    imu_coef: float = 1e-4                    # VM:500
    range_noise: float = 0.01
    dept_err: float = 0.02                    # config/avia.yaml:27
    beam_err: float = 0.05                    # config/avia.yaml:28


# BASELINE.json configs[0..3]
CONFIGS = {
    "room20k_w4": Workload("room20k_w4", 4, 0.5, 20000, "spin32", (10.0, 8.0, 3.0), 0, SEED_BASE + 0),
    "avia100k_w10": Workload("avia100k_w10", 10, 0.5, 100000, "avia", (40.0, 30.0, 6.0), 6, SEED_BASE + 1),
    "hesai200k_w10": Workload("hesai200k_w10", 10, 0.3, 200000, "spin32", (40.0, 30.0, 6.0), 6, SEED_BASE + 2),
}


def rot_z(yaw: float) -> np.ndarray:
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def so3_exp(w: np.ndarray) -> np.ndarray:
    """Rodrigues; same formula as the reference's Exp (tools.hpp:51-66)."""
    n = float(np.linalg.norm(w))
    if n < 1e-11:
        return np.eye(3)
    a = w / n
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(n) * K + (1 - math.cos(n)) * (K @ K)


def scene_planes(wl: Workload):
    """Returns a list of (axis, coord, lo(3), hi(3)) axis-aligned rectangles."""
    X, Y, Z = wl.room
    x0, x1, y0, y1, z0, z1 = -X / 2, X / 2, -Y / 2, Y / 2, 0.0, Z
    lo = np.array([x0, y0, z0])
    hi = np.array([x1, y1, z1])
    planes = []
    for ax in range(3):
        for c in (lo[ax], hi[ax]):
            planes.append((ax, float(c), lo.copy(), hi.copy()))
    # interior partitions: thin walls parallel to x or y, leaving the sensor corridor free
    part_specs = [
        (0, -X * 0.30, (y0, y0 + Y * 0.55)), (0, X * 0.25, (y1 - Y * 0.55, y1)),
        (1, -Y * 0.28, (x0 + X * 0.10, x0 + X * 0.40)), (1, Y * 0.30, (x1 - X * 0.45, x1 - X * 0.10)),
        (0, X * 0.05, (y0, y0 + Y * 0.35)), (1, Y * 0.12, (x0, x0 + X * 0.22)),
    ]
    for k in range(min(wl.partitions, len(part_specs))):
        ax, c, (a, b) = part_specs[k]
        plo, phi = lo.copy(), hi.copy()
        other = 1 - ax
        plo[other], phi[other] = a, b
        phi[2] = Z * 0.8
        planes.append((ax, float(c), plo, phi))
    return planes


def scan_dirs(wl: Workload, rng: np.random.Generator) -> np.ndarray:
    """Unit ray directions in the body frame, shape (n_pts, 3)."""
    n = wl.n_pts
    if wl.pattern == "spin32":
        n_el = 32
        n_az = n // n_el
        el = np.deg2rad(np.linspace(-16.0, 15.0, n_el))
        az = np.linspace(-math.pi, math.pi, n_az, endpoint=False)
        A, E = np.meshgrid(az, el, indexing="ij")   # azimuth-major like a spinning sensor
        A, E = A.ravel(), E.ravel()
    elif wl.pattern == "avia":
        A = rng.uniform(np.deg2rad(-35.2), np.deg2rad(35.2), n)
        E = rng.uniform(np.deg2rad(-38.6), np.deg2rad(38.6), n)
    else:
        raise ValueError(wl.pattern)
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=1)
    return d


def ray_cast(origin: np.ndarray, dirs_w: np.ndarray, planes) -> np.ndarray:
    """Distance along each world-frame ray to the nearest rectangle (inf if none)."""
    t_best = np.full(dirs_w.shape[0], np.inf)
    eps = 1e-9
    for ax, c, lo, hi in planes:
        dn = dirs_w[:, ax]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (c - origin[ax]) / dn
        ok = np.isfinite(t) & (t > 1e-3)
        t = np.where(ok, t, 0.0)
        hit = origin[None, :] + t[:, None] * dirs_w
        for k in range(3):
            if k != ax:
                ok &= (hit[:, k] >= lo[k] - eps) & (hit[:, k] <= hi[k] + eps)
        t_best = np.where(ok & (t < t_best), t, t_best)
    return t_best


def gt_poses(wl: Workload) -> Tuple[np.ndarray, np.ndarray]:
    """Ground truth: p_i = (-2+0.1 i, 0.05 i, 1.5), yaw = 1 deg * i."""
    W = wl.win_size
    R = np.stack([rot_z(math.radians(1.0) * i) for i in range(W)])
    p = np.stack([np.array([-2.0 + 0.1 * i, 0.05 * i, 1.5]) for i in range(W)])
    if wl.room[0] < 20:   # small room: keep the sensor inside
        p[:, 0] += 2.0
    return R, p


def perturbed_poses(R: np.ndarray, p: np.ndarray, rng: np.random.Generator,
                    rot_sigma_deg: float = 0.3, pos_sigma: float = 0.02) -> Tuple[np.ndarray, np.ndarray]:
    """Initial estimates = GT (+) N(0,(0.3 deg)^2) rot, N(0,(2 cm)^2) trans for i>=1; pose 0 exact (gauge)."""
    R2, p2 = R.copy(), p.copy()
    for i in range(1, R.shape[0]):
        R2[i] = R[i] @ so3_exp(rng.normal(0.0, math.radians(rot_sigma_deg), 3))
        p2[i] = p[i] + rng.normal(0.0, pos_sigma, 3)
    return R2, p2


def make_scans(wl: Workload) -> dict:
    """Returns dict(points=[W arrays (n_i,3) body frame], R_gt, p_gt, R0, p0)."""
    rng = np.random.default_rng(wl.seed)
    planes = scene_planes(wl)
    R_gt, p_gt = gt_poses(wl)
    scans = []
    for i in range(wl.win_size):
        d_b = scan_dirs(wl, rng)
        d_w = d_b @ R_gt[i].T
        t = ray_cast(p_gt[i], d_w, planes)
        ok = np.isfinite(t) & (t > 0.3) & (t < 80.0)
        t = t + rng.normal(0.0, wl.range_noise, t.shape[0])
        pts = d_b[ok] * t[ok, None]
        scans.append(np.ascontiguousarray(pts))
    R0, p0 = perturbed_poses(R_gt, p_gt, rng)
    return dict(points=scans, R_gt=R_gt, p_gt=p_gt, R0=R0, p0=p0)


def poses_flat(R: np.ndarray, p: np.ndarray) -> np.ndarray:
    """[W][12] = R row-major (9) + p (3): the pose layout of include/voxelba.h."""
    W = R.shape[0]
    out = np.empty((W, 12))
    out[:, :9] = R.reshape(W, 9)
    out[:, 9:] = p
    return out


def calc_body_var(pb: np.ndarray, range_inc: float, degree_inc: float) -> np.ndarray:
    """Per-point 3x3 body-frame covariance, the measurement model of calcBodyVar (voxelslam.hpp:180-200),
    vectorised; float32 narrowing of range / range_var as in the reference."""
    pb = pb.copy()
    pb[pb[:, 2] == 0, 2] = 0.0001
    rng_ = np.sqrt((pb * pb).sum(1)).astype(np.float32).astype(np.float64)
    range_var = np.float64(np.float32(range_inc) * np.float32(range_inc))
    dv = math.sin(math.radians(np.float32(degree_inc))) ** 2
    d = pb / np.linalg.norm(pb, axis=1, keepdims=True)
    b1 = np.stack([np.ones(len(d)), np.ones(len(d)), -(d[:, 0] + d[:, 1]) / d[:, 2]], 1)
    b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 = np.cross(b1, d)
    b2 /= np.linalg.norm(b2, axis=1, keepdims=True)
    # A = range * hat(d) @ [b1 b2]
    a1 = rng_[:, None] * np.cross(d, b1)
    a2 = rng_[:, None] * np.cross(d, b2)
    var = range_var * d[:, :, None] * d[:, None, :] + dv * (a1[:, :, None] * a1[:, None, :] + a2[:, :, None] * a2[:, None, :])
    return var


def make_imu(wl: Workload, rate_hz: float = 200.0, scan_dt: float = 0.1, gyr_sigma: float = 0.0, acc_sigma: float = 0.0):
    """IMU samples between consecutive scans for the constant-velocity / constant-yaw-rate GT trajectory.
    Returns list of (t[n], gyr[n,3], acc[n,3]) per interval, velocities v[W,3], gravity g."""
    rng = np.random.default_rng(wl.seed + 77)
    W = wl.win_size
    g = np.array([0.0, 0.0, -9.8])
    yaw_rate = math.radians(1.0) / scan_dt
    vel = np.array([0.1 / scan_dt, 0.05 / scan_dt, 0.0])
    n = int(round(rate_hz * scan_dt)) + 1
    out = []
    for i in range(W - 1):
        t = i * scan_dt + np.arange(n) / rate_hz
        gyr = np.tile(np.array([0.0, 0.0, yaw_rate]), (n, 1)) + rng.normal(0, 1, (n, 3)) * gyr_sigma
        acc = np.empty((n, 3))
        for k in range(n):
            Rk = rot_z(yaw_rate * t[k])
            acc[k] = Rk.T @ (-g)
        acc += rng.normal(0, 1, (n, 3)) * acc_sigma
        out.append((t, gyr, acc))
    v = np.tile(vel, (W, 1))
    return out, v, g


# ----------------------------------------------------------------------------------------------
# Root-voxel factor synthesis (numpy).  Used to produce LidarFactor-shaped inputs for factor-level
# tests before/without the device voxel map: one factor per planar ROOT voxel (no octree levels).

def voxel_key(pw: np.ndarray, voxel_size: float) -> np.ndarray:
    """The reference's key function (voxel_map.hpp:1907-1918): float narrowing, -1 if negative, truncation."""
    loc = (pw / voxel_size).astype(np.float32)
    loc = np.where(loc < 0, loc - np.float32(1.0), loc).astype(np.float32)
    return loc.astype(np.int64)


def pack_clusters(P: np.ndarray, v: np.ndarray, N: np.ndarray) -> np.ndarray:
    out = np.empty(P.shape[:-2] + (10,))
    out[..., 0] = P[..., 0, 0]; out[..., 1] = P[..., 1, 0]; out[..., 2] = P[..., 2, 0]
    out[..., 3] = P[..., 1, 1]; out[..., 4] = P[..., 2, 1]; out[..., 5] = P[..., 2, 2]
    out[..., 6:9] = v
    out[..., 9] = N
    return out


def root_factors(points: List[np.ndarray], R: np.ndarray, p: np.ndarray, wl: Workload, with_keys: bool = False) -> dict:
    W = len(points)
    keys, frames, pw_all, pb_all = [], [], [], []
    for i in range(W):
        pw = points[i] @ R[i].T + p[i]
        keys.append(voxel_key(pw, wl.voxel_size))
        frames.append(np.full(len(pw), i))
        pw_all.append(pw)
        pb_all.append(points[i])
    keys = np.concatenate(keys); frames = np.concatenate(frames)
    pw_all = np.concatenate(pw_all); pb_all = np.concatenate(pb_all)
    ukeys, vid = np.unique(keys, axis=0, return_inverse=True)
    vid = vid.ravel()
    V = int(vid.max()) + 1
    Pw = np.zeros((V, 3, 3)); vw = np.zeros((V, 3)); Nw = np.zeros(V)
    np.add.at(Pw, vid, pw_all[:, :, None] * pw_all[:, None, :])
    np.add.at(vw, vid, pw_all)
    np.add.at(Nw, vid, 1.0)
    Pb = np.zeros((V, W, 3, 3)); vb = np.zeros((V, W, 3)); Nb = np.zeros((V, W))
    np.add.at(Pb, (vid, frames), pb_all[:, :, None] * pb_all[:, None, :])
    np.add.at(vb, (vid, frames), pb_all)
    np.add.at(Nb, (vid, frames), 1.0)
    ok = Nw > wl.min_point[0]
    c = vw / np.maximum(Nw, 1)[:, None]
    cov = Pw / np.maximum(Nw, 1)[:, None, None] - c[:, :, None] * c[:, None, :]
    lam, U = np.linalg.eigh(cov)
    with np.errstate(divide="ignore", invalid="ignore"):
        plane = ok & (lam[:, 0] < wl.min_eigen_value) & (lam[:, 0] / lam[:, 2] < wl.plane_thre[0]) & (lam[:, 0] / lam[:, 1] <= 0.12)
    sel = np.nonzero(plane)[0]
    out = dict(
        clusters=np.ascontiguousarray(pack_clusters(Pb[sel], vb[sel], Nb[sel])),      # [V][W][10]
        fix=np.zeros((len(sel), 10)),
        coe=np.ones(len(sel)),
        eig_val=np.ascontiguousarray(lam[sel]),
        eig_vec=np.ascontiguousarray(U[sel].reshape(len(sel), 9)),                    # row-major, columns = eigenvectors
        pcr_add=np.ascontiguousarray(pack_clusters(Pw[sel], vw[sel], Nw[sel])),
    )
    if with_keys:
        out["keys"] = np.ascontiguousarray(ukeys[sel])
    return out


# ----------------------------------------------------------------------------------------------
# Initialisation window (vba_motion_init, voxelslam.cpp:617-819): raw lidar-frame clouds whose points carry their own capture time
# (PointType::curvature, ascending), distorted by the moving ground truth; per-scan IMU deques; perturbed states with a tilted,
# mis-scaled gravity.

def corridor_planes(length: float = 40.0, width: float = 3.0, height: float = 3.0):
    """Floor, ceiling and two parallel walls along x, open ends: every normal is perpendicular to x (degenerate along x)."""
    lo = np.array([-length / 2, -width / 2, 0.0])
    hi = np.array([length / 2, width / 2, height])
    return [(ax, float(c), lo.copy(), hi.copy()) for ax in (1, 2) for c in (lo[ax], hi[ax])]


def _ray_cast_many(org: np.ndarray, dirs_w: np.ndarray, planes) -> np.ndarray:
    """ray_cast with one origin per ray."""
    t_best = np.full(dirs_w.shape[0], np.inf)
    for ax, c, lo, hi in planes:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (c - org[:, ax]) / dirs_w[:, ax]
        ok = np.isfinite(t) & (t > 1e-3)
        t = np.where(ok, t, 0.0)
        hit = org + t[:, None] * dirs_w
        for k in range(3):
            if k != ax:
                ok &= (hit[:, k] >= lo[k] - 1e-9) & (hit[:, k] <= hi[k] + 1e-9)
        t_best = np.where(ok & (t < t_best), t, t_best)
    return t_best


def make_init_window(win_size: int = 10, n_pts: int = 20000, scene: str = "room", seed: int = SEED_BASE + 40,
                     lead: Tuple[int, ...] = (3, -2), imu_rate: float = 200.0, scan_dt: float = 0.1, g_tilt_deg: float = 2.0,
                     g_scale: float = 0.98, acc_unit_g: bool = True, ext_t: Tuple[float, float, float] = (0.04, 0.0, 0.03),
                     range_noise: float = 0.005, yaw_rate: float = 0.3, pitch_amp: float = 0.05) -> dict:
    """Returns dict(clouds, curvs, imus, beg_times, states, covs, ext, scale_gravity, gt_states).

    State i sits at T_i = scan_dt * (i + 1); deque i holds the IMU samples of [T_{i-1}, T_i] (deque 0: [T_0 - scan_dt, T_0]), so the
    pre-integration between states is consistent.  Scan i starts at beg_i = T_{i-1} + lead[i % len(lead)] / imu_rate and ends at T_i:
    a positive lead puts IMU samples before beg_time (point 0 is pushed again for every older pose), a negative one starts the deque
    after it (the points before the oldest pose are dropped)."""
    rng = np.random.default_rng(seed)
    if scene == "room":
        planes = scene_planes(Workload("init_room", win_size, 0.5, n_pts, "spin32", (10.0, 8.0, 3.0), 2, seed))
    elif scene == "corridor":
        planes = corridor_planes()
    else:
        raise ValueError(scene)
    G = 9.81
    g_w = np.array([0.0, 0.0, -G])
    vel = np.array([0.6, 0.25, 0.0])
    p_start = np.array([-1.0, -0.3, 1.4])

    def pose(t):   # yaw ramp + small pitch oscillation (the accelerometer then sees gravity from changing directions)
        R = rot_z(yaw_rate * t) @ so3_exp(np.array([0.0, pitch_amp * math.sin(2.0 * math.pi * t), 0.0]))
        return R, p_start + vel * t

    def ang_vel_body(t, h=1e-5):
        R0, _ = pose(t - h); R1, _ = pose(t + h)
        S = R0.T @ R1
        w = np.array([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]]) * 0.5
        return w / (2 * h)

    def acc_body(t):
        R, _ = pose(t)
        return R.T @ (np.zeros(3) - g_w)     # constant velocity: specific force = -g

    R_ext = np.eye(3)
    t_ext = np.array(ext_t)
    ext = np.concatenate([R_ext.ravel(), t_ext])
    imu_dt = 1.0 / imu_rate
    per = int(round(scan_dt * imu_rate))
    T = scan_dt * (np.arange(win_size) + 1)
    clouds, curvs, imus, begs = [], [], [], []
    for i in range(win_size):
        t_prev = T[i] - scan_dt
        ts = t_prev + np.arange(per + 1) * imu_dt
        gyr = np.stack([ang_vel_body(t) for t in ts])
        acc = np.stack([acc_body(t) for t in ts]) / (G if acc_unit_g else 1.0)
        imus.append(np.column_stack([ts, gyr, acc]))
        beg = t_prev + lead[i % len(lead)] * imu_dt
        begs.append(beg)
        span = T[i] - beg
        cv = np.sort(rng.uniform(0.0, span, n_pts).astype(np.float32)).astype(np.float64)
        az = rng.uniform(-math.pi, math.pi, n_pts)
        el = rng.uniform(math.radians(-30.0), math.radians(30.0), n_pts)
        dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
        Rs, ps = zip(*[pose(beg + c) for c in cv])       # each point from the lidar pose at its own time
        Rs, ps = np.stack(Rs), np.stack(ps)
        org = np.einsum("nij,j->ni", Rs, t_ext) + ps
        d_w = np.einsum("nij,nj->ni", Rs, dirs @ R_ext.T)
        tt = _ray_cast_many(org, d_w, planes)
        ok = np.isfinite(tt) & (tt > 0.3) & (tt < 80.0)
        pts = dirs * (tt + rng.normal(0.0, range_noise, n_pts))[:, None]
        clouds.append(pts[ok].astype(np.float32).astype(np.float64))
        curvs.append(cv[ok])
        begs[-1] = beg
    gt = np.zeros((win_size, 25))
    for i in range(win_size):
        R, p = pose(T[i])
        gt[i, 0] = T[i]; gt[i, 1:10] = R.ravel(); gt[i, 10:13] = p; gt[i, 13:16] = vel; gt[i, 22:25] = g_w
    states = gt.copy()
    tilt = so3_exp(np.array([math.radians(g_tilt_deg), -math.radians(g_tilt_deg) * 0.5, 0.0]))
    for i in range(win_size):
        if i > 0:
            states[i, 1:10] = (gt[i, 1:10].reshape(3, 3) @ so3_exp(rng.normal(0.0, math.radians(0.2), 3))).ravel()
            states[i, 10:13] = gt[i, 10:13] + rng.normal(0.0, 0.01, 3)
        states[i, 13:16] = vel + rng.normal(0.0, 0.05, 3)
        states[i, 22:25] = g_scale * (tilt @ g_w)
    covs = np.zeros((win_size, 15, 15))
    for i in range(win_size):
        covs[i] = np.diag([1e-5] * 3 + [1e-4] * 3 + [1e-3] * 3 + [1e-6] * 6)
    return dict(clouds=clouds, curvs=curvs, imus=imus, beg_times=np.array(begs), states=states, covs=covs.reshape(win_size, 225),
                ext=ext, scale_gravity=G if acc_unit_g else 1.0, gt_states=gt)


# ------------------------------------------------------------------------------------------------ loop retrieval (vba_btc_*)
def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def make_btc_sessions(n_sessions=2, n_kf=200, n_keypoints=900, max_desc=120, n_planes=60, plane_pts=4, view=30.0, seed=0,
                      loc_noise=0.01, flip_bits=2, occupy_len=50, std_side_resolution=0.2, min_len=2.0, max_len=50.0):
    """Sessions as the loop-closure thread sees them (VS:2404-2541), deterministic in `seed`.

    World: corner keypoints with a `occupy_len`-bit occupancy pattern each; planar voxels (centre, normal).  Each session drives a
    closed circuit around the same area (session k starts 2 pi k / n_sessions further on and turns once round), so it revisits its
    own start and the places of the other sessions.  Per keyframe: triangles of visible keypoints (a fixed global list, so a
    revisit regenerates the same triangles), as descriptor rows of include/voxelba.h (sides sorted and scaled by
    1 / std_side_resolution, A / B / C = the vertices opposite the shortest / middle / longest side, centre = centroid,
    frame_number = keyframe index in the session), with `flip_bits` occupancy bits flipped per observation; the plane cloud =
    visible planar voxels in the keyframe frame (float32 x y z nx ny nz).  Returns a list of sessions, each a dict of lists:
    rows, bits, cloud, R, p (keyframe pose in the world)."""
    rng = np.random.default_rng(seed)
    kp = np.column_stack([rng.uniform(-60, 60, n_keypoints), rng.uniform(-60, 60, n_keypoints), rng.uniform(0, 8, n_keypoints)])
    pat = rng.integers(0, 2, size=(n_keypoints, occupy_len)).astype(np.uint64)
    # global triangle list: each keypoint with pairs of its 6 nearest neighbours, sides within [min_len, max_len]
    d2 = ((kp[:, None, :] - kp[None, :, :]) ** 2).sum(-1)
    nn = np.argsort(d2, axis=1)[:, 1:7]
    tris = set()
    for a in range(n_keypoints):
        for u in range(6):
            for v in range(u + 1, 6):
                t = tuple(sorted((a, int(nn[a, u]), int(nn[a, v]))))
                if len(set(t)) == 3:
                    tris.add(t)
    tris = np.array(sorted(tris), dtype=np.int64)
    L = lambda i, j: np.linalg.norm(kp[tris[:, i]] - kp[tris[:, j]], axis=1)
    sides = np.stack([L(1, 2), L(0, 2), L(0, 1)], axis=1)          # side opposite vertex 0, 1, 2
    keep = (sides.min(1) >= min_len) & (sides.max(1) <= max_len) & (np.abs(np.diff(np.sort(sides, 1), axis=1)).min(1) > 0.3)
    tris, sides = tris[keep], sides[keep]
    order = np.argsort(sides, axis=1)                               # A, B, C = opposite the shortest, middle, longest side
    tris = np.take_along_axis(tris, order, axis=1)
    sides = np.take_along_axis(sides, order, axis=1)
    # planar voxels: centres on the ground and on vertical walls, unit normals
    pc = np.column_stack([rng.uniform(-60, 60, n_planes * 8), rng.uniform(-60, 60, n_planes * 8), np.zeros(n_planes * 8)])
    pn = np.tile([0.0, 0.0, 1.0], (n_planes * 8, 1))
    wall_a = rng.uniform(0, np.pi, n_planes)
    wc = np.column_stack([rng.uniform(-60, 60, n_planes), rng.uniform(-60, 60, n_planes), rng.uniform(1, 6, n_planes)])
    wn = np.column_stack([np.cos(wall_a), np.sin(wall_a), np.zeros(n_planes)])
    off = rng.uniform(-3, 3, (n_planes, plane_pts * 4))
    wpts = (wc[:, None, :] + off[..., None] * np.stack([-wn[:, 1], wn[:, 0], np.zeros(n_planes)], 1)[:, None, :]).reshape(-1, 3)
    wpts[:, 2] += rng.uniform(-2, 2, len(wpts))
    pc = np.concatenate([pc, wpts]); pn = np.concatenate([pn, np.repeat(wn, plane_pts * 4, axis=0)])
    sessions = []
    for s in range(n_sessions):
        out = dict(rows=[], bits=[], cloud=[], R=[], p=[])
        ph0 = 2 * np.pi * s / max(n_sessions, 1)
        for k in range(n_kf):
            ph = ph0 + 2 * np.pi * 1.25 * k / n_kf                   # 1.25 turns: the last quarter revisits the start
            pos = np.array([35 * np.cos(ph), 35 * np.sin(ph), 1.5])
            R = _rot_z(ph + np.pi / 2 + 0.05 * np.sin(3 * ph))
            vis = np.linalg.norm(kp[:, :2] - pos[:2], axis=1) < view
            tv = np.flatnonzero(vis[tris].all(1))[:max_desc]
            local = (kp - pos) @ R + rng.normal(0, loc_noise, kp.shape)
            rows = np.zeros((len(tv), 19))
            bits = np.zeros((len(tv), 3), dtype=np.uint64)
            for m, ti in enumerate(tv):
                vtx = tris[ti]
                rows[m, 0:3] = sides[ti] / std_side_resolution
                rows[m, 3:6] = local[vtx].mean(0)
                rows[m, 6] = k
                rows[m, 7:16] = local[vtx].reshape(-1)
                for e in range(3):
                    b = pat[vtx[e]].copy()
                    fl = rng.integers(0, occupy_len, flip_bits)
                    b[fl] ^= np.uint64(1)
                    rows[m, 16 + e] = float(b.sum())
                    bits[m, e] = np.bitwise_or.reduce(b << np.arange(occupy_len, dtype=np.uint64))
            pv = np.linalg.norm(pc[:, :2] - pos[:2], axis=1) < view
            cl = np.zeros((int(pv.sum()), 6), dtype=np.float32)
            cl[:, 0:3] = (pc[pv] - pos) @ R + rng.normal(0, 0.01, (int(pv.sum()), 3))
            cl[:, 3:6] = pn[pv] @ R
            out["rows"].append(rows); out["bits"].append(bits); out["cloud"].append(cl); out["R"].append(R); out["p"].append(pos)
        sessions.append(out)
    return sessions


def btc_plane_cloud(n, seed=0):
    """a float32 plane cloud of n points on five planes (x y z nx ny nz) for the ICP tests"""
    rng = np.random.default_rng(seed)
    normals = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [0.6, 0.8, 0], [0, 0.6, 0.8]], dtype=np.float64)
    ds = np.array([0.0, 8.0, -6.0, 4.0, 3.0])
    k = rng.integers(0, 5, n)
    nrm = normals[k]
    u = np.cross(nrm, [0.3, 0.5, 0.81]); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(nrm, u)
    a, b = rng.uniform(-10, 10, (2, n))
    pts = nrm * ds[k][:, None] + a[:, None] * u + b[:, None] * v + rng.normal(0, 0.005, (n, 3))
    return np.column_stack([pts, nrm]).astype(np.float32)


def _btc_world(rng, extent=70.0, n_boxes=40, n_poles=60, density=40.0):
    """surface points of a keyframe world: ground, a perimeter wall, boxes and poles of varied heights (world frame, float64)"""
    parts = []
    def rect(o, u, v, lu, lv):                       # points on the rectangle o + s u + t v, s in [0, lu], t in [0, lv]
        k = max(int(lu * lv * density), 8)
        s = rng.uniform(0, lu, k); t = rng.uniform(0, lv, k)
        return o + s[:, None] * u + t[:, None] * v
    ex, ey, ez = np.eye(3)
    parts.append(rect(np.array([-extent, -extent, 0.0]), ex, ey, 2 * extent, 2 * extent) * [1, 1, 0])
    for o, u in (((-extent, -extent), ex), ((-extent, extent), ex), ((-extent, -extent), ey), ((extent, -extent), ey)):
        parts.append(rect(np.array([o[0], o[1], 0.0]), u, ez, 2 * extent, 4.0))
    for _ in range(n_boxes):
        c = rng.uniform(-extent + 8, extent - 8, 2); w, d, h = rng.uniform(2, 7), rng.uniform(2, 7), rng.uniform(1.5, 9)
        yaw = rng.uniform(0, np.pi); R = _rot_z(yaw); a, b = R[:, 0], R[:, 1]
        o = np.array([c[0], c[1], 0.0]) - 0.5 * w * a - 0.5 * d * b
        parts += [rect(o, a, ez, w, h), rect(o + d * b, a, ez, w, h), rect(o, b, ez, d, h), rect(o + w * a, b, ez, d, h),
                  rect(o + h * ez, a, b, w, d)]
    for _ in range(n_poles):
        c = rng.uniform(-extent + 5, extent - 5, 2); r, h = rng.uniform(0.1, 0.3), rng.uniform(2, 8)
        k = int(2 * np.pi * r * h * density * 4) + 16
        th = rng.uniform(0, 2 * np.pi, k); z = rng.uniform(0, h, k)
        parts.append(np.column_stack([c[0] + r * np.cos(th), c[1] + r * np.sin(th), z]))
    return np.concatenate(parts)


def make_btc_keyframe_sessions(n_sessions=2, n_kf=20, n_points=200000, radius=20.0, view=45.0, noise=0.02, seed=0, extent=70.0):
    """Keyframe point clouds for descriptor generation (GenerateSTDescs input), deterministic in `seed`.

    World: ground, a perimeter wall, boxes and poles of varied heights (_btc_world).  Each session drives the same closed circuit
    of radius `radius` (session k starts 2 pi k / n_sessions further on and runs once round, so keyframes of different sessions
    revisit the same places); per keyframe: `n_points` world points within `view` metres (sampled with replacement), moved into
    the keyframe frame (p_k = R^T (p_w - t)) with Gaussian noise `noise`, as float32 [n_points][3].  The world spans
    [-extent, extent]^2, with boxes and poles in proportion to its area.  Returns a list of sessions, each a dict with lists
    cloud, R, t (the ground-truth keyframe poses in the world)."""
    rng = np.random.default_rng(seed)
    a = (extent / 70.0) ** 2
    world = _btc_world(rng, extent=extent, n_boxes=int(round(40 * a)), n_poles=int(round(60 * a)))
    out = []
    for s in range(n_sessions):
        ses = dict(cloud=[], R=[], t=[])
        for k in range(n_kf):
            a = 2 * np.pi * (s / n_sessions + k / n_kf)
            t = np.array([radius * np.cos(a), radius * np.sin(a), 1.5])
            R = _rot_z(a + np.pi / 2 + rng.normal(0, 0.05))
            t = t + np.append(rng.normal(0, 0.3, 2), 0.0)
            near = np.flatnonzero(np.sum((world[:, :2] - t[:2]) ** 2, axis=1) < view * view)
            pick = world[rng.choice(near, n_points, replace=len(near) < n_points)]
            loc = (pick - t) @ R + rng.normal(0, noise, (n_points, 3))
            ses["cloud"].append(loc.astype(np.float32)); ses["R"].append(R); ses["t"].append(t)
        out.append(ses)
    return out


def make_keyframe_path(n_kf=30, scans_per_kf=10, n_pts=20000, scan_step=None, seed=SEED_BASE + 60, with_var=True):
    """Keyframe windows for the keyframe store (vba_kf_*): n_kf * scans_per_kf spinning-sensor scans of the partitioned 40 x 30 x 6
    hall on a curved trajectory (an ellipse of 6 m x 4 m around the hall's centre with a little roll, pitch and height change;
    scan_step = the angle between scans, default: 300 degrees over the whole path).  Returns a list of keyframes, each a dict of
    points = [k arrays (n_i, 3), body frame], vars = [k arrays (n_i, 9)] from calc_body_var (None without with_var) and
    poses [k][12]."""
    wl = dataclasses.replace(CONFIGS["hesai200k_w10"], name="kf_path", n_pts=n_pts, win_size=scans_per_kf, seed=seed)
    rng = np.random.default_rng(seed)
    planes = scene_planes(wl)
    total = n_kf * scans_per_kf
    if scan_step is None:
        scan_step = math.radians(300.0) / max(total - 1, 1)
    out = []
    for k in range(n_kf):
        pts_k, var_k, poses = [], [], np.empty((scans_per_kf, 12))
        for i in range(scans_per_kf):
            a = scan_step * (k * scans_per_kf + i)
            p = np.array([6.0 * math.cos(a), 4.0 * math.sin(a), 1.5 + 0.2 * math.sin(3.0 * a)])
            R = rot_z(a + math.pi / 2) @ so3_exp(np.array([0.03 * math.sin(2.0 * a), 0.02 * math.cos(3.0 * a), 0.0]))
            d_b = scan_dirs(wl, rng)
            t = ray_cast(p, d_b @ R.T, planes)
            ok = np.isfinite(t) & (t > 0.3) & (t < 80.0)
            t = t + rng.normal(0.0, wl.range_noise, t.shape[0])
            pts = np.ascontiguousarray(d_b[ok] * t[ok, None])
            pts_k.append(pts)
            if with_var:
                var_k.append(np.ascontiguousarray(calc_body_var(pts, wl.dept_err, wl.beam_err).reshape(-1, 9)))
            poses[i, :9] = R.ravel(); poses[i, 9:] = p
        out.append(dict(points=pts_k, vars=var_k if with_var else None, poses=poses))
    return out
