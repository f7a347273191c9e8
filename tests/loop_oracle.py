"""numpy restatement of the host-visible arithmetic of the loop-closure map rebuild (vba_loop_map_build / vba_loop_update, DESIGN.md
section 14): the expansion table of VS:2601-2625, the world transform and the dx algebra of VS:2597-2598 / LR:29-34 / VS:1296-1331.
Every product and sum is formed elementwise, one numpy operation each, so nothing fuses: the values are the ones a baseline x86-64
build of the reference computes.  tests/host/loop_host.cpp adds the fixed insertion with covariances to the CPU oracle."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)


def expansion(size, init_num=5, cumulative=True):
    """VS:2601-2625: the keyframe indices of every cut_voxel call, in call order.  Call j holds keyframes first .. first + j
    (pvec_tem is never cleared); the corrected form holds keyframe first + j alone.  Indices below zero are skipped (VS:2607-2608)."""
    calls, tem = [], []
    for i in range(size - init_num, size):
        if i < 0:
            continue
        if not cumulative:
            tem = []
        tem = tem + [i]
        calls.append(list(tem))
    return calls


def expansion_counts(size, init_num=5, cumulative=True):
    """how often each keyframe of the store is inserted"""
    cnt = np.zeros(size, dtype=np.int64)
    for call in expansion(size, init_num, cumulative):
        for i in call:
            cnt[i] += 1
    return cnt


def world(pose12, pts):
    """pw = R p + t as ((R0 x + R1 y) + R2 z) + t, every operation rounded on its own"""
    pose12 = np.asarray(pose12, dtype=np.float64); pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    R = pose12[:9].reshape(3, 3); t = pose12[9:]
    out = np.empty_like(pts)
    for r in range(3):
        a = R[r, 0] * pts[:, 0]
        b = R[r, 1] * pts[:, 1]
        a = a + b
        b = R[r, 2] * pts[:, 2]
        a = a + b
        out[:, r] = a + t[r]
    return out


def diag_var(vd):
    """float [n][3] covariance diagonals -> double [n][9] (VS:2614-2621: var.setZero(); var(j, j) = normal[j])"""
    vd = np.asarray(vd)
    out = np.zeros((len(vd), 9))
    out[:, 0] = vd[:, 0].astype(np.float64); out[:, 4] = vd[:, 1].astype(np.float64); out[:, 8] = vd[:, 2].astype(np.float64)
    return out


def _mm(A, B):
    """3x3 product, s = a0 b0; s += a1 b1; s += a2 b2"""
    A = np.asarray(A, dtype=np.float64).reshape(3, 3); B = np.asarray(B, dtype=np.float64).reshape(3, 3)
    out = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            s = A[r, 0] * B[0, c]
            s = s + A[r, 1] * B[1, c]
            s = s + A[r, 2] * B[2, c]
            out[r, c] = s
    return out


def _mv(A, v):
    A = np.asarray(A, dtype=np.float64).reshape(3, 3); v = np.asarray(v, dtype=np.float64)
    out = np.empty(3)
    for r in range(3):
        s = A[r, 0] * v[0]
        s = s + A[r, 1] * v[1]
        s = s + A[r, 2] * v[2]
        out[r] = s
    return out


def loop_dx(x1, x3):
    """VS:2597-2598 on states [t, R(9), p(3), ...]: dx.R = x3.R x1.R^T; dx.p = x3.p - (x3.R x1.R^T) x1.p  -> pose layout [12]"""
    R1 = np.asarray(x1[1:10]).reshape(3, 3); R3 = np.asarray(x3[1:10]).reshape(3, 3)
    dR = _mm(R3, R1.T)
    dp = np.asarray(x3[10:13]) - _mv(dR, x1[10:13])
    return np.concatenate([dR.ravel(), dp])


def apply_dx(state25, dx12):
    """ScanPose::update (LR:29-34) / VS:1299-1305: v = dR v; p = dR p + dp; R = dR R"""
    s = np.array(state25, dtype=np.float64)
    dR = np.asarray(dx12[:9]).reshape(3, 3); dp = np.asarray(dx12[9:])
    s[13:16] = _mv(dR, state25[13:16])
    s[10:13] = _mv(dR, state25[10:13]) + dp
    s[1:10] = _mm(dR, np.asarray(state25[1:10]).reshape(3, 3)).ravel()
    return s


def loop_update_states(dx12, bl, x_buf, win_count, x_curr, g_update):
    """VS:1286-1331 and VS:1366-1367 -> (bl, x_buf, x_curr, g_update) after the call"""
    dR = np.asarray(dx12[:9]).reshape(3, 3)
    bl = np.array([apply_dx(b, dx12) for b in bl]).reshape(-1, 25)
    x_buf = np.array(x_buf, dtype=np.float64)
    for i in range(win_count):
        g = x_buf[i, 22:25].copy()
        x_buf[i] = apply_dx(x_buf[i], dx12)
        if g_update == 1:
            x_buf[i, 22:25] = _mv(dR, g)
    xc = np.array(x_curr, dtype=np.float64)
    v = _mv(dR, xc[13:16])
    xc[1:10] = x_buf[win_count - 1, 1:10]; xc[10:13] = x_buf[win_count - 1, 10:13]
    xc[13:16] = v; xc[22:25] = x_buf[win_count - 1, 22:25]
    return bl, x_buf, xc, (2 if g_update == 1 else g_update)


def pose_of(state25):
    return np.concatenate([np.asarray(state25[1:10]), np.asarray(state25[10:13])])


def move_pose(pose12, dx12):
    """a pose [12] moved by dx, as apply_dx moves a state"""
    s = np.zeros(25); s[1:10] = pose12[:9]; s[10:13] = pose12[9:]
    return pose_of(apply_dx(s, dx12))


_host = None


def host():
    """tests/host/loop_host.cpp as a shared library (g++, no contraction)"""
    global _host
    if _host is None:
        out = os.path.join(tempfile.mkdtemp(prefix="vba_loop_"), "libloophost.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-shared", "-o", out,
                               os.path.join(HERE, "host", "loop_host.cpp")])
        _host = C.CDLL(out)
    return _host


def cut_voxel_fix_var(omap, pnt_world, var, jour=0.0):
    """one fixed cut_voxel call with covariances on an oracle_api.VoxelMap"""
    p = np.ascontiguousarray(pnt_world, dtype=np.float64)
    v = np.ascontiguousarray(var, dtype=np.float64) if var is not None else None
    host().lh_map_cut_voxel_fix_var(omap.h, C.c_int(len(p)), p.ctypes.data_as(_dp), v.ctypes.data_as(_dp) if v is not None else None,
                                    C.c_double(jour))


def replay_build(omap, clouds, vardiags, poses, init_num=5, cumulative=True, fix_var=True):
    """VS:2601-2625 on the oracle with the reference's call sequence: one cut_voxel call per keyframe of the tail, each on the
    (cumulative) pvec_tem.  clouds / vardiags / poses are per keyframe of the store.  fix_var=False drops the covariances (what a
    fixed insertion without a covariance argument would store).  Returns the points inserted."""
    n = 0
    for call in expansion(len(clouds), init_num, cumulative):
        pw = np.concatenate([world(poses[i], clouds[i]) for i in call])
        var = np.concatenate([diag_var(vardiags[i]) for i in call])
        cut_voxel_fix_var(omap, pw, var if fix_var else None, 0.0)
        n += len(pw)
    return n


def replay_update(omap, oracle, bl_scans, bl_vars, bl_poses, win_scans, win_vars, win_poses, fix_var=True):
    """VS:1334-1363 on the oracle map that already holds map_loop (a fresh VoxelMapOracle has mp[i] = i): one fixed call per
    buf_lba2loop scan, cut_voxel per window frame, recut of every root.  Returns the oracle Factor of the recut."""
    wc = len(win_poses)
    for s, v, x in zip(bl_scans, bl_vars, bl_poses):
        cut_voxel_fix_var(omap, world(x, s), v if fix_var else None, 0.0)
    for i in range(wc):
        omap.cut_voxel(i, win_scans[i], win_poses[i], var=win_vars[i])
    f = oracle.Factor(omap.W)
    omap.recut(wc, np.ascontiguousarray(win_poses), f, multi=False)
    return f


def make_session(synth, n_kf=5, k_bl=3, W=4, extra=2, n_pts=20000):
    """The scene of the loop-closure tests: n_kf + k_bl + W + extra scans of the 10 x 8 x 3 m room along one trajectory (walls meeting
    in edges and corners at a 0.5 m voxel: roots that hold fixed points AND subdivide), perturbed poses, body covariances from the
    measurement model, a state covariance for pvec_update and a synthetic loop correction dx (VS:2597-2598 on a pose pair).
    Scans [0, n_kf) become keyframes, [n_kf, n_kf + k_bl) are marginalised before the loop closes (buf_lba2loop), the next W are
    the window, the rest arrive after loop_update."""
    import dataclasses
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="loop%d" % n_pts, n_pts=n_pts, win_size=W)
    n = n_kf + k_bl + W + extra
    s = synth.make_scans(dataclasses.replace(wl, win_size=n))
    poses = synth.poses_flat(s["R0"], s["p0"])
    vars_ = [np.ascontiguousarray(synth.calc_body_var(p, wl.dept_err, wl.beam_err).reshape(-1, 9)) for p in s["points"]]
    rng = np.random.default_rng(wl.seed + 7)
    A = rng.normal(0, 0.003, (15, 15))
    cov = A @ A.T + np.eye(15) * 1e-6
    x1 = np.zeros(25); x1[1:10] = poses[n_kf - 1, :9]; x1[10:13] = poses[n_kf - 1, 9:]
    x3 = x1.copy()
    x3[1:10] = (synth.so3_exp(np.array([0.004, -0.003, 0.012])) @ x1[1:10].reshape(3, 3)).ravel()
    x3[10:13] = x1[10:13] + np.array([0.06, -0.04, 0.015])
    return dict(wl=wl, W=W, n_kf=n_kf, k_bl=k_bl, points=s["points"], vars=vars_, poses=poses, cov=cov, dx=loop_dx(x1, x3))
