"""numpy restatement of Initialization::motion_init (voxelslam.cpp:470-819) for the tests of vba_motion_init.

The pieces without an oracle entry point are restated literally here (the backward IMU propagation and the point walk of
motion_blur, align_gravity); the map, the factor store, the LI-BA optimiser, the pre-integration and calcBodyVar / pvec_update
come from the C++ oracle through oracle_api.  TEST INFRASTRUCTURE only.
"""
import math

import numpy as np


def exp_dt(w, dt):
    """tools.hpp:68-84."""
    n = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if n <= 1e-7:
        return np.eye(3)
    a = w / n
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = n * dt
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def imu_poses(imu, xc, xl, beg_time, scale_gravity):
    """VS:508-544: rows [t, R(9), p(3), v(3), angvel(3), acc(3)], time descending."""
    bg, ba, g = xl[16:19], xl[19:22], xc[22:25]
    R = xc[1:10].reshape(3, 3).copy(); pos = xc[10:13].copy(); vel = xc[13:16].copy()
    rows = []
    for it in range(len(imu) - 1, 0, -1):
        head, tail = imu[it - 1], imu[it]
        w = 0.5 * (head[1:4] + tail[1:4]) - bg
        a = 0.5 * (head[4:7] + tail[4:7]) * scale_gravity - ba
        dt = head[0] - tail[0]
        E = exp_dt(w, dt)
        acc = R @ a + g
        pos = pos + vel * dt + 0.5 * acc * dt * dt
        vel = vel + acc * dt
        R = R @ E
        rows.append(np.concatenate([[head[0] - beg_time], R.ravel(), pos, vel, w, acc]))
    return np.array(rows).reshape(-1, 22)


def motion_blur(pnt, curv, imu, xc, xl, beg_time, ext, scale_gravity, point_notime=False):
    """VS:506-601 without the var: the compensated body points in the reference's push order (the literal walk)."""
    Rx, tx = ext[:9].reshape(3, 3), ext[9:12]
    if point_notime:
        return pnt @ Rx.T + tx
    tab = imu_poses(imu, xc, xl, beg_time, scale_gravity)
    Rc, pc = xc[1:10].reshape(3, 3), xc[10:13]
    out = []
    j = len(pnt) - 1
    if j < 0:
        return np.zeros((0, 3))
    for q in tab:
        R, p, v, w, a = q[1:10].reshape(3, 3), q[10:13], q[13:16], q[16:19], q[19:22]
        while curv[j] > q[0]:
            dt = curv[j] - q[0]
            Ri = R @ exp_dt(w, dt)
            T = p + v * dt + 0.5 * a * dt * dt - pc
            out.append(Rc.T @ (Ri @ (Rx @ pnt[j] + tx) + T))
            if j == 0:
                break
            j -= 1
    return np.array(out).reshape(-1, 3)


def align_gravity(xs):
    """VS:470-497 (Eigen::AngleAxisd::toRotationMatrix)."""
    xs = np.array(xs, dtype=np.float64, copy=True)
    g0 = xs[0, 22:25].copy()
    n0 = g0 / np.linalg.norm(g0)
    n1 = np.array([0.0, 0.0, -1.0 if n0[2] < 0 else 1.0])
    ax = np.cross(n0, n1)
    rn = np.linalg.norm(ax)
    ax = ax / rn
    ang = math.asin(rn)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    rot = math.cos(ang) * np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * np.outer(ax, ax)
    g0 = rot @ g0
    p0 = xs[0, 10:13].copy()
    for x in xs:
        x[10:13] = rot @ (x[10:13] - p0) + p0
        x[1:10] = (rot @ x[1:10].reshape(3, 3)).ravel()
        x[13:16] = rot @ x[13:16]
        x[22:25] = g0
    return xs


def motion_init(oa, W, wl, clouds, curvs, imus, beg_times, ext, dept_err, beam_err, scale_gravity, nm, nw, states, covs, imu_pre,
                point_notime=False, factor=None, vmap_out=None):
    """VS:617-819 on the oracle.  Returns the outputs of vba_motion_init plus the final map (vmap) and factor store (factor)."""
    xs = np.array(states, dtype=np.float64, copy=True)
    ip = np.array(imu_pre, dtype=np.float64, copy=True)
    eye = np.tile(np.eye(3).ravel(), 1)
    converge_flag, converge_thre, is_degrade, relaxed = 0, 0.05, True, True
    eig = np.zeros(3)
    log = []
    rounds = 0
    f = oa.Factor(W) if factor is None else factor
    vmap = None
    pvec = None
    hess = None
    for it in range(10):
        rounds = it + 1
        if converge_flag == 1:
            relaxed = False
        if relaxed:
            me, pt = 0.02, (0.25,) * 4
        else:
            me, pt = wl.min_eigen_value, wl.plane_thre
        vmap = oa.VoxelMap(W, wl.voxel_size, wl.max_layer, me, pt, wl.min_point, wl.max_points, 5)
        pvec = []
        poses = np.zeros((W, 12))
        for i in range(W):
            l = 0 if i == 0 else i - 1
            pb = motion_blur(clouds[i], curvs[i], imus[i], xs[i], xs[l], beg_times[i], ext, scale_gravity, point_notime)
            poses[i, :9] = xs[i, 1:10]; poses[i, 9:] = xs[i, 10:13]
            if converge_flag == 1:
                pb, vb = oa.var_init(pb, np.concatenate([np.eye(3).ravel(), np.zeros(3)]), dept_err, beam_err)
                var, _ = oa.pvec_update(pb, vb, xs[i], covs[i])
                var = var.reshape(-1, 9)
            else:
                var = np.tile(eye, (len(pb), 1))
            pvec.append((pb.copy(), var.reshape(-1, 3, 3).copy()))
            vmap.cut_voxel(i, pb, poses[i], var=var)
        f.clear()
        vmap.recut(W, poses, f, multi=False)
        nf = f.size()
        row = [nf, 0.0, 0.0, np.linalg.norm(xs[0, 22:25]), converge_flag]
        if nf < 10:
            log.append(row)
            break
        r = f.li_ba_damping_iter(xs, ip, gravity=True, imu_coef=wl.imu_coef, max_iter=3)
        xs, resis, hess = r["states"], r["resis"], r["hess"]
        for i in range(1, W):
            im = imus[i]
            ip[i - 1] = oa.imu_preintegrate(im[:, 0], im[:, 1:4], im[:, 4:7], xs[i - 1, 16:19], xs[i - 1, 19:22], nm, nw, scale_gravity)
        stop = False
        if abs(resis[0] - resis[1]) / resis[0] < converge_thre and it >= 2:
            _, evec, _ = f.read_back()
            v0 = evec.reshape(-1, 3, 3)[:, :, 0]
            nnt = v0.T @ v0
            eig = np.linalg.eigvalsh(nnt)
            is_degrade = eig[0] < 15
            converge_thre = 0.01
            if converge_flag == 0:
                xs = align_gravity(xs)
                converge_flag = 1
            else:
                stop = True
        row[1], row[2], row[3], row[4] = resis[0], resis[1], np.linalg.norm(xs[0, 22:25]), converge_flag
        log.append(row)
        if stop:
            break
    gnm = np.linalg.norm(xs[W - 1, 22:25])
    if is_degrade or gnm < 9.6 or gnm > 10.0:
        converge_flag = 0
    if converge_flag == 0:
        vmap = None
    return dict(converged=converge_flag, eigvalue3=eig, iterations=rounds, thresholds_left_relaxed=int(relaxed), round_log=np.array(log),
                states=xs, imu_pre=ip, hess=hess, pvec=pvec, vmap=vmap, factor=f)
