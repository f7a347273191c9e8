"""Cost of deterministic mode (vba_options::deterministic) at hesai200k_w10: both modes in one process, alternated
A/B/A/B, median of REPS rounds, for
  - K1: one 200k-point scan inserted into a map that holds the rest of the window (wall time of cut_voxel from device-resident points);
  - recut + factor extraction of the full window;
  - local_mapping_step (bench.py's step: margi, slide, pvec_update + cut_voxel_multi, multi recut, 3 LM iterations), lidar-only and LI-BA;
  - down_sampling_pvec of one scan.
Prints one JSON line per quantity and the source hash.  Kernel times of the new passes: run it under rocprofv3 --kernel-trace --stats."""
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctypes as C  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import voxel_slam_amd  # noqa: E402,F401
from voxel_slam_amd import capi, synth  # noqa: E402
from prof_summary import source_hash  # noqa: E402

REPS, STEPS, TURNOVER = int(os.environ.get("DET_PROBE_REPS", "5")), 8, 3
wl = synth.CONFIGS["hesai200k_w10"]
W = wl.win_size
nscan = W + TURNOVER + STEPS
wll = dataclasses.replace(wl, name=wl.name + "_traj%d" % nscan, win_size=nscan)
sl = synth.make_scans(wll)
x0 = synth.poses_flat(sl["R0"], sl["p0"])
ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
cov = np.eye(15) * 1e-6
imu_samples, vel, grav = synth.make_imu(wll, gyr_sigma=1e-3, acc_sigma=1e-2)
nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
imu_all = np.stack([capi.imu_preintegrate(t, gy, ac, np.zeros(3), np.zeros(3), nm, nw) for (t, gy, ac) in imu_samples])


def make_ctx(det):
    o = capi.options_from_workload(wl, stream=torch.cuda.current_stream().cuda_stream)
    o.max_points_per_scan, o.max_map_nodes, o.max_fix_points, o.max_voxels = 1 << 18, 1 << 21, 1 << 23, 1 << 17
    o.deterministic = det
    return capi.Context(o)


def sync():
    torch.cuda.synchronize()


def k1_and_recut(det):
    ctx = make_ctx(det)
    dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in sl["points"][:W]]
    t_ins = []
    for i in range(W):
        sync(); t0 = time.perf_counter()
        ctx._chk(ctx.lib.vba_map_cut_voxel(ctx.h, C.c_int(i), C.c_int(dev[i].shape[0]), C.c_void_p(dev[i].data_ptr()), None,
                                           x0[i].ctypes.data_as(C.POINTER(C.c_double)), C.c_int(0)))
        sync(); t_ins.append(time.perf_counter() - t0)
    sync(); t0 = time.perf_counter()
    ctx.recut(W, x0[:W], multi=False)
    sync(); t_rec = time.perf_counter() - t0
    ctx.close()
    return 1e6 * float(np.median(t_ins[1:])), 1e6 * t_rec


def session(det, li):
    ctx = make_ctx(det)
    pv = [ctx.var_init(p, ext, wl.dept_err, wl.beam_err) for p in sl["points"]]
    dp = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a, _ in pv]
    dv = [torch.from_numpy(np.ascontiguousarray(b)).cuda() for _, b in pv]

    def insert(slot, idx, pose):
        ctx._chk(ctx.lib.vba_map_pvec_update_cut_voxel(ctx.h, C.c_int(slot), C.c_int(dp[idx].shape[0]), C.c_void_p(dp[idx].data_ptr()),
                                                      C.c_void_p(dv[idx].data_ptr()), pose.ctypes.data_as(C.POINTER(C.c_double)),
                                                      cov.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(1)))
    for i in range(W):
        insert(i, i, x0[i])
    ctx.recut(W, x0[:W], multi=True)
    window, last, states, ts = np.ascontiguousarray(x0[:W]), W - 1, np.zeros((W, 25)), []
    for k in range(TURNOVER + STEPS):
        t0 = time.perf_counter()
        ctx.margi(W, window, jour=float(last)); ctx.slide(1)
        last += 1
        insert(W - 1, last, x0[last])
        pw = np.ascontiguousarray(np.concatenate([window[1:], x0[last:last + 1]]))
        ctx.recut(W, pw, multi=True)
        if li:
            for i in range(W):
                j = last - W + 1 + i
                states[i, 0] = 0.1 * j; states[i, 1:10] = pw[i, :9]; states[i, 10:13] = pw[i, 9:12]; states[i, 13:16] = vel[j]; states[i, 22:25] = grav
            r = ctx.li_ba_damping_iter(states, imu_all[last - W + 1:last], gravity=False, max_iter=3)
            window = np.ascontiguousarray(np.concatenate([r["states"][:, 1:10], r["states"][:, 10:13]], 1))
        else:
            ctx.lm_begin(pw, thd_num=2)
            for _ in range(3):
                ctx.lm_iterate(sync=False)
            window = np.ascontiguousarray(ctx.lm_end(fetch=True)[0])
        if k >= TURNOVER:
            ts.append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    return float(np.median(ts))


def down_sampling(det):
    ctx = make_ctx(det)
    p, v = ctx.var_init(sl["points"][0], ext, wl.dept_err, wl.beam_err)
    ctx.down_sampling_pvec(p, v, 0.5)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); ctx.down_sampling_pvec(p, v, 0.5); ts.append(time.perf_counter() - t0)
    ctx.close()
    return 1e6 * float(np.median(ts))


res = {q: {0: [], 1: []} for q in ("k1_scan_us", "recut_extract_us", "step_lidar_only_ms", "step_li_ba_ms", "down_sampling_pvec_us")}
for rep in range(REPS):
    for det in (0, 1) if rep % 2 == 0 else (1, 0):
        a, b = k1_and_recut(det)
        res["k1_scan_us"][det].append(a); res["recut_extract_us"][det].append(b)
        res["step_lidar_only_ms"][det].append(session(det, False))
        res["step_li_ba_ms"][det].append(session(det, True))
        res["down_sampling_pvec_us"][det].append(down_sampling(det))
for q, v in res.items():
    d0, d1 = float(np.median(v[0])), float(np.median(v[1]))
    print(json.dumps({"quantity": q, "default": d0, "deterministic": d1, "ratio": d1 / d0, "spread_default": [min(v[0]), max(v[0])],
                      "spread_deterministic": [min(v[1]), max(v[1])], "reps": REPS}))
print(json.dumps({"source_hash": source_hash(), "workload": wl.name}))
