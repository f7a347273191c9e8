"""Measurements of the per-scan front chain on a resident odometry state for DESIGN.md section 21 (run on an MI355X): one synthetic
26-byte-step Hesai message of 230 400 records (about 200k points after the filter), 21 IMU rows, against a map that a short
local-mapping session built, as tools/frontend_probe.py sets it up.  Wall time on host clocks, each leg ended by a device
synchronise; median, min and max of `reps` runs after a warm-up.
    python tools/odom_state_probe.py [out.json=profiles/odom_state_probe.json] [n_raw=230400] [reps=9] [kernel_trace_dir]
    python tools/odom_state_probe.py --propagate-only [launches=50]
  (p) parent    the three host-fed calls of the chain: vba_scan_prepare, vba_odom_lio_state_estimation_resident,
                vba_map_pvec_update_cut_voxel on the frame's device pointers, with the propagation's outputs (pose table, end_pose,
                state, covariance) computed beforehand and NOT timed: this favours the parent
  (s) on state  vba_odom_state_propagate (timed), vba_scan_prepare_on_state, vba_odom_lio_state_estimation_on_state,
                vba_map_pvec_update_cut_voxel_on_state
The two legs alternate and swap their order from one repetition to the next; the map is rebuilt and the state set (both untimed)
before each leg, so both insert into the same map from the same state.  The host-fed calls are the parent's code unchanged, so one
library serves both legs.  The durations of k_imu_propagate, k_odom_begin_dev and k_odom_commit_dev come from a rocprofv3
--kernel-trace run of the --propagate-only mode, whose output directory is the fourth argument."""
import csv
import dataclasses
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
import decode_oracle as do
from prof_summary import source_hash  # noqa: E402

DOWN_SIZE, MIN_POINTS, BLIND2 = 0.1, 500, 0.25
NOISE = np.array([0.01] * 3 + [0.1] * 3 + [1e-4] * 3 + [1e-4] * 3)
M_IMU = 21


def imu_rows(rng, t0, R_wb):
    imu = np.zeros((M_IMU, 7))
    imu[:, 0] = t0 + 0.005 * np.arange(M_IMU)
    imu[:, 1:4] = rng.normal(0, 0.02, (M_IMU, 3))
    imu[:, 4:7] = R_wb.T @ np.array([0, 0, 9.8]) + rng.normal(0, 0.05, (M_IMU, 3))
    return imu


def start_state(s, k, rng):
    state = np.zeros(25)
    state[0] = 100.0
    state[1:10] = s["R_gt"][k].ravel(); state[10:13] = s["p_gt"][k] + rng.normal(0, 0.02, 3); state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4; cov[9:, 9:] = np.eye(6) * 1e-5
    return state, cov


def propagate_only(launches):
    """`launches` propagations on one state object, each followed by an update on an empty scan (the image built and copied back on
    the device), for a kernel trace"""
    rng = np.random.default_rng(9)
    ctx = capi.Context(capi.default_options())
    st = ctx.odom_state()
    state = np.zeros(25); state[1:10] = np.eye(3).ravel(); state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4
    imu = imu_rows(rng, 99.998, np.eye(3))
    for _ in range(launches):
        st.set(state, cov)
        st.propagate(imu, NOISE, 100.0, 100.001, float(imu[-1, 0] + 0.002))
        st.lio_state_estimation(0, 0, 0)
    st.get()
    ctx.close()
    print("OK", launches)


def kernel_ns(trace_dir, name):
    dur = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if name in r["Kernel_Name"]:
                dur.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    if not dur:
        return None
    return dict(launches=len(dur), median_ns=statistics.median(dur), min_ns=min(dur), max_ns=max(dur))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--propagate-only":
        return propagate_only(int(sys.argv[2]) if len(sys.argv) > 2 else 50)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "odom_state_probe.json")
    n_raw, reps = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 230400), (3, 9))]
    trace_dir = sys.argv[4] if len(sys.argv) > 4 else None
    wl = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name="odom_state", n_pts=n_raw, win_size=4)
    W, nscan = wl.win_size, 6
    t0 = time.time()
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    rng = np.random.default_rng(9)
    ctx = capi.Context(capi.options_from_workload(wl))
    frame = ctx.scan_frame()
    frame.reserve(n_raw, 26)
    st = ctx.odom_state()
    st.reserve(64)
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    layout = capi.scan_layout("hesai")
    k = nscan - 1
    pts = s["points"][k].astype(np.float32)
    msg = do.make_message(layout, pts, rng.uniform(0, 255, len(pts)), 1.7e9 + np.sort(rng.uniform(0.0, 0.1, len(pts))))
    state, cov = start_state(s, k, rng)
    last_end, beg = 100.0, 100.001
    imu = imu_rows(rng, 99.998, state[1:10].reshape(3, 3))
    end_t = float(imu[-1, 0] + 0.002)
    var0 = [np.tile((np.eye(3) * 1e-4).ravel(), (len(s["points"][j]), 1)) for j in range(nscan - 1)]

    def build_map():                                              # untimed: the local-mapping session that the scan meets
        ctx.map_reset()
        xs, wc = [], 0
        for j in range(nscan - 1):
            xs.append(synth.poses_flat(s["R_gt"][j:j + 1], s["p_gt"][j:j + 1])[0])
            wc += 1
            ctx.cut_voxel(wc - 1, s["points"][j], xs[-1], var=var0[j], multi=True)
            ctx.recut(wc, np.array(xs), multi=True)
            if wc >= W:
                ctx.margi(wc, np.array(xs), jour=float(j))
                ctx.slide(1); xs = xs[1:]; wc -= 1
        st.set(state, cov)
        ctx.synchronize()
        return wc

    n, _ = frame.decode(layout, msg, 1, BLIND2)
    # the propagation's outputs for the parent leg, untimed: the library's own host propagation
    x_prop, cov_prop, table, end_pose = capi.imu_ekf_propagate(imu, NOISE, last_end, beg, end_t, state, cov)
    print("%d rays, %d decoded, %d scans, %d pose rows (%.1f s to set up)" % (n_raw, n, nscan, len(table), time.time() - t0), flush=True)

    def parent(wc):
        m, dp, dv = frame.prepare(table, end_pose, ext, DOWN_SIZE, wl.dept_err, wl.beam_err, min_points=MIN_POINTS)
        ok, x, cv, rep = ctx.lio_state_estimation_resident(m, dp, dv, x_prop, cov_prop)
        ctx.pvec_update_cut_voxel_dev(wc, m, dp, dv, np.concatenate([x[1:10], x[10:13]]), cv, multi=True)
        ctx.synchronize()
        return m, x

    def on_state(wc):
        st.propagate(imu, NOISE, last_end, beg, end_t)
        m, dp, dv = st.prepare(frame, ext, DOWN_SIZE, wl.dept_err, wl.beam_err, min_points=MIN_POINTS)
        ok, x, rep = st.lio_state_estimation(m, dp, dv)
        st.pvec_update_cut_voxel(wc, m, dp, dv, multi=True)
        ctx.synchronize()
        return m, x

    tp, ts = [], []
    for r in range(reps + 1):
        legs = ((parent, tp), (on_state, ts))
        for f, t in (legs if r % 2 == 0 else legs[::-1]):
            wc = build_map()
            t1 = time.perf_counter(); m, x = f(wc); t.append((time.perf_counter() - t1, m, x))
    assert tp[-1][1] == ts[-1][1]
    dx = float(np.abs(tp[-1][2] - ts[-1][2]).max())                # the device propagation against the host's, after the update

    def med(t):
        t = np.array([v[0] for v in t[1:]]) * 1e3
        return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))

    p, q = med(tp), med(ts)
    res = dict(source_hash=source_hash(), n_raw=n_raw, decoded=n, prepared=tp[-1][1], imu_rows=M_IMU, pose_rows=len(table), reps=reps,
               down_size=DOWN_SIZE, parent_ms=p, on_state_ms=q, on_state_minus_parent_ms=q["median"] - p["median"],
               parent_spread_ms=p["max"] - p["min"], state_difference_after_update=dx,
               kernels={k: kernel_ns(trace_dir, k) for k in ("k_imu_propagate", "k_odom_begin_dev", "k_odom_commit_dev")} if trace_dir else None)
    print("parent %.3f ms (%.3f .. %.3f) | on state, propagation included %.3f ms (%.3f .. %.3f) | difference %.3f ms, parent's spread %.3f ms"
          % (p["median"], p["min"], p["max"], q["median"], q["min"], q["max"], res["on_state_minus_parent_ms"], res["parent_spread_ms"]), flush=True)
    print("kernels:", res["kernels"])
    frame.close(); ctx.close()
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
