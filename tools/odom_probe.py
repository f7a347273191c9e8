"""Measurement of the scan-to-map EKF update for DESIGN.md section 17 (run on an MI355X): one 200k-point scan against the full
hesai200k_w10 window map (the set-up of bench.py's odometry_update), the same state and covariance for every call.
    python tools/odom_probe.py [out.json=profiles/odom_probe.json] [reps=5] [alone]
  (a) resident   vba_odom_lio_state_estimation_resident on device pointers (one upload, 8 launches, one download, one wait)
  (b) existing   vba_odom_lio_state_estimation, the staging front end of (a), on the SAME device pointers (a device-to-device copy of
                 points + covariances, then the loop of (a))
  (c) host       vba_odom_lio_state_estimation on host arrays (points + covariances uploaded per call: the number of the bench)
The three alternate in one process; median of `reps` after a warm-up round; host clocks around calls that end in a device
synchronise.  Every record holds the EKF iteration count: (a) reports its own, and (b), (c) run the same loop on a copy of the same
input (their results are checked against (a) at the bars of tests/test_gpu_odom.py).  Acceptance: median (a) <= median (b).
VBA_LIB=<another build's libvoxelba.so> times that build instead (an A/B run against a parent commit).
With `alone` every leg is timed by itself instead, back to back: 3 untimed calls, then 3 * reps timed ones, the three legs in turn,
twice; the record holds [median, min, max] per leg and block under "alone" (what a leg costs when its neighbours are calls of its
own kind, where the alternation gives what it costs after a call of another kind)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
from prof_summary import source_hash  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "odom_probe.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    wl = synth.CONFIGS["hesai200k_w10"]
    W = wl.win_size
    t0 = time.time()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")                # torch's HIP runtime comes up before the library's context, as in bench.py
    scans = synth.make_scans(wl)
    poses = synth.poses_flat(scans["R_gt"], scans["p_gt"])
    ctx = capi.Context(capi.options_from_workload(wl))
    rng = np.random.default_rng(1)

    def rand_var(n, scale):
        A = rng.normal(0, scale, (n, 3, 3))
        return np.ascontiguousarray((A @ A.transpose(0, 2, 1) + 1e-6 * np.eye(3)).reshape(n, 9))
    for i in range(W):
        ctx.cut_voxel(i, scans["points"][i], poses[i], var=rand_var(len(scans["points"][i]), 0.01), multi=True)
    ctx.recut(W, poses, multi=True)
    ctx.margi(W, poses, jour=0.0)                  # plane_update runs inside margi
    k = W - 1
    state = np.zeros(25); state[1:10] = scans["R_gt"][k].ravel(); state[10:13] = scans["p_gt"][k] + 0.01; state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4
    pts = np.ascontiguousarray(scans["points"][k], dtype=np.float64); var_b = rand_var(len(pts), 0.005)
    n = len(pts)
    d_p = torch.from_numpy(pts).to("cuda:0"); d_v = torch.from_numpy(var_b).to("cuda:0")
    torch.cuda.synchronize()
    ctx.synchronize()
    print("%d points, W = %d (%.1f s to set up)" % (n, W, time.time() - t0), flush=True)

    def resident():
        ok, st, cv, rep = ctx.lio_state_estimation_resident(n, d_p.data_ptr(), d_v.data_ptr(), state, cov)
        return ok, st, cv, rep["iterations"]

    def existing():
        return ctx.lio_state_estimation_dev(n, d_p.data_ptr(), d_v.data_ptr(), state, cov) + (None,)

    def host():
        return ctx.lio_state_estimation(pts, var_b, state, cov) + (None,)

    legs = (("resident_dev", resident), ("existing_dev", existing), ("existing_host", host))
    if len(sys.argv) > 3 and sys.argv[3] == "alone":
        res = dict(source_hash=source_hash(), workload=wl.name, points=n, reps=3 * reps, alone={})
        for block in range(2):
            for name, f in legs:
                for _ in range(3):
                    f()
                t = []
                for _ in range(3 * reps):
                    t1 = time.perf_counter(); f(); t.append((time.perf_counter() - t1) * 1e3)
                res["alone"]["%s_%d" % (name, block)] = [float(np.median(t)), float(min(t)), float(max(t))]
                print("%-14s alone, block %d: median %.4f ms (min %.4f, max %.4f)" % (name, block, np.median(t), min(t), max(t)), flush=True)
        ctx.close()
        json.dump(res, open(out_path, "w"), indent=1)
        print("OK")
        return
    recs = {name: [] for name, _ in legs}
    out = {}
    for r in range(reps + 1):                      # round 0 is the warm-up
        for name, f in legs:
            t1 = time.perf_counter(); res = f(); dt = time.perf_counter() - t1
            out[name] = res
            if r:
                recs[name].append(dt * 1e3)
    ok_a, st_a, cv_a, iters = out["resident_dev"]
    for name in ("existing_dev", "existing_host"):
        ok_b, st_b, cv_b, _ = out[name]
        assert ok_a == ok_b, name
        assert np.abs(st_a - st_b).max() < 1e-7, (name, np.abs(st_a - st_b).max())
        assert np.abs(cv_a - cv_b).max() < 1e-9 * np.abs(cv_b).max(), name
    rep = ctx.lio_state_estimation_resident(n, d_p.data_ptr(), d_v.data_ptr(), state, cov)[3]
    res = dict(source_hash=source_hash(), workload=wl.name, points=n, reps=reps, converged=bool(ok_a), iterations=int(iters),
               match_num=[int(x) for x in rep["match_num"]], nnt_eig_min=float(rep["nnt_eig_min"]),
               state_vs_existing=float(np.abs(st_a - out["existing_dev"][1]).max()))
    for name, _ in legs:
        t = np.array(recs[name])
        res[name] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), iterations=int(iters), runs_ms=[float(x) for x in t])
        print("%-14s median %.3f ms (min %.3f, max %.3f), %d EKF iterations" % (name, np.median(t), t.min(), t.max(), iters), flush=True)
    res["resident_over_existing_dev"] = res["resident_dev"]["median_ms"] / res["existing_dev"]["median_ms"]
    res["acceptance_met"] = bool(res["resident_dev"]["median_ms"] <= res["existing_dev"]["median_ms"])
    print("resident / existing on device pointers: %.3f -> acceptance %s" % (res["resident_over_existing_dev"], "met" if res["acceptance_met"] else "NOT met"))
    ctx.close()
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
