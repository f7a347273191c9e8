"""Measurement of the initialisation odometry for DESIGN.md section 18 (run on an MI355X): one 0.5 m down-sampled scan of the
hesai200k_w10 scene against the point-cloud map that four such scans leave, the same state and covariance for every call.
    python tools/kd_probe.py [out.json=profiles/kd_probe.json] [reps=5]
  (a) resident   vba_odom_lio_state_estimation_kdtree_resident on a device pointer (one upload, 17 launches + the re-sampling, one
                 download, one wait)
  (b) existing   vba_odom_lio_state_estimation_kdtree, the staging front end of (a), on the SAME device pointer (a device-to-device
                 copy of the points, then the loop of (a))
  (c) host       vba_odom_lio_state_estimation_kdtree on a host array (the points uploaded per call)
The three alternate in one process.  Before every call the map is put back, untimed: pl_tree->clear() and one seeding call at the
identity pose on the saved map points (which are float values, so the append reproduces them bit for bit), then a synchronise.
Median of `reps` after a warm-up round; host clocks around calls that end in a device synchronise.  Every record holds n, the map
size and the EKF iteration count; (b) and (c) are checked against (a) at the bars of tests/test_gpu_odom.py.
Acceptance: median (a) <= median (b).  No per-kernel trace is taken: nothing is claimed about how the time divides.
VBA_LIB=<another build's libvoxelba.so> times that build instead (an A/B run against a parent commit)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctypes as C
import numpy as np
import torch
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
from prof_summary import source_hash  # noqa: E402

N_MAP_SCANS = 4


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kd_probe.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    wl = synth.CONFIGS["hesai200k_w10"]
    t0 = time.time()
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")                # torch's HIP runtime comes up before the library's context, as in bench.py
    scans = synth.make_scans(wl)
    ctx = capi.Context(capi.options_from_workload(wl))

    def state_of(k, dp=0.0):
        s = np.zeros(25); s[1:10] = scans["R_gt"][k].ravel(); s[10:13] = scans["p_gt"][k] + dp; s[22:25] = [0, 0, -9.8]
        return s
    cov = np.eye(15) * 1e-4
    cov[9:, 9:] = np.eye(6) * 1e-5
    ds = [np.ascontiguousarray(ctx.down_sampling_voxel(scans["points"][k], 0.5)[0], dtype=np.float64) for k in range(N_MAP_SCANS + 1)]
    c = cov
    for k in range(N_MAP_SCANS):                   # the map: a seed and three estimations, each followed by the 0.5 m re-sampling
        it, _, c2 = ctx.lio_state_estimation_kdtree(ds[k], state_of(k), c)
        c = c2 if it else c
    tree = np.ascontiguousarray(ctx.kdtree_points())
    m = len(tree)
    pts = ds[N_MAP_SCANS]; n = len(pts)
    state = state_of(N_MAP_SCANS, 0.01)
    d_p = torch.from_numpy(pts).to("cuda:0"); d_tree = torch.from_numpy(tree).to("cuda:0")
    torch.cuda.synchronize()
    ident = np.zeros(25); ident[1:10] = np.eye(3).ravel()
    ctx.kdtree_reserve(2 * (m + n), n)
    print("scan of %d points, map of %d (%.1f s to set up)" % (n, m, time.time() - t0), flush=True)

    def restore():
        ctx._chk(ctx.lib.vba_odom_kdtree_reset(ctx.h))
        it, _, _, _ = ctx.lio_state_estimation_kdtree_resident(m, d_tree.data_ptr(), ident, cov)
        assert it == 0 and ctx.kdtree_size() == m
        ctx.synchronize()

    def resident():
        it, st, cv, rep = ctx.lio_state_estimation_kdtree_resident(n, d_p.data_ptr(), state, cov)
        return it, st, cv

    def existing():
        st = state.copy(); cv = cov.copy(); it = C.c_int(0)
        ctx._chk(ctx.lib.vba_odom_lio_state_estimation_kdtree(ctx.h, C.c_int(n), C.c_void_p(d_p.data_ptr()), capi._p(st), capi._p(cv), C.byref(it)))
        return it.value, st, cv

    def host():
        return ctx.lio_state_estimation_kdtree(pts, state, cov)

    restore()
    assert np.array_equal(ctx.kdtree_points(), tree)
    legs = (("resident_dev", resident), ("existing_dev", existing), ("existing_host", host))
    recs = {name: [] for name, _ in legs}
    out, maps = {}, {}
    for r in range(reps + 1):                      # round 0 is the warm-up
        for name, f in legs:
            restore()
            t1 = time.perf_counter(); res = f(); dt = time.perf_counter() - t1
            out[name] = res; maps[name] = ctx.kdtree_size()
            if r:
                recs[name].append(dt * 1e3)
    it_a, st_a, cv_a = out["resident_dev"]
    for name in ("existing_dev", "existing_host"):
        it_b, st_b, cv_b = out[name]
        assert it_a == it_b, name
        assert np.abs(st_a - st_b).max() < 1e-5, (name, np.abs(st_a - st_b).max())
        assert np.abs(cv_a - cv_b).max() < 1e-4 * np.abs(cv_b).max(), name
        assert abs(maps[name] - maps["resident_dev"]) <= max(2, maps[name] // 500), name
    restore()
    rep = ctx.lio_state_estimation_kdtree_resident(n, d_p.data_ptr(), state, cov)[3]
    res = dict(source_hash=source_hash(), workload=wl.name, points=n, map_points=m, map_points_after=int(maps["resident_dev"]), reps=reps,
               iterations=int(it_a), match_num=[int(x) for x in rep["match_num"]], state_vs_existing=float(np.abs(st_a - out["existing_dev"][1]).max()),
               per_kernel_trace=False)
    for name, _ in legs:
        t = np.array(recs[name])
        res[name] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), points=n, map_points=m, iterations=int(it_a),
                         runs_ms=[float(x) for x in t])
        print("%-14s median %.3f ms (min %.3f, max %.3f), n %d, map %d, %d EKF iterations" % (name, np.median(t), t.min(), t.max(), n, m, it_a), flush=True)
    res["resident_over_existing_dev"] = res["resident_dev"]["median_ms"] / res["existing_dev"]["median_ms"]
    res["acceptance_met"] = bool(res["resident_dev"]["median_ms"] <= res["existing_dev"]["median_ms"])
    print("resident / existing on device pointers: %.3f -> acceptance %s" % (res["resident_over_existing_dev"], "met" if res["acceptance_met"] else "NOT met"))
    ctx.close()
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
