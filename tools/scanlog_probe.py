"""Measurements of the scan log for DESIGN.md section 20 (run on an MI355X): what it costs, per scan, to keep a marginalised scan
until it is part of a keyframe.  One synthetic Hesai message of 230 400 records (the bench's hesai200k_w10 size) is decoded and
prepared once; the prepared scan stands in every frame of a window of W = 10.  A round is ten scans and one keyframe; the two routes
alternate in one process, median of `reps` rounds after a warm-up, host clocks, every round ended by a device synchronise.
    python tools/scanlog_probe.py [out.json=profiles/scanlog_probe.json] [n_raw=230400] [reps=5]
  Route A  what a node does today: vba_scan_frame_read stage 3 (points and covariances to the host, with its synchronise), the host
           copy into the ScanPose, and every ten scans vba_kf_build from the ten host arrays
  Route B  vba_scanlog_push_window per scan (device to device, no synchronise), and every ten scans vba_kf_build_from_log, then release
Both routes build into stores that are reserved, so no round allocates.  Route A's covariances are the frame's body covariances and
Route B's the map's world covariances: the kept clouds are the same points, the diagonals differ."""
import dataclasses
import json
import os
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

DOWN_SIZE, MIN_POINTS, BLIND2, VS10, K = 0.1, 500, 0.25, 0.05, 10


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scanlog_probe.json")
    n_raw, reps = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 230400), (3, 5))]
    wl = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name="scanlog", n_pts=n_raw)
    W = wl.win_size
    assert W == K
    s = synth.make_scans(wl)
    rng = np.random.default_rng(9)
    ctx = capi.Context(capi.options_from_workload(wl))
    kctx = capi.Context(capi.options_from_workload(wl))           # the loop-closure thread's context: the stores hang off it
    frame = ctx.scan_frame()
    frame.reserve(n_raw, 26)
    layout = capi.scan_layout("hesai")
    pts = s["points"][0].astype(np.float32)
    msg = do.make_message(layout, pts, rng.uniform(0, 255, len(pts)), 1.7e9 + np.sort(rng.uniform(0.0, 0.1, len(pts))))
    frame.decode(layout, msg, 1, BLIND2)
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    ip = np.zeros((2, 22)); ip[:, 0] = [0.0, 0.05]; ip[:, 1:10] = np.eye(3).ravel()
    n, dp, dv = frame.prepare(ip, ext, ext, DOWN_SIZE, wl.dept_err, wl.beam_err, min_points=MIN_POINTS)
    poses = synth.poses_flat(s["R_gt"], s["p_gt"])
    cov = np.eye(15) * 1e-4
    for i in range(W):
        ctx.pvec_update_cut_voxel_dev(i, n, dp, dv, poses[i], cov, multi=True)
    ctx.synchronize()
    log = ctx.scan_log()
    log.reserve((K + 1) * n, 2 * K)
    st_a, st_b = kctx.kf_store(), kctx.kf_store()
    for st in (st_a, st_b):
        st.reserve(4 * (reps + 2) * K * n // 4 + K * n, reps + 4, K * n)
    C = capi.C
    h_pnt, h_var = np.zeros((n, 3)), np.zeros((n, 9))
    held = [(np.zeros((n, 3)), np.zeros((n, 9))) for _ in range(K)]          # the ScanPose::pvec of the ten scans
    print("%d rays, %d prepared points per scan, W = %d" % (n_raw, n, W), flush=True)

    def route_a(rnd):
        per = []
        for i in range(K):
            t0 = time.perf_counter()
            ctx._chk(ctx.lib.vba_scan_frame_read(frame.h, C.c_int(3), capi._p(h_pnt), None, None, None, None, capi._p(h_var)))
            np.copyto(held[i][0], h_pnt); np.copyto(held[i][1], h_var)
            per.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        kept, _, _ = st_a.build([h[0] for h in held], poses, VS10, id=rnd, vars=[h[1] for h in held])
        kctx.synchronize()
        return per, time.perf_counter() - t0, kept

    def route_b(rnd):
        per = []
        first = log.range()[1]
        for i in range(K):
            t0 = time.perf_counter()
            log.push_window(i)
            per.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        kept, _, _ = st_b.build_from_log(log, first, poses, VS10, id=rnd)
        log.release(first + K)
        kctx.synchronize(); ctx.synchronize()
        return per, time.perf_counter() - t0, kept

    a0, b0 = log.allocations(), st_b.allocations()
    ra, rb = [], []
    for r in range(reps + 1):
        for f, acc in ((route_a, ra), (route_b, rb)):
            t0 = time.perf_counter()
            per, tb, kept = f(r)
            acc.append(dict(scan=float(np.median(per)), build=tb, round=time.perf_counter() - t0, kept=kept))
    assert log.allocations() == a0 and st_b.allocations() == b0, "a measured round allocated"
    assert ra[-1]["kept"] == rb[-1]["kept"]

    def med(rows, key):
        t = np.array([x[key] for x in rows[1:]]) * 1e3
        return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))

    res = dict(source_hash=source_hash(), n_raw=n_raw, points_per_scan=n, scans_per_keyframe=K, reps=reps, kept_points=ra[-1]["kept"],
               bytes_per_scan_host_link=96 * n, bytes_per_scan_device_copy=2 * 96 * n)
    for name, rows in (("route_a", ra), ("route_b", rb)):
        res[name] = dict(per_scan_ms=med(rows, "scan"), build_ms=med(rows, "build"), round_ms=med(rows, "round"))
        res[name]["per_scan_with_build_share_ms"] = res[name]["round_ms"]["median"] / K
    res["a_over_b_per_scan"] = res["route_a"]["per_scan_ms"]["median"] / res["route_b"]["per_scan_ms"]["median"]
    res["a_over_b_round"] = res["route_a"]["round_ms"]["median"] / res["route_b"]["round_ms"]["median"]
    for name in ("route_a", "route_b"):
        r = res[name]
        print("%s: per scan %.3f ms | keyframe build %.3f ms | round of %d scans %.3f ms (%.3f ms per scan)"
              % (name, r["per_scan_ms"]["median"], r["build_ms"]["median"], K, r["round_ms"]["median"], r["per_scan_with_build_share_ms"]), flush=True)
    print("A / B: per scan %.1f, per round %.2f" % (res["a_over_b_per_scan"], res["a_over_b_round"]))
    kctx.close(); ctx.close()
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
