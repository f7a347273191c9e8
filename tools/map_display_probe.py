"""Measurements of the local-map display export for DESIGN.md section 24 (run on an MI355X): vba_map_display on the hesai200k_w10
window (10 scans inserted and recut at their R0 / p0 poses), into device buffers and into host memory, in one process.
    python tools/map_display_probe.py [out.json = profiles/map_display_probe.json] [reps=5] [config=hesai200k_w10]
Legs, alternating after one warm-up round, median of `reps` with the spread:
  device   the call with device result buffers, timed with its one wait and to the end of the stream's work
  host     the call with host result buffers (staging, four copies, a second wait)
  sizes    the size query alone (everything up to the one wait)
Beside the times: (bytes read + written) / time, the bytes the passes cannot avoid, against the float4 copy rate MI355X reaches:
  per window point   40 = perm, pleaf, the inverse's fill and write (16), then inverse, pleaf and plane index in each of the two passes (24)
  per kept point     44 = the body point (24), the record (16), the plane index (4)
  per node           12 = state, layer, touched and plane flags in each of the two node passes (8), the plane index (4)
  per plane         233 = pcr_add (80), pcr_fix.N (8), quater_length (4), voxel_center (24), key (8), layer and path (5), record (64), key out (40)
There is no parent leg: before this call nothing could reach these points.  Times are host clocks around work that ends drained."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
from export_probe import COPY_RATE, hip_runtime
from prof_summary import source_hash  # noqa: E402

C = capi.C


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_display_probe.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    name = sys.argv[3] if len(sys.argv) > 3 else "hesai200k_w10"
    wl = synth.CONFIGS[name]
    W = wl.win_size
    t0 = time.time()
    s = synth.make_scans(wl)
    poses = synth.poses_flat(s["R0"], s["p0"])
    ctx = capi.Context(capi.options_from_workload(wl))
    for i in range(W):
        ctx.cut_voxel(i, s["points"][i], poses[i])
    ctx.recut(W, poses, multi=False)
    window = int(sum(len(p) for p in s["points"]))
    n, m, fb = ctx.map_display_sizes(W, poses)
    nodes = ctx.map_stats()["nodes_high_water"]
    print("%s: %d window points, %d nodes, %d planes, %d points in planes (%.1f s to set up)" % (name, window, nodes, m, n, time.time() - t0), flush=True)
    ctx.map_display_reserve(window, m)
    alloc0 = ctx.map_display_allocations()
    hip = hip_runtime()
    bufs = [C.c_void_p() for _ in range(4)]
    for d, b in zip(bufs, (16 * n, 4 * n, 64 * m, 40 * m)):
        assert hip.hipMalloc(C.byref(d), C.c_size_t(max(b, 16))) == 0
    kept = {}

    def device():
        r = ctx.map_display(W, poses, device_out=(n, bufs[0], bufs[1], m, bufs[2], bufs[3]))
        ctx.synchronize()
        kept["device"] = (r["n_points"], r["n_planes"])

    def host():
        r = ctx.map_display(W, poses)
        kept["host"] = (len(r["xyzi"]), len(r["planes"]))

    def sizes():
        kept["sizes"] = ctx.map_display_sizes(W, poses)[:2]

    legs = [("device", device), ("host", host), ("sizes", sizes)]
    t = {k: [] for k, _ in legs}
    for rep in range(reps + 1):                               # round 0 is the warm-up
        for k, f in legs:
            a = time.perf_counter(); f(); b = time.perf_counter()
            if rep:
                t[k].append((b - a) * 1e3)
    assert kept["device"] == kept["host"] == kept["sizes"] == (n, m)
    assert ctx.map_display_allocations() == alloc0            # (Context.map_display's host leg asks for max(n, 1) and max(m, 1) records: no more)
    algo = 40.0 * window + 44.0 * n + 12.0 * nodes + 233.0 * m
    res = dict(source_hash=source_hash(), config=name, window_points=window, nodes=int(nodes), planes=int(m), points_in_planes=int(n), reps=reps,
               algorithmic_bytes=algo, copy_rate_bytes_per_s=COPY_RATE, allocations=list(alloc0))
    for k, _ in legs:
        v = np.array(t[k])
        res[k + "_ms"] = dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))
    res["device_bytes_per_s"] = algo / (res["device_ms"]["median"] * 1e-3)
    res["device_share_of_copy_rate"] = res["device_bytes_per_s"] / COPY_RATE
    print("device %.3f ms (%.3f .. %.3f) | host %.3f ms (%.3f .. %.3f) | size query %.3f ms (%.3f .. %.3f)"
          % tuple(res[k + "_ms"][q] for k in ("device", "host", "sizes") for q in ("median", "min", "max")), flush=True)
    print("device leg: %.3g algorithmic bytes -> %.3g bytes/s = %.1f %% of the %.3g bytes/s float4 copy rate"
          % (algo, res["device_bytes_per_s"], 100 * res["device_share_of_copy_rate"], COPY_RATE), flush=True)
    for d in bufs:
        assert hip.hipFree(d) == 0
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
