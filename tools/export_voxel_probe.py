"""Measurements of the voxel-down-sampled global map for DESIGN.md section 23 (run on an MI355X): vba_kf_voxel_export against what
a node could do before it, on the store of tools/export_probe.py, in one process.
    python tools/export_voxel_probe.py [out.json] [n_kf=200] [scans_per_kf=3] [n_pts=60000] [reps=5]
Legs, alternating after one warm-up round, median of `reps` with the spread:
  voxel    vba_kf_voxel_export at jump 1 into device buffers, on a default and on a deterministic context (timed with its one wait
           and to the end of the stream's work)
  parent   vba_kf_export_world to host memory, widening to double, vba_scan_down_sampling_voxel (host in, host out)
at voxel 0.1 and 0.2.  Beside the ratio voxel / parent: (24 + 16 voxels / points) bytes x points / time, the bytes the call cannot
avoid (the store read once, the result written once), against the float4 copy rate MI355X reaches.  Times are host clocks."""
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


def context(det):
    o = capi.default_options()
    o.deterministic = det
    return capi.Context(o)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n_kf, spk, n_pts, reps = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 200), (3, 3), (4, 60000), (5, 5))]
    t0 = time.time()
    ctx = {"default": context(0), "deterministic": context(1)}
    store = ctx["default"].kf_store()
    for k, kf in enumerate(synth.make_keyframe_path(n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, with_var=False)):
        store.build(kf["points"], kf["poses"], 0.05, id=k, jour=0.0)
        if k % 20 == 19:
            print("  %d keyframes built (%.1f s)" % (k + 1, time.time() - t0), flush=True)
    total = int(store.sizes().sum())
    print("store: %d keyframes of %d x %d rays, %d points resident (%.1f s to set up)" % (n_kf, spk, n_pts, total, time.time() - t0), flush=True)
    res = dict(source_hash=source_hash(), n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, points=total, reps=reps, copy_rate_bytes_per_s=COPY_RATE)
    hip = hip_runtime()
    dx, dc = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dx), C.c_size_t(16 * max(total, 1))) == 0 and hip.hipMalloc(C.byref(dc), C.c_size_t(4 * max(total, 1))) == 0
    for c in ctx.values():
        c.kf_export_voxel_reserve(total)
    res["allocations_after_reserve"] = {k: c.kf_export_voxel_allocations() for k, c in ctx.items()}

    for voxel in (0.1, 0.2):
        kept = {}

        def new(mode):
            kept[mode] = ctx[mode].kf_export_voxel([store], [0.0], 1, voxel, cap=total, out=(dx, dc))
            ctx[mode].synchronize()

        def parent():
            S = ctx["default"].kf_export_world([store], [0.0], 1)
            pnt, cnt, first = ctx["default"].down_sampling_voxel(S[:, :3].astype(np.float64), voxel)
            kept["parent"] = len(pnt)

        legs = [("default", lambda: new("default")), ("deterministic", lambda: new("deterministic")), ("parent", parent)]
        t = {name: [] for name, _ in legs}
        for rep in range(reps + 1):                           # round 0 is the warm-up: buffers grow there
            for name, f in legs:
                a = time.perf_counter(); f(); b = time.perf_counter()
                if rep:
                    t[name].append((b - a) * 1e3)
        assert kept["default"] == kept["deterministic"] == kept["parent"]
        r = dict(voxels=kept["default"])
        for name, _ in legs:
            v = np.array(t[name])
            r[name + "_ms"] = dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))
        for mode in ("default", "deterministic"):
            r[mode + "_over_parent"] = r[mode + "_ms"]["median"] / r["parent_ms"]["median"]
            r[mode + "_bytes_per_s"] = (24.0 + 16.0 * r["voxels"] / total) * total / (r[mode + "_ms"]["median"] * 1e-3)
            r[mode + "_share_of_copy_rate"] = r[mode + "_bytes_per_s"] / COPY_RATE
        res["voxel_%g" % voxel] = r
        print("voxel %g: %d voxels of %d points | default %.3f ms (%.3f .. %.3f) | deterministic %.3f ms (%.3f .. %.3f) | parent %.3f ms (%.3f .. %.3f)"
              % (voxel, r["voxels"], total, r["default_ms"]["median"], r["default_ms"]["min"], r["default_ms"]["max"], r["deterministic_ms"]["median"],
                 r["deterministic_ms"]["min"], r["deterministic_ms"]["max"], r["parent_ms"]["median"], r["parent_ms"]["min"], r["parent_ms"]["max"]), flush=True)
        print("        new / parent: default %.4f, deterministic %.4f | unavoidable bytes/s: default %.3g (%.1f %% of the copy rate), deterministic %.3g (%.1f %%)"
              % (r["default_over_parent"], r["deterministic_over_parent"], r["default_bytes_per_s"], 100 * r["default_share_of_copy_rate"],
                 r["deterministic_bytes_per_s"], 100 * r["deterministic_share_of_copy_rate"]), flush=True)
    res["allocations_at_end"] = {k: c.kf_export_voxel_allocations() for k, c in ctx.items()}
    assert res["allocations_at_end"] == res["allocations_after_reserve"]
    assert hip.hipFree(dx) == 0 and hip.hipFree(dc) == 0
    for c in ctx.values():
        c.close()
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
