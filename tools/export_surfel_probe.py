"""Measurements of the surfel export of the global map for DESIGN.md section 25 (run on an MI355X): vba_kf_surfel_export against
vba_kf_voxel_export and against what a node could do before it, on the store of tools/export_probe.py, in one process.
    python tools/export_surfel_probe.py [out.json] [n_kf=200] [scans_per_kf=3] [n_pts=60000] [reps=5] [min_count=3]
Legs, alternating after one warm-up round, median of `reps` with the spread, at voxel 0.1 and 0.2, jump 1:
  surfel   vba_kf_surfel_export into device buffers (records, cov, counts), on a default and on a deterministic context (timed with
           its one wait and to the end of the stream's work)
  voxel    vba_kf_voxel_export into device buffers on the same two contexts: the yardstick, the same front half
  host     vba_kf_export_world to host memory, then a host fit in numpy: voxel keys, groups by sorting, two-pass centred moments,
           a batched symmetric eigen-solve of the kept voxels
The reserve is sized by a size query; nothing may be allocated after it.  Times are host clocks."""
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
from export_probe import hip_runtime
from prof_summary import source_hash  # noqa: E402

C = capi.C


def context(det):
    o = capi.default_options()
    o.deterministic = det
    return capi.Context(o)


def host_fit(S, voxel, min_count):
    """(records [m][12] float32, cov [m][6]) of the kept voxels from the exported records: what a node would write in numpy"""
    a = S[:, :3].astype(np.float64)
    loc = (a / voxel).astype(np.float32)
    loc = np.where(loc < 0, loc - np.float32(1.0), loc).astype(np.int64)
    key = ((loc[:, 0] & 0x1FFFFF) << 42) | ((loc[:, 1] & 0x1FFFFF) << 21) | (loc[:, 2] & 0x1FFFFF)
    _, first, inv, cnt = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    nv = len(cnt)
    c = np.stack([np.bincount(inv, weights=a[:, k], minlength=nv) for k in range(3)], axis=1) / cnt[:, None]
    d = a - c[inv]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov = np.stack([np.bincount(inv, weights=d[:, i] * d[:, j], minlength=nv) for i, j in pairs], axis=1) / cnt[:, None]
    keep = np.flatnonzero(cnt >= min_count)
    keep = keep[np.argsort(first[keep], kind="stable")]         # first-occurrence order
    cov, c, cnt = cov[keep], c[keep], cnt[keep]
    A = np.empty((len(keep), 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2] = cov.T
    A[:, 1, 0], A[:, 2, 0], A[:, 2, 1] = A[:, 0, 1], A[:, 0, 2], A[:, 1, 2]
    w, V = np.linalg.eigh(A)
    w = np.maximum(w, 0.0)
    tr = w.sum(axis=1)
    rec = np.concatenate([c, S[first[keep], 3:4], V[:, :, 0], np.sqrt(w), (w[:, 0] / np.where(tr > 0, tr, 1.0))[:, None], cnt[:, None]], axis=1)
    return rec.astype(np.float32), cov


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n_kf, spk, n_pts, reps, min_count = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 200), (3, 3), (4, 60000), (5, 5), (6, 3))]
    t0 = time.time()
    ctx = {"default": context(0), "deterministic": context(1)}
    store = ctx["default"].kf_store()
    for k, kf in enumerate(synth.make_keyframe_path(n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, with_var=False)):
        store.build(kf["points"], kf["poses"], 0.05, id=k, jour=0.0)
        if k % 20 == 19:
            print("  %d keyframes built (%.1f s)" % (k + 1, time.time() - t0), flush=True)
    total = int(store.sizes().sum())
    print("store: %d keyframes of %d x %d rays, %d points resident (%.1f s to set up)" % (n_kf, spk, n_pts, total, time.time() - t0), flush=True)
    res = dict(source_hash=source_hash(), n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, points=total, reps=reps, min_count=min_count)
    voxels = (0.1, 0.2)
    scout = context(0)                                        # the size query grows a context's arrays: not one of the measured two
    kept_max = max(scout.kf_export_surfel_size([store], [0.0], 1, v, min_count) for v in voxels)
    scout.close()
    hip = hip_runtime()
    dx, dv, dc = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for d, b in ((dx, 48), (dv, 48), (dc, 4)):
        assert hip.hipMalloc(C.byref(d), C.c_size_t(b * max(kept_max, 1))) == 0
    for c in ctx.values():
        c.kf_export_surfel_reserve(total, kept_max)
    res["reserved_voxels"] = kept_max
    res["allocations_after_reserve"] = {k: c.kf_export_surfel_allocations() for k, c in ctx.items()}
    res["voxel_export_allocations_after_reserve"] = {k: c.kf_export_voxel_allocations() for k, c in ctx.items()}

    for voxel in voxels:
        kept = {}

        def surfel(mode):
            kept["surfel_" + mode] = ctx[mode].kf_export_surfel([store], [0.0], 1, voxel, min_count, cap=kept_max, out=(dx, dv, dc))
            ctx[mode].synchronize()

        def vox(mode):
            kept["voxel_" + mode] = ctx[mode].kf_export_voxel([store], [0.0], 1, voxel, min_count, cap=kept_max, out=(dx, dc))
            ctx[mode].synchronize()

        def host():
            S = ctx["default"].kf_export_world([store], [0.0], 1)
            rec, _ = host_fit(S, voxel, min_count)
            kept["host"] = len(rec)

        legs = [("surfel_default", lambda: surfel("default")), ("voxel_default", lambda: vox("default")),
                ("surfel_deterministic", lambda: surfel("deterministic")), ("voxel_deterministic", lambda: vox("deterministic")), ("host", host)]
        t = {name: [] for name, _ in legs}
        for rep in range(reps + 1):                           # round 0 is the warm-up
            for name, f in legs:
                a = time.perf_counter(); f(); b = time.perf_counter()
                if rep:
                    t[name].append((b - a) * 1e3)
            print("  voxel %g round %d done (%.1f s)" % (voxel, rep, time.time() - t0), flush=True)
        assert len(set(kept.values())) == 1, kept
        r = dict(voxels=kept["host"])
        for name, _ in legs:
            v = np.array(t[name])
            r[name + "_ms"] = dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))
        for mode in ("default", "deterministic"):
            r["surfel_%s_over_host" % mode] = r["surfel_%s_ms" % mode]["median"] / r["host_ms"]["median"]
            r["surfel_%s_over_voxel" % mode] = r["surfel_%s_ms" % mode]["median"] / r["voxel_%s_ms" % mode]["median"]
            r["surfel_%s_minus_voxel_ms" % mode] = r["surfel_%s_ms" % mode]["median"] - r["voxel_%s_ms" % mode]["median"]
        res["voxel_%g" % voxel] = r
        print("voxel %g: %d surfels of %d points" % (voxel, r["voxels"], total))
        for name, _ in legs:
            print("    %-22s %10.3f ms (%.3f .. %.3f)" % (name, r[name + "_ms"]["median"], r[name + "_ms"]["min"], r[name + "_ms"]["max"]), flush=True)
        print("    surfel / host: default %.5f, deterministic %.5f | surfel / voxel: default %.3f, deterministic %.3f"
              % (r["surfel_default_over_host"], r["surfel_deterministic_over_host"], r["surfel_default_over_voxel"], r["surfel_deterministic_over_voxel"]), flush=True)
    res["allocations_at_end"] = {k: c.kf_export_surfel_allocations() for k, c in ctx.items()}
    assert res["allocations_at_end"] == res["allocations_after_reserve"]
    assert hip.hipFree(dx) == 0 and hip.hipFree(dv) == 0 and hip.hipFree(dc) == 0
    for c in ctx.values():
        c.close()
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
