"""Measurements of the surfel map and of the registration against it for DESIGN.md section 26 (run on an MI355X), on the store of
tools/export_probe.py, in one process.
    python tools/surfel_reg_probe.py [out.json] [n_kf=200] [scans_per_kf=3] [n_pts=60000] [reps=5] [scan_points=200000] [once=0]
Legs at voxel 0.2 and 0.5 (sigma 0.02, min_count 5), after one warm-up round, median of `reps` with the spread, host clocks around
calls that end in their one wait:
  build_kf      vba_surfel_map_build_from_kf from the store (the export into the map's arrays, then the table)
  build_dev     vba_surfel_map_build from device arrays of a surfel export made before the clock starts
  register_1/7  vba_surfel_register of a scan_points-point device scan (points of consecutive keyframes in the first one's frame) from a
                start 0.05 m / 0.5 degrees off, neighbors 1 and 7
  host          the composition a node had before: vba_kf_surfel_export to host memory, then tests/host/surfreg_host.cpp (g++ -O2) on the
                same records, scan and start, neighbors 7 (its time includes reading and writing its files)
once=1 runs every device leg once and nothing else: the form to put under rocprofv3 --kernel-trace --stats."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
from export_probe import hip_runtime
from prof_summary import source_hash  # noqa: E402

C = capi.C
SIGMA, MIN_COUNT = 0.02, 5
# counted bytes of one iteration: 24 of the point; per candidate one 16-byte slot probe (a 64-byte line, 1.0 to 1.3
# probes at a load of 1/4 to 1/2) and on a hit the cell's 64-byte line
COUNTED = {1: 24 + 64 + 64, 7: 24 + 7 * 64 + 3 * 64}


def stats(v):
    v = np.array(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
    n_kf, spk, n_pts, reps, n_scan, once = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 200), (3, 3), (4, 60000), (5, 5), (6, 200000), (7, 0))]
    t0 = time.time()
    ctx = capi.Context(capi.default_options())
    store = ctx.kf_store()
    for k, kf in enumerate(synth.make_keyframe_path(n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, with_var=False)):
        store.build(kf["points"], kf["poses"], 0.05, id=k, jour=0.0)
    total = int(store.sizes().sum())
    print("store: %d keyframes, %d points resident (%.1f s to set up)" % (n_kf, total, time.time() - t0), flush=True)
    # the scan: keyframes k0, k0 + 1, ... in the frame of k0, cut at n_scan points
    k0, pts = n_kf // 2, []
    x0 = store.get(k0)["x0"]; Rg, tg = x0[:9].reshape(3, 3), x0[9:12]
    k = k0
    while sum(len(p) for p in pts) < n_scan and k < n_kf:
        xk = store.get(k)["x0"]
        w = store.read(k)[0] @ xk[:9].reshape(3, 3).T + xk[9:12]
        pts.append((w - tg) @ Rg); k += 1
    scan = np.ascontiguousarray(np.concatenate(pts)[:n_scan])
    rng = np.random.default_rng(3)
    a = rng.normal(size=3); a *= np.deg2rad(0.5) / np.linalg.norm(a)
    b = rng.normal(size=3); b *= 0.05 / np.linalg.norm(b)
    from scipy.spatial.transform import Rotation
    R0, t0p = Rg @ Rotation.from_rotvec(a).as_matrix(), tg + b
    hip = hip_runtime()
    d_scan = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_scan), C.c_size_t(scan.nbytes)) == 0
    assert hip.hipMemcpy(d_scan, scan.ctypes.data_as(C.c_void_p), C.c_size_t(scan.nbytes), C.c_int(1)) == 0
    res = dict(source_hash=source_hash(), n_kf=n_kf, points=total, scan_points=len(scan), reps=reps, sigma=SIGMA, min_count=MIN_COUNT, counted_bytes_per_point=COUNTED)
    exe = None
    if not once:
        exe = os.path.join(tempfile.mkdtemp(), "surfreg_host")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "surfreg_host.cpp"), "-o", exe])
        import surfreg_ref as rr
    for voxel in (0.2, 0.5):
        kept = ctx.kf_export_surfel_size([store], [0.0], 1, voxel, MIN_COUNT)
        dx, dv = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(dx), C.c_size_t(48 * kept)) == 0 and hip.hipMalloc(C.byref(dv), C.c_size_t(48 * kept)) == 0
        assert ctx.kf_export_surfel([store], [0.0], 1, voxel, MIN_COUNT, cap=kept, out=(dx, dv, None)) == kept
        ctx.synchronize()
        m_kf, m_dev = ctx.surfel_map(), ctx.surfel_map()
        for m in (m_kf, m_dev):
            m.reserve(kept, len(scan))
        base = (m_kf.allocations(), m_dev.allocations())
        out = {}

        def build_kf():
            out["cells_kf"] = m_kf.build_from_kf([store], 1, voxel, SIGMA, MIN_COUNT)

        def build_dev():
            out["cells_dev"] = m_dev.build(dx, dv, voxel, SIGMA, MIN_COUNT, n=kept)

        def register(nb):
            def f():
                R, t, rep = m_dev.register(d_scan, R0, t0p, capi.surfel_reg_default_params(neighbors=nb), n=len(scan))
                out["reg_%d" % nb] = dict(iters=rep.iters, converged=rep.converged, lost=rep.lost, matches=list(rep.matches[:rep.iters]),
                                          dist_m=float(np.linalg.norm(t - tg)), eig_tt=list(rep.eig_tt))
            return f

        def host():
            rec, cov, _ = ctx.kf_export_surfel([store], [0.0], 1, voxel, MIN_COUNT, cap=kept)
            h = rr.host_run(exe, os.path.dirname(exe), rec, cov, scan, R0, t0p, voxel, sigma=SIGMA, min_count=MIN_COUNT, neighbors=7, max_iter=30, tag="probe")
            out["host"] = dict(iters=h["iters"], converged=h["converged"], dist_m=float(np.linalg.norm(h["t"] - tg)))

        legs = [("build_kf", build_kf), ("build_dev", build_dev), ("register_1", register(1)), ("register_7", register(7))]
        if not once:
            legs.append(("host", host))
        t = {name: [] for name, _ in legs}
        for rep in range(1 if once else reps + 1):            # round 0 is the warm-up
            for name, f in legs:
                a0 = time.perf_counter(); f(); b0 = time.perf_counter()
                if rep or once:
                    t[name].append((b0 - a0) * 1e3)
        assert out["cells_kf"] == out["cells_dev"] == kept and (m_kf.allocations(), m_dev.allocations()) == base
        r = dict(cells=kept, slots=m_dev.read()["slots"] if kept < 4_000_000 else None, **out)
        for name, _ in legs:
            r[name + "_ms"] = stats(t[name])
        for nb in (1, 7):
            it = out["reg_%d" % nb]["iters"]
            us = r["register_%d_ms" % nb]["median"] * 1e3
            r["register_%d_ns_per_point_iteration" % nb] = us * 1e3 / (it * len(scan))
            r["register_%d_counted_GBps" % nb] = COUNTED[nb] * it * len(scan) / (us * 1e-6) / 1e9
        res["voxel_%g" % voxel] = r
        print("voxel %g: %d cells" % (voxel, kept))
        for name, _ in legs:
            print("    %-12s %10.3f ms (%.3f .. %.3f)" % (name, r[name + "_ms"]["median"], r[name + "_ms"]["min"], r[name + "_ms"]["max"]), flush=True)
        for nb in (1, 7):
            print("    register_%d: %s; %.2f ns per point and iteration, %.0f GB/s of counted bytes"
                  % (nb, out["reg_%d" % nb], r["register_%d_ns_per_point_iteration" % nb], r["register_%d_counted_GBps" % nb]), flush=True)
        if not once:
            print("    host: %s" % out["host"], flush=True)
        m_kf.close(); m_dev.close()
        assert hip.hipFree(dx) == 0 and hip.hipFree(dv) == 0
    assert hip.hipFree(d_scan) == 0
    ctx.close()
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
