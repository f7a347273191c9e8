"""Measurements of the prior-map odometry update for DESIGN.md section 27 (run on an MI355X), on the store and scan of
tools/surfel_reg_probe.py, in one process.
    python tools/surfel_odom_probe.py [out.json] [n_kf=200] [scans_per_kf=3] [n_pts=60000] [reps=5] [scan_points=200000]
Legs at voxel 0.2 and 0.5 (sigma 0.02, min_count 5) on a map built from the store, after vba_surfel_map_reserve and one warm-up round,
median of `reps` with the spread, host clocks around calls that end in their one wait:
  update_1/7    vba_odom_surfel_update_on_state of a scan_points-point device scan from a state 0.02 m / 0.2 degrees off with a
                prior of (0.01 rad)^2 / (0.1 m)^2, neighbors 1 and 7 (the clock includes vba_odom_state_set of the prior, which
                does not wait)
  today_7       what a user had before: vba_odom_state_get, vba_surfel_register (max_iter 4, neighbors 7), vba_odom_state_set of
                the registered pose (no fusion with the prior on the host is counted: the floor of that path)"""
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
from surfel_reg_probe import COUNTED, stats

C = capi.C
SIGMA, MIN_COUNT = 0.02, 5


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
    n_kf, spk, n_pts, reps, n_scan = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 200), (3, 3), (4, 60000), (5, 5), (6, 200000))]
    t0 = time.time()
    ctx = capi.Context(capi.default_options())
    store = ctx.kf_store()
    for k, kf in enumerate(synth.make_keyframe_path(n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, with_var=False)):
        store.build(kf["points"], kf["poses"], 0.05, id=k, jour=0.0)
    total = int(store.sizes().sum())
    print("store: %d keyframes, %d points resident (%.1f s to set up)" % (n_kf, total, time.time() - t0), flush=True)
    k0, pts = n_kf // 2, []
    x0 = store.get(k0)["x0"]; Rg, tg = x0[:9].reshape(3, 3), x0[9:12]
    k = k0
    while sum(len(p) for p in pts) < n_scan and k < n_kf:
        xk = store.get(k)["x0"]
        w = store.read(k)[0] @ xk[:9].reshape(3, 3).T + xk[9:12]
        pts.append((w - tg) @ Rg); k += 1
    scan = np.ascontiguousarray(np.concatenate(pts)[:n_scan])
    rng = np.random.default_rng(3)
    a = rng.normal(size=3); a *= np.deg2rad(0.2) / np.linalg.norm(a)
    b = rng.normal(size=3); b *= 0.02 / np.linalg.norm(b)
    from scipy.spatial.transform import Rotation
    R0, t0p = Rg @ Rotation.from_rotvec(a).as_matrix(), tg + b
    state = np.zeros(25); state[1:10] = R0.ravel(); state[10:13] = t0p; state[22:25] = [0, 0, -9.8]
    P = np.diag(np.repeat([1e-4, 1e-2, 1e-2, 1e-6, 1e-4], 3))
    hip = hip_runtime()
    d_scan = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_scan), C.c_size_t(scan.nbytes)) == 0
    assert hip.hipMemcpy(d_scan, scan.ctypes.data_as(C.c_void_p), C.c_size_t(scan.nbytes), C.c_int(1)) == 0
    res = dict(source_hash=source_hash(), n_kf=n_kf, points=total, scan_points=len(scan), reps=reps, sigma=SIGMA, min_count=MIN_COUNT,
               start=dict(metres=0.02, degrees=0.2), counted_bytes_per_point=COUNTED)
    st = ctx.odom_state()
    for voxel in (0.2, 0.5):
        kept = ctx.kf_export_surfel_size([store], [0.0], 1, voxel, MIN_COUNT)
        m = ctx.surfel_map()
        m.reserve(kept, len(scan))
        assert m.build_from_kf([store], 1, voxel, SIGMA, MIN_COUNT) == kept
        out = {}

        def update(nb):
            def f():
                st.set(state, P)
                ok, s, rep = st.surfel_update(m, d_scan, capi.surfel_odom_default_params(neighbors=nb), n=len(scan))
                out["update_%d" % nb] = dict(ok=ok, iterations=rep["iterations"], match_num=[int(x) for x in rep["match_num"]],
                                             dist_m=float(np.linalg.norm(s[10:13] - tg)), nnt_eig_min=rep["nnt_eig_min"])
            return f

        def today():
            st.set(state, P)
            s, c = st.get()
            R, t, rep = m.register(d_scan, s[1:10].reshape(3, 3), s[10:13], capi.surfel_reg_default_params(neighbors=7, max_iter=4), n=len(scan))
            s[1:10] = R.ravel(); s[10:13] = t
            st.set(s, c)
            ctx.synchronize()
            out["today_7"] = dict(iters=rep.iters, matches=list(rep.matches[:rep.iters]), dist_m=float(np.linalg.norm(t - tg)))

        legs = [("update_1", update(1)), ("update_7", update(7)), ("today_7", today)]
        t = {name: [] for name, _ in legs}
        base = None
        for rep in range(reps + 1):                              # round 0 is the warm-up
            for name, f in legs:
                a0 = time.perf_counter(); f(); b0 = time.perf_counter()
                if rep:
                    t[name].append((b0 - a0) * 1e3)
            if rep == 0:
                base = (m.allocations(), st.allocations(), ctx.kdtree_allocations())
        assert (m.allocations(), st.allocations(), ctx.kdtree_allocations()) == base
        r = dict(cells=kept, **out)
        for name, _ in legs:
            r[name + "_ms"] = stats(t[name])
        for nb in (1, 7):
            it = out["update_%d" % nb]["iterations"]
            us = r["update_%d_ms" % nb]["median"] * 1e3
            r["update_%d_ns_per_point_iteration" % nb] = us * 1e3 / (it * len(scan))
            r["update_%d_counted_GBps" % nb] = COUNTED[nb] * it * len(scan) / (us * 1e-6) / 1e9
        res["voxel_%g" % voxel] = r
        print("voxel %g: %d cells" % (voxel, kept))
        for name, _ in legs:
            print("    %-10s %10.3f ms (%.3f .. %.3f)  %s" % (name, r[name + "_ms"]["median"], r[name + "_ms"]["min"], r[name + "_ms"]["max"], out[name]), flush=True)
        m.close()
    st.close()
    assert hip.hipFree(d_scan) == 0
    ctx.close()
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
