"""Measurements of the keyframe store for DESIGN.md section 13 (run on an MI355X): each resident path against the parent's way of
doing the same work on the same inputs, both timed in one process, alternating, after a warm-up; median and spread of `reps` runs.
    python tools/kf_probe.py [reps=12] [hba_keyframes=1000] [out.json]
    python tools/kf_probe.py trace        # a short session of builds, window generations and loads for rocprofv3 --kernel-trace --stats
  build   10 x 20k points: vba_kf_build with a database  |  host merge + vba_scan_down_sampling_pvec + vba_btc_generate_stds (host arrays)
  load    one keyframe of ~50k points: vba_kf_load       |  host transform + vba_map_cut_voxel_fix (host array)
  hba     vba_hba_global over hba_keyframes x ~50k points: the store's pointer  |  the same call on a host array
Times are host clocks around calls that end in a device synchronise."""
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
import kf_oracle as ko

C = capi.C
VS10 = 0.05
GBA = dict(gba_voxel_size=2.0, gba_min_eigen_value=0.1, gba_eig=[0.25, 0.25, 0.25, 0.25])


def stats(name, a, b, what_a="resident", what_b="parent"):
    a, b = np.array(a) * 1e3, np.array(b) * 1e3
    r = dict(name=name, reps=len(a),
             **{what_a + "_ms": dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max())),
                what_b + "_ms": dict(median=float(np.median(b)), min=float(b.min()), max=float(b.max()))},
             ratio_parent_over_resident=float(np.median(b) / np.median(a)))
    print("%-6s %s median %.3f ms [%.3f, %.3f] | %s median %.3f ms [%.3f, %.3f] | parent / resident %.2f"
          % (name, what_a, np.median(a), a.min(), a.max(), what_b, np.median(b), b.min(), b.max(), r["ratio_parent_over_resident"]), flush=True)
    return r


def make_db(ctx):
    db = ctx.btc_db(capi.btc_default_config(0))
    db.set_gen_config(capi.btc_default_gen_config(0))
    return db


def probe_build(reps):
    kf = synth.make_keyframe_path(n_kf=1, scans_per_kf=10, n_pts=20000, scan_step=0.02)[0]
    n = sum(len(p) for p in kf["points"])
    var = np.concatenate(kf["vars"]); pnt = np.concatenate(kf["points"])
    off = np.zeros(11, np.int32); off[1:] = np.cumsum([len(p) for p in kf["points"]])
    ctx = capi.Context(capi.default_options())
    store = ctx.kf_store(); db_a, db_b = make_db(ctx), make_db(ctx)
    store.reserve(points=(reps + 4) * n, keyframes=reps + 4, merge_points=n)
    for db in (db_a, db_b):
        db.gen_reserve(points=n, cells=1 << 22, frames=reps + 4)

    def resident():
        store.build(pnt, kf["poses"], VS10, id=1, jour=0.0, vars=var, db=db_a, offsets=off)

    def parent():
        m = ko.merge(kf["points"], kf["poses"])                       # the host merge of VS:2357-2371
        ctx.down_sampling_pvec(m, var, VS10)
        db_b.generate_stds(m.astype(np.float32), 1)

    ta, tb = [], []
    for r in range(reps + 2):
        for f, t in ((resident, ta), (parent, tb)):
            t0 = time.perf_counter(); f(); dt = time.perf_counter() - t0
            if r >= 2:
                t.append(dt)
    out = stats("build", ta, tb)
    out["points_merged"] = n
    ctx.close()
    return out


def probe_load(reps):
    kf = synth.make_keyframe_path(n_kf=1, scans_per_kf=5, n_pts=20000, scan_step=0.02)[0]
    wl = synth.CONFIGS["hesai200k_w10"]
    o = capi.options_from_workload(wl); o.max_map_nodes = 1 << 20; o.max_fix_points = 1 << 22
    ctx_a, ctx_b = capi.Context(o), capi.Context(o)
    store = ctx_a.kf_store()
    n, _, _ = store.build(kf["points"], kf["poses"], 0.1, id=0, jour=0.0, vars=kf["vars"])
    xyz, _ = store.read(0)
    x0 = store.get(0)["x0"]

    def resident():
        store.load(0, ctx_a, 1.0)

    def parent():
        ctx_b.cut_voxel_fix(ko.world(x0, xyz), 1.0)                   # the host transform of VS:1418-1427, then the upload

    ta, tb = [], []
    for r in range(reps + 2):
        for f, t, c in ((resident, ta, ctx_a), (parent, tb, ctx_b)):
            c.map_reset(); c.synchronize()
            t0 = time.perf_counter(); f(); dt = time.perf_counter() - t0
            if r >= 2:
                t.append(dt)
    out = stats("load", ta, tb)
    out["points"] = n
    ctx_a.close(); ctx_b.close()
    return out


def probe_hba(reps, nkf):
    BLK = 200
    wl = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name="kf_hba", win_size=min(BLK, nkf), n_pts=50000)
    t0 = time.time()
    s = synth.make_scans(wl)
    x0b = synth.poses_flat(s["R0"], s["p0"])
    ctx = capi.Context(capi.options_from_workload(dataclasses.replace(wl, win_size=10)))
    store = ctx.kf_store()
    store.reserve(points=nkf * 50000, keyframes=nkf, merge_points=50000)
    # blocks of 200 keyframes over the same path (the straight synthetic trajectory leaves the hall after ~250)
    x0 = []
    for k in range(nkf):
        j = k % len(s["points"])
        store.build([s["points"][j]], x0b[j][None, :], 0.001, id=k, jour=0.0)      # 1 mm voxels: nearly every point is kept
        x0.append(x0b[j])
    x0 = np.array(x0)
    d, off, n_kf = store.clouds()
    host = np.concatenate([store.read(k)[0] for k in range(nkf)])
    print("hba scene: %d keyframes, %.1f M points resident (%.1f s to set up)" % (nkf, off[-1] / 1e6, time.time() - t0), flush=True)
    nwin = (nkf - 10) // 5 + 1
    cap1 = nwin * 45 + 1; cap2 = nwin * (nwin - 1) // 2 + 1
    e1 = np.zeros((cap1, 20)); e2 = np.zeros((cap2, 20)); n1 = C.c_int(); n2 = C.c_int()
    res = {}

    def call(pnt_arg, key):
        ctx._chk(ctx.lib.vba_hba_global(ctx.h, C.c_int(nkf), off.ctypes.data_as(C.POINTER(C.c_int)), pnt_arg, capi._p(x0), capi._p(x0),
                                        C.c_double(GBA["gba_voxel_size"]), C.c_double(GBA["gba_min_eigen_value"]), capi._p(capi._c(GBA["gba_eig"])),
                                        C.c_int(2), C.c_int(10), C.c_int(5), capi._p(e1), C.c_int(cap1), C.byref(n1), capi._p(e2), C.c_int(cap2),
                                        C.byref(n2)))
        res[key] = (e1[:n1.value].copy(), e2[:n2.value].copy())

    ta, tb = [], []
    for r in range(reps + 1):
        for arg, key, t in ((C.c_void_p(d), "resident", ta), (capi._p(host), "parent", tb)):
            t0 = time.perf_counter(); call(arg, key); dt = time.perf_counter() - t0
            if r >= 1:
                t.append(dt)
    a, b = res["resident"], res["parent"]
    assert len(a[0]) == len(b[0]) == nwin * 45 and np.array_equal(a[0][:, :2], b[0][:, :2])
    print("hba: bottom-layer relative poses from the store and from the host array differ by <= %.2e" % np.abs(a[0][:, 2:14] - b[0][:, 2:14]).max())
    out = stats("hba", ta, tb)
    out.update(keyframes=nkf, points=int(off[-1]), cloud_bytes=int(off[-1]) * 24)
    ctx.close()
    return out


def trace_session():
    """what rocprofv3 --kernel-trace --stats should see: builds with descriptors at 10 x 20k, window generations, loads"""
    kfs = synth.make_keyframe_path(n_kf=6, scans_per_kf=10, n_pts=20000, scan_step=0.02)
    ctx = capi.Context(capi.options_from_workload(synth.CONFIGS["hesai200k_w10"]))
    store = ctx.kf_store(); db = make_db(ctx)
    for rep in range(3):
        for k, kf in enumerate(kfs):
            store.build(kf["points"], kf["poses"], VS10, id=k, jour=0.0, vars=kf["vars"], db=db)
    for f in range(0, 12, 3):
        store.generate_stds(f, 3, db)
    for k in range(12):
        store.load(k, ctx, 1.0)
    print("trace session: %d keyframes, %d points resident" % (store.size(), store.clouds()[1][-1]))
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace_session()
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    nkf = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    out = [probe_build(reps), probe_load(reps)]
    if nkf >= 10:
        out.append(probe_hba(max(reps, 10), nkf))
    if len(sys.argv) > 3:
        json.dump(out, open(sys.argv[3], "w"), indent=1)
    print("OK")
