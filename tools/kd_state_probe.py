"""Measurement of the initialisation odometry on a resident state for DESIGN.md section 22 (run on an MI355X), with the set-up and the
protocol of tools/kd_probe.py: one 0.5 m down-sampled scan of the hesai200k_w10 scene against the point-cloud map that four such
scans leave, the same state and covariance for every call, the map put back (untimed) before every call.
    python tools/kd_state_probe.py [out.json=profiles/kd_state_probe.json] [reps=9]
    python tools/kd_state_probe.py --merge this.json out.json parent_a.json[,parent_b.json...] [kernel_trace_dir]
  (a) resident_dev      vba_odom_lio_state_estimation_kdtree_resident on a device pointer: the leg of kd_probe.py, untouched by §22
  (b) resident_get_set  vba_odom_state_get, (a) on what it returned, vba_odom_state_set with the result: the round trip a node on a
                        state object makes without the on-state call
  (c) on_state          vba_odom_lio_state_estimation_kdtree_on_state (the state set, untimed, before the call)
  (d) export_host       vba_odom_state_export_scan of the scan to a host array (one synchronise), after (c)'s set
The legs alternate in one process; their order rotates by one and reverses from one repetition to the next.  Host clocks; (a), (b),
(c) end in a wait of their own, (b)'s set is stream-ordered as it is in a node.  (c) must return (a)'s iterations and state bit for bit.
VBA_LIB=<a parent commit's libvoxelba.so> times that build: only (a) exists there.  --merge (no GPU work) adds to the record of this
build the parent's runs of the same visit, pooled over its processes (run them before and after this build's), states whether the
median of (a) on this build lies within the parent's own [min, max], and takes the durations of the new kernels from
kernel_trace_dir, the output directory of a `rocprofv3 --kernel-trace --stats --output-format csv` run of this probe."""
import ctypes as C
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
from odom_state_probe import kernel_ns  # noqa: E402
from prof_summary import source_hash  # noqa: E402

N_MAP_SCANS = 4


def merge(this_path, out_path, parent_paths, trace_dir):
    res = json.load(open(this_path))
    runs = []
    for p in parent_paths:
        runs += json.load(open(p))["resident_dev"]["runs_ms"]
    t = np.array(runs)
    res["parent_resident_dev"] = dict(processes=len(parent_paths), median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()),
                                      runs_ms=[float(x) for x in t])
    med = res["resident_dev"]["median_ms"]
    res["resident_dev_within_parent_range"] = bool(t.min() <= med <= t.max())
    print("resident_dev median %.4f ms, parent [%.4f, %.4f] over %d runs -> %s" % (med, t.min(), t.max(), len(t),
                                                                                 "within" if res["resident_dev_within_parent_range"] else "OUTSIDE"))
    if trace_dir:
        res["kernels"] = {k: kernel_ns(trace_dir, k) for k in ("k_odom_begin_kd_dev", "k_odom_state_export", "k_odom_commit_dev")}
        print("kernels:", res["kernels"])
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--merge":
        return merge(sys.argv[2], sys.argv[3], sys.argv[4].split(","), sys.argv[5] if len(sys.argv) > 5 else None)
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kd_state_probe.json")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    raw = C.CDLL(capi.LIB_PATH)                    # a parent build lacks the calls of §22: its table of prototypes is the shorter one
    for name in [k for k in capi.PROTOTYPES if not hasattr(raw, k)]:
        del capi.PROTOTYPES[name]
    have_on_state = "vba_odom_lio_state_estimation_kdtree_on_state" in capi.PROTOTYPES
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
    st = ctx.odom_state() if have_on_state else None
    print("scan of %d points, map of %d (%.1f s to set up)" % (n, m, time.time() - t0), flush=True)

    def restore():
        ctx._chk(ctx.lib.vba_odom_kdtree_reset(ctx.h))
        it, _, _, _ = ctx.lio_state_estimation_kdtree_resident(m, d_tree.data_ptr(), ident, cov)
        assert it == 0 and ctx.kdtree_size() == m
        if st is not None:
            st.set(state, cov)
        ctx.synchronize()

    def resident():
        it, x, cv, rep = ctx.lio_state_estimation_kdtree_resident(n, d_p.data_ptr(), state, cov)
        return it, x

    def resident_get_set():
        x0, cv0 = st.get()
        it, x, cv, rep = ctx.lio_state_estimation_kdtree_resident(n, d_p.data_ptr(), x0, cv0)
        st.set(x, cv)
        return it, x

    def on_state():
        it, rep, x = st.lio_state_estimation_kdtree(ctx, n, d_p.data_ptr())
        return it, x

    def export_host():
        return 0, st.export_scan(ctx, n, d_p.data_ptr(), 0.0)

    legs = [("resident_dev", resident)]
    if have_on_state:
        legs += [("resident_get_set", resident_get_set), ("on_state", on_state), ("export_host", export_host)]
    recs = {name: [] for name, _ in legs}
    out = {}
    for r in range(reps + 1):                      # round 0 is the warm-up
        k = r % len(legs)
        order = legs[k:] + legs[:k]
        for name, f in (order[::-1] if r % 2 else order):
            restore()
            t1 = time.perf_counter(); res = f(); dt = time.perf_counter() - t1
            out[name] = res
            if r:
                recs[name].append(dt * 1e3)
    res = dict(source_hash=source_hash(), library=os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH),
               workload=wl.name, points=n, map_points=m, reps=reps, iterations=int(out["resident_dev"][0]))
    if have_on_state:
        for name in ("resident_get_set", "on_state"):
            assert out[name][0] == out["resident_dev"][0] and np.array_equal(out[name][1], out["resident_dev"][1]), name
        res["on_state_equals_resident_bit_for_bit"] = True
    for name, _ in legs:
        t = np.array(recs[name])
        res[name] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), runs_ms=[float(x) for x in t])
        print("%-17s median %.3f ms (min %.3f, max %.3f)" % (name, np.median(t), t.min(), t.max()), flush=True)
    if have_on_state:
        res["on_state_minus_resident_get_set_ms"] = res["on_state"]["median_ms"] - res["resident_get_set"]["median_ms"]
        res["on_state_minus_resident_dev_ms"] = res["on_state"]["median_ms"] - res["resident_dev"]["median_ms"]
    ctx.close()
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
