"""Measurements of the loop-closure map rebuild for DESIGN.md section 14 (run on an MI355X): the resident path against the only way
the parent commit can do the same work, both timed in one process, alternating, after a warm-up; median and [min, max] of `reps`.
    python tools/loop_probe.py [reps=8] [out.json]
    python tools/loop_probe.py trace              # two loop closures at 20k points per scan for rocprofv3 --kernel-trace --stats
    python tools/loop_probe.py check-trace kernel_stats.csv   # one fixed insertion per batch: k_fix_accum_ord twice per closure
  scene   5 keyframes of ~50k kept points, k = 20 marginalised scans with full covariances, W = 10, 20k and 200k points per scan
  build   vba_loop_map_build (one gather, one insertion)          |  numpy transform + vba_map_reset + 5 vba_map_cut_voxel_fix
  update  vba_loop_update, window from the outgoing map's ring    |  numpy transform + k vba_map_cut_voxel_fix + W vba_map_cut_voxel
          (and with explicit host arrays for the window)          |  from host arrays + vba_map_recut
The parent's way CANNOT carry the covariances of the fixed points (vba_map_cut_voxel_fix has no covariance argument): it does less
work and ends in a different map.  The marginalised scans are host arrays on both sides (their upload is part of both figures).
Times are host clocks around calls that end in a device synchronise."""
import csv
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
import loop_oracle as lo

C = capi.C
K_BL, W = 20, 10


def med(t):
    t = np.array(t) * 1e3
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def show(name, d):
    print("%-34s median %9.3f ms [%9.3f, %9.3f]" % (name, d["median"], d["min"], d["max"]), flush=True)


def scene(n_pts):
    kfs = synth.make_keyframe_path(n_kf=5, scans_per_kf=5, n_pts=20000, scan_step=0.02)
    wl = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name="loop_probe%d" % n_pts, n_pts=n_pts, win_size=K_BL + W)
    s = synth.make_scans(wl)
    poses = synth.poses_flat(s["R0"], s["p0"])
    vars_ = [np.ascontiguousarray(synth.calc_body_var(p, wl.dept_err, wl.beam_err).reshape(-1, 9)) for p in s["points"]]
    return dataclasses.replace(wl, win_size=W), kfs, s["points"], vars_, poses


class Session:
    """one context with its store and loop map; the flat arrays of a loop_update are prepared once"""

    def __init__(self, wl, kfs, pts, vars_, poses, explicit):
        o = capi.options_from_workload(wl)
        o.max_points_per_scan = max(len(p) for p in pts)
        self.ctx = capi.Context(o)
        self.store = self.ctx.kf_store()
        for k, kf in enumerate(kfs):
            self.store.build(kf["points"], kf["poses"], 0.1, id=k, jour=0.0, vars=kf["vars"])
        self.lm = self.ctx.loop_map()
        ip = C.POINTER(C.c_int)
        self.off = np.zeros(K_BL + 1, np.int32); self.off[1:] = np.cumsum([len(p) for p in pts[:K_BL]])
        self.pnt = np.ascontiguousarray(np.concatenate(pts[:K_BL])); self.var = np.ascontiguousarray(np.concatenate(vars_[:K_BL]))
        self.bl_poses = np.ascontiguousarray(poses[:K_BL]); self.win_poses = np.ascontiguousarray(poses[K_BL:K_BL + W])
        self.woff = np.zeros(W + 1, np.int32); self.woff[1:] = np.cumsum([len(p) for p in pts[K_BL:K_BL + W]])
        self.wp = np.ascontiguousarray(np.concatenate(pts[K_BL:K_BL + W])); self.wv = np.ascontiguousarray(np.concatenate(vars_[K_BL:K_BL + W]))
        self.explicit = explicit
        self.args = (C.c_int(K_BL), self.off.ctypes.data_as(ip), capi._p(self.pnt), capi._p(self.var), capi._p(self.bl_poses), C.c_int(W),
                     capi._p(self.wp) if explicit else None, capi._p(self.wv) if explicit else None,
                     self.woff.ctypes.data_as(ip) if explicit else None, capi._p(self.win_poses))
        self.lm.reserve(fix_points=int(self.off[-1]) + 16 * 60000, nodes=1 << 21)
        for i in range(W):                                          # the window the first closure finds in the ring
            self.ctx.cut_voxel(i, pts[K_BL + i], poses[K_BL + i], var=vars_[K_BL + i])
        self.ctx.recut(W, self.win_poses, multi=False)

    def build(self):
        return self.lm.build(self.store, 5, True)

    def update(self):
        nf = C.c_int()
        self.ctx._chk(self.ctx.lib.vba_loop_update(self.ctx.h, self.lm.h, None, *self.args, C.byref(nf)))
        return nf.value

    def close(self):
        self.ctx.close()


def probe(n_pts, reps):
    wl, kfs, pts, vars_, poses = scene(n_pts)
    res, exp = Session(wl, kfs, pts, vars_, poses, False), Session(wl, kfs, pts, vars_, poses, True)
    par = capi.Context(res.ctx.opt)
    clouds = [res.store.read(k)[0] for k in range(5)]
    x0 = [res.store.get(k)["x0"] for k in range(5)]
    calls = lo.expansion(5, 5, True)
    t = dict(build=[], update_resident=[], update_explicit=[], parent_build=[], parent_update=[], parent_recut=[])
    nf = {}
    for r in range(reps + 2):
        t0 = time.perf_counter(); n_ins = res.build(); t1 = time.perf_counter(); nf["resident"] = res.update(); t2 = time.perf_counter()
        exp.build()
        t3 = time.perf_counter(); nf["explicit"] = exp.update(); t4 = time.perf_counter()
        # the parent's way, from host arrays, without covariances on the fixed points
        t5 = time.perf_counter()
        par.map_reset()
        for call in calls:
            par.cut_voxel_fix(np.concatenate([lo.world(x0[i], clouds[i]) for i in call]), 0.0)
        t6 = time.perf_counter()
        for i in range(K_BL):
            par.cut_voxel_fix(lo.world(poses[i], pts[i]), 0.0)
        for i in range(W):
            par.cut_voxel(i, pts[K_BL + i], poses[K_BL + i], var=vars_[K_BL + i])
        t7 = time.perf_counter()
        par.recut(W, res.win_poses, multi=False)
        t8 = time.perf_counter()
        nf["parent"] = par.size()
        if r >= 2:
            for k, v in (("build", t1 - t0), ("update_resident", t2 - t1), ("update_explicit", t4 - t3), ("parent_build", t6 - t5),
                         ("parent_update", t8 - t6), ("parent_recut", t8 - t7)):
                t[k].append(v)
    assert nf["resident"] == nf["explicit"]
    out = dict(points_per_scan=n_pts, k=K_BL, W=W, reps=reps, keyframe_points=[len(c) for c in clouds], points_inserted_by_build=n_ins,
               bl_points=int(res.off[-1]), window_points=int(res.woff[-1]), factors=nf, **{k: med(v) for k, v in t.items()})
    print("--- %d points per scan: build inserts %d points, %d marginalised points, %d window points, factors %s" %
          (n_pts, n_ins, out["bl_points"], out["window_points"], nf))
    for k in t:
        show(k, out[k])
    rt = out["build"]["median"] + out["update_resident"]["median"]; pt = out["parent_build"]["median"] + out["parent_update"]["median"]
    out["resident_over_parent"] = dict(build=out["build"]["median"] / out["parent_build"]["median"],
                                       update=out["update_resident"]["median"] / out["parent_update"]["median"], total=rt / pt)
    out["recut_share_of_update"] = out["parent_recut"]["median"] / out["update_resident"]["median"]
    print("resident / parent: build %.2f, update %.2f, both %.2f; the recut (timed in the parent's way, same leaves) is %.2f of vba_loop_update"
          % (out["resident_over_parent"]["build"], out["resident_over_parent"]["update"], out["resident_over_parent"]["total"],
             out["recut_share_of_update"]), flush=True)
    res.close(); exp.close(); par.close()
    return out


TRACE_CLOSURES = 2


def trace_session():
    wl, kfs, pts, vars_, poses = scene(20000)
    s = Session(wl, kfs, pts, vars_, poses, False)
    for _ in range(TRACE_CLOSURES):
        s.build(); s.update()
    print("trace session: %d loop closures" % TRACE_CLOSURES)
    s.close()


def check_trace(path):
    """one fixed insertion per batch: k_fix_accum_ord and k_loop_gather run once per build and once per update, k_fix_to_soa never"""
    calls = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        n = int(float(row.get("Calls") or row.get("Count") or 0))
        for k in ("k_fix_accum_ord", "k_loop_gather", "k_fix_to_soa"):
            if k in name:
                calls[k] = calls.get(k, 0) + n
    print("kernel calls in the trace:", calls)
    assert calls.get("k_fix_accum_ord", 0) == 2 * TRACE_CLOSURES, calls
    assert calls.get("k_loop_gather", 0) == 2 * TRACE_CLOSURES, calls
    assert calls.get("k_fix_to_soa", 0) == 0, calls
    print("OK")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace_session()
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] == "check-trace":
        check_trace(sys.argv[2])
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    out = [probe(20000, reps), probe(200000, reps)]
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)
    print("OK")
