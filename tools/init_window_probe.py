"""Measurements of the initialisation window for DESIGN.md section 19 (run on an MI355X): median of `reps` runs after a warm-up, host
clocks, every timed step complete when it returns.
    python tools/init_window_probe.py [out.json=profiles/init_window_probe.json] [reps=5] [parent.json]
    python tools/init_window_probe.py --motion-init-only out.json [reps=5] [libvoxelba.so]
    python tools/init_window_probe.py --ab parent/libvoxelba.so out.json [reps=5]
  (a) per scan   vba_init_window_push against the host route on the same commit: frame.read(0), vba_scan_down_sampling_close (with the
                 retry), the numpy gather in ascending index order, and the upload of the gathered rows (a push_points into a second
                 window: the bytes vba_motion_init would upload).  On a hesai-like message of 200 k raw points (26-byte records) and
                 on a 20 000-point scan of the synthetic room window (livox records).
  (b) per call   vba_motion_init_resident against vba_motion_init on the same 20 000-point window (W = 10), alternating, each on a
                 context of its own that is reused from call to call (the warm-up call allocates the map's storage; a fresh context per
                 call would time hipMalloc).
  (c)            vba_motion_init alone, for the comparison with the parent commit: --motion-init-only runs just that (it uses nothing
                 this feature added, so it also runs on the parent's library, given as the last argument); the full run repeats it and,
                 given the parent's JSON, records whether this commit's median lies inside the parent's own min-max spread.
                 --ab loads the parent's library beside this tree's in ONE process (two handles, a context each) and alternates the
                 calls, so that both see the same machine at the same time; that is the comparison DESIGN.md states."""
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
import init_window_oracle as iwo
import oracle_api
from prof_summary import source_hash  # noqa: E402

W = 10
NM = np.array([0.01] * 3 + [1.0] * 3)
NW = np.array([1e-4] * 6)
DOWN_SIZE, MIN_POINTS = 0.1, 1000


def med(t):
    t = np.array(t) * 1e3
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def window():
    wl = synth.Workload("init", W, 0.5, 0, "spin32", (10.0, 8.0, 3.0), 0, 0)
    d = synth.make_init_window(win_size=W, n_pts=20000, scene="room")
    ims = d["imus"]
    oracle_api.build()
    ip = np.stack([oracle_api.imu_preintegrate(ims[i][:, 0], ims[i][:, 1:4], ims[i][:, 4:7], np.zeros(3), np.zeros(3), NM, NW, d["scale_gravity"])
                   for i in range(1, W)])
    return wl, d, ip


def host_fed(ctx, wl, d, ip):
    ctx.synchronize()
    t1 = time.perf_counter()
    a = ctx.motion_init(d["clouds"], d["curvs"], d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err, d["scale_gravity"], NM, NW,
                        d["states"], d["covs"], ip, want_pvec=False)
    return time.perf_counter() - t1, a


def motion_init_only(reps, wl, d, ip):
    ctx = capi.Context(capi.options_from_workload(wl))
    ts = []
    for r in range(reps + 1):
        t, a = host_fed(ctx, wl, d, ip)
        ts.append(t)
    ctx.close()
    return dict(med(ts[1:]), iterations=a["iterations"], converged=a["converged"])


def per_scan(ctx, layout, msg, reps):
    frame, win, win_h = ctx.scan_frame(), ctx.init_window(), ctx.init_window()
    n, _ = frame.decode(layout, msg, 1, 0.0)
    win.reserve(reps + 2, n); win_h.reserve(reps + 2, n)
    ta, tb = [], []
    for r in range(reps + 1):
        t1 = time.perf_counter(); kept, retried = win.push(frame, DOWN_SIZE, MIN_POINTS); ta.append(time.perf_counter() - t1)
        t1 = time.perf_counter()
        s0 = frame.read(0)
        idx, _ = iwo.push(s0["pnt"], s0["curvature"], DOWN_SIZE, MIN_POINTS, ctx.down_sampling_close)
        win_h.push_points(s0["pnt"][idx], s0["curvature"][idx])
        tb.append(time.perf_counter() - t1)
        assert kept == len(idx)
    gp, gc = win.read(reps); hp, hc = win_h.read(reps)
    assert np.array_equal(gp, hp) and np.array_equal(gc, hc)
    frame.close(); win.close(); win_h.close()
    a, b = med(ta[1:]), med(tb[1:])
    return dict(decoded=n, kept=kept, retried=retried, push_ms=a, host_route_ms=b, host_over_push=b["median"] / a["median"])


def main():
    args = sys.argv[1:]
    if args and args[0] == "--motion-init-only":
        if len(args) > 3:
            capi.LIB_PATH = os.path.abspath(args[3])
        wl, d, ip = window()
        import hashlib
        # the hash of the sources describes this tree's own library only; a library given by path is named by its file's hash
        res = dict(source_hash=source_hash() if len(args) <= 3 else None, library_sha256=hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest(),
                   reps=int(args[2]) if len(args) > 2 else 5)
        res["motion_init_ms"] = motion_init_only(res["reps"], wl, d, ip)
        json.dump(res, open(args[1], "w"), indent=1)
        print(res["motion_init_ms"])
        return
    if args and args[0] == "--ab":
        import hashlib
        reps = int(args[3]) if len(args) > 3 else 5
        wl, d, ip = window()
        this_path = capi.LIB_PATH
        ctx_this = capi.Context(capi.options_from_workload(wl))
        capi._lib = None; capi.LIB_PATH = os.path.abspath(args[1])       # a second handle: Context keeps the library it was created with
        ctx_parent = capi.Context(capi.options_from_workload(wl))
        assert ctx_parent.lib is not ctx_this.lib and not hasattr(ctx_parent.lib, "vba_motion_init_resident")
        tp, tt = [], []
        for r in range(reps + 1):
            order = ((ctx_parent, tp), (ctx_this, tt)) if r % 2 == 0 else ((ctx_this, tt), (ctx_parent, tp))
            for c, t in order:
                t.append(host_fed(c, wl, d, ip)[0])
        a, b = med(tp[1:]), med(tt[1:])
        res = dict(source_hash=source_hash(), reps=reps, parent_library_sha256=hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest(),
                   this_library_sha256=hashlib.sha256(open(this_path, "rb").read()).hexdigest(), parent_ms=a, this_ms=b,
                   this_median_within_parent_spread=bool(b["median"] <= a["max"]))
        json.dump(res, open(args[2], "w"), indent=1)
        print("(c) one process, alternating: motion_init parent %.3f ms [%.3f, %.3f] | this %.3f ms [%.3f, %.3f] | inside the parent's spread: %s"
              % (a["median"], a["min"], a["max"], b["median"], b["min"], b["max"], res["this_median_within_parent_spread"]))
        return
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "init_window_probe.json")
    reps = int(args[1]) if len(args) > 1 else 5
    res = dict(source_hash=source_hash(), reps=reps, down_size=DOWN_SIZE, min_points=MIN_POINTS, win_size=W)
    wl, d, ip = window()

    # (a) per scan
    ctx = capi.Context(capi.options_from_workload(wl))
    hw = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name="initw", win_size=2)
    s = synth.make_scans(hw)
    pts = s["points"][1].astype(np.float32)
    rng = np.random.default_rng(9)
    hesai = capi.scan_layout("hesai")
    msg = do.make_message(hesai, pts, rng.uniform(0, 255, len(pts)), 1.7e9 + np.sort(rng.uniform(0.0, 0.1, len(pts))))
    res["scan_hesai200k"] = per_scan(ctx, hesai, msg, reps)
    livox = capi.scan_layout("livox")
    msg = do.make_message(livox, d["clouds"][0], np.zeros(len(d["clouds"][0]), dtype=np.uint8), np.round(d["curvs"][0] * 1e9).astype(np.uint32))
    res["scan_room20k"] = per_scan(ctx, livox, msg, reps)
    ctx.close()
    for k in ("scan_hesai200k", "scan_room20k"):
        r = res[k]
        print("(a) %s: %d decoded, %d kept | push %.3f ms [%.3f, %.3f] | host route %.3f ms [%.3f, %.3f] | host / push %.2f"
              % (k, r["decoded"], r["kept"], r["push_ms"]["median"], r["push_ms"]["min"], r["push_ms"]["max"], r["host_route_ms"]["median"],
                 r["host_route_ms"]["min"], r["host_route_ms"]["max"], r["host_over_push"]), flush=True)

    # (b) per call, alternating
    tr, th = [], []
    c, ch = capi.Context(capi.options_from_workload(wl)), capi.Context(capi.options_from_workload(wl))
    win = c.init_window()
    for i in range(W):
        win.push_points(d["clouds"][i], d["curvs"][i])
    for r in range(reps + 1):
        c.synchronize()
        t1 = time.perf_counter()
        b = c.motion_init_resident(win, d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err, d["scale_gravity"], NM, NW, d["states"],
                                   d["covs"], ip, want_pvec=False)
        tr.append(time.perf_counter() - t1)
        t, a = host_fed(ch, wl, d, ip)
        th.append(t)
        assert a["iterations"] == b["iterations"] and a["converged"] == b["converged"]
    c.close(); ch.close()
    res["call_room20k"] = dict(iterations=a["iterations"], converged=a["converged"], resident_ms=med(tr[1:]), host_fed_ms=med(th[1:]),
                               host_over_resident=float(np.median(th[1:]) / np.median(tr[1:])))
    r = res["call_room20k"]
    print("(b) W = %d x 20000 points, %d rounds: resident %.3f ms [%.3f, %.3f] | host-fed %.3f ms [%.3f, %.3f] | host-fed / resident %.3f"
          % (W, r["iterations"], r["resident_ms"]["median"], r["resident_ms"]["min"], r["resident_ms"]["max"], r["host_fed_ms"]["median"],
             r["host_fed_ms"]["min"], r["host_fed_ms"]["max"], r["host_over_resident"]), flush=True)

    # (c) the existing call against the parent commit
    res["motion_init_ms"] = motion_init_only(reps, wl, d, ip)
    if len(args) > 2:
        p = json.load(open(args[2]))
        pm = p["motion_init_ms"]
        res["parent"] = dict(library_sha256=p["library_sha256"], motion_init_ms=pm)
        res["motion_init_within_parent_spread"] = bool(res["motion_init_ms"]["median"] <= pm["max"])
        print("(c) motion_init %.3f ms [%.3f, %.3f] | parent %.3f ms [%.3f, %.3f] | inside the parent's spread: %s"
              % (res["motion_init_ms"]["median"], res["motion_init_ms"]["min"], res["motion_init_ms"]["max"], pm["median"], pm["min"], pm["max"],
                 res["motion_init_within_parent_spread"]), flush=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
