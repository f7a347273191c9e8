"""Measurements of the scan front end for DESIGN.md section 16 (run on an MI355X): one synthetic 26-byte-step message of 230 400
records (the Hesai record: f64 time at offset 16, unaligned), point_filter_num 1 and 3, 21 IMU poses, against a map that a short
local-mapping session built; median of `reps` runs after a warm-up, each step ended by a device synchronise, host clocks.
    python tools/frontend_probe.py [out.json=profiles/frontend_probe.json] [n_raw=230400] [reps=5]
  (a) decode   vba_scan_decode (upload, decode + filter, sort, cut)
  (b) device   vba_scan_prepare, then the odometry and the insertion on the device pointers it returns
  (c) parent   the same decoded cloud from HOST arrays through the three stand-alone calls (undistort, down_sampling_voxel with the
               retry, var_init), then the odometry and the insertion from host arrays: what a node could do before the frame existed
(b) and (c) alternate; the map is rebuilt (untimed) before each of them, so both insert into the same map."""
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

DOWN_SIZE, MIN_POINTS, BLIND2 = 0.1, 500, 0.25


def imu_poses(m, rng, t_end):
    from scipy.spatial.transform import Rotation
    out = np.zeros((m, 22))
    out[:, 0] = np.linspace(0.0, t_end, m, endpoint=False)
    for j in range(m):
        out[j, 1:10] = Rotation.from_rotvec(rng.normal(0, 0.002, 3)).as_matrix().ravel()
        out[j, 10:13] = rng.normal(0, 0.005, 3); out[j, 13:16] = rng.normal(0, 0.3, 3)
        out[j, 16:19] = rng.normal(0, 0.05, 3); out[j, 19:22] = rng.normal(0, 0.3, 3)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frontend_probe.json")
    n_raw, reps = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 230400), (3, 5))]
    wl = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name="frontend", n_pts=n_raw, win_size=4)
    W, nscan = wl.win_size, 6
    t0 = time.time()
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    rng = np.random.default_rng(9)
    ctx = capi.Context(capi.options_from_workload(wl))
    frame = ctx.scan_frame()
    frame.reserve(n_raw, 26)
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    end = ext.copy()
    ip = imu_poses(21, rng, 0.1)
    layout = capi.scan_layout("hesai")
    k = nscan - 1
    pts = s["points"][k].astype(np.float32)
    msg = do.make_message(layout, pts, rng.uniform(0, 255, len(pts)), 1.7e9 + np.sort(rng.uniform(0.0, 0.1, len(pts))))
    state = np.zeros(25)
    state[1:10] = s["R_gt"][k].ravel(); state[10:13] = s["p_gt"][k] + rng.normal(0, 0.02, 3); state[22:25] = [0, 0, -9.8]
    cov = np.eye(15) * 1e-4; cov[9:, 9:] = np.eye(6) * 1e-5
    var0 = [np.tile((np.eye(3) * 1e-4).ravel(), (len(s["points"][j]), 1)) for j in range(nscan - 1)]

    def build_map():                                              # untimed: the local-mapping session that the scan meets
        ctx.map_reset()
        xs, wc = [], 0
        for j in range(nscan - 1):
            xs.append(synth.poses_flat(s["R_gt"][j:j + 1], s["p_gt"][j:j + 1])[0])
            wc += 1
            ctx.cut_voxel(wc - 1, s["points"][j], xs[-1], var=var0[j], multi=True)
            ctx.recut(wc, np.array(xs), multi=True)
            if wc >= W:
                ctx.margi(wc, np.array(xs), jour=float(j))
                ctx.slide(1); xs = xs[1:]; wc -= 1
        ctx.synchronize()
        return wc

    print("%d rays per scan, %d scans (%.1f s to set up)" % (n_raw, nscan, time.time() - t0), flush=True)
    res = dict(source_hash=source_hash(), n_raw=n_raw, point_step=layout.point_step, reps=reps, down_size=DOWN_SIZE, imu_poses=len(ip))

    def med(t):
        t = np.array(t) * 1e3
        return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))

    for pfn in (1, 3):
        ta = []
        for r in range(reps + 1):
            t1 = time.perf_counter(); n, last = frame.decode(layout, msg, pfn, BLIND2); ta.append(time.perf_counter() - t1)
        s0 = frame.read(0)
        want = do.decode(layout, msg, pfn, BLIND2)
        assert n == want["n"] and np.array_equal(s0["pnt"].astype(np.float32), want["pnt"])
        pose = np.concatenate([state[1:10], state[10:13]])

        def device(wc):
            m, dp, dv = frame.prepare(ip, end, ext, DOWN_SIZE, wl.dept_err, wl.beam_err, min_points=MIN_POINTS)
            ok, st, cv = ctx.lio_state_estimation_dev(m, dp, dv, state, cov)
            ctx.pvec_update_cut_voxel_dev(wc, m, dp, dv, pose, cv, multi=True)
            ctx.synchronize()
            return m, st

        def parent(wc):
            und = ctx.undistort(s0["pnt"], s0["curvature"], ip, end, ext)
            pd, cnt, first = ctx.down_sampling_voxel(und, DOWN_SIZE)
            if len(pd) < MIN_POINTS:
                pd, cnt, first = ctx.down_sampling_voxel(und, DOWN_SIZE / 2)
            pb, vb = ctx.var_init(pd, ext, wl.dept_err, wl.beam_err)
            ok, st, cv = ctx.lio_state_estimation(pb, vb, state, cov)
            ctx.pvec_update_cut_voxel(wc, pb, vb, pose, cv, multi=True)
            ctx.synchronize()
            return len(pd), st

        tb, tc = [], []
        for r in range(reps + 1):
            for f, t in ((device, tb), (parent, tc)):
                wc = build_map()
                t1 = time.perf_counter(); m, st = f(wc); t.append(time.perf_counter() - t1)
                t[-1] = (t[-1], m, float(np.abs(st - state).max()))
        assert tb[-1][1] == tc[-1][1], (tb[-1], tc[-1])
        a, b, c = med(ta[1:]), med([x[0] for x in tb[1:]]), med([x[0] for x in tc[1:]])
        res["pfn%d" % pfn] = dict(decoded=n, prepared=tb[-1][1], state_moved=tb[-1][2], decode_ms=a, device_ms=b, parent_ms=c,
                                  parent_over_device=c["median"] / b["median"])
        print("point_filter_num %d: %d decoded, %d prepared | (a) decode %.3f ms | (b) device %.3f ms | (c) parent %.3f ms | parent / device %.2f"
              % (pfn, n, tb[-1][1], a["median"], b["median"], c["median"], c["median"] / b["median"]), flush=True)
    frame.close(); ctx.close()
    json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
