"""Times the loop retrieval path (vba_btc_*) on a long synthetic workload: one batched SearchLoop over every session per keyframe
(vba_btc_search_loop_sessions, VS:2417-2421) and icp_normal on resident plane clouds.  Prints one JSON line with device times
(the "loop" timing family, event-bracketed) and, for a few keyframes, the per-call time of the numpy restatement
(tests/btc_oracle.py — a restatement, not a CPU baseline of the reference).

    python tools/btc_probe.py --sessions 3 --keyframes 2000 --desc 300
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--desc", type=int, default=300)
    ap.add_argument("--searches", type=int, default=50)
    ap.add_argument("--oracle", type=int, default=5)
    a = ap.parse_args()
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    import btc_oracle as bo
    S = synth.make_btc_sessions(n_sessions=a.sessions, n_kf=a.keyframes, max_desc=a.desc, n_keypoints=4000, seed=11)
    o = capi.default_options(); o.device = 0
    ctx = capi.Context(o)
    cfg = capi.btc_default_config(0)
    dbs = [ctx.btc_db(cfg) for _ in range(a.sessions)]
    n_std = 0
    for s in range(a.sessions - 1):                       # closed sessions, loaded whole (VS:310-410)
        for k in range(a.keyframes):
            dbs[s].push_plane_cloud(S[s]["cloud"][k], k)
            dbs[s].add_stds(S[s]["rows"][k], S[s]["bits"][k])
            n_std += len(S[s]["rows"][k])
        dbs[s].set_skip_near_num(-(a.keyframes + 10))
    cur, Sc = dbs[-1], S[-1]
    ks = a.keyframes - a.searches
    for k in range(ks):                                   # the live session up to the timed keyframes
        cur.push_plane_cloud(Sc["cloud"][k], k)
        cur.add_stds(Sc["rows"][k], Sc["bits"][k])
        n_std += len(Sc["rows"][k])
    ctx.timing_enable(True)
    ctx.timing_reset()
    wall, loops, icp_iters = [], 0, []
    for k in range(ks, a.keyframes):
        cur.push_plane_cloud(Sc["cloud"][k], k)
        t0 = time.perf_counter()
        res = ctx.btc_search_loop_sessions(dbs, Sc["rows"][k], Sc["bits"][k], cur)
        wall.append(time.perf_counter() - t0)
        loops += sum(r["loop_id"] >= 0 for r in res)
        cur.add_stds(Sc["rows"][k], Sc["bits"][k])
    search_us, nsearch = ctx.timing_get("loop")
    ctx.timing_reset()
    src = synth.btc_plane_cloud(20000, seed=1)
    cur.push_plane_cloud(src, a.keyframes)
    cur.push_plane_cloud(src, a.keyframes + 1)
    for _ in range(10):
        r = cur.icp_normal(a.keyframes, cur, a.keyframes + 1, np.array([0.2, -0.1, 0.05]), bo.so3_exp([0.01, 0.02, 0.0]), 0.1)
        icp_iters.append(r["iters"])
    icp_us, nicp = ctx.timing_get("loop")
    # the numpy restatement on the same databases, a few keyframes
    od = []
    for s in range(a.sessions):
        d = bo.BtcDb(cfg)
        for k in range(a.keyframes if s < a.sessions - 1 else ks):
            d.push_plane_cloud(S[s]["cloud"][k], k)
            d.add_stds(S[s]["rows"][k], S[s]["bits"][k])
        if s < a.sessions - 1:
            d.cfg["skip_near_num"] = -(a.keyframes + 10)
        od.append(d)
    t0 = time.perf_counter()
    for k in range(ks, ks + a.oracle):
        od[-1].push_plane_cloud(Sc["cloud"][k], k)
        for d in od:
            d.search_loop(Sc["rows"][k], Sc["bits"][k], Sc["cloud"][k])
        od[-1].add_stds(Sc["rows"][k], Sc["bits"][k])
    oracle_ms = (time.perf_counter() - t0) / a.oracle * 1e3
    try:
        rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        rev = None
    print(json.dumps(dict(sessions=a.sessions, keyframes=a.keyframes, desc_per_kf=a.desc, stored_stds=n_std, searches=nsearch,
                          loops_found=loops, search_device_us=search_us / max(nsearch, 1), search_wall_us=1e6 * float(np.median(wall)),
                          icp_points=20000, icp_device_us=icp_us / max(nicp, 1), icp_iters=icp_iters[0],
                          oracle_numpy_ms_per_batched_search=oracle_ms, rev=rev)))
    for d in dbs:
        d.close()
    ctx.close()


if __name__ == "__main__":
    main()
