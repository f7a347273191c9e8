"""Device time per keyframe of vba_btc_generate_stds (GenerateSTDescs) at 200k and 2M points, and the numpy restatement's time
(tests/btc_gen_oracle.py: a TEST ORACLE, not a CPU baseline of the reference, which cannot be built here).  Writes one JSON line.
For the per-stage breakdown run it under `rocprofv3 --kernel-trace --stats -- python tools/btc_gen_probe.py --reps 3` (no
counters in the same run) and read the k_bg_* rows of the stats file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle", action="store_true", help="also time the numpy restatement (slow)")
    a = ap.parse_args()
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    o = capi.default_options(); o.device = 0
    ctx = capi.Context(o)
    out = {}
    for npts in (200000, 2000000):
        ses = synth.make_btc_keyframe_sessions(n_sessions=1, n_kf=a.reps + 1, n_points=npts, seed=31)[0]["cloud"]
        for high in (0, 1):
            db = ctx.btc_db(capi.btc_default_config(high))
            db.set_gen_config(capi.btc_default_gen_config(high))
            db.gen_reserve(points=npts, cells=1 << 22)
            db.generate_stds(ses[0], 0)                   # warm-up
            ts = []
            for k in range(1, a.reps + 1):
                t0 = time.perf_counter(); rows, _ = db.generate_stds(ses[k], k); ts.append(time.perf_counter() - t0)
            r = dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), rows=len(rows))
            if a.oracle:
                import btc_gen_oracle as bg
                t0 = time.perf_counter(); bg.generate_stds(ses[1], 0, bg.read_parameters(high)); r["oracle_s"] = time.perf_counter() - t0
            out["%dk_cfg%d" % (npts // 1000, high)] = r
            db.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
