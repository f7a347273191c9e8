"""Wall time of vba_pgo_optimize at N = 4 000 / K = 400 and N = 20 000 / K = 2 000 scans / keyframes with HBA-shaped
edges (tests/pgo_oracle.py::reference_session).  Writes one JSON line.  For the split into linearise / eliminate / skeleton
factorisation / back substitution run it under `rocprofv3 --kernel-trace --stats -- python tools/pgo_probe.py` (no counters in
the same run) and pass the stats file to --stats: kernels are grouped as
  linearise   k_pgo_linearize, k_pgo_cost, k_pgo_assemble
  eliminate   k_pgo_seg_elim
  skeleton    k_pgo_skel_fill, k_pgo_skel_scatter, k_bigl_panel, k_bigl_update, k_pgo_pivots
  back-subst  k_bigl_bs_tri, k_bigl_bs_gemv, k_pgo_skel_dx, k_pgo_seg_back, k_pgo_relin"""
import argparse
import csv
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUPS = {"linearise": ("k_pgo_linearize", "k_pgo_cost", "k_pgo_assemble"), "eliminate": ("k_pgo_seg_elim",),
          "skeleton": ("k_pgo_skel_fill", "k_pgo_skel_scatter", "k_bigl_panel", "k_bigl_update", "k_pgo_pivots"),
          "back_subst": ("k_bigl_bs_tri", "k_bigl_bs_gemv", "k_pgo_skel_dx", "k_pgo_seg_back", "k_pgo_relin")}


def split(stats_csv):
    tot = defaultdict(float)
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "").split("(")[0].replace("void ", "").split("::")[-1]
            for g, names in GROUPS.items():
                if name in names:
                    tot[g] += float(row.get("TotalDurationNs", 0)) * 1e-6
    return {k: round(v, 3) for k, v in tot.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run of this probe: print the per-group split (ms)")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(split(a.stats)))
        return
    import pgo_oracle as po
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi
    o = capi.default_options(); o.device = 0
    ctx = capi.Context(o)
    out = {}
    for n in (4000, 20000):
        rng = np.random.default_rng(5)
        X, Y, edges, priors = po.reference_session(rng, n=n, n_loops=n // 1000)
        ctx.pgo_optimize(Y, edges, priors)                 # warm-up (allocations)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.pgo_optimize(Y, edges, priors)
            ts.append(time.perf_counter() - t0)
        out["N%d_K%d" % (n, n // 10)] = dict(edges=len(edges), seconds_median=float(np.median(ts)))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
