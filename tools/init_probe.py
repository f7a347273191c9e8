"""Times vba_motion_init (Initialization::motion_init, voxelslam.cpp:617-819) at W = 10 with ~30k points per scan: one warm-up call,
then a few timed calls on the same context.  Prints the per-round rows of the last call, the wall time per call, the device time per
timing family, and the CPU oracle's time for the same call (tests/init_oracle.py replay on liboracle.so) as the comparison."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import voxel_slam_amd  # noqa: E402,F401
from voxel_slam_amd import capi, synth  # noqa: E402
import init_oracle  # noqa: E402
import oracle_api  # noqa: E402
from prof_summary import source_hash  # noqa: E402

W, N, CALLS = 10, 30000, 3
NM = np.array([0.01] * 3 + [1.0] * 3)
NW = np.array([1e-4] * 6)
FAMILIES = ("init", "insert", "recut", "residual", "hessian", "reduce", "solve")

wl = synth.Workload("init", W, 0.5, N, "spin32", (10.0, 8.0, 3.0), 0, 0)
d = synth.make_init_window(win_size=W, n_pts=N, scene="room")
ims = d["imus"]
ip = np.stack([oracle_api.imu_preintegrate(ims[i][:, 0], ims[i][:, 1:4], ims[i][:, 4:7], np.zeros(3), np.zeros(3), NM, NW, d["scale_gravity"])
               for i in range(1, W)])
ctx = capi.Context(capi.options_from_workload(wl))


def call():
    return ctx.motion_init(d["clouds"], d["curvs"], d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err, d["scale_gravity"], NM, NW,
                           d["states"], d["covs"], ip, want_pvec=False)


call()                                   # warm-up: allocations, code objects
ctx.timing_enable(True)
ctx.timing_reset()
walls = []
for _ in range(CALLS):
    t0 = time.perf_counter()
    r = call()
    walls.append(time.perf_counter() - t0)
print("source hash %s" % source_hash()[:12])
print("window: W=%d, %d points in, %d rounds, converged=%d, eigvalue3=%s" % (W, sum(len(c) for c in d["clouds"]), r["iterations"], r["converged"],
                                                                           np.array2string(r["eigvalue3"], precision=3)))
print("round  factors      resis0      resis1        |g|  converge_flag")
for k, row in enumerate(r["round_log"]):
    print("%5d  %7d  %10.6f  %10.6f  %9.5f  %d" % (k, int(row[0]), row[1], row[2], row[3], int(row[4])))
print("wall ms per call: %s (median %.2f)" % (", ".join("%.2f" % (1e3 * w) for w in walls), 1e3 * float(np.median(walls))))
print("device time per call by timing family (us, launches per call):")
for f in FAMILIES:
    t, n = ctx.timing_get(f)
    print("  %-9s %10.1f  %6.1f" % (f, t / CALLS, n / CALLS))
t0 = time.perf_counter()
b = init_oracle.motion_init(oracle_api, W, wl, d["clouds"], d["curvs"], d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err,
                            d["scale_gravity"], NM, NW, d["states"], d["covs"], ip)
t_cpu = time.perf_counter() - t0
print("CPU oracle replay of the same call (numpy blur walk + C++ oracle map, LI-BA, pre-integration): %.1f ms (%d rounds, converged=%d); ratio to the device wall median %.0fx"
      % (1e3 * t_cpu, b["iterations"], b["converged"], t_cpu / float(np.median(walls))))
