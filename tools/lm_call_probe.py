"""The lidar LM call of bench.py's timed loop — [lm_begin, lm_refresh_eigen, 3 x lm_iterate(sync=False), lm_end] — for a kernel trace:
ten calls enqueued back to back without a fetch (the timed loop's form), then, each after a stream synchronisation and a pause of
PAUSE_S (what tools/lm_call_timeline.py splits the trace by), one call without a fetch and two with (what vba_lidar_ba_damping_iter and the local-mapping step do).  tools/lm_call_timeline.py prints the last
three as timelines.
    rocprofv3 --kernel-trace --output-format csv -d out -o lm -- python tools/lm_call_probe.py
    python tools/lm_call_timeline.py out/*/lm_kernel_trace.csv"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
wl = synth.CONFIGS["hesai200k_w10"]
s = synth.make_scans(wl)
poses = synth.poses_flat(s["R0"], s["p0"])
W = wl.win_size
PAUSE_S = 0.005
st = torch.cuda.Stream(); torch.cuda.set_stream(st)
ctx = capi.Context(capi.options_from_workload(wl, stream=st.cuda_stream))
for i in range(W):
    ctx.cut_voxel(i, s["points"][i], poses[i])
ctx.recut(W, poses, multi=False)


def call(fetch):
    ctx.lm_begin(poses, thd_num=2)
    ctx.lm_refresh_eigen()
    for _ in range(3):
        ctx.lm_iterate(sync=False)
    return ctx.lm_end(fetch=fetch)


for _ in range(10):
    call(False)
for fetch in (False, True, True):
    torch.cuda.synchronize()
    time.sleep(PAUSE_S)
    call(fetch)
torch.cuda.synchronize()
print("voxels %d, trace rows of the last call %d" % (ctx.size(), len(ctx.last_trace())))
