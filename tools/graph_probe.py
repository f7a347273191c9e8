"""How much of an LM call's device time is launch gaps?  The bench call (begin, restart pass, 3 iterations, end) enqueued directly
vs the same call with its three iterations replayed from a HIP graph.  The restart pass is the first LM kernel of a call and carries
the call's state init (the begin poses by value), so it stays outside the graph: a captured first pass would freeze the poses of the
begin it was captured after.  The graph holds launches after the first pass only, which read everything from the device state."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import voxel_slam_amd  # noqa: F401
from voxel_slam_amd import capi, synth
wl = synth.CONFIGS["hesai200k_w10"]
s = synth.make_scans(wl)
poses = synth.poses_flat(s["R0"], s["p0"])
W = wl.win_size
st = torch.cuda.Stream(); torch.cuda.set_stream(st)
ctx = capi.Context(capi.options_from_workload(wl, stream=st.cuda_stream))
for i in range(W):
    ctx.cut_voxel(i, s["points"][i], poses[i])
ctx.recut(W, poses, multi=False)
def iters():
    for _ in range(3):
        ctx.lm_iterate(sync=False)
def call_direct(fetch=False):
    ctx.lm_begin(poses, thd_num=2); ctx.lm_refresh_eigen(); iters(); return ctx.lm_end(fetch=fetch)
for _ in range(5): call_direct()
torch.cuda.synchronize()
N = 100
t0 = time.perf_counter()
for _ in range(N): call_direct()
torch.cuda.synchronize()
print("direct: %.1f us per call (3 iterations)" % (1e6 * (time.perf_counter() - t0) / N))
ctx.lm_begin(poses, thd_num=2); ctx.lm_refresh_eigen()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=st):
    iters()
ctx.lm_end(fetch=False)
def call_graph(fetch=False):
    ctx.lm_begin(poses, thd_num=2); ctx.lm_refresh_eigen(); g.replay(); return ctx.lm_end(fetch=fetch)
for _ in range(5): call_graph()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(N): call_graph()
torch.cuda.synchronize()
print("graph : %.1f us per call (3 iterations)" % (1e6 * (time.perf_counter() - t0) / N))
# the host does not know that the replayed graph left an accept/reject pending, so the fetched state lacks the last step's: compare
# what both forms have applied, the first two trace rows
call_graph(fetch=True); a = ctx.last_trace().copy()
call_direct(fetch=True); b = ctx.last_trace().copy()
print("trace rows graph %d, direct %d; common rows equal: %s" % (len(a), len(b), np.array_equal(a[:2], b[:2])))
