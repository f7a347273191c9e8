"""Child process of tests/test_gpu_edge.py::test_concurrent_first_use_of_the_lm_kernels: four threads, each with a context of its
own (W = 4, a few hundred voxels), make this process's first launches of the LM kernels side by side, as the workers of
vba_hba_global do: vba_lidar_ba_damping_iter, then vba_li_ba_damping_iter with gravity.  A fifth context then runs the same
inputs alone.  One pass, no retry.  Prints one JSON line; exit 0 when all five results are bit-identical."""
import dataclasses
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import voxel_slam_amd  # noqa: E402,F401
from voxel_slam_amd import capi, synth  # noqa: E402

W, THREADS, WAIT = 4, 4, 60.0


def inputs():
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=W, n_pts=4000)
    s = synth.make_scans(wl)
    f = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
    assert len(f["coe"]) >= 300
    fac = {k: np.ascontiguousarray(v[:300]) for k, v in f.items()}
    imu_samples, vel, g = synth.make_imu(wl, gyr_sigma=1e-3, acc_sigma=1e-2)
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    imus = np.stack([capi.imu_preintegrate(t, gy, ac, np.zeros(3), np.zeros(3), nm, nw) for (t, gy, ac) in imu_samples])
    states = np.zeros((W, 25))
    for i in range(W):
        states[i, 0] = 0.1 * i
        states[i, 1:10] = s["R0"][i].ravel(); states[i, 10:13] = s["p0"][i]; states[i, 13:16] = vel[i]; states[i, 22:25] = g
    return dict(wl=wl, fac=fac, poses=synth.poses_flat(s["R0"], s["p0"]), states=states, imus=imus)


def run(inp, gate=None):
    opt = capi.options_from_workload(inp["wl"])
    opt.device = 0
    ctx = capi.Context(opt)
    ctx.push_dict(inp["fac"])
    if gate is not None:
        gate.wait(WAIT)                          # the LM calls below start together
    a = ctx.lidar_ba_damping_iter(inp["poses"], max_iter=3, thd_num=2)
    b = ctx.li_ba_damping_iter(inp["states"], inp["imus"], gravity=True, max_iter=3)
    ctx.close()
    assert a["status"] == 0 and len(a["trace"]) > 0 and len(b["trace"]) > 0
    return [a["poses"], a["resis"], a["trace"], b["states"], b["imus"], b["resis"], b["trace"]]


def main():
    inp = inputs()
    gate = threading.Barrier(THREADS)
    results, errors = [None] * THREADS, []

    def worker(k):
        try:
            results[k] = run(inp, gate)
        except BaseException as e:               # (reported by the parent: a status of the library, a broken barrier)
            errors.append("thread %d: %r" % (k, e))
            gate.abort()

    ts = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(THREADS)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(2 * WAIT)
    if errors or any(t.is_alive() for t in ts):
        print(json.dumps(dict(ok=False, errors=errors, alive=[t.is_alive() for t in ts])), flush=True)
        os._exit(1)
    alone = run(inp)
    names = ["poses", "resis2", "trace", "li_states", "li_imus", "li_resis2", "li_trace"]
    differ = [(k, n) for k in range(THREADS) for n, x, y in zip(names, results[k], alone) if x.tobytes() != y.tobytes()]
    print(json.dumps(dict(ok=not differ, differ=differ, lm_rows=len(alone[2]), li_rows=len(alone[6]))), flush=True)
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(main())
