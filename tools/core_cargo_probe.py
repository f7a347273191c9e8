"""Same-bits probe of the BA core's host side: two builds of libvoxelba.so must return identical arrays from every flow that
hessian_pass / launch_residual / the sharded trial step / the pinned block serve.

    python3 tools/core_cargo_probe.py PARENT_LIB [CHILD_LIB] [--out result.json]

Each library runs in a fresh child process (VBA_LIB selects it; CHILD_LIB defaults to the tree's own build) and stores its arrays in an
.npz; the parent process compares them with array_equal and prints one JSON line.  Cases (stores of about 200 voxels pushed in a fixed
order, as tests/test_gpu_lm_trips.py pushes them):
  * vba_lidar_ba_damping_iter at W = 2, 10, 16 and vba_li_ba_damping_iter at W = 2, 10, 11, 16 with gravity off and on; each single-rank
    and with force_collective = 1 (the all-reduce hook returns its input), each with and without hess requested;
  * both calls on a hessian_compact_tiles context at W = 4;
  * vba_factor_acc_evaluate2 (whole store and a sub-range) and vba_debug_li_imu in its three forms.
It takes no part in the test suite."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _workload(synth, W):
    room, hesai = synth.CONFIGS["room20k_w4"], synth.CONFIGS["hesai200k_w10"]
    if W == 10:
        return dataclasses.replace(hesai, n_pts=40000), slice(5000, 5150)
    if W == 2:
        return dataclasses.replace(room, win_size=2, n_pts=4000), slice(200, 400)
    return dataclasses.replace(room, win_size=W, n_pts=8000 if W > 10 else 4000), slice(0, 200)


def _problem(capi, synth, W):
    wl, sl = _workload(synth, W)
    s = synth.make_scans(wl)
    fac = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
    assert len(fac["coe"]) >= sl.stop, (W, len(fac["coe"]))
    fac = {k: np.ascontiguousarray(v[sl]) for k, v in fac.items()}
    poses = synth.poses_flat(s["R0"], s["p0"])
    imu_samples, vel, g = synth.make_imu(wl, gyr_sigma=1e-3, acc_sigma=1e-2)
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    imus = np.stack([capi.imu_preintegrate(t, gy, ac, np.zeros(3), np.zeros(3), nm, nw) for (t, gy, ac) in imu_samples])
    states = np.zeros((W, 25))
    for i in range(W):
        states[i, 0] = 0.1 * i
        states[i, 1:10] = s["R0"][i].ravel(); states[i, 10:13] = s["p0"][i]; states[i, 13:16] = vel[i]; states[i, 22:25] = g
    return wl, fac, poses, states, imus


def _ctx(capi, wl, fac, **opts):
    o = capi.options_from_workload(wl)
    for k, v in opts.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    ctx = capi.Context(o)
    if opts.get("force_collective"):
        ctx.set_allreduce(lambda ptr, n, stream: 0)     # one rank: the sum over the ranks is the buffer itself
    ctx.push_dict(fac)
    return ctx


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _lidar(ctx, poses, want_hess):
    poses = np.ascontiguousarray(poses).copy(); n = 6 * ctx.W
    H = np.zeros((n, n)); resis = np.zeros(2); conv = C.c_int(0)
    st = ctx.lib.vba_lidar_ba_damping_iter(ctx.h, _p(poses), _p(H) if want_hess else None, _p(resis), C.c_int(5), C.c_int(2), C.byref(conv))
    assert st == 0, st
    return dict(poses=poses, hess=H, resis=resis, conv=np.array([conv.value]), trace=ctx.last_trace())


def _li(ctx, states, imus, gravity, want_hess):
    states = np.ascontiguousarray(states).copy(); imus = np.ascontiguousarray(imus).copy()
    n = 15 * ctx.W + (3 if gravity else 0)
    H = np.zeros((n, n)); resis = np.zeros(2)
    st = ctx.lib.vba_li_ba_damping_iter(ctx.h, _p(states), _p(imus), C.c_int(int(gravity)), C.c_int(4), _p(H) if want_hess else None, _p(resis))
    assert st == 0, st
    return dict(states=states, imus=imus, hess=H, resis=resis, trace=ctx.last_trace())


def child(out_path):
    sys.path.insert(0, ROOT)
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    out = {}

    def put(case, d):
        for k, v in d.items():
            out["%s/%s" % (case, k)] = np.asarray(v)

    problems = {W: _problem(capi, synth, W) for W in (2, 4, 10, 11, 16)}
    for W, (wl, fac, poses, states, imus) in problems.items():
        put("input/w%d" % W, dict(fac, poses=poses, states=states, imus=imus))
    for W in (2, 10, 11, 16):
        wl, fac, poses, states, imus = problems[W]
        for coll in (0, 1):
            ctx = _ctx(capi, wl, fac, force_collective=coll)
            try:
                for hess in (1, 0):
                    tag = "w%d/coll%d/hess%d" % (W, coll, hess)
                    if W != 11:
                        put("lidar/" + tag, _lidar(ctx, poses, hess))
                    for gravity in (0, 1):
                        put("li/%s/g%d" % (tag, gravity), _li(ctx, states, imus, gravity, hess))
            finally:
                ctx.close()
    wl, fac, poses, states, imus = problems[4]
    ctx = _ctx(capi, wl, fac, hessian_compact_tiles=1)
    try:
        put("compact/lidar", _lidar(ctx, poses, 1))
        for gravity in (0, 1):
            put("compact/li/g%d" % gravity, _li(ctx, states, imus, gravity, 1))
            put("compact/imu_h3/g%d" % gravity, ctx.debug_li_imu(states, imus, gravity=bool(gravity), form="h3", trial=True))
    finally:
        ctx.close()
    wl, fac, poses, states, imus = problems[10]
    ctx = _ctx(capi, wl, fac)
    try:
        for name, (head, end) in (("all", (0, None)), ("part", (17, 101)), ("empty", (40, 40))):
            H, g, r = ctx.acc_evaluate2(poses, head, end)
            put("acc_evaluate2/" + name, dict(H=H, g=g, r=np.array([r])))
        put("residual/all", dict(r=np.array([ctx.evaluate_only_residual(poses)])))
        for gravity in (0, 1):
            for form in ("alone", "h2"):
                put("imu_%s/g%d" % (form, gravity), ctx.debug_li_imu(states, imus, gravity=bool(gravity), form=form, trial=True))
    finally:
        ctx.close()
    np.savez(out_path, **out)


def main(argv):
    if argv[:1] == ["--child"]:
        return child(argv[1])
    out_json = None
    if "--out" in argv:
        i = argv.index("--out"); out_json = argv[i + 1]; del argv[i:i + 2]
    libs = [os.path.abspath(a) for a in argv] + [os.path.join(ROOT, "voxel-slam_amd", "libvoxelba.so")]
    libs = libs[:2]
    assert len(libs) == 2 and all(os.path.exists(p) for p in libs), libs
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            path = os.path.join(tmp, "lib%d.npz" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=dict(os.environ, VBA_LIB=lib), check=True, timeout=600)
            with np.load(path) as z:
                res.append({k: z[k] for k in z.files})
    a, b = res
    assert sorted(a) == sorted(b)
    differ = [k for k in sorted(a) if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=True)]
    finite = all(np.isfinite(v).all() for v in b.values())
    traces = {k: int(len(v)) for k, v in b.items() if k.endswith("/trace")}
    line = dict(libs=libs, arrays=len(a), cases=len({k.rsplit("/", 1)[0] for k in a}), differ=differ, all_finite=bool(finite),
                trace_rows_min=min(traces.values()), trace_rows_max=max(traces.values()), identical=not differ)
    print(json.dumps(line))
    if out_json:
        with open(out_json, "w") as f:
            json.dump(line, f, indent=1)
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
