"""Measurements of the global-map export for DESIGN.md section 15 (run on an MI355X): vba_kf_export_world against the only way a
node had to produce the same cloud before it, on the same store, in one process; median of `reps` runs after a warm-up.
    python tools/export_probe.py [out.json] [n_kf=200] [scans_per_kf=3] [n_pts=60000] [reps=5]
  (a) device   vba_kf_export_world into a device buffer at jump 1 and jump 3 (timed to the end of the stream's work)
  (b) host     the same into host memory
  (c) parent   one vba_kf_read per keyframe (points only, 24 B per point) + the numpy world transform, stride and narrowing
For (a) at jump 1 the achieved rate is (24 + 16) bytes x exported points / time, beside the float4 copy rate MI355X reaches.
Times are host clocks around calls that end in a device synchronise."""
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
import kf_oracle as ko
from prof_summary import source_hash  # noqa: E402

C = capi.C
COPY_RATE = 6.29e12        # bytes/s, float4 copy measured on MI355X (8.0e12 specified)


def hip_runtime():
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def timed(f, reps):
    f()                                                       # warm-up: buffers grow here
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n_kf, spk, n_pts, reps = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 200), (3, 3), (4, 60000), (5, 5))]
    t0 = time.time()
    path = synth.make_keyframe_path(n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, with_var=False)
    ctx = capi.Context(capi.default_options())
    store = ctx.kf_store()
    for k, kf in enumerate(path):
        store.build(kf["points"], kf["poses"], 0.05, id=k, jour=0.0)
    sizes = store.sizes()
    total = int(sizes.sum())
    poses = np.stack([store.get(k)["x0"] for k in range(n_kf)])
    print("store: %d keyframes of %d x %d rays, %d points resident (%.1f s to set up)" % (n_kf, spk, n_pts, total, time.time() - t0), flush=True)
    res = dict(source_hash=source_hash(), n_kf=n_kf, scans_per_kf=spk, n_pts=n_pts, points=total, reps=reps, copy_rate_bytes_per_s=COPY_RATE)

    hip = hip_runtime()
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(16 * max(total, 1))) == 0

    def parent(jump):                                         # what a node had to do: ONE vba_kf_read per keyframe, 24 B per point, no diagonals
        out = []
        for k in range(n_kf):
            xyz = np.empty((max(int(sizes[k]), 1), 3)); n = C.c_int()
            ctx._chk(ctx.lib.vba_kf_read(store.h, C.c_int(k), C.c_int(int(sizes[k])), capi._p(xyz), None, C.byref(n)))
            w = ko.world(poses[k], xyz[:n.value:jump]).astype(np.float32)
            out.append(np.concatenate([w, np.zeros((len(w), 1), np.float32)], axis=1))
        return np.concatenate(out)

    for jump in (1, 3):
        n = int(((sizes.astype(np.int64) + jump - 1) // jump).sum())

        def device():
            ctx.kf_export_world([store], [0.0], jump, 0, n, out=d)
            ctx.synchronize()

        a = timed(device, reps)
        b = timed(lambda: ctx.kf_export_world([store], [0.0], jump, 0, n), reps)
        c = timed(lambda: parent(jump), reps)
        assert np.array_equal(ctx.kf_export_world([store], [0.0], jump, 0, n), parent(jump))
        r = dict(exported=n, device_ms=a, host_ms=b, parent_ms=c, parent_over_host=c["median"] / b["median"])
        if jump == 1:
            r["device_bytes_per_s"] = 40.0 * n / (a["median"] * 1e-3)
            r["device_share_of_copy_rate"] = r["device_bytes_per_s"] / COPY_RATE
        res["jump%d" % jump] = r
        print("jump %d: %d records | (a) device %.3f ms | (b) host %.3f ms | (c) parent %.3f ms | parent / host %.2f"
              % (jump, n, a["median"], b["median"], c["median"], r["parent_over_host"]), flush=True)
        if jump == 1:
            print("        (a) moves %.3g bytes/s = %.1f %% of the %.3g bytes/s float4 copy rate" % (r["device_bytes_per_s"], 100 * r["device_share_of_copy_rate"], COPY_RATE))
    assert hip.hipFree(d) == 0
    ctx.close()
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    print("OK")


if __name__ == "__main__":
    main()
