"""Create / grow / destroy cycles of a context and its handle objects on the MI355X ("Source layout": a buffer is freed by
its member's destructor, vba_destroy lists no buffers).  One warm-up cycle, then six: every cycle creates a context (win_size 3),
runs the BA core on a small factor store and again after the store grew, takes a keyframe store, a BTC database, a scan frame, a
loop map and the kd-tree odometry through their first allocation and one growth, and destroys everything.  Every call returns
VBA_OK (the wrappers raise otherwise), the grown keyframe store reads back the bits it was given, and the device's free memory
after each cycle's destroy does not drift.

The sizes are the smallest that cross each buffer's first capacity: the factor store starts at 4096 voxels (6208 after the stride
skew), the keyframe arrays, the kd-tree map and the plane clouds at 65536 points, the descriptor rows, offsets and votes at 1024,
the match list at 65536, a scan frame's message at 1 MiB and its point block at 65536 points.  The tables that only grow past 64
scans or segments (keyframe transforms, undistortion parameters, loop-map segments) are allocated, not grown, here."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 3
GRANULE = 2 << 20
# free bytes after cycle 1 minus free bytes after cycle 6, measured with this test on the parent commit (raw owning pointers, the
# free lists of vba_destroy and the handles' destroy functions) and on this one, same MI355X, same visit: both 0, the six readings
# identical in either run (the parent's series does not scatter, so the bound is asserted)
PARENT_DRIFT = 0
CHILD_DRIFT = 0


def _hip():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _free_bytes(hip):
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return fr.value


@pytest.fixture(scope="module")
def inputs():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=W, n_pts=4000)
    s = synth.make_scans(wl)
    f = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
    assert len(f["coe"]) >= 64
    small = {k: np.ascontiguousarray(v[:64]) for k, v in f.items()}
    big = {k: np.ascontiguousarray(np.concatenate([v[:64]] * 100)) for k, v in f.items()}       # 6400 voxels: past the first stride
    kfs = synth.make_keyframe_path(n_kf=2, scans_per_kf=2, n_pts=300, with_var=False)
    return dict(capi=capi, wl=wl, poses=synth.poses_flat(s["R0"], s["p0"]), small=small, big=big, kfs=kfs, planes=synth.btc_plane_cloud(400, seed=3))


def _cycle(inp):
    capi = inp["capi"]
    opt = capi.options_from_workload(inp["wl"])
    opt.device = 0
    ctx = capi.Context(opt)
    # BA core: fixed blocks, pinned staging, upload staging, the factor store; then the store grown with its first voxels kept
    ctx.push_dict(inp["small"])
    a = ctx.lidar_ba_damping_iter(inp["poses"], max_iter=1, thd_num=2)
    assert a["status"] == 0 and ctx.size() == 64
    ev0 = ctx.read_back()
    ctx.push_dict(inp["big"])
    assert ctx.size() == 64 + 6400
    ev1 = ctx.read_back()
    assert all(np.array_equal(x[:64], y) for x, y in zip(ev1, ev0))
    assert ctx.lidar_ba_damping_iter(inp["poses"], max_iter=1, thd_num=2)["status"] == 0
    # keyframe store: two keyframes of a few hundred points, then the arrays grown under them
    store = ctx.kf_store()
    for i, kf in enumerate(inp["kfs"]):
        assert store.build(kf["points"], kf["poses"], 0.05, id=i)[0] > 0
    before = [store.read(k) for k in range(2)]
    n0, _ = store.allocations()
    store.reserve(points=4 * 65536, keyframes=4 * 64, merge_points=4 * 65536)
    assert store.allocations()[0] > n0
    after = [store.read(k) for k in range(2)]
    for (p0, v0), (p1, v1) in zip(before, after):
        assert len(p0) > 0 and p0.tobytes() == p1.tobytes() and v0.tobytes() == v1.tobytes()
    rec = ctx.kf_export_world([store], [1.0], 1)                                      # the export table ring and staging
    assert len(rec) == sum(len(p) for p, _ in before)
    # BTC database: two plane clouds, one ICP (the shared ICP state), then every array grown
    db = ctx.btc_db()
    db.push_plane_cloud(inp["planes"], 0)
    db.push_plane_cloud(inp["planes"], 1)
    r = db.icp_normal(0, db, 1, np.zeros(3), np.eye(3), 0.0)
    assert np.isfinite(r["t"]).all()
    db.reserve(stds=4 * 1024, frames=4 * 1024, cloud_points=4 * 65536, matches=4 * 65536)
    assert np.array_equal(db.plane_cloud(1), inp["planes"])
    # scan frame and loop map: first allocation, then four times the size
    fr = ctx.scan_frame()
    fr.reserve(60000, 20)
    n0, _ = fr.allocations()
    fr.reserve(4 * 60000, 20)
    assert fr.allocations()[0] > n0
    lm = ctx.loop_map()
    lm.reserve(fix_points=2000, nodes=2000)
    assert lm.build(store, init_num=2) > 0
    lm.reserve(fix_points=8000, nodes=8000)
    # kd-tree odometry: both halves of the map and the scan scratch, then grown
    ctx.kdtree_reserve(60000, 2000)
    n0, _ = ctx.kdtree_allocations()
    ctx.kdtree_reserve(4 * 60000, 4 * 16384)
    assert ctx.kdtree_allocations()[0] > n0
    fr.close(); lm.close(); db.close(); store.close()
    ctx.close()


def test_cycles_leave_no_device_memory_behind(inputs):
    _cycle(inputs)                                   # warm-up: code objects, the runtime's own pools
    hip = _hip()
    free = []
    for _ in range(6):
        _cycle(inputs)
        free.append(_free_bytes(hip))
    drift = free[0] - free[-1]
    print("free bytes after each cycle's destroy: %s; drift %d (parent %d, child %d as measured)" % (free, drift, PARENT_DRIFT, CHILD_DRIFT))
    assert drift <= PARENT_DRIFT + GRANULE
