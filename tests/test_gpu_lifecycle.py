"""Create / grow / destroy cycles of a context and its handle objects on the MI355X ("Source layout": a buffer is freed by
its member's destructor, vba_destroy lists no buffers).  One warm-up cycle, then six: every cycle creates a context (win_size 3),
runs the BA core on a small factor store and again after the store grew, takes a keyframe store, a BTC database, a scan frame, a
loop map and the kd-tree odometry through their first allocation and one growth, and destroys everything.  Every call returns
VBA_OK (the wrappers raise otherwise), the grown keyframe store reads back the bits it was given, and the device's free memory
after each cycle's destroy does not drift.

The sizes are the smallest that cross each buffer's first capacity: the factor store starts at 4096 voxels (6208 after the stride
skew), the keyframe arrays, the kd-tree map and the plane clouds at 65536 points, the descriptor rows, offsets and votes at 1024,
the match list at 65536, a scan frame's message at 1 MiB and its point block at 65536 points.  The tables that only grow past 64
scans or segments (keyframe transforms, undistortion parameters, loop-map segments) are allocated, not grown, here.

A second test does the same for the stores whose blocks are owning members beside a view ("Buffer ownership": the voxel
map, the global-BA stores, the descriptor generator): each through its first allocation and the smallest growth that exists.  The
node family of the map starts at 2^18 and the first recut asks for nodes + 8 * 65536, so it grows to 2^20 with the first scan's
leaves kept; the scan family starts at 65536 points a slot and a 70 000-point scan grows it with slot 0 kept; the fixed pool is
allocated (2^20 points, its growth runs the same code as the other two families); the point group of the global BA starts at
n + n / 4 + 1024; the generator's point group goes 65536 -> 131072.  That a grown map holds what a map sized in advance holds is
checked in deterministic mode, where the leaf dump has a canonical order: bit for bit."""
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
# the same for test_store_cycles_leave_no_device_memory_behind, parent = the commit before the stores' blocks became owning members
# (hand-kept free lists in map_free, GbaStore::free_all, BigStore::release, btcgen_free), same MI355X, same visit: the six readings
# after each cycle's destroy and their drift; neither series scatters
STORE_PARENT_FREE = [308092600320] * 6              # (this test alone in its process)
STORE_CHILD_FREE = [307979354112] * 6               # (after the test above in the same process)
STORE_PARENT_DRIFT = 0
STORE_CHILD_DRIFT = 0


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


# ---------------------------------------------------------------- the satellites' state ("Source layout": where state lives)
# (allocations, bytes) of vba_kf_voxel_export_allocations and of vba_odom_kdtree_allocations after the sequence of
# test_destroy_right_after_one_export, returned by the parent commit's library (the fields still members of vba_ctx) on the same
# MI355X in the same visit as this commit's: the sequence adds nothing to either counter
PARENT_VOXEL_EXPORT_ALLOCATIONS = (0, 0)
PARENT_KDTREE_ALLOCATIONS = (0, 0)


def test_context_without_a_satellite_call(inputs):
    """created and destroyed with its satellite state never touched: the state is made and released with the context"""
    capi = inputs["capi"]
    opt = capi.options_from_workload(inputs["wl"])
    opt.device = 0
    hip, free = None, []
    for _ in range(3):
        ctx = capi.Context(opt)
        assert ctx.h
        ctx.close()
        hip = hip or _hip()
        free.append(_free_bytes(hip))
    print("free bytes after each destroy: %s" % free)
    assert free[1] - free[2] <= GRANULE


def test_destroy_right_after_one_export(inputs):
    """one vba_kf_export_world of a single keyframe of 64 points to host memory, so that the export's ring, its events, the table and
    the staging exist, and the destroy straight after it: the events go with the satellite state, not by a list in vba_destroy"""
    capi = inputs["capi"]
    opt = capi.options_from_workload(inputs["wl"])
    opt.device = 0
    g = np.arange(4.0) + 0.25
    pts = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))     # one point a voxel
    pose = np.concatenate([np.eye(3).ravel(), np.zeros(3)])[None]
    hip, free = None, []
    for _ in range(2):
        ctx = capi.Context(opt)
        store = ctx.kf_store()
        assert store.build([pts], pose, 0.1, id=0)[0] == 64
        rec = ctx.kf_export_world([store], [1.0], 1)
        assert rec.shape == (64, 4) and set(map(tuple, rec[:, :3].tolist())) == set(map(tuple, pts.tolist())) and (rec[:, 3] == 1.0).all()
        vx, kd = ctx.kf_export_voxel_allocations(), ctx.kdtree_allocations()
        print("voxel export allocations %s (parent %s), kd-tree allocations %s (parent %s)" % (vx, PARENT_VOXEL_EXPORT_ALLOCATIONS, kd, PARENT_KDTREE_ALLOCATIONS))
        assert vx == PARENT_VOXEL_EXPORT_ALLOCATIONS and kd == PARENT_KDTREE_ALLOCATIONS
        ctx.close()                                      # (closes the store first)
        hip = hip or _hip()
        free.append(_free_bytes(hip))
    print("free bytes after each destroy: %s" % free)
    assert free[0] - free[1] <= GRANULE


# ---------------------------------------------------------------- the stores with a view beside their owners
GBA = dict(gba_voxel_size=2.0, gba_min_eigen_value=0.1, gba_eig=[0.25, 0.25, 0.25, 0.25])


@pytest.fixture(scope="module")
def store_inputs():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=W, n_pts=90000)
    s = synth.make_scans(wl)
    assert min(len(p) for p in s["points"]) >= 70000
    rng = np.random.default_rng(5)
    A = rng.normal(0, 0.01, (70000, 3, 3))
    var = np.ascontiguousarray((A @ A.transpose(0, 2, 1) + 1e-6 * np.eye(3)).reshape(-1, 9))
    poses = synth.poses_flat(s["R0"], s["p0"])
    fixed = np.ascontiguousarray((s["points"][2] @ s["R0"][2].T + s["p0"][2])[:500])
    wl4 = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=4, n_pts=4000)
    s4 = synth.make_scans(wl4)
    f32 = lambda a: np.ascontiguousarray(a).astype(np.float32).astype(np.float64)
    cloud = synth.make_btc_keyframe_sessions(n_sessions=1, n_kf=1, n_points=100000, seed=11)[0]["cloud"][0]
    assert len(cloud) >= 70000
    return dict(capi=capi, wl=wl, pts=[np.ascontiguousarray(s["points"][0][:2000]), np.ascontiguousarray(s["points"][1][:70000])], var=var, poses=poses,
                fixed=fixed, gba_small=[f32(p[:300]) for p in s["points"]], gba_big=[f32(p[:2000]) for p in s["points"]],
                clouds4=[f32(p) for p in s4["points"]], poses4=synth.poses_flat(s4["R0"], s4["p0"]), cloud=np.ascontiguousarray(cloud[:70000], dtype=np.float32))


def _map_sequence(inp, ctx):
    """first allocation of the node, scan and fixed families and the root table, growth of the node and scan families with contents
    kept; returns the leaf dump after recut(2)"""
    pts, var, poses = inp["pts"], inp["var"], inp["poses"]
    ctx.cut_voxel(0, pts[0], poses[0], var=var[:2000])
    ctx.recut(1, poses)
    ctx.cut_voxel(1, pts[1], poses[1], var=var)
    ctx.recut(2, poses)
    dump = ctx.dump_leaves()
    assert len(dump) > 100
    ctx.margi(2, poses, jour=1.0)
    ctx.cut_voxel_fix(inp["fixed"], jour=2.0)
    ctx.prune(2.0)
    ctx.map_reset()
    assert ctx.num_roots() == 0
    return dump


def _store_cycle(inp):
    capi = inp["capi"]

    def context(**kw):
        opt = capi.options_from_workload(inp["wl"])
        opt.device = 0
        for k, v in kw.items():
            setattr(opt, k, v)
        return capi.Context(opt)

    ctx = context()
    _map_sequence(inp, ctx)
    # global BA: the octree of a window (point group allocated, then grown), then a window of another size: the sparse path's arena
    assert ctx.gba_build(inp["gba_small"], inp["poses"], GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"]) >= 0
    assert ctx.gba_build(inp["gba_big"], inp["poses"], GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"]) > 0
    got = ctx.hba_add_edge(inp["clouds4"], inp["poses4"], GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 1, 2, want_cloud=False)
    assert np.isfinite(got["poses"]).all()
    # descriptor generator: every group allocated, then the point group (and the planes sized by it) grown
    db = ctx.btc_db(capi.btc_default_config(0))
    db.set_gen_config(capi.btc_default_gen_config(0))
    db.generate_stds(inp["cloud"][:2000], 0)
    n0, _ = db.gen_allocations()
    assert n0 > 0
    db.generate_stds(inp["cloud"], 1)
    assert db.gen_allocations()[0] > n0
    db.close()
    ctx.close()
    # deterministic mode (hfirst, the stable sort's histograms): the grown map against one sized in advance
    grown, sized = context(deterministic=1), context(deterministic=1, max_points_per_scan=131072, max_map_nodes=1 << 20)
    a, b = _map_sequence(inp, grown), _map_sequence(inp, sized)
    assert a.shape == b.shape and np.array_equal(a, b)
    grown.close(); sized.close()


def test_store_cycles_leave_no_device_memory_behind(store_inputs):
    _store_cycle(store_inputs)                       # warm-up
    hip = _hip()
    free = []
    for _ in range(6):
        _store_cycle(store_inputs)
        free.append(_free_bytes(hip))
    drift = free[0] - free[-1]
    print("free bytes after each cycle's destroy: %s; drift %d (parent %d, child %d as measured)" % (free, drift, STORE_PARENT_DRIFT, STORE_CHILD_DRIFT))
    assert drift <= STORE_PARENT_DRIFT + GRANULE
