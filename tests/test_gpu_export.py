"""The global-map export (vba_kf_export_plan / vba_kf_export_world) on the MI355X against the restatement
tests/export_oracle.py of ResultOutput::pub_globalmap (voxelslam.cpp:110-154).

Every comparison of exported values is np.array_equal against export_oracle.points fed with store.read(k) and the poses in force:
both sides round every product and sum on its own in the order include/voxelba.h states and narrow once to float, so there is no
tolerance to choose."""
import numpy as np
import pytest

import export_oracle as eo

pytestmark = pytest.mark.gpu

EDGE_SIZES = [0, 1, 2, 3, 255, 256, 257, 1000]      # around one workgroup's 256 outputs; 1774 points = 7 workgroups at jump 1
SENT = np.float32(-12345.5)


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


@pytest.fixture(scope="module")
def synth():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth as s
    return s


def _ctx(capi):
    o = capi.default_options()
    o.device = 0
    return capi.Context(o)


def _hip():
    """the HIP runtime libvoxelba.so has already loaded (for a device buffer of the test's own)"""
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _poses(n, seed):
    """n distinct poses with non-trivial rotations"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([Rotation.from_rotvec(rng.uniform(-1.2, 1.2, 3)).as_matrix().ravel(), rng.uniform(-40, 40, 3)]) for _ in range(n)])


def _lattice(n, seed):
    """n points 1 m apart (distinct cells of the integer lattice, float-exact coordinates), in random order"""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(16 ** 3)[:n]
    return np.stack([idx % 16, (idx // 16) % 16, idx // 256], axis=1).astype(np.float64) - 7.75


def _edge_store(capi, ctx, sizes, seed):
    """One store whose keyframe k holds exactly sizes[k] points: one scan of points 1 m apart at voxel_size 0.05 without
    covariances, so every point is its own voxel and the kept cloud is the input in input order."""
    store = ctx.kf_store()
    poses = _poses(len(sizes), seed)
    for k, n in enumerate(sizes):
        kept, _, _ = store.build([_lattice(n, seed + 100 + k)], poses[k:k + 1], 0.05, id=k, jour=float(k))
        assert kept == n
    clouds = [store.read(k)[0] for k in range(len(sizes))]
    assert [len(c) for c in clouds] == list(sizes) and store.sizes().tolist() == list(sizes)
    return store, clouds, poses


@pytest.fixture(scope="module")
def edge(capi):
    ctx = _ctx(capi)
    store, clouds, poses = _edge_store(capi, ctx, EDGE_SIZES, 5)
    yield dict(ctx=ctx, store=store, clouds=clouds, poses=poses)
    ctx.close()


def _want(e, jump, intensity=3.0):
    return eo.points(e["clouds"], e["poses"], [intensity] * len(e["clouds"]), jump)


@pytest.mark.parametrize("jump", [1, 2, 3, 7, 2000])
def test_edge_sizes(capi, edge, jump):
    """Keyframes of exactly 0, 1, 2, 3, 255, 256, 257 and 1000 points with distinct, rotated poses, exported at jump 1, 2, 3, 7
    and 2000.  The sizes are not multiples of the jumps: a stride that ran on across keyframe boundaries without restarting at
    every keyframe would pick other points and fail this comparison, and so would a lane that took the pose of the wrong keyframe
    (the keyframe boundaries fall inside workgroups, at their edges and one past them)."""
    want = _want(edge, jump)
    _, kb, _ = capi.kf_export_plan(EDGE_SIZES, 5_000_000, jump)
    got = edge["ctx"].kf_export_world([edge["store"]], [3.0], jump)
    print("jump %d: %d records" % (jump, len(got)))
    assert got.dtype == np.float32 and got.shape == (kb[-1], 4) == want.shape
    assert len(want) == sum(-(-n // jump) for n in EDGE_SIZES)
    assert np.array_equal(got, want)
    # the kept clouds are the inputs in input order, so the exported rows are known without the store as well
    k = 7
    direct = eo.points([_lattice(EDGE_SIZES[k], 5 + 100 + k)], edge["poses"][k:k + 1], [3.0], jump)
    assert np.array_equal(got[kb[k]:kb[k + 1]], direct)


def test_current_poses_and_read_only(capi):
    ctx = _ctx(capi)
    store, clouds, poses = _edge_store(capi, ctx, [5, 300, 0, 41], 11)
    store.set_history(2)                                                       # exist = 1, 1, 0, 0
    before = [store.get(k) for k in range(4)]
    assert [b["exist"] for b in before] == [1, 1, 0, 0]
    assert np.array_equal(ctx.kf_export_world([store], [1.0], 2), eo.points(clouds, poses, [1.0] * 4, 2))
    new = _poses(4, 12)
    store.set_poses(1, new[1:3])                                               # keyframes 1 and 2 move, 0 and 3 stay
    now = np.concatenate([poses[:1], new[1:3], poses[3:]])
    got = ctx.kf_export_world([store], [1.0], 2)
    assert np.array_equal(got, eo.points(clouds, now, [1.0] * 4, 2))
    assert not np.array_equal(got, eo.points(clouds, poses, [1.0] * 4, 2))
    for k in range(4):                                                         # nothing in the store changed
        g = store.get(k)
        assert g["exist"] == before[k]["exist"] and np.array_equal(g["x0"], now[k]) and g["n_points"] == len(clouds[k])
        assert np.array_equal(store.read(k)[0], clouds[k])
    assert store.history_size() == 2
    ctx.close()


@pytest.mark.parametrize("jump", [1, 3])
def test_windows(capi, edge, jump):
    ctx, store = edge["ctx"], edge["store"]
    full = _want(edge, jump)
    _, kb, _ = capi.kf_export_plan(EDGE_SIZES, 5_000_000, jump)
    total = int(kb[-1])
    mid4, mid7 = int(kb[4] + (kb[5] - kb[4]) // 2), int(kb[7] + (kb[8] - kb[7]) // 3)
    for begin, count in [(mid4, mid7 - mid4),        # from the middle of keyframe 4 to the middle of keyframe 7
                         (mid4, 1), (0, 1),          # one point
                         (mid7, 0), (total, 0),      # count = 0
                         (total - 1, 1),             # the last point alone
                         (int(kb[5]), int(kb[6] - kb[5])),   # exactly one keyframe
                         (0, total)]:
        got = ctx.kf_export_world([store], [3.0], jump, begin, count)
        assert got.shape == (count, 4)
        assert np.array_equal(got, full[begin:begin + count]), (begin, count)
    assert np.array_equal(ctx.kf_export_world([store], [3.0], jump, begin=mid7), full[mid7:])     # count None: up to the end


def test_messages(capi, edge):
    ctx, store = edge["ctx"], edge["store"]
    for jump in (0, 1, 2):
        j, kb, me = capi.kf_export_plan(store.sizes(), 300, jump)
        oj, okb, ome = eo.plan(EDGE_SIZES, 300, jump)
        assert j == oj and np.array_equal(kb, okb) and np.array_equal(me, ome)
        print("interval 300, jump %d -> %d: messages end at keyframes %s" % (jump, j, me.tolist()))
        assert len(me) >= 2
        parts, k0 = [], 0
        for m in me:
            parts.append(ctx.kf_export_world([store], [3.0], j, int(kb[k0]), int(kb[m] - kb[k0])))
            k0 = m
        assert np.array_equal(np.concatenate(parts), _want(edge, j))


def test_two_sessions(capi, edge):
    """a second store on a second context of the same device, exported on the first context"""
    ctx, store = edge["ctx"], edge["store"]
    ctx2 = _ctx(capi)
    sizes2 = [300, 0, 7, 513]
    store2, clouds2, poses2 = _edge_store(capi, ctx2, sizes2, 21)
    for jump in (1, 3):
        want = np.concatenate([_want(edge, jump, 4.0), eo.points(clouds2, poses2, [9.0] * 4, jump)])
        got = ctx.kf_export_world([store, store2], [4.0, 9.0], jump)
        n1 = len(_want(edge, jump))
        assert np.array_equal(got, want)
        assert (got[:n1, 3] == 4.0).all() and (got[n1:, 3] == 9.0).all() and len(got) > n1
        assert np.array_equal(ctx.kf_export_world([store, store2], [4.0, 9.0], jump, n1 - 5, 40), want[n1 - 5:n1 + 35])   # across the store boundary
        assert np.array_equal(ctx.kf_export_world([store, store2], [4.0, 9.0], jump, n1, 1), want[n1:n1 + 1])
        # the other order, and the plan over both stores' sizes
        got = ctx.kf_export_world([store2, store], [9.0, 4.0], jump)
        assert np.array_equal(got, np.concatenate([want[n1:], want[:n1]]))
        _, kb, _ = capi.kf_export_plan(np.concatenate([store.sizes(), store2.sizes()]), 5_000_000, jump)
        assert kb[-1] == len(want)
    ctx2.close()


def test_device_output(capi, edge):
    ctx, store = edge["ctx"], edge["store"]
    C = capi.C
    hip = _hip()
    host = ctx.kf_export_world([store], [3.0], 2, 100, 700)
    assert np.array_equal(host, _want(edge, 2)[100:800])
    buf = np.full((700 + 8, 4), SENT, dtype=np.float32)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(buf.nbytes)) == 0
    assert hip.hipMemcpy(d, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice
    assert ctx.kf_export_world([store], [3.0], 2, 100, 700, out=d) is None
    ctx.synchronize()
    assert hip.hipMemcpy(buf.ctypes.data_as(C.c_void_p), d, C.c_size_t(buf.nbytes), C.c_int(2)) == 0      # hipMemcpyDeviceToHost
    assert hip.hipFree(d) == 0
    assert np.array_equal(buf[:700], host)
    assert (buf[700:] == SENT).all()                                           # nothing past the window


def test_realistic_keyframes(capi, synth):
    path = synth.make_keyframe_path(n_kf=30, scans_per_kf=3, n_pts=6000)
    ctx = _ctx(capi)
    store = ctx.kf_store()
    for k, kf in enumerate(path):
        store.build(kf["points"], kf["poses"], 0.5 / 10, id=k, jour=float(k), vars=kf["vars"])
    clouds = [store.read(k)[0] for k in range(30)]
    poses = np.stack([store.get(k)["x0"] for k in range(30)])
    sizes = store.sizes()
    assert sizes.tolist() == [len(c) for c in clouds] and sizes.min() > 256
    interval = int(sizes.sum()) // 45                      # the reference's rule at this interval: jump = 45 // 10 + 1 = 5
    j, kb, me = capi.kf_export_plan(sizes, interval, 0)
    oj, okb, ome = eo.plan(sizes, interval, 0)
    print("%d points in 30 keyframes, interval %d -> jump %d, %d messages" % (sizes.sum(), interval, j, len(me)))
    assert j == oj == 5 and np.array_equal(kb, okb) and np.array_equal(me, ome)
    for jump in (1, j):
        got = ctx.kf_export_world([store], [2.0], jump)
        assert np.array_equal(got, eo.points(clouds, poses, [2.0] * 30, jump))
    ctx.close()


def test_beyond_one_grid_and_one_staging_pass(capi):
    """The two sizes at which the code takes another path: more than 2048 x 256 = 524 288 records in one launch (the capped grid
    strides over the rest) and more than 2^22 = 4 194 304 records to host memory (a second pass through the staging buffer).
    16 keyframes of ~270 000 random points kept at 1 mm voxels."""
    rng = np.random.default_rng(31)
    ctx = _ctx(capi)
    store = ctx.kf_store()
    poses = _poses(16, 32)
    store.reserve(points=4_400_000, keyframes=16, merge_points=271_000)
    for k in range(16):
        store.build([rng.uniform(-30, 30, (270_000 + 17 * k, 3))], poses[k:k + 1], 0.001, id=k, jour=0.0)
    clouds = [store.read(k)[0] for k in range(16)]
    total = sum(len(c) for c in clouds)
    print("%d points resident" % total)
    assert total > (1 << 22) + 8192
    want = eo.points(clouds, poses, [6.0] * 16, 1)
    assert np.array_equal(ctx.kf_export_world([store], [6.0], 1), want)                                  # two passes, each grid-strided
    assert np.array_equal(ctx.kf_export_world([store], [6.0], 1, 1000, (1 << 22) + 5000), want[1000:1000 + (1 << 22) + 5000])
    got = ctx.kf_export_world([store], [6.0], 3)                                                         # one pass, grid-strided
    assert len(got) > 2048 * 256 and np.array_equal(got, eo.points(clouds, poses, [6.0] * 16, 3))
    ctx.close()


def test_refusals(capi, edge):
    ctx, store = edge["ctx"], edge["store"]
    C = capi.C
    lib = ctx.lib
    total = sum(-(-n // 2) for n in EDGE_SIZES)
    one = (C.c_void_p * 1)(store.h.value)
    null_store = (C.c_void_p * 1)(None)
    inten = (C.c_float * 1)(3.0)
    buf = np.full((total + 4, 4), SENT, dtype=np.float32)
    out = buf.ctypes.data_as(C.c_void_p)

    def call(n_stores=1, stores=one, intensity=inten, jump=2, begin=0, count=total, xyzi=out):
        return lib.vba_kf_export_world(ctx.h, C.c_int(n_stores), stores, intensity, C.c_int(jump), C.c_int64(begin), C.c_int64(count), xyzi)

    cases = {
        "n_stores < 1": dict(n_stores=0),
        "n_stores negative": dict(n_stores=-1),
        "a NULL store": dict(stores=null_store),
        "NULL stores": dict(stores=None),
        "NULL intensity": dict(intensity=None),
        "jump < 1": dict(jump=0),
        "jump negative": dict(jump=-2),
        "begin < 0": dict(begin=-1, count=5),
        "count < 0": dict(count=-1),
        "begin + count beyond the total": dict(begin=1, count=total),
        "begin beyond the total": dict(begin=total + 1, count=0),
        "count beyond the total": dict(count=total + 1),
        "count > 0 with a NULL xyzi": dict(xyzi=None),
    }
    for what, kw in cases.items():
        assert call(**kw) == capi.ERR_BAD_ARG, what
        assert (buf == SENT).all(), what
    assert call(count=0) == 0 and call(begin=total, count=0) == 0 and call(count=0, xyzi=None) == 0      # count == 0 does nothing
    assert (buf == SENT).all()
    assert call() == 0                                                         # and the same arguments unrefused do export
    assert np.array_equal(buf[:total], _want(edge, 2)) and (buf[total:] == SENT).all()
