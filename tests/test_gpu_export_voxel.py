"""The voxel-down-sampled global map (vba_kf_voxel_export) on the MI355X against the numpy restatement
tests/export_voxel_ref.py, which tests/test_export_voxel_cpu.py holds to the CPU oracle.

Bars.  A deterministic context forms every sum as the restatement does, a chain in sequence order, so xyzi, counts and n_out are
np.array_equal and two calls are equal byte for byte.  A default context may add in any order: two f64 sums of the same cnt < 2^26
floats differ by less than 2 cnt 2^-53 sum|a|, far below half a float ulp, so after the narrowing every coordinate is the
restatement's float or an adjacent one; voxel set, order, counts and intensity are equal."""
import os
import struct
import subprocess

import numpy as np
import pytest

import export_voxel_ref as ev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.float32(-12345.5)
ISENT = np.int32(-777)


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


def _ctx(capi, det):
    o = capi.default_options()
    o.device = 0
    o.deterministic = 1 if det else 0
    return capi.Context(o)


def _hip():
    """the HIP runtime libvoxelba.so has already loaded (for device buffers of the test's own)"""
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _build(ctx, clouds, poses):
    """a store whose keyframe k holds clouds[k] as given: one scan each, points far enough apart to be alone in a 0.05 voxel"""
    store = ctx.kf_store()
    for k, c in enumerate(clouds):
        kept, _, _ = store.build([c], poses[k:k + 1], 0.05, id=k, jour=float(k))
        assert kept == len(c)
    kept = [store.read(k)[0] for k in range(len(clouds))]
    assert all(np.array_equal(a, b) for a, b in zip(kept, clouds))
    return store


@pytest.fixture(scope="module")
def world(capi):
    """the edge store of tests/test_gpu_export.py with its poses (far: translations of +-40 m) and with translations within +-2 m
    (near: the keyframes overlap), on a default and a deterministic context of the device"""
    ctxs = {False: _ctx(capi, False), True: _ctx(capi, True)}
    clouds = ev.edge_clouds()
    w = dict(ctx=ctxs, clouds=clouds, stores={}, poses={}, hip=_hip())
    for name, spread in (("far", 40.0), ("near", 2.0)):
        w["poses"][name] = ev.edge_poses(len(clouds), 5, spread)
        w["stores"][name] = _build(ctxs[False], clouds, w["poses"][name])
    yield w
    for c in ctxs.values():
        c.close()


def _adjacent_or_equal(got, want):
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


def _check(ctx, det, stores, intensity, sessions, jump, voxel, min_count=1, what=""):
    want, wcnt, _ = ev.export_voxel(sessions, jump, voxel, min_count)
    got, cnt = ctx.kf_export_voxel(stores, intensity, jump, voxel, min_count)
    assert got.dtype == np.float32 and cnt.dtype == np.int32 and got.shape == want.shape and cnt.shape == wcnt.shape
    assert np.array_equal(cnt, wcnt) and np.array_equal(got[:, 3], want[:, 3])
    unequal = int((got[:, :3] != want[:, :3]).sum())
    print("%s %s jump %d voxel %g min_count %d: %d voxels, %d coordinates differ from the restatement"
          % (what, "deterministic" if det else "default", jump, voxel, min_count, len(got), unequal))
    if det:
        assert np.array_equal(got, want)
        again, cnt2 = ctx.kf_export_voxel(stores, intensity, jump, voxel, min_count)
        assert got.tobytes() == again.tobytes() and cnt.tobytes() == cnt2.tobytes()
    else:
        assert _adjacent_or_equal(got[:, :3], want[:, :3]).all()
    return got, cnt


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("name", ["far", "near"])
@pytest.mark.parametrize("jump", [1, 3])
def test_edge_store(world, det, name, jump):
    sessions = [(world["clouds"], world["poses"][name], 3.0)]
    for voxel in (0.5, 2.0, 4.0, 1000.0):
        _check(world["ctx"][det], det, [world["stores"][name]], [3.0], sessions, jump, voxel, what=name)


def test_the_stores_exercise_shared_voxels(world):
    """the conditions the restatement must meet on these inputs: voxels of many records, fed from several keyframes (and so from
    several workgroups: the keyframes of 255 to 1000 records lie in different workgroups)"""
    near = [(world["clouds"], world["poses"]["near"], 3.0)]
    far = [(world["clouds"], world["poses"]["far"], 3.0)]
    vox, multi, span, big = ev.voxel_census(near, 1, 2.0)
    assert (vox, multi, span, big) == (679, 449, 336, 8) and 2 * span >= multi
    vox, multi, span, big = ev.voxel_census(near, 1, 4.0)
    assert (vox, span, big) == (148, 108, 36) and 2 * span >= multi
    vox, multi, span, big = ev.voxel_census(far, 1, 1000.0)
    assert (vox, span, big) == (6, 4, 556)


@pytest.mark.parametrize("det", [True, False])
def test_min_count(world, det):
    ctx, store = world["ctx"][det], world["stores"]["near"]
    sessions = [(world["clouds"], world["poses"]["near"], 3.0)]
    full, fcnt = _check(ctx, det, [store], [3.0], sessions, 1, 2.0, 1, "near")
    kept, kcnt = _check(ctx, det, [store], [3.0], sessions, 1, 2.0, 3, "near")
    assert len(full) == 679 and len(kept) == 316
    assert np.array_equal(kcnt, fcnt[fcnt >= 3])                              # the order of the kept voxels is unchanged
    if det:
        assert np.array_equal(kept, full[fcnt >= 3])
    assert ctx.kf_export_voxel_size([store], [3.0], 1, 2.0, 3) == 316 and ctx.kf_export_voxel_size([store], [3.0], 1, 2.0, 9) == 0


@pytest.mark.parametrize("det", [True, False])
def test_boundary_grid(world, det):
    """The grid of the CPU test's key boundaries at the identity pose.  (x, y, -0.0) and (x, y, 0.0) are one voxel for the store's
    own down-sampler at any size, so the -0.0 layer is a keyframe of its own: every point is kept."""
    ctx = world["ctx"][det]
    g = ev.boundary_grid()
    neg = np.signbit(g[:, 2]) & (g[:, 2] == 0)
    clouds = [g[~neg], g[neg]]
    assert len(clouds[0]) == 1875 and len(clouds[1]) == 625
    poses = np.stack([ev.IDENTITY, ev.IDENTITY])
    store = _build(world["ctx"][False], clouds, poses)
    sessions = [(clouds, poses, 1.0)]
    for voxel, n_vox in [(1.0, 128), (0.25, 1875)]:
        got, cnt = _check(ctx, det, [store], [1.0], sessions, 1, voxel, what="grid")
        assert len(got) == n_vox and cnt.sum() == 2500


@pytest.mark.parametrize("det", [True, False])
def test_two_stores(capi, world, det):
    ctx = world["ctx"][det]
    clouds, poses = world["clouds"], world["poses"]["near"]
    a = world["stores"]["near"]
    ctx2 = _ctx(capi, False)                                                   # the second store hangs off another context of the device
    b = _build(ctx2, clouds, poses)
    one, cnt1 = _check(ctx, det, [a], [1.0], [(clouds, poses, 1.0)], 1, 2.0, what="one store")
    two, cnt2 = _check(ctx, det, [a, b], [1.0, 2.0], [(clouds, poses, 1.0), (clouds, poses, 2.0)], 1, 2.0, what="two stores")
    assert np.array_equal(cnt2, 2 * cnt1) and (two[:, 3] == 1.0).all() and len(two) == len(one)   # every count doubles, store 0 is first
    assert _adjacent_or_equal(two[:, :3], one[:, :3]).all()                  # and the order is that of store 0
    # the result follows set_poses; nothing in the stores changes
    before = [b.get(k) for k in range(len(clouds))]
    new = ev.edge_poses(len(clouds), 9, 2.0)
    b.set_poses(2, new[2:6])
    now = np.concatenate([poses[:2], new[2:6], poses[6:]])
    moved, _ = _check(ctx, det, [a, b], [1.0, 2.0], [(clouds, poses, 1.0), (clouds, now, 2.0)], 1, 2.0, what="after set_poses")
    assert moved.shape != two.shape or not np.array_equal(moved, two)
    for k in range(len(clouds)):
        g = b.get(k)
        assert g["exist"] == before[k]["exist"] and np.array_equal(g["x0"], now[k]) and g["n_points"] == len(clouds[k])
        assert np.array_equal(b.read(k)[0], clouds[k]) and np.array_equal(a.read(k)[0], clouds[k])
    ctx2.close()


def _dev(hip, C, arr):
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(arr.nbytes)) == 0
    assert hip.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice
    return d


def _back(hip, C, d, arr):
    assert hip.hipMemcpy(arr.ctypes.data_as(C.c_void_p), d, C.c_size_t(arr.nbytes), C.c_int(2)) == 0      # hipMemcpyDeviceToHost


@pytest.mark.parametrize("det", [True, False])
def test_output_sides_and_capacity(capi, world, det):
    ctx, store, hip, C = world["ctx"][det], world["stores"]["near"], world["hip"], capi.C
    lib = ctx.lib
    host, hcnt = ctx.kf_export_voxel([store], [3.0], 1, 2.0)
    m = len(host)
    assert m == 679 and ctx.kf_export_voxel_size([store], [3.0], 1, 2.0) == m
    # device buffers with room for 8 more records: the sentinel behind n_out records is untouched
    xb = np.full((m + 8, 4), SENT, dtype=np.float32); cb = np.full(m + 8, ISENT, dtype=np.int32)
    dx, dc = _dev(hip, C, xb), _dev(hip, C, cb)
    assert ctx.kf_export_voxel([store], [3.0], 1, 2.0, cap=m + 8, out=(dx, dc)) == m
    ctx.synchronize()
    _back(hip, C, dx, xb); _back(hip, C, dc, cb)
    assert np.array_equal(cb[:m], hcnt) and (cb[m:] == ISENT).all() and (xb[m:] == SENT).all()
    assert np.array_equal(xb[:m], host) if det else _adjacent_or_equal(xb[:m], host).all()
    # counts may be NULL, on both sides; cap == n_out is enough
    xb2 = np.full((m + 1, 4), SENT, dtype=np.float32)
    assert ctx.kf_export_voxel([store], [3.0], 1, 2.0, cap=m, out=(xb2.ctypes.data_as(C.c_void_p), None)) == m
    assert (xb2[m] == SENT).all() and np.array_equal(xb2[:m, 3], host[:, 3])
    # one record too few: VBA_ERR_CAPACITY, *n_out says what is needed, nothing is written on either side
    one = (C.c_void_p * 1)(store.h.value)
    inten = (C.c_float * 1)(3.0)
    n = C.c_int64(-1)
    xh = np.full((m, 4), SENT, dtype=np.float32); ch = np.full(m, ISENT, dtype=np.int32)
    st = lib.vba_kf_voxel_export(ctx.h, 1, one, inten, 1, 2.0, 1, m - 1, xh.ctypes.data_as(C.c_void_p), ch.ctypes.data_as(C.c_void_p), C.byref(n))
    assert st == capi.ERR_CAPACITY and n.value == m and (xh == SENT).all() and (ch == ISENT).all()
    xb[:] = SENT; cb[:] = ISENT
    assert hip.hipMemcpy(dx, xb.ctypes.data_as(C.c_void_p), C.c_size_t(xb.nbytes), C.c_int(1)) == 0
    assert hip.hipMemcpy(dc, cb.ctypes.data_as(C.c_void_p), C.c_size_t(cb.nbytes), C.c_int(1)) == 0
    n = C.c_int64(-1)
    assert lib.vba_kf_voxel_export(ctx.h, 1, one, inten, 1, 2.0, 1, m - 1, dx, dc, C.byref(n)) == capi.ERR_CAPACITY and n.value == m
    ctx.synchronize()
    _back(hip, C, dx, xb); _back(hip, C, dc, cb)
    assert (xb == SENT).all() and (cb == ISENT).all()
    # cap == 0 with a buffer is no size query
    n = C.c_int64(-1)
    assert lib.vba_kf_voxel_export(ctx.h, 1, one, inten, 1, 2.0, 1, 0, xh.ctypes.data_as(C.c_void_p), None, C.byref(n)) == capi.ERR_CAPACITY and n.value == m
    assert (xh == SENT).all()

    # ---- every refusal, outputs untouched
    def call(n_stores=1, stores=one, intensity=inten, jump=1, voxel=2.0, min_count=1, cap=m, xyzi=xh.ctypes.data_as(C.c_void_p),
             counts=ch.ctypes.data_as(C.c_void_p), n_out=C.byref(n)):
        return lib.vba_kf_voxel_export(ctx.h, n_stores, stores, intensity, jump, voxel, min_count, cap, xyzi, counts, n_out)

    null_store = (C.c_void_p * 1)(None)
    cases = {
        "n_stores < 1": dict(n_stores=0), "n_stores negative": dict(n_stores=-1), "a NULL store": dict(stores=null_store),
        "NULL stores": dict(stores=None), "NULL intensity": dict(intensity=None), "jump < 1": dict(jump=0), "jump negative": dict(jump=-3),
        "min_count < 1": dict(min_count=0), "cap < 0": dict(cap=-1), "a NULL n_out": dict(n_out=None), "cap > 0 with a NULL xyzi": dict(xyzi=None),
        "voxel_size < 0.001": dict(voxel=0.0009), "voxel_size 0": dict(voxel=0.0), "voxel_size negative": dict(voxel=-1.0),
        "voxel_size NaN": dict(voxel=float("nan")),
        "a misaligned device xyzi": dict(xyzi=C.c_void_p(dx.value + 4), counts=dc),
        "device xyzi with host counts": dict(xyzi=dx),
    }
    import torch
    if torch.cuda.device_count() > 1:                                         # another device
        o = capi.default_options(); o.device = 1
        other = capi.Context(o)
        cases["a store of another device"] = dict(stores=(C.c_void_p * 1)(other.kf_store().h.value))
    for what, kw in cases.items():
        n.value = -1
        assert call(**kw) == capi.ERR_BAD_ARG, what
        assert n.value == -1 and (xh == SENT).all() and (ch == ISENT).all(), what
    ctx.synchronize()
    _back(hip, C, dx, xb); _back(hip, C, dc, cb)
    assert (xb == SENT).all() and (cb == ISENT).all()
    assert call() == 0 and n.value == m and np.array_equal(ch, hcnt)         # the same arguments unrefused do export
    assert hip.hipFree(dx) == 0 and hip.hipFree(dc) == 0
    with pytest.raises(capi.VbaError) as e:                                   # an empty list of stores is n_stores < 1
        ctx.kf_export_voxel([], [], 1, 2.0, cap=4)
    assert e.value.status == capi.ERR_BAD_ARG


def test_nothing_to_export(capi, world):
    ctx = world["ctx"][True]
    empty = world["ctx"][False].kf_store()                                    # no keyframes
    hollow = _build(world["ctx"][False], [np.zeros((0, 3))] * 3, ev.edge_poses(3, 1, 2.0))      # keyframes without points
    for stores in ([empty], [hollow], [empty, hollow]):
        got, cnt = ctx.kf_export_voxel(stores, [1.0] * len(stores), 1, 2.0, cap=4)
        assert got.shape == (0, 4) and cnt.shape == (0,)
        assert ctx.kf_export_voxel_size(stores, [1.0] * len(stores), 2, 0.5) == 0
    # empty keyframes and stores between full ones change nothing
    near = world["stores"]["near"]
    a = ctx.kf_export_voxel([near], [3.0], 1, 2.0)
    b = ctx.kf_export_voxel([empty, hollow, near, hollow], [7.0, 8.0, 3.0, 9.0], 1, 2.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_cross_check_with_the_scan_down_sampler(world):
    """two device paths of one deterministic context: the fused call, and vba_kf_export_world to the host, widened, through
    down_sampling_voxel"""
    ctx, store = world["ctx"][True], world["stores"]["near"]
    for jump in (1, 3):
        S = ctx.kf_export_world([store], [3.0], jump)
        pnt, cnt, first = ctx.down_sampling_voxel(S[:, :3].astype(np.float64), 2.0)
        got, gcnt = ctx.kf_export_voxel([store], [3.0], jump, 2.0)
        assert np.array_equal(gcnt, cnt) and np.array_equal(got[:, :3].astype(np.float64), pnt) and np.array_equal(got[:, 3], S[first, 3])


@pytest.mark.parametrize("det", [True, False])
def test_no_allocation_after_reserve(capi, world, det):
    ctx, hip, C = _ctx(capi, det), world["hip"], capi.C
    assert ctx.kf_export_voxel_allocations() == (0, 0)
    total = sum(ev.EDGE_SIZES)
    ctx.kf_export_voxel_reserve(2 * total)
    base = ctx.kf_export_voxel_allocations()
    assert base[0] >= 5 and base[1] >= 2 * total * (4 + 2 * 16 + 2 * 24)    # slot, table and sums at the least
    ctx.kf_export_voxel_reserve(total)                                        # less than is held: nothing happens
    near, far = world["stores"]["near"], world["stores"]["far"]
    xb = np.zeros((2 * total, 4), dtype=np.float32); cb = np.zeros(2 * total, dtype=np.int32)
    dx, dc = _dev(hip, C, xb), _dev(hip, C, cb)
    for jump in (1, 3):
        for voxel in (0.5, 2.0, 1000.0):
            ctx.kf_export_voxel([near], [3.0], jump, voxel)
            ctx.kf_export_voxel([near, far], [3.0, 4.0], jump, voxel, min_count=2)
            ctx.kf_export_voxel([far, near], [3.0, 4.0], jump, voxel, cap=2 * total, out=(dx, dc))
            ctx.kf_export_voxel_size([far], [3.0], jump, voxel)
    ctx.synchronize()
    assert ctx.kf_export_voxel_allocations() == base
    # a longer sequence than was reserved grows the arrays (by doubling), and the result is the same
    three = [(world["clouds"], world["poses"][k], it) for k, it in (("near", 3.0), ("far", 4.0), ("near", 5.0))]
    _check(ctx, det, [near, far, near], [3.0, 4.0, 5.0], three, 1, 2.0, what="grown")
    grown = ctx.kf_export_voxel_allocations()
    assert grown[0] > base[0] and grown[1] > base[1]
    assert hip.hipFree(dx) == 0 and hip.hipFree(dc) == 0
    ctx.close()


def test_adapter_program(capi, world, tmp_path):
    """vba::pub_globalmap_voxel through tests/host/export_voxel_host.cpp: its messages, concatenated, are the Python result"""
    exe = str(tmp_path / "export_voxel_host")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "export_voxel_host.cpp"),
                           "-o", exe, "-L", libdir, "-lvoxelba", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    clouds = world["clouds"]
    sessions = [(clouds, world["poses"]["near"]), (clouds[:6], world["poses"]["far"][:6])]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(sessions)))
        for cl, ps in sessions:
            f.write(struct.pack("<i", len(cl)))
            for c, x in zip(cl, ps):
                f.write(struct.pack("<i", len(c))); f.write(np.ascontiguousarray(x, dtype=np.float64).tobytes())
                f.write(np.ascontiguousarray(c, dtype=np.float64).tobytes())
    ctx = world["ctx"][True]
    b = _build(world["ctx"][False], clouds[:6], world["poses"]["far"][:6])
    for min_count, interval in ((1, 100), (3, 5_000_000)):
        want, _ = ctx.kf_export_voxel([world["stores"]["near"], b], [0.0, 1.0], 1, 2.0, min_count)
        r = subprocess.run([exe, "gpu", fin, fout, "2.0", str(min_count), str(interval), "1", "1"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        raw = open(fout, "rb").read()
        msgs, q = [], 0
        while q < len(raw):
            n = struct.unpack_from("<q", raw, q)[0]; q += 8
            msgs.append(np.frombuffer(raw, dtype=np.float32, count=4 * n, offset=q).reshape(n, 4)); q += 16 * n
        ends = ev.message_ends(len(want), interval)
        print("min_count %d interval %d: %d records in %d messages" % (min_count, interval, len(want), len(msgs)))
        assert [len(x) for x in msgs] == [e - s for s, e in zip([0] + ends[:-1], ends)] and len(msgs) >= 1
        assert r.stdout.split() == ["records", str(len(want)), "messages", str(len(msgs))]
        assert np.array_equal(np.concatenate(msgs), want) and len(want) > 100
