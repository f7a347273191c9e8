"""The surfel export of the global map (vba_kf_surfel_export) on the MI355X against the numpy restatement
tests/surfel_ref.py, which tests/test_export_surfel_cpu.py holds to a 60-digit reference, and against a host build of the fit header
(tests/host/export_surfel_host.cpp).

Bars.  A deterministic context forms every sum as the restatement does, a chain in sequence order, and fits with correctly rounded
operations only: counts, order, cov and the records are np.array_equal, [0..3] equal vba_kf_voxel_export's, two calls are equal byte
for byte.  A default context may add in any order: set, order and counts are equal; every cov entry is within surfel_ref.cov_bar (a
count of roundings, any order) of the exact covariance of the float records; the eigen fields of a record are within the bars of
eig3_ref.check, carried to floats by surfel_ref.check_record, of the decomposition of the cov the device returned; every normal of a
voxel of three records or more points to the sensor, and agrees in sign with the restatement's wherever it is determined."""
import struct
import subprocess

import numpy as np
import pytest

import eig3_ref as er
import export_voxel_ref as ev
import surfel_ref as sr

pytestmark = pytest.mark.gpu

SENT = np.float32(-12345.5)
DSENT = -54321.25
ISENT = np.int32(-777)
VOXELS = (0.5, 1.0)


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
    """a store whose keyframe k holds clouds[k] as given: one scan each, every point alone in a build voxel of surfel_ref.GRID"""
    store = ctx.kf_store()
    for k, c in enumerate(clouds):
        kept, _, _ = store.build([c], poses[k:k + 1], sr.GRID, id=k, jour=float(k))
        assert kept == len(c)
    kept = [store.read(k)[0] for k in range(len(clouds))]
    assert all(np.array_equal(a, b) for a, b in zip(kept, clouds))
    return store


@pytest.fixture(scope="module")
def world(capi, tmp_path_factory):
    """the scene of surfel_ref under its poses (near) and shifted by about 1000 m (far), on a default and a deterministic context of
    the device; the host build of the fit; a cache of restated results, computed once per case"""
    ctxs = {False: _ctx(capi, False), True: _ctx(capi, True)}
    clouds, poses = sr.scene()
    d = tmp_path_factory.mktemp("export_surfel_gpu")
    exe = sr.build_host(d, capi.LIB_PATH)
    w = dict(ctx=ctxs, clouds=clouds, stores={}, poses={"near": poses, "far": sr.shifted(poses)}, hip=_hip(), exe=exe, dir=d,
             fit=sr.host_solver(exe, d), cache={})
    for name in ("near", "far"):
        w["stores"][name] = _build(ctxs[False], clouds, w["poses"][name])
    yield w
    for c in ctxs.values():
        c.close()


def _want(world, key, sessions, jump, voxel):
    """the restatement of every voxel (min_count 1) with the exact covariance and its bar, cached under `key`"""
    k = (key, jump, voxel)
    if k not in world["cache"]:
        S, kf = ev.sequence(sessions, jump)
        mo = sr.moments(S, voxel)
        rec, C, cnt = sr.surfels(sessions, jump, voxel, 1, world["fit"])
        _, cov, D, A = sr.exact(S, mo["first"], mo["cnt"], mo["vox"])
        world["cache"][k] = dict(rec=rec, C=C, cnt=cnt, exact=cov, bar=sr.cov_bar(mo["cnt"], D, A),
                                 sensor=sr.sensors(sessions, kf, mo["first"]), c=mo["c"])
    return world["cache"][k]


def _adjacent_or_equal(got, want):
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


def _check(world, det, stores, intensity, key, sessions, jump, voxel, min_count, what=""):
    ctx = world["ctx"][det]
    ref = _want(world, key, sessions, jump, voxel)
    keep = ref["cnt"] >= min_count
    wrec, wC, wcnt = ref["rec"][keep], ref["C"][keep], ref["cnt"][keep]
    rec, cov, cnt = ctx.kf_export_surfel(stores, intensity, jump, voxel, min_count)
    assert rec.dtype == np.float32 and cov.dtype == np.float64 and cnt.dtype == np.int32
    assert rec.shape == wrec.shape and cov.shape == wC.shape and cnt.shape == wcnt.shape
    # set, order, counts: the voxel export's and the restatement's
    xyzi, vcnt = ctx.kf_export_voxel(stores, intensity, jump, voxel, min_count)
    assert np.array_equal(cnt, wcnt) and np.array_equal(cnt, vcnt) and np.array_equal(rec[:, 3], wrec[:, 3]) and np.array_equal(rec[:, 3], xyzi[:, 3])
    assert np.array_equal(rec[:, 11], cnt.astype(np.float32))
    assert ctx.kf_export_surfel_size(stores, intensity, jump, voxel, min_count) == len(rec)
    if det:
        assert np.array_equal(rec[:, :4], xyzi)
        assert np.array_equal(cov, wC)
        assert np.array_equal(rec, wrec)
        rec2, cov2, cnt2 = ctx.kf_export_surfel(stores, intensity, jump, voxel, min_count)
        assert rec.tobytes() == rec2.tobytes() and cov.tobytes() == cov2.tobytes() and cnt.tobytes() == cnt2.tobytes()
        print("%s deterministic jump %d voxel %g min_count %d: %d surfels, bit for bit" % (what, jump, voxel, min_count, len(rec)))
        return rec, cov, cnt
    assert _adjacent_or_equal(rec[:, :3], wrec[:, :3]).all()
    ratio = np.abs(cov - ref["exact"][keep]) / ref["bar"][keep]
    worst = {}
    big = cnt >= 3
    determined = np.zeros(len(rec), dtype=bool)
    for v in range(len(rec)):
        ref_v = er.Ref(sr.sym(cov[v]))                                         # of the covariance the device fitted
        for k, r in sr.check_record(cov[v], rec[v], cnt[v], ref_v).items():
            worst[k] = max(worst.get(k, 0.0), r)
        determined[v] = big[v] and not _degenerate(ref_v)
    los = ref["sensor"][keep] - ref["c"][keep]
    toward = np.einsum("ij,ij->i", rec[:, 4:7].astype(np.float64), los)
    agree = np.einsum("ij,ij->i", rec[:, 4:7].astype(np.float64), wrec[:, 4:7].astype(np.float64))
    print("%s default jump %d voxel %g min_count %d: %d surfels, %d cov entries differ from the restatement, worst cov error / bar %.3g, "
          "worst eigen ratios %s, %d normals determined" % (what, jump, voxel, min_count, len(rec), int((cov != wC).sum()), ratio.max() if len(rec) else 0.0,
                                                            {k: "%.3g" % r for k, r in worst.items()}, determined.sum()))
    assert (ratio <= 1.0).all()
    assert not worst or max(worst.values()) <= 1.0
    assert (toward[big] > 0).all() and not rec[~big, 4:7].any()
    assert (agree[determined] > 0.99).all()
    return rec, cov, cnt


def _degenerate(ref):
    """the smallest eigenvalue belongs to a close pair or a triple, or its gap is below 1e3 bars: its vector is not determined"""
    if ref.s == 0.0:
        return True
    return ref.triple or (ref.pair is not None and 0 in ref.pair[:2]) or er.C_BAR * er.EPS * ref.s / max(ref.gap[0], er.TINY) > 1e-3


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("jump", [1, 3])
def test_scene(world, det, name, jump):
    sessions = [(world["clouds"], world["poses"][name], 3.0)]
    for voxel in VOXELS:
        full = _check(world, det, [world["stores"][name]], [3.0], name, sessions, jump, voxel, 1, name)
        kept = _check(world, det, [world["stores"][name]], [3.0], name, sessions, jump, voxel, 3, name)
        assert len(kept[0]) < len(full[0]) and np.array_equal(kept[2], full[2][full[2] >= 3])      # the order of the kept voxels is unchanged
        if det:
            assert np.array_equal(kept[0], full[0][full[2] >= 3]) and np.array_equal(kept[1], full[1][full[2] >= 3])


@pytest.mark.parametrize("det", [True, False])
def test_two_stores(capi, world, det):
    clouds, poses = world["clouds"], world["poses"]["near"]
    a = world["stores"]["near"]
    ctx2 = _ctx(capi, False)                                                   # the second store hangs off another context of the device
    moved = np.array(poses)
    moved[:, 9:12] += np.array([0.125, -0.25, 0.0625])
    b = _build(ctx2, clouds, moved)
    two = [(clouds, poses, 1.0), (clouds, moved, 2.0)]
    r2 = _check(world, det, [a, b], [1.0, 2.0], "two", two, 1, 0.5, 3, "two stores")
    assert (r2[0][:, 3] == 1.0).sum() > 100 and (r2[0][:, 3] == 2.0).sum() >= 1
    # the result follows set_poses; nothing in the stores changes
    again = np.array(moved)
    again[2:5, 9:12] += np.array([0.5, 0.25, -0.375])
    b.set_poses(2, again[2:5])
    now = [(clouds, poses, 1.0), (clouds, again, 2.0)]
    r3 = _check(world, det, [a, b], [1.0, 2.0], "two moved", now, 1, 0.5, 3, "after set_poses")
    assert r3[0].shape != r2[0].shape or not np.array_equal(r3[0], r2[0])
    for k in range(len(clouds)):
        assert np.array_equal(b.get(k)["x0"], again[k]) and np.array_equal(b.read(k)[0], clouds[k]) and np.array_equal(a.read(k)[0], clouds[k])
    ctx2.close()


def _dev(hip, C, arr):
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(arr.nbytes)) == 0
    assert hip.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice
    return d


def _up(hip, C, d, arr):
    assert hip.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), C.c_int(1)) == 0


def _back(hip, C, d, arr):
    assert hip.hipMemcpy(arr.ctypes.data_as(C.c_void_p), d, C.c_size_t(arr.nbytes), C.c_int(2)) == 0      # hipMemcpyDeviceToHost


@pytest.mark.parametrize("det", [True, False])
def test_output_sides_and_capacity(capi, world, det):
    ctx, store, hip, C = world["ctx"][det], world["stores"]["far"], world["hip"], capi.C
    lib = ctx.lib
    host, hcov, hcnt = ctx.kf_export_surfel([store], [3.0], 1, 0.5, 1)
    m = len(host)
    assert m == 183 and ctx.kf_export_surfel_size([store], [3.0], 1, 0.5, 1) == m

    def same(got, want):
        return np.array_equal(got, want) if det else np.allclose(got, want, rtol=1e-3, atol=1e-6)   # (default mode: _check holds the bars)

    # device buffers with room for 8 more records: the sentinel behind n_out records is untouched
    xb = np.full((m + 8, 12), SENT, dtype=np.float32); vb = np.full((m + 8, 6), DSENT, dtype=np.float64); cb = np.full(m + 8, ISENT, dtype=np.int32)
    dx, dv, dc = _dev(hip, C, xb), _dev(hip, C, vb), _dev(hip, C, cb)
    assert ctx.kf_export_surfel([store], [3.0], 1, 0.5, 1, cap=m + 8, out=(dx, dv, dc)) == m
    ctx.synchronize()
    _back(hip, C, dx, xb); _back(hip, C, dv, vb); _back(hip, C, dc, cb)
    assert np.array_equal(cb[:m], hcnt) and (cb[m:] == ISENT).all() and (xb[m:] == SENT).all() and (vb[m:] == DSENT).all()
    assert same(xb[:m], host) and same(vb[:m], hcov) and np.array_equal(xb[:m, [3, 11]], host[:, [3, 11]])
    # cov and counts may be NULL, together or alone, on both sides; cap == n_out is enough
    for want_cov, want_cnt in ((False, False), (True, False), (False, True)):
        xb[:] = SENT; vb[:] = DSENT; cb[:] = ISENT
        _up(hip, C, dx, xb); _up(hip, C, dv, vb); _up(hip, C, dc, cb)
        assert ctx.kf_export_surfel([store], [3.0], 1, 0.5, 1, cap=m, out=(dx, dv if want_cov else None, dc if want_cnt else None)) == m
        ctx.synchronize()
        _back(hip, C, dx, xb); _back(hip, C, dv, vb); _back(hip, C, dc, cb)
        assert same(xb[:m], host) and (xb[m:] == SENT).all()
        assert (same(vb[:m], hcov) and (vb[m:] == DSENT).all()) if want_cov else (vb == DSENT).all()
        assert (np.array_equal(cb[:m], hcnt) and (cb[m:] == ISENT).all()) if want_cnt else (cb == ISENT).all()
        r, v, c = ctx.kf_export_surfel([store], [3.0], 1, 0.5, 1, cap=m, want_cov=want_cov, want_counts=want_cnt)
        assert same(r, host) and (v is None if not want_cov else same(v, hcov)) and (c is None if not want_cnt else np.array_equal(c, hcnt))
    # one record too few: VBA_ERR_CAPACITY, *n_out says what is needed, nothing is written on either side
    one = (C.c_void_p * 1)(store.h.value)
    inten = (C.c_float * 1)(3.0)
    n = C.c_int64(-1)
    xh = np.full((m, 12), SENT, dtype=np.float32); vh = np.full((m, 6), DSENT, dtype=np.float64); ch = np.full(m, ISENT, dtype=np.int32)
    px, pv, pc = xh.ctypes.data_as(C.c_void_p), vh.ctypes.data_as(C.c_void_p), ch.ctypes.data_as(C.c_void_p)
    assert lib.vba_kf_surfel_export(ctx.h, 1, one, inten, 1, 0.5, 1, m - 1, px, pv, pc, C.byref(n)) == capi.ERR_CAPACITY
    assert n.value == m and (xh == SENT).all() and (vh == DSENT).all() and (ch == ISENT).all()
    xb[:] = SENT; vb[:] = DSENT; cb[:] = ISENT
    _up(hip, C, dx, xb); _up(hip, C, dv, vb); _up(hip, C, dc, cb)
    n = C.c_int64(-1)
    assert lib.vba_kf_surfel_export(ctx.h, 1, one, inten, 1, 0.5, 1, m - 1, dx, dv, dc, C.byref(n)) == capi.ERR_CAPACITY and n.value == m
    ctx.synchronize()
    _back(hip, C, dx, xb); _back(hip, C, dv, vb); _back(hip, C, dc, cb)
    assert (xb == SENT).all() and (vb == DSENT).all() and (cb == ISENT).all()
    # cap == 0 with a buffer is no size query
    n = C.c_int64(-1)
    assert lib.vba_kf_surfel_export(ctx.h, 1, one, inten, 1, 0.5, 1, 0, px, None, None, C.byref(n)) == capi.ERR_CAPACITY and n.value == m
    assert (xh == SENT).all()

    # ---- every refusal, outputs untouched
    def call(n_stores=1, stores=one, intensity=inten, jump=1, voxel=0.5, min_count=1, cap=m, surfels=px, cov=pv, counts=pc, n_out=C.byref(n)):
        return lib.vba_kf_surfel_export(ctx.h, n_stores, stores, intensity, jump, voxel, min_count, cap, surfels, cov, counts, n_out)

    null_store = (C.c_void_p * 1)(None)
    cases = {
        "n_stores < 1": dict(n_stores=0), "n_stores negative": dict(n_stores=-1), "a NULL store": dict(stores=null_store),
        "NULL stores": dict(stores=None), "NULL intensity": dict(intensity=None), "jump < 1": dict(jump=0), "jump negative": dict(jump=-3),
        "min_count < 1": dict(min_count=0), "cap < 0": dict(cap=-1), "a NULL n_out": dict(n_out=None), "cap > 0 with a NULL surfels": dict(surfels=None),
        "voxel_size < 0.001": dict(voxel=0.0009), "voxel_size 0": dict(voxel=0.0), "voxel_size negative": dict(voxel=-1.0),
        "voxel_size NaN": dict(voxel=float("nan")),
        "a misaligned device surfels": dict(surfels=C.c_void_p(dx.value + 4), cov=dv, counts=dc),
        "a misaligned device cov": dict(surfels=dx, cov=C.c_void_p(dv.value + 4), counts=dc),
        "device surfels with host counts": dict(surfels=dx, cov=dv),
        "device surfels with host cov": dict(surfels=dx, counts=dc),
        "host surfels with device cov": dict(cov=dv),
        "host surfels with device counts": dict(counts=dc),
    }
    ndev = C.c_int(0)
    assert hip.hipGetDeviceCount(C.byref(ndev)) == 0
    if ndev.value > 1:                                                        # another device
        o = capi.default_options(); o.device = 1
        other = capi.Context(o)
        cases["a store of another device"] = dict(stores=(C.c_void_p * 1)(other.kf_store().h.value))
    for what, kw in cases.items():
        n.value = -1
        assert call(**kw) == capi.ERR_BAD_ARG, what
        assert n.value == -1 and (xh == SENT).all() and (vh == DSENT).all() and (ch == ISENT).all(), what
    ctx.synchronize()
    _back(hip, C, dx, xb); _back(hip, C, dv, vb); _back(hip, C, dc, cb)
    assert (xb == SENT).all() and (vb == DSENT).all() and (cb == ISENT).all()
    assert call() == 0 and n.value == m and np.array_equal(ch, hcnt) and same(xh, host) and same(vh, hcov)   # the same arguments unrefused do export
    assert hip.hipFree(dx) == 0 and hip.hipFree(dv) == 0 and hip.hipFree(dc) == 0
    with pytest.raises(capi.VbaError) as e:                                   # an empty list of stores is n_stores < 1
        ctx.kf_export_surfel([], [], 1, 0.5, cap=4)
    assert e.value.status == capi.ERR_BAD_ARG


def test_nothing_to_export(capi, world):
    ctx = world["ctx"][True]
    empty = world["ctx"][False].kf_store()                                    # no keyframes
    hollow = _build(world["ctx"][False], [np.zeros((0, 3))] * 3, ev.edge_poses(3, 1, 2.0))      # keyframes without points
    for stores in ([empty], [hollow], [empty, hollow]):
        rec, cov, cnt = ctx.kf_export_surfel(stores, [1.0] * len(stores), 1, 0.5, 1, cap=4)
        assert rec.shape == (0, 12) and cov.shape == (0, 6) and cnt.shape == (0,)
        assert ctx.kf_export_surfel_size(stores, [1.0] * len(stores), 2, 0.5) == 0
    near = world["stores"]["near"]
    a = ctx.kf_export_surfel([near], [3.0], 1, 0.5)
    b = ctx.kf_export_surfel([empty, hollow, near, hollow], [7.0, 8.0, 3.0, 9.0], 1, 0.5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[2] >= 3).all() and len(a[0]) == 163       # min_count defaults to 3
    assert ctx.kf_export_surfel_size([near], [3.0], 1, 0.5, 600) == 0


@pytest.mark.parametrize("det", [True, False])
def test_no_allocation_after_reserve(capi, world, det):
    ctx, hip, C = _ctx(capi, det), world["hip"], capi.C
    assert ctx.kf_export_surfel_allocations() == (0, 0)
    total = sum(len(c) for c in world["clouds"])
    ctx.kf_export_surfel_reserve(2 * total, 400)
    base = ctx.kf_export_surfel_allocations()
    # slot, table and sums of the shared arrays at the least, and the 52 bytes per kept voxel of this feature's own
    assert base[0] >= 7 and base[1] >= 2 * total * (4 + 2 * 16 + 2 * 24) + 400 * 52
    ctx.kf_export_surfel_reserve(total, 100)                                  # less than is held: nothing happens
    assert ctx.kf_export_surfel_allocations() == base
    near, far = world["stores"]["near"], world["stores"]["far"]
    xb = np.zeros((400, 12), dtype=np.float32); vb = np.zeros((400, 6)); cb = np.zeros(400, dtype=np.int32)
    dx, dv, dc = _dev(hip, C, xb), _dev(hip, C, vb), _dev(hip, C, cb)
    for jump in (1, 3):
        for voxel in VOXELS:
            ctx.kf_export_surfel([near], [3.0], jump, voxel, 1)
            ctx.kf_export_surfel([near, far], [3.0, 4.0], jump, voxel, 2)
            assert ctx.kf_export_surfel([far, near], [3.0, 4.0], jump, voxel, 1, cap=400, out=(dx, dv, dc)) <= 400
            ctx.kf_export_surfel_size([far], [3.0], jump, voxel)
            ctx.kf_export_voxel([near, far], [3.0, 4.0], jump, voxel)         # the voxel export runs on the same arrays
    ctx.synchronize()
    assert ctx.kf_export_surfel_allocations() == base
    # more kept voxels than were reserved grow this feature's rows, and the result is the same
    sessions = [(world["clouds"], world["poses"]["near"], 3.0), (world["clouds"], world["poses"]["far"], 4.0)]
    ref = _want(world, "near+far", sessions, 1, 0.125)
    assert len(ref["cnt"]) > 400
    rec, cov, cnt = ctx.kf_export_surfel([near, far], [3.0, 4.0], 1, 0.125, 1)
    assert np.array_equal(cnt, ref["cnt"]) and (not det or (np.array_equal(rec, ref["rec"]) and np.array_equal(cov, ref["C"])))
    grown = ctx.kf_export_surfel_allocations()
    assert grown[0] > base[0] and grown[1] > base[1]
    assert hip.hipFree(dx) == 0 and hip.hipFree(dv) == 0 and hip.hipFree(dc) == 0
    ctx.close()


@pytest.mark.parametrize("det", [True, False])
def test_alternating_with_the_voxel_export(world, det):
    """the two calls share the table, the sums and the sort arrays of one context: each leaves the other's next result as it was"""
    ctx = world["ctx"][det]
    near, far = world["stores"]["near"], world["stores"]["far"]
    v0 = ctx.kf_export_voxel([near], [3.0], 1, 0.5, 1)
    s0 = ctx.kf_export_surfel([far], [3.0], 1, 1.0, 3)
    for _ in range(2):
        v = ctx.kf_export_voxel([near], [3.0], 1, 0.5, 1)
        s = ctx.kf_export_surfel([far], [3.0], 1, 1.0, 3)
        assert np.array_equal(v[1], v0[1]) and np.array_equal(s[2], s0[2]) and np.array_equal(s[0][:, [3, 11]], s0[0][:, [3, 11]])
        if det:
            assert all(np.array_equal(x, y) for x, y in zip(v, v0)) and all(np.array_equal(x, y) for x, y in zip(s, s0))
    sessions = [(world["clouds"], world["poses"]["far"], 3.0)]
    _check(world, det, [far], [3.0], "far", sessions, 1, 1.0, 3, "after alternating")
    want, wcnt, _ = ev.export_voxel([(world["clouds"], world["poses"]["near"], 3.0)], 1, 0.5, 1)
    assert np.array_equal(v0[1], wcnt) and (np.array_equal(v0[0], want) if det else _adjacent_or_equal(v0[0][:, :3], want[:, :3]).all())


def test_adapter_program(capi, world):
    """vba::pub_globalmap_surfel through tests/host/export_surfel_host.cpp: its messages, concatenated, are the Python result"""
    clouds = world["clouds"]
    sessions = [(clouds, world["poses"]["far"]), (clouds[:4], world["poses"]["near"][:4])]
    fin, fout = str(world["dir"] / "in.bin"), str(world["dir"] / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(sessions)))
        for cl, ps in sessions:
            f.write(struct.pack("<i", len(cl)))
            for c, x in zip(cl, ps):
                f.write(struct.pack("<i", len(c))); f.write(np.ascontiguousarray(x, dtype=np.float64).tobytes())
                f.write(np.ascontiguousarray(c, dtype=np.float64).tobytes())
    ctx = world["ctx"][True]
    b = _build(world["ctx"][False], clouds[:4], world["poses"]["near"][:4])
    for min_count, interval in ((1, 50), (3, 5_000_000)):
        want, wcov, _ = ctx.kf_export_surfel([world["stores"]["far"], b], [0.0, 1.0], 1, 0.5, min_count)
        r = subprocess.run([world["exe"], "gpu", fin, fout, "0.5", str(min_count), str(interval), "1", "1", repr(sr.GRID)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        raw = open(fout, "rb").read()
        recs, covs, q = [], [], 0
        while q < len(raw):
            n = struct.unpack_from("<q", raw, q)[0]; q += 8
            recs.append(np.frombuffer(raw, dtype=np.float32, count=12 * n, offset=q).reshape(n, 12)); q += 48 * n
            covs.append(np.frombuffer(raw, dtype=np.float64, count=6 * n, offset=q).reshape(n, 6)); q += 48 * n
        ends = ev.message_ends(len(want), interval)
        print("min_count %d interval %d: %d records in %d messages" % (min_count, interval, len(want), len(recs)))
        assert [len(x) for x in recs] == [e - s for s, e in zip([0] + ends[:-1], ends)] and len(recs) >= 1
        assert r.stdout.split() == ["records", str(len(want)), "messages", str(len(recs))]
        assert np.array_equal(np.concatenate(recs), want) and np.array_equal(np.concatenate(covs), wcov) and len(want) > 100
