"""The device-resident keyframe store (vba_kf_*) on the MI355X against the numpy restatement tests/kf_oracle.py
and the CPU oracle: building a keyframe from its scans (merge, kept cloud, descriptors), descriptors of windows of stored
keyframes, keyframe_loading into the voxel map, the hierarchical BA reading the store in place, residency and refusals,
determinism."""
import dataclasses

import numpy as np
import pytest

import kf_oracle as ko

pytestmark = pytest.mark.gpu

VS10 = 0.5 / 10            # voxel_size / 10 of VS:2385 at Odometry/voxel_size 0.5


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


def _ctx(capi, **kw):
    o = capi.default_options()
    o.device = 0
    for k, v in kw.items():
        setattr(o, k, v)
    return capi.Context(o)


def _hip():
    """the HIP runtime libvoxelba.so has already loaded (for a device buffer of the test's own)"""
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _db(capi, ctx):
    db = ctx.btc_db(capi.btc_default_config(0))
    db.set_gen_config(capi.btc_default_gen_config(0))
    return db


@pytest.fixture(scope="module")
def small_path(synth):
    """thirty keyframes of 3 scans x 6000 points on the curved path"""
    return synth.make_keyframe_path(n_kf=30, scans_per_kf=3, n_pts=6000)


def _within_one_float_spacing(got, want, what):
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    bound = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want)
    worst = float((err / bound).max()) if len(want) else 0.0
    print("%s: %d values, %d differ, largest difference %.3g float spacings" % (what, want.size, int((err > 0).sum()), worst))
    assert (err <= bound).all(), "%s: %d values further than one float spacing, worst %.3g spacings" % (what, int((err > bound).sum()), worst)


@pytest.mark.parametrize("n_pts", [20000, 200000])
def test_build_against_restatement_and_oracle(capi, synth, oracle, n_pts):
    """10 scans with covariances -> one keyframe.  The descriptors prove the device merge bit for bit: they equal
    vba_btc_generate_stds on the restatement's merged float cloud.  The kept cloud against the oracle's down_sampling_pvec on the
    restatement's merged doubles: same voxels, order and counts; every value within ONE float spacing (both sides form the mean in
    double to ~1e-13 relative and round once to float, so they differ only where that rounding straddles)."""
    kf = synth.make_keyframe_path(n_kf=1, scans_per_kf=10, n_pts=n_pts, scan_step=0.02, seed=synth.SEED_BASE + 61 + (n_pts > 20000))[0]
    ctx = _ctx(capi)
    store = ctx.kf_store()
    db, db2 = _db(capi, ctx), _db(capi, ctx)
    n, rows, bits = store.build(kf["points"], kf["poses"], VS10, id=41, jour=3.5, vars=kf["vars"], db=db)
    mf = ko.merge_float(kf["points"], kf["poses"])
    r2, b2 = db2.generate_stds(mf, 41)
    print("merged %d points -> %d kept, %d descriptors, %d plane points" % (len(mf), n, len(rows), len(db.plane_cloud(0))))
    assert len(db2.plane_cloud(0)) > 0
    assert np.array_equal(db.plane_cloud(0), db2.plane_cloud(0))
    assert np.array_equal(rows, r2) and np.array_equal(bits, b2)
    assert db.num_frames() == 1 and db.frame_seq(0) == 41
    g = store.get(0)
    assert np.array_equal(g["x0"], kf["poses"][-1]) and (g["id"], g["jour"], g["exist"], g["n_points"]) == (41, 3.5, 0, n)
    merged = ko.merge(kf["points"], kf["poses"])
    var = np.concatenate(kf["vars"])
    o_out, o_vd, o_cnt = oracle.down_sampling_pvec(merged, var, VS10)
    xyz, vd = store.read(0)
    cnt = store.last_counts()
    assert n == len(o_out) == len(xyz) and store.size() == 1
    assert np.array_equal(cnt, o_cnt)                                      # same voxels in the same (first-occurrence) order
    first, rcnt, _ = ko.voxel_groups(merged, VS10, True)
    assert np.array_equal(cnt, rcnt)
    assert np.array_equal(xyz, xyz.astype(np.float32).astype(np.float64))  # float values carried in doubles
    _within_one_float_spacing(xyz, o_out, "kept cloud (pvec)")
    _within_one_float_spacing(vd, o_vd, "covariance diagonals")
    # the offline form (var == NULL): down_sampling_voxel of the merged points narrowed to float, diagonals zero
    n0, _, _ = store.build(kf["points"], kf["poses"], VS10, id=42, jour=4.5)
    d_out, d_cnt, _ = ctx.down_sampling_voxel(mf.astype(np.float64), VS10)
    xyz0, vd0 = store.read(1)
    assert n0 == len(d_out) == len(xyz0) and np.array_equal(store.last_counts(), d_cnt)
    _within_one_float_spacing(xyz0, d_out, "kept cloud (voxel)")
    assert not vd0.any()
    # device-resident input gives the same keyframe as host input
    hip = _hip()
    C = capi.C
    off = np.zeros(11, np.int32); off[1:] = np.cumsum([len(p) for p in kf["points"]])
    hp = np.ascontiguousarray(np.concatenate(kf["points"])); hv = np.ascontiguousarray(var)
    dp, dv = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dp), C.c_size_t(hp.nbytes)) == 0 and hip.hipMalloc(C.byref(dv), C.c_size_t(hv.nbytes)) == 0
    assert hip.hipMemcpy(dp, hp.ctypes.data_as(C.c_void_p), C.c_size_t(hp.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice
    assert hip.hipMemcpy(dv, hv.ctypes.data_as(C.c_void_p), C.c_size_t(hv.nbytes), C.c_int(1)) == 0
    npt = C.c_int(); ns = C.c_int()
    ctx._chk(ctx.lib.vba_kf_build(store.h, C.c_int(10), off.ctypes.data_as(C.POINTER(C.c_int)), dp, dv, capi._p(np.ascontiguousarray(kf["poses"])),
                                  C.c_double(VS10), C.c_int(43), C.c_double(5.5), None, C.c_int(0), None, None, C.byref(ns), C.byref(npt)))
    assert hip.hipFree(dp) == 0 and hip.hipFree(dv) == 0
    xyz2, vd2 = store.read(2)
    assert np.array_equal(store.last_counts(), cnt)
    if ctx.opt.deterministic:
        assert np.array_equal(xyz2, xyz) and np.array_equal(vd2, vd)
    else:
        _within_one_float_spacing(xyz2, o_out, "kept cloud (device input)")
        _within_one_float_spacing(vd2, o_vd, "covariance diagonals (device input)")
    ctx.close()


def _fill(store, kfs, db=None, with_var=True, first_id=100):
    out = []
    for k, kf in enumerate(kfs):
        out.append(store.build(kf["points"], kf["poses"], VS10, id=first_id + k, jour=0.7 * k, vars=kf["vars"] if with_var else None, db=db))
    return out


def test_window_descriptors(capi, small_path):
    ctx = _ctx(capi)
    store = ctx.kf_store()
    _fill(store, small_path[:9])
    db, db2 = _db(capi, ctx), _db(capi, ctx)
    for w, (first, count) in enumerate([(0, 3), (2, 4), (5, 3), (8, 1), (0, 9)]):
        rows, bits = store.generate_stds(first, count, db)
        clouds = [store.read(k)[0] for k in range(first, first + count)]
        poses = [store.get(k)["x0"] for k in range(first, first + count)]
        mf = ko.merge_float(clouds, poses)
        r2, b2 = db2.generate_stds(mf, 100 + first + count - 1)
        print("window (%d, %d): %d points, %d descriptors, %d plane points" % (first, count, len(mf), len(rows), len(db.plane_cloud(w))))
        assert len(db2.plane_cloud(w)) > 0
        assert np.array_equal(db.plane_cloud(w), db2.plane_cloud(w))
        assert np.array_equal(rows, r2) and np.array_equal(bits, b2)
        assert db.frame_seq(w) == 100 + first + count - 1
    ctx.close()


def _queries(pos, n_hist, radius):
    """a walk of query positions beside the path; asserted on the CPU to stay clear of the two cases the reference leaves to its
    kd-tree: no keyframe within 1e-3 m of a query sphere, and the float squared distances of a query's candidates differ pairwise"""
    qs = []
    for j in list(range(0, 30, 2)) + list(range(29, 0, -3)) + [3, 4, 5, 6, 7, 20, 21, 22]:
        qs.append(pos[j] + np.array([0.37, -0.21, 0.11]) * (1 + (j % 3)))
    qs.append(np.array([100.0, 0.0, 0.0]))                             # nothing nearby
    h = ko.History(pos); h.set_history(n_hist)
    for q in qs:
        d = np.sqrt(((pos[:n_hist] - q) ** 2).sum(1))
        assert (np.abs(d - radius) > 1e-3).all()
        idx, d2 = h.candidates(q, radius)
        assert len(np.unique(d2)) == len(d2)
    return qs


def test_keyframe_loading(capi, synth, oracle, small_path):
    from test_gpu_map import _compare_leaves, _omap, _opts
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="kf_map")
    W, radius, n_hist = wl.win_size, 3.0, 25
    ctx = capi.Context(_opts(capi, wl))
    ctx2 = capi.Context(_opts(capi, wl))
    store = ctx.kf_store()
    _fill(store, small_path)
    assert store.size() == 30
    pos = np.array([store.get(k)["x0"][9:] for k in range(30)])
    qs = _queries(pos, n_hist, radius)
    win = small_path[12]["points"] + small_path[13]["points"][:1]      # the W window scans inserted between the loads
    wposes = np.concatenate([small_path[12]["poses"], small_path[13]["poses"][:1]])

    def session(map_ctx, om):
        store.set_history(0)
        assert store.load_nearby(map_ctx, qs[0], radius, 0.0) == -1 and map_ctx.num_roots() == 0     # before set_history: switched off
        store.set_history(n_hist)
        h = ko.History(pos); h.set_history(n_hist)
        loaded = []
        for j, q in enumerate(qs):
            got = store.load_nearby(map_ctx, q, radius, jour=float(j))
            want = h.load_nearby(q, radius)
            assert got == want, (j, got, want)
            assert store.history_size() == h.size
            assert [store.get(k)["exist"] for k in range(30)] == h.exist.tolist()
            if want >= 0:
                loaded.append(want)
                if om is not None:
                    om.cut_voxel_fix(ko.world(store.get(want)["x0"], store.read(want)[0]), jour=float(j))
            if j % 7 == 3 and j // 7 < W:
                i = j // 7
                map_ctx.cut_voxel(i, win[i], wposes[i])
                if om is not None:
                    om.cut_voxel(i, win[i], wposes[i])
        map_ctx.recut(W, wposes, multi=False)
        return loaded

    om = _omap(oracle, wl)
    loaded = session(ctx, om)
    print("loaded keyframes:", loaded)
    assert len(loaded) >= 15 and len(set(loaded)) == len(loaded)
    om.recut(W, wposes, oracle.Factor(W), multi=False)
    gd = ctx.dump_leaves()
    nplane = _compare_leaves(gd, om.dump_leaves())
    assert nplane > 20
    # the same session into the map of a second context on the device gives the same leaves
    assert session(ctx2, None) == loaded
    # (leaf by leaf at the same bars: the dump's unused fields of non-planar leaves are not defined)
    _compare_leaves(ctx2.dump_leaves(), om.dump_leaves())
    _compare_leaves(ctx2.dump_leaves(), gd)
    # set_history(0) switches loading off again
    store.set_history(0)
    assert store.load_nearby(ctx, qs[0], radius) == -1 and store.history_size() == 0
    # set_poses moves a keyframe: the next load writes the new world points
    x = store.get(2)["x0"].copy(); x[9:] += [0.5, 0.25, 0.0]
    store.set_poses(2, x[None, :])
    assert np.array_equal(store.get(2)["x0"], x)
    store.close(); ctx.close(); ctx2.close()


def test_hba_reads_the_store_in_place(capi, synth, oracle):
    import ctypes as C
    from test_gpu_gba import GBA, _cfg13
    wl = synth.CONFIGS["room20k_w4"]
    s = synth.make_scans(wl)
    W = wl.win_size
    poses = synth.poses_flat(s["R0"], s["p0"])
    ctx = capi.Context(capi.options_from_workload(wl))
    store = ctx.kf_store()
    # keyframe 0 is not part of the window: the window's base pointer is not the store's
    for k in [0] + list(range(W)):
        store.build([s["points"][k]], poses[k][None, :], VS10, id=k, jour=0.0)
    d, off, n_kf = store.clouds()
    assert n_kf == W + 1 and off[0] == 0 and off[-1] == sum(store.get(k)["n_points"] for k in range(n_kf))
    clouds = [store.read(k)[0] for k in range(n_kf)]
    # the store's array, copied to the host, is the concatenation of the keyframes
    flat = np.zeros((int(off[-1]), 3)); cnt = np.zeros(len(flat), np.int32); first = np.zeros(len(flat), np.int32); m = C.c_int()
    # (a voxel size below 0.001 makes the down-sampler hand its input back unchanged: a device-to-host copy through the library)
    ctx._chk(ctx.lib.vba_scan_down_sampling_voxel(ctx.h, C.c_int(len(flat)), C.c_void_p(d), C.c_double(0.0), capi._p(flat),
                                                  cnt.ctypes.data_as(C.POINTER(C.c_int)), first.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m)))
    assert m.value == len(flat)
    assert np.array_equal(flat, np.concatenate(clouds))
    x0 = np.array([store.get(k)["x0"] for k in range(1, W + 1)])
    got = store.hba_add_edge(ctx, 1, W, x0, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 3, 2)
    want = oracle.hba_add_edge(clouds[1:], x0, _cfg13(oracle, wl, ctx), 3, 2)
    assert want["status"] == 0 and len(got["resis"]) == len(want["resis"])
    np.testing.assert_allclose(got["resis"], want["resis"], rtol=1e-6)
    np.testing.assert_allclose(got["poses"], want["poses"], rtol=0, atol=1e-6)
    ge, we = got["edges"], want["edges"]
    assert len(ge) == len(we) and len(ge) > 0
    np.testing.assert_array_equal(ge[:, :2], we[:, :2])
    np.testing.assert_allclose(ge[:, 2:14], we[:, 2:14], rtol=0, atol=1e-6)
    np.testing.assert_allclose(ge[:, 14:], we[:, 14:], rtol=1e-5)
    # and the same call from a host copy of the same clouds gives the same result as from the store
    host = ctx.hba_add_edge(clouds[1:], x0, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 3, 2)
    np.testing.assert_allclose(got["poses"], host["poses"], rtol=0, atol=1e-9)
    store.close(); ctx.close()


def test_residency_and_refusals(capi, synth, small_path):
    wl = synth.CONFIGS["room20k_w4"]
    opt = capi.options_from_workload(wl); opt.deterministic = 1        # (so that a second store can be compared bit for bit)
    ctx = capi.Context(opt)
    kfs = small_path[:8]
    merged = max(sum(len(p) for p in kf["points"]) for kf in kfs)
    # --- a reserved session leaves the allocation count alone
    store = ctx.kf_store()
    db = _db(capi, ctx)
    db.gen_reserve(points=4 * merged, cells=1 << 22, frames=32)
    store.reserve(points=8 * merged, keyframes=16, merge_points=4 * merged)
    a0 = store.allocations()
    res = _fill(store, kfs, db=db)
    rows_w = [store.generate_stds(f, c, db) for f, c in ((0, 3), (4, 4))]
    store.set_history(6)
    for k in (1, 4):
        store.load(k, ctx, jour=1.0)
    assert store.load_nearby(ctx, store.get(3)["x0"][9:], 3.0) >= 0
    assert store.allocations() == a0, (a0, store.allocations())
    assert a0[0] > 0 and a0[1] >= 8 * merged * 36
    # --- a store that has to grow gives the same bits
    ctx_b = capi.Context(opt)
    grown = ctx_b.kf_store()
    db_b = _db(capi, ctx_b)
    res_b = _fill(grown, kfs, db=db_b)
    assert grown.allocations()[0] > 2
    for k in range(len(kfs)):
        assert res[k][0] == res_b[k][0] and np.array_equal(res[k][1], res_b[k][1]) and np.array_equal(res[k][2], res_b[k][2])
        a, b = store.read(k), grown.read(k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(db.plane_cloud(k), db_b.plane_cloud(k))
    for (ra, ba), (f, c) in zip(rows_w, ((0, 3), (4, 4))):
        rb, bb = grown.generate_stds(f, c, db_b)
        assert np.array_equal(ra, rb) and np.array_equal(ba, bb)
    # --- refusals: nothing changes
    def state():
        return (store.size(), db.num_frames(), store.history_size(), store.allocations(), store.read(store.size() - 1)[0].tobytes(),
                [store.get(k)["exist"] for k in range(store.size())])
    before = state()
    kf = kfs[0]
    off = np.zeros(4, np.int32); off[1:] = np.cumsum([len(p) for p in kf["points"]])
    pnt = np.concatenate(kf["points"]); poses = np.ascontiguousarray(kf["poses"])
    cap = capi.btc_max_stds(db.gcfg)
    rows = np.zeros((cap, capi.BTC_ROW_LEN)); bits = np.zeros((cap, 3), np.uint64)
    C = capi.C

    def raw_build(k, off, cap_rows, dbh):
        ns = C.c_int(); npt = C.c_int()
        return ctx.lib.vba_kf_build(store.h, C.c_int(k), off.ctypes.data_as(C.POINTER(C.c_int)), capi._p(pnt), None, capi._p(poses),
                                    C.c_double(VS10), C.c_int(7), C.c_double(0.0), dbh, C.c_int(cap_rows), capi._p(rows),
                                    bits.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ns), C.byref(npt))

    assert raw_build(0, off, cap, db.h) == capi.ERR_BAD_ARG                            # k < 1
    bad = off.copy(); bad[2] = bad[1] - 5
    assert raw_build(3, bad, cap, db.h) == capi.ERR_BAD_ARG                            # offsets not non-decreasing
    assert raw_build(3, off, cap - 1, db.h) == capi.ERR_BAD_ARG                        # cap below the generator's bound
    for call in (lambda: store.generate_stds(7, 2, db), lambda: store.generate_stds(-1, 1, db), lambda: store.load(8, ctx),
                 lambda: store.read(8), lambda: store.get(-1), lambda: store.set_poses(7, np.tile(poses[0], (2, 1))),
                 lambda: store.set_history(9), lambda: store.generate_stds(0, 2, db, cap=cap - 1)):
        with pytest.raises(capi.VbaError) as e:                                        # an index out of range
            call()
        assert e.value.status == capi.ERR_BAD_ARG
    ndev = capi.C.c_int(0)
    assert _hip().hipGetDeviceCount(capi.C.byref(ndev)) == 0
    if ndev.value > 1:                                                  # a map context on another device
        o = capi.options_from_workload(wl); o.device = 1
        other = capi.Context(o)
        with pytest.raises(capi.VbaError) as e:
            store.load(0, other)
        assert e.value.status == capi.ERR_BAD_ARG
        other.close()
    assert state() == before
    ctx.close(); ctx_b.close()


def test_determinism(capi, small_path):
    kfs = small_path[:4]

    def run(det):
        ctx = _ctx(capi, deterministic=det)
        store = ctx.kf_store(); db = _db(capi, ctx)
        res, counts = [], []
        for k, kf in enumerate(kfs):
            res.append(store.build(kf["points"], kf["poses"], VS10, id=100 + k, jour=0.7 * k, vars=kf["vars"], db=db))
            counts.append(store.last_counts())
        win = store.generate_stds(0, 4, db)
        out = dict(res=res, win=win, counts=counts, clouds=[store.read(k) for k in range(4)], planes=[db.plane_cloud(k) for k in range(5)],
                   keys=[ko.voxel_keys(store.read(k)[0], VS10, True) for k in range(4)])
        ctx.close()
        return out

    a, b = run(1), run(1)
    for k in range(4):
        assert np.array_equal(a["clouds"][k][0], b["clouds"][k][0]) and np.array_equal(a["clouds"][k][1], b["clouds"][k][1])
        assert np.array_equal(a["res"][k][1], b["res"][k][1]) and np.array_equal(a["res"][k][2], b["res"][k][2])
    assert np.array_equal(a["win"][0], b["win"][0]) and np.array_equal(a["win"][1], b["win"][1])
    for k in range(5):
        assert np.array_equal(a["planes"][k], b["planes"][k])
    c, d = run(0), run(0)
    for k in range(4):
        # without the mode the sums may differ in the last bit, the voxels, their order and their counts may not
        assert c["res"][k][0] == d["res"][k][0] == a["res"][k][0]
        assert np.array_equal(c["counts"][k], d["counts"][k]) and np.array_equal(c["counts"][k], a["counts"][k])
        assert np.array_equal(c["keys"][k], d["keys"][k]) and np.array_equal(c["keys"][k], a["keys"][k])
        assert len(c["clouds"][k][0]) == len(d["clouds"][k][0]) == len(a["clouds"][k][0])
        assert np.abs(c["clouds"][k][0] - d["clouds"][k][0]).max() <= 4e-6 and np.abs(c["clouds"][k][0] - a["clouds"][k][0]).max() <= 4e-6
        assert np.array_equal(c["res"][k][1], a["res"][k][1]) and np.array_equal(c["res"][k][2], a["res"][k][2])   # the merge has no atomics
