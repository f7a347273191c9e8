"""Hierarchical global BA on the device against the oracle: OctreeGBA build (loop_refine.hpp:273-537)
and HBA_add_edge (voxelslam.cpp:2822-3015) on one keyframe window."""
import dataclasses
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GBA = dict(gba_voxel_size=2.0, gba_min_eigen_value=0.1, gba_eig=[0.25, 0.25, 0.25, 0.25])     # config/avia.yaml:59-65 (inverted)


def _setup(name):
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    if name == "spin40k_w10":
        wl = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name=name, n_pts=40000)
    else:
        wl = synth.CONFIGS[name]
    s = synth.make_scans(wl)
    clouds = [p.astype(np.float32).astype(np.float64) for p in s["points"]]           # PCL stores floats
    poses = synth.poses_flat(s["R0"], s["p0"])
    ctx = capi.Context(capi.options_from_workload(wl))
    return wl, s, clouds, poses, ctx


def _cfg13(oracle, wl, ctx):
    o = ctx.opt
    return oracle.gba_cfg13(GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], o.voxel_size, o.min_eigen_value,
                            list(o.plane_eigen_value_thre), o.max_layer)


@pytest.mark.parametrize("name", ["room20k_w4", "spin40k_w10"])
def test_gba_build_parity(oracle, name):
    wl, s, clouds, poses, ctx = _setup(name)
    n_dev = ctx.gba_build(clouds, poses, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"])
    f = oracle.gba_build(clouds, poses, _cfg13(oracle, wl, ctx))
    assert n_dev == f.size() and n_dev > 20
    ev, evec, pa = ctx.read_back()
    oev, oevec, opa = f.read_back()
    ka = np.lexsort((pa[:, 6], pa[:, 9])); kb = np.lexsort((opa[:, 6], opa[:, 9]))
    np.testing.assert_array_equal(pa[ka, 9], opa[kb, 9])                              # point counts: exact
    scale = np.abs(opa[kb, :9]).max()
    np.testing.assert_allclose(pa[ka], opa[kb], rtol=0, atol=1e-12 * scale)           # f64 atomics: summation order only
    np.testing.assert_allclose(ev[ka], oev[kb], rtol=0, atol=1e-11 * max(1.0, np.abs(oev).max()))
    # the per-keyframe body clusters enter through H, g and the residual
    H, g, r = ctx.acc_evaluate2(poses)
    oH, og, orr = f.acc_evaluate2(poses)
    np.testing.assert_allclose(r, orr, rtol=1e-10)
    np.testing.assert_allclose(H, oH, rtol=0, atol=1e-9 * np.abs(oH).max())
    np.testing.assert_allclose(g, og, rtol=0, atol=1e-9 * np.abs(og).max())
    ctx.close()


@pytest.mark.parametrize("W,max_iter", [(24, 2), (40, 1), (3, 2)])
def test_hba_add_edge_any_window_size(oracle, W, max_iter):
    """The top layer of the hierarchical BA optimises all submaps at once (VS:3103-3113): windows of any size go through the
    sparse path (hashed (node, frame) clusters, CSR factor store, atomics Hessian, host LDL^T)."""
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="room_w%d" % W, win_size=W, n_pts=4000)
    s = synth.make_scans(wl)
    clouds = [p.astype(np.float32).astype(np.float64) for p in s["points"]]
    poses = synth.poses_flat(s["R0"], s["p0"])
    ctx = capi.Context(capi.options_from_workload(synth.CONFIGS["hesai200k_w10"]))     # a context built for W = 10
    o = ctx.opt
    cfg = oracle.gba_cfg13(GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], o.voxel_size, o.min_eigen_value,
                           list(o.plane_eigen_value_thre), o.max_layer)
    got = ctx.hba_add_edge(clouds, poses, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], max_iter, 5)
    want = oracle.hba_add_edge(clouds, poses, cfg, max_iter, 5)
    assert want["status"] == 0 and len(got["resis"]) == len(want["resis"])
    np.testing.assert_allclose(got["resis"], want["resis"], rtol=1e-6)
    np.testing.assert_allclose(got["poses"], want["poses"], rtol=0, atol=1e-6)
    ge, we = got["edges"], want["edges"]
    assert len(ge) == len(we) and len(ge) > 0
    np.testing.assert_array_equal(ge[:, :2], we[:, :2])
    np.testing.assert_allclose(ge[:, 2:14], we[:, 2:14], rtol=0, atol=1e-6)
    np.testing.assert_allclose(ge[:, 14:], we[:, 14:], rtol=1e-5)
    n = sum(len(c) for c in clouds)
    assert got["cloud_count"].sum() == n
    assert abs(len(got["cloud"]) - len(want["cloud"])) <= max(3, len(want["cloud"]) // 500)
    ctx.close()


def test_gba_build_other_window_size_is_refused(oracle):
    from voxel_slam_amd import capi
    wl, s, clouds, poses, ctx = _setup("room20k_w4")
    with pytest.raises(capi.VbaError):
        ctx.gba_build(clouds[:3], poses[:3], 2.0, 0.1, GBA["gba_eig"])
    ctx.close()


@pytest.mark.parametrize("name,max_iter,thread_num", [("room20k_w4", 1, 2), ("room20k_w4", 6, 5), ("spin40k_w10", 3, 2)])
def test_hba_add_edge_parity(oracle, name, max_iter, thread_num):
    wl, s, clouds, poses, ctx = _setup(name)
    W = wl.win_size
    got = ctx.hba_add_edge(clouds, poses, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], max_iter, thread_num)
    want = oracle.hba_add_edge(clouds, poses, _cfg13(oracle, wl, ctx), max_iter, thread_num)
    assert want["status"] == 0
    assert len(got["resis"]) == len(want["resis"])                                     # same number of outer rounds
    np.testing.assert_allclose(got["resis"], want["resis"], rtol=1e-6)
    np.testing.assert_allclose(got["poses"], want["poses"], rtol=0, atol=1e-6)
    # the optimisation moved the poses towards the ground truth
    err0 = np.abs(poses[:, 9:] - s["p_gt"]).max(); err1 = np.abs(got["poses"][:, 9:] - s["p_gt"]).max()
    assert err1 < err0
    ge, we = got["edges"], want["edges"]
    assert len(ge) == len(we) and len(ge) > 0
    np.testing.assert_array_equal(ge[:, :2], we[:, :2])
    np.testing.assert_allclose(ge[:, 2:14], we[:, 2:14], rtol=0, atol=1e-6)            # rot, tra
    np.testing.assert_allclose(ge[:, 14:], we[:, 14:], rtol=1e-5)                       # 1 / |H_kk|
    # submap cloud: same voxel grid on poses that agree to ~1e-9 -> only points within float rounding of a cell boundary differ
    n = sum(len(c) for c in clouds)
    assert got["cloud_count"].sum() == n and want["cloud_count"].sum() == n
    assert abs(len(got["cloud"]) - len(want["cloud"])) <= max(3, len(want["cloud"]) // 500)
    k = min(len(got["cloud"]), len(want["cloud"]), 200)
    same = (got["cloud_count"][:k] == want["cloud_count"][:k])
    assert same.mean() > 0.9
    np.testing.assert_allclose(got["cloud"][:k][same], want["cloud"][:k][same], rtol=0, atol=1e-4)
    ctx.close()


def test_hba_global_hierarchy_parity(oracle):
    """thd_globalmapping's optimisation work (VS:3018-3141) on 25 keyframes: four bottom-layer windows of 10 (stride 5) on the
    templated kernels, their submap clouds, then the top-level window over the four submaps on the sparse path — against the
    same orchestration of the oracle's HBA_add_edge."""
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    nkf, wd, mg = 25, 10, 5
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="room_kf", win_size=nkf, n_pts=6000)
    s = synth.make_scans(wl)
    clouds = [p.astype(np.float32).astype(np.float64) for p in s["points"]]
    x0 = synth.poses_flat(s["R0"], s["p0"])
    ctx = capi.Context(capi.options_from_workload(dataclasses.replace(wl, win_size=wd)))
    o = ctx.opt
    cfg = oracle.gba_cfg13(GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], o.voxel_size, o.min_eigen_value,
                           list(o.plane_eigen_value_thre), o.max_layer)
    e1, e2 = ctx.hba_global(clouds, x0, x0, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 2, wd, mg)
    # the same hierarchy with the oracle
    o1, subs, firsts = [], [], []
    for start in range(0, nkf - wd + 1, mg):
        r = oracle.hba_add_edge(clouds[start:start + wd], x0[start:start + wd], cfg, 1, 2)
        assert r["status"] == 0
        ee = r["edges"].copy(); ee[:, :2] += start
        o1.append(ee); subs.append(r["cloud"]); firsts.append(start)
    o1 = np.concatenate(o1)
    r2 = oracle.hba_add_edge(subs, x0[firsts], cfg, 2, 5, want_cloud=False)
    assert r2["status"] == 0
    o2 = r2["edges"].copy()
    o2[:, 0] = np.array(firsts)[o2[:, 0].astype(int)]; o2[:, 1] = np.array(firsts)[o2[:, 1].astype(int)]
    assert len(e1) == len(o1) == 4 * 45
    np.testing.assert_array_equal(e1[:, :2], o1[:, :2])
    np.testing.assert_allclose(e1[:, 2:14], o1[:, 2:14], rtol=0, atol=1e-6)
    np.testing.assert_allclose(e1[:, 14:], o1[:, 14:], rtol=1e-5)
    # top layer: the submap clouds of the two sides differ by float rounding of a few boundary points (see the window test),
    # so its Hessian-diagonal weights agree to ~1e-3 and the relative poses to ~1e-5
    assert len(e2) == len(o2) == 6
    np.testing.assert_array_equal(e2[:, :2], o2[:, :2])
    np.testing.assert_allclose(e2[:, 2:14], o2[:, 2:14], rtol=0, atol=1e-4)
    np.testing.assert_allclose(e2[:, 14:], o2[:, 14:], rtol=2e-2)
    # the top-level window on IDENTICAL inputs (the oracle's submap clouds on both sides): the sparse any-window path itself
    top = ctx.hba_add_edge(subs, x0[firsts], GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 2, 5, want_cloud=False)
    np.testing.assert_allclose(top["poses"], r2["poses"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(top["edges"][:, :2], r2["edges"][:, :2])
    np.testing.assert_allclose(top["edges"][:, 2:14], r2["edges"][:, 2:14], rtol=0, atol=1e-6)
    np.testing.assert_allclose(top["edges"][:, 14:], r2["edges"][:, 14:], rtol=1e-4)
    ctx.close()


def test_hba_global_at_scale(oracle):
    """BASELINE.json configs[4] on one GPU at a tenth of its length: 200 keyframes x 50k points -> 39 bottom-layer windows of 10
    (stride 5) + the top-level BA over the 39 submaps (a 234 x 234 system on the sparse any-window path), against the oracle's
    HBA_add_edge run in the same hierarchy.  Bottom-layer edges are compared tightly; the top level is compared twice: through the
    hierarchy (the two sides' down-sampled submap clouds differ in a few cell-boundary points) and on identical submap clouds."""
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    nkf, wd, mg = 200, 10, 5
    wl = dataclasses.replace(synth.CONFIGS["hesai200k_w10"], name="hba_scale", win_size=nkf, n_pts=50000)
    s = synth.make_scans(wl)
    clouds = [p.astype(np.float32).astype(np.float64) for p in s["points"]]
    assert sum(len(c) for c in clouds) > 8e6
    x0 = synth.poses_flat(s["R0"], s["p0"])
    ctx = capi.Context(capi.options_from_workload(dataclasses.replace(wl, win_size=wd)))
    o = ctx.opt
    cfg = oracle.gba_cfg13(GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], o.voxel_size, o.min_eigen_value,
                           list(o.plane_eigen_value_thre), o.max_layer)
    e1, e2 = ctx.hba_global(clouds, x0, x0, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 2, wd, mg)
    o1, subs, firsts = [], [], []
    for start in range(0, nkf - wd + 1, mg):
        r = oracle.hba_add_edge(clouds[start:start + wd], x0[start:start + wd], cfg, 1, 2)
        assert r["status"] == 0
        ee = r["edges"].copy(); ee[:, :2] += start
        o1.append(ee); subs.append(r["cloud"]); firsts.append(start)
    o1 = np.concatenate(o1)
    nwin = len(firsts)
    assert nwin == 39 and len(e1) == len(o1) == nwin * 45
    np.testing.assert_array_equal(e1[:, :2], o1[:, :2])
    np.testing.assert_allclose(e1[:, 2:14], o1[:, 2:14], rtol=0, atol=1e-6)             # bar: 1e-4 m / 1e-4 rad
    # 1 / |H_kk| of a cross block: a sum of ~1e5 signed voxel terms — the few entries that nearly cancel carry the summation-order
    # difference relative to their small value (one of 10530 weights differs by 1.4e-4; all others < 1e-5)
    np.testing.assert_allclose(e1[:, 14:], o1[:, 14:], rtol=1e-3)
    rel = np.abs(e1[:, 14:] / o1[:, 14:] - 1)
    assert np.quantile(rel, 0.99) < 1e-5 and np.quantile(rel, 0.999) < 1e-4 and np.median(rel) < 1e-8
    r2 = oracle.hba_add_edge(subs, x0[firsts], cfg, 2, 5, want_cloud=False)
    assert r2["status"] == 0
    o2 = r2["edges"].copy()
    o2[:, 0] = np.array(firsts)[o2[:, 0].astype(int)]; o2[:, 1] = np.array(firsts)[o2[:, 1].astype(int)]
    assert len(e2) == len(o2) and len(e2) > nwin
    np.testing.assert_array_equal(e2[:, :2], o2[:, :2])
    np.testing.assert_allclose(e2[:, 2:14], o2[:, 2:14], rtol=0, atol=1e-4)
    top = ctx.hba_add_edge(subs, x0[firsts], GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 2, 5, want_cloud=False)
    np.testing.assert_allclose(top["poses"], r2["poses"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(top["edges"][:, :2], r2["edges"][:, :2])
    np.testing.assert_allclose(top["edges"][:, 2:14], r2["edges"][:, 2:14], rtol=0, atol=1e-6)
    np.testing.assert_allclose(top["edges"][:, 14:], r2["edges"][:, 14:], rtol=1e-4)
    ctx.close()
    # the run above optimised the 39 windows on 4 worker contexts side by side (vba_options::hba_workers, default); one after the other:
    o1w = capi.options_from_workload(dataclasses.replace(wl, win_size=wd)); o1w.hba_workers = 1
    ctx1 = capi.Context(o1w)
    s1, s2 = ctx1.hba_global(clouds, x0, x0, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 2, wd, mg)
    ctx1.close()
    assert s1.shape == e1.shape and s2.shape == e2.shape and np.array_equal(s1[:, :2], e1[:, :2]) and np.array_equal(s2[:, :2], e2[:, :2])
    np.testing.assert_allclose(s1[:, 2:14], e1[:, 2:14], rtol=0, atol=1e-6)    # (the GBA octree sums with f64 atomics: two runs agree to the bar of the oracle comparison above)
    np.testing.assert_allclose(s2[:, 2:14], e2[:, 2:14], rtol=0, atol=1e-6)


@pytest.fixture(scope="module")
def small_hba():
    """25 keyframes x 6000 points, windows of 10 at stride 5: four bottom-layer windows, the smallest shape at which two worker
    contexts engage (4 >= 2 * 2).  The edges of a fresh context per hba_workers value, computed once."""
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    nkf, wd, mg = 25, 10, 5
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="room_kf", win_size=nkf, n_pts=6000)
    s = synth.make_scans(wl)
    clouds = [p.astype(np.float32).astype(np.float64) for p in s["points"]]
    x0 = synth.poses_flat(s["R0"], s["p0"])

    def context(workers):
        o = capi.options_from_workload(dataclasses.replace(wl, win_size=wd)); o.hba_workers = workers
        return capi.Context(o)

    def run(ctx, cl):
        return ctx.hba_global(cl, x0, x0, GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"], 2, wd, mg)

    edges = {}
    for workers in (1, 2):
        ctx = context(workers)
        edges[workers] = run(ctx, clouds)
        ctx.close()
    return dict(clouds=clouds, x0=x0, wd=wd, mg=mg, context=context, run=run, edges=edges, capi=capi)


def _same_edges(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x[:, :2], y[:, :2])
        np.testing.assert_allclose(x[:, 2:14], y[:, 2:14], rtol=0, atol=1e-6)      # the bar of test_hba_global_at_scale for this comparison


def test_hba_global_workers_equal_sequential_at_the_small_shape(small_hba):
    """Two worker contexts against one window after the other where worker mode first engages."""
    (w1, w2), (s1, s2) = small_hba["edges"][2], small_hba["edges"][1]
    assert len(s1) == 4 * 45 and len(s2) == 6
    _same_edges((w1, w2), (s1, s2))


def test_hba_global_failing_window_in_worker_mode(small_hba):
    """A window that fails in worker mode (keyframes 5..14 see nothing planar: window 1 fails in its LM loop) returns the status it
    returns one window after the other, and the stopped call leaves the workers and d_hba_all usable: the clean input on the SAME
    context gives the edges of a fresh context."""
    capi = small_hba["capi"]
    bad = list(small_hba["clouds"])
    rng = np.random.default_rng(0)
    for i in range(5, 15):
        bad[i] = rng.normal(0, 3.0, (400, 3)).astype(np.float32).astype(np.float64)
    status = {}
    for workers in (1, 2):
        ctx = small_hba["context"](workers)
        with pytest.raises(capi.VbaError) as e:
            small_hba["run"](ctx, bad)
        status[workers] = e.value.status
        if workers == 2:
            _same_edges(small_hba["run"](ctx, small_hba["clouds"]), small_hba["edges"][2])
        ctx.close()
    assert status[1] != 0 and status[2] == status[1]


@pytest.mark.parametrize("workers", [1, 2])
def test_hba_global_edge_capacity(small_hba, workers):
    """cap1 one row short of the result: VBA_ERR_CAPACITY with n_edges1 == cap1; exact: VBA_OK.  Once through the sequential driver's
    append and once through the collecting walk of the worker driver."""
    import ctypes as C
    capi = small_hba["capi"]
    n1_full, n2_full = len(small_hba["edges"][workers][0]), len(small_hba["edges"][workers][1])
    off, pnt = capi.Context._ragged(small_hba["clouds"])
    x0 = np.ascontiguousarray(small_hba["x0"], dtype=np.float64)
    eig = np.ascontiguousarray(GBA["gba_eig"], dtype=np.float64)
    dp = C.POINTER(C.c_double)
    ctx = small_hba["context"](workers)
    for cap1, want in ((n1_full - 1, capi.ERR_CAPACITY), (n1_full, 0)):
        e1 = np.zeros((cap1, 20)); e2 = np.zeros((n2_full, 20)); n1 = C.c_int(-1); n2 = C.c_int(-1)
        st = ctx.lib.vba_hba_global(ctx.h, len(small_hba["clouds"]), off.ctypes.data_as(C.POINTER(C.c_int)), pnt.ctypes.data_as(dp), x0.ctypes.data_as(dp),
                                    x0.ctypes.data_as(dp), GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], eig.ctypes.data_as(dp), 2,
                                    small_hba["wd"], small_hba["mg"], e1.ctypes.data_as(dp), cap1, C.byref(n1), e2.ctypes.data_as(dp), n2_full, C.byref(n2))
        assert st == want and n1.value == cap1
        np.testing.assert_array_equal(e1[:, :2], small_hba["edges"][workers][0][:cap1, :2])      # the rows that fitted are written
        if want == 0:
            assert n2.value == n2_full
    ctx.close()


def test_hba_global_full_length():
    """BASELINE.json configs[4] at its full length on ONE GPU: 2000 keyframes x 50k points (98.5 M points) -> 399 bottom-layer windows
    + the 399-submap top-level BA in one vba_hba_global call; the bottom layer is checked against the oracle on 12 windows spread over
    the session (tools/hba_fullsize.py: relative-pose entries to 1e-6, edge weights q99 to 1e-4; measured 8e-10 / 2e-6, 1.1 s per call)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "hba_fullsize.py"), "2000", "12"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("OK"), r.stdout[-2000:]
