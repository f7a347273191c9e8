"""The surfel map and the registration against it (vba_surfel_map_build, vba_surfel_map_build_from_kf, vba_surfel_register,
vba_debug_surfel_reg_pass) on the MI355X against the host build of csrc/vba_surfreg_math.hpp
(tests/host/surfreg_host.cpp) and the numpy restatement tests/surfreg_ref.py, which tests/test_surfreg_cpu.py holds to each other
and to exact sums.

Bars.  The build: cells, keys and W equal the host program's bit for bit.  One pass: cell and gate equal the host program's for
every point; the 29 sums are within surfreg_ref.sums_bar (any order of the additions) of the exact sums, and since the host program
restates the kernels' order they are also its bits; the step meets the exact-residual bars of solve_ref.  The loop: iters, converged
and matches[] equal the host program's; the final pose and cost[] are within surfreg_ref.pose_bars, 4 x the spread the restatement
shows over 16 starts 1e-12 apart (measured: 3e-16 .. 9e-16 on R, 0 .. 3e-15 on t, 8e-11 .. 1.2e-10 relative on cost[])."""
import struct
import subprocess

import numpy as np
import pytest

import eig3_ref as er
import surfel_ref as sr
import surfreg_ref as rr

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1564)


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


def _hip():
    import ctypes
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _dev(hip, C, arr):
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(arr.nbytes)) == 0
    assert hip.hipMemcpy(d, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), C.c_int(1)) == 0      # hipMemcpyHostToDevice
    return d


def _store(ctx, clouds, poses):
    store = ctx.kf_store()
    for k, c in enumerate(clouds):
        kept, _, _ = store.build([c], poses[k:k + 1], sr.GRID, id=k, jour=float(k))
        assert kept == len(c)
    return store


@pytest.fixture(scope="module")
def world(capi, tmp_path_factory):
    """a deterministic context with the scene of surfel_ref in a near and a far store, the exported records of both at both voxel
    sizes (every voxel: the map's min_count filters), the scans, and the host program"""
    o = capi.default_options(); o.device = 0; o.deterministic = 1
    ctx = capi.Context(o)
    clouds, poses = sr.scene()
    d = tmp_path_factory.mktemp("surfreg_gpu")
    w = dict(ctx=ctx, clouds=clouds, exe=rr.build_host(d), dir=d, hip=_hip(), stores={}, poses={"near": poses, "far": sr.shifted(poses)}, sc={}, cache={})
    for name in ("near", "far"):
        w["stores"][name] = _store(ctx, clouds, w["poses"][name])
        _, S = rr.world(name)
        pnt, Rg, tg = rr.scan_of(S, name)
        per = {}
        for voxel in rr.VOXELS:
            rec, cov, cnt = ctx.kf_export_surfel([w["stores"][name]], [2.0], 1, voxel, 1)
            wrec, wcov = rr.records_of(S, voxel)
            assert np.array_equal(rec[:, :3], wrec[:, :3]) and np.array_equal(rec[:, 11], wrec[:, 11]) and np.array_equal(cov, wcov)
            per[voxel] = dict(rec=rec, cov=cov, ref=rr.Map(rec, cov, voxel, rr.SIGMA, rr.MIN_COUNT))
        w["sc"][name] = dict(pnt=pnt, Rg=Rg, tg=tg, per=per)
    yield w
    ctx.close()


def _map(world, name, voxel, min_count=rr.MIN_COUNT):
    k = ("map", name, voxel, min_count)
    if k not in world["cache"]:
        m = world["ctx"].surfel_map()
        pv = world["sc"][name]["per"][voxel]
        m.build(pv["rec"], pv["cov"], voxel, rr.SIGMA, min_count)
        world["cache"][k] = m
    return world["cache"][k]


def _sorted(rd):
    o = np.argsort(rd["key"])
    return {k: (v[o] if isinstance(v, np.ndarray) else v) for k, v in rd.items()}


def _host(world, pv, pnt, R, t, voxel, **kw):
    return rr.host_run(world["exe"], world["dir"], pv["rec"], pv["cov"], pnt, R, t, voxel, **kw)


# ---------------------------------------------------------------- build
@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", rr.VOXELS)
def test_build_paths_give_the_host_programs_map(capi, world, name, voxel):
    ctx, hip, C = world["ctx"], world["hip"], capi.C
    sc = world["sc"][name]; pv = sc["per"][voxel]; ref = pv["ref"]
    h = _host(world, pv, sc["pnt"][:4], sc["Rg"], sc["tg"], voxel, tag="build")
    want = np.argsort(ref.keys)
    m = _map(world, name, voxel)
    assert m.size() == (ref.n_cells, voxel, rr.SIGMA) and h["n_cells"] == ref.n_cells and ref.n_cells == {0.5: 151}.get(voxel, ref.n_cells)

    def same(rd):
        rd = _sorted(rd)
        assert rd["slots"] >= 2 * ref.n_cells and rd["slots"] & (rd["slots"] - 1) == 0
        assert np.array_equal(rd["key"], ref.keys[want]) and np.array_equal(rd["key"], h["key"][ref.rows][want])
        assert np.array_equal(rd["W"], h["W"][ref.rows][want])                          # bit for bit
        assert np.array_equal(rd["c"][:, :3], pv["rec"][ref.rows][want][:, :3]) and np.array_equal(rd["c"][:, 3], pv["rec"][ref.rows][want][:, 11])
        return rd

    a = same(m.read())
    assert np.array_equal(a["row"], ref.rows[want])
    # device arrays, read in place
    d_rec, d_cov = _dev(hip, C, pv["rec"]), _dev(hip, C, pv["cov"])
    m2 = ctx.surfel_map()
    assert m2.build(d_rec, d_cov, voxel, rr.SIGMA, rr.MIN_COUNT, n=len(pv["rec"])) == ref.n_cells
    assert np.array_equal(same(m2.read())["row"], ref.rows[want])
    # from the stores: the export with min_count already applied, rows are those of the kept records
    m3 = ctx.surfel_map()
    assert m3.build_from_kf([world["stores"][name]], 1, voxel, rr.SIGMA, rr.MIN_COUNT) == ref.n_cells
    assert np.array_equal(same(m3.read())["row"], np.argsort(np.argsort(ref.rows))[want])
    # mixed sides are refused, the map stays as it was
    with pytest.raises(capi.VbaError) as e:
        ctx._chk(ctx.lib.vba_surfel_map_build(m2.h, len(pv["rec"]), d_rec, pv["cov"].ctypes.data_as(C.c_void_p), voxel, rr.SIGMA, 5, C.byref(C.c_int64())))
    assert e.value.status == capi.ERR_BAD_ARG and m2.size()[0] == ref.n_cells
    assert hip.hipFree(d_rec) == 0 and hip.hipFree(d_cov) == 0
    m2.close(); m3.close()


def test_build_refusals_filter_and_rebuild(capi, world):
    ctx, C = world["ctx"], capi.C
    sc = world["sc"]["near"]; pv = sc["per"][0.5]
    m = ctx.surfel_map()
    assert m.size()[0] == 0
    n = C.c_int64(-77)
    rec, cov = pv["rec"], pv["cov"]
    rp, cp = rec.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p)
    for args in ((len(rec), rp, cp, 0.5, 0.99e-4, 5), (len(rec), rp, cp, 0.0009, 0.02, 5), (len(rec), rp, cp, 0.5, 0.02, 0), (-1, rp, cp, 0.5, 0.02, 5),
                 (len(rec), None, cp, 0.5, 0.02, 5), (len(rec), rp, None, 0.5, 0.02, 5), (len(rec), rp, cp, float("nan"), 0.02, 5)):
        assert ctx.lib.vba_surfel_map_build(m.h, *args, C.byref(n)) == capi.ERR_BAD_ARG and n.value == -77, args
    assert ctx.lib.vba_surfel_map_build(m.h, len(rec), rp, cp, 0.5, 0.02, 5, None) == capi.ERR_BAD_ARG
    hs = (C.c_void_p * 1)(world["stores"]["near"].h)
    for args in ((0, hs, 1, 0.5, 0.02, 5), (1, None, 1, 0.5, 0.02, 5), (1, hs, 0, 0.5, 0.02, 5), (1, hs, 1, 0.5, 1e-5, 5), (1, hs, 1, 0.5, 0.02, 0)):
        assert ctx.lib.vba_surfel_map_build_from_kf(m.h, *args, C.byref(n)) == capi.ERR_BAD_ARG and n.value == -77, args
    # the min_count filter
    assert m.build(rec, cov, 0.5, rr.SIGMA, 1) == len(rec) and m.build(rec, cov, 0.5, rr.SIGMA, 5) == 151
    assert m.build(rec, cov, 0.5, rr.SIGMA, 10 ** 6) == 0 and m.size()[0] == 0
    # records made at 0.5 m keyed at 1 m meet in one key: refused, the map is empty, a registration against it is refused
    assert m.build(rec, cov, 0.5, rr.SIGMA, 5) == 151
    with pytest.raises(capi.VbaError) as e:
        m.build(rec, cov, 1.0, rr.SIGMA, 5)
    assert e.value.status == capi.ERR_BAD_ARG and m.size()[0] == 0
    with pytest.raises(capi.VbaError) as e:
        m.register(sc["pnt"], sc["Rg"], sc["tg"])
    assert e.value.status == capi.ERR_BAD_ARG
    # rebuilt on the same object after set_poses on a copy of the store: the map of the moved records
    store = _store(ctx, world["clouds"], world["poses"]["near"])
    assert m.build_from_kf([store], 1, 0.5, rr.SIGMA, 5) == 151
    before = _sorted(m.read())
    moved = np.array(world["poses"]["near"]); moved[:, 9:12] += np.array([0.125, -0.25, 0.375])
    store.set_poses(0, moved)
    nc = m.build_from_kf([store], 1, 0.5, rr.SIGMA, 5)
    rec2, cov2, _ = ctx.kf_export_surfel([store], [2.0], 1, 0.5, 5)
    ref2 = rr.Map(rec2, cov2, 0.5, rr.SIGMA, 5)
    after = _sorted(m.read())
    o = np.argsort(ref2.keys)
    assert nc == ref2.n_cells and np.array_equal(after["key"], ref2.keys[o]) and np.array_equal(after["W"], ref2.W[ref2.rows][o])
    assert not np.array_equal(after["key"], before["key"])
    store.close(); m.close()


def test_no_allocation_after_reserve(capi, world):
    ctx = world["ctx"]
    sc = world["sc"]["near"]
    m = ctx.surfel_map()
    assert m.allocations() == (0, 0)
    m.reserve(400, 2000)
    base = m.allocations()
    assert base[0] >= 9 and base[1] >= 1024 * 16 + 400 * (64 + 96) + 2000 * 24 + 1024 * 29 * 8
    m.reserve(100, 100)
    assert m.allocations() == base
    for voxel in rr.VOXELS:
        pv = sc["per"][voxel]
        m.build(pv["rec"], pv["cov"], voxel, rr.SIGMA, 5)
        m.register(sc["pnt"], *rr.start_of(sc["Rg"], sc["tg"], "small"))
        m.build_from_kf([world["stores"]["near"]], 1, voxel, rr.SIGMA, 1)
        m.register(sc["pnt"], *rr.start_of(sc["Rg"], sc["tg"], "small"))
    assert m.allocations() == base
    # beyond the reservation: more records (a finer export), more points; the results do not change with the growth
    rec, cov, _ = ctx.kf_export_surfel([world["stores"]["near"]], [2.0], 1, 0.125, 1)
    assert len(rec) > 400
    assert m.build(rec, cov, 0.125, rr.SIGMA, 1) == len(rec)
    grown = m.allocations()
    assert grown[0] > base[0] and grown[1] > base[1]
    pv = sc["per"][0.5]
    m.build(pv["rec"], pv["cov"], 0.5, rr.SIGMA, 5)
    big = np.concatenate([sc["pnt"], sc["pnt"]])
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    a = m.register(big, R0, t0)
    assert m.allocations()[0] > grown[0]
    b = _map(world, "near", 0.5).register(big, R0, t0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and bytes(a[2]) == bytes(b[2])
    m.close()


def test_staging_larger_than_table_and_cells(capi, world):
    """The record staging and the table with its cells grow on their own (a build from device arrays needs no staging), so the
    staging can come to hold more records than table and cells do: a device build of 100 records, host builds of 40 and 100 (the
    staging doubles 40 -> 80 -> 160), then 151 records from the stores, which fit the staging and not the cells.  The build sizes
    table and cells on every path; the map is the host program's."""
    ctx, hip, C = world["ctx"], world["hip"], capi.C
    sc = world["sc"]["near"]; pv = sc["per"][0.5]; ref = pv["ref"]
    rec, cov = pv["rec"], pv["cov"]
    m = ctx.surfel_map()
    d_rec, d_cov = _dev(hip, C, np.ascontiguousarray(rec[:100])), _dev(hip, C, np.ascontiguousarray(cov[:100]))
    assert m.build(d_rec, d_cov, 0.5, rr.SIGMA, 1, n=100) == 100
    a0 = m.allocations()
    assert m.build(rec[:40], cov[:40], 0.5, rr.SIGMA, 1) == 40 and m.build(rec[:100], cov[:100], 0.5, rr.SIGMA, 1) == 100
    a1 = m.allocations()
    assert a1[1] - a0[1] == (40 + 160) * 96                                       # staging alone grew: 40, then 160 records of 48 + 48 B
    assert m.build_from_kf([world["stores"]["near"]], 1, 0.5, rr.SIGMA, rr.MIN_COUNT) == ref.n_cells == 151
    a2 = m.allocations()
    assert a2[0] == a1[0] + 2 and a2[1] - a1[1] == 512 * 16 + 200 * 64            # table and cells for 200 records, no staging
    h = _host(world, pv, sc["pnt"][:4], sc["Rg"], sc["tg"], 0.5, tag="grow")
    want = np.argsort(ref.keys)
    rd = _sorted(m.read())
    assert rd["slots"] == 512 and np.array_equal(rd["key"], h["key"][ref.rows][want]) and np.array_equal(rd["W"], h["W"][ref.rows][want])
    assert np.array_equal(rd["c"][:, :3], rec[ref.rows][want][:, :3]) and np.array_equal(rd["row"], np.arange(151)[want])
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    a = m.register(sc["pnt"], R0, t0); b = _map(world, "near", 0.5).register(sc["pnt"], R0, t0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and bytes(a[2]) == bytes(b[2])
    assert hip.hipFree(d_rec) == 0 and hip.hipFree(d_cov) == 0
    m.close()


# ---------------------------------------------------------------- one pass
def _check_pass(world, m, pv, pnt, R, t, voxel, nb, what, min_count=rr.MIN_COUNT, full_rank=True, ref=None):
    """full_rank False: fewer points than fix six degrees of freedom (n = 1: H has rank 3).  g = J^T W d lies in the range of H, so
    the system is consistent and the LDLT, which divides by no vanishing pivot, returns a finite step that meets the backward bar;
    the forward bar, which divides by the condition number, is asked only of a full-rank H."""
    p = world["capi"].surfel_reg_default_params(neighbors=nb, min_matches=1)
    got = m.debug_pass(pnt, R, t, p)
    h = _host(world, pv, pnt, R, t, voxel, neighbors=nb, max_iter=1, min_matches=1, min_count=min_count, tag="pass")
    assert np.array_equal(got["cell"], h["cell"]) and np.array_equal(got["gate"], h["gate"]), what
    ps = rr.one_pass(ref if ref is not None else pv["ref"], pnt, R, t, 3.0, nb)
    assert np.array_equal(got["cell"], ps["cell"]) and np.array_equal(got["gate"].astype(bool), ps["gate"]), what
    exact, ab = rr.exact_sums(ps)
    bar = rr.sums_bar(int(ps["gate"].sum()), ab)
    err = np.abs(got["sums"] - exact)
    ratio = float((err[:28] / np.maximum(bar[:28], 1e-300)).max()) if ps["gate"].any() else float(err.max())
    assert got["sums"][28] == ps["gate"].sum() and ratio <= 1.0, (what, ratio)
    assert np.array_equal(got["sums"], h["sums"]), what                              # the kernels' order, restated by the host program
    # the step: the host program's bits (the same header on the same sums), the pose after it within the spacing of two libraries'
    # sin and cos, and the exact residual of H dx = -g
    assert np.array_equal(got["dx"], h["dx"]) and np.isfinite(got["dx"]).all() and got["dx"].any() and h["singular"] == 0 and h["lost"] == 0, what
    assert np.abs(got["R"] - h["R"]).max() <= 4 * 2.0 ** -52 and np.abs(got["t"] - h["t"]).max() <= 4 * np.spacing(np.abs(h["t"]).max()), what
    assert np.array_equal(got["t"], np.asarray(t) + got["dx"][3:]), what
    H, g = rr.unpack_H(got["sums"]), got["sums"][21:27]
    r = rr.solve_ref.residual(H, got["dx"], -g)
    bw = np.abs(r).max() / (np.abs(H).sum(axis=1).max() * np.abs(got["dx"]).max() + np.abs(g).max()) / (rr.solve_ref.C_BAR * 6 * rr.U)
    assert bw <= 1.0, (what, bw)
    if full_rank:
        bw2, fw = rr.step_check(got["sums"], got["dx"])
        assert bw2 <= 1.0 and fw <= 1.0, (what, bw2, fw)
    else:
        assert np.linalg.matrix_rank(H) < 6, what
    print("%s: %d points, %d gated, %d without a cell, sum error / bar %.4f" % (what, len(pnt), ps["gate"].sum(), (ps["cell"] < 0).sum(), ratio))
    return got, ps


@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", rr.VOXELS)
@pytest.mark.parametrize("nb", [1, 7])
def test_one_pass_at_every_size(capi, world, name, voxel, nb):
    world["capi"] = capi
    sc = world["sc"][name]; pv = sc["per"][voxel]
    m = _map(world, name, voxel)
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    for n in SIZES:
        pnt = sc["pnt"][-n:] if n < 1564 else sc["pnt"]
        got, ps = _check_pass(world, m, pv, pnt, R0, t0, voxel, nb, "%s voxel %g neighbors %d n %d" % (name, voxel, nb, n), full_rank=n >= 63)
    # the scene has cells with a negative axis index, and points choose them
    chosen = rr.axis_keys(pv["rec"][ps["cell"][ps["cell"] >= 0], :3], voxel)
    assert (chosen < 0).any() and (chosen > 0).any()


def test_one_pass_edge_scans(capi, world):
    world["capi"] = capi
    ctx = world["ctx"]
    sc = world["sc"]["near"]; pv = sc["per"][0.5]
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    # points outside every cell: each probe ends at an empty slot
    rng = np.random.default_rng(5)
    pnt = np.concatenate([sc["pnt"][:200], sc["pnt"][:100] + 50.0, rng.uniform(-2000, 2000, (300, 3))])
    got, ps = _check_pass(world, _map(world, "near", 0.5), pv, pnt, R0, t0, 0.5, 7, "misses")
    assert (got["cell"][200:] == -1).all() and (got["gate"][200:] == 0).all() and got["gate"][:200].sum() > 150
    # every record a cell: the table at its smallest legal size for its cells, so probes chain
    m1 = _map(world, "near", 0.5, 1)
    rd = m1.read()
    n_all = len(pv["rec"])
    assert len(rd["key"]) == n_all and rd["slots"] >= 2 * n_all and rd["slots"] < 4 * n_all
    home = np.array([rr_hash(int(k)) & (rd["slots"] - 1) for k in rd["key"]])
    assert (home != rd["slot"]).sum() >= 5                                           # (keys that sit behind another key)
    ref1 = rr.Map(pv["rec"], pv["cov"], 0.5, rr.SIGMA, 1)
    _check_pass(world, m1, pv, sc["pnt"], R0, t0, 0.5, 7, "every record a cell", min_count=1, ref=ref1)
    # a map of one cell
    one = ctx.surfel_map()
    big = int(np.argmax(pv["rec"][:, 11]))
    pv1 = dict(rec=pv["rec"][big:big + 1], cov=pv["cov"][big:big + 1])
    assert one.build(pv1["rec"], pv1["cov"], 0.5, rr.SIGMA, 5) == 1 and one.read()["slots"] == 2
    ref = rr.Map(pv1["rec"], pv1["cov"], 0.5, rr.SIGMA, 5)
    got, ps = _check_pass(world, one, pv1, sc["pnt"], sc["Rg"], sc["tg"], 0.5, 7, "one cell", ref=ref)
    assert 50 <= got["gate"].sum() < 600 and set(got["cell"]) == {-1, 0}
    # the constructed tie: own and -x give the same m, own is taken
    rec, cov, p1, R, t = rr.tie_case()
    assert one.build(rec, cov, 0.5, rr.SIGMA, 5) == 2
    got = one.debug_pass(p1, R, t, capi.surfel_reg_default_params(min_matches=1))
    ps = rr.one_pass(rr.Map(rec, cov, 0.5, rr.SIGMA, 5), p1, R, t, 3.0, 7)
    assert ps["ties"].all() and got["cell"][0] == 1 and got["gate"][0] == 1 and np.array_equal(got["sums"], ps["sums"])
    one.close()


def rr_hash(k):
    """ds_hash"""
    M = (1 << 64) - 1
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & M; k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & M; k ^= k >> 33
    return k & 0xFFFFFFFF


# ---------------------------------------------------------------- the loop
def _report(rep):
    return dict(iters=rep.iters, converged=rep.converged, lost=rep.lost, singular=rep.singular, matches=np.array(rep.matches), cost=np.array(rep.cost),
                step_rot=np.array(rep.step_rot), step_tra=np.array(rep.step_tra), H=np.array(rep.H), g=np.array(rep.g), eig_tt=np.array(rep.eig_tt))


@pytest.mark.parametrize("case", rr.LOOP_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_loop_equals_the_host_programs(capi, world, case):
    name, which, nb = case
    voxel = rr.LOOP_VOXEL[which]
    sc = world["sc"][name]; pv = sc["per"][voxel]
    m = _map(world, name, voxel)
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], which)
    p = capi.surfel_reg_default_params(neighbors=nb)
    R, t, rep = m.register(sc["pnt"], R0, t0, p)
    g = _report(rep)
    h = _host(world, pv, sc["pnt"], R0, t0, voxel, neighbors=nb, max_iter=30, tag="loop")
    k = h["iters"]
    assert (g["iters"], g["converged"], g["lost"], g["singular"]) == (k, 1, 0, 0) and h["converged"] == 1
    assert np.array_equal(g["matches"][:k], h["matches"][:k]) and (g["matches"][k:] == 0).all() and g["matches"][k - 1] >= 0.95 * len(sc["pnt"])
    # 4 x the measured spread of the restatement over 16 starts 1e-12 apart (surfreg_ref.SPREAD, floors in pose_bars)
    bR, bt, bc = rr.pose_bars(case, h["t"])
    eR, et = np.abs(R - h["R"]).max(), np.abs(t - h["t"]).max()
    ec = (np.abs(g["cost"][:k] - h["cost"][:k]) / np.abs(h["cost"][:k])).max()
    print("%s: %d iterations; |R - host| %.2e (bar %.2e), |t - host| %.2e (bar %.2e), cost %.2e (bar %.2e)" % (case, k, eR, bR, et, bt, ec, bc))
    assert eR <= bR and et <= bt and ec <= bc
    dt, dr = rr.pose_distance(R, t, sc["Rg"], sc["tg"])
    assert dt < voxel / 100 and dr < voxel / 100
    # the degeneracy figure: the eigenvalues of the translation block of the last H
    tt = g["H"][15:21]
    ref = er.Ref(sr.sym(tt))
    assert max(abs(g["eig_tt"][i] - ref.w[i]) for i in range(3)) <= er.C_BAR * er.EPS * ref.s and g["eig_tt"][0] > 1e5
    # two calls, and host or device points: the same bytes
    R2, t2, rep2 = m.register(sc["pnt"], R0, t0, p)
    assert R.tobytes() == R2.tobytes() and t.tobytes() == t2.tobytes() and bytes(rep) == bytes(rep2)
    d = _dev(world["hip"], capi.C, np.ascontiguousarray(sc["pnt"]))
    R3, t3, rep3 = m.register(d, R0, t0, p, n=len(sc["pnt"]))
    assert R.tobytes() == R3.tobytes() and t.tobytes() == t3.tobytes() and bytes(rep) == bytes(rep3)
    assert world["hip"].hipFree(d) == 0


def test_loop_ends_and_refusals(capi, world):
    C = capi.C
    sc = world["sc"]["near"]; pv = sc["per"][0.5]
    m = _map(world, "near", 0.5)
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    n = len(sc["pnt"])
    # lost: more matches asked for than there are points; the pose is untouched
    R, t, rep = m.register(sc["pnt"], R0, t0, capi.surfel_reg_default_params(min_matches=n + 1))
    assert (rep.iters, rep.converged, rep.lost, rep.singular) == (1, 0, 1, 0) and R.tobytes() == R0.tobytes() and t.tobytes() == t0.tobytes()
    assert 0.9 * n < rep.matches[0] <= n and rep.step_tra[0] == 0.0
    # a scan 50 m away
    R, t, rep = m.register(sc["pnt"] + 50.0, R0, t0)
    assert rep.lost == 1 and rep.iters == 1 and rep.matches[0] < 50 and R.tobytes() == R0.tobytes() and t.tobytes() == t0.tobytes()
    # the iteration limit
    R, t, rep = m.register(sc["pnt"], R0, t0, capi.surfel_reg_default_params(max_iter=1))
    assert (rep.iters, rep.converged, rep.lost) == (1, 0, 0) and rep.step_tra[0] > 1e-3 and not np.array_equal(t, t0)
    h = _host(world, pv, sc["pnt"], R0, t0, 0.5, neighbors=7, max_iter=1, tag="one")
    assert np.abs(t - h["t"]).max() <= 4 * np.spacing(np.abs(t).max())
    # wall points only: the translation along the wall is weakly held
    wall = sc["pnt"][np.abs((sc["pnt"] @ sc["Rg"].T + sc["tg"])[:, 0] - 3.3) < 0.05]
    assert len(wall) > 300
    R, t, rep = m.register(wall, sc["Rg"], sc["tg"], capi.surfel_reg_default_params(max_iter=2))
    assert rep.lost == 0 and rep.eig_tt[0] < 0.05 * rep.eig_tt[2]                   # (the whole scan: about 0.25)
    # refusals, before any device work, outputs untouched
    pnt = np.ascontiguousarray(sc["pnt"]); pp = pnt.ctypes.data_as(C.c_void_p)
    Rb = np.array(R0).reshape(9).copy(); tb = np.array(t0).copy(); rp, tp = Rb.ctypes.data_as(C.c_void_p), tb.ctypes.data_as(C.c_void_p)
    rep = capi.SurfelRegReport(); rep.iters = -5
    ok = capi.surfel_reg_default_params()
    bad = [capi.surfel_reg_default_params(neighbors=3), capi.surfel_reg_default_params(max_iter=0), capi.surfel_reg_default_params(max_iter=33),
           capi.surfel_reg_default_params(gate=0.0), capi.surfel_reg_default_params(gate=-1.0)]
    lib = world["ctx"].lib
    for q in bad:
        assert lib.vba_surfel_register(m.h, n, pp, C.byref(q), rp, tp, C.byref(rep)) == capi.ERR_BAD_ARG
    for args in ((None, n, pp, C.byref(ok), rp, tp), (m.h, 0, pp, C.byref(ok), rp, tp), (m.h, n, None, C.byref(ok), rp, tp), (m.h, n, pp, None, rp, tp),
                 (m.h, n, pp, C.byref(ok), None, tp), (m.h, n, pp, C.byref(ok), rp, None)):
        assert lib.vba_surfel_register(*args, C.byref(rep)) == capi.ERR_BAD_ARG
        assert lib.vba_debug_surfel_reg_pass(*args, None, None, None, None) == capi.ERR_BAD_ARG
    empty = world["ctx"].surfel_map()
    assert lib.vba_surfel_register(empty.h, n, pp, C.byref(ok), rp, tp, C.byref(rep)) == capi.ERR_BAD_ARG
    empty.close()
    assert rep.iters == -5 and np.array_equal(Rb, np.array(R0).reshape(9)) and np.array_equal(tb, t0)


# ---------------------------------------------------------------- the adapter
def test_adapter_program(capi, world):
    """vba::SurfelMap built from stores and vba::relocalize on keyframes of another session's store, through
    tests/host/surfreg_adapter_host.cpp: the pose of the keyframe that holds the scan is the Python result, the keyframe 50 m away
    returns false with x untouched"""
    ctx = world["ctx"]
    sc = world["sc"]["near"]
    clouds, poses = world["clouds"], world["poses"]["near"]
    scans = [np.ascontiguousarray(sc["pnt"]), np.ascontiguousarray(sc["pnt"] + 50.0)]
    ident = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    fin, fout = str(world["dir"] / "adapter_in.bin"), str(world["dir"] / "adapter_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", 2))
        for cl, ps in ((clouds, poses), (scans, [ident, ident])):
            f.write(struct.pack("<i", len(cl)))
            for c, x in zip(cl, ps):
                f.write(struct.pack("<i", len(c))); f.write(np.ascontiguousarray(x, dtype=np.float64).tobytes()); f.write(np.ascontiguousarray(c).tobytes())
        f.write(np.ascontiguousarray(R0).tobytes()); f.write(np.ascontiguousarray(t0).tobytes())
    exe = rr.build_adapter(world["dir"], capi.LIB_PATH)
    r = subprocess.run([exe, fin, fout, "0.5", repr(rr.SIGMA), str(rr.MIN_COUNT), repr(sr.GRID)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = open(fout, "rb").read()
    cells = struct.unpack_from("<q", raw, 0)[0]
    got = [(struct.unpack_from("<ii", raw, 8 + 104 * k), np.frombuffer(raw, dtype=np.float64, count=12, offset=16 + 104 * k)) for k in range(2)]
    # the same in Python: the scans as keyframes of a second store, registered in place
    other = ctx.kf_store()
    for k, c in enumerate(scans):
        other.build([c], ident[None, :], sr.GRID, id=k, jour=float(k))
    m = ctx.surfel_map()
    assert m.build_from_kf([world["stores"]["near"]], 1, 0.5, rr.SIGMA, rr.MIN_COUNT) == cells == 151
    d, off, n_kf = other.clouds()
    assert n_kf == 2 and off[1] > 1500
    R, t, rep = m.register(d + 24 * int(off[0]), R0, t0, n=int(off[1] - off[0]))
    (ok, iters), x = got[0]
    assert ok == 1 and rep.converged == 1 and iters == rep.iters and x[:9].tobytes() == R.tobytes() and x[9:].tobytes() == t.tobytes()
    dt, dr = rr.pose_distance(R, t, sc["Rg"], sc["tg"])
    assert dt < 0.005 and dr < 0.005
    (ok, iters), x = got[1]
    assert ok == 0 and iters == 1 and x[:9].tobytes() == np.ascontiguousarray(R0).tobytes() and x[9:].tobytes() == np.ascontiguousarray(t0).tobytes()
    m.close(); other.close()
