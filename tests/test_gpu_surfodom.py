"""The prior-map odometry update (vba_odom_surfel_update, vba_odom_surfel_update_on_state, vba_debug_odom_surfel_sums, DESIGN.md
section 27) on the MI355X against the host build of csrc/vba_surfreg_math.hpp + csrc/vba_odom_ekf.hpp
(tests/host/surfodom_host.cpp) and the numpy restatement tests/surfodom_ref.py, which tests/test_surfodom_cpu.py holds to each other
and to exact sums.

Bars.  One point loop: cell and gate equal the host program's for every point; the workgroup rows, their costs and the 34 sums are
its bits (it restates the kernels' order) and within surfreg_ref.sums_bar (any order of the additions) of the exact sums.  The
loop: iterations, match_num[] and ok equal the host program's; state, covariance, rot_add[] and tra_add[] are within
surfodom_ref.bars, 4 x the spread the host program shows over 16 priors 1e-12 apart (measured: 9e-15 .. 1.3e-14 on R, 0 .. 1.1e-13
on p, 1.9e-12 on v / bg / ba, 6e-15 .. 1.2e-14 of the largest covariance entry, 2.2e-12 .. 3.2e-12 on rot_add[] and tra_add[]),
never below 4 units in the last place."""
import struct
import subprocess

import numpy as np
import pytest

import surfodom_ref as so
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


@pytest.fixture(scope="module")
def world(capi, tmp_path_factory):
    """a deterministic context, the scenes of surfreg_ref with their records at both voxel sizes, the scans, the prior, the host
    program; maps and host runs are made once and shared"""
    o = capi.default_options(); o.device = 0; o.deterministic = 1
    ctx = capi.Context(o)
    d = tmp_path_factory.mktemp("surfodom_gpu")
    w = dict(ctx=ctx, capi=capi, exe=so.build_host(d), dir=d, hip=_hip(), sc={}, cache={}, P=so.prior_cov())
    for name in ("near", "far"):
        _, S = rr.world(name)
        pnt, Rg, tg = rr.scan_of(S, name)
        per = {}
        for voxel in rr.VOXELS:
            rec, cov = rr.records_of(S, voxel)
            per[voxel] = dict(rec=rec, cov=cov, ref=rr.Map(rec, cov, voxel, rr.SIGMA, rr.MIN_COUNT))
        w["sc"][name] = dict(pnt=np.ascontiguousarray(pnt), Rg=Rg, tg=tg, per=per)
    yield w
    for k, m in w["cache"].items():
        if k[0] == "map":
            m.close()
    ctx.close()


def _map(world, name, voxel, ctx=None):
    k = ("map", name, voxel, id(ctx) if ctx is not None else 0)
    if k not in world["cache"]:
        m = (ctx or world["ctx"]).surfel_map()
        pv = world["sc"][name]["per"][voxel]
        assert m.build(pv["rec"], pv["cov"], voxel, rr.SIGMA, rr.MIN_COUNT) == pv["ref"].n_cells
        world["cache"][k] = m
    return world["cache"][k]


def _inputs(world, name, voxel, which):
    sc = world["sc"][name]; pv = sc["per"][voxel]
    R0, t0 = so.start_of(sc["Rg"], sc["tg"], which)
    return sc, pv, R0, t0, so.state_of(R0, t0), world["P"]


def _host(world, pv, pnt, state, P, voxel, **kw):
    return so.host_run(world["exe"], world["dir"], pv["rec"], pv["cov"], pnt, state, P, voxel, **kw)


def _result(ok, state, cov, rep):
    return dict(ok=int(ok), state=state, cov=np.asarray(cov).reshape(15, 15), iterations=rep["iterations"], match_num=rep["match_num"],
                rot_add=rep["rot_add"], tra_add=rep["tra_add"], eig_min=rep["nnt_eig_min"])


def _same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("state", "cov", "match_num", "rot_add", "tra_add")) and \
        (a["ok"], a["iterations"], a["eig_min"]) == (b["ok"], b["iterations"], b["eig_min"])


# ---------------------------------------------------------------- one point loop
def _check_sums(world, m, pv, pnt, R, t, voxel, nb, what, ref=None, exact=True):
    p = world["capi"].surfel_odom_default_params(neighbors=nb)
    got = world["ctx"].debug_odom_surfel_sums(m, pnt, R, t, p)
    h = _host(world, pv, pnt, so.state_of(R, t), world["P"], voxel, neighbors=nb, tag="sums")
    assert got["nb"] == h["nb"] == so.blocks(len(pnt)), what
    assert np.array_equal(got["cell"], h["cell"]) and np.array_equal(got["gate"], h["gate"]), what
    assert np.array_equal(got["partial"], h["partial"]) and np.array_equal(got["cost"], h["cost"]) and np.array_equal(got["sums"], h["sums"]), what
    if not exact:
        return got, None
    ps = rr.one_pass(ref if ref is not None else pv["ref"], pnt, R, t, 3.0, nb)
    assert np.array_equal(got["cell"], ps["cell"]) and np.array_equal(got["gate"].astype(bool), ps["gate"]), what
    ex, bar = so.exact34(ps)
    err = np.abs(got["sums"] - ex)
    ratio = float((err[:33] / np.maximum(bar[:33], 1e-300)).max()) if ps["gate"].any() else float(err.max())
    assert got["sums"][33] == ps["gate"].sum() and ratio <= 1.0, (what, ratio)
    print("%s: %d points, %d gated, %d without a cell, sum error / bar %.4f" % (what, len(pnt), ps["gate"].sum(), (ps["cell"] < 0).sum(), ratio))
    return got, ps


@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", rr.VOXELS)
@pytest.mark.parametrize("nb", [1, 7])
def test_one_point_loop_at_every_size(world, name, voxel, nb):
    sc, pv, R0, t0, state, P = _inputs(world, name, voxel, "track")
    m = _map(world, name, voxel)
    for n in SIZES:
        pnt = sc["pnt"][-n:] if n < 1564 else sc["pnt"]
        got, ps = _check_sums(world, m, pv, pnt, R0, t0, voxel, nb, "%s voxel %g neighbors %d n %d" % (name, voxel, nb, n))
    # the scene has cells with a negative axis index, and points choose them
    chosen = rr.axis_keys(pv["rec"][ps["cell"][ps["cell"] >= 0], :3], voxel)
    assert (chosen < 0).any() and (chosen > 0).any()
    assert np.array_equal(got["sums"][27:33], got["sums"][15:21]) and got["sums"][21:27].any()


def test_point_loop_beyond_the_grid_cap(world):
    """1024 * 256 + 257 points: 1024 workgroups whose lanes chain over strided tiles; the host program's bits"""
    sc, pv, R0, t0, state, P = _inputs(world, "near", 0.5, "track")
    n = 1024 * 256 + 257
    pnt = np.ascontiguousarray(np.tile(sc["pnt"], (n // len(sc["pnt"]) + 1, 1))[:n])
    got, _ = _check_sums(world, _map(world, "near", 0.5), pv, pnt, R0, t0, 0.5, 7, "capped grid", exact=False)
    assert got["nb"] == 1024 and got["sums"][33] > 0.9 * n


def test_point_loop_edge_scans(world):
    capi, ctx = world["capi"], world["ctx"]
    sc, pv, R0, t0, state, P = _inputs(world, "near", 0.5, "track")
    rng = np.random.default_rng(5)
    pnt = np.concatenate([sc["pnt"][:200], sc["pnt"][:100] + 50.0, rng.uniform(-2000, 2000, (300, 3))])
    got, ps = _check_sums(world, _map(world, "near", 0.5), pv, pnt, R0, t0, 0.5, 7, "misses")
    assert (got["cell"][200:] == -1).all() and (got["gate"][200:] == 0).all() and got["gate"][:200].sum() > 150
    # the constructed tie: own and -x give the same m, own is taken
    rec, cov, p1, R, t = rr.tie_case()
    one = ctx.surfel_map()
    assert one.build(rec, cov, 0.5, rr.SIGMA, 5) == 2
    got = ctx.debug_odom_surfel_sums(one, p1, R, t)
    ps = rr.one_pass(rr.Map(rec, cov, 0.5, rr.SIGMA, 5), p1, R, t, 3.0, 7)
    assert ps["ties"].all() and got["cell"][0] == 1 and got["gate"][0] == 1 and np.array_equal(got["sums"], so.to34(ps["sums"]))
    assert got["cost"][0] == ps["sums"][27]
    one.close()


# ---------------------------------------------------------------- the loop
@pytest.mark.parametrize("case", so.LOOP_CASES, ids=so.case_id)
def test_loop_equals_the_host_programs(world, case):
    capi, ctx, hip = world["capi"], world["ctx"], world["hip"]
    name, voxel, which, nb = case
    sc, pv, R0, t0, state, P = _inputs(world, name, voxel, which)
    m = _map(world, name, voxel)
    p = capi.surfel_odom_default_params(neighbors=nb)
    g = _result(*ctx.odom_surfel_update(m, sc["pnt"], state, P, p))
    h = _host(world, pv, sc["pnt"], state, P, voxel, neighbors=nb, tag="loop")
    k = h["iterations"]
    assert g["iterations"] == k == so.EXPECTED_ITERATIONS[which] and np.array_equal(g["match_num"], h["match_num"]) and g["ok"] == h["ok"] == 1
    err, bar = so.errors(g, h), so.bars(case, h)
    print("%s: %d iterations; R %.2e (bar %.2e), p %.2e (%.2e), v bg ba %.2e (%.2e), cov %.2e (%.2e), rot_add %.2e (%.2e), tra_add %.2e (%.2e)"
          % (so.case_id(case), k, err["R"], bar["R"], err["p"], bar["p"], err["v"], bar["v"], err["P"], bar["P"], err["rot"].max(), bar["rot"].min(),
             err["tra"].max(), bar["tra"].min()))
    assert so.within(err, bar), (err, bar)
    assert (g["rot_add"][k:] == 0).all() and (g["tra_add"][k:] == 0).all()
    assert abs(g["eig_min"] - h["eig_min"]) <= 1e-12 * h["eig_min"] and 4.0e5 < g["eig_min"] < 5.5e5
    dt, dr = so.pose_distance(g["state"], sc["Rg"], sc["tg"])
    assert dt < voxel / 100 and dr < voxel / 100
    # on a state object: state_out, state_get and the covariance equal the host-state call's bit for bit
    st = ctx.odom_state()
    st.set(state, P)
    ok2, s2, rep2 = st.surfel_update(m, sc["pnt"], p)
    sg, cg = st.get()
    assert s2.tobytes() == g["state"].tobytes() == sg.tobytes() and cg.tobytes() == g["cov"].tobytes()
    assert _same_bytes(g, _result(ok2, s2, cg, rep2))
    # two calls, host or device points: the same bytes
    assert _same_bytes(g, _result(*ctx.odom_surfel_update(m, sc["pnt"], state, P, p)))
    d = _dev(hip, capi.C, sc["pnt"])
    assert _same_bytes(g, _result(*ctx.odom_surfel_update(m, d, state, P, p, n=len(sc["pnt"]))))
    st.set(state, P)
    ok3, s3, rep3 = st.surfel_update(m, d, p, n=len(sc["pnt"]))
    assert s3.tobytes() == g["state"].tobytes() and st.get()[1].tobytes() == g["cov"].tobytes()
    assert hip.hipFree(d) == 0
    st.close()


def test_default_context_gives_the_deterministic_contexts_bytes(world):
    capi = world["capi"]
    o = capi.default_options(); o.device = 0
    other = capi.Context(o)
    for case in (("near", 0.5, "small", 7), ("far", 1.0, "fine", 1)):
        name, voxel, which, nb = case
        sc, pv, R0, t0, state, P = _inputs(world, name, voxel, which)
        p = capi.surfel_odom_default_params(neighbors=nb)
        a = _result(*world["ctx"].odom_surfel_update(_map(world, name, voxel), sc["pnt"], state, P, p))
        b = _result(*other.odom_surfel_update(_map(world, name, voxel, other), sc["pnt"], state, P, p))
        assert _same_bytes(a, b), case
    for k in [k for k in world["cache"] if k[0] == "map" and k[3] == id(other)]:
        world["cache"].pop(k).close()
    other.close()


def test_chain_on_a_state_object(world):
    """set -> update -> a second update on the same object, against the host program's chain"""
    capi, ctx = world["capi"], world["ctx"]
    case = ("near", 0.5, "fine", 7)
    sc, pv, R0, t0, state, P = _inputs(world, *case[:3])
    m = _map(world, "near", 0.5)
    h1 = _host(world, pv, sc["pnt"], state, P, 0.5, tag="chain1")
    h2 = _host(world, pv, sc["pnt"], h1["state"], h1["cov"], 0.5, tag="chain2")
    assert (h1["iterations"], h2["iterations"]) == (3, 2)
    st = ctx.odom_state()
    st.set(state, P)
    ok1, s1, r1 = st.surfel_update(m, sc["pnt"])
    ok2, s2, r2 = st.surfel_update(m, sc["pnt"])
    sg, cg = st.get()
    assert (ok1, ok2) == (True, True) and (r1["iterations"], r2["iterations"]) == (3, 2)
    assert np.array_equal(r1["match_num"], h1["match_num"]) and np.array_equal(r2["match_num"], h2["match_num"])
    g = dict(state=sg, cov=cg, rot_add=r2["rot_add"], tra_add=r2["tra_add"])
    # two updates: the first one's difference (within its bar) is the second one's input, and a converged update hands it on
    bar = so.bars(case, h2)
    bar = {k: 2 * v for k, v in bar.items()}
    err = so.errors(g, h2)
    print("chain: R %.2e p %.2e v %.2e cov %.2e" % (err["R"], err["p"], err["v"], err["P"]))
    assert so.within(err, bar), (err, bar)
    assert s2.tobytes() == sg.tobytes()
    # the same chain through the host-state call
    a = ctx.odom_surfel_update(m, sc["pnt"], state, P)
    b = ctx.odom_surfel_update(m, sc["pnt"], a[1], a[2])
    assert b[1].tobytes() == sg.tobytes() and b[2].tobytes() == cg.tobytes()
    st.close()


# ---------------------------------------------------------------- degenerate and filtered forms
def test_degenerate_and_filtered_forms(world):
    capi, ctx = world["capi"], world["ctx"]
    sc, pv, R0, t0, state, P = _inputs(world, "near", 0.5, "track")
    m = _map(world, "near", 0.5)
    n = len(sc["pnt"])
    st = ctx.odom_state()
    for pnt in (sc["pnt"] + 50.0, np.zeros((0, 3))):
        # no match at all / no point at all: the prediction, bit for bit
        ok, s, c, rep = ctx.odom_surfel_update(m, pnt, state, P)
        assert not ok and rep["iterations"] == 2 and (rep["match_num"] == 0).all() and rep["nnt_eig_min"] == 0.0
        assert s.tobytes() == state.tobytes() and c.tobytes() == P.tobytes()
        st.set(state, P)
        ok, s, rep = st.surfel_update(m, pnt)
        sg, cg = st.get()
        assert not ok and rep["iterations"] == 2 and s.tobytes() == state.tobytes() == sg.tobytes() and cg.tobytes() == P.tobytes()
    assert ctx.odom_surfel_update(m, np.zeros((0, 3)), state, P, capi.surfel_odom_default_params(min_matches=0))[0] is True
    # more matches asked for than there are: not ok, the state updated all the same
    full = ctx.odom_surfel_update(m, sc["pnt"], state, P)
    ok, s, c, rep = ctx.odom_surfel_update(m, sc["pnt"], state, P, capi.surfel_odom_default_params(min_matches=n + 1))
    assert full[0] and not ok and s.tobytes() == full[1].tobytes() and c.tobytes() == full[2].tobytes() and rep["match_num"][3] > 0.95 * n
    # wall points only: the direction along the wall is weakly held.  min_eig at the geometric mean of the two eigenvalues as the
    # host program measures them
    wall = np.ascontiguousarray(sc["pnt"][np.abs((sc["pnt"] @ sc["Rg"].T + sc["tg"])[:, 0] - 3.3) < 0.05])
    assert len(wall) > 300
    xg = so.state_of(sc["Rg"], sc["tg"])
    e_wall = _host(world, pv, wall, xg, P, 0.5, tag="wall")["eig_min"]; e_all = _host(world, pv, sc["pnt"], xg, P, 0.5, tag="whole")["eig_min"]
    assert 0 < e_wall < 0.2 * e_all
    p = capi.surfel_odom_default_params(min_eig=float(np.sqrt(e_wall * e_all)))
    a = ctx.odom_surfel_update(m, wall, xg, P, p); b = ctx.odom_surfel_update(m, sc["pnt"], xg, P, p)
    print("wall only: eig %.4g (host %.4g), whole scan %.4g (host %.4g), min_eig %.4g" % (a[3]["nnt_eig_min"], e_wall, b[3]["nnt_eig_min"], e_all, p.min_eig))
    assert not a[0] and b[0] and a[3]["match_num"][a[3]["iterations"] - 1] > 250
    st.close()


def test_refusals_leave_everything_untouched(world):
    capi, ctx, hip = world["capi"], world["ctx"], world["hip"]
    C = capi.C
    sc, pv, R0, t0, state, P = _inputs(world, "near", 0.5, "track")
    m = _map(world, "near", 0.5)
    lib = ctx.lib
    n = len(sc["pnt"]); pp = sc["pnt"].ctypes.data_as(C.c_void_p)
    sb = state.copy(); cb = np.ascontiguousarray(P).copy(); sp, cp = sb.ctypes.data_as(C.c_void_p), cb.ctypes.data_as(C.c_void_p)
    ok = C.c_int(-77); rep = capi.OdomReport(); rep.iterations = -5; out = np.full(25, -3.0); op = out.ctypes.data_as(C.c_void_p)
    good = capi.surfel_odom_default_params()
    st = ctx.odom_state()
    st.set(state, P)
    empty = ctx.surfel_map()
    o = capi.default_options(); o.device = 0; o.deterministic = 1
    other = capi.Context(o)
    foreign = other.surfel_map()
    assert foreign.build(pv["rec"], pv["cov"], 0.5, rr.SIGMA, rr.MIN_COUNT) == 151
    bad = [capi.surfel_odom_default_params(neighbors=3), capi.surfel_odom_default_params(gate=0.0), capi.surfel_odom_default_params(gate=-1.0),
           capi.surfel_odom_default_params(min_matches=-1), capi.surfel_odom_default_params(min_eig=-1.0), capi.surfel_odom_default_params(gate=float("nan"))]
    calls = [(ctx.h, m.h, n, pp, C.byref(q)) for q in bad] + [(None, m.h, n, pp, C.byref(good)), (ctx.h, None, n, pp, C.byref(good)), (ctx.h, m.h, -1, pp, C.byref(good)),
                                                               (ctx.h, m.h, n, None, C.byref(good)), (ctx.h, m.h, n, pp, None), (ctx.h, empty.h, n, pp, C.byref(good)),
                                                               (ctx.h, foreign.h, n, pp, C.byref(good))]
    for c, mm, nn, ptr, q in calls:
        assert lib.vba_odom_surfel_update(c, mm, nn, ptr, q, sp, cp, C.byref(ok), C.byref(rep)) == capi.ERR_BAD_ARG
        assert lib.vba_odom_surfel_update_on_state(c, st.h, mm, nn, ptr, q, C.byref(ok), C.byref(rep), op) == capi.ERR_BAD_ARG
    assert lib.vba_odom_surfel_update(ctx.h, m.h, n, pp, C.byref(good), None, cp, C.byref(ok), C.byref(rep)) == capi.ERR_BAD_ARG
    assert lib.vba_odom_surfel_update(ctx.h, m.h, n, pp, C.byref(good), sp, None, C.byref(ok), C.byref(rep)) == capi.ERR_BAD_ARG
    assert lib.vba_odom_surfel_update_on_state(ctx.h, None, m.h, n, pp, C.byref(good), C.byref(ok), C.byref(rep), op) == capi.ERR_BAD_ARG
    nb = C.c_int(-77)
    for args in ((ctx.h, m.h, 0, pp, C.byref(good), sp, sp), (ctx.h, m.h, n, pp, C.byref(bad[0]), sp, sp), (ctx.h, m.h, n, pp, C.byref(good), None, sp),
                 (ctx.h, empty.h, n, pp, C.byref(good), sp, sp)):
        assert lib.vba_debug_odom_surfel_sums(*args, 0, None, None, None, None, None, C.byref(nb)) == capi.ERR_BAD_ARG and nb.value == -77
    part = np.zeros((3, 34))
    assert lib.vba_debug_odom_surfel_sums(ctx.h, m.h, n, pp, C.byref(good), sp, sp, 3, part.ctypes.data_as(C.c_void_p), None, None, None, None,
                                          C.byref(nb)) == capi.ERR_CAPACITY and nb.value == 7 and not part.any()
    sg, cg = st.get()
    assert ok.value == -77 and rep.iterations == -5 and (out == -3.0).all() and np.array_equal(sb, state) and np.array_equal(cb, P)
    assert sg.tobytes() == state.tobytes() and cg.tobytes() == np.ascontiguousarray(P).tobytes()
    foreign.close(); other.close(); empty.close(); st.close()


def test_no_allocation_after_reserve_and_a_first_call(world):
    capi, ctx = world["capi"], world["ctx"]
    C = capi.C
    sc, pv, R0, t0, state, P = _inputs(world, "near", 0.5, "track")
    m = ctx.surfel_map()
    m.reserve(400, 2000)
    m.build(pv["rec"], pv["cov"], 0.5, rr.SIGMA, rr.MIN_COUNT)
    st = ctx.odom_state()
    st.set(state, P)
    first = ctx.odom_surfel_update(m, sc["pnt"], state, P)
    st.surfel_update(m, sc["pnt"])
    base = (m.allocations(), st.allocations(), ctx.kdtree_allocations())
    for voxel in rr.VOXELS:
        pv = sc["per"][voxel]
        m.build(pv["rec"], pv["cov"], voxel, rr.SIGMA, rr.MIN_COUNT)
        for nb in (1, 7):
            ctx.odom_surfel_update(m, sc["pnt"], state, P, capi.surfel_odom_default_params(neighbors=nb))
            st.set(state, P)
            st.surfel_update(m, sc["pnt"][:700], capi.surfel_odom_default_params(neighbors=nb))
    assert (m.allocations(), st.allocations(), ctx.kdtree_allocations()) == base
    m.close(); st.close()


# ---------------------------------------------------------------- the adapter
def test_adapter_program(world):
    """vba::lio_state_estimation_prior and vba::OdomState::lio_state_estimation_prior through tests/host/surfodom_adapter_host.cpp:
    the bytes of the Python calls"""
    capi, ctx = world["capi"], world["ctx"]
    sc, pv, R0, t0, state, P = _inputs(world, "near", 0.5, "small")
    fin, fout = str(world["dir"] / "adapter_in.bin"), str(world["dir"] / "adapter_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qq", len(pv["rec"]), len(sc["pnt"])))
        f.write(np.ascontiguousarray(pv["rec"], dtype=np.float32).tobytes()); f.write(np.ascontiguousarray(pv["cov"]).tobytes()); f.write(sc["pnt"].tobytes())
        f.write(state.tobytes()); f.write(np.ascontiguousarray(P).tobytes())
    exe = so.build_adapter(world["dir"], capi.LIB_PATH)
    r = subprocess.run([exe, fin, fout, "0.5", repr(rr.SIGMA), str(rr.MIN_COUNT)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = open(fout, "rb").read()
    assert struct.unpack_from("<q", raw, 0)[0] == 151 and len(raw) == 8 + (8 + 250 * 8) + (8 + 275 * 8)
    ok, s, c, rep = ctx.odom_surfel_update(_map(world, "near", 0.5), sc["pnt"], state, P)
    a_ok, a_it = struct.unpack_from("<ii", raw, 8)
    assert (a_ok, a_it) == (1, rep["iterations"]) and raw[16:16 + 200] == s.tobytes() and raw[216:216 + 1800] == c.tobytes()
    b_ok, b_it = struct.unpack_from("<ii", raw, 2016)
    assert (b_ok, b_it) == (1, rep["iterations"]) and raw[2024:2224] == s.tobytes() and raw[2224:2424] == s.tobytes() and raw[2424:] == c.tobytes()
    dt, dr = so.pose_distance(s, sc["Rg"], sc["tg"])
    assert dt < 0.005 and dr < 0.005
