"""The any-window path on the device (csrc/vba_kernels_big.hpp: k_big_eidx, k_big_slot, k_big_syrk, k_big_diag, k_big_blockdiag,
k_big_residual and the (node, frame) hashed build k_gbab_*), pass by pass through vba_debug_big_*, against the references and bars of
tests/big_ref.py.  The context has win_size = 10, so every W below is "another window size", the path vba_hba_add_edge takes for the
top layer of a hierarchical global BA.
  * Hessian pass, W in 2, 3, 8, 9, 16, 17, 25, 41 (1, 1, 1, 2, 2, 3, 4, 6 frame tiles, the last with 2, 3, 8, 1, 8, 1, 1, 1 frames) x the
    slice counts 0 (the pass's choice), 1, 3, nchunk and nchunk - 1 (empty last slices): store(W) whole, every class loaded as a store of
    its own, origin(W) whole and every voxel loaded alone.  H, g, r within the per-entry bars (each half of H on its own, hess_ref
    sym=False), exact zeros where no voxel sees the frame pair, and the [W][W][6] output of k_big_blockdiag equal bit for bit to the same
    entries of the returned H.
  * Residual pass, same W: loaded with stale eigen-data, run at poses and at true_poses; the stored sums against the double-double
    transform, the stored eigen-data against eig3_ref on the device's own sums, r against the sum of the device's own eigenvalues; then
    a Hessian pass at the same poses against the reference fed the refreshed eigen-data (what an accepted LM step runs).
  * The eigen-solver at its two sites here: k_big_residual on the eig3_ref corpus (one-entry voxels under the identity pose: cov = A
    exactly, eig3_ref's bars unchanged), k_gbab_decide on the designed clouds of tests/test_gpu_eig3.py over 12 keyframes.
  * Build parity with the oracle's OctreeGBA build, W in 3, 9, 17, both parameter sets of vba_hba_add_edge, and the Hessian pass on the
    store the build left.
  * The empty store and the refusals of vba_debug_big_load.
f64 atomics: two runs do not agree bit for bit and nothing here asks them to.  The printed ratios are reports."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import big_ref as B
import eig3_ref as E3
import hess_ref as R

pytestmark = pytest.mark.gpu

WS = [2, 3, 8, 9, 16, 17, 25, 41]
SLICES = ["own", "1", "3", "nchunk", "nchunk-1"]
GBA = dict(gba_voxel_size=2.0, gba_min_eigen_value=0.1, gba_eig=[0.25, 0.25, 0.25, 0.25])


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    o = capi.default_options()
    o.win_size = 10
    c = capi.Context(o)
    yield c
    c.close()


def _slices(kind, V):
    n = B.nchunk(V)
    return {"own": 0, "1": 1, "3": 3, "nchunk": max(n, 1), "nchunk-1": max(n - 1, 1)}[kind]


def _load(ctx, st, idx=None):
    sub = st if idx is None else B.subset(st, idx)
    vptr, efr, ecl = B.to_csr(sub["clusters"])
    ctx.debug_big_load(st["W"], vptr, efr, ecl, sub["eig_val"], sub["eig_vec"], sub["pcr_add"])
    return vptr, efr, ecl


def _hessian(ctx, poses, slices, W):
    """the pass, with k_big_blockdiag's output held to the returned H bit for bit"""
    H, g, r, bd = ctx.debug_big_hessian(poses, slices)
    k = np.arange(6)
    want = H.reshape(W, 6, W, 6)[:, k, :, k].transpose(1, 2, 0)           # [W][W][6]: H(6 i + k, 6 j + k)
    assert np.array_equal(bd, want)
    return H, g, r


class Worst:
    """largest ratio to its bar per (class, quantity), and the failures"""

    def __init__(self, site):
        self.site, self.w, self.bad = site, {}, []

    def add(self, cls, q, what=None):
        for k, v in q.items():
            self.w[(cls, k)] = max(self.w.get((cls, k), 0.0), v)
        if max(q.values()) > 1.0:
            self.bad.append((cls, what, q))

    def done(self):
        print("\n%s worst ratio to bar: %s" % (self.site, {"%s/%s" % k: "%.3g" % v for k, v in sorted(self.w.items()) if k[1] != "zero"}))
        assert not self.bad, (self.site, len(self.bad), self.bad[:4])


# ------------------------------------------------------------------------------------------------ Hessian pass
@pytest.mark.parametrize("kind", SLICES)
@pytest.mark.parametrize("W", WS)
def test_hessian_pass(ctx, W, kind):
    st = B.store(W)
    ref = B.ref_of(st, ("store", W))
    V = len(st["cls"])
    rep = Worst("big Hessian W=%d slices=%s" % (W, kind))
    _load(ctx, st)
    assert ctx.debug_big_size() == (W, V, int((st["clusters"][:, :, 9] != 0).sum()))
    rep.add("all", ref.check(*_hessian(ctx, st["poses"], _slices(kind, V), W), np.arange(V), sym=False))
    for cls in B.CLASSES:
        idx = np.flatnonzero(st["cls"] == cls)
        _load(ctx, st, idx)
        rep.add(cls, ref.check(*_hessian(ctx, st["poses"], _slices(kind, len(idx)), W), idx, sym=False), cls)
    rep.done()


@pytest.mark.parametrize("kind", SLICES)
@pytest.mark.parametrize("W", WS)
def test_hessian_pass_at_the_origin(ctx, W, kind):
    st = B.origin(W)
    ref = B.ref_of(st, ("origin", W))
    V = len(st["cls"])
    rep = Worst("big Hessian origin W=%d slices=%s" % (W, kind))
    _load(ctx, st)
    rep.add("all", ref.check(*_hessian(ctx, st["poses"], _slices(kind, V), W), np.arange(V), sym=False))
    for v in range(V):                                                  # every voxel alone: V = 1, E <= W
        _load(ctx, st, [v])
        assert ctx.debug_big_size()[1] == 1
        rep.add(st["cls"][v], ref.check(*_hessian(ctx, st["poses"], _slices(kind, 1), W), [v], sym=False), v)
    rep.done()


# ------------------------------------------------------------------------------------------------ residual pass
def _check_eigen(rep, cls, pa, w, U):
    ref, m2 = E3.ref_from_sums(pa)
    rep.add(cls, {"eig_" + k: v for k, v in E3.check(ref, w, U, scale=m2).items()}, (pa[9], ref.w.tolist()))


@pytest.mark.parametrize("W", WS)
def test_residual_pass(ctx, W):
    st = B.store(W)
    V = len(st["cls"])
    vptr, efr, ecl = B.to_csr(st["clusters"])
    stale = np.zeros((V, 10)); stale[:, 9] = st["pcr_add"][:, 9]
    ctx.debug_big_load(W, vptr, efr, ecl, np.zeros((V, 3)), np.tile(np.eye(3).ravel(), (V, 1)), stale)
    rep = Worst("big residual W=%d" % W)
    for name in ("poses", "true_poses"):
        X = st[name]
        r = ctx.debug_big_residual(X)
        rb = ctx.debug_big_read()
        assert np.array_equal(rb["vptr"], vptr) and np.array_equal(rb["efr"], efr) and np.array_equal(rb["ecl"], ecl)
        rep.add(name, B.check_sums(vptr, efr, ecl, X, rb["pcr_add"]))
        for v in range(V):
            _check_eigen(rep, name, rb["pcr_add"][v], rb["eig_val"][v], rb["eig_vec"][v])
        rep.add(name, {"r": B.check_r(r, rb["eig_val"][:, 0])})
        # the Hessian pass an accepted step runs next reads what this pass stored
        ref = R.Ref(st["clusters"], st["coe"], rb["eig_val"], rb["eig_vec"], rb["pcr_add"], X)
        rep.add(name + "+hessian", ref.check(*_hessian(ctx, X, 0, W), np.arange(V), sym=False))
    rep.done()


# ------------------------------------------------------------------------------------------------ eigen-solver sites
IDENT = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])


def test_eig3_corpus_through_the_residual_pass(ctx):
    items = E3.corpus()
    refs = E3.refs(items)
    A6 = np.array([E3.tri(A) for _, A in items])
    V, W = len(A6), 2
    ecl = np.zeros((V, 10)); ecl[:, :6] = A6; ecl[:, 9] = 1.0
    stale = np.zeros((V, 10)); stale[:, 9] = 1.0
    ctx.debug_big_load(W, np.arange(V + 1), np.zeros(V, dtype=np.int32), ecl, np.zeros((V, 3)), np.tile(np.eye(3).ravel(), (V, 1)), stale)
    r = ctx.debug_big_residual(np.tile(IDENT, (W, 1)))
    rb = ctx.debug_big_read()
    pa = rb["pcr_add"]
    assert np.array_equal(pa[:, :6], A6) and np.all(pa[:, 6:9] == 0.0) and np.all(pa[:, 9] == 1.0)      # the kernel saw A, bit for bit
    rep = Worst("k_big_residual eig3 corpus")
    seen = {}
    for (cls, _), ref, w, U in zip(items, refs, rb["eig_val"], rb["eig_vec"]):
        key = (id(ref), w.tobytes(), U.tobytes())
        if key not in seen:
            seen[key] = E3.check(ref, w, U)
        rep.add(cls, seen[key], ref.w.tolist())
    rep.add("all", {"r": B.check_r(r, rb["eig_val"][:, 0])})
    rep.done()


def test_eig3_designed_clouds_through_the_build(capi):
    import test_gpu_eig3 as T
    W = 12
    cs = T.clouds(seed=8)
    rng = np.random.default_rng(9)
    frames = [[] for _ in range(W)]
    for _, p in cs:                                                     # every cluster seen by every keyframe
        assert len(p) >= W
        f = rng.integers(0, W, len(p))
        f[:W] = np.arange(W)
        for i in range(W):
            frames[i].append(p[f == i])
    clouds_w = [np.concatenate(fr) for fr in frames]
    o = T._map_opts(capi, 10)
    c = capi.Context(o)
    try:
        V, E = c.debug_big_build(clouds_w, np.tile(IDENT, (W, 1)), T.VOX, 0.1, [0.25] * 4)
        assert V >= 24 and E >= 2 * V
        rb = c.debug_big_read()
        rep = Worst("k_gbab_decide")
        for k in range(V):
            ref, m2 = E3.ref_from_sums(rb["pcr_add"][k])
            rep.add("factor", E3.check(ref, rb["eig_val"][k], rb["eig_vec"][k], scale=m2), (rb["pcr_add"][k, 9], ref.w.tolist()))
            assert E3.plane_judge(ref.w, 0.1, 0.25) or T._near_threshold(ref.w, 0.1, 0.25)
        rep.done()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ build parity
@pytest.mark.parametrize("params", ["gba", "local"])
@pytest.mark.parametrize("W", [3, 9, 17])
def test_build_parity(oracle, capi, W, params):
    from voxel_slam_amd import synth
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], name="room_w%d" % W, win_size=W, n_pts=2000)
    s = synth.make_scans(wl)
    clouds = [p.astype(np.float32).astype(np.float64) for p in s["points"]]           # PCL stores floats
    poses = synth.poses_flat(s["R0"], s["p0"])
    c = capi.Context(capi.options_from_workload(synth.CONFIGS["hesai200k_w10"]))     # a context built for W = 10
    try:
        o = c.opt
        local = (o.voxel_size, o.min_eigen_value, list(o.plane_eigen_value_thre))      # the set of vba_hba_add_edge's last pass
        vs, me, ea = (GBA["gba_voxel_size"], GBA["gba_min_eigen_value"], GBA["gba_eig"]) if params == "gba" else local
        f = oracle.gba_build(clouds, poses, oracle.gba_cfg13(vs, me, ea, *local, o.max_layer))
        V, E = c.debug_big_build(clouds, poses, vs, me, ea)
        assert V == f.size() and V > 20
        rb = c.debug_big_read()
        ocl, _, _ = f.read_inputs()
        oev, _, opa = f.read_back()
        # the store is consistent
        vptr, efr, evox, eidx = rb["vptr"], rb["efr"], rb["evox"], rb["eidx"]
        assert vptr[0] == 0 and vptr[-1] == E == len(efr) and np.all(np.diff(vptr) >= 2)
        assert np.array_equal(evox, np.repeat(np.arange(V), np.diff(vptr)))
        assert all(np.all(np.diff(efr[vptr[v]:vptr[v + 1]]) > 0) for v in range(V)) and efr.min() >= 0 and efr.max() < W
        want = np.full((V, W), -1, dtype=np.int32); want[evox, efr] = np.arange(E)
        assert np.array_equal(eidx, want)
        # and it is the oracle's, voxel for voxel
        pa, ev = rb["pcr_add"], rb["eig_val"]
        dcl = B.to_dense(vptr, efr, rb["ecl"], W)
        ka = np.lexsort((pa[:, 6], pa[:, 9])); kb = np.lexsort((opa[:, 6], opa[:, 9]))
        np.testing.assert_array_equal(pa[ka, 9], opa[kb, 9])
        np.testing.assert_array_equal(dcl[ka][:, :, 9], ocl[kb][:, :, 9])               # occupancy and every N: exact
        np.testing.assert_allclose(pa[ka], opa[kb], rtol=0, atol=1e-12 * np.abs(opa[:, :9]).max())
        np.testing.assert_allclose(dcl[ka], ocl[kb], rtol=0, atol=1e-12 * np.abs(ocl[:, :, :9]).max())
        np.testing.assert_allclose(ev[ka], oev[kb], rtol=0, atol=1e-11 * max(1.0, np.abs(oev).max()))
        # the Hessian pass on the built store, the reference fed the device's own store
        ref = R.Ref(dcl, np.ones(V), ev, rb["eig_vec"], pa, poses)
        rep = Worst("big Hessian on the built store W=%d %s" % (W, params))
        rep.add("all", ref.check(*_hessian(c, poses, 0, W), np.arange(V), sym=False))
        rep.done()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ empty store, refusals
def test_empty_store(ctx):
    W = 9
    z = np.zeros((0, 10))
    ctx.debug_big_load(W, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), z, z[:, :3], z[:, :9], z)
    assert ctx.debug_big_size() == (W, 0, 0)
    for k in (0, 1, 3):
        H, g, r = _hessian(ctx, B.store(W)["poses"], k, W)
        assert not H.any() and not g.any() and r == 0.0
    assert ctx.debug_big_residual(B.store(W)["poses"]) == 0.0


def test_refusals_leave_the_store(capi, ctx):
    W = 9
    st = B.store(W)
    ref = B.ref_of(st, ("store", W))
    V = len(st["cls"])
    vptr, efr, ecl = _load(ctx, st)
    ev, evec, pa = st["eig_val"], st["eig_vec"], st["pcr_add"]
    H0, g0, r0 = _hessian(ctx, st["poses"], 0, W)
    assert max(ref.check(H0, g0, r0, np.arange(V), sym=False).values()) <= 1.0

    def bad(what, W_=W, **kw):
        a = dict(vptr=vptr.copy(), efr=efr.copy(), ecl=ecl.copy(), eig_val=ev.copy(), eig_vec=evec.copy(), pcr_add=pa.copy())
        for k, fn in kw.items():
            fn(a[k])
        assert ctx.debug_big_load(W_, a["vptr"], a["efr"], a["ecl"], a["eig_val"], a["eig_vec"], a["pcr_add"], raw=True) == capi.ERR_BAD_ARG, what
        assert ctx.debug_big_size() == (W, V, len(efr)), what
        H, g, r = _hessian(ctx, st["poses"], 0, W)
        assert max(ref.check(H, g, r, np.arange(V), sym=False).values()) <= 1.0, what
        assert np.array_equal(ctx.debug_big_read()["ecl"], ecl), what

    def put(i, x):
        def fn(a):
            a.reshape(-1)[i] = x
        return fn

    two = int(np.flatnonzero(np.diff(vptr) >= 2)[0])                    # a voxel with two entries or more
    e = int(vptr[two])
    bad("W = 1", W_=1)
    bad("W = 1025", W_=1025)
    bad("W too small for efr", W_=int(efr.max()))
    bad("vptr[0] != 0", vptr=put(0, 1))
    bad("vptr decreasing", vptr=put(two + 1, vptr[two] - 1) if two > 0 else put(1, -1))
    bad("voxel without an entry", vptr=put(two + 1, vptr[two]))
    bad("efr repeated", efr=put(e + 1, efr[e]))
    bad("efr decreasing", efr=lambda a: a.__setitem__(slice(e, e + 2), a[e:e + 2][::-1].copy()))
    bad("efr = W", efr=put(int(vptr[two + 1]) - 1, W))
    bad("efr = -1", efr=put(e, -1))
    for name, n in (("ecl", ecl.size), ("eig_val", ev.size), ("eig_vec", evec.size), ("pcr_add", pa.size)):
        bad(name + " nan", **{name: put(n // 2, np.nan)})
        bad(name + " inf", **{name: put(n - 1, np.inf)})
    # NULL pointers
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    args = [pi(vptr), pi(efr), pd(ecl), pd(np.ascontiguousarray(ev)), pd(np.ascontiguousarray(evec)), pd(np.ascontiguousarray(pa))]
    for k in range(len(args)):
        a = list(args); a[k] = None
        assert ctx.lib.vba_debug_big_load(ctx.h, C.c_int(W), C.c_int(V), *a) == capi.ERR_BAD_ARG, k
    H, g, r = _hessian(ctx, st["poses"], 0, W)
    assert max(ref.check(H, g, r, np.arange(V), sym=False).values()) <= 1.0
    # the passes themselves
    nanp = st["poses"].copy(); nanp[3, 2] = np.nan
    for call in (lambda: ctx.debug_big_hessian(nanp), lambda: ctx.debug_big_residual(nanp), lambda: ctx.debug_big_hessian(st["poses"], -1)):
        with pytest.raises(capi.VbaError) as err:
            call()
        assert err.value.status == capi.ERR_BAD_ARG


def test_sharded_context_is_refused(capi):
    o = capi.default_options()
    o.win_size = 10
    c = capi.Context(o)
    try:
        c.set_shard(0, 2)
        st = B.origin(3)
        vptr, efr, ecl = B.to_csr(st["clusters"])
        assert c.debug_big_load(3, vptr, efr, ecl, st["eig_val"], st["eig_vec"], st["pcr_add"], raw=True) == capi.ERR_UNSUPPORTED
        for call in (lambda: c.debug_big_size(), lambda: c.debug_big_read(), lambda: c.debug_big_hessian(st["poses"]),
                     lambda: c.debug_big_residual(st["poses"])):
            with pytest.raises(capi.VbaError) as err:
                call()
            assert err.value.status == capi.ERR_UNSUPPORTED
    finally:
        c.close()
