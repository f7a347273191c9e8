"""The Hessian / gradient pass on the device (k_hessian2<W>, k_hessian3<W>, slot_terms, tl_fetch, k_reduce_partials) against the
double-double reference and the per-entry bars of tests/hess_ref.py, through the C ABI.  The stored eigen-data is pushed with the voxels
(vba_factor_push_voxels), so device and reference read the same doubles.
  * k_hessian2, every W in 2..16, three launch shapes (hessian_workgroups default = one tile per workgroup, 2 = two tiles per workgroup:
    the loop that prefetches tile n + 1 under the contraction of tile n, 3 = an uneven split), each on the whole store, [3, V - 2),
    [TV - 1, TV + 1) and [TV, 2 TV);
  * the same kernel on each class of the corpus as a store of its own (the table per W, class and quantity), and on the store at the
    origin (planes and near-gap rods), where the bars are tightest: every voxel alone and the whole store;
  * k_hessian3 (hessian_compact_tiles), W in 2..10, the corpus with a run of 100 equal-mask voxels in popcount order and shuffled;
  * the LM loop, W = 3, 10, 16: the hess of lidar_ba_damping_iter(max_iter = 1), and the Hessian pass of a second iteration, which
    carries the accept / reject bookkeeping in its prologue (lm != nullptr) and runs on the trial poses of an accepted step.
Every case asserts H, g, r within the bars, H equal to its transpose bit for bit and exact zeros where no voxel contributes; the printed
ratios are reports, nothing depends on them."""
import itertools

import numpy as np
import pytest

import hess_ref as R

pytestmark = pytest.mark.gpu

WS = list(range(2, 17))


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


def _ctx(capi, W, V, **kw):
    o = capi.default_options()
    o.win_size = W
    o.max_voxels = max(int(o.max_voxels), V)
    for k, v in kw.items():
        setattr(o, k, v)
    return capi.Context(o)


def _push(ctx, st):
    ctx.push_voxels(st["clusters"], st["fix"], st["coe"], st["eig_val"], st["eig_vec"], st["pcr_add"])


class Worst:
    """largest ratio to its bar per (class, quantity), and the failures"""

    def __init__(self, site):
        self.site, self.w, self.bad = site, {}, []

    def add(self, cls, q, what=None):
        for k, v in q.items():
            self.w[(cls, k)] = max(self.w.get((cls, k), 0.0), v)
        if R.worst(q) > 1.0:
            self.bad.append((cls, what, q))

    def done(self):
        print("\n%s worst ratio to bar: %s" % (self.site, {"%s/%s" % k: "%.3g" % v for k, v in sorted(self.w.items()) if k[1] in "Hgr"}))
        assert not self.bad, (self.site, len(self.bad), self.bad[:4])


# ------------------------------------------------------------------------------------------------ k_hessian2
@pytest.mark.parametrize("wg", [0, 2, 3])
@pytest.mark.parametrize("W", WS)
def test_hessian2_ranges(capi, W, wg):
    st = R.store(W)
    ref = R.ref_of(st, ("corpus", W))
    V = len(st["coe"])
    ctx = _ctx(capi, W, V, hessian_workgroups=wg)
    rep = Worst("k_hessian2 W=%d workgroups=%s" % (W, wg or "default"))
    try:
        _push(ctx, st)
        for a, b in R.ranges(st):
            H, g, r = ctx.acc_evaluate2(st["poses"], a, b)
            rep.add("[%d,%d)" % (a, b), ref.check(H, g, r, np.arange(a, b)), (a, b))
    finally:
        ctx.close()
    rep.done()


@pytest.mark.parametrize("W", WS)
def test_hessian2_per_class(capi, W):
    st = R.store(W)
    ref = R.ref_of(st, ("corpus", W))
    ctx = _ctx(capi, W, len(st["coe"]))
    rep = Worst("k_hessian2 W=%d per class" % W)
    try:
        for cls in R.CLASSES:
            idx = np.flatnonzero(st["cls"] == cls)
            ctx.clear()
            _push(ctx, R.reorder(st, idx))
            H, g, r = ctx.acc_evaluate2(st["poses"])
            rep.add(cls, ref.check(H, g, r, idx), cls)
    finally:
        ctx.close()
    rep.done()


@pytest.mark.parametrize("W", WS)
def test_hessian2_at_the_origin(capi, W):
    st = R.origin_store(W)
    ref = R.ref_of(st, ("origin", W))
    V = len(st["coe"])
    ctx = _ctx(capi, W, V)
    rep = Worst("k_hessian2 W=%d origin" % W)
    try:
        _push(ctx, st)
        for a, b in [(v, v + 1) for v in range(V)] + [(0, V)]:
            H, g, r = ctx.acc_evaluate2(st["poses"], a, b)
            rep.add(st["cls"][a] if b - a == 1 else "all", ref.check(H, g, r, np.arange(a, b)), (a, b))
    finally:
        ctx.close()
    rep.done()


# ------------------------------------------------------------------------------------------------ k_hessian3
@pytest.mark.parametrize("order", ["popcount", "shuffled"])
@pytest.mark.parametrize("W", list(range(2, 11)))
def test_hessian3(capi, W, order):
    """popcount order: k_factor_tiles sees several classes, and the run of 100 voxels of one mask (frame 0) is cut at H3_MAXNV = 96 while
    the full-mask voxels are cut by nv * p <= 256; shuffled: one class whose union is all W frames"""
    base = R.store(W, extra_run=100)
    ref = R.ref_of(base, ("h3", W))
    perm = R.order_popcount(base) if order == "popcount" else R.order_shuffled(base)
    st = R.reorder(base, perm)
    V = len(st["coe"])
    if order == "popcount":
        m = R.occupancy_masks(st)
        run = max(len(list(g)) for _, g in itertools.groupby(m.tolist()))
        assert run > 96
    ctx = _ctx(capi, W, V, hessian_compact_tiles=1)
    rep = Worst("k_hessian3 W=%d %s" % (W, order))
    try:
        _push(ctx, st)
        H, g, r = ctx.acc_evaluate2(st["poses"])
        rep.add("all", ref.check(H, g, r, np.arange(V)), order)          # (the sum over all voxels does not depend on their order)
    finally:
        ctx.close()
    rep.done()


# ------------------------------------------------------------------------------------------------ the LM loop
def _lm_part(st):
    return np.flatnonzero(np.isin(st["cls"], ("plane", "fixed")))


@pytest.mark.parametrize("W", [3, 10, 16])
def test_lm_first_hessian(capi, W):
    """hess of lidar_ba_damping_iter(max_iter = 1) on the plane + fixed part of the corpus: formed at the poses passed in, from the
    pushed eigen-data, by the gated launch of the LM loop"""
    st = R.store(W)
    ref = R.ref_of(st, ("corpus", W))
    idx = _lm_part(st)
    ctx = _ctx(capi, W, len(idx))
    rep = Worst("LM first Hessian W=%d" % W)
    try:
        _push(ctx, R.reorder(st, idx))
        out = ctx.lidar_ba_damping_iter(st["poses"], max_iter=1, thd_num=2)
        assert out["status"] == 0
        H = out["hess"]
        (Hs, _, _), (barH, _, _) = ref.sums(idx)
        err = Hs.err_to(H)
        z = barH == 0.0
        assert not H[z].any() and np.array_equal(H, H.T)
        rep.add("plane+fixed", {"H": float((err[~z] / barH[~z]).max())})
    finally:
        ctx.close()
    rep.done()


@pytest.mark.parametrize("W", [3, 10, 16])
def test_lm_second_hessian_rides_the_update(capi, W):
    """The Hessian pass of the second iteration carries the accept / reject bookkeeping of the first in its prologue (lm != nullptr),
    reads the trial poses and the eigen-data the residual pass stored at them.  From the generating poses the first step is accepted
    (asserted).  One run learns the accepted poses; a second, identical run reads the eigen-data back between the two iterations."""
    st = R.store(W)
    idx = _lm_part(st)
    sub = R.reorder(st, idx)
    x0 = st["true_poses"]
    sub["eig_val"], sub["eig_vec"], sub["pcr_add"] = R.host_eigen(sub["clusters"], sub["fix"], x0)
    ctx = _ctx(capi, W, len(idx))
    rep = Worst("LM second Hessian W=%d" % W)
    try:
        _push(ctx, sub)
        ctx.lm_begin(x0, thd_num=2)
        ctx.lm_iterate(sync=False)
        x1, H1, _ = ctx.lm_end()
        assert np.abs(x1 - x0).max() > 0.0                              # accepted
        ctx.clear()
        _push(ctx, sub)
        ctx.lm_begin(x0, thd_num=2)
        ctx.lm_iterate(sync=False)
        ev, evec, pa = ctx.read_back()                                  # what the residual pass stored at the trial poses
        ctx.lm_iterate(sync=False)
        _, H2, _ = ctx.lm_end()
        assert not np.array_equal(H2, H1)                               # the second pass ran
        ref = R.Ref(sub["clusters"], sub["coe"], ev, evec, pa, x1)
        (Hs, _, _), (barH, _, _) = ref.sums(np.arange(len(idx)))
        err = Hs.err_to(H2)
        z = barH == 0.0
        assert not H2[z].any() and np.array_equal(H2, H2.T)
        rep.add("plane+fixed", {"H": float((err[~z] / barH[~z]).max())})
    finally:
        ctx.close()
    rep.done()
