"""Edge shapes of the dense-tile Hessian pass k_hessian2<W>: the per-wave unit table (csrc/vba_hess_units.hpp) and the epilogue that sums
the E / gradient / residual terms of aligned 8-column groups out of LDS.  Against the double-double reference and the bars of
tests/hess_ref.py, as tests/test_gpu_hess.py (same corpus, same cached reference), through the C ABI.
  * W = 2, 3, 6, 10, 11, 16: every distinct (NU, KS, UPW) of the unit table (tests/test_hess_units_cpu.py asserts that these are all), the
    one window without the prescaled image (W = 3), and W = 16, whose epilogue staging outgrows the main LDS image;
  * V = 1, 7, 8, 9, TV - 1, TV, TV + 1 voxels (the first V of the corpus): partly filled 8-lane groups, one full group, a group and one
    voxel, a tile short of one voxel, a whole tile, and a second tile that holds one voxel — as a workgroup of its own and, with
    hessian_workgroups = 1, as the second trip of one workgroup's tile loop (also run over the whole store: four tiles);
  * a store in which one frame has no slot at all (the voxels of the corpus that frame does not see): its rows of H and g are exact zeros.
Every launch is made twice on the same store and must give the same bits."""
import numpy as np
import pytest

import hess_ref as R

pytestmark = pytest.mark.gpu

WS = [2, 3, 6, 10, 11, 16]


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


def _twice(ctx, poses, a, b):
    H, g, r = ctx.acc_evaluate2(poses, a, b)
    H2, g2, r2 = ctx.acc_evaluate2(poses, a, b)
    assert np.array_equal(H, H2) and np.array_equal(g, g2) and np.array_equal(np.float64(r), np.float64(r2)), (a, b)
    return H, g, r


def _check(ref, H, g, r, idx, what):
    q = ref.check(H, g, r, idx)
    print("%s ratio to bar: %s" % (what, {k: "%.3g" % v for k, v in sorted(q.items())}))
    assert R.worst(q) <= 1.0, (what, q)


@pytest.mark.parametrize("W", WS)
def test_small_stores(capi, W):
    st = R.store(W)
    ref = R.ref_of(st, ("corpus", W))
    V, TV = len(st["coe"]), st["TV"]
    for wg, sizes in ((0, (1, 7, 8, 9, TV - 1, TV, TV + 1)), (1, (TV + 1, V))):
        ctx = _ctx(capi, W, V, hessian_workgroups=wg)
        try:
            _push(ctx, st)
            for n in sizes:
                H, g, r = _twice(ctx, st["poses"], 0, n)
                _check(ref, H, g, r, np.arange(n), "W=%d workgroups=%s V=%d" % (W, wg or "default", n))
        finally:
            ctx.close()


@pytest.mark.parametrize("W", WS)
def test_a_frame_without_slots(capi, W):
    st = R.store(W)
    ref = R.ref_of(st, ("corpus", W))
    fr = W - 1
    idx = np.flatnonzero(st["clusters"][:, fr, 9] == 0.0)
    assert 8 < len(idx) < len(st["coe"])
    ctx = _ctx(capi, W, len(idx))
    try:
        _push(ctx, R.reorder(st, idx))
        H, g, r = _twice(ctx, st["poses"], 0, len(idx))
    finally:
        ctx.close()
    _check(ref, H, g, r, idx, "W=%d without frame %d" % (W, fr))
    rows = slice(6 * fr, 6 * fr + 6)
    assert not H[rows, :].any() and not H[:, rows].any() and not g[rows].any()
