"""The LM state of a lidar LM call is written by the first kernel the call launches (vba_lm_begin copies nothing), and a fetching
vba_lm_end is one launch (k_lm_finish).  Three sequences on stores pushed from synth.root_factors must agree bit for bit:
  R   lm_begin -> timing_launch_hessian -> [refresh] -> lm_iterate x k -> lm_end(fetch)   (not a fused site: the stand-alone init kernel)
  F1  lm_begin -> lm_iterate x k -> lm_end(fetch)                                          (init carried by the first Hessian pass)
  F2  lm_begin -> lm_refresh_eigen -> lm_iterate x k -> lm_end(fetch)                      (init carried by the refresh pass)
over the window sizes (W = 2, 4, 10 and 16: the smallest and the largest init argument, the bench's, and k_hessian2 beyond W = 10), a
3-voxel store (almost every Hessian workgroup owns no tile, workgroup 0 must still write the image) and the option fields that
change which kernel runs first."""
import dataclasses
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 5
KEYS = ("trace", "poses", "hess", "resis")


@pytest.fixture(scope="module")
def mods():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    return capi, synth


def _workload(synth, name):
    room, hesai = synth.CONFIGS["room20k_w4"], synth.CONFIGS["hesai200k_w10"]
    return {"w2": dataclasses.replace(room, win_size=2, n_pts=4000),
            "w4": dataclasses.replace(room, n_pts=4000),
            "w10": dataclasses.replace(hesai, n_pts=40000),
            "w16": dataclasses.replace(room, win_size=16, n_pts=8000)}[name]


_CACHE = {}


@pytest.fixture(scope="module")
def data(mods):
    """name -> (workload, factors, begin poses); computed once per name and never modified"""
    capi, synth = mods

    def get(name):
        if name not in _CACHE:
            wl = _workload(synth, name)
            s = synth.make_scans(wl)
            fac = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
            assert len(fac["coe"]) >= 20, (name, len(fac["coe"]))
            _CACHE[name] = (wl, fac, synth.poses_flat(s["R0"], s["p0"]))
        return _CACHE[name]
    return get


def _ctx(capi, wl, fac, **opts):
    o = capi.options_from_workload(wl)
    for k, v in opts.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    ctx = capi.Context(o)
    if opts.get("force_collective"):
        ctx.set_allreduce(lambda ptr, n, stream: 0)     # one rank: the sum over the ranks is the buffer itself
    ctx.push_dict(fac)
    return ctx


def _fetch(ctx):
    p, h, r = ctx.lm_end(fetch=True)
    return dict(poses=p, hess=h, resis=r, trace=ctx.last_trace())


def _seq(capi, wl, fac, poses, kind, refresh=False, iters=ITERS, sync=False, **opts):
    ctx = _ctx(capi, wl, fac, **opts)
    ctx.lm_begin(poses, thd_num=2)
    if kind == "R":
        ctx.timing_launch_hessian()
    if refresh:
        ctx.lm_refresh_eigen()
    for _ in range(iters):
        ctx.lm_iterate(sync=sync)
    out = _fetch(ctx)
    ctx.close()
    return out


def _same(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max())


def _check_fused(capi, wl, fac, poses, min_trace=2, **opts):
    r0 = _seq(capi, wl, fac, poses, "R", refresh=False, **opts)
    r1 = _seq(capi, wl, fac, poses, "R", refresh=True, **opts)
    assert len(r0["trace"]) >= min_trace and len(r1["trace"]) >= min_trace
    assert np.isfinite(r0["poses"]).all() and np.isfinite(r0["hess"]).all()
    for r in (r0, r1):      # the image itself, not only its agreement between the sequences: the first step ran at u = 0.01, v = 2 (VM:427)
        assert r["trace"][0, 2] == 0.01 and r["trace"][0, 3] == 2.0, r["trace"][0]
    _same(_seq(capi, wl, fac, poses, "F", refresh=False, **opts), r0, "F1")
    _same(_seq(capi, wl, fac, poses, "F", refresh=True, **opts), r1, "F2")
    return r0, r1


@pytest.mark.parametrize("name", ["w2", "w4", "w10", "w16"])
def test_fused_init_equals_standalone_init(mods, data, name):
    capi, _ = mods
    wl, fac, poses = data(name)
    r0, _r1 = _check_fused(capi, wl, fac, poses)
    # the one-call form runs F1
    ctx = _ctx(capi, wl, fac)
    a = ctx.lidar_ba_damping_iter(poses, max_iter=ITERS, thd_num=2)
    ctx.close()
    _same(a, r0, "lidar_ba_damping_iter")
    # sync=True: the stand-alone accept/reject kernel after every step; sync=False: it rides in the next Hessian pass and the
    # finish kernel applies the last one
    _same(_seq(capi, wl, fac, poses, "F", sync=True), r0, "sync")


def test_three_voxel_store(mods, data):
    capi, _ = mods
    wl, fac, poses = data("w4")
    tiny = {k: np.ascontiguousarray(v[:3]) for k, v in fac.items()}
    _check_fused(capi, wl, tiny, poses, min_trace=1)
    _check_fused(capi, wl, tiny, poses, min_trace=1, residual_vpl_from=1)    # k_residual_v: its only workgroup is a partial one


@pytest.mark.parametrize("name,opts", [
    ("w4", dict(residual_vpl_from=1)), ("w10", dict(residual_vpl_from=1)),           # the refresh is k_residual_v
    ("w4", dict(hessian_compact_tiles=1)), ("w10", dict(hessian_compact_tiles=1)),   # k_hessian3: the stand-alone init in front of it
    ("w4", dict(lm_spec=1)), ("w4", dict(lm_spec=4)),
    ("w4", dict(force_collective=1)),                                                # the multi-rank flow with one rank
])
def test_option_fields(mods, data, name, opts):
    capi, _ = mods
    wl, fac, poses = data(name)
    _check_fused(capi, wl, fac, poses, **opts)


@pytest.mark.parametrize("name", ["w4", "w10"])
def test_bench_pattern_leaks_nothing_between_calls(mods, data, name):
    capi, _ = mods
    wl, fac, poses = data(name)

    def call(ctx, fetch):
        ctx.lm_begin(poses, thd_num=2)
        ctx.lm_refresh_eigen()
        for _ in range(3):
            ctx.lm_iterate(sync=False)
        return _fetch(ctx) if fetch else ctx.lm_end(fetch=False)

    fresh = _ctx(capi, wl, fac)
    ref = call(fresh, True)
    fresh.close()
    assert len(ref["trace"]) >= 2
    ctx = _ctx(capi, wl, fac)
    for _ in range(3):
        call(ctx, False)
    _same(call(ctx, True), ref, "after three unfetched calls")
    _same(call(ctx, True), ref, "after a fetched call")
    ctx.close()


def test_end_right_after_begin(mods, data):
    capi, _ = mods
    wl, fac, poses = data("w4")
    ctx = _ctx(capi, wl, fac)
    ctx.lm_begin(poses, thd_num=2)
    out = _fetch(ctx)
    assert np.array_equal(out["poses"], poses) and out["trace"].shape == (0, 5)
    # a second begin replaces a pending init; an unfetched end drops it
    other = poses.copy(); other[1:, 9:] += 0.125
    ctx.lm_begin(other, thd_num=2)
    ctx.lm_begin(poses, thd_num=2)
    out = _fetch(ctx)
    assert np.array_equal(out["poses"], poses) and out["trace"].shape == (0, 5)
    ctx.lm_begin(other, thd_num=2)
    ctx.lm_end(fetch=False)
    ref = _seq(capi, wl, fac, poses, "R")
    ctx.lm_begin(poses, thd_num=2)
    for _ in range(ITERS):
        ctx.lm_iterate(sync=False)
    _same(_fetch(ctx), ref, "after a dropped init")
    ctx.close()


def test_too_few_voxels_leaves_nothing_pending(mods, data):
    capi, _ = mods
    wl, fac, poses = data("w4")
    ctx = _ctx(capi, wl, fac)
    other = poses.copy(); other[1:, 9:] += 0.125
    a = ctx.lidar_ba_damping_iter(other, max_iter=ITERS, thd_num=len(fac["coe"]) + 1)
    assert a["status"] == -1
    ctx.lm_begin(poses, thd_num=2)
    out = _fetch(ctx)                                   # the stand-alone init of THIS call, not the refused call's poses
    assert np.array_equal(out["poses"], poses)
    b = ctx.lidar_ba_damping_iter(poses, max_iter=ITERS, thd_num=2)
    ctx.close()
    _same(b, _seq(capi, wl, fac, poses, "R"), "after TOO_FEW_VOXELS")
