"""The fused trial launch of the lidar LM iteration (k_lm_trial: the residual workgroups ride in the solve's launch and take the
trial poses through an in-launch hand-off) against the two-launch form k_lm_solve_m + k_residual_s it replaces
(vba_options::lm_trial_launches = 0 / 2).  Nothing in the arithmetic or in the order of a sum differs, so everything a call returns
and everything it leaves in the factor store must be equal to the bit.

Stores are pushed with push_dict in a fixed voxel order and the begin poses are those of test_gpu_lm_trips.py (whose data this module
shares), whose traces hold an accepted step, a rejection served by a damping candidate (the riders take xt as launched, no wait), a
rejection after the candidates ran out (the riders wait for the hand-off) and a stop (every workgroup returns).  That each of the four
occurred where the fused kernel runs is asserted from the device's own trace.  W = 16 keeps the two launches under either value of the
option: there the switch must be inert."""
import numpy as np
import pytest

import test_gpu_lm_trips as trips

pytestmark = pytest.mark.gpu

KEYS = ("poses", "hess", "resis", "trace", "eig_values", "eig_vectors", "pcr_adds")
FUSED_W = range(2, 11)          # windows whose k_lm_trial instance is launched (LmTrialFits, voxelba.hip)
ITERS = 8

mods = trips.mods
data = trips.data


def _stores(tiny, small):
    """3 voxels: one rider, partly filled; 33: two riders, the second with one voxel; ~200"""
    return {"3": tiny, "33": {k: np.ascontiguousarray(v[:33]) for k, v in small.items()}, "200": small}


def _state(ctx, out):
    ev, evec, pcr = ctx.read_back()
    out.update(eig_values=ev, eig_vectors=evec, pcr_adds=pcr)
    # the fault word of the LM state: every fetching call tests it, fails if it is set, and names the kernel in the context's error text
    assert b"k_lm_trial" not in ctx.lib.vba_last_error(ctx.h)
    return out


def _one_call(ctx, begin):
    r = ctx.lidar_ba_damping_iter(begin, max_iter=ITERS, thd_num=2)
    return _state(ctx, dict(poses=r["poses"], hess=r["hess"], resis=r["resis"], trace=r["trace"]))


def _bench_call(ctx, begin, refresh):
    ctx.lm_begin(begin, thd_num=2)
    if refresh:
        ctx.lm_refresh_eigen()
    for _ in range(ITERS):
        ctx.lm_iterate(sync=False)
    return _state(ctx, trips._fetch(ctx))


def _same(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max())


def _sequence(capi, wl, fac, begin, **opts):
    """three calls on one context, each with what it returns and the store's eigen state behind it: the enqueued pattern on the store as
    pushed (the construction of test_gpu_lm_trips.py), the one-call form on what that left, the bench's pattern (refresh first)"""
    ctx = trips._ctx(capi, wl, fac, **opts)
    out = [_bench_call(ctx, begin, refresh=False), _one_call(ctx, begin), _bench_call(ctx, begin, refresh=True)]
    ctx.close()
    return out


@pytest.mark.parametrize("lm_spec", [1, 4])
@pytest.mark.parametrize("name", trips.NAMES)
def test_fused_trial_equals_two_launches(mods, data, name, lm_spec):
    capi, _ = mods
    wl, tiny, small, poses, gt = data(name)
    got = set()
    for sname, fac in _stores(tiny, small).items():
        for bname, begin in (("poses", poses), ("gt", gt)):
            fused = _sequence(capi, wl, fac, begin, lm_spec=lm_spec, lm_trial_launches=0)
            two = _sequence(capi, wl, fac, begin, lm_spec=lm_spec, lm_trial_launches=2)
            for i, (a, b) in enumerate(zip(fused, two)):
                assert 1 <= len(a["trace"]) <= ITERS
                _same(a, b, (name, lm_spec, sname, bname, i))
                got |= trips._cases(a["trace"], lm_spec)
    print(name, lm_spec, sorted(got))
    if wl.win_size in FUSED_W:                            # every path of the riders was taken where they exist
        want = {"accepted", "rejected, no candidate", "stop"} | ({"rejected, candidate"} if lm_spec > 1 else set())
        assert got >= want, (name, lm_spec, sorted(want - got))


@pytest.mark.parametrize("name", trips.NAMES)
def test_fused_trial_repeated_calls(mods, data, name):
    """one call pattern 50 times over on the ~200-voxel store: a call opens on whatever xt_seq the call before left, and every call must
    return what the first did, which is what the two-launch form returns"""
    capi, _ = mods
    wl, _tiny, small, poses, _gt = data(name)
    ctx = trips._ctx(capi, wl, small, lm_trial_launches=2)
    ref = _bench_call(ctx, poses, refresh=True)
    ctx.close()
    ctx = trips._ctx(capi, wl, small, lm_trial_launches=0)
    for i in range(50):
        _same(_bench_call(ctx, poses, refresh=True), ref, (name, i))
    ctx.close()


@pytest.mark.parametrize("name", trips.NAMES)
def test_fused_trial_is_what_runs(mods, data, name):
    """the timing spans tell which form a context enqueues: a fused launch is bracketed as "solve" and leaves no "residual" span"""
    capi, _ = mods
    wl, _tiny, small, poses, _gt = data(name)
    for launches in (0, 2):
        ctx = trips._ctx(capi, wl, small, lm_trial_launches=launches)
        ctx.timing_enable(True)
        ctx.lm_begin(poses, thd_num=2)
        for _ in range(3):
            ctx.lm_iterate(sync=False)
        trips._fetch(ctx)
        fused = launches == 0 and wl.win_size in FUSED_W
        assert ctx.timing_get("solve")[1] == 3 and ctx.timing_get("residual")[1] == (0 if fused else 3), (name, launches)
        ctx.close()
