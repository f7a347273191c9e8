"""The lidar LM call keeps its results bit for bit while two of its serial memory trips are gone:
  * the LmDev image of a call whose first kernel carries the init is written from the poses that kernel already holds in LDS
    (lm_init_store_lds: k_residual_s, k_hessian2) and must equal the image of the stand-alone k_lm_init;
  * the accept/reject bookkeeping requests everything a decision can need in one batch (all damping candidates, selected after
    spec_i has arrived), in k_lm_update, in k_lm_finish and in the prologue of the Hessian pass, and must decide and store as before.
Stores are pushed with push_dict in a fixed voxel order (synth.root_factors), so every sequence sees the same bytes.  The slices and
begin poses of the accept/reject test were chosen on the CPU oracle's trace; the cases they are meant to produce are asserted from the
device's own trace."""
import dataclasses
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("trace", "poses", "hess", "resis")
NAMES = ("w2", "w4", "w10", "w16")
# about 200 voxels of each store: the slice whose LM trace holds the cases test_accept_reject_one_trip asserts
SLICE = {"w2": slice(200, 400), "w4": slice(0, 200), "w10": slice(5000, 5150), "w16": slice(0, 200)}


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
    """name -> (workload, 3-voxel store, ~200-voxel store, begin poses, ground-truth poses); computed once, never modified"""
    _, synth = mods

    def get(name):
        if name not in _CACHE:
            wl = _workload(synth, name)
            s = synth.make_scans(wl)
            fac = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
            sl = SLICE[name]
            assert len(fac["coe"]) >= sl.stop, (name, len(fac["coe"]))
            tiny = {k: np.ascontiguousarray(v[:3]) for k, v in fac.items()}
            small = {k: np.ascontiguousarray(v[sl]) for k, v in fac.items()}
            _CACHE[name] = (wl, tiny, small, synth.poses_flat(s["R0"], s["p0"]), synth.poses_flat(s["R_gt"], s["p_gt"]))
        return _CACHE[name]
    return get


def _ctx(capi, wl, fac, **opts):
    o = capi.options_from_workload(wl)
    for k, v in opts.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    ctx = capi.Context(o)
    ctx.push_dict(fac)
    return ctx


def _fetch(ctx):
    p, h, r = ctx.lm_end(fetch=True)
    return dict(poses=p, hess=h, resis=r, trace=ctx.last_trace())


def _same(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max())


def _call(ctx, poses, first, iters=3, standalone=False):
    """one LM call; first = "K4": the refresh pass is the first kernel, "K3": the first Hessian pass is.  standalone: a Hessian launch
    that is not a fused site goes in front, so the image comes from k_lm_init and no pass carries it."""
    ctx.lm_begin(poses, thd_num=2)
    if standalone:
        ctx.timing_launch_hessian()
    if first == "K4":
        ctx.lm_refresh_eigen()
    for _ in range(iters):
        ctx.lm_iterate(sync=False)
    return _fetch(ctx)


# residual_vpl_from = 1: every store of more than one voxel takes k_residual_v, whose INIT instance then carries the image from its
# argument (it has no LDS).  (The option's 0 means "the library's default", 45 000 voxels: it would select k_residual_s again.)
@pytest.mark.parametrize("opts", [dict(), dict(residual_vpl_from=1)], ids=["k_residual_s", "k_residual_v"])
@pytest.mark.parametrize("store", ["tiny", "small"])
@pytest.mark.parametrize("name", NAMES)
def test_fused_init_equals_standalone_init(mods, data, name, store, opts):
    capi, _ = mods
    wl, tiny, small, poses, gt = data(name)
    fac = tiny if store == "tiny" else small
    other = poses.copy(); other[1:, 9:] += 0.125
    for first in ("K4", "K3"):
        # (a residual pass leaves the store's eigen state at its trial poses and only the refresh pass puts it back, so a call
        #  that opens with the Hessian pass runs on a context of its own)
        ctx = _ctx(capi, wl, fac, **opts)
        ref = _call(ctx, poses, first, standalone=True)
        ctx.close()
        assert len(ref["trace"]) >= 1 and ref["trace"][0, 2] == 0.01 and ref["trace"][0, 3] == 2.0, ref["trace"][:1]
        assert np.isfinite(ref["poses"]).all() and np.isfinite(ref["hess"]).all()
        ctx = _ctx(capi, wl, fac, **opts)
        if first == "K4":
            _call(ctx, other, first)                    # a whole call on other poses: its state is what the next image overwrites
        # the stand-alone image itself: vba_lm_end right after vba_lm_begin launches k_lm_init and fetches what it wrote
        ctx.lm_begin(other, thd_num=2)
        img = _fetch(ctx)
        assert np.array_equal(img["poses"], other) and img["trace"].shape == (0, 5)
        # a second begin, now carried by the call's first kernel, over the image of the other poses
        _same(_call(ctx, poses, first), ref, (name, store, first))
        if first == "K4":
            _same(_call(ctx, poses, first), ref, (name, store, first, "again"))
        ctx.close()


def _cases(trace, lm_spec):
    """which accept/reject cases the rows [r1, r2, u, v, q1] of a trace hold.  A damping candidate serves the k-th rejection in a
    row (counted from the last solve that ran) while k < lm_spec; the rejection after that finds none and a fresh solve follows."""
    got, k = set(), 0
    for r1, r2 in trace[:, :2]:
        if r1 - r2 > 0:
            got.add("accepted"); k = 0
        else:
            k += 1
            if k < lm_spec:
                got.add("rejected, candidate")
            else:
                got.add("rejected, no candidate"); k = 0
        if abs((r1 - r2) / r1) < 1e-6:
            got.add("stop")
    return got


@pytest.mark.parametrize("lm_spec", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_accept_reject_one_trip(mods, data, name, lm_spec):
    capi, _ = mods
    wl, _tiny, small, poses, gt = data(name)
    got = set()
    for begin in (poses, gt):
        # (a context per sequence: no refresh pass opens these calls, so each needs the store's eigen state as pushed)
        # the bookkeeping rides in the next Hessian pass and, for the last step, in k_lm_finish
        ctx = _ctx(capi, wl, small, lm_spec=lm_spec)
        ctx.lm_begin(begin, thd_num=2)
        for _ in range(8):
            ctx.lm_iterate(sync=False)
        a = _fetch(ctx)
        ctx.close()
        # the flags asked for after every iteration: the stand-alone k_lm_update
        ctx = _ctx(capi, wl, small, lm_spec=lm_spec)
        ctx.lm_begin(begin, thd_num=2)
        flags = [ctx.lm_iterate(sync=True) for _ in range(8)]
        b = _fetch(ctx)
        ctx.close()
        _same(a, b, (name, lm_spec))
        tr = a["trace"]
        assert 1 <= len(tr) <= 8
        print(name, lm_spec, "".join("A" if r1 - r2 > 0 else "R" for r1, r2 in tr[:, :2]), sorted(_cases(tr, lm_spec)))
        # the flags the host saw are the trace's decisions; after a stop nothing more is recorded
        for (acc, stop), (r1, r2) in zip(flags, tr[:, :2]):
            assert acc == (r1 - r2 > 0)
        stopped = abs((tr[-1, 0] - tr[-1, 1]) / tr[-1, 0]) < 1e-6
        assert flags[-1][1] == stopped and (stopped or len(tr) == 8)
        got |= _cases(tr, lm_spec)
    want = {"accepted", "rejected, no candidate", "stop"} | ({"rejected, candidate"} if lm_spec > 1 else set())
    assert got >= want, (name, lm_spec, sorted(want - got))
