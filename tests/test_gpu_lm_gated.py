"""Gated launches of the lidar LM solve (k_lm_solve_m returns at once after the stop test or when a speculative candidate is already
installed): the loop must give the same bits whether the host reads the flags after every step (lm_iterate(sync=True): the stand-alone
accept/reject kernel) or only enqueues the steps (the accept/reject rides in the next Hessian pass), and with one damping candidate per
launch (vba_options::lm_spec = 1) or four.  W = 10 on the bench workload, W = 4 and W = 16 on small synthetic windows."""
import dataclasses
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 8


@pytest.fixture(scope="module")
def mods():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi, synth
    return capi, synth


def _workload(synth, name):
    if name == "w16":
        return dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=16, n_pts=8000)
    return synth.CONFIGS[name]


def _run(capi, wl, fac, poses, spec, sync):
    o = capi.options_from_workload(wl)
    o.lm_spec = spec
    ctx = capi.Context(o)
    ctx.push_dict(fac)
    ctx.lm_begin(poses, thd_num=2)
    for _ in range(ITERS):           # past the stop test the launches are gated off on the device: the result stays put
        ctx.lm_iterate(sync=sync)
    p, h, r = ctx.lm_end(fetch=True)
    out = dict(poses=p, hess=h, resis=r, trace=ctx.last_trace())
    ctx.close()
    return out


@pytest.mark.parametrize("name", ["hesai200k_w10", "room20k_w4", "w16"])
def test_lidar_lm_gated_launches_bit_identical(mods, name):
    capi, synth = mods
    wl = _workload(synth, name)
    s = synth.make_scans(wl)
    fac = synth.root_factors(s["points"], s["R0"], s["p0"], wl)
    poses = synth.poses_flat(s["R0"], s["p0"])
    runs = {(spec, sync): _run(capi, wl, fac, poses, spec, sync) for spec in (1, 4) for sync in (True, False)}
    ref = runs[(1, True)]
    assert len(ref["trace"]) >= 2
    for key, o in runs.items():
        for k in ("trace", "poses", "hess", "resis"):
            assert o[k].shape == ref[k].shape, (key, k)
            assert np.array_equal(o[k], ref[k]), (key, k, np.abs(o[k] - ref[k]).max())
    # the one-call form (vba_lidar_ba_damping_iter) runs the same loop
    o = capi.options_from_workload(wl)
    ctx = capi.Context(o)
    ctx.push_dict(fac)
    a = ctx.lidar_ba_damping_iter(poses, max_iter=ITERS, thd_num=2)
    ctx.close()
    assert np.array_equal(a["trace"], ref["trace"]) and np.array_equal(a["poses"], ref["poses"]) and np.array_equal(a["hess"], ref["hess"])
