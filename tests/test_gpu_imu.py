"""The IMU factor pass of LI-BA on the device (li_imu_body in its three launch forms, the trial-state residual of k_li_update) against
the double-double reference and the per-entry bars of tests/imu_ref.py, through vba_debug_li_imu, and the hess of the production call
vba_li_ba_damping_iter against imu_coef * H_imu* + H_lidar*.
  * alone (k_li_imu): every class of the corpus at every W = 2..16, both gravity modes: every entry of H and g, rimu[0], rimu[1] (the
    trial flag, same states) within the bars, entries outside the pattern exactly 0, a repeat identical in its bits;
  * riding k_hessian2 (W = 2, 3, 10, 11, 16) and riding k_hessian3 (hessian_compact_tiles contexts, W = 2, 3, 10: the kernel exists up
    to W = 10, and the hook refuses the form at 11 and 16, asserted) over a five-voxel store of the hess_ref corpus: the same bits as
    the stand-alone form, and within the bars;
  * the reference is computed once for the whole corpus, on the cov^-1 blocks the hook hands back, and shared by the forms;
  * the production call on the `offset` window at W = 3, 10, 16 with gravity (max_iter = 1) and W = 3, 10 without: see
    test_production_hess for which state its hess belongs to, and how the three forced iterations of the second mode are ended;
  * the same call through its sharded flow with one rank (force_collective, W = 2 and 11, both gravity modes): hess under the same
    bar, states, increments and trace against the CPU oracle (test_collective_flow_one_rank).
The printed ratios are reports; nothing depends on them."""
import numpy as np
import pytest

import hess_ref as R
import imu_ref as I

pytestmark = pytest.mark.gpu

RIDE_WS = [2, 3, 10, 11, 16]


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


def _ctx(capi, W, **kw):
    o = capi.default_options()
    o.win_size = W
    for k, v in kw.items():
        setattr(o, k, v)
    return capi.Context(o)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("H", "g", "rimu", "covinv"))


@pytest.fixture(scope="module")
def alone(capi):
    """the stand-alone form on every window of the corpus (with the trial flag, twice), and the reference on the cov^-1 it returned"""
    out = {}
    for W in I.WS:
        ctx = _ctx(capi, W)
        try:
            for cls in I.CLASSES:
                st, im = I.inputs(cls, W)
                for gravity in (0, 1):
                    out[(cls, W, gravity)] = [ctx.debug_li_imu(st, im, gravity=bool(gravity), form="alone", trial=True) for _ in range(2)]
        finally:
            ctx.close()
    keys = [(c, W) for c in I.CLASSES for W in I.WS]
    for c, W in keys:
        assert np.array_equal(out[(c, W, 0)][0]["covinv"], out[(c, W, 1)][0]["covinv"])
    ref = I.Ref([I.inputs(c, W) + (out[(c, W, 1)][0]["covinv"],) for c, W in keys])
    return ref, {k: i for i, k in enumerate(keys)}, out


def test_reference_is_the_pinned_one(alone):
    """the corpus condition and the counts hold on the reference the device is held to (its cov^-1 is the hook's)"""
    ref = alone[0]
    assert ref.margins() == [] and ref.branch_consistent() == []
    assert ref.counts() == dict(D_RR=I.D_RR, D_JOC=I.D_JOC, D_CJ=I.D_CJ, D_HF=I.D_HF, D_GF=I.D_GF, D_QF=I.D_QF)


@pytest.mark.parametrize("W", I.WS)
def test_alone_every_class(alone, W):
    ref, ix, out = alone
    worst, bad = {}, []
    for cls in I.CLASSES:
        for gravity in (0, 1):
            a, b = out[(cls, W, gravity)]
            assert _same(a, b), (cls, gravity, "a repeat differs")
            assert not a["H"][~I.pattern_mask(W, gravity)].any()
            q = I.check(*ref.window(ix[(cls, W)], gravity), a["H"], a["g"], a["rimu"][0], a["rimu"][1])
            for k, v in q.items():
                worst[(gravity, k)] = max(worst.get((gravity, k), 0.0), v)
            if not max(q.values()) <= 1.0:
                bad.append((cls, gravity, q))
    print("\nk_li_imu alone W=%d worst ratio to bar (gravity, quantity): %s" % (W, {"%d/%s" % k: "%.3g" % v for k, v in sorted(worst.items())}))
    assert not bad, bad[:6]


@pytest.mark.parametrize("form", ["h2", "h3"])
@pytest.mark.parametrize("W", RIDE_WS)
def test_riding_forms(capi, alone, W, form):
    ref, ix, out = alone
    st5 = R.reorder(R.store(W), np.arange(5))
    ctx = _ctx(capi, W, hessian_compact_tiles=1 if form == "h3" else 0)
    worst = {}
    try:
        st0, im0 = I.inputs("offset", W)
        with pytest.raises(capi.VbaError) as e:                             # a riding form without a pushed store
            ctx.debug_li_imu(st0, im0, gravity=True, form=form)
        assert e.value.status == capi.ERR_BAD_ARG
        ctx.push_voxels(st5["clusters"], st5["fix"], st5["coe"], st5["eig_val"], st5["eig_vec"], st5["pcr_add"])
        other = "h2" if form == "h3" else "h3"
        with pytest.raises(capi.VbaError) as e:                             # the form the context does not select for this window
            ctx.debug_li_imu(st0, im0, gravity=True, form=other if W <= 10 else "h3")
        assert e.value.status == capi.ERR_BAD_ARG
        if form == "h3" and W > 10:                                         # k_hessian3 exists for W <= 10 only: nothing to ride
            return
        for cls in I.CLASSES:
            for gravity in (0, 1):
                a = ctx.debug_li_imu(*I.inputs(cls, W), gravity=bool(gravity), form=form, trial=True)
                assert _same(a, out[(cls, W, gravity)][0]), (cls, gravity, "differs from the stand-alone form")
                q = I.check(*ref.window(ix[(cls, W)], gravity), a["H"], a["g"], a["rimu"][0], a["rimu"][1])
                assert max(q.values()) <= 1.0, (cls, gravity, q)
                for k, v in q.items():
                    worst[(gravity, k)] = max(worst.get((gravity, k), 0.0), v)
    finally:
        ctx.close()
    print("\nriding %s W=%d worst ratio to bar (gravity, quantity): %s" % (form, W, {"%d/%s" % k: "%.3g" % v for k, v in sorted(worst.items())}))


def test_hook_refuses(capi):
    W = 4
    st, im = I.inputs("offset", W)
    ctx = _ctx(capi, W)
    try:
        def bad(status=None, **kw):
            with pytest.raises(capi.VbaError) as e:
                ctx.debug_li_imu(kw.pop("st", st), kw.pop("im", im), **kw)
            assert e.value.status == (capi.ERR_BAD_ARG if status is None else status)
        bad(raw_flags=8); bad(raw_flags=3); bad(raw_flags=-1)
        bad(form="h2"); bad(form="h3")                                      # no store
        x = st.copy(); x[2, 5] = np.nan
        bad(st=x)
        y = im.copy(); y[1, 100] = np.inf
        bad(im=y)
        lib = ctx.lib
        import ctypes as C
        z = np.zeros(8)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.vba_debug_li_imu(ctx.h, C.c_int(5), C.c_int(0), C.c_int(0), p(st), p(im), p(z), p(z), p(z), None) == capi.ERR_BAD_ARG      # not the context's W
        assert lib.vba_debug_li_imu(ctx.h, C.c_int(W), C.c_int(2), C.c_int(0), p(st), p(im), p(z), p(z), p(z), None) == capi.ERR_BAD_ARG
        assert lib.vba_debug_li_imu(ctx.h, C.c_int(W), C.c_int(0), C.c_int(0), None, p(im), p(z), p(z), p(z), None) == capi.ERR_BAD_ARG
        a = ctx.debug_li_imu(st, im, gravity=True)                          # and the context still works
        assert np.isfinite(a["H"]).all() and a["rimu"][1] == 0.0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the production call
def _store_at(poses, seed, V=5, ballast=0.0):
    """V planar voxels seen by every frame, consistent with the window's poses (so that the LM loop has a sensible lidar part).
    ballast: one more voxel that holds a fixed cluster only (no frame sees it: it adds nothing to H and g, exactly) with coe chosen so
    that its constant residual coe * lambda_0 is `ballast`"""
    rng = np.random.default_rng(seed)
    W = len(poses)
    n_all = V + (1 if ballast else 0)
    clusters = np.zeros((n_all, W, 10)); fix = np.zeros((n_all, 10)); coe = np.concatenate([rng.uniform(0.5, 2.0, V), np.ones(n_all - V)])
    for a in range(n_all):
        n, t1, t2 = R._frame(rng)
        c0 = poses[W // 2, 9:] + rng.normal(0, 3.0, 3)
        patch = lambda m: c0 + np.outer(rng.uniform(-0.4, 0.4, m), t1) + np.outer(rng.uniform(-0.4, 0.4, m), t2) + np.outer(rng.normal(0, 0.01, m), n)
        if a >= V:
            fix[a] = R.cluster(patch(100))
            continue
        for i in range(W):
            clusters[a, i] = R.cluster(R._body(patch(int(rng.integers(20, 200))), poses[i]))
    ev, evec, pa = R.host_eigen(clusters, fix, poses)
    if ballast:
        coe[V] = ballast / ev[V, 0]
    return dict(clusters=clusters, fix=fix, coe=coe, eig_val=ev, eig_vec=evec, pcr_add=pa)


def _poses(states):
    return np.ascontiguousarray(states[:, 1:13])


@pytest.mark.parametrize("W,gravity", [(3, 1), (10, 1), (16, 1), (3, 0), (10, 0)])
def test_production_hess(capi, W, gravity):
    """hess of vba_li_ba_damping_iter.  From VM:565-578 / 803-814 and li_ba_device: *hess is the assembled imu_coef * IMU + lidar matrix
    BEFORE the gauge and the damping (k_li_solve applies both while it loads the system and never writes them back), of the LAST
    Hessian evaluation of the call.  With gravity and max_iter = 1 that is the evaluation at the states passed in, from the pushed
    eigen-data.  Without gravity the call runs three iterations whatever max_iter says (VM:643), and after an accepted step its hess
    belongs to a state it does not return.  So the store of those two cases carries one more voxel with a fixed cluster only: it adds
    exactly nothing to H and g and a constant to the residual, 1e8 times the whole residual of the window at the states passed in
    (taken from the references: imu_coef / 2 * rimu* + sum coe lambda_0).  No step can then change the cost by 1e-6 of itself, the
    loop's own criterion (VM:492) ends it after the first iteration (asserted: one trace row), and hess is the evaluation at the
    states passed in."""
    st, im = I.inputs("offset", W)
    ctx = _ctx(capi, W)
    try:
        covinv = ctx.debug_li_imu(st, im, gravity=bool(gravity))["covinv"]
        coef = float(ctx.opt.imu_coef)
        Ht, _, rt = I.Ref([(st, im, covinv)]).window(0, gravity)
        store = _store_at(_poses(st), 77 + W)
        if not gravity:
            whole = 0.5 * coef * float(rt.v.f64()) + float((store["coe"] * store["eig_val"][:, 0]).sum())
            store = _store_at(_poses(st), 77 + W, ballast=1e8 * whole)
        ctx.push_voxels(store["clusters"], store["fix"], store["coe"], store["eig_val"], store["eig_vec"], store["pcr_add"])
        out = ctx.li_ba_damping_iter(st, im, gravity=bool(gravity), max_iter=1)
        tr = out["trace"]
        print("\nproduction W=%d gravity=%d trace rows [r1 r2 u v q1]:\n%s" % (W, gravity, tr))
        assert len(tr) == 1, tr
    finally:
        ctx.close()
    lid = R.Ref(store["clusters"], store["coe"], store["eig_val"], store["eig_vec"], store["pcr_add"], _poses(st))
    (Hl, _, _), (barL, _, _) = lid.sums(np.arange(len(store["coe"])))
    n = 15 * W + 3 * gravity
    pose = np.array([15 * (k // 6) + k % 6 for k in range(6 * W)])
    Hs = R.DD(Ht.v.hi.copy(), Ht.v.lo.copy()) * R.DD(np.full((n, n), coef))
    L = R.DD(np.zeros((n, n)))
    L.hi[np.ix_(pose, pose)] = Hl.hi; L.lo[np.ix_(pose, pose)] = Hl.lo
    Hs = Hs + L
    bar = coef * Ht.bar()
    bar[np.ix_(pose, pose)] += barL
    H = out["hess"]
    assert np.isfinite(H).all()
    err = Hs.err_to(H)
    z = bar == 0.0
    assert not H[z].any()
    ratio = float((err[~z] / bar[~z]).max())
    print("production W=%d gravity=%d hess worst ratio to imu_coef * bar_imu + bar_lidar: %.3g" % (W, gravity, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ the LI call's sharded flow, one rank
COLL_V = 70        # voxels of the store: three workgroups of the residual pass, pushed in one fixed order


def _oracle_li(W, store, st, im, gravity, coef, max_iter):
    import oracle_api
    f = oracle_api.Factor(W)
    f.push_dict(store)
    return f.li_ba_damping_iter(st, im, gravity=bool(gravity), imu_coef=coef, max_iter=max_iter)


@pytest.mark.parametrize("gravity", [0, 1])
@pytest.mark.parametrize("W", [2, 11])
def test_collective_flow_one_rank(capi, W, gravity):
    """vba_li_ba_damping_iter with force_collective = 1 and an all-reduce hook that returns its input: the sharded branch of the LI call
    (stand-alone init, the trial step with its speculative Hessian pass and the one all-reduce, *hess from the saved copy `raw`) with
    one rank, which otherwise runs only under the two-process shard tests.  W = 2, and W = 11, the smallest window whose k_li_solve
    keeps L outside the LDS; gravity off and on.  Two calls per case on a context of its own:
      * *hess, in the setting of test_production_hess (max_iter = 1 with gravity, the ballast voxel without), against the same
        double-double sum and under the same bar, worst ratio <= 1;
      * states, the IMU increments and the trace of a three-iteration call on the plain store (an iteration after an accepted step
        starts from the all-reduced Hessian of the trial step) against the CPU oracle.  This file held no bar for them; they are the bars of the
        single-rank LI cases of test_gpu_factor.py (test_li_ba_damping_iter_parity), unchanged: trace rtol 1e-6 / atol 1e-10, states
        and increments 1e-7."""
    st, im = I.inputs("offset", W)
    plain = _ctx(capi, W)
    try:
        covinv = plain.debug_li_imu(st, im, gravity=bool(gravity))["covinv"]      # (the hook is not available on a collective context)
        coef = float(plain.opt.imu_coef)
    finally:
        plain.close()
    Ht, _, rt = I.Ref([(st, im, covinv)]).window(0, gravity)
    store = _store_at(_poses(st), 177 + W, V=COLL_V)
    pinned = store
    if not gravity:
        whole = 0.5 * coef * float(rt.v.f64()) + float((store["coe"] * store["eig_val"][:, 0]).sum())
        pinned = _store_at(_poses(st), 177 + W, V=COLL_V, ballast=1e8 * whole)
    outs = []
    for fac, max_iter in ((pinned, 1), (store, 3)):
        ctx = _ctx(capi, W, force_collective=1)
        try:
            ctx.set_allreduce(lambda ptr, n, stream: 0)     # one rank: the sum over the ranks is the buffer itself
            ctx.push_voxels(fac["clusters"], fac["fix"], fac["coe"], fac["eig_val"], fac["eig_vec"], fac["pcr_add"])
            outs.append(ctx.li_ba_damping_iter(st, im, gravity=bool(gravity), max_iter=max_iter))
        finally:
            ctx.close()
    one, three = outs
    assert len(one["trace"]) == 1, one["trace"]
    # *hess of the pinned call
    lid = R.Ref(pinned["clusters"], pinned["coe"], pinned["eig_val"], pinned["eig_vec"], pinned["pcr_add"], _poses(st))
    (Hl, _, _), (barL, _, _) = lid.sums(np.arange(len(pinned["coe"])))
    n = 15 * W + 3 * gravity
    pose = np.array([15 * (k // 6) + k % 6 for k in range(6 * W)])
    Hs = R.DD(Ht.v.hi.copy(), Ht.v.lo.copy()) * R.DD(np.full((n, n), coef))
    L = R.DD(np.zeros((n, n)))
    L.hi[np.ix_(pose, pose)] = Hl.hi; L.lo[np.ix_(pose, pose)] = Hl.lo
    Hs = Hs + L
    bar = coef * Ht.bar()
    bar[np.ix_(pose, pose)] += barL
    H = one["hess"]
    assert np.isfinite(H).all()
    err = Hs.err_to(H)
    z = bar == 0.0
    assert not H[z].any()
    ratio = float((err[~z] / bar[~z]).max())
    print("\ncollective W=%d gravity=%d hess worst ratio to imu_coef * bar_imu + bar_lidar: %.3g" % (W, gravity, ratio))
    # states, increments and trace of the three-iteration call against the oracle (the pinned call is built for *hess alone: beside its
    # ballast the accept test of the gravity-free mode compares two sums that agree to 1e-8 of themselves)
    b = _oracle_li(W, store, st, im, gravity, coef, 3)
    tr_ok = three["trace"].shape == b["trace"].shape and np.allclose(three["trace"], b["trace"], rtol=1e-6, atol=1e-10)
    ds = float(np.abs(three["states"] - b["states"]).max()); di = float(np.abs(three["imus"] - b["imus"]).max())
    print("collective W=%d gravity=%d max_iter=3: %d trace rows (oracle %d), close %s; states %.3g, increments %.3g (bar 1e-7)"
          % (W, gravity, len(three["trace"]), len(b["trace"]), tr_ok, ds, di))
    assert ratio <= 1.0
    assert tr_ok and ds < 1e-7 and di < 1e-7
