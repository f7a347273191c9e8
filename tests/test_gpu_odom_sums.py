"""ONE point loop of each resident odometry update on the device (odom_match_body; kd_match_body, kd_fit_body, kd_accum_body; the
fixed-order reduction of k_odom_update), through vba_debug_odom_sums, against the references, margins and counted bars of
tests/odom_ref.py.  Decisions (match counts, 5-NN candidates, rejected fits) are compared exactly on points the reference calls clear;
values within bars of the form (counted roundings + terms) u (shadow).  The device's sums must equal a host sum of its own partials in
the documented order bit for bit.  Every case prints its worst ratio to bar; nothing depends on the printed value."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import odom_ref as orf

pytestmark = pytest.mark.gpu

LO = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def capi():
    import torch
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")                   # torch's HIP runtime comes up first, as in bench.py: the library then shares it
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


# ------------------------------------------------------------------------------------------------ voxel map
@pytest.fixture(scope="module")
def vox(capi):
    """the map of test_gpu_odom_resident.py (room20k_w4, 8 scans, local mapping on the ground-truth poses), its own leaf dump as the
    reference's plane data, and one corpus per (pose, covariance)"""
    from voxel_slam_amd import synth
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=4)
    W, nscan = wl.win_size, 8
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    ctx = capi.Context(capi.options_from_workload(wl))
    x_g, win_count = [], 0
    for k in range(nscan - 1):
        pose = synth.poses_flat(s["R_gt"][k:k + 1], s["p_gt"][k:k + 1])[0]
        x_g.append(pose.copy()); win_count += 1
        ctx.cut_voxel(win_count - 1, s["points"][k], x_g[-1], var=orf.rand_var(len(s["points"][k]), 100 + k, 0.01), multi=True)
        ctx.recut(win_count, np.array(x_g), multi=True)
        if win_count >= W:
            ctx.margi(win_count, np.array(x_g), jour=float(k))
            ctx.slide(1)
            x_g = x_g[1:]; win_count -= 1
    lm = orf.LeafMap.from_device(ctx.dump_leaves(), ctx.dump_plane_var(), wl.voxel_size, wl.max_layer)
    k = nscan - 1
    scan_world = s["points"][k] @ s["R_gt"][k].T + s["p_gt"][k]
    corpora = {}
    for pn, (R, t) in orf.scene_poses(s, k, synth).items():
        for cn, cov in orf.scene_covs().items():
            state = orf.state_of(R, t)
            pose = orf.Pose(state, cov)
            co = orf.voxel_corpus(lm, pose, scan_world, 11)
            assert co["dropped_random"] <= 0.02 * co["n_random"] and len(co["pts"]) >= 3585
            for c in orf.VOXEL_CLASSES:
                assert (co["cls"][:300] == c).sum() >= 2, c
            corpora[(pn, cn)] = dict(co, state=state, cov=cov)
    yield dict(ctx=ctx, lm=lm, corpora=corpora, wl=wl)
    ctx.close()


COMBOS = [("gt", "diag"), ("gt", "full"), ("perturbed", "diag"), ("perturbed", "full")]


def _check_voxel(out, ref, idx0, n):
    """partial rows against their 256 points, sums against all, sums == the documented host sum of partial; returns the worst ratio"""
    nb = (n + 255) // 256
    assert out["partial"].shape == (nb, 34)
    worst = 0.0
    for b in range(nb):
        worst = max(worst, orf.check_sums(out["partial"][b], ref.sums(idx0[256 * b:256 * b + 256])))
    worst = max(worst, orf.check_sums(out["sums"], ref.sums(idx0)))
    assert np.array_equal(out["sums"], orf.reduce_partials(out["partial"]))
    return worst


@pytest.mark.parametrize("pn,cn", COMBOS)
def test_voxel_single_points(vox, pn, cn):
    """n = 1: the decision of each of the first 300 points exact, its 34 terms within bars"""
    co, ctx = vox["corpora"][(pn, cn)], vox["ctx"]
    worst, seen = 0.0, set()
    for i in range(300):
        out = ctx.debug_odom_sums("voxel", co["pts"][i:i + 1], co["var"][i:i + 1], co["state"], co["cov"])
        assert out["sums"][33] == float(co["ref"].match[i]), "point %d (%s): device %r, reference %s" % (i, co["cls"][i], out["sums"][33], orf.REASONS[co["ref"].reason[i]])
        worst = max(worst, _check_voxel(out, co["ref"], [i], 1))
        seen.add((co["cls"][i], int(co["ref"].reason[i])))
    print("%s / %s: 300 single points, worst ratio to bar %.3g; (class, decision) pairs seen: %d" % (pn, cn, worst, len(seen)))
    assert {c for c, _ in seen} == set(orf.VOXEL_CLASSES)


@pytest.mark.parametrize("pn,cn", COMBOS)
def test_voxel_batches(vox, pn, cn):
    """prefixes whose sizes sit below, at and above a workgroup, and with 1, 2, 7, 8 and 15 partial rows; each ends in a match"""
    co, ctx = vox["corpora"][(pn, cn)], vox["ctx"]
    worst = {}
    for n in orf.BATCHES:
        assert co["ref"].match[n - 1]
        out = ctx.debug_odom_sums("voxel", co["pts"][:n], co["var"][:n], co["state"], co["cov"])
        worst[n] = _check_voxel(out, co["ref"], list(range(n)), n)
    print("%s / %s: worst ratio to bar by n: %s" % (pn, cn, {n: float("%.3g" % r) for n, r in worst.items()}))


def test_voxel_lone_match_and_no_match(vox):
    """a tail workgroup whose single point is the batch's only match; a batch that matches nothing gives exact zeros"""
    co, ctx = vox["corpora"][("perturbed", "full")], vox["ctx"]
    miss = np.nonzero(~co["ref"].match)[0][:256]
    hit = np.nonzero(co["ref"].match)[0][:1]
    assert len(miss) == 256
    idx = list(miss) + list(hit)
    out = ctx.debug_odom_sums("voxel", co["pts"][idx], co["var"][idx], co["state"], co["cov"])
    assert (out["partial"][0] == 0.0).all() and out["sums"][33] == 1.0 and out["partial"][1][33] == 1.0
    w = _check_voxel(out, orf.VoxelRef(vox["lm"], orf.Pose(co["state"], co["cov"]), co["pts"][idx], co["var"][idx]), list(range(257)), 257)
    out = ctx.debug_odom_sums("voxel", co["pts"][miss], co["var"][miss], co["state"], co["cov"])
    assert (out["partial"] == 0.0).all() and (out["sums"] == 0.0).all()
    assert not np.signbit(out["sums"]).any()
    print("lone match in the tail workgroup: worst ratio to bar %.3g" % w)


def _raw(capi, ctx, kind, n, pts, var, state, cov, slices, partial, sums, cand, planes):
    p = capi._p
    return ctx.lib.vba_debug_odom_sums(ctx.h, C.c_int(kind), C.c_int(n), p(pts), p(var), p(state), p(cov), C.c_int(slices), p(partial), p(sums),
                                       None if cand is None else cand.ctypes.data_as(C.c_void_p), p(planes), None)


def test_errors(vox, capi):
    co, ctx = vox["corpora"][("gt", "diag")], vox["ctx"]
    pts, var = np.ascontiguousarray(co["pts"][:4]), np.ascontiguousarray(co["var"][:4])
    st, cov = co["state"].copy(), np.ascontiguousarray(co["cov"])
    part, sums = np.zeros((1, 34)), np.zeros(34)
    cand, planes = np.zeros((8, 4, 5), dtype=np.uint64), np.zeros((4, 4))
    B = capi.ERR_BAD_ARG
    assert _raw(capi, ctx, 0, 4, pts, var, st, cov, 0, part, sums, None, None) == capi.OK
    assert _raw(capi, ctx, 0, 0, pts, var, st, cov, 0, part, sums, None, None) == B
    assert _raw(capi, ctx, 2, 4, pts, var, st, cov, 0, part, sums, None, None) == B
    assert _raw(capi, ctx, 0, 4, pts, var, st, cov, 1, part, sums, None, None) == B
    for missing in range(6):
        a = [pts, var, st, cov, part, sums]
        a[missing] = None
        assert _raw(capi, ctx, 0, 4, a[0], a[1], a[2], a[3], 0, a[4], a[5], None, None) == B
    for which in range(4):
        a = [pts.copy(), var.copy(), st.copy(), cov.copy()]
        a[which].reshape(-1)[1] = np.inf if which % 2 else np.nan
        assert _raw(capi, ctx, 0, 4, a[0], a[1], a[2], a[3], 0, part, sums, None, None) == B
    ctx.lib.vba_odom_kdtree_reset(ctx.h)
    assert _raw(capi, ctx, 1, 4, pts, None, st, cov, 1, part, sums, cand, planes) == B        # fewer than 100 map points
    sharded = capi.Context(capi.options_from_workload(vox["wl"]))
    try:
        sharded.set_shard(0, 2)
        assert _raw(capi, sharded, 0, 4, pts, var, st, cov, 0, part, sums, None, None) == capi.ERR_UNSUPPORTED
    finally:
        sharded.close()


# ------------------------------------------------------------------------------------------------ kd
IDENT_STATE = orf.state_of(np.eye(3), np.zeros(3))
COV = np.eye(15) * 1e-4
SLICES = (0, 1, 4, 8)
SIZES = (1, 255, 256, 257, 1793)


@pytest.fixture(scope="module")
def kctx(capi):
    from voxel_slam_amd import synth
    ctx = capi.Context(capi.options_from_workload(synth.CONFIGS["room20k_w4"]))
    yield ctx
    ctx.close()


def _seed(ctx, tree):
    """one call at the identity pose on an empty map: the map is then the float points themselves"""
    ctx.lib.vba_odom_kdtree_reset(ctx.h)
    ctx.lio_state_estimation_kdtree(tree, IDENT_STATE, COV)
    assert np.array_equal(ctx.kdtree_points(), tree)


def _kd_common(out, n):
    """what holds of every kd call: slices, zero columns, the exact count, the device's sums == the documented sum of its partials"""
    assert (out["partial"][:, 27:33] == 0.0).all() and (out["sums"][27:33] == 0.0).all()
    assert out["sums"][33] == float((out["planes"][:, 3] >= 0).sum())
    rej = out["planes"][:, 3] < 0
    assert (out["planes"][rej] == (0.0, 0.0, 0.0, -1.0)).all()
    assert np.array_equal(out["sums"], orf.reduce_partials(out["partial"]))
    for b in range(len(out["partial"])):
        assert out["partial"][b, 33] == float((out["planes"][256 * b:256 * b + 256, 3] >= 0).sum())


def _cand_equal(out, want, what):
    got = out["cand"]
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=(0, 2)))[0]
    if len(bad):
        s, k = np.argwhere(got[:, bad[0]] != want[:, bad[0]])[0]
        raise AssertionError("%s: %d of %d queries differ from the unfused float32 restatement; query %d, slice %d, slot %d: device %#x, restatement %#x"
                             % (what, len(bad), got.shape[1], bad[0], s, k, int(got[s, bad[0], k]), int(want[s, bad[0], k])))


@pytest.mark.parametrize("m", [100, 256, 257, 600, 2100])
def test_kd_lattice_is_bit_exact(kctx, m):
    """integer lattice, half-integer queries: every float operation exact, ties everywhere; all slice counts (empty slices included),
    scans below, at and above a workgroup"""
    tree, q = orf.lattice_corpus(m, max(SIZES))
    _seed(kctx, tree)
    pose = orf.Pose(IDENT_STATE, COV)
    unfilled = 0
    for slices in SLICES:
        for n in SIZES:
            out = kctx.debug_odom_sums("kd", q[:n], None, IDENT_STATE, COV, slices=slices)
            ns = slices or 8                                            # kd_slices_of(nb) for fewer than 128 workgroups
            assert out["slices"] == ns
            want = orf.kd_candidates(orf.kd_query(pose, q[:n]), tree, ns)
            _cand_equal(out, want, "m %d, slices %d, n %d" % (m, slices, n))
            empty = (out["cand"] & LO) == LO
            assert (out["cand"][empty] == orf.UNFILLED).all()
            unfilled += int(empty.sum())
            _kd_common(out, n)
    assert unfilled > 0 or m >= 2100
    print("m %d: candidates bit for bit over slices %s x n %s; %d unfilled slots seen" % (m, SLICES, SIZES, unfilled))


def test_kd_near_ties_follow_the_unfused_float_distance(kctx):
    """queries whose neighbours a fused and an unfused float distance order differently (exact-arithmetic emulation): the candidates
    are those of FLANN's separately rounded accumulation"""
    tree, q = orf.near_tie_corpus()
    assert len(q) >= 50
    _seed(kctx, tree)
    pose = orf.Pose(IDENT_STATE, COV)
    qf = orf.kd_query(pose, q)
    fused = orf.kd_candidates(qf, tree, 1, "fused")
    for slices in SLICES:
        out = kctx.debug_odom_sums("kd", q, None, IDENT_STATE, COV, slices=slices)
        want = orf.kd_candidates(qf, tree, out["slices"])
        if slices == 1:
            print("near ties: %d of %d queries carry the fused emulation's words" % ((out["cand"] == fused).all(axis=(0, 2)).sum(), len(q)))
        _cand_equal(out, want, "near ties, slices %d" % slices)
        _kd_common(out, len(q))


@pytest.mark.parametrize("general", [False, True])
def test_kd_room(kctx, general):
    """plane-like points: candidates bit for bit, planes of clear points within the perturbation bar, rejected fits exactly (0, 0, 0, -1),
    partials and sums within counted bars of the reference evaluated from the device's planes"""
    tree, q = orf.room_corpus(2100, max(SIZES))
    _seed(kctx, tree)
    state = IDENT_STATE
    if general:
        R, t = orf.general_pose()
        state = orf.state_of(R, t)
        drop = orf.fused_query_differs(orf.Pose(state, COV), q)
        assert drop.sum() <= 0.001 * len(q)
        q = q[~drop]
    pose = orf.Pose(state, COV)
    worst = dict(normal=0.0, distance=0.0, sums=0.0)
    for slices in SLICES:
        for n in SIZES:
            n = min(n, len(q))
            out = kctx.debug_odom_sums("kd", q[:n], None, state, COV, slices=slices)
            _cand_equal(out, orf.kd_candidates(orf.kd_query(pose, q[:n]), tree, out["slices"]), "room, slices %d, n %d" % (slices, n))
            _kd_common(out, n)
            fit = orf.kd_fit_ref(tree, orf.kd_merge(out["cand"]))
            clear = ~fit["unclear"]
            assert (~clear).sum() <= max(1, 0.02 * n)
            assert np.array_equal(out["planes"][clear, 3] < 0, fit["reject"][clear])
            mk = clear & ~fit["reject"]
            if mk.any():
                worst["normal"] = max(worst["normal"], (np.abs(out["planes"][mk, :3] - fit["planes"][mk, :3]).max(axis=1) / fit["bar_n"][mk]).max())
                worst["distance"] = max(worst["distance"], (np.abs(out["planes"][mk, 3] - fit["planes"][mk, 3]) / fit["bar_d"][mk]).max())
            ks = orf.KdSumsRef(pose, q[:n], out["planes"])
            for b in range(len(out["partial"])):
                worst["sums"] = max(worst["sums"], orf.check_sums(out["partial"][b], ks.sums(range(256 * b, min(n, 256 * b + 256)))))
            worst["sums"] = max(worst["sums"], orf.check_sums(out["sums"], ks.sums(range(n))))
    print("room, general pose %s: worst ratios to bar %s" % (general, {k: float("%.3g" % v) for k, v in worst.items()}))
    assert worst["normal"] <= 1 and worst["distance"] <= 1


def test_kd_errors(kctx, capi):
    tree, q = orf.room_corpus(150, 8)
    _seed(kctx, tree)
    pts = np.ascontiguousarray(q[:4]); st = IDENT_STATE.copy(); cov = np.ascontiguousarray(COV)
    part, sums = np.zeros((1, 34)), np.zeros(34)
    cand, planes = np.zeros((8, 4, 5), dtype=np.uint64), np.zeros((4, 4))
    B = capi.ERR_BAD_ARG
    assert _raw(capi, kctx, 1, 4, pts, None, st, cov, 0, part, sums, cand, planes) == capi.OK
    assert _raw(capi, kctx, 1, 4, pts, None, st, cov, 9, part, sums, cand, planes) == B
    assert _raw(capi, kctx, 1, 4, pts, None, st, cov, -1, part, sums, cand, planes) == B
    assert _raw(capi, kctx, 1, 4, pts, None, st, cov, 1, part, sums, None, planes) == B
    assert _raw(capi, kctx, 1, 4, pts, None, st, cov, 1, part, sums, cand, None) == B
    assert _raw(capi, kctx, 1, -1, pts, None, st, cov, 1, part, sums, cand, planes) == B
    bad = pts.copy(); bad[2, 1] = np.nan
    assert _raw(capi, kctx, 1, 4, bad, None, st, cov, 1, part, sums, cand, planes) == B
    assert kctx.kdtree_size() == 150 and np.array_equal(kctx.kdtree_points(), tree)              # the map is read, not appended to
