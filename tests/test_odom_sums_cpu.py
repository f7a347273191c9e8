"""The references of tests/odom_ref.py for one point loop of the two resident odometry updates, on the host alone: the counted rounding
numbers, the double-double code against mpmath, plain-f64 restatements of both loops inside every bar (calibration: the voxel loop on
the ORACLE map's dump of the scene of test_gpu_odom_resident.py), the caps on unclear points, and the teeth: each listed defect of a
restatement exceeds a bar or flips a clear decision.  Worst ratios to bar are printed; nothing depends on the printed values."""
import dataclasses

import numpy as np
import pytest

import odom_ref as orf


# ------------------------------------------------------------------------------------------------ voxel scene (oracle map)
@pytest.fixture(scope="module")
def vscene(oracle):
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=4)
    W, nscan = wl.win_size, 8
    s = synth.make_scans(dataclasses.replace(wl, win_size=nscan))
    om = oracle.VoxelMap(W, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, 5)
    of = oracle.Factor(W)
    x_o, win_count = [], 0
    for k in range(nscan - 1):
        pose = synth.poses_flat(s["R_gt"][k:k + 1], s["p_gt"][k:k + 1])[0]
        x_o.append(pose.copy()); win_count += 1
        om.cut_voxel(win_count - 1, s["points"][k], x_o[-1], var=orf.rand_var(len(s["points"][k]), 100 + k, 0.01), multi=True)
        om.recut(win_count, np.array(x_o), of, multi=True)
        if win_count >= W:
            om.margi(win_count, np.array(x_o), of)
            om.slide(1)
            x_o = x_o[1:]; win_count -= 1
    lm = orf.LeafMap(om.dump_leaves(), om.dump_plane_var(), wl.voxel_size, wl.max_layer)
    return dict(lm=lm, poses=orf.scene_poses(s, nscan - 1, synth), scan_world=s["points"][nscan - 1] @ s["R_gt"][nscan - 1].T + s["p_gt"][nscan - 1])


@pytest.fixture(scope="module")
def corpora(vscene):
    out = {}
    for pn, (R, t) in vscene["poses"].items():
        for cn, cov in orf.scene_covs().items():
            pose = orf.Pose(orf.state_of(R, t), cov)
            out[(pn, cn)] = (pose, orf.voxel_corpus(vscene["lm"], pose, vscene["scan_world"], 11))
    return out


def test_counted_roundings_are_what_the_code_keeps(corpora):
    """D_* of the module docstring against the reference's own count, at a general pose and a full covariance"""
    pose, co = corpora[("perturbed", "full")]
    ref = co["ref"]
    assert (ref.k_w, ref.k_resi, ref.k_sigma) == (orf.K_W, orf.K_RESI, orf.K_SIGMA)
    assert max(ref.k[:21]) == orf.D_HTH and max(ref.k[21:27]) == orf.D_HTZ and max(ref.k[27:33]) == orf.D_NNT and ref.k[33] == 0
    tree, q = orf.room_corpus(300, 64)
    ks = orf.KdSumsRef(pose, q, orf.kd_fit_restate(tree, orf.kd_merge(orf.kd_candidates(orf.kd_query(pose, q), tree, 1))))
    assert max(ks.k[:21]) == orf.D_KD_HTH and max(ks.k[21:27]) == orf.D_KD_HTZ


def test_double_double_against_mpmath(vscene, corpora):
    """the same formula over mpmath numbers at 200 bits: the double-double terms agree to 1e-28 of their shadows"""
    mpmath = pytest.importorskip("mpmath")
    pose, co = corpora[("perturbed", "full")]
    idx = np.nonzero(co["ref"].match)[0][:6]
    with mpmath.workprec(200):
        a = orf.VoxelRef(vscene["lm"], pose, co["pts"][idx], co["var"][idx], T=orf.MP)
        b = orf.VoxelRef(vscene["lm"], pose, co["pts"][idx], co["var"][idx])
        assert a.match.all() and b.match.all()
        worst = 0.0
        for x, y in zip(a.t, b.t):
            err = x.v.err_to(y.v.f64()) / y.m
            worst = max(worst, err.max())
            assert (err <= 4 * orf.U).all()                       # f64 of the double-double value: one rounding of a 106-bit number
            lo = np.array([abs(float(p - mpmath.mpf(float(h)) - mpmath.mpf(float(l)))) for p, h, l in zip(x.v.a, y.v.hi, y.v.lo)])
            assert (lo <= 1e-28 * y.m).all()
    print("double-double vs mpmath: f64 of the value within %.3g u of the shadow" % (worst / orf.U))


@pytest.mark.parametrize("pn", ["gt", "perturbed"])
@pytest.mark.parametrize("cn", ["diag", "full"])
def test_voxel_restatement_inside_every_bar(vscene, corpora, pn, cn):
    """calibration: plain f64, literal formula, every workgroup row and every prefix of BATCHES; the reduction order bit for bit"""
    pose, co = corpora[(pn, cn)]
    ref = co["ref"]
    terms = orf.voxel_restate(vscene["lm"], pose, co["pts"], co["var"])
    assert np.array_equal(terms[:, 33] == 1.0, ref.match)
    worst = 0.0
    for n in orf.BATCHES:
        part = orf.wg_partials(terms[:n])
        for b in range(len(part)):
            worst = max(worst, orf.check_sums(part[b], ref.sums(range(256 * b, min(n, 256 * b + 256)))))
        worst = max(worst, orf.check_sums(orf.reduce_partials(part), ref.sums(range(n))))
    print("%s / %s: worst ratio to bar %.3g; classes %s" % (pn, cn, worst, {c: int((co["cls"] == c).sum()) for c in orf.VOXEL_CLASSES}))


def test_caps(corpora):
    for key, (pose, co) in corpora.items():
        print(key, "unclear random points dropped: %d of %d" % (co["dropped_random"], co["n_random"]))
        assert co["dropped_random"] <= 0.02 * co["n_random"]
        assert len(co["pts"]) >= 3585
        for c in orf.VOXEL_CLASSES:
            assert (co["cls"][:300] == c).sum() >= 2 and (co["cls"] == c).sum() >= 15, c
        assert not co["ref"].unclear.any()
        assert all(co["ref"].match[n - 1] for n in orf.BATCHES)
        deep = co["cls"] == "max_layer"
        assert (co["ref"].layer[deep] == 2).all() and co["ref"].match[deep].all()


def _voxel_bites(vscene, pose, co, n, defect=None, part_defect=None, red_defect=None):
    terms = orf.voxel_restate(vscene["lm"], pose, co["pts"][:n], co["var"][:n], defect)
    part = orf.wg_partials(terms, part_defect)
    try:
        for b in range(len(part)):
            orf.check_sums(part[b], co["ref"].sums(range(256 * b, min(n, 256 * b + 256))))
        orf.check_sums(orf.reduce_partials(part, red_defect), co["ref"].sums(range(n)))
    except AssertionError as e:
        return str(e)
    return ""


@pytest.mark.parametrize("defect", ["no_tsl_var", "no_rot_var", "R_for_Rt", "0.0004", "sigma_float"])
def test_teeth_formula(vscene, corpora, defect):
    pose, co = corpora[("perturbed", "full")]
    assert _voxel_bites(vscene, pose, co, 257) == ""
    why = _voxel_bites(vscene, pose, co, 257, defect)
    print(defect, "->", why)
    assert why


def test_teeth_reduction(vscene, corpora):
    pose, co = corpora[("perturbed", "diag")]
    assert _voxel_bites(vscene, pose, co, 1793) == ""
    why = _voxel_bites(vscene, pose, co, 257, part_defect="drop_tail")     # the last point of the partial workgroup is a match
    print("drop_tail ->", why)
    assert why
    why = _voxel_bites(vscene, pose, co, 1793, red_defect="drop_group")
    print("drop_group ->", why)
    assert why


def test_teeth_sigma_gate_le():
    """`<=` for `<`: a comparison of exact zeros (a point at the centre of a plane through the origin, no variance anywhere) is clear,
    0 < 0 is no match, and the defect matches it"""
    leaves = np.zeros((1, 39)); leaves[0, 7] = 1.0; leaves[0, 37] = 1.0; leaves[0, 38] = 0.01
    lm = orf.LeafMap(leaves, np.zeros((1, 36)), 0.5, 2)
    pose = orf.Pose(orf.state_of(np.eye(3), np.zeros(3)), np.zeros((15, 15)))
    pts, var = np.zeros((1, 3)), np.zeros((1, 9))
    ref = orf.VoxelRef(lm, pose, pts, var)
    assert not ref.unclear.any() and ref.reason[0] == orf.SIGMA_GATE
    orf.check_sums(orf.voxel_restate(lm, pose, pts, var).sum(axis=0), ref.sums([0]))
    with pytest.raises(AssertionError):
        orf.check_sums(orf.voxel_restate(lm, pose, pts, var, "le_gate").sum(axis=0), ref.sums([0]))


# ------------------------------------------------------------------------------------------------ kd
IDENT = orf.Pose(orf.state_of(np.eye(3), np.zeros(3)), np.eye(15) * 1e-4)


@pytest.fixture(scope="module")
def near_tie():
    return orf.near_tie_corpus()


def test_near_tie_corpus(near_tie):
    """at least 50 queries whose neighbours the fused and the unfused float distance order differently, by exact arithmetic; numpy's
    float32 is the unfused one"""
    tree, q = near_tie
    assert len(q) >= 50 and len(tree) == 7 * len(q)
    qf = orf.kd_query(IDENT, q)
    assert np.array_equal(qf.astype(np.float64), q) and np.array_equal(tree.astype(np.float32).astype(np.float64), tree)
    cu = orf.kd_candidates(qf, tree, 1)
    lo = np.uint64(0xFFFFFFFF)
    for i in range(len(q)):
        own = range(7 * i, 7 * i + 7)
        for fused in (False, True):
            d = [orf.kd_dist_exact(qf[i], tree[j].astype(np.float32), fused) for j in own]
            want = sorted(own, key=lambda j: (d[j - 7 * i], j))[:5]
            if not fused:
                assert [int(w & lo) for w in cu[0, i]] == want
                assert [np.uint32(int(w) >> 32).view(np.float32) for w in cu[0, i]] == [d[j - 7 * i] for j in want]
            else:
                assert [int(w & lo) for w in cu[0, i]] != want


def test_teeth_selection(near_tie):
    tree, q = near_tie
    qf = orf.kd_query(IDENT, q)
    good = orf.kd_candidates(qf, tree, 4)
    for mode in ("fused", "double"):
        bad = orf.kd_candidates(qf, tree, 4, mode)
        differ = (orf.kd_merge(bad) != orf.kd_merge(good)).any(axis=1).sum()
        print(mode, "distance: %d of %d near-tie queries select differently" % (differ, len(q)))
        assert differ > 0
    lt, lq = orf.lattice_corpus(600, 257)
    lf = orf.kd_query(IDENT, lq)
    good = orf.kd_candidates(lf, lt, 8)
    assert (orf.kd_candidates(lf, lt, 8, later_wins=True) != good).any()                         # a tie to the later index
    assert (orf.kd_merge(good, first_slice_only=True) != orf.kd_merge(good)).any()               # slices >= 1 ignored
    assert np.array_equal(orf.kd_merge(good), orf.kd_merge(orf.kd_candidates(lf, lt, 1)))        # the slicing itself changes nothing
    assert np.array_equal(orf.kd_candidates(lf, lt, 8, "fused"), good)                          # exact arithmetic: fused or not


@pytest.mark.parametrize("general", [False, True])
def test_kd_restatement_inside_every_bar(general):
    tree, q = orf.room_corpus(2100, 1793)
    pose = IDENT
    if general:
        R, t = orf.general_pose()
        pose = orf.Pose(orf.state_of(R, t), np.eye(15) * 1e-4)
        drop = orf.fused_query_differs(pose, q)
        assert drop.sum() <= 0.001 * len(q)
        q = q[~drop]
    best = orf.kd_merge(orf.kd_candidates(orf.kd_query(pose, q), tree, 4))
    fit = orf.kd_fit_ref(tree, best)
    rs = orf.kd_fit_restate(tree, best)
    clear = ~fit["unclear"]
    assert (~clear).sum() <= 0.02 * len(q)
    assert fit["reject"][clear].sum() >= 5 and (~fit["reject"])[clear].sum() >= 1000
    assert np.array_equal(rs[clear, 3] < 0, fit["reject"][clear])
    assert (rs[clear & fit["reject"]] == (0.0, 0.0, 0.0, -1.0)).all()
    m = clear & ~fit["reject"]
    rn = (np.abs(rs[m, :3] - fit["planes"][m, :3]).max(axis=1) / fit["bar_n"][m]).max()
    rd = (np.abs(rs[m, 3] - fit["planes"][m, 3]) / fit["bar_d"][m]).max()
    assert rn <= 1 and rd <= 1
    ks = orf.KdSumsRef(pose, q, rs)
    part = orf.wg_partials(orf.kd_accum_restate(pose, q, rs))
    worst = 0.0
    for b in range(len(part)):
        worst = max(worst, orf.check_sums(part[b], ks.sums(range(256 * b, min(len(q), 256 * b + 256)))))
    worst = max(worst, orf.check_sums(orf.reduce_partials(part), ks.sums(range(len(q)))))
    print("general %s: %d unclear, %d rejected; worst ratio to bar: normal %.3g, distance %.3g, sums %.3g" % (general, (~clear).sum(), fit["reject"].sum(), rn, rd, worst))


def test_reduction_order_is_the_documented_one():
    """reduce_partials against the same sum written with index arithmetic only, for nb below, at and above a multiple of 7"""
    rng = np.random.default_rng(3)
    for nb in (1, 2, 7, 8, 15):
        p = rng.normal(0, 1, (nb, 34)) * 10.0 ** rng.integers(-8, 8, (nb, 34))
        want = np.zeros(34)
        for c in range(34):
            groups = []
            for g in range(7):
                s = 0.0
                for r in range(g, nb, 7):
                    s += p[r, c]
                groups.append(s)
            s = groups[0]
            for g in range(1, 7):
                s += groups[g]
            want[c] = s
        assert np.array_equal(orf.reduce_partials(p), want)
