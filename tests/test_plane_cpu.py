"""The references of tests/plane_ref.py for plane_update, var_init and pvec_update + Bf_var, on the host alone: the counted rounding
numbers, the double-double code against mpmath, plain-f64 restatements of the three device routines inside every bar (plane_update
also with one rounding per contractible multiply-add), the C++ oracle's own marginalisation dumps inside the bars of the
dump-consistency check that tests/test_gpu_plane.py applies to the device, the caps, and the teeth: each listed defect of a restatement
exceeds a bar, and a 1e-4 error of the centre block alone, which the comparison max|G - O| <= 1e-5 max|O| lets through, does not pass.
Worst ratios to bar are printed; nothing depends on the printed values."""
import numpy as np
import pytest

import odom_ref as orf
import plane_ref as prf


# ------------------------------------------------------------------------------------------------ plane_update
@pytest.fixture(scope="module")
def pcorpus():
    co = prf.plane_corpus()
    co["ref"] = prf.plane_ref_of_rows(co["rows"])
    return co


def _restate_all(co, fused=False, defect=None, lower=None):
    return np.array([prf.plane_restate(r[:10], r[10:13], r[13:22], prf.cov9_of(r[22:], lower), fused, defect) for r in co["rows"]])


def test_plane_corpus_classes_and_counts(pcorpus):
    co, ref = pcorpus, pcorpus["ref"]
    assert len(co["rows"]) == prf.N_LEAVES == 257
    for c in prf.PLANE_CLASSES:
        assert (co["cls"] == c).sum() >= 32, c
        assert (co["cls"][:63] == c).sum() >= 7, c                    # every tested prefix holds every class
    add, ev, Um, cov = prf.split67(co["rows"])
    gap = (ev[:, 1] - ev[:, 0]) / ev[:, 2]
    for c, g in (("line3", 1e-3), ("line6", 1e-6), ("line9", 1e-9)):
        assert np.allclose(gap[co["cls"] == c], g, rtol=1e-3), (c, gap[co["cls"] == c])
    assert (add[co["cls"] == "bigN", 9] == 1e5).all() and add[:, 9].min() == 6
    assert (ev[co["cls"] == "neg", 0] == -1e-18).all()
    assert (np.abs(add[co["cls"] == "far", 6:9] / add[co["cls"] == "far", 9:10]).max(axis=1) > 400).all()
    ax = co["cls"] == "axis"
    assert (np.isin(np.abs(Um[ax]), (0.0, 1.0))).all() and ((add[ax, 6:9] == 0).sum(axis=1) == 2).all()
    assert ((ref.m.T[ax] == 0).sum(axis=1) >= 10).all()               # exact zeros expected of the outputs
    assert (np.linalg.norm(add[co["cls"] == "wall", 6:9] / add[co["cls"] == "wall", 9:10], axis=1) >= 5).all()
    # the counted roundings of the module docstring are what the code keeps
    k = ref.k
    assert list(k[:3]) == [prf.K_CENTRE] * 3 and list(k[3:7]) == [0] * 4
    pv = k[7:].reshape(6, 6)
    assert (pv[:3, :3] == prf.K_NN).all() and (pv[:3, 3:] == prf.K_CROSS).all() and (pv[3:, :3] == prf.K_CROSS).all() and (pv[3:, 3:] == prf.K_CC).all()
    assert (ref.k_uc, ref.k_jc) == (13, 17)


def test_plane_double_double_against_mpmath(pcorpus):
    """the same formula over mpmath numbers at 200 bits, on two leaves of every class"""
    mpmath = pytest.importorskip("mpmath")
    idx = np.concatenate([np.arange(8), np.arange(248, 256)])
    rows = pcorpus["rows"][idx]
    with mpmath.workprec(200):
        a = prf.plane_ref_of_rows(rows, T=prf.MP)
        b = prf.plane_ref_of_rows(rows)
        err = a.v.err_to(b.v.f64())
        assert np.array_equal(a.k, b.k) and np.allclose(a.m, b.m, rtol=1e-12)
        live = b.m > 0
        worst = (err[live] / b.m[live]).max()
        assert worst <= 4 * prf.U
        assert (err[~live] == 0).all()
    print("plane_update, double-double vs mpmath: f64 of the value within %.3g u of the shadow" % (worst / prf.U))


@pytest.mark.parametrize("fused", [False, True])
def test_plane_restatement_inside_every_bar(pcorpus, fused):
    """plane_update_dev restated from the kernel text: unfused, and with every contractible multiply-add rounded once (the unit is
    compiled with contraction on)"""
    dev = _restate_all(pcorpus, fused)
    bad, ratio = prf.judge(dev, pcorpus["ref"])
    print("fused %s: worst ratio to bar per class %s" % (fused, {c: round(float(ratio[pcorpus["cls"] == c].max()), 3) for c in prf.PLANE_CLASSES}))
    prf.check(dev, pcorpus["ref"], "restatement", names=pcorpus["cls"])
    assert np.array_equal(dev[:, 3:7], pcorpus["ref"].f64()[:, 3:7])     # normal and radius: bit-exact


@pytest.mark.parametrize("defect", prf.PLANE_DEFECTS)
def test_plane_teeth(pcorpus, defect):
    lower = 1.001 if defect == "lower" else None                        # the asymmetric probe: the strict lower triangle scaled
    assert not prf.judge(_restate_all(pcorpus, lower=lower), pcorpus["ref"])[0].any()
    bad, _ = prf.judge(_restate_all(pcorpus, defect=defect, lower=lower), pcorpus["ref"])
    caught = {c: int(bad[pcorpus["cls"] == c].any(axis=1).sum()) for c in prf.PLANE_CLASSES}
    print("%s -> leaves outside a bar, per class: %s" % (defect, caught))
    assert bad.any()
    assert caught["wall"] > 0                                           # the class every formula defect shows in (a large centre, a general U)


# ------------------------------------------------------------------------------------------------ the C++ oracle, in situ
@pytest.fixture(scope="module")
def oracle_session(oracle):
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth
    wl, s, poses, var = prf.insitu_workload(synth)
    om = oracle.VoxelMap(wl.win_size, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, 5)
    of = oracle.Factor(wl.win_size)
    first, second = prf.insitu_session(
        wl, s, poses, var, lambda i, p, x, v: om.cut_voxel(i, p, x, var=v, multi=True), lambda W, x: om.recut(W, x, of, multi=True),
        of.evaluate_only_residual, lambda W, x: om.margi(W, x, of), om.slide, lambda: (om.dump_leaves(), om.dump_plane_var(), om.dump_cov_add()))
    return wl, first, second


def test_oracle_dumps_are_consistent(oracle_session):
    """what test_gpu_plane.py asks of the device's dumps holds for the oracle's: the check is sound before a GPU sees it"""
    wl, first, second = oracle_session
    w1 = prf.written(first)
    assert len(w1) > 20
    r1 = prf.dump_consistency(first, w1, "first marginalisation")
    for k in w1:
        assert np.array_equal(first[k][0][35:38], first[k][0][13:22].reshape(3, 3)[:, 0])
        assert first[k][0][38] == float(np.float32(first[k][0][12]))
    fire, keep = prf.predict_second_pass(first, second, wl.max_points)
    assert len(fire) > 0 and len(keep) > 0
    r2 = prf.dump_consistency(second, fire, "second marginalisation")
    for k in keep:
        assert np.array_equal(first[k][0][32:39], second[k][0][32:39]) and np.array_equal(first[k][1], second[k][1]), k
    print("oracle: %d planes after the first pass, worst ratio %.3g; second pass %d firing (worst %.3g), %d kept" % (len(w1), r1, len(fire), r2, len(keep)))


def test_centre_block_error_is_caught_where_the_matrix_maximum_is_not(oracle_session):
    """1e-4 relative on the centre block (3:6, 3:6) alone: outside the bars on every leaf, inside max|G - O| <= 1e-5 max|O| on most
    (the maximum of plane_var lies in the normal block)"""
    wl, first, second = oracle_session
    keys = prf.written(first)
    got, ref = prf.dump_pairs(first, keys)
    assert not prf.judge(got, ref)[0].any()
    O = got[:, 7:].reshape(-1, 6, 6)
    G = O.copy(); G[:, 3:, 3:] *= 1.0 + 1e-4
    old_pass = np.abs(G - O).max(axis=(1, 2)) <= 1e-5 * np.abs(O).max(axis=(1, 2))
    bad = prf.judge(np.concatenate([got[:, :7], G.reshape(-1, 36)], axis=1), ref)[0]
    assert not bad[:, :7].any() and not bad[:, 7:].reshape(-1, 6, 6)[:, :3, :].any()       # (only the injected block is flagged)
    caught = bad.any(axis=1)
    print("centre block * (1 + 1e-4): outside the bars on %d of %d leaves; inside the 1e-5 * max comparison on %d" % (caught.sum(), len(keys), old_pass.sum()))
    assert caught.all() and old_pass.sum() > len(keys) // 2


# ------------------------------------------------------------------------------------------------ var_init
@pytest.fixture(scope="module")
def points():
    return prf.point_corpus()


EXTS = {"identity": prf.IDENT_EXT, "general": prf.general_ext()}


def test_point_corpus_covers_the_edges(points):
    p, cls = points["pts"], points["cls"]
    r = np.linalg.norm(p, axis=1)
    assert r.min() < 0.5 and r.max() > 60 and r.min() >= 0.3 and r.max() <= 100
    assert len({tuple(np.sign(q)) for q in p[cls == "random"]}) == 8
    for c in prf.POINT_CLASSES:
        assert (cls[:255] == c).sum() >= 1, c
    assert (p[cls == "z0", 2] == 0).all() and (cls == "z0").sum() == 8
    for c, f in (("z1e-12", 1e-12), ("z1e-9", 1e-9), ("z1e-6", 1e-6)):
        assert np.allclose(np.abs(p[cls == c, 2]) / r[cls == c], f, rtol=1e-6)
    assert (p[cls == "x=-y", 0] == -p[cls == "x=-y", 1]).all()
    assert ((p[cls == "axis"] != 0).sum(axis=1) == 1).all() and (cls == "axis").sum() == 6
    for name, ext in EXTS.items():
        ref = prf.var_init_ref(p, ext, prf.DEPT_ERR, prf.BEAM_ERR)
        print(name, "unclear: %d of %d" % (ref["unclear"].sum(), len(p)))
        assert ref["unclear"].sum() <= 0.01 * len(p)
        assert ref["unclear"][cls == "midpoint"].all()                  # the constructed one is found
        assert list(ref["pnt"].k) == [0 if name == "identity" else prf.K_PNT] * 3
        assert list(ref["var"].k) == [ref["k_body"] if name == "identity" else prf.K_VAR] * 9 and ref["k_body"] == 161


@pytest.mark.parametrize("name", list(EXTS))
def test_var_init_restatement_inside_every_bar(points, name):
    ref = prf.var_init_ref(points["pts"], EXTS[name], prf.DEPT_ERR, prf.BEAM_ERR)
    keep = ~ref["unclear"]
    pnt, var = prf.var_init_restate(points["pts"], EXTS[name], prf.DEPT_ERR, prf.BEAM_ERR)
    bp, rp = prf.judge(pnt, ref["pnt"]); bv, rv = prf.judge(var, ref["var"])
    assert not bp[keep].any() and not bv[keep].any()
    print("%s: worst ratio to bar, points %.3g, variances %.3g" % (name, rp[keep].max(), rv[keep].max()))


def test_var_init_sqrt_and_sin_against_mpmath(points):
    mpmath = pytest.importorskip("mpmath")
    p = points["pts"][:48]
    with mpmath.workprec(200):
        a = prf.var_init_ref(p, EXTS["general"], prf.DEPT_ERR, prf.BEAM_ERR, T=prf.MP)
        b = prf.var_init_ref(p, EXTS["general"], prf.DEPT_ERR, prf.BEAM_ERR)
        err = a["var"].v.err_to(b["var"].v.f64())
        assert (err <= 4 * prf.U * b["var"].m).all() and np.array_equal(a["unclear"], b["unclear"])
        s = prf._sin_exact(float(np.float32(prf.BEAM_ERR)) * prf.DEG2RAD)
        assert abs(mpmath.sin(mpmath.mpf(float(np.float32(prf.BEAM_ERR)) * prf.DEG2RAD)) - mpmath.mpf(s.numerator) / s.denominator) < mpmath.mpf(10) ** -40


@pytest.mark.parametrize("defect", prf.VAR_DEFECTS)
def test_var_init_teeth(points, defect):
    ref = prf.var_init_ref(points["pts"], EXTS["general"], prf.DEPT_ERR, prf.BEAM_ERR)
    keep = ~ref["unclear"]
    pnt, var = prf.var_init_restate(points["pts"], EXTS["general"], prf.DEPT_ERR, prf.BEAM_ERR, defect)
    bad = prf.judge(var, ref["var"])[0][keep]
    print("%s -> points outside a bar, per class: %s" % (defect, {c: int(bad[points["cls"][keep] == c].any(axis=1).sum()) for c in prf.POINT_CLASSES}))
    assert bad.any()


# ------------------------------------------------------------------------------------------------ pvec_update and Bf_var
def _pvec_cases():
    R, t = orf.general_pose()
    cov = orf.full_cov()
    return {"identity": (np.eye(3), np.zeros(3), cov[:3, :3], cov[3:6, 3:6]), "general": (R, t, cov[:3, :3], cov[3:6, 3:6]),
            "zero_rot_var": (R, t, np.zeros((3, 3)), cov[3:6, 3:6])}


@pytest.mark.parametrize("name", ["identity", "general", "zero_rot_var"])
def test_pvec_restatement_inside_every_bar(points, name):
    R, t, rv, tv = _pvec_cases()[name]
    p = np.concatenate([np.zeros((1, 3)), points["pts"][:256]])         # the body origin first: hat(p) = 0
    var = prf.rand_spd(len(p), np.random.default_rng(3)).reshape(-1, 9)
    ref = prf.pvec_update_ref(p, var, R, t, rv, tv)
    vw, pw, bf = prf.pvec_restate(p, var, R, t, rv, tv)
    out = [prf.check(a, ref[k], k) for a, k in ((vw, "var_world"), (pw, "pw"), (bf, "bf"))]
    if name == "general":
        assert (ref["var_world"].k.max(), ref["pw"].k.max(), ref["bf"].k.max()) == (prf.K_VW, prf.K_PW, prf.K_BF)
    if name == "identity":
        assert np.array_equal(pw, p) and ref["pw"].k.max() == 0
    if name == "zero_rot_var":
        assert np.array_equal(vw[0], (prf.pvec_restate(p[:1], var[:1], R, t, rv, tv)[0])[0])
    # the origin: the rotation-covariance term has shadow 0 there
    assert (prf.pvec_update_ref(p[:1], np.zeros((1, 9)), R, t, rv, np.zeros((3, 3)))["var_world"].m == 0).all()
    # Bf_var of GIVEN var_world and pw (what the device test compares the other 39 entries with, next to the tracked ones)
    given = prf.bf_var_ref(vw, pw)
    prf.check(bf, given, "bf of the restatement's own var_world")
    print("%s: worst ratio to bar, var_world %.3g, pw %.3g, Bf_var %.3g" % ((name,) + tuple(out)))


@pytest.mark.parametrize("defect", prf.PVEC_DEFECTS)
def test_pvec_teeth(points, defect):
    R, t, rv, tv = _pvec_cases()["general"]
    p = points["pts"][:64]
    var = prf.rand_spd(len(p), np.random.default_rng(3)).reshape(-1, 9)
    ref = prf.pvec_update_ref(p, var, R, t, rv, tv)
    vw, pw, bf = prf.pvec_restate(p, var, R, t, rv, tv, defect)
    bad = prf.judge(vw, ref["var_world"])[0]
    print("%s -> %d of %d points outside a bar" % (defect, bad.any(axis=1).sum(), len(p)))
    assert bad.any() and prf.judge(bf, ref["bf"])[0].any()
