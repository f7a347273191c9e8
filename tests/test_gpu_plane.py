"""The device against the references and counted bars of tests/plane_ref.py (MI355X): plane_update_dev alone through
vba_debug_plane_update, k_var_init through vba_scan_var_init, k_scan_to_soa_pvec_update and the Bf_var terms of the insert through
vba_map_pvec_update_cut_voxel with one point per voxel, and the real marginalisation's own dumps (the plane data a leaf holds follow
from the sums, eigen-pairs and cov_add the same dump shows).  Every case prints its worst ratio to bar; nothing depends on the printed
values.  tests/test_plane_cpu.py holds the same checks for f64 restatements and for the C++ oracle."""
import numpy as np
import pytest

import odom_ref as orf
import plane_ref as prf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


def _ctx(capi, voxel_size=0.5):
    o = capi.default_options(); o.win_size = 4; o.voxel_size = voxel_size
    return capi.Context(o)


@pytest.fixture(scope="module")
def ctx(capi):
    return _ctx(capi)


# ------------------------------------------------------------------------------------------------ a. plane_update_dev alone
@pytest.fixture(scope="module")
def pcorpus():
    co = prf.plane_corpus()
    co["ref"] = prf.plane_ref_of_rows(co["rows"])
    return co


@pytest.fixture(scope="module")
def singles(ctx, pcorpus):
    """every leaf of the corpus in a call of its own (n = 1)"""
    return np.concatenate([ctx.debug_plane_update(r) for r in pcorpus["rows"]])


def test_plane_update_every_leaf_singly(pcorpus, singles):
    bad, ratio = prf.judge(singles, pcorpus["ref"])
    print("n = 1 x %d: worst ratio to bar per class %s" % (len(singles), {c: round(float(ratio[pcorpus["cls"] == c].max()), 3) for c in prf.PLANE_CLASSES}))
    prf.check(singles, pcorpus["ref"], "single leaf", names=pcorpus["cls"])
    assert np.array_equal(singles[:, 3:7], pcorpus["ref"].f64()[:, 3:7])          # normal = U column 0, radius = (double)(float)ev2


@pytest.mark.parametrize("n", prf.PREFIXES)
def test_plane_update_prefixes(ctx, pcorpus, singles, n):
    rows = pcorpus["rows"][:n].copy()
    out = ctx.debug_plane_update(rows)
    assert np.array_equal(rows, pcorpus["rows"][:n])                             # the inputs come back unchanged
    worst = prf.check(out, prf.plane_ref_of_rows(rows), "prefix %d" % n, names=pcorpus["cls"])
    assert np.array_equal(out, singles[:n])                                      # no dependence on n
    print("n = %d: worst ratio to bar %.3g" % (n, worst))


def test_plane_update_does_not_depend_on_position(ctx, pcorpus, singles):
    perm = np.random.default_rng(5).permutation(len(singles))
    assert np.array_equal(ctx.debug_plane_update(pcorpus["rows"][perm]), singles[perm])
    assert np.array_equal(ctx.debug_plane_update(pcorpus["rows"][::-1]), singles[::-1])


def test_plane_update_refusals(capi, ctx, pcorpus):
    import ctypes as C
    rows = np.ascontiguousarray(pcorpus["rows"][:2]); out = np.full((2, 43), np.nan)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                          # noqa: E731
    for n, a, b in ((0, rows, out), (-1, rows, out), ((1 << 20) + 1, rows, out), (2, None, out), (2, rows, None)):
        st = ctx.lib.vba_debug_plane_update(ctx.h, C.c_int(n), None if a is None else p(a), None if b is None else p(b))
        assert st == capi.ERR_BAD_ARG and np.isnan(out).all()


@pytest.mark.parametrize("col", [0, 1, 2])
def test_plane_update_eigenvector_sign(ctx, pcorpus, singles, col):
    """u_0 -> -u_0: the normal block and the centre block bit-identical, the cross blocks and the normal exactly negated;
    u_1 or u_2 flipped: everything bit-identical"""
    rows = pcorpus["rows"].copy()
    rows[:, [13 + col, 16 + col, 19 + col]] *= -1.0
    out = ctx.debug_plane_update(rows)
    worst = prf.check(out, prf.plane_ref_of_rows(rows), "flipped u_%d" % col, names=pcorpus["cls"])
    want = singles.copy()
    if col == 0:
        want[:, 3:6] *= -1.0
        pv = want[:, 7:].reshape(-1, 6, 6)
        pv[:, :3, 3:] *= -1.0; pv[:, 3:, :3] *= -1.0
    assert np.array_equal(out, want)
    print("u_%d flipped: worst ratio to bar %.3g" % (col, worst))


# ------------------------------------------------------------------------------------------------ b. var_init
@pytest.fixture(scope="module")
def points():
    return prf.point_corpus()


EXTS = {"identity": prf.IDENT_EXT, "general": prf.general_ext()}


@pytest.mark.parametrize("name", list(EXTS))
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_var_init(ctx, points, n, name):
    p = points["pts"][:n].copy()
    ref = prf.var_init_ref(p, EXTS[name], prf.DEPT_ERR, prf.BEAM_ERR)
    keep = np.nonzero(~ref["unclear"])[0]
    assert n - len(keep) <= 0.01 * n
    pnt, var = ctx.var_init(p, EXTS[name], prf.DEPT_ERR, prf.BEAM_ERR)
    assert np.array_equal(p, points["pts"][:n])
    rp = prf.check(pnt[keep], ref["pnt"].rows(keep), "points", names=points["cls"][keep])
    rv = prf.check(var[keep], ref["var"].rows(keep), "variances", names=points["cls"][keep])
    print("n = %d, %s extrinsic: %d unclear; worst ratio to bar, points %.3g, variances %.3g" % (n, name, n - len(keep), rp, rv))


# ------------------------------------------------------------------------------------------------ b. pvec_update + Bf_var
def _pose_cases():
    R, t = orf.general_pose()
    t = t - 0.75                                                        # the voxel of t itself is free of lattice sites (origin case)
    cov = orf.full_cov()
    diag = np.eye(15) * 1e-4
    norot = cov.copy(); norot[:3, :] = 0.0; norot[:, :3] = 0.0
    return {"general": (R, t, cov, False), "identity": (np.eye(3), np.zeros(3), diag, False), "zero_rot_var": (R, t, norot, False),
            "origin": (R, t, cov, True)}


@pytest.mark.parametrize("name,n", [("general", 1), ("general", 256), ("general", 257), ("identity", 257), ("zero_rot_var", 257), ("origin", 65)])
def test_pvec_update_one_point_per_voxel(capi, name, n):
    """every leaf holds ONE point, so its cov_add row is that point's Bf_var: entries 39..44 are the upper triangle of var_world"""
    R, t, cov, origin = _pose_cases()[name]
    vs = 0.5
    pts, keys = prf.lattice_points(n, vs, R, t, origin=origin)
    var = np.ascontiguousarray(prf.rand_spd(n, np.random.default_rng(7)).reshape(-1, 9))
    c = _ctx(capi, vs)
    c.pvec_update_cut_voxel(0, pts, var, np.concatenate([R.ravel(), t]), cov, multi=False)
    assert c.num_roots() == n
    lv, pv, ca = prf.device_dump(c)
    assert len(lv) == n and (lv[:, 5] == 1).all() and (lv[:, 3] == 0).all()
    row = {tuple(int(v) for v in r[:3]): i for i, r in enumerate(lv)}
    order = [row[tuple(int(v) for v in k)] for k in keys]                # leaf of point i
    got = ca[order]
    ref = prf.pvec_update_ref(pts, var, R, t, cov[:3, :3], cov[3:6, 3:6])
    rv = prf.check(got[:, 39:45], ref["var_world"].take([0, 1, 2, 4, 5, 8]), "var_world")
    rb = prf.check(got, ref["bf"], "Bf_var")
    # the world point is the leaf's cluster sum v (N = 1)
    rw = prf.check(lv[order][:, 28:31], ref["pw"], "pw")
    if origin:
        assert (pts[0] == 0).all()                                       # hat(p) = 0: the rotation-covariance term has shadow 0 there
    print("%s, n = %d: worst ratio to bar, var_world %.3g, Bf_var %.3g, pw %.3g" % (name, n, rv, rb, rw))


# ------------------------------------------------------------------------------------------------ c. in situ
def test_marginalisation_hands_plane_update_the_right_inputs(capi):
    from voxel_slam_amd import synth
    wl, s, poses, var = prf.insitu_workload(synth)
    c = capi.Context(capi.options_from_workload(wl))
    first, second = prf.insitu_session(
        wl, s, poses, var, lambda i, p, x, v: c.cut_voxel(i, p, x, var=v, multi=True), lambda W, x: c.recut(W, x, multi=True),
        c.evaluate_only_residual, lambda W, x: c.margi(W, x), c.slide, lambda: prf.device_dump(c))
    w1 = prf.written(first)
    assert len(w1) > 20
    r1 = prf.dump_consistency(first, w1, "first marginalisation")
    for k in w1:
        assert np.array_equal(first[k][0][35:38], first[k][0][13:22].reshape(3, 3)[:, 0]), k
        assert first[k][0][38] == float(np.float32(first[k][0][12])), k
    fire, keep = prf.predict_second_pass(first, second, wl.max_points)
    assert len(fire) > 0 and len(keep) > 0
    r2 = prf.dump_consistency(second, fire, "second marginalisation")
    for k in keep:
        assert np.array_equal(first[k][0][32:39], second[k][0][32:39]) and np.array_equal(first[k][1], second[k][1]), k
    print("first pass: %d planes, worst ratio to bar %.3g; second pass: %d firing, worst ratio %.3g, %d kept bit for bit" % (len(w1), r1, len(fire), r2, len(keep)))
