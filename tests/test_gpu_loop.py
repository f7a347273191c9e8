"""The device-resident loop-closure map rebuild (vba_loop_map_*, vba_loop_update) on the MI355X against the CPU
oracle driven with the reference's call sequence (tests/loop_oracle.py, tests/host/loop_host.cpp): map_loop from the keyframe store
(VS:2601-2625, five cumulative cut_voxel calls), loop_update (VS:1262-1363) with the covariances of the fixed points, the window
re-inserted from the outgoing map's own scan ring, the session continuing afterwards, residency, refusals and determinism.
Structure and the f64 sums pcr_add / cov_add are compared BIT FOR BIT, as everywhere else in the map; plane
eigenvalues, refined planes and poses at the bars of tests/test_gpu_map.py / tests/test_gpu_fullsize.py.
tests/test_loop_cpu.py shows on the oracle alone that this scene makes cov_add depend on the fixed covariances."""
import numpy as np
import pytest

import loop_oracle as lo

pytestmark = pytest.mark.gpu

VS10 = 0.5 / 10
EXT = np.concatenate([np.eye(3).ravel(), np.zeros(3)])


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


@pytest.fixture(scope="module")
def synth():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth as s
    return s


@pytest.fixture(scope="module")
def ses(synth):
    return lo.make_session(synth, n_kf=8, k_bl=3, W=4, extra=3, n_pts=20000)


def _opts(capi, wl, **kw):
    o = capi.options_from_workload(wl)
    o.device = 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _omap(oracle, wl):
    return oracle.VoxelMap(wl.win_size, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, 5)


def _sorted(d, extra=None):
    order = np.lexsort((d[:, 4], d[:, 3], d[:, 2], d[:, 1], d[:, 0]))
    return d[order], (extra[order] if extra is not None else None), order


def _defined(dump, pv):
    """key-sorted leaf records reduced to the fields that are defined for every leaf (key, layer, path, N_add, N_fix, is_plane, isexist,
    pcr_add), the plane eigen-pairs where is_plane, and cov_add"""
    g, _, _ = _sorted(dump)
    p, _, _ = _sorted(pv)
    eig = np.where(g[:, 7:8] != 0, g[:, 10:22], 0.0)
    return np.concatenate([g[:, :9], g[:, 22:32], eig], 1), p[:, 41:]


def _fill_store(store, ses, n_kf):
    for i in range(n_kf):
        store.build([ses["points"][i]], ses["poses"][i][None, :], VS10, id=i, jour=0.5 * i, vars=[ses["vars"][i]])


def _store_host(store):
    n = store.size()
    rd = [store.read(k) for k in range(n)]
    return [r[0] for r in rd], [r[1] for r in rd], [store.get(k)["x0"] for k in range(n)]


def _state(pose):
    s = np.zeros(25); s[1:10] = pose[:9]; s[10:13] = pose[9:]
    return s


class Side:
    """One device context driven through the local-mapping history that precedes a loop closure.  `inserted[k]` = the covariance of
    scan k exactly as the map received it: what buf_lba2loop / pvec_buf hold in the reference."""

    def __init__(self, capi, oracle, ses, fused, **optkw):
        self.capi, self.oracle, self.ses, self.fused = capi, oracle, ses, fused
        self.wl, self.W = ses["wl"], ses["W"]
        self.ctx = capi.Context(_opts(capi, self.wl, **optkw))
        self.inserted = {}
        self.window = []          # scan indices in frame order
        self.bl = []              # scans marginalised so far (buf_lba2loop)

    def scan_var(self, k, pose):
        """the world covariance pvec_update gives scan k at `pose` (oracle restatement), or the body covariance as it is"""
        if self.fused:
            return self.oracle.pvec_update(self.ses["points"][k], self.ses["vars"][k], _state(pose), self.ses["cov"])[0]
        return self.ses["vars"][k]

    def insert(self, slot, k, pose):
        self.inserted[k] = self.scan_var(k, pose)
        if self.fused:
            self.ctx.pvec_update_cut_voxel(slot, self.ses["points"][k], self.ses["vars"][k], pose, self.ses["cov"], multi=True)
        else:
            self.ctx.cut_voxel(slot, self.ses["points"][k], pose, var=self.ses["vars"][k], multi=True)

    def poses(self):
        return np.ascontiguousarray(self.ses["poses"][self.window])

    def history(self, win_count):
        """fill the window, then slide it k_bl times (margi, slide, insert, multi_recut); win_count = W - 1 marginalises once more"""
        W, ses = self.W, self.ses
        base = ses["n_kf"]
        for j in range(W):
            self.insert(j, base + j, ses["poses"][base + j])
            self.window.append(base + j)
        self.ctx.recut(W, self.poses(), multi=True)
        nxt = base + W
        for step in range(ses["k_bl"] + (1 if win_count < W else 0)):
            self.ctx.evaluate_only_residual(self.poses())
            self.ctx.margi(len(self.window), self.poses(), jour=float(step))
            self.ctx.slide(1)
            self.bl.append(self.window.pop(0))
            if step < ses["k_bl"]:
                self.insert(W - 1, nxt, ses["poses"][nxt])
                self.window.append(nxt)
                nxt += 1
                self.ctx.recut(len(self.window), self.poses(), multi=True)
        assert len(self.window) == win_count
        self.next_scan = nxt

    def close(self):
        self.ctx.close()


def _loop_inputs(side):
    """everything loop_update is given, poses already moved by dx"""
    ses, dx = side.ses, side.ses["dx"]
    return dict(bl_scans=[ses["points"][k] for k in side.bl], bl_vars=[side.inserted[k] for k in side.bl],
                bl_poses=np.array([lo.move_pose(ses["poses"][k], dx) for k in side.bl]),
                win_scans=[ses["points"][k] for k in side.window], win_vars=[side.inserted[k] for k in side.window],
                win_poses=np.array([lo.move_pose(ses["poses"][k], dx) for k in side.window]))


def _close_loop(side, store, lm, resident=True, n_kf=5):
    """set_poses with the correction, map_loop, loop_update -> (inputs, factor count)"""
    dx = side.ses["dx"]
    store.set_poses(0, np.array([lo.move_pose(side.ses["poses"][i], dx) for i in range(store.size())]))
    lm.build(store, 5, True)
    inp = _loop_inputs(side)
    nf = side.ctx.loop_update(lm, inp["win_poses"], inp["bl_scans"], inp["bl_poses"], inp["bl_vars"],
                              win_scans=None if resident else inp["win_scans"], win_vars=None if resident else inp["win_vars"], dx12=dx)
    return inp, nf


def _oracle_loop(oracle, wl, store, inp):
    om = _omap(oracle, wl)
    clouds, diags, kposes = _store_host(store)
    lo.replay_build(om, clouds, diags, kposes, 5, True)
    of = lo.replay_update(om, oracle, inp["bl_scans"], inp["bl_vars"], inp["bl_poses"], inp["win_scans"], inp["win_vars"], inp["win_poses"])
    return om, of


def _assert_map_equals_oracle(ctx_dump, ctx_pv, om, check_plane=True):
    from test_gpu_fullsize import _assert_structure_equal
    g, _, _ = _sorted(ctx_dump); gpv, _, _ = _sorted(ctx_pv)
    o, oca, _ = _sorted(om.dump_leaves(), om.dump_cov_add())
    nplane = _assert_structure_equal(g, o, check_plane=check_plane)       # leaf set, N_add / N_fix, isexist, pcr_add bit for bit, planes
    assert np.array_equal(gpv[:, :5], o[:, :5])
    bad = (gpv[:, 41:] != oca).any(1)
    print("leaves %d, planes %d, cov_add rows that differ %d" % (len(o), nplane, int(bad.sum())))
    assert not bad.any(), "cov_add is not bit-identical on %d of %d leaves" % (int(bad.sum()), len(o))
    return g, o, oca


# ---------------------------------------------------------------------------------------------------------------- 1. map_loop
@pytest.mark.parametrize("n_kf", [3, 8])
@pytest.mark.parametrize("cumulative", [True, False])
def test_loop_map_build_against_oracle(capi, oracle, ses, cumulative, n_kf):
    """vba_loop_map_build against the oracle replay with the reference's call sequence (one cut_voxel call per keyframe of the tail
    on the cumulative pvec_tem, NOT the concatenation): same roots, N_fix, pcr_add bit for bit.  (The dump carries N_fix and pcr_add;
    in a map that holds only fixed points pcr_fix is the same chain of additions as pcr_add.)  exist flags as VS:2612."""
    wl = ses["wl"]
    ctx = capi.Context(_opts(capi, wl))
    store = ctx.kf_store()
    _fill_store(store, ses, n_kf)
    store.set_poses(0, np.array([lo.move_pose(ses["poses"][i], ses["dx"]) for i in range(n_kf)]))
    store.set_history(n_kf)                                        # exist = 1 everywhere, so that the build's clearing shows
    lm = ctx.loop_map()
    n = lm.build(store, 5, cumulative)
    clouds, diags, kposes = _store_host(store)
    om = _omap(oracle, wl)
    n2 = lo.replay_build(om, clouds, diags, kposes, 5, cumulative)
    cnt = lo.expansion_counts(n_kf, 5, cumulative)
    print("keyframes %d, cumulative %d: %d points inserted, %d roots" % (n_kf, cumulative, n, lm.num_roots()))
    assert n == n2 == int(sum(c * len(p) for c, p in zip(cnt, clouds))) > 0
    assert lm.num_roots() == om.num_roots() > 100
    g, o, _ = _assert_map_equals_oracle(lm.dump_leaves(), lm.dump_plane_var(), om, check_plane=False)
    assert (g[:, 3] == 0).all() and (g[:, 5] == g[:, 6]).all() and g[:, 6].sum() == n      # every root a leaf, only fixed points
    assert [store.get(k)["exist"] for k in range(n_kf)] == [0 if k >= n_kf - 5 else 1 for k in range(n_kf)]
    # a second build resets the map first: same result
    assert lm.build(store, 5, cumulative) == n
    _assert_map_equals_oracle(lm.dump_leaves(), lm.dump_plane_var(), om, check_plane=False)
    lm.close(); store.close(); ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 2. loop_update
@pytest.mark.parametrize("win_count", [4, 3])
def test_loop_update_against_oracle(capi, oracle, ses, win_count):
    """VS:1262-1363 after a local-mapping history (window filled, slid k_bl times with marginalisation: the ring's frame order is
    rotated): map_loop adopted, the marginalised scans inserted as fixed points with their full covariances, the window re-inserted
    from the outgoing map's ring, recut.  Leaf set, plane flags, N_add / N_fix equal; pcr_add and cov_add bit for bit; plane
    eigenvalues at 1e-12 of the second moments; factor count equal.  (centre / normal / plane_var are written by the marginalisation:
    compared in test_session_goes_on.)  win_count = 3 takes the loop map from a second context of the device."""
    wl = ses["wl"]
    side = Side(capi, oracle, ses, fused=True)
    side.history(win_count)
    store = side.ctx.kf_store()
    _fill_store(store, ses, 8)
    other = capi.Context(_opts(capi, wl)) if win_count < ses["W"] else None
    lm = (other or side.ctx).loop_map()
    inp, nf = _close_loop(side, store, lm)
    assert len(inp["bl_scans"]) >= 3 and len(inp["win_scans"]) == win_count
    om, of = _oracle_loop(oracle, wl, store, inp)
    g, o, oca = _assert_map_equals_oracle(side.ctx.dump_leaves(), side.ctx.dump_plane_var(), om)
    assert nf == side.ctx.size() == of.size() > 50
    split_with_fix = (o[:, 3] > 0) & (o[:, 6] > 0)
    assert split_with_fix.sum() > 50 and (np.abs(oca[split_with_fix]).max(1) > 0).all()
    assert side.ctx.num_roots() == om.num_roots() and side.ctx.num_slide_roots() == om.num_slide_roots()
    # the outgoing map is empty and belongs to the loop map now
    assert lm.num_roots() == 0 and len(lm.dump_leaves()) == 0
    # the factor stores are equivalent
    H, gg, r = side.ctx.acc_evaluate2(_pad(inp["win_poses"], ses["W"]))
    H2, g2, r2 = of.acc_evaluate2(_pad(inp["win_poses"], ses["W"]))
    assert abs(r - r2) < 1e-11 * abs(r2)
    assert np.abs(H - H2).max() < 1e-9 * np.abs(H2).max() and np.abs(gg - g2).max() < 1e-9 * np.abs(g2).max()
    lm.close(); store.close(); side.close()
    if other is not None:
        other.close()


def _pad(poses, W):
    out = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (W, 1))
    out[:len(poses)] = poses
    return out


# ---------------------------------------------------------------------------------------------------------------- 3. resident = explicit
@pytest.mark.parametrize("fused", [False, True])
def test_resident_window_equals_explicit(capi, oracle, ses, fused):
    """The window re-inserted from the outgoing map's scan ring (device to device) against the same call with explicit host arrays.
    fused: the scans went in through vba_map_pvec_update_cut_voxel, so only the device ever held their world covariances; the
    explicit side gets them from the restatement of pvec_update."""
    out = []
    for resident in (True, False):
        side = Side(capi, oracle, ses, fused=fused)
        side.history(ses["W"])
        store = side.ctx.kf_store()
        _fill_store(store, ses, 5)
        lm = side.ctx.loop_map()
        _, nf = _close_loop(side, store, lm, resident=resident)
        a, b = _defined(side.ctx.dump_leaves(), side.ctx.dump_plane_var())
        out.append((a, b, nf, side.ctx.map_stats()["fixed_points"]))
        lm.close(); store.close(); side.close()
    (a1, b1, n1, f1), (a0, b0, n0, f0) = out
    assert n1 == n0 > 50 and f1 == f0 > 0
    assert np.array_equal(a1, a0), "leaf records differ between the resident and the explicit window"
    assert np.array_equal(b1, b0) and np.abs(b1).max() > 0, "cov_add differs between the resident and the explicit window"


# ---------------------------------------------------------------------------------------------------------------- 4. the session goes on
def test_session_goes_on(capi, oracle, ses):
    """After loop_update two full local-mapping steps (LM, margi, slide, insert, multi_recut) on the device and on the oracle, at the
    per-call bars of tests/test_gpu_map.py; then keyframe_loading from the same store into the adopted map."""
    from test_gpu_map import _compare_leaves, _leaf_table
    wl, W, dx = ses["wl"], ses["W"], ses["dx"]
    side = Side(capi, oracle, ses, fused=True)
    side.history(W)
    ctx = side.ctx
    store = ctx.kf_store()
    _fill_store(store, ses, 8)
    lm = ctx.loop_map()
    inp, nf = _close_loop(side, store, lm)
    om, of = _oracle_loop(oracle, wl, store, inp)
    assert nf == of.size()
    x_g = [p.copy() for p in inp["win_poses"]]; x_o = [p.copy() for p in inp["win_poses"]]
    nxt = side.next_scan
    for step in range(2):
        a = ctx.lidar_ba_damping_iter(np.array(x_g), max_iter=3, thd_num=2)
        b = of.lidar_ba_damping_iter(np.array(x_o), max_iter=3, thd_num=2)
        assert np.abs(a["poses"] - b["poses"]).max() < 1e-6      # bar: 1e-4 m / 1e-4 rad
        # both sides continue from the device poses, so that the marginalisation sees identical inputs (tests/test_gpu_map.py)
        x_g = [p for p in a["poses"]]; x_o = [p.copy() for p in a["poses"]]
        ctx.evaluate_only_residual(np.array(x_g)); of.evaluate_only_residual(np.array(x_o))
        ctx.margi(W, np.array(x_g), jour=10.0 + step); om.margi(W, np.array(x_o), of, jour=10.0 + step)
        assert ctx.num_slide_roots() == om.num_slide_roots()
        gd, od = ctx.dump_leaves(), om.dump_leaves()
        _compare_leaves(gd, od)
        g, o = _leaf_table(gd), _leaf_table(od)
        npl = 0
        for key, ro in o.items():                                 # refined planes written by plane_update (VM:1344-1388)
            if ro[7] and np.abs(ro[35:38]).max() > 0:
                rg = g[key]
                assert np.abs(rg[32:35] - ro[32:35]).max() < 1e-9, (key, "center")
                assert abs(abs(np.dot(rg[35:38], ro[35:38])) - 1) < 1e-9, (key, "normal")
                assert abs(rg[38] - ro[38]) < 1e-6 * max(1e-3, abs(ro[38])), (key, "radius")
                npl += 1
        assert npl > 20
        # plane_var (VM:1356-1383) at the bar of tests/test_gpu_fullsize.py; the normal's sign is free
        gs, _, _ = _sorted(gd); gpv, _, _ = _sorted(ctx.dump_plane_var())
        os_, opv, _ = _sorted(od, om.dump_plane_var())
        upd = (os_[:, 7] != 0) & (np.abs(os_[:, 35:38]).max(1) > 0)
        sgn = np.sign((gs[upd, 35:38] * os_[upd, 35:38]).sum(1))
        G = gpv[upd, 5:41].reshape(-1, 6, 6).copy(); O = opv[upd].reshape(-1, 6, 6)
        G[:, :3, 3:] *= sgn[:, None, None]; G[:, 3:, :3] *= sgn[:, None, None]
        sc = np.abs(O).reshape(len(O), -1).max(1); err = np.abs(G - O).reshape(len(O), -1).max(1)
        print("step %d: %d refined planes, plane_var worst relative error %.3g" % (step, npl, float((err / np.maximum(sc, 1e-300)).max())))
        assert (err <= 1e-5 * sc + 1e-18).all(), ("plane_var", float((err / np.maximum(sc, 1e-300)).max()))
        ctx.slide(1); om.slide(1)
        x_g = x_g[1:]; x_o = x_o[1:]
        pose = lo.move_pose(ses["poses"][nxt], dx)
        v_w = oracle.pvec_update(ses["points"][nxt], ses["vars"][nxt], _state(pose), ses["cov"])[0]
        ctx.pvec_update_cut_voxel(W - 1, ses["points"][nxt], ses["vars"][nxt], pose, ses["cov"], multi=True)
        om.cut_voxel(W - 1, ses["points"][nxt], pose, var=v_w, multi=True)
        x_g.append(pose.copy()); x_o.append(pose.copy())
        nxt += 1
        ctx.recut(W, np.array(x_g), multi=True); om.recut(W, np.array(x_o), of, multi=True)
        assert ctx.size() == of.size() > 50
        _assert_map_equals_oracle(ctx.dump_leaves(), ctx.dump_plane_var(), om)
    # keyframe_loading (VS:1407-1432) from the same store into the adopted map: fixed points WITHOUT covariance, as before
    clouds, _, kposes = _store_host(store)
    for k in (0, 2):
        store.load(k, ctx, jour=20.0 + k)
        om.cut_voxel_fix(lo.world(kposes[k], clouds[k]), jour=20.0 + k)
    ctx.recut(W, np.array(x_g), multi=True); om.recut(W, np.array(x_o), of, multi=True)
    assert ctx.size() == of.size()
    _assert_map_equals_oracle(ctx.dump_leaves(), ctx.dump_plane_var(), om)
    lm.close(); store.close(); side.close()


# ---------------------------------------------------------------------------------------------------------------- 5. residency, refusals
def test_residency_after_one_cycle(capi, oracle, ses):
    """After vba_loop_map_reserve and one full cycle (which trades the maps and equalises their capacities), a second build plus
    update allocates nothing: vba_loop_map_allocations, vba_kf_allocations and the capacity field of vba_map_stats stay put."""
    side = Side(capi, oracle, ses, fused=False)
    side.history(ses["W"])
    store = side.ctx.kf_store()
    store.reserve(points=1 << 19, keyframes=16, merge_points=1 << 16)
    _fill_store(store, ses, 8)
    lm = side.ctx.loop_map()
    lm.reserve(fix_points=1 << 19, nodes=1 << 20)
    _, nf1 = _close_loop(side, store, lm)
    before = (lm.allocations(), store.allocations(), side.ctx.map_stats()["hash_capacity"])
    d1 = _defined(side.ctx.dump_leaves(), side.ctx.dump_plane_var())
    _, nf2 = _close_loop(side, store, lm)                          # the window now comes from the ring of the map adopted in cycle 1
    after = (lm.allocations(), store.allocations(), side.ctx.map_stats()["hash_capacity"])
    print("allocations (loop map, store, root table):", before, "->", after)
    assert after == before
    d2 = _defined(side.ctx.dump_leaves(), side.ctx.dump_plane_var())
    assert nf1 == nf2 and np.array_equal(d1[0], d2[0]) and np.array_equal(d1[1], d2[1])     # the same loop closure twice: the same map
    lm.close(); store.close(); side.close()


def test_refusals_leave_the_map_alone(capi, oracle, ses):
    wl, W = ses["wl"], ses["W"]
    side = Side(capi, oracle, ses, fused=False)
    side.history(W)
    ctx = side.ctx
    store = ctx.kf_store()
    _fill_store(store, ses, 5)
    lm = ctx.loop_map()
    lm.build(store)
    roots = lm.num_roots()
    inp = _loop_inputs(side)
    before = _defined(ctx.dump_leaves(), ctx.dump_plane_var())

    def refused(code, c=ctx, m=lm, poses=inp["win_poses"], **kw):
        with pytest.raises(capi.VbaError) as e:
            c.loop_update(m, poses, inp["bl_scans"], inp["bl_poses"], inp["bl_vars"], **kw)
        assert e.value.status == code, (e.value.status, code)

    refused(capi.ERR_BAD_ARG, poses=np.zeros((0, 12)))                                    # win_count 0
    refused(capi.ERR_BAD_ARG, poses=_pad(inp["win_poses"], W + 1))                        # win_count W + 1
    bad = inp["win_poses"].copy(); bad[1, 10] = np.nan
    refused(capi.ERR_BAD_ARG, poses=bad)
    other = capi.Context(_opts(capi, wl, voxel_size=wl.voxel_size * 2))                   # a loop map with other map options
    lm_other = other.loop_map()
    refused(capi.ERR_BAD_ARG, m=lm_other)
    ctx.set_shard(0, 2)                                                                   # a sharded context
    refused(capi.ERR_UNSUPPORTED)
    ctx.set_shard(0, 1)
    after = _defined(ctx.dump_leaves(), ctx.dump_plane_var())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert lm.num_roots() == roots                                                        # and the loop map is still built
    # the call goes through afterwards
    nf = ctx.loop_update(lm, inp["win_poses"], inp["bl_scans"], inp["bl_poses"], inp["bl_vars"])
    om, of = _oracle_loop(oracle, wl, store, inp)
    assert nf == of.size()
    _assert_map_equals_oracle(ctx.dump_leaves(), ctx.dump_plane_var(), om)
    lm_other.close(); other.close(); lm.close(); store.close(); side.close()


def test_empty_store_and_no_marginalised_scans(capi, oracle, ses):
    """An empty store gives an empty map_loop; k = 0 skips the fixed insertion: loop_update then rebuilds the window alone."""
    wl, W = ses["wl"], ses["W"]
    side = Side(capi, oracle, ses, fused=False)
    side.history(W)
    ctx = side.ctx
    store = ctx.kf_store()
    lm = ctx.loop_map()
    assert lm.build(store) == 0 and lm.num_roots() == 0
    inp = _loop_inputs(side)
    nf = ctx.loop_update(lm, inp["win_poses"])
    om = _omap(oracle, wl)
    of = lo.replay_update(om, oracle, [], [], [], inp["win_scans"], inp["win_vars"], inp["win_poses"])
    assert nf == of.size() > 50 and ctx.map_stats()["fixed_points"] == 0
    _assert_map_equals_oracle(ctx.dump_leaves(), ctx.dump_plane_var(), om)
    lm.close(); store.close(); side.close()


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
def test_deterministic_mode_repeats_bit_for_bit(capi, oracle, ses):
    """deterministic = 1: the session of test 2 twice; dumps (rows in ascending node id), cov_add, the factor store and its order equal
    bit for bit.  The fixed-point path is covered by deterministic mode (k_ins_newroots_det ranks new roots by their first point)."""
    outs = []
    for run in range(2):
        side = Side(capi, oracle, ses, fused=True, deterministic=1)
        side.history(ses["W"])
        store = side.ctx.kf_store()
        _fill_store(store, ses, 8)
        lm = side.ctx.loop_map()
        inp, nf = _close_loop(side, store, lm)
        ev, evec, pa = side.ctx.read_back()
        H, g, r = side.ctx.acc_evaluate2(inp["win_poses"])
        outs.append(dict(nf=np.array(nf), dump=side.ctx.dump_leaves(), pv=side.ctx.dump_plane_var(), masks=side.ctx.factor_occupancy_masks(),
                         ev=ev, evec=evec, pa=pa, H=H, g=g, r=np.array(r)))
        lm.close(); store.close(); side.close()
    a, b = outs
    assert a["nf"] > 50
    for k in a:
        assert np.array_equal(a[k], b[k]), k
