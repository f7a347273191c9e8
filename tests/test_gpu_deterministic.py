"""Deterministic mode (vba_options::deterministic = 1) on the MI355X: the canonical numbering and order of
tests/det_replay.py on real dumps, bit-identical results from run to run at full size, and parity with the oracle kept.
Every comparison between two runs is np.array_equal."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import det_replay as dr

pytestmark = pytest.mark.gpu

NAME = "hesai200k_w10"


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


@pytest.fixture(scope="module")
def synth():
    from voxel_slam_amd import synth as s
    return s


@pytest.fixture(scope="module")
def scans(synth):
    wl = synth.CONFIGS[NAME]
    return wl, synth.make_scans(wl)


def _ctx(capi, wl, **kw):
    o = capi.options_from_workload(wl)
    o.deterministic = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return capi.Context(o)


def _omap(oracle, wl):
    return oracle.VoxelMap(wl.win_size, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, 5)


def _sorted(d):
    return d[np.lexsort((d[:, 4], d[:, 3], d[:, 2], d[:, 1], d[:, 0]))]


# ---------------------------------------------------------------------------------------------------------------- 1. root numbering
def test_root_numbering(capi, synth, scans):
    wl, s = scans
    poses = synth.poses_flat(s["R0"], s["p0"])
    ctx = _ctx(capi, wl)
    rn = dr.RootNumbering()
    ctx.cut_voxel(0, s["points"][0], poses[0])
    rn.insert(dr.voxel_keys(dr.world_points(s["points"][0], poses[0]), wl.voxel_size))
    scan0 = list(rn.ids)
    d = ctx.dump_leaves()
    assert len(d) > 10000 and (d[:, 3] == 0).all()
    assert np.array_equal(d[:, :3].astype(np.int64), rn.live_in_id_order()), "roots are not numbered by their voxel's first point"

    # keyframe points (world frame) at journey 500 create roots of their own (journey 500) next to the scan's (journey 0);
    # prune at 800 frees the scan's roots only; the next scan reuses the freed ids in ascending order, then fresh ones, and keeps
    # the ids of the keyframe roots it touches
    wfix = dr.world_points(s["points"][3][::3], poses[3])
    ctx.cut_voxel_fix(wfix, jour=500.0)
    assert len(rn.insert(dr.voxel_keys(wfix, wl.voxel_size))) > 1000
    d = ctx.dump_leaves()
    assert np.array_equal(d[:, :3].astype(np.int64), rn.live_in_id_order())
    ctx.prune(800.0, 700)
    rn.prune(scan0)
    assert ctx.map_stats()["free_roots"] == len(rn.free) == len(scan0)
    ctx.cut_voxel(1, s["points"][1], poses[1])
    rn.insert(dr.voxel_keys(dr.world_points(s["points"][1], poses[1]), wl.voxel_size))
    d = ctx.dump_leaves()
    assert np.array_equal(d[:, :3].astype(np.int64), rn.live_in_id_order()), "freed ids are not reused in first-touch order"
    st = ctx.map_stats()
    assert st["nodes_high_water"] == rn.nodes and st["free_roots"] == len(rn.free)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 2. store order
def _rebuild(capi, synth, wl, s, multi=False, **kw):
    W = wl.win_size
    poses = synth.poses_flat(s["R0"], s["p0"])
    ctx = _ctx(capi, wl, **kw)
    for i in range(W):
        ctx.cut_voxel(i, s["points"][i], poses[i])
    ctx.recut(W, poses, multi=multi)
    return ctx, poses


def test_store_order_and_child_blocks(capi, synth, scans):
    wl, s = scans
    W = wl.win_size
    ctx, poses = _rebuild(capi, synth, wl, s)
    d = ctx.dump_leaves()
    V = ctx.size()
    assert V > 10000
    masks = ctx.factor_occupancy_masks()
    rows = np.nonzero(d[:, 9] >= 0)[0]
    pos = d[rows, 9].astype(np.int64)
    assert len(rows) == V and np.array_equal(np.sort(pos), np.arange(V))
    # store position p holds the factor of dump row rows[k] with pos[k] == p; the store must be sorted by (bucket, row)
    o = dr.store_order(masks[pos], rows, W)
    assert np.array_equal(pos[o], np.arange(V)), "factor store is not ordered by (mask bucket, node id)"
    # child leaves: a fresh map allocates roots (first-touch order, scan by scan), then each level's blocks by parent id, so the
    # leaves in id order are sorted by (layer, root rank, octant path)
    rn = dr.RootNumbering()
    for i in range(W):
        rn.insert(dr.voxel_keys(dr.world_points(s["points"][i], poses[i]), wl.voxel_size))
    rank = np.array([rn.ids[tuple(int(v) for v in k)] for k in d[:, :3]])
    assert (d[:, 3] > 0).sum() > 1000
    exp = np.lexsort((d[:, 4], rank, d[:, 3]))
    assert np.array_equal(exp, np.arange(len(d))), "child blocks are not allocated in (parent rank, octant) order"
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 3. rebuild twice
def _rebuild_outputs(capi, synth, wl, s):
    W = wl.win_size
    ctx, poses = _rebuild(capi, synth, wl, s)
    out = dict(dump=ctx.dump_leaves(), pv=ctx.dump_plane_var(), masks=ctx.factor_occupancy_masks())
    out["H"], out["g"], out["r"] = ctx.acc_evaluate2(poses)
    a = ctx.lidar_ba_damping_iter(poses, max_iter=3, thd_num=2)
    out.update(lid_poses=a["poses"], lid_hess=a["hess"], lid_trace=a["trace"], lid_resis=a["resis"])
    imu_samples, vel, grav = synth.make_imu(wl, gyr_sigma=1e-3, acc_sigma=1e-2)
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    imus = np.stack([capi.imu_preintegrate(t, gy, ac, np.zeros(3), np.zeros(3), nm, nw) for (t, gy, ac) in imu_samples])
    states = np.zeros((W, 25))
    for i in range(W):
        states[i, 0] = 0.1 * i
        states[i, 1:10] = s["R0"][i].ravel(); states[i, 10:13] = s["p0"][i]; states[i, 13:16] = vel[i]; states[i, 22:25] = grav
    for gravity in (False, True):
        out["res%d" % gravity] = ctx.evaluate_only_residual(poses)
        b = ctx.li_ba_damping_iter(states, imus, gravity=gravity, max_iter=3)
        out.update({"li%d_states" % gravity: b["states"], "li%d_hess" % gravity: b["hess"], "li%d_trace" % gravity: b["trace"]})
    out["dump_after"] = ctx.dump_leaves()
    ctx.close()
    return out


def test_rebuild_twice_is_bit_identical(capi, synth, scans):
    wl, s = scans
    a = _rebuild_outputs(capi, synth, wl, s)
    b = _rebuild_outputs(capi, synth, wl, s)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------- 4. session twice
def _session(capi, synth, wl, li, steps=12):
    """The local-mapping step of bench.py (margi, slide, pvec_update + cut_voxel_multi, multi recut, 3 LM iterations, refined
    poses fed forward), with one keyframe load (cut_voxel_fix) and one prune inserted."""
    W = wl.win_size
    nscan = W + steps
    wll = dataclasses.replace(wl, name=wl.name + "_traj%d" % nscan, win_size=nscan)
    sl = synth.make_scans(wll)
    x0 = synth.poses_flat(sl["R0"], sl["p0"])
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    cov = np.eye(15) * 1e-6
    imu_samples, vel, g = synth.make_imu(wll, gyr_sigma=1e-3, acc_sigma=1e-2)
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    imu_all = np.stack([capi.imu_preintegrate(t, gy, ac, np.zeros(3), np.zeros(3), nm, nw) for (t, gy, ac) in imu_samples])
    ctx = _ctx(capi, wl)
    pv = [ctx.var_init(p, ext, wl.dept_err, wl.beam_err) for p in sl["points"]]
    for i in range(W):
        ctx.pvec_update_cut_voxel(i, pv[i][0], pv[i][1], x0[i], cov, multi=True)
    ctx.recut(W, x0[:W], multi=True)
    window = np.ascontiguousarray(x0[:W])
    last = W - 1
    states = np.zeros((W, 25))
    rec = []
    for k in range(steps):
        ctx.margi(W, window, jour=float(last))
        ctx.slide(1)
        if k == 3:     # a keyframe's points come back as fixed points (loop closure / map reload)
            ctx.cut_voxel_fix(dr.world_points(sl["points"][0][::4], x0[0]), jour=float(last))
        if k == 7:
            ctx.prune(float(last), 4)
        last += 1
        ctx.pvec_update_cut_voxel(W - 1, pv[last][0], pv[last][1], x0[last], cov, multi=True)
        pw = np.ascontiguousarray(np.concatenate([window[1:], x0[last:last + 1]]))
        ctx.recut(W, pw, multi=True)
        if li:
            for i in range(W):
                j = last - W + 1 + i
                states[i, 0] = 0.1 * j; states[i, 1:10] = pw[i, :9]; states[i, 10:13] = pw[i, 9:12]; states[i, 13:16] = vel[j]; states[i, 22:25] = g
            r = ctx.li_ba_damping_iter(states, imu_all[last - W + 1:last], gravity=False, max_iter=3)
            window = np.ascontiguousarray(np.concatenate([r["states"][:, 1:10], r["states"][:, 10:13]], 1))
            tr = r["trace"]
        else:
            ctx.lm_begin(pw, thd_num=2)
            for _ in range(3):
                ctx.lm_iterate(sync=False)
            window = np.ascontiguousarray(ctx.lm_end(fetch=True)[0])
            tr = ctx.last_trace()
        rec.append(dict(size=ctx.size(), trace=tr.copy(), window=window.copy(), stats=np.array(list(ctx.map_stats().values()))))
    rec.append(dict(dump=ctx.dump_leaves()))
    ctx.close()
    return rec


@pytest.mark.parametrize("li", [False, True], ids=["lidar_only", "li_ba"])
def test_session_twice_is_bit_identical(capi, synth, scans, li):
    wl, _ = scans
    a = _session(capi, synth, wl, li)
    b = _session(capi, synth, wl, li)
    for k, (ra, rb) in enumerate(zip(a, b)):
        for key in ra:
            assert np.array_equal(ra[key], rb[key]), (k, key)
    assert a[-2]["size"] > 10000
    print("planar voxels after %d steps: %d" % (len(a) - 1, a[-2]["size"]))


# ---------------------------------------------------------------------------------------------------------------- 5. parity kept
def test_parity_with_oracle(capi, oracle, synth, scans):
    wl, s = scans
    W = wl.win_size
    poses = synth.poses_flat(s["R0"], s["p0"])
    ctx = _ctx(capi, wl)
    om = _omap(oracle, wl)
    for i in range(W):
        ctx.cut_voxel(i, s["points"][i], poses[i]); om.cut_voxel(i, s["points"][i], poses[i])
    g, o = _sorted(ctx.dump_leaves()), _sorted(om.dump_leaves())
    assert np.array_equal(g[:, :9], o[:, :9]) and np.array_equal(g[:, 22:32], o[:, 22:32])
    of = oracle.Factor(W)
    ctx.recut(W, poses, multi=False); om.recut(W, poses, of, multi=False)
    g, o = _sorted(ctx.dump_leaves()), _sorted(om.dump_leaves())
    assert ctx.size() == of.size() > 10000
    assert np.array_equal(g[:, :5], o[:, :5]) and np.array_equal(g[:, 5:9], o[:, 5:9])
    assert np.array_equal(g[:, 9] >= 0, o[:, 9] >= 0)                           # the same leaves are factors
    assert np.array_equal(g[:, 22:32], o[:, 22:32]), "pcr_add after recut is not bit-identical to the oracle"
    H, gr, r = ctx.acc_evaluate2(poses)
    H2, gr2, r2 = of.acc_evaluate2(poses)
    assert abs(r - r2) < 1e-11 * abs(r2)
    assert np.abs(H - H2).max() < 1e-9 * np.abs(H2).max() and np.abs(gr - gr2).max() < 1e-9 * np.abs(gr2).max()
    b = of.lidar_ba_damping_iter(poses, max_iter=3, thd_num=2, parallel=True)
    ctx.evaluate_only_residual(b["poses"]); of.evaluate_only_residual(b["poses"])
    ctx.margi(W, b["poses"], jour=3.0); om.margi(W, b["poses"], of, jour=3.0)
    g, o = _sorted(ctx.dump_leaves()), _sorted(om.dump_leaves())
    assert np.array_equal(g[:, :9], o[:, :9]) and np.array_equal(g[:, 22:32], o[:, 22:32]), "leaf sums after margi"
    ctx.close()


def test_motion_init_parity_and_repeatability(capi, oracle, synth):
    import init_oracle
    W = 10
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    wl = synth.Workload("init", W, 0.5, 0, "spin32", (10.0, 8.0, 3.0), 0, 0)
    d = synth.make_init_window(win_size=W, n_pts=20000, scene="room")
    ims = d["imus"]
    ip = np.stack([oracle.imu_preintegrate(ims[i][:, 0], ims[i][:, 1:4], ims[i][:, 4:7], np.zeros(3), np.zeros(3), nm, nw, d["scale_gravity"])
                   for i in range(1, W)])
    ref = init_oracle.motion_init(oracle, W, wl, d["clouds"], d["curvs"], d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err,
                                  d["scale_gravity"], nm, nw, d["states"], d["covs"], ip)
    runs = []
    for _ in range(2):
        ctx = _ctx(capi, wl)
        a = ctx.motion_init(d["clouds"], d["curvs"], d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err, d["scale_gravity"], nm, nw,
                            d["states"], d["covs"], ip, want_hess=True)
        a["dump"] = ctx.dump_leaves()
        ctx.close()
        runs.append(a)
    a, b = runs
    assert a["converged"] == ref["converged"] == 1 and a["iterations"] == ref["iterations"]
    assert np.array_equal(a["round_log"][:, 0], ref["round_log"][:, 0])
    assert np.abs(a["states"] - ref["states"]).max() < 1e-6
    for k in ("states", "round_log", "eigvalue3", "imu_pre", "hess", "dump"):
        assert np.array_equal(a[k], b[k]), k
    for (pa, va), (pb, vb) in zip(a["pvec"], b["pvec"]):
        assert np.array_equal(pa, pb) and np.array_equal(va, vb)


# ---------------------------------------------------------------------------------------------------------------- 6. down-sampling
def test_down_sampling_in_index_order(capi, synth):
    rng = np.random.default_rng(11)
    n = 200000
    # few voxels, many points each, coordinates and variances spanning many magnitudes: sums that depend on the order
    pnt = rng.uniform(-2.0, 2.0, (n, 3)) * (10.0 ** rng.integers(-6, 1, (n, 1)))
    pnt[::7] += 1e3 * rng.uniform(-1e-3, 1e-3, (len(pnt[::7]), 3))
    var = np.zeros((n, 9))
    var[:, [0, 4, 8]] = 10.0 ** rng.uniform(-12, 6, (n, 3))
    wl = synth.CONFIGS["room20k_w4"]
    ctx = _ctx(capi, wl)
    ctx2 = _ctx(capi, wl)
    cen, vd, cnt, first = dr.down_sampling(pnt, 0.5, var)
    assert cnt.max() > 1000
    a = ctx.down_sampling_pvec(pnt, var, 0.5)
    assert np.array_equal(a[0], cen) and np.array_equal(a[1], vd) and np.array_equal(a[2], cnt)
    assert all(np.array_equal(x, y) for x, y in zip(a, ctx2.down_sampling_pvec(pnt, var, 0.5)))
    cen, _, cnt, first = dr.down_sampling(pnt, 0.5)
    a = ctx.down_sampling_voxel(pnt, 0.5)
    assert np.array_equal(a[0], cen) and np.array_equal(a[1], cnt) and np.array_equal(a[2], first)
    assert all(np.array_equal(x, y) for x, y in zip(a, ctx2.down_sampling_voxel(pnt, 0.5)))
    assert np.array_equal(ctx.down_sampling_close(pnt, 0.5), ctx2.down_sampling_close(pnt, 0.5))
    ctx.close(); ctx2.close()


# ---------------------------------------------------------------------------------------------------------------- 7. harness
def test_harness_deterministic_mode0(oracle, synth, tmp_path):
    import test_gpu_harness as th
    harness = th.HARNESS
    assert os.path.exists(harness)
    W, nscan = 4, 8
    wl, sc, cov = th._problem(synth, oracle, W, nscan, 20000)
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    fin = str(tmp_path / "in.bin")
    th._write_input(fin, wl, sc, cov, 0, nm, nw)
    outs = []
    for k in range(2):
        fout = str(tmp_path / ("out%d.bin" % k))
        r = subprocess.run([harness, fin, fout, "--deterministic"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(open(fout, "rb").read())
    assert outs[0] == outs[1], "harness output differs between two deterministic runs"
    out = np.frombuffer(outs[0], dtype=np.float64)
    recs, om = th._oracle_replay(oracle, wl, sc, cov, 0, nm, nw)
    q = 0
    for k, xs, v6 in recs:
        assert out[q] == k
        got = out[q + 1:q + 1 + W * 25].reshape(W, 25); gv6 = out[q + 1 + W * 25:q + 7 + W * 25]
        q += 7 + W * 25
        assert np.abs(got - xs).max() < 1e-6, (k, np.abs(got - xs).max())
        assert np.allclose(gv6, v6, rtol=1e-5)
    assert out[q] == -1
    nl = int(out[q + 1]); q += 2
    leaves = out[q:q + nl * 39].reshape(nl, 39)
    od = om.dump_leaves()
    assert nl == len(od)
    g, o = _sorted(leaves), _sorted(od)
    assert np.array_equal(g[:, :9], o[:, :9])
    scale = np.maximum(1.0, np.abs(o[:, 22:31]).max(1))
    assert (np.abs(g[:, 22:32] - o[:, 22:32]).max(1) < 1e-6 * scale).all()


def test_harness_deterministic_mode3(oracle, synth, tmp_path):
    """Mode 3 (initialisation through the adapter, then the steady-state loop): two runs byte for byte, and the initialisation
    record against the oracle replay (the full oracle comparison of this mode is test_gpu_motion_init.py::test_harness_mode3)."""
    import init_oracle
    import test_gpu_harness as th
    W, extra = 10, 3
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    wl = synth.Workload("init", W, 0.5, 0, "spin32", (10.0, 8.0, 3.0), 0, 0)
    d = synth.make_init_window(win_size=W + extra, n_pts=20000, scene="room")
    ims = d["imus"]
    ip = np.stack([oracle.imu_preintegrate(ims[i][:, 0], ims[i][:, 1:4], ims[i][:, 4:7], np.zeros(3), np.zeros(3), nm, nw, d["scale_gravity"])
                   for i in range(1, W)])
    b = init_oracle.motion_init(oracle, W, wl, d["clouds"][:W], d["curvs"][:W], d["imus"][:W], d["beg_times"][:W], d["ext"], wl.dept_err,
                                wl.beam_err, d["scale_gravity"], nm, nw, d["states"][:W], d["covs"][:W], ip)
    assert b["converged"] == 1
    gt = d["gt_states"]
    Rf, Rg = b["states"][W - 1, 1:10].reshape(3, 3), gt[W - 1, 1:10].reshape(3, 3)
    RA = Rf @ Rg.T
    tA = b["states"][W - 1, 10:13] - RA @ gt[W - 1, 10:13]
    ext = d["ext"]
    head = [20241004.0, W, W + extra, 3, wl.voxel_size, wl.max_layer, wl.max_points, wl.min_eigen_value, *wl.plane_thre, *wl.min_point,
            wl.imu_coef, 5, 0, wl.dept_err, wl.beam_err, d["scale_gravity"], *ext]
    chunks = [np.array(head, dtype=np.float64)]
    for i in range(W):
        chunks.append(np.concatenate([[len(d["clouds"][i]), len(d["imus"][i]), d["beg_times"][i]], d["states"][i], d["covs"][i]]))
        chunks += [d["clouds"][i].ravel(), d["curvs"][i].ravel(), d["imus"][i].ravel()]
    for k in range(W, W + extra):
        st = b["states"][W - 1].copy()
        st[0] = gt[k, 0]
        st[1:10] = (RA @ gt[k, 1:10].reshape(3, 3)).ravel(); st[10:13] = RA @ gt[k, 10:13] + tA; st[13:16] = RA @ gt[k, 13:16]
        p, vb = oracle.var_init(d["clouds"][k], ext, wl.dept_err, wl.beam_err)
        im = d["imus"][k]
        chunks.append(np.concatenate([[len(p)], st, d["covs"][k], [len(im)]]))
        chunks += [p.ravel(), vb.ravel(), im[:, 0], im[:, 1:4].ravel(), im[:, 4:7].ravel()]
    chunks.append(np.concatenate([nm, nw]))
    fin = str(tmp_path / "in.bin")
    np.concatenate(chunks).astype(np.float64).tofile(fin)
    outs = []
    for k in range(2):
        fout = str(tmp_path / ("out%d.bin" % k))
        r = subprocess.run([th.HARNESS, fin, fout, "--deterministic"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(open(fout, "rb").read())
    assert outs[0] == outs[1], "harness output differs between two deterministic runs"
    out = np.frombuffer(outs[0], dtype=np.float64)
    assert out[0] == -2 and out[1] == b["converged"] and out[2] == b["iterations"] and out[3] == b["thresholds_left_relaxed"]
    assert np.abs(out[7:7 + W * 25].reshape(W, 25) - b["states"]).max() < 1e-6
