"""vba_motion_init (Initialization::motion_init, voxelslam.cpp:617-819) on the MI355X against a replay on the CPU oracle
(tests/init_oracle.py: the oracle's VoxelMap rebuilt every round with that round's thresholds, Factor.li_ba_damping_iter(gravity),
imu_preintegrate, and numpy restatements of the initialisation motion blur and align_gravity)."""
import os

import numpy as np
import pytest

import init_oracle

pytestmark = pytest.mark.gpu

W = 10
NM = np.array([0.01] * 3 + [1.0] * 3)
NW = np.array([1e-4] * 6)


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.fixture(scope="module")
def synth():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth as s
    return s


def _wl(synth, **kw):
    return synth.Workload("init", W, 0.5, 0, "spin32", (10.0, 8.0, 3.0), 0, 0, **kw)


def _imu_pre(oracle, d):
    ims = d["imus"]
    return np.stack([oracle.imu_preintegrate(ims[i][:, 0], ims[i][:, 1:4], ims[i][:, 4:7], np.zeros(3), np.zeros(3), NM, NW, d["scale_gravity"])
                     for i in range(1, W)])


def _ctx(capi, wl, **kw):
    o = capi.options_from_workload(wl)
    for k, v in kw.items():
        setattr(o, k, v)
    return capi.Context(o)


def _run_dev(ctx, wl, d, ip, point_notime=False):
    return ctx.motion_init(d["clouds"], d["curvs"], d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err, d["scale_gravity"], NM, NW,
                           d["states"], d["covs"], ip, point_notime=point_notime, want_hess=True)


def _run_ora(oracle, wl, d, ip, point_notime=False):
    return init_oracle.motion_init(oracle, W, wl, d["clouds"], d["curvs"], d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err,
                                   d["scale_gravity"], NM, NW, d["states"], d["covs"], ip, point_notime=point_notime)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if np.size(b) else 0.0


def _compare(a, b, pnt_bar, var_bar):
    """a = device, b = oracle replay.  Returns the measured deviations (printed with -s)."""
    assert a["round_log"].shape == b["round_log"].shape, (a["round_log"], b["round_log"])
    assert np.array_equal(a["round_log"][:, 0], b["round_log"][:, 0]), (a["round_log"][:, 0], b["round_log"][:, 0])   # factor counts
    assert np.array_equal(a["round_log"][:, 4], b["round_log"][:, 4])
    assert np.abs(a["round_log"][:, 3] - b["round_log"][:, 3]).max() < 1e-9     # |x_buf[0].g| per round
    if b["hess"] is not None:                                                  # the last damping_iter's Hessian
        assert np.abs(a["hess"] - b["hess"]).max() < 1e-6 * np.abs(b["hess"]).max()
    assert (a["iterations"], a["converged"], a["thresholds_left_relaxed"]) == (b["iterations"], b["converged"], b["thresholds_left_relaxed"])
    dev = dict(resis=_rel(a["round_log"][:, 1:3], b["round_log"][:, 1:3]) if b["round_log"][:, 1].any() else 0.0,
               eig=_rel(a["eigvalue3"], b["eigvalue3"]) if b["eigvalue3"].any() else 0.0,
               states=float(np.abs(a["states"] - b["states"]).max()), imu_pre=float(np.abs(a["imu_pre"] - b["imu_pre"]).max()))
    assert dev["resis"] < 1e-6 and dev["eig"] < 1e-6, dev              # measured worst 2.2e-11 / 1.2e-12
    assert dev["states"] < 1e-6 and dev["imu_pre"] < 1e-6, dev         # measured worst 2.3e-13 / 4.7e-15
    dp = dv = 0.0
    for (pa, va), (pb, vb) in zip(a["pvec"], b["pvec"]):
        assert pa.shape == pb.shape
        if len(pb):
            dp = max(dp, float(np.abs(pa - pb).max()))
            dv = max(dv, float((np.abs(va - vb) / np.maximum(np.abs(vb).max(axis=(1, 2), keepdims=True), 1e-300)).max()))
    dev["pnt"], dev["var"] = dp, dv
    assert dp < pnt_bar and dv < var_bar, dev                          # measured worst 4.3e-14 / 2.9e-14 (rel)
    print("deviations vs oracle:", dev)
    return dev


def _leaf_table(dump):
    return {tuple(int(v) for v in r[:5]): r for r in dump}


def _compare_leaves(gd, od):
    g, o = _leaf_table(gd), _leaf_table(od)
    assert set(g) == set(o), "leaf sets differ: %d vs %d" % (len(g), len(o))
    ds = dc = dn = 0.0
    for k, ro in o.items():
        rg = g[k]
        assert rg[5] == ro[5] and rg[6] == ro[6] and rg[7] == ro[7] and rg[8] == ro[8], (k, rg[5:9], ro[5:9])   # counts, plane, isexist
        ds = max(ds, float(np.abs(rg[22:32] - ro[22:32]).max() / max(np.abs(ro[22:32]).max(), 1.0)))
        if ro[7]:
            dc = max(dc, float(np.abs(rg[32:35] - ro[32:35]).max()))
            dn = max(dn, float(min(np.abs(rg[35:38] - ro[35:38]).max(), np.abs(rg[35:38] + ro[35:38]).max())))   # normal up to sign
    return ds, dc, dn


@pytest.fixture(scope="module")
def room(synth, oracle):
    wl = _wl(synth)
    d = synth.make_init_window(win_size=W, n_pts=20000, scene="room")
    ip = _imu_pre(oracle, d)
    b = _run_ora(oracle, wl, d, ip)
    return wl, d, ip, b


@pytest.fixture(scope="module")
def corridor(synth, oracle):
    wl = _wl(synth)
    d = synth.make_init_window(win_size=W, n_pts=20000, scene="corridor")
    ip = _imu_pre(oracle, d)
    b = _run_ora(oracle, wl, d, ip)
    return wl, d, ip, b


def test_converged_window(capi, room):
    wl, d, ip, b = room
    # the oracle itself converges after >= 3 rounds with |g| in range
    assert b["converged"] == 1 and b["iterations"] >= 3 and 9.6 <= np.linalg.norm(b["states"][-1, 22:25]) <= 10.0
    assert any(len(p[0]) > len(c) for p, c in zip(b["pvec"], d["clouds"])) and any(len(p[0]) < len(c) for p, c in zip(b["pvec"], d["clouds"]))
    ctx = _ctx(capi, wl)
    a = _run_dev(ctx, wl, d, ip)
    _compare(a, b, pnt_bar=1e-12, var_bar=1e-9)
    ds, dc, dn = _compare_leaves(ctx.dump_leaves(), b["vmap"].dump_leaves())
    print("leaf deviations: sums %.3g centres %.3g normals %.3g" % (ds, dc, dn))
    assert ds < 1e-9 and dc < 1e-9 and dn < 1e-9        # measured worst: sums 1.7e-14 (relative), centres 0, normals 0
    assert ctx.size() == b["factor"].size()


def test_degenerate_corridor(capi, corridor):
    wl, d, ip, b = corridor
    assert b["converged"] == 0 and b["eigvalue3"][0] < 15
    ctx = _ctx(capi, wl)
    a = _run_dev(ctx, wl, d, ip)
    assert a["converged"] == 0 and a["eigvalue3"][0] < 15
    assert a["thresholds_left_relaxed"] == b["thresholds_left_relaxed"]
    assert ctx.num_roots() == 0
    _compare(a, b, pnt_bar=1e-12, var_bar=1e-9)


def test_too_few_planes(capi, oracle, synth):
    wl = _wl(synth)
    d = synth.make_init_window(win_size=W, n_pts=30, scene="room")
    ip = _imu_pre(oracle, d)
    b = _run_ora(oracle, wl, d, ip)
    ctx = _ctx(capi, wl)
    a = _run_dev(ctx, wl, d, ip)
    assert a["iterations"] == 1 and b["iterations"] == 1 and a["converged"] == 0
    assert np.array_equal(a["states"], d["states"]) and np.array_equal(a["imu_pre"], ip)
    _compare(a, b, pnt_bar=1e-12, var_bar=1e-12)   # same states as the oracle: the blur alone


def test_blur_full_size_exact(capi, room):
    # no plane can form (min_point huge): round 1 breaks before the LM, so pvec_buf is the blur of the INPUT states at full size
    wl, d, ip, _ = room
    o = capi.options_from_workload(wl)
    for k in range(4):
        o.min_point[k] = 1e9
    ctx = capi.Context(o)
    a = _run_dev(ctx, wl, d, ip)
    assert a["iterations"] == 1 and a["round_log"][0, 0] == 0
    dp = 0.0
    for i in range(W):
        l = 0 if i == 0 else i - 1
        ref = init_oracle.motion_blur(d["clouds"][i], d["curvs"][i], d["imus"][i], d["states"][i], d["states"][l], d["beg_times"][i], d["ext"],
                                      d["scale_gravity"])
        pa, va = a["pvec"][i]
        assert pa.shape == ref.shape
        dp = max(dp, float(np.abs(pa - ref).max()))
        assert np.array_equal(va, np.broadcast_to(np.eye(3), va.shape))
    print("blur deviation %.3g" % dp)
    assert dp < 1e-12                                                  # measured worst 3.6e-15


def test_point_notime(capi, oracle, synth):
    wl = _wl(synth)
    d = synth.make_init_window(win_size=W, n_pts=8000, scene="room")
    ip = _imu_pre(oracle, d)
    b = _run_ora(oracle, wl, d, ip, point_notime=True)
    ctx = _ctx(capi, wl)
    a = _run_dev(ctx, wl, d, ip, point_notime=True)
    assert all(len(p[0]) == len(c) for p, c in zip(a["pvec"], d["clouds"]))
    _compare(a, b, pnt_bar=1e-12, var_bar=1e-9)


def test_one_context_many_calls(capi, oracle, synth, room, corridor):
    wl, d, ip, b = room
    _, dc, ipc, bc = corridor
    fresh = _ctx(capi, wl)
    a0 = _run_dev(fresh, wl, d, ip)
    live0 = fresh.map_stats()["roots"]
    ctx = _ctx(capi, wl)
    ac = _run_dev(ctx, wl, dc, ipc)
    assert ac["converged"] == 0 and ctx.num_roots() == 0
    for _ in range(2):
        a = _run_dev(ctx, wl, d, ip)
        _compare(a, b, pnt_bar=1e-12, var_bar=1e-9)
        # the fresh context's result at the case-1 bars (not bit for bit: a reused map's storage order differs)
        assert np.array_equal(a["round_log"][:, 0], a0["round_log"][:, 0]) and np.abs(a["states"] - a0["states"]).max() < 1e-6
        assert ctx.map_stats()["roots"] <= live0
    # the context's own thresholds are in force again: a plain window at the original options matches the oracle
    full = np.zeros((W, 12))
    full[:, :9] = d["gt_states"][:, 1:10]; full[:, 9:] = d["gt_states"][:, 10:13]
    ctx.map_reset()
    om = oracle.VoxelMap(W, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, 5)
    for i in range(W):
        ctx.cut_voxel(i, d["clouds"][i], full[i])
        om.cut_voxel(i, d["clouds"][i], full[i])
    f = oracle.Factor(W)
    ctx.recut(W, full)
    om.recut(W, full, f)
    assert ctx.size() == f.size()
    ds, dcen, dn = _compare_leaves(ctx.dump_leaves(), om.dump_leaves())
    assert ds == 0.0 and dcen < 1e-9 and dn < 1e-9


def test_timing_family(capi, synth, oracle):
    wl = _wl(synth)
    d = synth.make_init_window(win_size=W, n_pts=3000, scene="room")
    ip = _imu_pre(oracle, d)
    ctx = _ctx(capi, wl)
    ctx.timing_enable(True)
    a = _run_dev(ctx, wl, d, ip)
    t, n = ctx.timing_get("init")
    assert n >= a["iterations"] and t > 0.0


def test_harness_mode3(capi, oracle, synth, tmp_path):
    """motion_init through include/voxelba_adapter.hpp (vba::Initialization) on the first W scans, then the steady-state loop of
    mode 1 from the initialised window for 3 more scans, against the oracle replay at the bars of the harness test."""
    import subprocess
    harness = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-slam_amd", "vba_harness")
    assert os.path.exists(harness)
    wl = _wl(synth)
    extra = 3
    d = synth.make_init_window(win_size=W + extra, n_pts=20000, scene="room")
    dw = {k: (v[:W] if k in ("clouds", "curvs", "imus", "beg_times", "states", "covs") else v) for k, v in d.items()}
    ip = _imu_pre(oracle, dw)
    b = _run_ora(oracle, wl, dw, ip)
    assert b["converged"] == 1
    # the extra scans: ground truth carried into the frame the initialisation left (align_gravity rotates the window)
    gt = d["gt_states"]
    Rf, Rg = b["states"][W - 1, 1:10].reshape(3, 3), gt[W - 1, 1:10].reshape(3, 3)
    RA = Rf @ Rg.T
    tA = b["states"][W - 1, 10:13] - RA @ gt[W - 1, 10:13]
    ext = d["ext"]
    scans = []
    for k in range(W, W + extra):
        st = b["states"][W - 1].copy()
        st[0] = gt[k, 0]
        st[1:10] = (RA @ gt[k, 1:10].reshape(3, 3)).ravel(); st[10:13] = RA @ gt[k, 10:13] + tA; st[13:16] = RA @ gt[k, 13:16]
        p, vb = oracle.var_init(d["clouds"][k], ext, wl.dept_err, wl.beam_err)
        scans.append(dict(state=st, pts=p, var_body=vb, imu=d["imus"][k], cov=d["covs"][k]))
    head = [20241004.0, W, W + extra, 3, wl.voxel_size, wl.max_layer, wl.max_points, wl.min_eigen_value, *wl.plane_thre, *wl.min_point,
            wl.imu_coef, 5, 0, wl.dept_err, wl.beam_err, d["scale_gravity"], *ext]
    chunks = [np.array(head, dtype=np.float64)]
    for i in range(W):
        chunks.append(np.concatenate([[len(d["clouds"][i]), len(d["imus"][i]), d["beg_times"][i]], d["states"][i], d["covs"][i]]))
        chunks += [d["clouds"][i].ravel(), d["curvs"][i].ravel(), d["imus"][i].ravel()]
    for sc in scans:
        im = sc["imu"]
        chunks.append(np.concatenate([[len(sc["pts"])], sc["state"], sc["cov"], [len(im)]]))
        chunks += [sc["pts"].ravel(), sc["var_body"].ravel(), im[:, 0], im[:, 1:4].ravel(), im[:, 4:7].ravel()]
    chunks.append(np.concatenate([NM, NW]))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate(chunks).astype(np.float64).tofile(fin)
    r = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(fout, dtype=np.float64)
    # the initialisation record
    assert out[0] == -2 and out[1] == b["converged"] and out[2] == b["iterations"] and out[3] == b["thresholds_left_relaxed"]
    assert _rel(out[4:7], b["eigvalue3"]) < 1e-6
    assert np.abs(out[7:7 + W * 25].reshape(W, 25) - b["states"]).max() < 1e-6
    q = 7 + W * 25
    # oracle replay of the steady-state steps (tests/test_gpu_harness.py, mode 1) from the initialised window
    om, of = b["vmap"], b["factor"]
    x_buf, imus = [x.copy() for x in b["states"]], [x.copy() for x in b["imu_pre"]]
    win_count, jour, recs = W, 0.0, []

    def poses_of(xs):
        return np.array([np.concatenate([x[1:10], x[10:13]]) for x in xs])

    def step(k):
        nonlocal x_buf, imus, win_count, jour
        res = of.li_ba_damping_iter(np.array(x_buf), np.array(imus), gravity=False, imu_coef=wl.imu_coef, max_iter=3)
        x_buf = [x.copy() for x in res["states"]]; imus = [x.copy() for x in res["imus"]]
        recs.append((k, np.array(x_buf).copy(), 1.0 / np.abs(np.array([res["hess"][i, 15 + i] for i in range(6)]))))
        om.margi(win_count, poses_of(x_buf), of, jour=jour)
        jour += 0.1
        om.slide(1)
        x_buf.pop(0); imus.pop(0)
        win_count -= 1
    step(W - 1)
    for j, sc in enumerate(scans):
        win_count += 1
        x_buf.append(sc["state"].copy())
        im = sc["imu"]
        imus.append(oracle.imu_preintegrate(im[:, 0], im[:, 1:4], im[:, 4:7], x_buf[-2][16:19], x_buf[-2][19:22], NM, NW, d["scale_gravity"]))
        v_w, _ = oracle.pvec_update(sc["pts"], sc["var_body"], sc["state"], sc["cov"])
        om.cut_voxel(win_count - 1, sc["pts"], poses_of([sc["state"]])[0], var=v_w, multi=True)
        of.clear()
        om.recut(win_count, poses_of(x_buf), of, multi=True)
        step(W + j)
    for k, xs, v6 in recs:
        assert out[q] == k
        got = out[q + 1:q + 1 + W * 25].reshape(W, 25); gv6 = out[q + 1 + W * 25:q + 7 + W * 25]
        q += 7 + W * 25
        assert np.abs(got - xs).max() < 1e-6, (k, np.abs(got - xs).max())
        assert np.allclose(gv6, v6, rtol=1e-5), (k, gv6, v6)
    assert out[q] == -1
    nl = int(out[q + 1]); q += 2
    leaves = out[q:q + nl * 39].reshape(nl, 39)
    od = om.dump_leaves()
    assert nl == len(od)
    key = lambda m: np.lexsort((m[:, 4], m[:, 3], m[:, 2], m[:, 1], m[:, 0]))   # noqa: E731
    g, o = leaves[key(leaves)], od[key(od)]
    assert np.array_equal(g[:, :9], o[:, :9]), "leaf keys / counts / plane flags / isexist differ"
    scale = np.maximum(1.0, np.abs(o[:, 22:31]).max(1))
    assert (np.abs(g[:, 22:32] - o[:, 22:32]).max(1) < 1e-6 * scale).all()
    pl = (o[:, 7] != 0) & (np.abs(o[:, 35:38]).max(1) > 0)
    if pl.any():
        assert np.abs(g[pl, 32:35] - o[pl, 32:35]).max() < 1e-5
        assert np.abs(np.abs((g[pl, 35:38] * o[pl, 35:38]).sum(1)) - 1).max() < 1e-8
