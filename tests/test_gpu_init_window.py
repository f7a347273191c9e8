"""The initialisation window resident in HBM: vba_init_window_push against the host route it replaces
(frame.read(0) -> vba_scan_down_sampling_close -> gather in ascending index order, tests/init_window_oracle.py), bit for bit, and
vba_motion_init_resident against vba_motion_init, bit for bit in deterministic mode and at the bars of
tests/test_gpu_motion_init.py::test_converged_window against the CPU oracle replay otherwise.  Expected clouds always come from the
frame's own read(0), so the time quantisation of the message layout cancels."""
import os
import subprocess

import numpy as np
import pytest

import decode_oracle as do
import init_window_oracle as iwo
import test_gpu_motion_init as tmi

pytestmark = pytest.mark.gpu

W = tmi.W
NM, NW = tmi.NM, tmi.NW


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


@pytest.fixture(scope="module")
def room(synth, oracle):
    """the window of test_gpu_motion_init.py (W = 10, 20 000 points per scan) and its oracle replay, computed once"""
    wl = tmi._wl(synth)
    d = synth.make_init_window(win_size=W, n_pts=20000, scene="room")
    ip = tmi._imu_pre(oracle, d)
    b = tmi._run_ora(oracle, wl, d, ip)
    return wl, d, ip, b


@pytest.fixture(scope="module")
def small(synth):
    """one scan of about 6000 points: several 256-lane blocks"""
    d = synth.make_init_window(win_size=2, n_pts=6500, scene="room")
    return d["clouds"][0], d["curvs"][0]


def _message(capi, pts, curv):
    """a livox message (time in ns, u32) of the cloud; returns (layout, bytes)"""
    lay = capi.scan_layout("livox")
    return lay, do.make_message(lay, pts, np.zeros(len(pts), dtype=np.uint8), np.round(np.asarray(curv) * 1e9).astype(np.uint32))


def _decode(capi, frame, pts, curv):
    lay, msg = _message(capi, pts, curv)
    n, _ = frame.decode(lay, msg, 1, 0.0)
    r = frame.read(0)
    assert len(r["pnt"]) == n
    return r["pnt"], r["curvature"]


def _host_route(ctx, P0, C0, down_size, min_points):
    idx, retried = iwo.push(P0, C0, down_size, min_points, ctx.down_sampling_close)
    return P0[idx], C0[idx], idx, retried


def _ctx(capi, wl, **kw):
    return tmi._ctx(capi, wl, **kw)


def _resident(ctx, win, wl, d, ip, point_notime=False):
    return ctx.motion_init_resident(win, d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err, d["scale_gravity"], NM, NW,
                                    d["states"], d["covs"], ip, point_notime=point_notime, want_hess=True)


def _assert_same_result(a, b):
    for k in ("states", "imu_pre", "hess", "round_log", "eigvalue3", "pvec_offsets"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["converged"], a["iterations"], a["thresholds_left_relaxed"]) == (b["converged"], b["iterations"], b["thresholds_left_relaxed"])
    assert len(a["pvec"]) == len(b["pvec"])
    for (pa, va), (pb, vb) in zip(a["pvec"], b["pvec"]):
        assert np.array_equal(pa, pb) and np.array_equal(va, vb)


# ---------------------------------------------------------------- 1. push equals the host route, bit for bit

@pytest.mark.parametrize("det", [1, 0])
def test_push_equals_the_host_route(capi, synth, small, det):
    pts, curv = small
    if not det:
        curv = np.sort(np.round(curv, 3))                    # 1 ms: ties are frequent
    ctx = _ctx(capi, tmi._wl(synth), deterministic=det)
    frame, win = ctx.scan_frame(), ctx.init_window()
    P0, C0 = _decode(capi, frame, pts, curv)
    assert len(P0) > 5 * 256
    if not det:
        assert len(np.unique(C0)) < len(C0) // 20
    down_size = 0.1
    idx = np.sort(ctx.down_sampling_close(P0, down_size))
    assert 1000 < len(idx) < len(P0)
    n_kept, retried = win.push(frame, down_size, 1000)
    assert (n_kept, retried) == (len(idx), 0)
    assert win.size() == 1 and np.array_equal(win.offsets(), [0, len(idx)])
    gp, gc = win.read(0)
    assert np.array_equal(gp, P0[idx]) and np.array_equal(gc, C0[idx])
    assert np.all(np.diff(gc) >= 0)
    # stage 0 survives the push: a second push appends the same scan again
    assert win.push(frame, down_size, 1000) == (len(idx), 0)
    gp2, gc2 = win.read(1)
    assert np.array_equal(gp2, gp) and np.array_equal(gc2, gc)
    ctx.close()


# ---------------------------------------------------------------- 2. the retry and its boundary

def test_retry_and_its_boundary(capi, synth):
    ctx = _ctx(capi, tmi._wl(synth), deterministic=1)
    frame, win = ctx.scan_frame(), ctx.init_window()
    # 999 voxels x 3 points: 999 < 1000 retries from the full cloud at half the size
    P0, C0 = _decode(capi, frame, *iwo.grid_cloud(999))
    assert len(P0) == 2997 and len(ctx.down_sampling_close(P0, 0.5)) == 999
    wp, wc, idx, want_retry = _host_route(ctx, P0, C0, 0.5, 1000)
    assert want_retry and np.array_equal(idx, np.sort(ctx.down_sampling_close(P0, 0.25))) and len(idx) > 999
    assert win.push(frame, 0.5, 1000) == (len(idx), 1)
    gp, gc = win.read(0)
    assert np.array_equal(gp, wp) and np.array_equal(gc, wc)
    # min_points = 0 never retries
    assert win.push(frame, 0.5, 0) == (999, 0)
    gp, gc = win.read(1)
    i1 = np.sort(ctx.down_sampling_close(P0, 0.5))
    assert np.array_equal(gp, P0[i1]) and np.array_equal(gc, C0[i1])
    # down_size below a millimetre copies the cloud whole, on both passes
    assert win.push(frame, 0.0005, 0) == (len(P0), 0)
    gp, gc = win.read(2)
    assert np.array_equal(gp, P0) and np.array_equal(gc, C0)
    assert win.push(frame, 0.0005, 5000) == (len(P0), 1)
    gp, gc = win.read(3)
    assert np.array_equal(gp, P0) and np.array_equal(gc, C0)
    # 1000 voxels x 3 points: exactly min_points does not retry
    P1, C1 = _decode(capi, frame, *iwo.grid_cloud(1000))
    assert win.push(frame, 0.5, 1000) == (1000, 0)
    gp, gc = win.read(4)
    i2 = np.sort(ctx.down_sampling_close(P1, 0.5))
    assert len(i2) == 1000 and np.array_equal(gp, P1[i2]) and np.array_equal(gc, C1[i2])
    assert np.array_equal(win.offsets(), np.cumsum([0, len(idx), 999, len(P0), len(P0), 1000]))
    ctx.close()


# ---------------------------------------------------------------- 3. degenerate frames and arguments

def test_degenerate_frames_and_arguments(capi, synth, small):
    wl = tmi._wl(synth)
    ctx = _ctx(capi, wl, deterministic=1)
    frame, win = ctx.scan_frame(), ctx.init_window()
    pts, curv = small
    # every time beyond the cut: the decode's n = 0, an empty scan
    lay, msg = _message(capi, pts[:300], np.full(300, 0.115))
    assert frame.decode(lay, msg, 1, 0.0)[0] == 0
    assert win.push(frame, 0.1, 1000) == (0, 0)
    assert win.size() == 1 and np.array_equal(win.offsets(), [0, 0])
    gp, gc = win.read(0)
    assert gp.shape == (0, 3) and gc.shape == (0,)
    # an undecoded frame
    fresh = ctx.scan_frame()
    with pytest.raises(capi.VbaError) as e:
        win.push(fresh, 0.1, 1000)
    assert e.value.status == capi.ERR_BAD_ARG
    assert win.size() == 1 and np.array_equal(win.offsets(), [0, 0])
    # descending curvature in a host array
    with pytest.raises(capi.VbaError) as e:
        win.push_points(pts[:3], [0.01, 0.03, 0.02])
    assert e.value.status == capi.ERR_BAD_ARG and win.size() == 1
    # a window of W - 1 scans: refused before any device work, the context's map stays as it was
    d = synth.make_init_window(win_size=W, n_pts=300, scene="room")
    win.clear()
    for i in range(W - 1):
        win.push_points(d["clouds"][i], d["curvs"][i])
    pose = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    ctx.cut_voxel(0, pts, pose)
    before, leaves = ctx.map_stats(), ctx.dump_leaves()
    assert ctx.num_roots() > 0
    ip = np.zeros((W - 1, 304))
    with pytest.raises(capi.VbaError) as e:
        _resident(ctx, win, wl, d, ip)
    assert e.value.status == capi.ERR_BAD_ARG
    assert ctx.map_stats() == before and np.array_equal(ctx.dump_leaves(), leaves)
    assert win.size() == W - 1
    ctx.close()


# ---------------------------------------------------------------- 4. append, growth, clear, reservation

def test_append_growth_clear_and_reservation(capi, oracle, room):
    wl, d, ip, _ = room
    ctx = _ctx(capi, wl, deterministic=1)
    frame = ctx.scan_frame()
    win = ctx.init_window()
    sizes = [0.0005 if i % 2 == 0 else 0.05 * (1 + i) for i in range(W)]   # whole clouds (the rows pass the first block) and thinned ones
    want, n_max = [], 0
    for i in range(W):
        P0, C0 = _decode(capi, frame, d["clouds"][i], d["curvs"][i])
        n_max = max(n_max, len(P0))
        wp, wc, idx, retried = _host_route(ctx, P0, C0, sizes[i], 1000)
        assert win.push(frame, sizes[i], 1000) == (len(idx), int(retried))
        want.append((wp, wc))
    lens = [len(p) for p, _ in want]
    assert len(set(lens)) >= 4 and sum(lens) > 65536                       # the window grew at least once on the way
    assert win.size() == W and np.array_equal(win.offsets(), np.cumsum([0] + lens))
    for k in range(W):                                                    # growth kept the earlier scans
        gp, gc = win.read(k)
        assert np.array_equal(gp, want[k][0]) and np.array_equal(gc, want[k][1]), k
    allocs = win.allocations()
    assert allocs[0] > 3 and allocs[1] >= sum(lens) * 32
    win.clear()
    assert win.size() == 0 and np.array_equal(win.offsets(), [0]) and win.allocations() == allocs
    # inside a reservation nothing allocates: W pushes and one resident call
    win2 = ctx.init_window()
    win2.reserve(W, n_max)
    frame.reserve(n_max, 20)
    a0, f0 = win2.allocations(), frame.allocations()
    for i in range(W):
        lay, msg = _message(capi, d["clouds"][i], d["curvs"][i])
        frame.decode(lay, msg, 1, 0.0)
        win2.push(frame, sizes[i], 1000)
    res = _resident(ctx, win2, wl, d, ip)
    assert res["iterations"] >= 1
    assert win2.allocations() == a0 and frame.allocations() == f0
    assert np.array_equal(win2.offsets(), np.cumsum([0] + lens))
    ctx.close()


# ---------------------------------------------------------------- 5. the resident call equals vba_motion_init, bit for bit

def _both(capi, wl, d, ip, point_notime=False):
    ca = _ctx(capi, wl, deterministic=1)
    a = tmi._run_dev(ca, wl, d, ip, point_notime=point_notime)
    da = ca.dump_leaves()
    ca.close()
    cb = _ctx(capi, wl, deterministic=1)
    win = cb.init_window()
    for i in range(W):
        win.push_points(d["clouds"][i], d["curvs"][i])
    b = _resident(cb, win, wl, d, ip, point_notime=point_notime)
    db = cb.dump_leaves()
    assert win.size() == W                                                # the call does not clear the window
    cb.close()
    return a, da, b, db


@pytest.mark.parametrize("case", ["room", "point_notime", "one_scan_empty"])
def test_resident_equals_motion_init_bit_for_bit(capi, room, case):
    wl, d, ip, ref = room
    if case == "one_scan_empty":
        d = dict(d)
        d["clouds"] = [c if i != 4 else np.zeros((0, 3)) for i, c in enumerate(d["clouds"])]
        d["curvs"] = [c if i != 4 else np.zeros(0) for i, c in enumerate(d["curvs"])]
    a, da, b, db = _both(capi, wl, d, ip, point_notime=(case == "point_notime"))
    if case == "room":                                                    # both walk cases: point 0 pushed again, leading points dropped
        assert a["converged"] == 1 and a["iterations"] >= 3
        assert any(len(p[0]) > len(c) for p, c in zip(a["pvec"], d["clouds"])) and any(len(p[0]) < len(c) for p, c in zip(a["pvec"], d["clouds"]))
    assert a["round_log"][0, 0] >= 10                                     # the LM ran
    _assert_same_result(a, b)
    assert np.array_equal(da, db)


# ---------------------------------------------------------------- 6. end to end: raw messages -> decode -> push -> resident call

E2E_DOWN_SIZE = 0.1     # the CPU oracle replay of the host-fed window at this size starts its LM (see the test)


def test_end_to_end_from_raw_messages(capi, room):
    wl, d, ip, _ = room
    cb = _ctx(capi, wl, deterministic=1)
    frame, win = cb.scan_frame(), cb.init_window()
    clouds, curvs = [], []
    for i in range(W):
        P0, C0 = _decode(capi, frame, d["clouds"][i], d["curvs"][i])
        wp, wc, idx, retried = _host_route(cb, P0, C0, E2E_DOWN_SIZE, 1000)
        assert win.push(frame, E2E_DOWN_SIZE, 1000) == (len(idx), int(retried))
        clouds.append(wp); curvs.append(wc)
    dd = dict(d)
    dd["clouds"], dd["curvs"] = clouds, curvs
    ca = _ctx(capi, wl, deterministic=1)
    a = tmi._run_dev(ca, wl, dd, ip)
    assert a["round_log"][0, 0] >= 10, a["round_log"]                     # a condition on the input: the host-fed run started its LM
    b = _resident(cb, win, wl, dd, ip)
    _assert_same_result(a, b)
    assert np.array_equal(ca.dump_leaves(), cb.dump_leaves())
    ca.close(); cb.close()


# ---------------------------------------------------------------- 7. default mode against the oracle

def test_default_mode_against_the_oracle(capi, room):
    wl, d, ip, ref = room
    ctx = _ctx(capi, wl)
    win = ctx.init_window()
    for i in range(W):
        win.push_points(d["clouds"][i], d["curvs"][i])
    a = _resident(ctx, win, wl, d, ip)
    tmi._compare(a, ref, pnt_bar=1e-12, var_bar=1e-9)
    ctx.close()


# ---------------------------------------------------------------- 8. harness mode 8

def test_harness_mode8(capi, room, tmp_path):
    """raw messages -> vba::ScanFrame::decode -> vba::InitWindow::push -> the InitWindow overload of motion_init, against the same
    sequence from Python; deterministic on both sides, at the bars test_harness_mode3 uses for its initialisation record."""
    harness = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-slam_amd", "vba_harness")
    assert os.path.exists(harness)
    wl, d, ip, _ = room
    ctx = _ctx(capi, wl, deterministic=1)
    frame, win = ctx.scan_frame(), ctx.init_window()
    lay = capi.scan_layout("livox")
    head = [20241004.0, W, W, 8, wl.voxel_size, wl.max_layer, wl.max_points, wl.min_eigen_value, *wl.plane_thre, *wl.min_point,
            wl.imu_coef, 5, 0, wl.dept_err, wl.beam_err, d["scale_gravity"], *d["ext"],
            E2E_DOWN_SIZE, 1000, 1, 0.0, lay.point_step, lay.off_x, lay.off_y, lay.off_z, lay.off_intensity, lay.intensity_type, lay.off_time,
            lay.time_type, lay.filter]
    chunks = [np.array(head, dtype=np.float64)]
    kept = []
    for i in range(W):
        _, msg = _message(capi, d["clouds"][i], d["curvs"][i])
        frame.decode(lay, msg, 1, 0.0)
        kept += list(win.push(frame, E2E_DOWN_SIZE, 1000))
        n_raw = len(msg) // lay.point_step
        words = np.zeros((len(msg) + 7) // 8 * 8, dtype=np.uint8)
        words[:len(msg)] = msg
        chunks.append(np.concatenate([[n_raw, len(words) // 8, len(d["imus"][i]), d["beg_times"][i]], d["states"][i], d["covs"][i].ravel()]))
        chunks += [words.view(np.float64), d["imus"][i].ravel()]
    chunks.append(np.concatenate([NM, NW]))
    b = _resident(ctx, win, wl, d, ip)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for c in chunks:
            f.write(np.ascontiguousarray(c, dtype=np.float64).tobytes())
    r = subprocess.run([harness, fin, fout, "--deterministic"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(fout, dtype=np.float64)
    assert out[0] == -2 and out[1] == b["converged"] and out[2] == b["iterations"] and out[3] == b["thresholds_left_relaxed"]
    assert b["round_log"][0, 0] >= 10
    assert tmi._rel(out[4:7], b["eigvalue3"]) < 1e-6
    assert np.abs(out[7:7 + W * 25].reshape(W, 25) - b["states"]).max() < 1e-6
    q = 7 + W * 25
    assert np.array_equal(out[q:q + 2 * W], np.array(kept, dtype=np.float64))
    assert out[q + 2 * W] == -1
    ctx.close()
