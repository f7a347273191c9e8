"""Harness mode 10: the initialisation phase on a vba::OdomState through include/voxelba_adapter.hpp, per scan
raw message -> ScanFrame::decode -> OdomState::propagate -> OdomState::prepare -> OdomState::lio_state_estimation_kdtree ->
vba::pub_localtraj -> IMU_PRE::push_imu -> InitWindow::push, then the InitWindow overload of motion_init, against the same sequence
driven from Python through capi on a deterministic context.  Both sides make the same library calls in the same order: what the
odometry produces per scan (iterations, states, kept and retried counts, the published scan's count and checksum) must be EQUAL; the
initialisation record is held to the bars of test_gpu_init_window.py::test_harness_mode8.  Whether motion_init converges on states
that the odometry produced is recorded (printed), not asserted."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_motion_init as tmi
from scan_export_ref import checksum
from test_gpu_init_window import E2E_DOWN_SIZE, NM, NW, W, _ctx, _message, capi, synth  # noqa: F401  (fixtures of this module too)

pytestmark = pytest.mark.gpu

EKF_NOISE = np.array([0.1] * 3 + [0.1] * 3 + [1e-4] * 3 + [1e-4] * 3)        # cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc


@pytest.fixture(scope="module")
def scene(synth):
    """the room window of test_gpu_init_window.py (W = 10, 20 000 points per scan) without its CPU oracle replay, which nothing here
    is compared with and which takes longer than the test"""
    return tmi._wl(synth), synth.make_init_window(win_size=W, n_pts=20000, scene="room")


def _x0(d):
    """x_curr before the first scan: the pose at t = 0 of the generator (constant velocity, no rotation yet), the window's gravity"""
    g = d["gt_states"][0]
    x = np.zeros(25)
    x[1:10] = np.eye(3).ravel()
    x[13:16] = g[13:16]
    x[10:13] = g[10:13] - g[0] * g[13:16]
    x[22:25] = g[22:25]
    cov = np.eye(15) * 1e-4
    cov[9:, 9:] = np.eye(6) * 1e-5
    return x, cov


def test_harness_mode10(capi, scene, tmp_path):
    harness = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-slam_amd", "vba_harness")
    assert os.path.exists(harness)
    wl, d = scene
    sg = d["scale_gravity"]
    x0, cov0 = _x0(d)
    ctx = _ctx(capi, wl, deterministic=1)
    frame, win, st = ctx.scan_frame(), ctx.init_window(), ctx.odom_state()
    lay = capi.scan_layout("livox")
    head = [20241004.0, W, W, 10, wl.voxel_size, wl.max_layer, wl.max_points, wl.min_eigen_value, *wl.plane_thre, *wl.min_point,
            wl.imu_coef, 5, 0, wl.dept_err, wl.beam_err, sg, *d["ext"],
            E2E_DOWN_SIZE, 1000, 1, 0.0, lay.point_step, lay.off_x, lay.off_y, lay.off_z, lay.off_intensity, lay.intensity_type, lay.off_time,
            lay.time_type, lay.filter, *EKF_NOISE, *x0, *cov0.ravel()]
    chunks = [np.array(head, dtype=np.float64)]
    st.set(x0, cov0)
    per_scan, states, ip = [], [], []
    end = 0.0
    for i in range(W):
        _, msg = _message(capi, d["clouds"][i], d["curvs"][i])
        imu = d["imus"][i]
        beg = float(d["beg_times"][i])
        last_end, end = min(end, beg), float(d["gt_states"][i][0])
        n_raw = len(msg) // lay.point_step
        words = np.zeros((len(msg) + 7) // 8 * 8, dtype=np.uint8)
        words[:len(msg)] = msg
        chunks += [np.array([n_raw, len(words) // 8, len(imu), last_end, beg, end]), words.view(np.float64), imu.ravel()]
        # the same calls from Python
        frame.decode(lay, msg, 1, 0.0)
        assert st.propagate(imu, EKF_NOISE, last_end, beg, end, sg) > 0
        n, dp, _ = st.prepare(frame, d["ext"], max(E2E_DOWN_SIZE, 0.5), wl.dept_err, wl.beam_err, min_points=0)
        it, rep, x = st.lio_state_estimation_kdtree(ctx, n, dp)
        rec = st.export_scan(ctx, n, dp, 0.0)
        if i > 0:
            ip.append(capi.imu_preintegrate(imu[:, 0], imu[:, 1:4], imu[:, 4:7], states[-1][16:19], states[-1][19:22], NM, NW, sg))
        states.append(x)
        kept, retried = win.push(frame, E2E_DOWN_SIZE, 1000)
        per_scan.append(np.concatenate([[it], x, [kept, retried, len(rec), checksum(rec)]]))
        print("scan %d: %d points prepared, iterations %d, valid %s, kept %d, |p - gt| %.3g" % (
            i, n, it, rep["match_num"][:it], kept, np.linalg.norm(x[10:13] - d["gt_states"][i][10:13])))
    chunks.append(np.concatenate([NM, NW]))
    assert per_scan[0][0] == 0 and all(p[0] >= 2 for p in per_scan[1:])            # the first scan seeded the map, the others estimated
    b = ctx.motion_init_resident(win, d["imus"], d["beg_times"], d["ext"], wl.dept_err, wl.beam_err, sg, NM, NW, np.array(states),
                                 np.array([cov0] * W), np.array(ip), want_hess=True)
    print("motion_init on the produced states: converged %d, iterations %d, eigvalue %s" % (b["converged"], b["iterations"], b["eigvalue3"]))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for c in chunks:
            f.write(np.ascontiguousarray(c, dtype=np.float64).tobytes())
    r = subprocess.run([harness, fin, fout, "--deterministic"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(fout, dtype=np.float64)
    assert out[0] == -2 and out[1] == b["converged"] and out[2] == b["iterations"] and out[3] == b["thresholds_left_relaxed"]
    if np.any(b["eigvalue3"]):
        assert tmi._rel(out[4:7], b["eigvalue3"]) < 1e-6
    else:
        assert not np.any(out[4:7])
    assert np.abs(out[7:7 + W * 25].reshape(W, 25) - b["states"]).max() < 1e-6
    q = 7 + W * 25
    got = out[q:q + W * 30].reshape(W, 30)
    assert np.array_equal(got, np.array(per_scan))
    assert out[q + W * 30] == -1
    ctx.close()
