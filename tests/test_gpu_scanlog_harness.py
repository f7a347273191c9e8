"""Harness modes 7 and 9 (voxel-slam_amd/harness/local_mapping_harness.cpp) on one input with --deterministic: the session of mode 7
with a vba::ScanLog in place of the host ScanPose::pvec (push before multi_margi, keyframes built from the log, loop_update from the
log, release after each build).  Every output field that does not derive from a point covariance is equal bit for bit.

Left out of the comparison, because they derive from the point covariances: the keyframes' diag rows (normal_x/y/z) and the
plane-covariance dump of the final map.  Mode 7's host route passes the covariances of the INPUT on to the keyframes and to
loop_update, mode 9 the world covariances the map's ring holds (what the reference's pvec_update leaves in pv.var, VH:259);
tests/test_gpu_scanlog.py holds the log's covariance values against vba_kf_build and vba_loop_update fed with the same arrays."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import loop_oracle as lo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "voxel-slam_amd", "vba_harness")


def _problem(synth, oracle, W, nscan, n_pts):
    """nscan scans of the room along one trajectory with body covariances from the measurement model, a state covariance and IMU
    samples between the scans (the per-scan input of the harness)"""
    wl = dataclasses.replace(synth.CONFIGS["room20k_w4"], win_size=W, n_pts=n_pts)
    big = dataclasses.replace(wl, win_size=nscan)
    s = synth.make_scans(big)
    imu_samples, vel, g = synth.make_imu(big, gyr_sigma=1e-3, acc_sigma=1e-2)
    ext = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    rng = np.random.default_rng(9)
    A = rng.normal(0, 0.002, (15, 15)); cov = A @ A.T + np.eye(15) * 1e-6
    scans = []
    for k in range(nscan):
        st = np.zeros(25)
        st[0] = 0.1 * k; st[1:10] = s["R0"][k].ravel(); st[10:13] = s["p0"][k]; st[13:16] = vel[k]; st[22:25] = g
        p, vb = oracle.var_init(s["points"][k], ext, wl.dept_err, wl.beam_err)
        scans.append(dict(state=st, pts=p, var_body=vb, imu=imu_samples[k - 1] if k > 0 else None))
    return wl, scans, cov


def _write_input(path, wl, scans, cov, mode, n_loop, kf_every, dx):
    head = [20241004.0, wl.win_size, len(scans), mode, wl.voxel_size, wl.max_layer, wl.max_points, wl.min_eigen_value,
            *wl.plane_thre, *wl.min_point, wl.imu_coef, 5, n_loop, kf_every, *dx]
    chunks = [np.array(head, dtype=np.float64)]
    for sc in scans:
        n_imu = 0 if sc["imu"] is None else len(sc["imu"][0])
        chunks.append(np.concatenate([[len(sc["pts"])], sc["state"], cov.ravel(), [n_imu]]))
        chunks.append(sc["pts"].ravel()); chunks.append(sc["var_body"].ravel())
        if n_imu:
            t, gy, ac = sc["imu"]
            chunks += [t.ravel(), gy.ravel(), ac.ravel()]
    chunks.append(np.array([0.01] * 3 + [1.0] * 3 + [1e-4] * 6))
    np.concatenate(chunks).astype(np.float64).tofile(path)


def _parse(out, W, n_loop, nscan):
    """the output of modes 7 and 9 -> dict of its fields"""
    q = 0
    steps, rec = [], None
    for k in range(nscan):
        if k == n_loop:
            assert out[q] == -3
            rec = dict(n_ins=int(out[q + 1]), nf=int(out[q + 2]), n_kf=int(out[q + 3]), kf=[]); q += 4
            for _ in range(rec["n_kf"]):
                n = int(out[q]); x0 = out[q + 1:q + 13].copy(); q += 13
                xyz = out[q:q + 3 * n].copy(); q += 3 * n
                diag = out[q:q + 3 * n].copy(); q += 3 * n
                rec["kf"].append(dict(n=n, x0=x0, xyz=xyz, diag=diag))
            kb = int(out[q]); q += 1
            rec["bl"] = out[q:q + 26 * kb].copy(); q += 26 * kb
            wc = int(out[q]); q += 1
            rec["win"] = out[q:q + 25 * wc].copy(); q += 25 * wc
        if k >= W - 1:
            assert out[q] == k
            steps.append(out[q:q + 7 + 25 * W].copy()); q += 7 + 25 * W
    assert out[q] == -1
    nl = int(out[q + 1]); q += 2
    leaves = out[q:q + nl * 39].reshape(nl, 39); q += nl * 39
    pv = out[q:q + nl * 86].reshape(nl, 86); q += nl * 86
    assert q == len(out)
    return dict(steps=steps, rec=rec, leaves=leaves, pv=pv)


def test_mode_9_equals_mode_7(oracle, tmp_path):
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth
    assert os.path.exists(HARNESS), "voxel-slam_amd/vba_harness must be built in-tree by __graft_entry__.build()"
    W, nscan, n_loop, kf_every = 4, 10, 8, 2
    wl, scans, cov = _problem(synth, oracle, W, nscan, 6000)
    x1 = scans[5]["state"]; x3 = x1.copy()
    x3[1:10] = (synth.so3_exp(np.array([0.004, -0.003, 0.012])) @ x1[1:10].reshape(3, 3)).ravel()
    x3[10:13] = x1[10:13] + np.array([0.06, -0.04, 0.015])
    dx = lo.loop_dx(x1, x3)
    res = {}
    for mode in (7, 9):
        fin, fout = str(tmp_path / ("in%d.bin" % mode)), str(tmp_path / ("out%d.bin" % mode))
        _write_input(fin, wl, scans, cov, mode, n_loop, kf_every, dx)
        r = subprocess.run([HARNESS, fin, fout, "--deterministic"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        res[mode] = _parse(np.fromfile(fout, dtype=np.float64), W, n_loop, nscan)
    a, b = res[7], res[9]
    # the window states and v6 of every local-mapping step, before and after the loop closure
    assert len(a["steps"]) == len(b["steps"]) == nscan - W + 1
    for sa, sb in zip(a["steps"], b["steps"]):
        assert np.array_equal(sa, sb), int(sa[0])
    # the loop closure's record: n_ins, nf, the keyframe count; the keyframes' poses, sizes and points; the bl and window lists
    ra, rb = a["rec"], b["rec"]
    assert (ra["n_ins"], ra["nf"], ra["n_kf"]) == (rb["n_ins"], rb["nf"], rb["n_kf"]) and ra["n_kf"] >= 2 and ra["nf"] > 50
    for ka, kb in zip(ra["kf"], rb["kf"]):
        assert ka["n"] == kb["n"] > 0 and np.array_equal(ka["x0"], kb["x0"]) and np.array_equal(ka["xyz"], kb["xyz"])
    assert len(ra["bl"]) > 0 and np.array_equal(ra["bl"], rb["bl"]) and np.array_equal(ra["win"], rb["win"])
    # the final map: the fields of the leaf dump (keys, counts, flags, point sums, plane centres and normals), not the plane covariances
    assert len(a["leaves"]) == len(b["leaves"]) > 100 and np.array_equal(a["leaves"], b["leaves"])
    # the covariance-derived fields are NOT compared (see the module's docstring); they do differ, which shows that mode 9 reads the map's values
    assert any(not np.array_equal(ka["diag"], kb["diag"]) for ka, kb in zip(ra["kf"], rb["kf"]))
