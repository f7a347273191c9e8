"""Harness mode 6: build_graph (VS:2078-2156) + topDownProcess's gba edges (VS:2733-2764) + ISAM2 + set_state (LR:36-43) driven
through include/voxelba_adapter.hpp (vba::PoseGraph, vba::set_state) by voxel-slam_amd/harness/local_mapping_harness.cpp over two
sessions, against the same graph solved by tests/pgo_oracle.py and the velocity rotation of set_state restated in numpy."""
import os
import subprocess

import numpy as np
import pytest

import pgo_oracle as po
from test_gpu_pgo import cost_floor, cost_rel, pose_diff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "voxel-slam_amd", "vba_harness")


@pytest.mark.parametrize("lpedge_enable", [1, 0])
def test_mode6_matches_oracle(tmp_path, lpedge_enable):
    rng = np.random.default_rng(21)
    sizes = [120, 90]
    step = [0, sizes[0], sizes[0] + sizes[1]]
    truth, init, states, v6s = [], [], [], []
    for s, n in enumerate(sizes):
        X = po.trajectory(rng, n)
        if s:
            X = np.array([po.compose(po.exp6(np.array([0, 0, 0.2, 3.0, 1.0, 0])), x) for x in X])
        Y = po.drift(rng, X)
        st = np.zeros((n, 25))
        st[:, 0] = 100.0 * s + np.arange(n) * 0.1
        st[:, 1:10] = Y[:, :9]; st[:, 10:13] = Y[:, 9:]
        st[:, 13:16] = rng.normal(size=(n, 3))                    # velocities (turned by set_state)
        st[:, 16:25] = rng.normal(size=(n, 9)) * 1e-3
        truth.append(X); init.append(Y); states.append(st); v6s.append(10.0 ** rng.uniform(-6, -3, (n, 6)))
    X = np.concatenate(truth)
    # loop edges (m1, m2, id1, id2, rot, tra) and gba edges (+ v6) with scan ids, keyframes every 10 scans
    loops = []
    for (m1, i1), (m2, i2) in [((0, 30), (1, 20)), ((0, 100), (1, 80)), ((0, 60), (0, 10))]:
        rot, tra = po.relative(X[step[m1] + i1], X[step[m2] + i2])
        loops.append(np.concatenate([[m1, m2, i1, i2], rot, tra]))
    gba = []
    for s, n in enumerate(sizes):
        kfs = list(range(0, n, 10))
        for a in range(len(kfs)):
            for b in range(a + 1, min(a + 4, len(kfs))):
                rot, tra = po.relative(X[step[s] + kfs[a]], X[step[s] + kfs[b]])
                gba.append(np.concatenate([[s, s, kfs[a], kfs[b]], rot, tra, 10.0 ** rng.uniform(-6, -4, 6)]))
    rot, tra = po.relative(X[step[0] + 110], X[step[1] + 0])     # a cross-session row: the sessions stay connected without loops
    gba.append(np.concatenate([[0, 1, 110, 0], rot, tra, np.full(6, 1e-5)]))
    n_upd, thr = 6, 0.01
    head = [20241004.0, 0, 2, 6, lpedge_enable, n_upd, thr]
    parts = [np.array(head)]
    for s in range(2):
        parts += [np.array([sizes[s]], float), states[s].ravel(), v6s[s].ravel()]
    parts += [np.array([len(loops)], float), np.array(loops).ravel(), np.array([len(gba)], float), np.array(gba).ravel()]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(parts).astype(np.float64).tofile(inp)
    subprocess.run([HARNESS, str(inp), str(outp)], check=True, timeout=600)
    got = np.fromfile(outp, dtype=np.float64)
    N = step[-1]
    gst = got[N * 25:].reshape(n_upd, 3)
    got = got[:N * 25].reshape(N, 25)
    # the same graph for the oracle, in build_graph's order
    Y = np.concatenate(init)
    V6 = np.concatenate(v6s)
    ed = []
    for s in range(2):
        for j in range(step[s] + 1, step[s + 1]):
            ed.append(po.edge_row(j - 1, j, Y[j - 1], Y[j], V6[j - 1]))
    if lpedge_enable:
        for r in loops:
            ed.append(np.concatenate([[step[int(r[0])] + r[2], step[int(r[1])] + r[3]], r[4:16], np.full(6, 1e-4)]))
    for r in gba:
        ed.append(np.concatenate([[step[int(r[0])] + r[2], step[int(r[1])] + r[3]], r[4:22]]))
    pr = np.array([po.prior_row(0, Y[0], np.full(6, 1e-9))])
    want, wst, deltas = po.optimize(Y, np.array(ed), pr, n_upd, thr)
    assert po.relin_margin(deltas, thr) > 1e-6
    gp = np.concatenate([got[:, 1:10], got[:, 10:13]], axis=1)
    rot, tra = pose_diff(gp, want)
    cost = cost_rel(gst[:, 1], wst[:, 1], cost_floor(Y, np.array(ed), pr))
    print("   cost per update: device %s oracle %s" % (gst[:, 1].tolist(), wst[:, 1].tolist()))
    print("mode 6 (loops %d): rot %.3g rad, tra %.3g, cost rel %.3g" % (lpedge_enable, rot, tra, cost))
    assert rot <= 1e-9 and tra <= 1e-9 and cost <= 1e-9
    np.testing.assert_array_equal(gst[:, 0], wst[:, 0])
    # set_state (LR:36-43): v <- R_new R_old^T v; time, biases and gravity untouched
    S0 = np.concatenate(states)
    for k in range(N):
        rot_chg = want[k, :9].reshape(3, 3) @ S0[k, 1:10].reshape(3, 3).T
        np.testing.assert_allclose(got[k, 13:16], rot_chg @ S0[k, 13:16], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(got[:, 0], S0[:, 0])
    np.testing.assert_array_equal(got[:, 16:25], S0[:, 16:25])
