"""Harness mode 4: the loop-detection step of the loop-closure thread (VS:2404-2541) driven through include/voxelba_adapter.hpp
(vba::BtcDatabase, vba::icp_normal) by voxel-slam_amd/harness/local_mapping_harness.cpp over a synthetic two-session stream, against
the same sequence replayed on the numpy restatement tests/btc_oracle.py: per keyframe and session, the detection, the score, whether
ICP ran, its outcome, iterations and pose."""
import os
import subprocess

import numpy as np
import pytest

import btc_oracle as bo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "voxel-slam_amd", "vba_harness")
REC = 23


def test_mode4_matches_oracle(tmp_path):
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth
    n_kf, juds, icp_eigval = 60, [0.2, 0.2], 0.05
    S = synth.make_btc_sessions(n_sessions=2, n_kf=n_kf, seed=4)
    head = [20241004.0, 0, 2 * n_kf, 4, 0, icp_eigval, 2, *juds]
    parts = [np.array(head)]
    for s in range(2):
        for k in range(n_kf):
            rows, bits, cl = S[s]["rows"][k], S[s]["bits"][k], S[s]["cloud"][k]
            assert int(bits.max()) < 2 ** 53
            parts += [np.array([s, len(rows), len(cl)], float), rows.ravel(), bits.astype(np.float64).ravel(), cl.astype(np.float64).ravel()]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(parts).astype(np.float64).tofile(inp)
    subprocess.run([HARNESS, str(inp), str(outp)], check=True, timeout=600)
    got = np.fromfile(outp, dtype=np.float64).reshape(-1, REC)
    # the oracle replay of the same step
    cfg = bo.read_parameters(0)
    dbs, want = [], []
    for s in range(2):
        if dbs:
            dbs[-1].cfg["skip_near_num"] = -(len(dbs[-1].clouds) + 10)
        dbs.append(bo.BtcDb(cfg))
        cur = dbs[-1]
        for k in range(n_kf):
            rows, bits, cl = S[s]["rows"][k], S[s]["bits"][k], S[s]["cloud"][k]
            cur.push_plane_cloud(cl, k)
            for i, d in enumerate(dbs):
                r, _ = d.search_loop(rows, bits, cl)
                ran = int(r["loop_id"] >= 0 and r["score"] > juds[i])
                t = r["t"] if r["t"] is not None else None
                rec = dict(key=(s, k, i), loop_id=r["loop_id"], score=r["score"], ran=ran, t=t, R=r["R"])
                if ran:
                    o = bo.icp_normal(cl, d.clouds[r["loop_id"]], r["t"], r["R"], icp_eigval)
                    rec.update(ok=o["ok"], iters=o["iters"], t=o["t"], R=o["R"])
                want.append(rec)
            cur.add_stds(rows, bits)
    assert len(got) == len(want)
    icps = full = 0
    for g, w in zip(got, want):
        assert tuple(int(v) for v in g[0:3]) == w["key"]
        assert int(g[3]) == w["loop_id"] and g[4] == w["score"] and int(g[5]) == w["ran"]
        if w["loop_id"] >= 0 and not w["ran"]:                      # SearchLoop's transform
            assert np.abs(g[8:11] - w["t"]).max() < 1e-9 and np.abs(g[11:20].reshape(3, 3) - w["R"]).max() < 1e-9
        if w["ran"]:
            icps += 1
            assert int(g[6]) == w["ok"]
            # A registration the reference itself rejects (eig[0] <= icp_eigval: mat_norm degenerate) has a near-singular 6x6 system;
            # its iterates depend on the last bits of the sums and the loop discards its pose.  Iterations and pose are compared
            # where the reference accepts the loop.
            if w["ok"]:
                full += 1
                assert int(g[7]) == w["iters"]
                assert np.abs(g[8:11] - w["t"]).max() < 1e-9 and np.abs(g[11:20].reshape(3, 3) - w["R"]).max() < 1e-9
    assert icps > 0 and full > 0
    assert any(w["loop_id"] >= 0 and w["key"][2] == 0 and w["key"][0] == 1 for w in want)   # a cross-session loop
