"""Harness mode 5: the loop-detection step of the loop-closure thread with descriptor generation (VS:2404-2541: GenerateSTDescs,
SearchLoop over the sessions, icp_normal, AddSTDescs) driven through include/voxelba_adapter.hpp (vba::BtcDatabase::GenerateSTDescs,
vba::icp_normal) by voxel-slam_amd/harness/local_mapping_harness.cpp over two sessions of keyframe clouds, against the same sequence
replayed on the numpy restatements tests/btc_gen_oracle.py (generation) and tests/btc_oracle.py (retrieval, ICP)."""
import os
import subprocess

import numpy as np
import pytest

import btc_gen_oracle as bg
import btc_oracle as bo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "voxel-slam_amd", "vba_harness")
REC = 23


def test_mode5_matches_oracle(tmp_path):
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth
    n_kf, juds, icp_eigval = 8, [0.2, 0.2], 0.05
    S = synth.make_btc_keyframe_sessions(n_sessions=2, n_kf=n_kf, n_points=100000, seed=8)
    head = [20241004.0, 0, 2 * n_kf, 5, 0, icp_eigval, 2, *juds]
    parts = [np.array(head)]
    for s in range(2):
        for k in range(n_kf):
            cl = S[s]["cloud"][k]
            parts += [np.array([s, len(cl)], float), cl.astype(np.float64).ravel()]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(parts).astype(np.float64).tofile(inp)
    subprocess.run([HARNESS, str(inp), str(outp)], check=True, timeout=600)
    got = np.fromfile(outp, dtype=np.float64).reshape(-1, REC)
    # the restatement replaying the same sequence
    gcfg = bg.read_parameters(0)
    cfg = bo.read_parameters(0)
    dbs, want = [], []
    for s in range(2):
        if dbs:
            dbs[-1].cfg["skip_near_num"] = -(len(dbs[-1].clouds) + 10)
        dbs.append(bo.BtcDb(cfg))
        cur = dbs[-1]
        for k in range(n_kf):
            g = bg.generate_stds(S[s]["cloud"][k], k, gcfg)          # frame_number_ = AddSTDescs count = k
            rows, bits, pl = g["rows"], g["bits"], g["planes"]
            cur.push_plane_cloud(pl, k)
            for i, d in enumerate(dbs):
                r, _ = d.search_loop(rows, bits, pl)
                ran = int(r["loop_id"] >= 0 and r["score"] > juds[i])
                rec = dict(key=(s, k, i), loop_id=r["loop_id"], score=r["score"], ran=ran, t=r["t"], R=r["R"])
                if ran:
                    o = bo.icp_normal(pl, d.clouds[r["loop_id"]], r["t"], r["R"], icp_eigval)
                    rec.update(ok=o["ok"], iters=o["iters"], t=o["t"], R=o["R"])
                want.append(rec)
            cur.add_stds(rows, bits)
    assert len(got) == len(want)
    loops = icps = full = 0
    for g, w in zip(got, want):
        assert tuple(int(v) for v in g[0:3]) == w["key"]
        assert int(g[3]) == w["loop_id"] and g[4] == w["score"] and int(g[5]) == w["ran"]
        loops += int(w["loop_id"] >= 0)
        if w["loop_id"] >= 0 and not w["ran"]:
            assert np.abs(g[8:11] - w["t"]).max() < 1e-9 and np.abs(g[11:20].reshape(3, 3) - w["R"]).max() < 1e-9
        if w["ran"]:
            icps += 1
            assert int(g[6]) == w["ok"]
            if w["ok"]:                                               # as in mode 4: poses compared where the loop is accepted
                full += 1
                assert int(g[7]) == w["iters"]
                assert np.abs(g[8:11] - w["t"]).max() < 1e-9 and np.abs(g[11:20].reshape(3, 3) - w["R"]).max() < 1e-9
    print("mode 5: %d records, %d loops, %d ICP runs, %d accepted" % (len(want), loops, icps, full))
    assert loops > 0 and icps > 0 and full > 0
