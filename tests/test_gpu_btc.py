"""Loop retrieval on the MI355X (vba_btc_*: STDescManager::SearchLoop, BTC.cpp:205-256, and icp_normal, loop_refine.hpp:47-139)
against the numpy restatement in tests/btc_oracle.py, over synthetic sessions of voxel_slam_amd.synth.make_btc_sessions."""
import numpy as np
import pytest

import btc_oracle as bo

pytestmark = pytest.mark.gpu

N_KF = 200


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
def ctx(capi):
    o = capi.default_options()
    o.device = 0
    c = capi.Context(o)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sessions(synth):
    return synth.make_btc_sessions(n_sessions=3, n_kf=N_KF, seed=3)


def _same_result(a, b, tol=1e-9):
    assert a["loop_id"] == b["loop_id"]
    assert a["score"] == b["score"]
    if b["loop_id"] >= 0:
        assert np.abs(a["t"] - b["t"]).max() < tol
        assert np.abs(a["R"] - b["R"]).max() < tol


def _same_candidates(dev, ora):
    assert [c["frame"] for c in dev] == [c["frame"] for c in ora]
    assert [c["votes"] for c in dev] == [c["votes"] for c in ora]
    assert [c["match_len"] for c in dev] == [c["match_len"] for c in ora]
    assert [c["max_vote_index"] for c in dev] == [c["max_vote_index"] for c in ora]
    assert [c["max_vote"] for c in dev] == [c["max_vote"] for c in ora]
    for a, b in zip(dev, ora):
        assert a["score"] == b["score"] or (np.isnan(a["score"]) and np.isnan(b["score"]))


def _run_session(capi, ctx, S, cfg, db=None):
    """one session through device and oracle, keyframe by keyframe (push cloud, search, add): per-keyframe results"""
    db = db or ctx.btc_db(cfg)
    od = bo.BtcDb(cfg)
    out = []
    for k in range(len(S["rows"])):
        db.push_plane_cloud(S["cloud"][k], k)
        od.push_plane_cloud(S["cloud"][k], k)
        r = db.search_loop(S["rows"][k], S["bits"][k], db)
        cands = db.last_candidates()
        ro, co = od.search_loop(S["rows"][k], S["bits"][k], S["cloud"][k])
        out.append((r, cands, ro, co))
        db.add_stds(S["rows"][k], S["bits"][k])
        od.add_stds(S["rows"][k], S["bits"][k])
    return db, out


def test_session_matches_oracle_and_ground_truth(capi, ctx, sessions):
    cfg = capi.btc_default_config(0)
    S = sessions[0]
    _, out = _run_session(capi, ctx, S, cfg)
    loops = 0
    for k, (r, cands, ro, co) in enumerate(out):
        _same_candidates(cands, co)
        _same_result(r, ro)
        if r["loop_id"] >= 0:
            loops += 1
            j = r["loop_id"]                                       # ground truth: T_j^-1 T_k
            Rg = S["R"][j].T @ S["R"][k]
            tg = S["R"][j].T @ (S["p"][k] - S["p"][j])
            # one triangle's transform: 1 cm of keypoint noise over 2-10 m sides, a lever of ~35 m
            assert np.abs(r["R"] - Rg).max() < 0.02 and np.abs(r["t"] - tg).max() < 0.5
    assert loops >= 20                                            # the revisits are found


def test_runs_are_identical(capi, ctx, sessions):
    cfg = capi.btc_default_config(0)
    S = sessions[1]
    n = 80
    runs = []
    for _ in range(2):
        db = ctx.btc_db(cfg)
        res = []
        for k in range(n):
            db.push_plane_cloud(S["cloud"][k], k)
            r = db.search_loop(S["rows"][k], S["bits"][k], db)
            res.append((r["loop_id"], r["score"], r["t"].copy(), r["R"].copy(), db.last_candidates()))
            db.add_stds(S["rows"][k], S["bits"][k])
        runs.append(res)
        db.close()
    for a, b in zip(runs[0], runs[1]):
        assert a[0] == b[0] and a[1] == b[1]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert a[4] == b[4]


def test_sessions_batched_equal_per_session(capi, ctx, sessions):
    cfg = capi.btc_default_config(0)
    dbs = []
    n = 60
    for s in range(3):
        db = ctx.btc_db(cfg)
        for k in range(n):
            db.push_plane_cloud(sessions[s]["cloud"][k], k)
            db.add_stds(sessions[s]["rows"][k], sessions[s]["bits"][k])
        dbs.append(db)
    dbs[0].set_skip_near_num(-(n + 10))                             # closed sessions (VS:2242)
    dbs[1].set_skip_near_num(-(n + 10))
    S = sessions[2]
    checked = 0
    for k in range(n, n + 40):
        dbs[2].push_plane_cloud(S["cloud"][k], k)
        batched = ctx.btc_search_loop_sessions(dbs, S["rows"][k], S["bits"][k], dbs[2])
        for s in range(3):
            one = dbs[s].search_loop(S["rows"][k], S["bits"][k], dbs[2])
            assert one["loop_id"] == batched[s]["loop_id"] and one["score"] == batched[s]["score"]
            assert np.array_equal(one["t"], batched[s]["t"]) and np.array_equal(one["R"], batched[s]["R"])
            checked += one["loop_id"] >= 0
        dbs[2].add_stds(S["rows"][k], S["bits"][k])
    assert checked > 0                                              # cross-session loops exist in the stream
    for db in dbs:
        db.close()


def test_edge_cases(capi, ctx, sessions):
    cfg = capi.btc_default_config(0)
    S = sessions[0]
    db = ctx.btc_db(cfg)
    db.push_plane_cloud(S["cloud"][0], 0)
    # empty database: no candidates, no loop
    r = db.search_loop(S["rows"][0], S["bits"][0], db)
    assert r["loop_id"] == -1 and r["score"] == 0.0 and db.last_candidates() == []
    # empty query: (-1, 0)
    r = db.search_loop(np.zeros((0, 19)), np.zeros((0, 3), np.uint64), db)
    assert r["loop_id"] == -1 and r["score"] == 0.0
    db.add_stds(S["rows"][0], S["bits"][0])
    # frames under the vote floor: 4 matching descriptors -> no candidate
    q = S["rows"][0][:4].copy(); q[:, 6] = 100
    r = db.search_loop(q, S["bits"][0][:4], db)
    assert r["loop_id"] == -1 and db.last_candidates() == []
    # 5 -> one candidate; an empty pl_cur scores NaN, which never wins
    q = S["rows"][0][:8].copy(); q[:, 6] = 100
    db.push_plane_cloud(np.zeros((0, 6), np.float32), 1)
    r = db.search_loop(q, S["bits"][0][:8], db, cur_frame=1)
    c = db.last_candidates()
    assert len(c) == 1 and c[0]["votes"] == 8 and r["loop_id"] == -1
    assert c[0]["max_vote"] < 4 or np.isnan(c[0]["score"])
    # a frame_number outside the pushed clouds is refused
    bad = S["rows"][0][:1].copy(); bad[0, 6] = 7
    with pytest.raises(capi.VbaError):
        db.add_stds(bad, S["bits"][0][:1])
    db.close()


@pytest.mark.parametrize("n", [200, 24000])
def test_icp_matches_oracle(capi, ctx, synth, n):
    tar = synth.btc_plane_cloud(n, seed=1)
    Rt = bo.so3_exp([0.02, -0.03, 0.05]); tt = np.array([0.3, -0.2, 0.1])
    src = tar.copy()
    src[:, 0:3] = ((tar[:, 0:3].astype(np.float64) - tt) @ Rt).astype(np.float32)   # tar = Rt src + tt
    src[:, 3:6] = (tar[:, 3:6].astype(np.float64) @ Rt).astype(np.float32)
    db = ctx.btc_db(capi.btc_default_config(0))
    db.push_plane_cloud(src, 0)
    db.push_plane_cloud(tar, 1)
    t0 = np.zeros(3); R0 = np.eye(3)
    a = db.icp_normal(0, db, 1, t0, R0, 0.1)
    b = db.icp_normal(0, db, 1, t0, R0, 0.1)
    o = bo.icp_normal(src, tar, t0, R0, 0.1)
    assert a["ok"] == o["ok"] == 1 and a["iters"] == o["iters"]
    assert np.abs(a["t"] - o["t"]).max() < 1e-9 and np.abs(a["R"] - o["R"]).max() < 1e-9
    assert np.abs(a["eig"] - o["eig"]).max() <= 1e-9 * np.abs(o["eig"]).max()
    assert np.abs(a["R"] - Rt).max() < 1e-3 and np.abs(a["t"] - tt).max() < 1e-2
    for k in ("t", "R", "eig"):
        assert np.array_equal(a[k], b[k])
    assert a["iters"] == b["iters"] and a["ok"] == b["ok"]
    db.close()


def test_loop_timing_family(capi, ctx, sessions):
    S = sessions[0]
    db = ctx.btc_db(capi.btc_default_config(0))
    ctx.timing_enable(True)
    ctx.timing_reset()
    db.push_plane_cloud(S["cloud"][0], 0)
    db.search_loop(S["rows"][0], S["bits"][0], db)
    db.icp_normal(0, db, 0, np.zeros(3), np.eye(3), 0.1)
    tot, cnt = ctx.timing_get("loop")
    ctx.timing_enable(False)
    assert cnt == 2 and tot > 0
    db.close()


def _growth_stream(S, n_kf=120, n_big=300):
    """keyframes of a session, then one add_stds of n_big copies of one descriptor (one cell gets > 4 chunks in a single call) and a
    query of n_big copies whose match list (n_big x n_big pairs and more) overflows the initial 65 536-pair list"""
    steps = [("kf", k) for k in range(n_kf)]
    row = S["rows"][0][0].copy()
    big = np.tile(row, (n_big, 1)); big[:, 6] = np.arange(n_big) % n_kf
    bigbits = np.tile(S["bits"][0][:1], (n_big, 1))
    q = np.tile(row, (n_big, 1)); q[:, 6] = 10 * n_kf
    steps.append(("big", (big, bigbits, q, bigbits.copy())))
    return steps


def _play(db, od, S, steps):
    out = []
    for kind, arg in steps:
        if kind == "kf":
            k = arg
            db.push_plane_cloud(S["cloud"][k], k)
            rows, bits, cl = S["rows"][k], S["bits"][k], S["cloud"][k]
            if od is not None:
                od.push_plane_cloud(cl, k)
        else:
            big, bigbits, rows, bits = arg
            db.add_stds(big, bigbits)
            if od is not None:
                od.add_stds(big, bigbits)
            cl = S["cloud"][0]
            db.push_plane_cloud(cl, 0)
            if od is not None:
                od.push_plane_cloud(cl, 0)
        r = db.search_loop(rows, bits, db)
        c = db.last_candidates()
        o = od.search_loop(rows, bits, cl) if od is not None else None
        out.append((r, c, o))
        if kind == "kf":
            db.add_stds(rows, bits)
            if od is not None:
                od.add_stds(rows, bits)
    return out


def test_grown_equals_reserved_and_big_cell(capi, ctx, sessions):
    cfg = capi.btc_default_config(0)
    S = sessions[1]
    steps = _growth_stream(S)
    grown = ctx.btc_db(cfg)                                         # 1024 rows / 1024 slots / 256 chunks / 65 536 pairs to start
    a = _play(grown, bo.BtcDb(cfg), S, steps)
    big = ctx.btc_db(cfg)
    big.reserve(stds=1 << 16, frames=1024, cloud_points=1 << 20, matches=1 << 18)
    b = _play(big, None, S, steps)
    for (ra, ca, o), (rb, cb, _) in zip(a, b):
        _same_candidates(ca, o[1])
        _same_result(ra, o[0])
        assert ra["loop_id"] == rb["loop_id"] and ra["score"] == rb["score"]
        assert np.array_equal(ra["t"], rb["t"]) and np.array_equal(ra["R"], rb["R"])
        assert ca == cb
    assert len(a[-1][1]) > 0                                        # the big keyframe has candidates
    od = bo.BtcDb(cfg)                                              # and its match list overflowed the initial 65 536 pairs
    for k in range(120):
        od.push_plane_cloud(S["cloud"][k], k)
        od.add_stds(S["rows"][k], S["bits"][k])
    bigrows, bigbits, q, qb = steps[-1][1]
    od.add_stds(bigrows, bigbits)
    assert len(od.match_list(q, qb)[0]) > 65536
    grown.close(); big.close()
