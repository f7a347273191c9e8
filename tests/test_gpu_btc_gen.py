"""BTC descriptor generation on the MI355X (vba_btc_generate_stds: GenerateSTDescs, BTC.cpp:156-203) against the numpy
restatement in tests/btc_gen_oracle.py, bit for bit, over keyframe clouds of voxel_slam_amd.synth.make_btc_keyframe_sessions;
its edge cases on the device, repeat runs, its interplay with the retrieval half, and an end-to-end loop detection."""
import numpy as np
import pytest

import btc_gen_oracle as bg

pytestmark = pytest.mark.gpu


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
def clouds(synth):
    return synth.make_btc_keyframe_sessions(n_sessions=1, n_kf=20, n_points=200000, seed=11)[0]["cloud"]


def make_db(capi, ctx, high):
    db = ctx.btc_db(capi.btc_default_config(high))
    db.set_gen_config(capi.btc_default_gen_config(high))
    return db


def check_equal(db, out, ref, frame):
    rows, bits = out
    pl = db.plane_cloud(frame)
    assert np.array_equal(pl, ref["planes"]), "plane cloud differs (%d vs %d points)" % (len(pl), len(ref["planes"]))
    loc, summ, cb = db.last_corners()
    rl, rs, rb = ref["corners"]
    assert np.array_equal(loc, rl) and np.array_equal(summ, rs) and np.array_equal(cb, rb), "corners differ (%d vs %d)" % (len(loc), len(rl))
    assert np.array_equal(rows, ref["rows"]) and np.array_equal(bits, ref["bits"]), "rows differ (%d vs %d)" % (len(rows), len(ref["rows"]))


@pytest.mark.parametrize("high", [0, 1])
def test_parity_keyframes(capi, ctx, clouds, high):
    db = make_db(capi, ctx, high)
    cfg = bg.read_parameters(high)
    assert bg.config_dict(capi.btc_default_gen_config(high)) == cfg
    n_rows = []
    for k, cl in enumerate(clouds):
        out = db.generate_stds(cl, 100 + k)
        ref = bg.generate_stds(cl, k, cfg)
        check_equal(db, out, ref, k)
        assert db.frame_seq(k) == 100 + k
        db.add_stds(*out)
        n_rows.append(len(out[0]))
    assert min(n_rows) > 0
    print("config %d: rows per keyframe min %d median %d max %d" % (high, min(n_rows), int(np.median(n_rows)), max(n_rows)))
    db.close()


def test_parity_full_size(capi, ctx, synth):
    """two keyframes of 10 x 200k points (the merged cloud of a win_size = 10 keyframe)"""
    ses = synth.make_btc_keyframe_sessions(n_sessions=1, n_kf=2, n_points=2000000, seed=12)[0]
    db = make_db(capi, ctx, 0)
    for k, cl in enumerate(ses["cloud"]):
        out = db.generate_stds(cl, k)
        check_equal(db, out, bg.generate_stds(cl, 0, bg.read_parameters(0)), k)
    db.close()


def test_determinism(capi, ctx, clouds):
    a, b = make_db(capi, ctx, 0), make_db(capi, ctx, 0)
    for k in range(3):
        ra, rb = a.generate_stds(clouds[k], k), b.generate_stds(clouds[k], k)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        assert np.array_equal(a.plane_cloud(k), b.plane_cloud(k))
    a.close(); b.close()


def test_edge_cases_on_device(capi, ctx):
    db = make_db(capi, ctx, 0)
    cfg = bg.read_parameters(0)
    # empty input: an empty plane cloud, no descriptors
    rows, bits = db.generate_stds(np.zeros((0, 3), np.float32), 7)
    assert len(rows) == 0 and db.num_frames() == 1 and len(db.plane_cloud(0)) == 0 and db.frame_seq(0) == 7
    assert len(db.last_corners()[0]) == 0
    rng = np.random.default_rng(5)
    # no planar voxel: the single_plane branch (normal (0, 0, 1) through the first point)
    noise = rng.uniform(-20, 20, (20000, 3)).astype(np.float32)
    ref = bg.generate_stds(noise, 0, cfg)
    assert ref["groups"] == 0
    check_equal(db, db.generate_stds(noise, 1), ref, 1)
    # fewer corners than K: min(K, n) neighbours; keys at negative and exact-boundary coordinates
    g = np.stack(np.meshgrid(np.arange(-6, 6, 0.25), np.arange(-6, 6, 0.25), [0.0]), -1).reshape(-1, 3)
    posts = [np.column_stack([np.full(200, x), np.full(200, y), np.linspace(0, h, 200)]) for x, y, h in
             ((-3, -3, 4.9), (3, -2, 3.0), (-2, 3, 4.0), (2.5, 2.5, 2.0))]
    small = np.concatenate([g] + posts).astype(np.float32)
    ref = bg.generate_stds(small, 0, cfg)
    assert 0 < len(ref["corners"][0]) < 15
    check_equal(db, db.generate_stds(small, 2), ref, 2)
    db.close()


def _small_scene():
    g = np.stack(np.meshgrid(np.arange(-6, 6, 0.25), np.arange(-6, 6, 0.25), [0.0]), -1).reshape(-1, 3)
    posts = [np.column_stack([np.full(200, x), np.full(200, y), np.linspace(0, h, 200)]) for x, y, h in
             ((-3, -3, 4.9), (3, -2, 3.0), (-2, 3, 4.0), (2.5, 2.5, 2.0))]
    return np.concatenate([g] + posts)


@pytest.mark.parametrize("n", [8191, 8192, 8193, 16385])
def test_point_counts_at_the_scan_chunk_edges(capi, ctx, n):
    """the voxel pass scans one flag per point with the one-workgroup chunked scan (k_bg_scan: chunks of 8192 entries linked by a
    carry): a last chunk that is one entry short, full, and one entry long, and a third chunk of one entry.  Six copies of the small
    scene cut to n points; every voxel start, and so every plane, corner and row, follows from the scanned positions."""
    scene = np.concatenate([_small_scene() + [14.0 * i, 14.0 * j, 0.0] for i in range(3) for j in range(2)]).astype(np.float32)
    assert len(scene) > 16385
    db = make_db(capi, ctx, 0)
    ref = bg.generate_stds(scene[:n], 0, bg.read_parameters(0))
    assert len(ref["planes"]) > 0 and len(ref["rows"]) > 0
    check_equal(db, db.generate_stds(scene[:n], 0), ref, 0)
    db.close()


def test_quirks_on_device(capi, ctx):
    """the section-3 quirks on the device, each on a crafted cloud compared bit for bit with the restatement"""
    cfg = bg.read_parameters(0)
    db = make_db(capi, ctx, 0)
    frame = 0
    def run(cloud, c=None):
        nonlocal frame
        gc = capi.btc_default_gen_config(0)
        for k, v in (c or {}).items():
            setattr(gc, k, v)
        db.set_gen_config(gc)
        cc = bg.config_dict(gc)
        ref = bg.generate_stds(cloud.astype(np.float32), 0, cc)
        check_equal(db, db.generate_stds(cloud.astype(np.float32), frame), ref, frame)
        frame += 1
        return ref
    # histogram index == cut_num: a column reaching 4.995 above the ground plane (counted in the cell, no occupancy bit)
    g = np.stack(np.meshgrid(np.arange(-4, 4, 0.1), np.arange(-4, 4, 0.1), [0.0]), -1).reshape(-1, 3)
    cols = [np.column_stack([np.full(60, x), np.full(60, y), np.linspace(0.05, 4.995, 60)]) for x, y in ((0.3, 0.3), (-2.2, 1.7), (2.6, -2.1))]
    ref = run(np.concatenate([g] + cols))
    assert len(ref["corners"][0]) > 0 and int(ref["corners"][2].max()) < (1 << 49)
    # useful_corner_num == size (sorted, ties stable) and size + 1 (kept unsorted)
    big = np.concatenate([_small_scene(), _small_scene() + [14.0, 0, 0], _small_scene() + [0, 14.0, 0]])
    n_pass = len(bg.generate_stds(big.astype(np.float32), 0, dict(cfg, useful_corner_num=10 ** 6))["corners"][1])
    assert n_pass >= 3
    run(big, dict(useful_corner_num=n_pass))
    run(big, dict(useful_corner_num=n_pass + 1))
    # congruent copies of one scene: their triangles share float side keys, the first emitted wins
    ref = run(np.concatenate([_small_scene(), _small_scene() + [30.0, 0, 0]]))
    assert len(ref["rows"]) > 0 and ref["dupes"] > 0
    db.close()


def test_refusals_have_no_side_effects(capi, ctx, clouds):
    db = make_db(capi, ctx, 0)
    need = capi.btc_max_stds(capi.btc_default_gen_config(0))
    with pytest.raises(capi.VbaError):
        db.generate_stds(clouds[0], 0, cap=need - 1)
    assert db.num_frames() == 0
    db.close()
    c = capi.btc_default_config(0)
    c.occupy_len = 48                                   # cut_num is 49
    db = ctx.btc_db(c)
    with pytest.raises(capi.VbaError):
        db.generate_stds(clouds[0], 0)
    assert db.num_frames() == 0
    c.occupy_len = 49
    db2 = ctx.btc_db(c)
    assert len(db2.generate_stds(clouds[0], 0)[0]) > 0 and db2.num_frames() == 1
    db.close(); db2.close()


def test_frame_number_and_search_interplay(capi, ctx, clouds):
    """frame_number_ follows the add_stds count; a generated plane cloud searches like the restatement's cloud pushed by hand"""
    cfg = bg.read_parameters(0)
    gen = make_db(capi, ctx, 0)
    man = ctx.btc_db(capi.btc_default_config(0))
    for k in range(6):
        rows, bits = gen.generate_stds(clouds[k], 50 + k)
        assert np.all(rows[:, 6] == k)
        ref = bg.generate_stds(clouds[k], k, cfg)
        man.push_plane_cloud(ref["planes"], 50 + k)
        if k < 5:
            gen.add_stds(rows, bits); man.add_stds(ref["rows"], ref["bits"])
    gen.add_stds(np.zeros((0, 19)), np.zeros((0, 3), np.uint64))     # an empty AddSTDescs still counts
    rows, bits = gen.generate_stds(clouds[6], 56)
    assert np.all(rows[:, 6] == 6)           # five non-empty calls and one empty one
    for db in (gen, man):
        db.set_skip_near_num(0)
    r5 = bg.generate_stds(clouds[5], 5, cfg)
    q, qb = r5["rows"], r5["bits"]
    ra = gen.search_loop(q, qb, gen, 5)
    rb = man.search_loop(q, qb, man, 5)
    assert ra["loop_id"] == rb["loop_id"] and ra["score"] == rb["score"]
    assert np.array_equal(ra["R"], rb["R"]) and np.array_equal(ra["t"], rb["t"])
    gen.close(); man.close()


def test_reserved_generation_does_not_allocate(capi, ctx, clouds):
    db = make_db(capi, ctx, 0)
    db.reserve(stds=200000, frames=64, matches=1 << 18)
    db.gen_reserve(points=250000, cells=1 << 22, frames=4)
    n0 = db.gen_allocations()
    for k in range(4):
        db.add_stds(*db.generate_stds(clouds[k], k))
    assert db.gen_allocations() == n0
    db.close()


def test_end_to_end_revisits(capi, ctx, synth):
    """two sessions over one circuit of radius 130 m, 12 keyframes each (67 m apart, more than twice the 25 m view, so that no two
    keyframes of one session share structure; the second session's keyframe k revisits the first's k + 6):
    generate -> search_loop_sessions -> icp_normal.  Measured on MI355X: 3 of 12 keyframes find a loop, all at the revisited place
    (0.27-0.84 m from ground truth), none elsewhere; ICP within 0.010 m / 0.026 degrees.  Bars: at least a quarter of the second
    session's keyframes find a loop; every loop joins the revisited place (within 5 m of ground truth: any other keyframe is >= 60 m
    away and shares no structure); every ICP pose within 0.5 m / 2 degrees of the ground-truth relative pose."""
    ses = synth.make_btc_keyframe_sessions(n_sessions=2, n_kf=12, n_points=200000, radius=130.0, view=25.0, extent=165.0, seed=21)
    d0, d1 = make_db(capi, ctx, 0), make_db(capi, ctx, 0)
    for k, cl in enumerate(ses[0]["cloud"]):
        d0.add_stds(*d0.generate_stds(cl, k))
    d0.set_skip_near_num(0)
    found, wrong, dists, terr, rerr = 0, 0, [], [], []
    for k, cl in enumerate(ses[1]["cloud"]):
        rows, bits = d1.generate_stds(cl, k)
        res = ctx.btc_search_loop_sessions([d0], rows, bits, d1)[0]
        if res["loop_id"] >= 0:
            j = res["loop_id"]
            dist = float(np.linalg.norm(ses[1]["t"][k] - ses[0]["t"][j]))
            dists.append(dist)
            if dist > 5.0:
                wrong += 1
                continue
            found += 1
            R0, t0, R1, t1 = ses[0]["R"][j], ses[0]["t"][j], ses[1]["R"][k], ses[1]["t"][k]
            Rg, tg = R0.T @ R1, R0.T @ (t1 - t0)
            icp = d1.icp_normal(d1.num_frames() - 1, d0, j, res["t"], res["R"], 14)
            terr.append(float(np.linalg.norm(icp["t"] - tg)))
            rerr.append(float(np.degrees(np.arccos(np.clip((np.trace(Rg.T @ icp["R"]) - 1) / 2, -1, 1)))))
        d1.add_stds(rows, bits)
    n = len(ses[1]["cloud"])
    print("end to end: loops at the revisited place %d / %d, wrong loops %d, distances %s, icp t err max %.3f m, R err max %.3f deg"
          % (found, n, wrong, np.round(dists, 2).tolist(), max(terr) if terr else -1, max(rerr) if rerr else -1))
    assert wrong == 0
    assert found >= n // 4
    assert max(terr) < 0.5 and max(rerr) < 2.0
    d0.close(); d1.close()
