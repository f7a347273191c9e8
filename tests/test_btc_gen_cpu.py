"""CPU checks of the descriptor-generation restatement (tests/btc_gen_oracle.py) and of the reference quirks vba_btc_generate_stds
pins (include/voxelba.h), on small hand-built clouds; and the host build of the plane fit against the header."""
import os
import re

import numpy as np
import pytest

import btc_gen_oracle as bg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def cfg0():
    return bg.read_parameters(0)


def test_float_config_quirks():
    for h in (0, 1):
        c = bg.read_parameters(h)
        assert bg.cut_num(c) == 49                                      # (int)(5 / 0.1f) = (int)(10 / 0.2f) = 49, not 50
    assert 1.0 / bg.read_parameters(0)["std_side_resolution"] == pytest.approx(4.99999992549, abs=1e-10)
    assert 1.0 / bg.read_parameters(0)["std_side_resolution"] != 5.0


def test_header_defaults_match_restatement():
    """vba_btc_default_gen_config in vba_btc.hip states the same values as read_parameters here"""
    src = open(os.path.join(ROOT, "voxel-slam_amd", "csrc", "vba_btc.hip")).read()
    body = src[src.index("int vba_btc_default_gen_config"):]
    body = body[:body.index("return VBA_OK;")]
    for h in (0, 1):
        c = bg.read_parameters(h)
        for k, v in c.items():
            m = re.search(r"f->%s = (.*?);" % k, body)
            assert m, k
            e = m.group(1)
            if "?" in e:
                a, b = re.match(r"is_high_fly \? (\S+) : (\S+)", e).groups()
                e = a if h else b
            val = float(e.rstrip("f"))
            assert (float(np.float32(val)) if isinstance(v, float) else int(val)) == v, k
    h = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    assert "vba_btc_generate_stds" in h and "vba_btc_gen_config" in h


def test_voxel_key_negative_and_boundary():
    c = cfg0()
    # -0.5 -> -1; 0.0 -> 0; exactly -1.0 -> (int64)(-1 - 1) = -2 (the reference subtracts 1 before truncating); 0.999 -> 0
    pts = np.array([[0.999, 0.2, 0.2], [-0.5, 0.2, 0.2], [0.0, 0.2, 0.2], [-1.0, 0.2, 0.2], [-0.5, 0.3, 0.3]], np.float32)
    key, vox, counts = bg.voxel_keys(pts, c)
    assert key[:, 0].tolist() == [0, -1, 0, -2, -1]
    # voxels in the order of their first point, points of one voxel share it
    assert vox.tolist() == [0, 1, 0, 2, 1] and counts.tolist() == [2, 2, 1]


def _patch(n, center, normal_axis, size=0.8, seed=0):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 3))
    ax = [a for a in range(3) if a != normal_axis]
    p[:, ax[0]] = rng.uniform(-size / 2, size / 2, n); p[:, ax[1]] = rng.uniform(-size / 2, size / 2, n)
    return (p + center).astype(np.float32)


def test_more_than_voxel_init_num():
    c = cfg0()
    ten = _patch(10, [0.5, 0.5, 0.5], 2)
    eleven = _patch(11, [0.5, 0.5, 0.5], 2)
    assert len(bg.voxel_planes(ten, c)) == 0                            # == voxel_init_num: not fitted
    assert len(bg.voxel_planes(eleven, c)) == 1


def test_sign_rule_and_host_twin():
    covs = np.array([[1, 0, 0, 1, 0, 1e-6], [1e-6, 0, 0, 1, 0, 1], [1, 0, 0, 1e-6, 0, 1],
                     [0.5, 0.5, 0, 0.5, 0, 1], [2, 0.1, 0.3, 1.5, 0.2, 0.01]], np.float64)
    w, n, direct = bg.plane_eig(covs)
    for i in range(len(covs)):
        k = int(np.argmax(np.abs(n[i])))
        assert n[i][k] > 0 and abs(np.linalg.norm(n[i]) - 1) < 1e-12
        A = np.array([[covs[i, 0], covs[i, 1], covs[i, 2]], [covs[i, 1], covs[i, 3], covs[i, 4]], [covs[i, 2], covs[i, 4], covs[i, 5]]])
        ev, V = np.linalg.eigh(A)
        assert abs(w[i] - ev[0]) < 1e-12
        assert abs(abs(V[:, 0] @ n[i]) - 1) < 1e-9
    # a tie of magnitudes: the lowest index is made positive
    w, n, _ = bg.plane_eig(np.array([[1.5, -0.5, 0, 1.5, 0, 3.0]]))      # smallest eigenvector (1, 1, 0) / sqrt 2
    assert n[0][0] > 0 and abs(n[0][0] - n[0][1]) < 1e-12
    # the line-like case takes the Jacobi fallback
    _, _, d = bg.plane_eig(np.array([[1e-6, 0, 0, 1e-6, 0, 1.0]]))
    assert d[0] == 0


def test_histogram_index_at_cut_num():
    """dis close to proj_dis_max gives (int)((dis - min) / high_inc) == cut_num: counted, but no occupancy bit"""
    c = cfg0()
    assert int((4.99 - c["proj_dis_min"]) / c["proj_image_high_inc"]) == 49
    g = np.stack(np.meshgrid(np.arange(-4, 4, 0.1), np.arange(-4, 4, 0.1), [0.0]), -1).reshape(-1, 3)
    col = np.column_stack([np.full(60, 0.3), np.full(60, 0.3), np.linspace(0.05, 4.99, 60)])
    top = np.array([[0.3, 0.3, 4.995]])
    p = np.concatenate([g, col, top]).astype(np.float32)
    corners = bg.extract_binary(np.array([0.0, 0, 0]), np.array([0.0, 0, 1]), p, c)
    for _, s, b in corners:
        assert b < (1 << 49) and s == bin(b).count("1")


def test_min_k_and_first_wins_dedupe():
    c = cfg0()
    tri = np.array([[0.0, 0, 0], [3, 0, 0], [0, 4, 0]])
    locs = np.concatenate([tri, tri + [100.0, 0, 0]])                   # two congruent triangles, 100 m apart
    corners = [(locs[i], 20, i) for i in range(6)]                      # 6 corners < K = 15: min(K, n) neighbours
    rows, bits = bg.generate_std(corners, 4, c)
    assert len(rows) == 1 and np.all(rows[:, 6] == 4)                   # the copy has the same key: the first found wins
    assert set(bits[0].tolist()) == {0, 1, 2}
    assert np.allclose(rows[0, :3], np.array([3, 4, 5]) / c["std_side_resolution"])
    assert sorted(map(tuple, rows[0, 7:16].reshape(3, 3).tolist())) == sorted(map(tuple, tri.tolist()))
    # float side keys: (int64)(float)(a * 1000)
    assert int(np.float32(2.0000004 * 1000)) == 2000


def test_stable_sort_ties():
    P = [bg.Plane(np.zeros(3), np.array([0, 0, 1.0]), np.zeros(6), n, 0.0) for n in (5, 7, 5, 7, 6)]
    for i, q in enumerate(P):
        q.c = np.array([float(i), 0, 0])
    s = bg.stable_sort_planes(P)
    assert [int(q.c[0]) for q in s] == [1, 3, 4, 0, 2]


def test_useful_corner_num_boundary():
    """binary_extractor's tail (bg.select_corners): useful_corner_num > size keeps the list unsorted, equality sorts stably"""
    c = cfg0()
    c["non_max_suppression_radius"] = bg.f(0.01)
    three = [(np.array([10.0 * i, 0, 0]), s, i) for i, s in enumerate((4, 9, 9))]
    c["useful_corner_num"] = 4
    assert [t[2] for t in bg.select_corners(three, c)] == [0, 1, 2]
    c["useful_corner_num"] = 3
    assert [t[2] for t in bg.select_corners(three, c)] == [1, 2, 0]           # ties keep their order
    c["useful_corner_num"] = 2
    assert [t[2] for t in bg.select_corners(three, c)] == [1, 2]
    # NMS before the cut: a neighbour within the radius with a summary >= drops a corner
    c["non_max_suppression_radius"] = bg.f(15.0)
    c["useful_corner_num"] = 4
    assert [t[2] for t in bg.select_corners(three, c)] == []                   # 0 <= 1, 1 <= 2 and 2 <= 1 (equal summaries)


def test_nms_strict_radius():
    c = cfg0()
    r2 = np.float32(float(c["non_max_suppression_radius"]) ** 2)
    t = [(np.array([0.0, 0, 0]), 5, 0), (np.array([float(np.sqrt(np.float64(r2))), 0, 0]), 9, 0)]
    d2 = bg.pairwise_d2(np.array([x[0] for x in t]))[0, 1]
    kept = bg.nms(t, c)
    assert (len(kept) == 1) == bool(d2 < r2)


def test_empty_and_no_plane():
    c = cfg0()
    r = bg.generate_stds(np.zeros((0, 3), np.float32), 0, c)
    assert len(r["planes"]) == 0 and len(r["rows"]) == 0
    rng = np.random.default_rng(1)
    noise = rng.uniform(-20, 20, (5000, 3)).astype(np.float32)
    r = bg.generate_stds(noise, 0, c)
    assert r["groups"] == 0                                             # single_plane branch, no UB walk of an empty list
