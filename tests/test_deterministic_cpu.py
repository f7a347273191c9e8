"""Deterministic mode without a GPU: the option's ABI and the host replay of the canonical order (tests/det_replay.py) that the
GPU tests (test_gpu_deterministic.py) check the device against."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import det_replay as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


def test_options_field_defaults_to_zero(capi):
    names = [f[0] for f in capi.Options._fields_]
    assert names[-1] == "deterministic"                      # appended: the layout of every earlier field is unchanged
    assert capi.Options.deterministic.offset + C.sizeof(C.c_int) <= C.sizeof(capi.Options)
    assert capi.default_options().deterministic == 0


def test_options_from_workload_keeps_default_mode(capi):
    from voxel_slam_amd import synth
    assert capi.options_from_workload(synth.CONFIGS["room20k_w4"]).deterministic == 0


def test_header_declares_field_last_and_no_new_function(capi):
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    body = re.search(r"typedef struct vba_options \{(.*?)\} vba_options;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*[a-z_ ]+\*?\s*\b([a-z_0-9]+)(?:\[\d+\])?;", body, re.M)
    assert fields[-1] == "deterministic"
    declared = set(re.findall(r"\b(vba_[a-z0-9_]+)\s*\(", hdr)) - {"vba_allreduce_fn"}
    assert declared == set(capi.EXPORTS)


def test_key_axis_quirk():
    # float narrowing first, then -1 for negatives, then truncation toward zero
    assert list(dr.key_axis(np.array([0.2999999999, -0.0001, -0.3, 0.6]), 0.3)) == [1, -1, -2, 2]


def test_root_numbering_replay():
    keys = np.array([[2, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [1, 0, 0], [0, 0, 0]])
    assert dr.first_touch_order(keys).tolist() == [[2, 0, 0], [1, 0, 0], [3, 0, 0], [0, 0, 0]]
    rn = dr.RootNumbering()
    assert rn.insert(keys) == [0, 1, 2, 3]
    assert rn.insert(np.array([[5, 0, 0], [1, 0, 0], [4, 0, 0]])) == [4, 5]         # [1,0,0] exists
    rn.prune([[3, 0, 0], [2, 0, 0], [5, 0, 0]])                                      # frees ids 2, 0, 4
    assert rn.free == [0, 2, 4]
    # first-touch order maps onto the ascending free ids, then fresh ids
    assert rn.insert(np.array([[9, 0, 0], [8, 0, 0], [1, 0, 0], [7, 0, 0], [6, 0, 0]])) == [0, 2, 4, 6]
    assert rn.nodes == 7 and rn.free == []
    assert rn.live_in_id_order().tolist() == [[9, 0, 0], [1, 0, 0], [8, 0, 0], [0, 0, 0], [7, 0, 0], [4, 0, 0], [6, 0, 0]]


def test_child_block_replay():
    bases, free, nodes = dr.allocate_blocks([40, 7, 19], [64, 16], 100)
    assert bases == {7: 16, 19: 64, 40: 100} and free == [] and nodes == 108
    bases, free, nodes = dr.allocate_blocks([5], [24, 8, 72], 100)
    assert bases == {5: 8} and free == [24, 72] and nodes == 100


def test_mask_bucket_is_a_ranking():
    for nb in (1, 3, 4, 10):
        b = [dr.mask_bucket(m, nb) for m in range(1 << nb)]
        assert sorted(b) == list(range(1 << nb))                                    # a bijection onto [0, 2^nb)
        pc = [bin(m).count("1") for m in range(1 << nb)]
        order = np.argsort(b)
        assert all(pc[order[i]] >= pc[order[i + 1]] for i in range(len(order) - 1))   # popcount descending
    assert dr.mask_bucket((1 << 10) - 1, 10) == 0


def test_store_order_on_hand_made_dump():
    # a dump of 6 leaves in ascending node id: (id, occupancy mask)
    ids = np.array([3, 8, 9, 12, 20, 21])
    masks = np.array([0b0011, 0b1111, 0b0011, 0b0001, 0b1111, 0b0111])
    o = dr.store_order(masks, ids, 4)
    # full masks first (ids 8, 20), then popcount 3 (21), then 2 (3, 9 in id order), then 1 (12)
    assert ids[o].tolist() == [8, 20, 21, 3, 9, 12]


def test_down_sampling_replay_adds_in_index_order():
    pnt = np.array([[0.1, 0.1, 0.1], [5.0, 5.0, 5.0], [0.2, 0.2, 0.2], [1e-12, 1e-12, 1e-12], [5.1, 5.1, 5.1]])
    cen, vd, cnt, first = dr.down_sampling(pnt, 1.0)
    assert first.tolist() == [0, 1] and cnt.tolist() == [3, 2] and vd is None
    s = (0.0 + float(np.float32(0.1))) + float(np.float32(0.2))
    s = s + float(np.float32(1e-12))
    assert cen[0, 0] == float(np.float32(s * (1.0 / 3)))
    var = np.zeros((5, 9)); var[:, 0] = [1e6, 1.0, 1e-12, 3.0, 2.0]
    cen, vd, cnt, first = dr.down_sampling(pnt, 1.0, var)
    assert vd[0, 0] == float(np.float32(((0.0 + 1e6) + 1e-12 + 3.0) * (1.0 / 3)))
