"""CPU-side checks of the local-map display export (vba_map_display): the new prototypes and their refusals that
need no device, and the restatement tests/map_display_ref.py against the CPU oracle: the geometric descent places every window point
in a leaf of the oracle's dump, and its per-leaf counts are the oracle's N_add - N_fix at every state of the sessions the GPU tests run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import map_display_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.fixture(scope="module")
def synth():
    from voxel_slam_amd import synth as s
    return s


def test_new_prototypes(capi):
    from voxel_slam_amd import abi
    want = {"vba_map_display_reserve": "i:pqq", "vba_map_display_allocations": "i:ppp", "vba_map_display": "i:pipiqpppqpppp"}
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    lib = capi.load()
    for name, proto in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert abi.PROTOTYPES.get(name) == proto and name in capi.EXPORTS and hasattr(lib, name), name
    names = list(abi.PROTOTYPES)
    assert names[names.index("vba_map_dump_plane_var") + 1:][:3] == list(want)          # the "Map level" block
    for m in ("map_display", "map_display_sizes", "map_display_reserve", "map_display_allocations"):
        assert hasattr(capi.Context, m), m


def test_refused_without_a_context(capi):
    """without a context every call is refused before it touches a device, outputs untouched"""
    lib = capi.load()
    n = C.c_int64(-77); m = C.c_int64(-77); a = C.c_int(-77); b = C.c_int64(-77)
    xyzi = np.full((4, 4), 7.0, dtype=np.float32); pop = np.full(4, 7, dtype=np.int32); fb = np.full(3, 7, dtype=np.int64)
    planes = np.full((4, 16), 7.0, dtype=np.float32); key = np.full((4, 5), 7, dtype=np.int64)
    poses = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (2, 1))
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    st = lib.vba_map_display(None, 2, p(poses), 0, 4, p(xyzi), p(pop), p(fb), 4, p(planes), p(key), C.byref(n), C.byref(m))
    assert st == capi.ERR_BAD_ARG and (n.value, m.value) == (-77, -77)
    assert (xyzi == 7).all() and (pop == 7).all() and (fb == 7).all() and (planes == 7).all() and (key == 7).all()
    assert lib.vba_map_display_reserve(None, 100, 100) == capi.ERR_BAD_ARG
    assert lib.vba_map_display_allocations(None, C.byref(a), C.byref(b)) == capi.ERR_BAD_ARG and (a.value, b.value) == (-77, -77)


def test_root_key_against_the_oracle(oracle):
    rng = np.random.default_rng(11)
    pw = np.concatenate([rng.uniform(-30, 30, (200, 3)), np.array([[-1.0, -0.0, 0.0], [-0.5, 0.5, 1.0], [-2.75, 3.0, -3.0]])])
    for vs in (0.3, 0.5, 1.0):
        got = mr.root_keys(pw, vs)
        for q, k in zip(pw, got):
            assert np.array_equal(oracle.map_key(vs, q), k), (vs, q)


@pytest.mark.parametrize("n_pts,nscan", [(700, 7), (3000, 9)])
def test_reference_against_oracle(oracle, synth, n_pts, nscan):
    """Every window point is placed, and the per-leaf counts are N_add - N_fix of the oracle's dump, after every recut and every
    margi + slide.  Observed: 0 mismatches, 0 unassigned points in all 11 + 15 states."""
    wl, scans, poses = mr.make_session(synth, n_pts, nscan)
    side = mr.OracleSide(oracle, wl)
    seen = []

    def on_state(kind, win):
        dump = side.dump_leaves()
        ref = mr.display(dump, [scans[k] for k in win], poses[win], wl.voxel_size, wl.max_layer)
        assert ref["unassigned"] == 0, (kind, win)
        assert np.array_equal(ref["counts"], (dump[:, 5] - dump[:, 6]).astype(np.int64)), (kind, win)
        per = np.diff(ref["frame_begin"])
        assert ref["frame_begin"][-1] == sum(len(f["xyzi"]) for f in ref["frames"]) and (per <= [len(scans[k]) for k in win]).all()
        seen.append((kind, len(win), int(per.min()), int(per.max()), len(ref["plane_keys"])))

    mr.run_session([side], scans, poses, wl.win_size, on_state)
    print("n_pts %d: %d states, exported per frame %d .. %d, planes %d .. %d"
          % (n_pts, len(seen), min(s[2] for s in seen), max(s[3] for s in seen), min(s[4] for s in seen), max(s[4] for s in seen)))
    assert len(seen) == 2 * nscan - 3 and {s[1] for s in seen if s[0] == "margi"} == {3}
    assert max(s[3] for s in seen) > 0 and max(s[4] for s in seen) > 0


def test_descent_has_teeth(oracle, synth):
    """a descent with the octant bits in the other order no longer reproduces the oracle's counts"""
    wl, scans, poses = mr.make_session(synth, 3000, 4)
    side = mr.OracleSide(oracle, wl)
    mr.run_session([side], scans[:3], poses[:3], wl.win_size, lambda kind, win: None)
    dump = side.dump_leaves()
    assert (dump[:, 3] > 0).any()
    good = mr.display(dump, scans[:3], poses[:3], wl.voxel_size, wl.max_layer)
    assert good["unassigned"] == 0
    flipped = dump.copy()
    deep = flipped[:, 3] == 1
    p = flipped[deep, 4].astype(np.int64)
    flipped[deep, 4] = ((p & 1) << 2) | (p & 2) | ((p >> 2) & 1)              # x and z bits swapped at layer 1
    bad = mr.display(flipped, scans[:3], poses[:3], wl.voxel_size, wl.max_layer)
    assert bad["unassigned"] > 0 or not np.array_equal(bad["counts"], good["counts"])
