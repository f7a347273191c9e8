"""CPU-side checks of the voxel-down-sampled global map (vba_kf_voxel_export): the new prototypes, the
restatement tests/export_voxel_ref.py against the CPU oracle's down_sampling_voxel, against key boundaries worked out by hand and
against six mutations of itself, and the host halves of the adapter's pub_globalmap_voxel / pub_global_path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import export_oracle as eo
import export_voxel_ref as ev
import kf_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.fixture(scope="module")
def host(capi, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("export_voxel") / "export_voxel_host")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "export_voxel_host.cpp"),
                           "-o", exe, "-L", libdir, "-lvoxelba", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _edge(spread):
    return [(ev.edge_clouds(), ev.edge_poses(len(ev.EDGE_SIZES), 5, spread), 3.0)]


def test_new_prototypes(capi):
    from voxel_slam_amd import abi
    want = {"vba_kf_voxel_export_reserve": "i:pq", "vba_kf_voxel_export_allocations": "i:ppp", "vba_kf_voxel_export": "i:pippidiqppp"}
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    lib = capi.load()
    for name, proto in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert abi.PROTOTYPES.get(name) == proto and name in capi.EXPORTS and hasattr(lib, name), name
    names = list(abi.PROTOTYPES)
    assert names[names.index("vba_kf_export_world") + 1:][:3] == list(want)
    for m in ("kf_export_voxel", "kf_export_voxel_size", "kf_export_voxel_reserve", "kf_export_voxel_allocations"):
        assert hasattr(capi.Context, m), m
    # without a context every call is refused before it touches a device, outputs untouched
    n = C.c_int64(-77); a = C.c_int(-77); b = C.c_int64(-77)
    assert lib.vba_kf_voxel_export(None, 1, None, None, 1, 0.5, 1, 0, None, None, C.byref(n)) == capi.ERR_BAD_ARG and n.value == -77
    assert lib.vba_kf_voxel_export_reserve(None, 100) == capi.ERR_BAD_ARG
    assert lib.vba_kf_voxel_export_allocations(None, C.byref(a), C.byref(b)) == capi.ERR_BAD_ARG and (a.value, b.value) == (-77, -77)


# ---------------------------------------------------------------- (a) the oracle
@pytest.mark.parametrize("spread", [40.0, 2.0])
@pytest.mark.parametrize("voxel", [0.5, 2.0, 4.0, 1000.0])
@pytest.mark.parametrize("jump", [1, 3])
def test_restatement_against_the_oracle(oracle, spread, voxel, jump):
    """oracle_api.down_sampling_voxel (the reference's running float mean) on the widened records of S.  first and count are equal;
    a centroid is within 3 cnt 2^-24 max|a| of the restatement's: the running mean takes three float roundings per update on
    quantities of at most (k + 1) max|a|, divided by k + 1, and the restatement narrows once; max|a| is taken per voxel and axis.
    Singletons are bit-equal."""
    S, _ = ev.sequence(_edge(spread), jump)
    first, cnt, vox, xyz, _ = ev.centroids(S, voxel)
    oc, ocnt, ofirst = oracle.down_sampling_voxel(S[:, :3].astype(np.float64), voxel)
    assert np.array_equal(ofirst, first) and np.array_equal(ocnt, cnt)
    amax = np.zeros((len(first), 3))
    np.maximum.at(amax, vox, np.abs(S[:, :3].astype(np.float64)))
    bar = 3.0 * cnt[:, None] * 2.0 ** -24 * amax
    err = np.abs(oc - xyz.astype(np.float64))
    multi = cnt > 1
    ratio = (err[multi] / bar[multi]).max() if multi.any() else 0.0
    print("spread %g voxel %g jump %d: %d voxels, %d multi-point, largest count %d, worst error / bar %.3g"
          % (spread, voxel, jump, len(first), multi.sum(), cnt.max(), ratio))
    assert (err <= bar).all()
    assert np.array_equal(oc[~multi].astype(np.float32), xyz[~multi]) and np.array_equal(oc[~multi], xyz[~multi].astype(np.float64))


def test_overlapping_store_has_the_voxels_the_gpu_test_needs():
    """the figures tests/test_gpu_export_voxel.py asserts again on the device"""
    for spread, voxel, want in [(2.0, 2.0, (679, 449, 336, 8)), (2.0, 4.0, (148, None, 108, 36)), (40.0, 1000.0, (6, None, 4, 556))]:
        got = ev.voxel_census(_edge(spread), 1, voxel)
        print("spread %g voxel %g: voxels, multi-point, spanning keyframes, largest count = %s" % (spread, voxel, got))
        assert all(w is None or w == g for w, g in zip(want, got)), (got, want)
    xyzi, cnt, _ = ev.export_voxel(_edge(2.0), 1, 2.0, 3)
    assert len(cnt) == 316 and (cnt >= 3).all()


# ---------------------------------------------------------------- (b) key boundaries by hand
def test_key_boundaries_by_hand():
    g = ev.boundary_grid()
    assert g.shape == (2500, 3) and np.array_equal(g.astype(np.float32).astype(np.float64), g)
    sess = [([g], [ev.IDENTITY], 1.0)]
    S, _ = ev.sequence(sess, 1)
    assert np.array_equal(S[:, :3].astype(np.float64), g)                    # the world floats are the inputs
    for voxel, n_vox in [(1.0, 128), (0.25, 1875)]:
        xyzi, cnt, first = ev.export_voxel(sess, 1, voxel)
        assert len(xyzi) == n_vox and cnt.sum() == 2500
    key = lambda v, s: int(ko.voxel_keys([[v, 0.0, 0.0]], s, False)[0, 0])
    assert key(-1.0, 1.0) == -2 and key(-1.0, 0.25) == -5                    # loc < 0 -> loc - 1, then truncation
    assert key(-0.0, 1.0) == 0 and key(-0.0, 0.25) == 0 and key(0.0, 1.0) == 0
    assert [key(v, 1.0) for v in (-3.0, -2.75, -2.0, -1.75, -0.25, 0.25, 1.0, 3.0)] == [-4, -3, -3, -2, -1, 0, 1, 3]
    assert [key(v, 0.25) for v in (-3.0, -2.75, -0.25, 0.25, 0.5)] == [-13, -12, -2, 1, 2]


# ---------------------------------------------------------------- (c) teeth
def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _from_S(S, voxel, min_count=1, first_cnt_vox=None, last_intensity=False, le=False, key_order=False):
    first, cnt, vox = first_cnt_vox if first_cnt_vox is not None else ko.voxel_groups(S[:, :3], voxel, pvec=False)
    sums = np.zeros((len(first), 3))
    np.add.at(sums, vox, S[:, :3].astype(np.float64))
    xyz = (sums * (1.0 / cnt)[:, None]).astype(np.float32)
    src = first
    if last_intensity:
        src = np.zeros(len(first), np.int64)
        np.maximum.at(src, vox, np.arange(len(S)))
    keep = cnt > min_count if le else cnt >= min_count
    order = np.arange(len(first))
    if key_order:
        keys = ko.voxel_keys(S[first, :3], voxel, False)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    order = order[keep[order]]
    return np.concatenate([xyz, S[src, 3:4]], axis=1)[order].astype(np.float32), cnt[order].astype(np.int32), first[order]


def test_mutations_change_the_result():
    two = [(ev.edge_clouds(), ev.edge_poses(8, 5, 2.0), 1.0), (ev.edge_clouds(), ev.edge_poses(8, 6, 2.0), 2.0)]
    S, _ = ev.sequence(two, 3)
    base = ev.export_voxel(two, 3, 2.0)
    assert _same(base, _from_S(S, 2.0))                                       # the scaffold itself is the restatement
    # key from the double before narrowing: a world coordinate whose double and float fall on two sides of a voxel boundary
    p = np.array([[3.0 - 0.9 * 2.0 ** -23, 0.0, 0.0]])                       # 3.0 as a float; p / 3 narrows to 1 - 2^-24, (float)p / 3 is 1
    sess = [([p], [ev.IDENTITY], 1.0)]
    Sp, _ = ev.sequence(sess, 1)
    assert Sp[0, 0] == np.float32(3.0)
    assert ko.voxel_keys(p, 3.0, True)[0, 0] == 0 and ko.voxel_keys(Sp[:, :3], 3.0, False)[0, 0] == 1
    assert ko.voxel_keys(ev.export_voxel(sess, 1, 3.0)[0][:, :3], 3.0, False)[0, 0] == 1
    # loc - 1 dropped: -0.5 and 0.5 share voxel 0 of size 1.0
    q = np.array([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0]])
    assert len(ev.export_voxel([([q], [ev.IDENTITY], 1.0)], 1, 1.0)[0]) == 2
    loc = (q / 1.0).astype(np.float32).astype(np.int64)
    assert len(np.unique(loc, axis=0)) == 1
    # a stride that does not restart per keyframe picks other records
    run_on = np.concatenate([eo.points([c], [x], [it], 1) for cl, ps, it in two for c, x in zip(cl, ps)])[::3]
    assert len(run_on) != len(S) or not np.array_equal(run_on, S)
    assert not _same(base, _from_S(run_on, 2.0))
    # intensity of the LAST record: some voxel spans both stores
    assert not _same(base, _from_S(S, 2.0, last_intensity=True))
    # filter cnt <= min_count
    assert not _same(ev.export_voxel(two, 3, 2.0, 2), _from_S(S, 2.0, 2, le=True))
    # output in key order
    assert not _same(base, _from_S(S, 2.0, key_order=True))


# ---------------------------------------------------------------- (d) the host halves of the adapter
@pytest.mark.parametrize("n,interval,want", [(0, 5, [0]), (5, 5, [5]), (6, 5, [5, 6]), (4, 5, [4]), (10, 5, [5, 10]), (11, 5, [5, 10, 11]), (3, 1, [1, 2, 3])])
def test_message_cuts(host, n, interval, want):
    r = subprocess.run([host, "cuts", str(n), str(interval)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert got == want == ev.message_ends(n, interval)
    assert all(b - a <= interval for a, b in zip([0] + got[:-1], got))         # no message longer than the interval


def test_global_path_records(host):
    r = subprocess.run([host, "path"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    want = []
    for s, size in [(2, 2), (0, 3)]:                                          # ids = {2, 0}; session 1 is empty and not asked for
        for i in range(size):
            want.append([np.float32(100.0 * s + i + 0.1), np.float32(-float(i) - 1.0 / 3.0), np.float32(16777217.0 + s), np.float32(s)])
    got = np.array([[np.float32(v) for v in ln.split()] for ln in lines[:5]], dtype=np.float32)
    assert np.array_equal(got, np.array(want, dtype=np.float32))
    assert got[0, 2] == np.float32(16777220.0) or got[0, 2] == np.float32(16777218.0)      # narrowed: 16777219 is no float
    assert lines[5] == "records 5 messages 1" and lines[6] == "records 0 messages 1"


def test_unknown_mode_is_an_error(host):
    assert subprocess.run([host, "nothing"], capture_output=True, timeout=60).returncode == 2
