"""CPU-side checks of the keyframe store (vba_kf_*): the exports, the adapter's KeyframeStore as plain C++17,
and the numpy restatement tests/kf_oracle.py pinned on hand-made cases (the GPU tests compare the device against it)."""
import os
import re
import subprocess

import numpy as np
import pytest

import kf_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KF_SYMBOLS = ["vba_kf_create", "vba_kf_destroy", "vba_kf_reserve", "vba_kf_allocations", "vba_kf_size", "vba_kf_build",
              "vba_kf_generate_stds", "vba_kf_set_poses", "vba_kf_get", "vba_kf_set_history", "vba_kf_load", "vba_kf_load_nearby",
              "vba_kf_read", "vba_kf_clouds"]


def _capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def _pose(rotvec, p):
    from scipy.spatial.transform import Rotation
    return np.concatenate([Rotation.from_rotvec(rotvec).as_matrix().ravel(), np.asarray(p, dtype=np.float64)])


IDENT = np.concatenate([np.eye(3).ravel(), np.zeros(3)])


def test_kf_symbols_exported_declared_and_bound():
    capi = _capi()
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    declared = set(re.findall(r"\b(vba_kf_[a-z0-9_]+)\s*\(", hdr))
    lib = capi.load()
    for s in KF_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    assert declared <= set(capi.EXPORTS)
    assert hasattr(capi, "KeyframeStore")


def test_adapter_keyframe_store_compiles(tmp_path):
    capi = _capi()
    src = tmp_path / "kf_adapter_check.cpp"
    src.write_text(r'''
#include "voxelba_adapter.hpp"
#include <cstdio>
// the device-side wrappers only have to compile and link here
int drive(vba::Context &ctx, vba::Context &map, vba::BtcDatabase &db) {
  vba::KeyframeStore kfs(ctx);
  kfs.reserve(1000000, 100, 250000);
  std::vector<vba::pointVar> scan(10);
  vba::IMUST x{};
  std::vector<vba::ScanPoseRef> bl_local(3, vba::ScanPoseRef{&x, &scan});
  std::vector<vba::STD> stds_vec;
  int kept = kfs.build(bl_local, 0.5 / 10, 9, 1.5, &db, &stds_vec);
  kfs.GenerateSTDescs(0, 1, db, stds_vec);
  kfs.set_poses(0, std::vector<vba::IMUST>(1, x));
  kfs.set_history(1);
  int k = kfs.keyframe_loading(map, x, 2.5);
  const double *d_pnt; const int *off; int n;
  kfs.clouds(d_pnt, off, n);
  std::vector<vba::XYZ> xyz, nrm;
  kfs.read(0, xyz, &nrm);
  return kept + k + n + kfs.size() + kfs.history_kfsize();
}
int main() { std::printf("ok %p\n", (void *)&drive); return 0; }
''')
    exe = tmp_path / "kf_adapter_check"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lvoxelba", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_merge_identity_poses_is_the_concatenation():
    rng = np.random.default_rng(0)
    clouds = [rng.uniform(-30, 30, (n, 3)) for n in (5, 0, 17, 3)]
    m = ko.merge(clouds, np.tile(IDENT, (4, 1)))
    assert np.array_equal(m, np.concatenate(clouds))
    assert np.array_equal(ko.merge_float(clouds, np.tile(IDENT, (4, 1))), np.concatenate(clouds).astype(np.float32))


def test_merge_single_scan_and_operation_order():
    rng = np.random.default_rng(1)
    c = rng.uniform(-30, 30, (50, 3))
    x = _pose([0.3, -0.2, 0.9], [4.0, -7.0, 1.5])
    # k = 1: dR = R^T R in the stated order (the identity only up to rounding), dp = exactly 0
    dR, dp = ko.delta(x, x)
    assert np.array_equal(dp, np.zeros(3)) and np.abs(dR - np.eye(3)).max() < 1e-15
    assert np.array_equal(ko.merge([c], [x]), ko.apply(dR, dp, c))
    # two scans: the stated order, element by element
    y = _pose([-0.1, 0.4, 0.2], [5.0, -6.5, 1.0])
    A, B = x[:9].reshape(3, 3), y[:9].reshape(3, 3)
    dR, dp = ko.delta(x, y)
    for r in range(3):
        for cc in range(3):
            assert dR[r, cc] == (A[0, r] * B[0, cc] + A[1, r] * B[1, cc]) + A[2, r] * B[2, cc]
        d = y[9:] - x[9:]
        assert dp[r] == (A[0, r] * d[0] + A[1, r] * d[1]) + A[2, r] * d[2]
    q = ko.merge([c, c], [y, x])[:50]
    for i in (0, 7, 49):
        for r in range(3):
            assert q[i, r] == ((dR[r, 0] * c[i, 0] + dR[r, 1] * c[i, 1]) + dR[r, 2] * c[i, 2]) + dp[r]
    assert np.abs(q - ((c @ B.T + y[9:]) - x[9:]) @ A).max() < 1e-12


def test_voxel_key_on_a_negative_face_and_float_narrowing():
    # a point exactly on voxel faces with negative coordinates: loc = -2 and -1 exactly, then the "-1" rule
    k = ko.voxel_keys([[-0.5, -0.25, 0.5]], 0.25, True)
    assert k.tolist() == [[-3, -2, 2]]                       # -2 -> -3, -1 -> -2: faces belong to the voxel below
    # the key is narrowed to float before the test and the truncation: a double just below a face lands ON the face in float
    x = np.nextafter(-0.5, 0.0)                              # p / 0.25 = -1.9999999999999998 -> (float) -2 -> -3
    assert ko.voxel_keys([[x, 0.0, 0.0]], 0.25, True)[0, 0] == -3
    x = np.nextafter(0.5, 0.0)                               # 1.9999999999999998 -> (float) 2 -> 2, not 1
    assert ko.voxel_keys([[x, 0.0, 0.0]], 0.25, True)[0, 0] == 2
    # the PCL form narrows the coordinate itself first
    p = 0.1 + 1e-12
    assert ko.voxel_keys([[p, 0, 0]], 0.1, False)[0, 0] == int(np.float32(np.float64(np.float32(p)) / 0.1))
    first, cnt, of = ko.voxel_groups([[0.3, 0.3, 0.3], [-0.3, 0.1, 0.1], [0.26, 0.4, 0.3], [-0.26, 0.2, 0.01]], 0.25, True)
    assert first.tolist() == [0, 1] and cnt.tolist() == [2, 2] and of.tolist() == [0, 1, 0, 1]   # first-occurrence order


def test_history_and_nearby_selection():
    pos = np.array([[0.0, 0, 0], [3.0, 0, 0], [6.0, 0, 0], [9.0, 0, 0], [50.0, 0, 0], [4.0, 0.5, 0]])
    h = ko.History(pos)
    assert h.load_nearby([0, 0, 0], 10) == -1                # before set_history: history_kfsize = 0
    h.set_history(0)
    assert h.load_nearby([0, 0, 0], 10) == -1 and h.size == 0   # set_history(0) switches loading off
    h.set_history(5)                                          # keyframe 5 is not history: exist = 0, no snapshot
    assert h.exist.tolist() == [1, 1, 1, 1, 1, 0] and h.size == 5 and len(h.snap) == 5
    idx, d2 = h.candidates([3.2, 0, 0], 5.0)
    assert idx.tolist() == [1, 2, 0] and d2.dtype == np.float32
    assert h.load_nearby([3.2, 0, 0], 5.0) == 1 and h.size == 4 and h.exist[1] == 0    # one load per call, decrement
    assert h.load_nearby([3.2, 0, 0], 5.0) == 2 and h.size == 3                         # skip over exist == 0, continue
    assert h.load_nearby([3.2, 0, 0], 5.0) == 0 and h.size == 2
    assert h.load_nearby([3.2, 0, 0], 5.0) == -1 and h.size == 2                        # nothing left inside: no decrement
    assert h.load_nearby([100.0, 0, 0], 5.0) == -1
    assert h.load_nearby([49.0, 0, 0], 5.0) == 4 and h.size == 1
    # the distance is float: positions and query are narrowed first
    h2 = ko.History([[1e-9, 0, 0], [0.0, 0, 0]]); h2.set_history(2)
    idx, d2 = h2.candidates([1.0, 0, 0], 2.0)
    assert idx.tolist() == [0, 1] and d2[0] == d2[1]          # equal in float: the lower index first


def test_world_transform_matches_merge_order():
    rng = np.random.default_rng(2)
    c = rng.uniform(-20, 20, (20, 3)).astype(np.float32).astype(np.float64)
    x = _pose([0.2, 0.1, -0.7], [10.0, 2.0, -1.0])
    R = x[:9].reshape(3, 3)
    w = ko.world(x, c)
    for i in range(20):
        for r in range(3):
            assert w[i, r] == ((R[r, 0] * c[i, 0] + R[r, 1] * c[i, 1]) + R[r, 2] * c[i, 2]) + x[9 + r]
