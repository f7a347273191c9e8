"""CPU-side checks of the loop-closure map rebuild (vba_loop_map_*, vba_loop_update): the exports, the adapter
as plain C++17 and its host algebra against the numpy restatement tests/loop_oracle.py, the expansion table of VS:2601-2625, and the
POWER of the covariance comparison the GPU tests make: on the CPU oracle alone, the loop_update sequence replayed with and without
the fixed points' covariances must end in different cov_add sums."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loop_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)

LOOP_SYMBOLS = ["vba_loop_map_create", "vba_loop_map_destroy", "vba_loop_map_reserve", "vba_loop_map_allocations", "vba_loop_map_build",
                "vba_loop_map_num_roots", "vba_loop_map_dump_leaves", "vba_loop_map_dump_plane_var", "vba_loop_update"]


def _capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def _synth():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import synth
    return synth


def test_loop_symbols_exported_declared_and_bound():
    capi = _capi()
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    declared = set(re.findall(r"\b(vba_loop_[a-z0-9_]+)\s*\(", hdr))
    lib = capi.load()
    assert declared == set(LOOP_SYMBOLS)
    for s in LOOP_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    assert hasattr(capi, "LoopMap") and hasattr(capi.Context, "loop_update") and hasattr(capi.Context, "loop_map")


def test_adapter_loop_update_compiles(tmp_path):
    capi = _capi()
    src = tmp_path / "loop_adapter_check.cpp"
    src.write_text(r'''
#include "voxelba_adapter.hpp"
#include <cstdio>
// the device-side wrappers only have to compile and link here
int drive(vba::Context &ctx, vba::Context &loop_ctx, vba::KeyframeStore &keyframes) {
  vba::LoopMap map_loop(loop_ctx);
  map_loop.reserve(1000000, 1 << 20);
  vba::IMUST x1{}, x3{}, x_curr{};
  const vba::IMUST dx = vba::loop_dx(x1, x3);
  int n = map_loop.build(keyframes);
  n += map_loop.build(keyframes, 5, false);
  auto pv = std::make_shared<vba::PVec>(10);
  vba::ScanPose bl(x1, pv);
  std::vector<vba::ScanPose *> buf_lba2loop(3, &bl);
  std::vector<vba::IMUST> x_buf(10);
  int g_update = 1;
  vba::VoxelMap surf_map(ctx);
  n += surf_map.loop_update(map_loop, dx, buf_lba2loop, x_buf, 7, x_curr, g_update);
  std::vector<const vba::PVec *> pvec_buf(7, pv.get());
  n += surf_map.loop_update(map_loop, dx, buf_lba2loop, x_buf, 7, x_curr, g_update, &pvec_buf);
  return n + g_update + (int)map_loop.size();
}
int main() { std::printf("ok %p\n", (void *)&drive); return 0; }
''')
    exe = tmp_path / "loop_adapter_check"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lvoxelba", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def _state(rng, scale=5.0):
    from scipy.spatial.transform import Rotation
    s = np.zeros(25)
    s[0] = rng.uniform(0, 100)
    s[1:10] = Rotation.from_rotvec(rng.normal(size=3)).as_matrix().ravel()
    s[10:13] = rng.normal(size=3) * scale
    s[13:16] = rng.normal(size=3)
    s[16:22] = rng.normal(size=6) * 0.01
    s[22:25] = rng.normal(size=3) * 9.8
    return s


def test_adapter_host_algebra_equals_the_restatement():
    """vba::loop_dx, ScanPose::update and the host half of VoxelMap::loop_update (window states, x.g while g_update == 1, x_curr,
    g_update 1 -> 2), compiled without contraction, against tests/loop_oracle.py: bit for bit."""
    h = lo.host()
    h.lh_loop_update_states.restype = C.c_int
    rng = np.random.default_rng(3)
    for trial in range(40):
        x1, x3 = _state(rng), _state(rng)
        dx = np.zeros(12)
        h.lh_loop_dx(x1.ctypes.data_as(_dp), x3.ctypes.data_as(_dp), dx.ctypes.data_as(_dp))
        want = lo.loop_dx(x1, x3)
        assert np.array_equal(dx, want)
        # dx moves x1 onto x3 (the meaning of VS:2597-2598), to rounding
        moved = lo.apply_dx(x1, dx)
        assert np.abs(moved[1:13] - x3[1:13]).max() < 1e-12
        k, n_buf = int(rng.integers(0, 5)), 6
        win_count = int(rng.integers(1, n_buf + 1))
        g_update = int(trial % 3)
        bl = np.array([_state(rng) for _ in range(k)]).reshape(k, 25)
        xb = np.array([_state(rng) for _ in range(n_buf)])
        xc = _state(rng)
        bl2, xb2, xc2 = bl.copy(), xb.copy(), xc.copy()
        g2 = h.lh_loop_update_states(dx.ctypes.data_as(_dp), C.c_int(k), bl2.ctypes.data_as(_dp), C.c_int(n_buf), xb2.ctypes.data_as(_dp),
                                     C.c_int(win_count), xc2.ctypes.data_as(_dp), C.c_int(g_update))
        wbl, wxb, wxc, wg = lo.loop_update_states(dx, bl, xb, win_count, xc, g_update)
        assert g2 == wg == (2 if g_update == 1 else g_update)
        assert np.array_equal(bl2, wbl) and np.array_equal(xb2, wxb) and np.array_equal(xc2, wxc)
        assert np.array_equal(xb2[win_count:], xb[win_count:])                      # states beyond win_count are not touched
        if g_update != 1:
            assert np.array_equal(xb2[:, 22:25], xb[:, 22:25])                      # x.g only moves while g_update == 1


@pytest.mark.parametrize("cumulative", [True, False])
@pytest.mark.parametrize("size", [0, 1, 3, 5, 9])
def test_expansion_table(size, cumulative):
    """VS:2601-2625: pvec_tem is never cleared, so the last five keyframes go in 5, 4, 3, 2, 1 times (oldest first); indices below
    zero are skipped; the corrected form inserts each once."""
    calls = lo.expansion(size, 5, cumulative)
    m = min(size, 5)
    assert len(calls) == m
    cnt = lo.expansion_counts(size, 5, cumulative)
    want = np.zeros(size, dtype=np.int64)
    first = max(0, size - 5)
    for j in range(m):
        want[first + j] = (m - j) if cumulative else 1
    assert np.array_equal(cnt, want)
    if size >= 5 and cumulative:
        assert cnt[first:].tolist() == [5, 4, 3, 2, 1]
    for j, call in enumerate(calls):
        assert call == (list(range(first, first + j + 1)) if cumulative else [first + j])
    assert sum(len(c) for c in calls) == (m * (m + 1) // 2 if cumulative else m)


def test_world_transform_order():
    """((R0 x + R1 y) + R2 z) + t with every operation rounded on its own: pinned against Python floats on a case where a fused or
    re-associated form differs"""
    rng = np.random.default_rng(1)
    from scipy.spatial.transform import Rotation
    pose = np.concatenate([Rotation.from_rotvec([0.3, -0.2, 0.9]).as_matrix().ravel(), [12.5, -7.25, 1.125]])
    pts = rng.normal(size=(2000, 3)) * 20
    got = lo.world(pose, pts)
    R = pose[:9].reshape(3, 3)
    differs = 0
    for i in range(len(pts)):
        for r in range(3):
            w = ((float(R[r, 0]) * float(pts[i, 0]) + float(R[r, 1]) * float(pts[i, 1])) + float(R[r, 2]) * float(pts[i, 2])) + float(pose[9 + r])
            assert got[i, r] == w
            alt = float(R[r, 0]) * float(pts[i, 0]) + (float(R[r, 1]) * float(pts[i, 1]) + float(R[r, 2]) * float(pts[i, 2])) + float(pose[9 + r])
            differs += alt != w
    assert differs > 100


def test_covariance_check_has_power_on_the_oracle(oracle):
    """The loop_update sequence (map_loop from five keyframes in the reference's cumulative order, three buf_lba2loop scans with full
    covariances, the window, recut) on the CPU oracle, once with the fixed points' covariances and once with zeros in their place.
    At least one root that holds fixed points subdivides in this scene, and cov_add of the recut leaves differs between the two
    replays: a device that left fvar at zero could not pass the GPU comparison of cov_add."""
    synth = _synth()
    ses = lo.make_session(synth, n_kf=5, k_bl=3, W=4, extra=0, n_pts=6000)
    wl, W, n_kf, k_bl = ses["wl"], ses["W"], ses["n_kf"], ses["k_bl"]
    dx = ses["dx"]
    # keyframes as the store holds them: float values in doubles, float covariance diagonals
    clouds = [ses["points"][i].astype(np.float32).astype(np.float64) for i in range(n_kf)]
    diags = [ses["vars"][i][:, [0, 4, 8]].astype(np.float32) for i in range(n_kf)]
    kposes = [lo.move_pose(ses["poses"][i], dx) for i in range(n_kf)]
    bl = list(range(n_kf, n_kf + k_bl)); win = list(range(n_kf + k_bl, n_kf + k_bl + W))
    dumps = {}
    for fix_var in (True, False):
        om = oracle.VoxelMap(W, wl.voxel_size, wl.max_layer, wl.min_eigen_value, wl.plane_thre, wl.min_point, wl.max_points, 5)
        n = lo.replay_build(om, clouds, diags, kposes, 5, True, fix_var=fix_var)
        assert n == sum((5 - i) * len(clouds[i]) for i in range(5))
        f = lo.replay_update(om, oracle, [ses["points"][i] for i in bl], [ses["vars"][i] for i in bl],
                             [lo.move_pose(ses["poses"][i], dx) for i in bl], [ses["points"][i] for i in win],
                             [ses["vars"][i] for i in win], np.array([lo.move_pose(ses["poses"][i], dx) for i in win]), fix_var=fix_var)
        dumps[fix_var] = (om.dump_leaves(), om.dump_cov_add(), f.size())
    (d1, c1, n1), (d0, c0, n0) = dumps[True], dumps[False]
    # the covariances do not steer the octree: same leaves, same point sums, same factors
    assert np.array_equal(d1[:, :10], d0[:, :10]) and np.array_equal(d1[:, 22:32], d0[:, 22:32]) and n1 == n0 > 20
    split_with_fix = (d1[:, 3] > 0) & (d1[:, 6] > 0)                    # leaves below a root (layer > 0) that hold fixed points
    print("leaves %d, of them below a subdivided root and holding fixed points %d, cov_add rows that differ %d"
          % (len(d1), int(split_with_fix.sum()), int((c1 != c0).any(1).sum())))
    assert split_with_fix.sum() > 0, "no root holding fixed points subdivided: the scene cannot show the covariances"
    differ = (c1 != c0).any(1)
    assert differ[split_with_fix].any(), "cov_add of the recut leaves does not depend on the fixed covariances"
    # and only there: a leaf whose fixed points were never pushed down again (a root that stayed a leaf) has not added them yet
    assert not differ[(d1[:, 3] == 0)].any()
