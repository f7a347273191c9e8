"""CPU-side checks of the initialisation window (vba_init_window_*, vba_motion_init_resident): the argument that
lets the device skip the sort (tests/init_window_oracle.py over the C++ oracle's down_sampling_close), the retry boundary, the exports,
the adapter as plain C++17, and the window's device-free half under the sanitizers (tests/host/init_window_host.cpp)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import init_window_oracle as iwo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

NEW_SYMBOLS = ["vba_init_window_create", "vba_init_window_destroy", "vba_init_window_reserve", "vba_init_window_allocations",
               "vba_init_window_clear", "vba_init_window_size", "vba_init_window_push", "vba_init_window_push_points",
               "vba_init_window_read", "vba_motion_init_resident"]


def _capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def test_tie_order_is_the_ascending_index_order(oracle):
    """Curvatures quantised to 1 ms: many ties.  The kept indices in ascending order ARE the stable curvature sort of the kept cloud."""
    rng = np.random.default_rng(7)
    n = 6000
    pts = rng.uniform(-8, 8, (n, 3)).astype(np.float32).astype(np.float64)
    curv = np.sort(np.round(rng.uniform(0, 0.1, n), 3).astype(np.float32)).astype(np.float64)
    assert len(np.unique(curv)) < n // 20
    idx, retried = iwo.push(pts, curv, 0.5, 1000, oracle.down_sampling_close)
    assert not retried and 1000 <= len(idx) < n
    kept = np.asarray(oracle.down_sampling_close(pts, 0.5))
    assert not np.array_equal(kept, np.sort(kept))                       # the down-sampler itself emits another order
    assert np.array_equal(idx, iwo.sorted_by_curvature(kept, curv))
    assert np.all(np.diff(curv[idx]) >= 0)


def test_no_retry_at_exactly_min_points(oracle):
    pts, curv = iwo.grid_cloud(1000)
    assert len(pts) == 3000
    idx, retried = iwo.push(pts, curv, 0.5, 1000, oracle.down_sampling_close)
    assert len(idx) == 1000 and not retried


def test_retry_at_999(oracle):
    pts, curv = iwo.grid_cloud(999)
    assert len(oracle.down_sampling_close(pts, 0.5)) == 999
    idx, retried = iwo.push(pts, curv, 0.5, 1000, oracle.down_sampling_close)
    assert retried
    assert np.array_equal(idx, np.sort(oracle.down_sampling_close(pts, 0.25)))     # from the full cloud at half the size
    assert len(idx) > 999
    idx0, retried0 = iwo.push(pts, curv, 0.5, 0, oracle.down_sampling_close)        # min_points <= 0 never retries
    assert len(idx0) == 999 and not retried0


def test_voxel_size_below_a_millimetre_keeps_everything():
    pts, curv = iwo.grid_cloud(50)

    def close(p, vs):
        raise AssertionError("down_sampling_close must not run below 0.001")
    idx, retried = iwo.push(pts, curv, 0.0005, 0, close)
    assert np.array_equal(idx, np.arange(len(pts))) and not retried
    idx, retried = iwo.push(pts, curv, 0.0009, 1000, close)                          # both passes leave the cloud as it is
    assert np.array_equal(idx, np.arange(len(pts))) and retried


def test_symbols_exported_declared_and_bound():
    capi = _capi()
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    declared = set(re.findall(r"\b(vba_init_window_[a-z0-9_]+|vba_motion_init_resident)\s*\(", hdr))
    lib = capi.load()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    assert declared == set(NEW_SYMBOLS)
    assert hasattr(capi, "InitWindow") and hasattr(capi.Context, "motion_init_resident") and hasattr(capi.Context, "init_window")


def test_adapter_init_window_compiles(tmp_path):
    capi = _capi()
    src = tmp_path / "init_window_adapter_check.cpp"
    src.write_text(r'''
#include "voxelba_adapter.hpp"
// the device-side wrappers only have to compile and link here
int drive(vba::Context &ctx, vba::ScanFrame &frame, vba::Initialization &init, vba::LidarFactor &voxhess, vba::VoxelMap &surf_map) {
  vba::InitWindow pl_origs(ctx);
  pl_origs.reserve(10, 200000);
  bool retried = false;
  int n = pl_origs.push(frame, 0.1) + pl_origs.push(frame, 0.1, 1000, &retried);
  const double p[3] = {1, 2, 3}, c[1] = {0.0};
  pl_origs.push_points(1, p, c);
  std::vector<std::vector<vba::ImuSample>> vec_imus;
  std::vector<double> beg_times, hess;
  std::vector<vba::IMUST> x_buf;
  std::vector<std::shared_ptr<vba::PVec>> pvec_buf;
  std::deque<vba::IMU_PRE *> imu_pre_buf;
  vba::IMUST x_curr, ext;
  n += init.motion_init(pl_origs, vec_imus, beg_times, &hess, voxhess, x_buf, surf_map, pvec_buf, 10, x_curr, imu_pre_buf, ext);
  pl_origs.clear();
  return n + pl_origs.size() + (int)pl_origs.points();
}
int main() { return 0; }
''')
    out = tmp_path / "init_window_adapter_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(out),
                           "-L" + os.path.dirname(capi.LIB_PATH), "-lvoxelba", "-Wl,-rpath," + os.path.dirname(capi.LIB_PATH),
                           "-Wl,-rpath-link,/opt/rocm/lib"])


@pytest.fixture(scope="module")
def window_host():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_initw_"), "init_window_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                           os.path.join(HERE, "host", "init_window_host.cpp")])
    return out


@pytest.mark.parametrize("case", ["offsets", "as_int", "grow", "args"])
def test_window_host_under_the_sanitizers(window_host, case):
    r = subprocess.run([window_host, case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""


def test_window_host_unknown_case_is_an_error(window_host):
    assert subprocess.run([window_host, "no_such_case"], capture_output=True, timeout=60).returncode == 2
