"""CPU-side checks of the scan log (vba_scanlog_*): the exports, the adapter's ScanLog and its readers as
plain C++17, the refusal of NULL handles without a device, and the ring bookkeeping of csrc/vba_scanlog_ring.hpp, whose stand-alone
program tests/host/scanlog_host.cpp is built by g++ with the address and undefined-behaviour sanitizers and run as a child
process, one case per run."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SCANLOG_SYMBOLS = ["vba_scanlog_create", "vba_scanlog_destroy", "vba_scanlog_reserve", "vba_scanlog_allocations", "vba_scanlog_push_window",
                   "vba_scanlog_push_points", "vba_scanlog_range", "vba_scanlog_release", "vba_scanlog_read", "vba_scanlog_export_world",
                   "vba_scanlog_loop_update", "vba_kf_build_from_log"]


def _capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def test_scanlog_symbols_exported_declared_and_bound():
    capi = _capi()
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    declared = set(re.findall(r"\b(vba_[a-z0-9_]+)\s*\(", hdr))
    lib = capi.load()
    for s in SCANLOG_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    assert {d for d in declared if d.startswith("vba_scanlog_")} <= set(SCANLOG_SYMBOLS)
    assert hasattr(capi, "ScanLog")
    for m in ("reserve", "allocations", "push_window", "push_points", "range", "release", "read", "export_world"):
        assert hasattr(capi.ScanLog, m), m
    assert hasattr(capi.KeyframeStore, "build_from_log") and hasattr(capi.Context, "scanlog_loop_update")


def test_adapter_scan_log_compiles(tmp_path):
    capi = _capi()
    src = tmp_path / "scanlog_adapter_check.cpp"
    src.write_text(r'''
#include "voxelba_adapter.hpp"
#include <cstdio>
// the device-side wrappers only have to compile and link here
long long drive(vba::Context &ctx, vba::Context &loop_ctx, vba::BtcDatabase &db) {
  vba::VoxelMap map(ctx);
  vba::ScanLog log(ctx);
  log.reserve(2000000, 64);
  std::vector<vba::IMUST> x_buf(10), bl(3);
  vba::IMUST x_curr{}, dx{};
  long long seq = log.push(map, 0);
  vba::PVec scan(10);
  seq += log.push(scan);
  vba::PVec back; std::vector<vba::XYZ> xyz;
  log.read(log.first(), &back, &xyz);
  long long n = log.size(log.first()) + (log.end() - log.first());
  vba::KeyframeStore kfs(loop_ctx);
  std::vector<vba::STD> stds_vec;
  n += kfs.build(log, log.first(), bl, 0.5 / 10, 9, 1.5, &db, &stds_vec);
  vba::LoopMap map_loop(ctx);
  int g_update = 1;
  n += map.loop_update(map_loop, dx, log, log.first(), bl, x_buf, 10, x_curr, g_update);
  n += vba::pub_localmap(ctx, log, log.first(), 1, x_buf, 0, [](const float *xyzi, int64_t m) { (void)xyzi; (void)m; });
  vba::save_pcd(log, log.first(), "/nonexistent");
  log.release(log.first() + 1);
  return n + seq;
}
int main() { std::printf("ok %p\n", (void *)&drive); return 0; }
''')
    exe = tmp_path / "scanlog_adapter_check"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lvoxelba", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)


def test_null_handles_are_bad_arguments_without_a_device():
    capi = _capi()
    lib = capi.load()
    h = C.c_void_p()
    n = C.c_int(); b = C.c_int64(); e = C.c_int64()
    bad = capi.ERR_BAD_ARG
    assert lib.vba_scanlog_create(None, C.byref(h)) == bad and not h.value
    lib.vba_scanlog_destroy(None)                                    # a no-op
    assert lib.vba_scanlog_reserve(None, C.c_int64(10), C.c_int(1)) == bad
    assert lib.vba_scanlog_allocations(None, C.byref(n), C.byref(b)) == bad
    assert lib.vba_scanlog_push_window(None, C.c_int(0), C.byref(b)) == bad
    assert lib.vba_scanlog_push_points(None, C.c_int(0), None, None, C.byref(b)) == bad
    assert lib.vba_scanlog_range(None, C.byref(b), C.byref(e), C.c_int(0), None) == bad
    assert lib.vba_scanlog_release(None, C.c_int64(0)) == bad
    assert lib.vba_scanlog_read(None, C.c_int64(0), C.c_int(0), None, None, None, C.byref(n)) == bad
    assert lib.vba_scanlog_export_world(None, None, C.c_int64(0), C.c_int(0), None, C.c_int(1), C.c_float(0), C.c_int64(0), None, C.byref(b)) == bad
    assert lib.vba_kf_build_from_log(None, None, C.c_int64(0), C.c_int(1), None, C.c_double(0.1), C.c_int(0), C.c_double(0), None, C.c_int(0),
                                     None, None, None, C.byref(n)) == bad
    assert lib.vba_scanlog_loop_update(None, None, None, None, C.c_int64(0), C.c_int(0), None, C.c_int(1), None, C.byref(n)) == bad


# ---------------------------------------------------------------- the ring bookkeeping, stand-alone
@pytest.fixture(scope="module")
def scanlog_host():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_scanlog_"), "scanlog_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", out, os.path.join(HERE, "host", "scanlog_host.cpp")])
    return out


@pytest.mark.parametrize("case", ["sizes", "exact_tail", "skip_tail", "release", "growth", "reserve_condition"])
def test_ring(scanlog_host, case):
    r = subprocess.run([scanlog_host, case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""                     # no failed expectation, no sanitizer report, no leak report at exit


def test_unknown_case_is_an_error(scanlog_host):
    assert subprocess.run([scanlog_host, "no_such_case"], capture_output=True, timeout=60).returncode == 2


def test_ring_header_is_host_only():
    text = open(os.path.join(ROOT, "voxel-slam_amd", "csrc", "vba_scanlog_ring.hpp")).read()
    assert "hip" not in text.lower() and re.findall(r'#\s*include\s+"', text) == []
