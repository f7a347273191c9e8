"""CPU-side checks of the global-map export (vba_kf_export_plan / vba_kf_export_world): the exports, the
host-only plan against the restatement tests/export_oracle.py AND against results worked out by hand below, and the adapter's
vba::pub_globalmap / KeyframeStore::sizes as plain C++17."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import export_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
SENT = -77


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def _raw(capi, sizes, interval, jump, cap_msgs=None, n_kf=None, null=()):
    """vba_kf_export_plan with every output pre-filled with SENT -> (status, jump_out, kf_begin, msg_end_kf buffer, n_msgs)"""
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    n = len(sizes) if n_kf is None else n_kf
    cap = len(sizes) + 1 if cap_msgs is None else cap_msgs
    j = C.c_int(SENT); nm = C.c_int(SENT)
    kb = np.full(max(n, 0) + 1, SENT, dtype=np.int64); me = np.full(len(sizes) + 4, SENT, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    st = capi.load().vba_kf_export_plan(
        C.c_int(n), sizes.ctypes.data_as(ip), C.c_int64(interval), C.c_int(jump), None if "jump_out" in null else C.byref(j),
        None if "kf_begin" in null else kb.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int(cap),
        None if "msg_end_kf" in null else me.ctypes.data_as(ip), None if "n_msgs" in null else C.byref(nm))
    return st, j.value, kb, me, nm.value


def _check(capi, sizes, interval, jump, want_jump, want_begin, want_end):
    j, kb, me = capi.kf_export_plan(sizes, interval, jump)
    oj, okb, ome = eo.plan(sizes, interval, jump)
    print("sizes %s interval %d jump %d -> jump %d kf_begin %s msg_end_kf %s" % (list(sizes), interval, jump, j, kb.tolist(), me.tolist()))
    assert (oj, okb.tolist(), ome.tolist()) == (want_jump, want_begin, want_end)          # the restatement against the hand result
    assert (j, kb.tolist(), me.tolist()) == (want_jump, want_begin, want_end)             # the library against the hand result
    assert kb.dtype == np.int64 and me.dtype == np.int32


def test_export_symbols_declared_exported_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    declared = set(re.findall(r"\b(vba_kf_export_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"vba_kf_export_plan", "vba_kf_export_world"}
    lib = capi.load()
    for s in declared:
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    assert hasattr(capi, "kf_export_plan") and hasattr(capi.Context, "kf_export_world") and hasattr(capi.KeyframeStore, "sizes")


SIZES = [0, 1, 2, 3, 4, 5, 0, 9]     # a keyframe shorter than the jump, sizes % jump == 0 and != 0, empty keyframes first and in the middle


@pytest.mark.parametrize("jump,begin", [
    (1, [0, 0, 1, 3, 6, 10, 15, 15, 24]),        # counts 0 1 2 3 4 5 0 9
    (2, [0, 0, 1, 2, 4, 6, 9, 9, 14]),           # counts 0 1 1 2 2 3 0 5
    (3, [0, 0, 1, 2, 3, 5, 7, 7, 10]),           # counts 0 1 1 1 2 2 0 3
    (10, [0, 0, 1, 2, 3, 4, 5, 5, 6]),           # counts 0 1 1 1 1 1 0 1
])
def test_plan_counts_one_message(capi, jump, begin):
    _check(capi, SIZES, 1000, jump, jump, begin, [8])


@pytest.mark.parametrize("jump,begin,ends", [
    # running counts at interval 5, cut on > 5:
    (1, [0, 0, 1, 3, 6, 10, 15, 15, 24], [4, 6, 8, 8]),   # 0 1 3 6| 4 9| 0 9| : the empty keyframe 6 follows a cut, the last message is empty
    (2, [0, 0, 1, 2, 4, 6, 9, 9, 14], [5, 8, 8]),         # 0 1 2 4 6| 3 3 8| : the empty keyframe 6 precedes the cut of keyframe 7
    (3, [0, 0, 1, 2, 3, 5, 7, 7, 10], [6, 8]),            # 0 1 2 3 5 7| 0 3 : 5 == interval does not cut
    (10, [0, 0, 1, 2, 3, 4, 5, 5, 6], [8, 8]),            # 0 1 2 3 4 5 5 6| : cut at the very end, then the empty final message
])
def test_plan_cuts_around_empty_keyframes(capi, jump, begin, ends):
    _check(capi, SIZES, 5, jump, jump, begin, ends)


def test_plan_cut_is_strictly_more_than_the_interval(capi):
    # running 3, 7 (== 7: no cut), 8 (> 7: cut) | 7 (no cut), 15 (cut) | empty final message
    _check(capi, [3, 4, 1, 7, 8], 7, 1, 1, [0, 3, 7, 8, 15, 23], [3, 5, 5])
    # the same sizes ending on the exact interval: the final message carries the remainder
    _check(capi, [3, 4, 1, 7], 7, 1, 1, [0, 3, 7, 8, 15], [3, 4])


def test_plan_last_message_empty_and_no_keyframes(capi):
    _check(capi, [8], 7, 1, 1, [0, 8], [1, 1])
    _check(capi, [], 7, 0, 1, [0], [0])                     # n_kf = 0: one empty message, psize 0 -> jump 1
    _check(capi, [], 7, 4, 4, [0], [0])
    _check(capi, [0, 0], 7, 0, 1, [0, 0, 0], [2])


def test_plan_jump_rule(capi):
    # jump = psize / (10 * interval_size) + 1 in integer division, interval_size 7
    _check(capi, [30, 39], 7, 0, 1, [0, 30, 69], [1, 2, 2])             # psize 69 = 10 * 7 - 1 -> 1
    _check(capi, [30, 40], 7, 0, 2, [0, 15, 35], [1, 2, 2])             # psize 70 = 10 * 7 -> 2: counts 15, 20
    # the reference's interval: 49 999 999 points -> 1, 50 000 000 -> 2 (hand result only: the restatement walks every point)
    j, kb, me = capi.kf_export_plan([49_999_999], 5_000_000, 0)
    assert (j, kb.tolist(), me.tolist()) == (1, [0, 49_999_999], [1, 1])
    j, kb, me = capi.kf_export_plan([25_000_000, 25_000_000], 5_000_000, 0)
    assert (j, kb.tolist(), me.tolist()) == (2, [0, 12_500_000, 25_000_000], [1, 2, 2])


def test_plan_cap_msgs_below_the_message_count(capi):
    st, j, kb, me, nm = _raw(capi, SIZES, 5, 1, cap_msgs=2)
    assert st == 0 and nm == 4 and j == 1                  # *n_msgs is exact
    assert me[:2].tolist() == [4, 6] and (me[2:] == SENT).all()   # nothing past the cap
    assert kb.tolist() == [0, 0, 1, 3, 6, 10, 15, 15, 24]
    st, j, kb, me, nm = _raw(capi, SIZES, 5, 1, cap_msgs=0, null=("msg_end_kf",))     # NULL msg_end_kf is allowed with cap_msgs == 0
    assert st == 0 and nm == 4 and kb[-1] == 24


def test_plan_refuses_a_total_of_2_pow_32(capi):
    # the reference's 32-bit psize would wrap to 0 here and choose jump 1; the sum is formed in 64 bits and refused instead
    st, j, kb, me, nm = _raw(capi, [INT32_MAX, INT32_MAX, 2], 5_000_000, 0)
    assert st == capi.ERR_BAD_ARG
    assert j == SENT and nm == SENT and (kb == SENT).all() and (me == SENT).all()
    # one point less is a valid plan: 4294967295 / 50000000 + 1 = 86; counts ceil(2147483647 / 86) = 24970741, 24970741, 1
    j, kb, me = capi.kf_export_plan([INT32_MAX, INT32_MAX, 1], 5_000_000, 0)
    assert (j, kb.tolist(), me.tolist()) == (86, [0, 24970741, 49941482, 49941483], [1, 2, 3])
    # a jump given by the caller is used as given, whatever the sum
    j, kb, me = capi.kf_export_plan([INT32_MAX, INT32_MAX, 2], 5_000_000, 1)
    assert j == 1 and kb.tolist() == [0, INT32_MAX, 2 * INT32_MAX, 2 ** 32] and me.tolist() == [1, 2, 3]


@pytest.mark.parametrize("what,kw", [
    ("n_kf < 0", dict(sizes=[1, 2], interval=7, jump=1, n_kf=-1)),
    ("a negative size", dict(sizes=[1, -2, 3], interval=7, jump=1)),
    ("a negative size with the jump rule", dict(sizes=[1, 2, -3], interval=7, jump=0)),
    ("interval_size < 1", dict(sizes=[1, 2], interval=0, jump=1)),
    ("jump < 0", dict(sizes=[1, 2], interval=7, jump=-1)),
    ("NULL jump_out", dict(sizes=[1, 2], interval=7, jump=1, null=("jump_out",))),
    ("NULL kf_begin", dict(sizes=[1, 2], interval=7, jump=1, null=("kf_begin",))),
    ("NULL n_msgs", dict(sizes=[1, 2], interval=7, jump=1, null=("n_msgs",))),
    ("NULL msg_end_kf with cap_msgs > 0", dict(sizes=[1, 2], interval=7, jump=1, null=("msg_end_kf",))),
])
def test_plan_argument_errors_write_nothing(capi, what, kw):
    st, j, kb, me, nm = _raw(capi, kw.pop("sizes"), kw.pop("interval"), kw.pop("jump"), **kw)
    assert st == capi.ERR_BAD_ARG, what
    assert j == SENT and nm == SENT and (kb == SENT).all() and (me == SENT).all(), what


def test_restatement_points_agree_with_the_plan(capi):
    """export_oracle.points on values small enough to check by eye (identity pose, keyframes of 3 and 4 points, jump 2), and its
    rows per keyframe against the library's plan: the GPU tests compare vba_kf_export_world with this function, so the two halves
    of the restatement and vba_kf_export_plan must describe the same sequence."""
    ident = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    shift = np.concatenate([np.eye(3).ravel(), [10.0, 0, 0]])
    a = np.arange(9, dtype=np.float64).reshape(3, 3); b = 100 + np.arange(12, dtype=np.float64).reshape(4, 3)
    got = eo.points([a, b], [ident, shift], [3, 5], 2)
    want = np.array([[0, 1, 2, 3], [6, 7, 8, 3], [110, 101, 102, 5], [116, 107, 108, 5]], dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)       # rows 0, 2 of a; rows 0, 2 of b (not 1, 3: the stride restarts)
    assert eo.points([], [], [], 1).shape == (0, 4)
    rng = np.random.default_rng(4)
    clouds = [rng.uniform(-5, 5, (n, 3)) for n in SIZES]
    for jump in (1, 2, 3, 10):
        _, kb, _ = capi.kf_export_plan(SIZES, 1000, jump)
        rows = eo.points(clouds, [shift] * len(SIZES), list(range(len(SIZES))), jump)
        assert len(rows) == kb[-1]
        for k in range(len(SIZES)):                           # the intensity column says which keyframe a row came from
            assert (rows[kb[k]:kb[k + 1], 3] == k).all()


def test_adapter_pub_globalmap_compiles(capi, tmp_path):
    src = tmp_path / "export_adapter_check.cpp"
    src.write_text(r'''
#include "voxelba_adapter.hpp"
#include <cstdio>
// the device-side wrappers only have to compile and link here
int64_t drive(vba::Context &ctx, vba::KeyframeStore &a, vba::KeyframeStore &b) {
  std::vector<vba::KeyframeStore *> relc_submaps{&a, &b};
  std::vector<int> ids{1, 0};
  int64_t total = 0; int msgs = 0;
  const int jump = vba::pub_globalmap(ctx, relc_submaps, ids, [&](const float *xyzi, int64_t n) { total += n + (n ? (int64_t)xyzi[3] : 0); msgs++; });
  const std::vector<int> sz = a.sizes();
  return total + msgs + jump + (int64_t)sz.size();
}
// the host-only half runs without a device
int main() {
  const int sizes[3] = {4, 0, 5};
  int jump = -1, n_msgs = -1, msg_end[4];
  int64_t kf_begin[4];
  if (vba_kf_export_plan(3, sizes, 3, 2, &jump, kf_begin, 4, msg_end, &n_msgs) != VBA_OK) return 2;
  std::printf("ok %p %d %d %lld %d\n", (void *)&drive, jump, n_msgs, (long long)kf_begin[3], msg_end[0]);
  return (jump == 2 && n_msgs == 2 && kf_begin[3] == 5 && msg_end[0] == 3 && msg_end[1] == 3) ? 0 : 3;
}
''')
    exe = tmp_path / "export_adapter_check"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lvoxelba", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
