"""CPU-side checks of the IMU forward propagation: the g++ build of csrc/vba_imu_ekf.hpp (-O2
-ffp-contract=off) against the high-precision reference and counted bars of tests/imu_ekf_ref.py on its corpus, the teeth, the
lane-parallel 15 x 15 inverse bit for bit against vbh::inverse_pplu, the host entry point vba_imu_ekf_propagate and its refusals, the
exports, and the adapter's ImuEkf as a stand-alone C++17 program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import imu_ekf_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def host():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_imu_ekf_"), "libimuekfhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-pthread", "-shared", "-o", out,
                           os.path.join(HERE, "host", "imu_ekf_host.cpp")])
    return C.CDLL(out)


@pytest.fixture(scope="module")
def corpus():
    c = R.corpus()
    return {k: (v, R.reference(v)) for k, v in c.items()}


def prm_of(case):
    return np.concatenate([[case["last_end"], case["beg"], case["end"], case["sg"]], case["noise"]])


def run_host(host, case, nl=1):
    m = case["m"]
    imu = np.ascontiguousarray(case["imu"], dtype=np.float64); prm = prm_of(case)
    st = np.array(case["state"], dtype=np.float64); cov = np.array(case["cov"], dtype=np.float64)
    poses = np.zeros((m - 1, 22)); end = np.zeros(12)
    if nl == 1:
        n = host.imu_ekf_propagate_host(C.c_int(m), _p(imu), _p(prm), _p(st), _p(cov), _p(poses), _p(end))
    else:
        n = host.imu_ekf_propagate_lanes_host(C.c_int(nl), C.c_int(m), _p(imu), _p(prm), _p(st), _p(cov), _p(poses), _p(end))
    return dict(n=n, state=st, cov=cov, poses=poses[:max(n, 0)], end_pose=end)


def _report(name, q):
    print("%-8s " % name + "  ".join("%s %.3g of its bar (k <= %d)" % (k, v[0], v[1]) for k, v in q.items()))


CASES = ("m6", "m21", "m64", "still", "repeat")


def test_corpus_holds_what_it_claims(corpus):
    assert set(corpus) == set(CASES)
    assert [corpus[k][0]["m"] for k in ("m6", "m21", "m64")] == [6, 21, 64]
    for name, (case, ref) in corpus.items():
        t, le = case["imu"][:, 0], case["last_end"]
        assert any(t[j] < le <= t[j + 1] for j in range(case["m"] - 1)), name          # a straddling interval
        assert ref["n"] == sum(not t[j + 1] < le for j in range(case["m"] - 1))
    for name in ("m21", "m64"):
        case = corpus[name][0]
        assert (case["imu"][1:, 0] < case["last_end"]).sum() >= 2                      # intervals wholly before it
        assert corpus[name][1]["n"] < case["m"] - 1
    assert corpus["m6"][0]["end"] > corpus["m6"][0]["imu"][-1, 0] and corpus["m21"][0]["end"] < corpus["m21"][0]["imu"][-1, 0]
    still = corpus["still"][0]
    assert np.linalg.norm(0.5 * (still["imu"][:-1, 1:4] + still["imu"][1:, 1:4]) - still["state"][16:19], axis=1).max() < 1e-8
    assert (np.diff(corpus["repeat"][0]["imu"][:, 0]) == 0).sum() == 1
    assert corpus["m21"][0]["sg"] == 9.8


@pytest.mark.parametrize("name", CASES)
def test_host_build_within_the_bars(host, corpus, name):
    case, ref = corpus[name]
    got = run_host(host, case)
    assert got["n"] == ref["n"]
    q = R.ratios(ref, got)
    _report(name, q)
    assert all(v[0] <= 1.0 for v in q.values()), q
    assert got["state"][0] == case["end"] and np.array_equal(got["state"][16:25], case["state"][16:25])     # t; bg, ba, g untouched
    assert np.array_equal(got["end_pose"], got["state"][1:13])


@pytest.mark.parametrize("name", CASES)
def test_lanes_give_the_same_bits(host, corpus, name):
    """an element is computed by one lane in one fixed order whatever nl is"""
    case = corpus[name][0]
    a, b = run_host(host, case), run_host(host, case, nl=64)
    assert a["n"] == b["n"]
    for k in ("state", "cov", "poses", "end_pose"):
        assert np.array_equal(a[k], b[k]), k


def test_model_control(corpus):
    """the f64 model of the teeth with nothing altered stays within the bars"""
    for name, (case, ref) in corpus.items():
        got = R.model(case)
        assert got["n"] == ref["n"]
        q = R.ratios(ref, got)
        _report(name, q)
        assert all(v[0] <= 1.0 for v in q.values()), (name, q)


@pytest.mark.parametrize("tooth", R.TEETH)
def test_teeth(corpus, tooth):
    worst = {}
    for name, (case, ref) in corpus.items():
        q = R.ratios(ref, R.model(case, tooth))
        worst[name] = max(v[0] for v in q.values())
    print(tooth, {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) > 1.0, (tooth, worst)


def _spd(rng, scale):
    A = rng.normal(0, 1, (15, 15))
    return scale * (A @ A.T / 15 + np.diag(rng.uniform(0.1, 1.0, 15)))


def test_inverse15_is_inverse_pplu_bit_for_bit(host):
    rng = np.random.default_rng(7)
    mats = [_spd(rng, s) for s in (1.0, 1e-4, 1e-6, 1e3)]
    cov = np.eye(15) * 1e-4; cov[9:, 9:] = np.eye(6) * 1e-5
    mats.append(cov)
    ex = _spd(rng, 1.0); ex[0, 0] = 1e-3; ex[5, 0] = ex[0, 5] = 4.0      # column 0 takes row 5: a row exchange
    mats.append(ex)
    tie = _spd(rng, 1.0); tie[3, 0] = tie[0, 0]; tie[7, 0] = -tie[0, 0]   # equal magnitudes: the first row wins
    mats.append(tie)
    mats.append(rng.normal(0, 1, (15, 15)))                               # unsymmetric: exchanges at most columns
    for A in mats:
        A = np.ascontiguousarray(A)
        want = np.zeros((15, 15)); host.inverse_pplu_host(_p(A), _p(want))
        assert np.abs(want @ A - np.eye(15)).max() < 1e-6 * np.linalg.cond(A)
        for nl in (1, 64):
            got = np.full((15, 15), np.nan); host.inverse15_pplu_host(C.c_int(nl), _p(A), _p(got))
            assert np.array_equal(got, want), nl
    piv = np.argmax(np.abs(ex[:, 0]))
    assert piv == 5


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


NEW = ["vba_imu_ekf_propagate", "vba_odom_state_create", "vba_odom_state_destroy", "vba_odom_state_reserve", "vba_odom_state_allocations",
       "vba_odom_state_set", "vba_odom_state_get", "vba_odom_state_poses", "vba_odom_state_propagate", "vba_scan_prepare_on_state",
       "vba_odom_lio_state_estimation_on_state", "vba_map_pvec_update_cut_voxel_on_state"]


def test_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    declared = set(re.findall(r"\b(vba_[a-z0-9_]+)\s*\(", hdr))
    lib = capi.load()
    for s in NEW:
        assert s in declared and s in capi.EXPORTS and hasattr(lib, s), s
    assert "EK:" in hdr[hdr.index("vba_imu_ekf_propagate") - 3000:hdr.index("vba_imu_ekf_propagate")]


def _call(capi, case, **over):
    c = dict(case); c.update(over)
    return capi.imu_ekf_propagate(c["imu"], c["noise"], c["last_end"], c["beg"], c["end"], c["state"], c["cov"], c["sg"])


@pytest.mark.parametrize("name", CASES)
def test_library_host_call_within_the_bars(capi, corpus, name):
    case, ref = corpus[name]
    st, cov, poses, end = _call(capi, case)
    assert len(poses) == ref["n"]
    q = R.ratios(ref, dict(state=st, cov=cov, poses=poses, end_pose=end))
    _report(name, q)
    assert all(v[0] <= 1.0 for v in q.values()), q


def test_library_host_call_refusals(capi, corpus):
    case = corpus["m21"][0]
    lib = capi.load()

    def refused(**over):
        c = dict(case); c.update(over)
        imu = np.ascontiguousarray(c["imu"], dtype=np.float64)
        st = np.array(c["state"]); cov = np.array(c["cov"]); poses = np.full((len(imu), 22), np.nan); end = np.full(12, np.nan); n = C.c_int(-7)
        r = lib.vba_imu_ekf_propagate(C.c_int(c.get("m_arg", len(imu))), _p(imu), _p(np.ascontiguousarray(c["noise"])), C.c_double(c["sg"]),
                                      C.c_double(c["last_end"]), C.c_double(c["beg"]), C.c_double(c["end"]), _p(st), _p(cov), _p(poses), _p(end), C.byref(n))
        assert r == capi.ERR_BAD_ARG, over.keys()
        assert np.array_equal(st, c["state"]) and np.array_equal(cov, c["cov"]) and np.isnan(poses).all() and np.isnan(end).all() and n.value == -7

    refused(m_arg=1)
    refused(last_end=case["imu"][-1, 0] + 1.0, beg=case["imu"][-1, 0] + 1.0)                      # every tail lies before it
    refused(beg=case["last_end"] - 0.011)                                                        # LiDAR time regress
    bad = case["imu"].copy(); bad[5, 2] = np.nan
    refused(imu=bad)
    refused(end=np.inf)
    nz = case["noise"].copy(); nz[4] = np.nan
    refused(noise=nz)
    refused(sg=np.nan)
    assert _call(capi, case, beg=case["last_end"] - 0.0099)[2].shape[0] == corpus["m21"][1]["n"]   # inside the tolerance: accepted


# ------------------------------------------------------------------------------------------------ the adapter's ImuEkf
ADAPTER_MAIN = r'''
#include "voxelba_adapter.hpp"
#include <cstdio>
// three consecutive scans through vba::ImuEkf on the host: prints what EK:125-133 leave behind
int main() {
  vba::ImuEkf ekf;
  ekf.imu_topic = "/other/imu";
  ekf.min_init_num = 3;
  for (int k = 0; k < 3; k++) { ekf.cov_gyr[k] = 0.01; ekf.cov_acc[k] = 0.1; ekf.cov_bias_gyr[k] = ekf.cov_bias_acc[k] = 1e-4; }
  vba::IMUST x;
  for (int i = 0; i < 15; i++) x.cov[16 * i] = 1e-4;
  double t = 100.0;
  auto sample = [&](int i) { vba::ImuSample s; s.t = t; for (int k = 0; k < 3; k++) { s.gyr[k] = 0.01 * (i % 7) - 0.02 * k; s.acc[k] = (k == 2 ? 9.8 : 0.1 * (i % 3)); } return s; };
  int idx = 0;
  for (int scan = 0; scan < 4; scan++) {
    std::deque<vba::ImuSample> imus;
    for (int i = 0; i < 5; i++) { t += 0.005; imus.push_back(sample(idx++)); }
    ekf.pcl_beg_time = imus.front().t - 0.002;
    ekf.pcl_end_time = imus.back().t + (scan % 2 ? 0.001 : -0.001);
    const double last_before = ekf.last_pcl_end_time;
    const int r = ekf.process(x, imus);
    std::printf("scan %d r %d init %d num %d size %zu n_poses %d\n", scan, r, (int)ekf.init_flag, ekf.init_num, imus.size(), ekf.n_poses);
    std::printf("front %.17g back %.17g last_imu %.17g last_end %.17g before %.17g xt %.17g\n", imus.front().t, imus.back().t, ekf.last_imu.t,
                ekf.last_pcl_end_time, last_before, x.t);
    std::printf("g %.17g %.17g %.17g sg %.17g p %.17g %.17g %.17g rows %zu\n", x.g[0], x.g[1], x.g[2], ekf.scale_gravity, x.p[0], x.p[1], x.p[2],
                ekf.imu_poses.size());
  }
  // a regress is an exception and leaves the deque as it came
  std::deque<vba::ImuSample> imus;
  for (int i = 0; i < 5; i++) { t += 0.005; imus.push_back(sample(idx++)); }
  ekf.pcl_beg_time = ekf.last_pcl_end_time - 0.02; ekf.pcl_end_time = imus.back().t;
  try { ekf.process(x, imus); std::printf("regress accepted\n"); } catch (const std::exception &e) { std::printf("regress refused size %zu\n", imus.size()); }
  return 0;
}
'''


def test_adapter_imu_ekf_under_sanitizers(capi, tmp_path):
    """plain C++17, its own main, address + undefined-behaviour sanitizers; the deque bookkeeping against a numpy restatement"""
    src = tmp_path / "imu_ekf_adapter.cpp"
    src.write_text(ADAPTER_MAIN)
    exe = tmp_path / "imu_ekf_adapter"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lvoxelba", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath-link,/opt/rocm/lib"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, env=env).stdout.splitlines()
    print("\n".join(out))
    assert out[-1] == "regress refused size 5"
    # the numpy restatement: the same samples, EK:167-214 and EK:43, EK:125-133
    t, idx = 100.0, 0
    init_num, mean_acc, last_imu_t, last_end, init_flag = 0, np.zeros(3), None, 0.0, False
    for scan in range(4):
        ts, accs = [], []
        for i in range(5):
            t += 0.005
            ts.append(t); accs.append(np.array([0.1 * (idx % 3), 0.1 * (idx % 3), 9.8])); idx += 1
        beg, end = ts[0] - 0.002, ts[-1] + (0.001 if scan % 2 else -0.001)
        head = out[3 * scan].split(); mid = out[3 * scan + 1].split(); tail = out[3 * scan + 2].split()
        if not init_flag:
            for a in accs:
                if init_num:
                    mean_acc = mean_acc + (a - mean_acc) / init_num
                else:
                    mean_acc, init_num = a.copy(), 1
                init_num += 1
            init_flag = init_num > 3
            assert head[3] == "0" and int(head[7]) == init_num and int(head[5]) == int(init_flag) and head[9] == "5"
            assert [float(x) for x in tail[1:4]] == list(-mean_acc * 1.0) and float(tail[5]) == 1.0
            assert float(mid[1]) == ts[0] and float(mid[3]) == ts[-1]                      # the deque is not edited
            last_imu_t, last_end = ts[-1], end
            assert float(mid[5]) == last_imu_t and float(mid[7]) == last_end
            continue
        rows = [last_imu_t] + ts                                                            # push_front(last_imu)
        n_poses = sum(not rows[j + 1] < last_end for j in range(len(rows) - 1))
        assert head[3] == "1" and head[9] == "6" and int(head[11]) == n_poses and int(tail[-1]) == 22 * n_poses
        assert float(mid[1]) == last_end                                                    # front re-stamped to the old last_pcl_end_time
        assert float(mid[3]) == end                                                         # back re-stamped to pcl_end_time
        assert float(mid[5]) == ts[-1]                                                      # last_imu keeps the back as it came
        assert float(mid[7]) == end and float(mid[9]) == last_end and float(mid[11]) == end
        last_imu_t, last_end = ts[-1], end
    assert init_flag
