// Host build of the IMU forward propagation and of the lane-parallel 15 x 15 inverse (voxel-slam_amd/csrc/vba_imu_ekf.hpp) for the
// CPU-side checks of tests/test_imu_ekf_cpu.py: one lane, plain arrays, no barrier; and the same text run by `nl` emulated lanes.
// Test harness only: the product runs this code on the device, spread over the lanes of one workgroup.
#include "../../voxel-slam_amd/csrc/vba_imu_ekf.hpp"

#include <condition_variable>
#include <mutex>
#include <thread>

namespace {
struct NoSync { void operator()() const {} };

// a barrier for nl threads, each of which plays one lane
struct Barrier {
  std::mutex mu; std::condition_variable cv; int n, waiting = 0; unsigned gen = 0;
  explicit Barrier(int n_) : n(n_) {}
  void wait() {
    std::unique_lock<std::mutex> l(mu);
    const unsigned g = gen;
    if (++waiting == n) { waiting = 0; gen++; cv.notify_all(); }
    else cv.wait(l, [&] { return gen != g; });
  }
};
struct LaneSync { Barrier *b; void operator()() const { b->wait(); } };
}  // namespace

// prm [16] as vbh::IE_*; state [25], cov [225] in / out; poses [m - 1][22]; end_pose [12].  Returns the row count, -1 when refused.
extern "C" int imu_ekf_propagate_host(int m, const double *imu, const double *prm, double *state, double *cov, double *poses, double *end_pose) {
  if (!vbh::imu_ekf_args_ok(m, imu, prm)) return -1;
  std::vector<double> w(vbh::IE_WORK);
  vbh::State x;
  std::memcpy(&x, state, sizeof(x));
  const int n = vbh::imu_ekf_propagate(w.data(), m, imu, prm, &x, cov, poses, end_pose, 0, 1, NoSync());
  std::memcpy(state, &x, sizeof(x));
  return n;
}

// the same by nl emulated lanes (threads on a barrier)
extern "C" int imu_ekf_propagate_lanes_host(int nl, int m, const double *imu, const double *prm, double *state, double *cov, double *poses,
                                            double *end_pose) {
  if (!vbh::imu_ekf_args_ok(m, imu, prm)) return -1;
  std::vector<double> w(vbh::IE_WORK);
  vbh::State x;
  std::memcpy(&x, state, sizeof(x));
  Barrier bar(nl);
  std::vector<int> rows(nl);
  std::vector<std::thread> th;
  for (int l = 0; l < nl; l++)
    th.emplace_back([&, l] { rows[l] = vbh::imu_ekf_propagate(w.data(), m, imu, prm, &x, cov, poses, end_pose, l, nl, LaneSync{&bar}); });
  for (auto &t : th) t.join();
  std::memcpy(state, &x, sizeof(x));
  return rows[0];
}

extern "C" void inverse_pplu_host(const double *A, double *Ainv) { vbh::inverse_pplu(A, Ainv, 15); }

extern "C" void inverse15_pplu_host(int nl, const double *A, double *Ainv) {
  double w[vbh::INV15_WORK];
  if (nl == 1) { vbh::inverse15_pplu((double *)w, A, Ainv, 0, 1, NoSync()); return; }
  Barrier bar(nl);
  std::vector<std::thread> th;
  for (int l = 0; l < nl; l++) th.emplace_back([&, l] { vbh::inverse15_pplu((double *)w, A, Ainv, l, nl, LaneSync{&bar}); });
  for (auto &t : th) t.join();
}
