// Host build of the EKF algebra of the resident odometry loop (voxel-slam_amd/csrc/vba_odom_ekf.hpp) for CPU-side checks against a
// numpy restatement of voxelslam.cpp:1053-1086 (tests/test_odom_ekf_cpu.py): one lane, a plain array as the work area, no barrier.
// Test harness only: the product runs this code on the device, spread over the lanes of one workgroup.
#include "../../voxel-slam_amd/csrc/vba_odom_ekf.hpp"

namespace {
struct NoSync { void operator()() const {} };
}

// one step on given sums: solution [15], G(:,0:6) [15][6], K_1(:,0:6) [15][6]
extern "C" void odom_ekf_step_host(const double *s34, const double *cov_inv, const double *x_prop25, const double *x_curr25, double *sol,
                                   double *G, double *K) {
  double w[vbh::OE_WORK] = {0};
  vbh::State xp, xc;
  std::memcpy(&xp, x_prop25, sizeof(xp));
  std::memcpy(&xc, x_curr25, sizeof(xc));
  for (int k = 0; k < 34; k++) w[vbh::OE_S34 + k] = s34[k];
  vbh::odom_ekf_solve((double *)w, cov_inv, xp, xc, 0, 1, NoSync());
  for (int k = 0; k < 15; k++) sol[k] = w[vbh::OE_SOL + k];
  for (int k = 0; k < 90; k++) { G[k] = w[vbh::OE_G + k]; K[k] = w[vbh::OE_K + k]; }
}

// the whole loop as the device runs it: every launch of the four checks `done` first.  sums(user-free callback) fills the 34 sums
// for the current x_curr.  state / cov in/out; trace [4][3] = (match_num, rot_add, tra_add); cov_iter = the iteration whose update
// wrote the covariance (-1: none), launches_run = update launches that did not return at the gate.  Returns the iteration count.
typedef void (*sums_fn)(int iter, const double *x_curr25, double *s34);
extern "C" int odom_ekf_loop_host(sums_fn sums, double *state, double *cov, double *trace, int *cov_iter, int *launches_run, double *nnt) {
  double cov_inv[225];
  vbh::inverse_pplu(cov, cov_inv, 15);
  vbh::OdomEkf S;
  vbh::odom_ekf_begin(S, state, cov, cov_inv);
  *cov_iter = -1;
  *launches_run = 0;
  for (int iter = 0; iter < vbh::ODOM_EKF_MAX_ITER; iter++) {
    if (S.done) continue;
    double w[vbh::OE_WORK] = {0};
    sums(iter, &S.x_curr.t, w + vbh::OE_S34);
    double before[225];
    std::memcpy(before, S.P_out, sizeof(before));
    vbh::odom_ekf_iterate((double *)w, &S, iter, 0, 1, NoSync());
    (*launches_run)++;
    if (S.done && *cov_iter < 0) *cov_iter = iter;
    if (!S.done && std::memcmp(before, S.P_out, sizeof(before)) != 0) *cov_iter = 100 + iter;   // written before the stop: wrong
  }
  std::memcpy(state, &S.x_curr, sizeof(S.x_curr));
  std::memcpy(cov, S.P_out, sizeof(S.P_out));
  for (int k = 0; k < 4; k++) { trace[3 * k] = S.match_num[k]; trace[3 * k + 1] = S.rot_add[k]; trace[3 * k + 2] = S.tra_add[k]; }
  for (int k = 0; k < 9; k++) nnt[k] = S.nnt[k];
  return S.iterations;
}

extern "C" double odom_nnt_eig_min_host(const double *nnt9) { return vbh::odom_nnt_eig_min(nnt9); }
