// Host build of the kd mode of the resident EKF algebra (voxel-slam_amd/csrc/vba_odom_ekf.hpp with kd = 1: the step and the stop rule
// of lio_state_estimation_kdtree, voxelslam.cpp:1206-1233) for CPU-side checks against a numpy restatement
// (tests/test_kd_resident_cpu.py): one lane, a plain array as the work area, no barrier.  Test harness only: the product runs this code
// on the device, spread over the lanes of one workgroup.
#include "../../voxel-slam_amd/csrc/vba_odom_ekf.hpp"

namespace {
struct NoSync { void operator()() const {} };
// the 28 sums of k_kd_accum_dev in the 34-column layout: HTH 0-20, HTz 21-26, zeros 27-32, valid 33
void widen(const double *s28, double *s34) {
  for (int k = 0; k < 27; k++) s34[k] = s28[k];
  for (int k = 27; k < 33; k++) s34[k] = 0.0;
  s34[33] = s28[27];
}
// what the library writes into the image: P^-1 with every entry divided by 1000
void kd_cov_inv(const double *cov, double *out) {
  vbh::inverse_pplu(cov, out, 15);
  for (int k = 0; k < 225; k++) out[k] = out[k] / 1000;
}
}  // namespace

// one step on given sums: solution [15], G(:,0:6) [15][6], K_1(:,0:6) [15][6]; cov_inv_1000 = P^-1 / 1000
extern "C" void kd_ekf_step_host(const double *s28, const double *cov_inv_1000, const double *x_prop25, const double *x_curr25, double *sol,
                                 double *G, double *K) {
  double w[vbh::OE_WORK] = {0};
  vbh::State xp, xc;
  std::memcpy(&xp, x_prop25, sizeof(xp));
  std::memcpy(&xc, x_curr25, sizeof(xc));
  widen(s28, w + vbh::OE_S34);
  vbh::odom_ekf_solve((double *)w, cov_inv_1000, xp, xc, 0, 1, NoSync());
  for (int k = 0; k < 15; k++) sol[k] = w[vbh::OE_SOL + k];
  for (int k = 0; k < 90; k++) { G[k] = w[vbh::OE_G + k]; K[k] = w[vbh::OE_K + k]; }
}

// The whole loop as the device runs it: every update launch checks `done` first, and the point loop of an iteration is told whether
// the neighbour search runs (S.refind, as k_kd_match_dev / k_kd_fit_dev read it).  sums(iter, x_curr, refind, s28) fills the 28 sums.
// state / cov in/out; trace [4][3] = (valid, rot_add, tra_add); refind_seen [4] = the flag each iteration's point loop found (-1: the
// iteration did not run); refind_after / rematch_after [4] = the flag and rematch_num each update left; cov_iter = the iteration whose
// update wrote the covariance (-1: none; 100 + iter: written before the stop); launches_run = updates that passed the gate.
typedef void (*kd_sums_fn)(int iter, const double *x_curr25, int refind, double *s28);
extern "C" int kd_ekf_loop_host(kd_sums_fn sums, double *state, double *cov, double *trace, int *refind_seen, int *refind_after,
                                int *rematch_after, int *cov_iter, int *launches_run) {
  double cov_inv[225];
  kd_cov_inv(cov, cov_inv);
  vbh::OdomEkf S;
  vbh::odom_ekf_begin(S, state, cov, cov_inv);
  S.refind = 1;
  *cov_iter = -1;
  *launches_run = 0;
  for (int iter = 0; iter < vbh::ODOM_EKF_MAX_ITER; iter++) {
    refind_seen[iter] = refind_after[iter] = rematch_after[iter] = -1;
    if (S.done) continue;
    double w[vbh::OE_WORK] = {0}, s28[28] = {0};
    refind_seen[iter] = S.refind;
    sums(iter, &S.x_curr.t, S.refind, s28);
    widen(s28, w + vbh::OE_S34);
    double before[225];
    std::memcpy(before, S.P_out, sizeof(before));
    vbh::odom_ekf_iterate((double *)w, &S, iter, 0, 1, NoSync(), 1);
    (*launches_run)++;
    refind_after[iter] = S.refind; rematch_after[iter] = S.rematch_num;
    if (S.done && *cov_iter < 0) *cov_iter = iter;
    if (!S.done && std::memcmp(before, S.P_out, sizeof(before)) != 0) *cov_iter = 100 + iter;
  }
  std::memcpy(state, &S.x_curr, sizeof(S.x_curr));
  std::memcpy(cov, S.P_out, sizeof(S.P_out));
  for (int k = 0; k < 4; k++) { trace[3 * k] = S.match_num[k]; trace[3 * k + 1] = S.rot_add[k]; trace[3 * k + 2] = S.tra_add[k]; }
  return S.iterations;
}
