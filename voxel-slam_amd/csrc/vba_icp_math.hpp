// The arithmetic of one icp_normal iteration (loop_refine.hpp:77-134) that k_btc_icp_nn, k_btc_icp_accum and k_btc_icp_step run
// (vba_kernels_btc.hpp), written once for the device and for the g++ build of tests/host/icp_host.cpp: the 1-NN query of a source
// point, its gate and 35 terms against the matched target point, the 6x6 solve with the pose update, and the convergence /
// parameter-switch table.  No kernel, no launch, no reduction: the order of the sums is the kernels' ("What pins the
// ICP passes").
#pragma once
#include "vba_btc_svd.hpp"
#include "vba_hostmath.hpp"
#include "vba_ldlt6.hpp"

namespace vba {

constexpr int BTC_ICP_PART = 35;   // Hess (21, upper) | JacT (6) | resi | match_num | mat_norm (6)
constexpr int BTC_ICP_ITERS = 20;  // loop_refine.hpp:69

BTC_HD __attribute__((always_inline)) double btc_norm3(double x, double y, double z) {
  BTC_NOCONTRACT
  return sqrt(x * x + y * y + z * z);
}

// the point the 1-NN search is asked for: pose.second * plocal + pose.first, stored in a pcl::PointXYZ (loop_refine.hpp:81-85)
BTC_HD __attribute__((always_inline)) void btc_icp_query(const double *R, const double *t, const float *sp, float *q) {
  BTC_NOCONTRACT
  const double x = sp[0], y = sp[1], z = sp[2];
  q[0] = (float)(((R[0] * x + R[1] * y) + R[2] * z) + t[0]);
  q[1] = (float)(((R[3] * x + R[4] * y) + R[5] * z) + t[1]);
  q[2] = (float)(((R[6] * x + R[7] * y) + R[8] * z) + t[2]);
}

// One source point sp (xyz | normal) against its nearest target point tp under (R, t) and the thresholds pa (loop_refine.hpp:86-110).
// Returns the gate; s[35] is written only when it passes.
BTC_HD __attribute__((always_inline)) bool btc_icp_point(const double *R, const double *t, const double *pa, const float *sp, const float *tp, double *s) {
  BTC_NOCONTRACT
  const double x = sp[0], y = sp[1], z = sp[2];
  double pi[3], ni[3];
  for (int r = 0; r < 3; r++) {
    pi[r] = ((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + t[r];
    ni[r] = (R[3 * r] * sp[3] + R[3 * r + 1] * (double)sp[4]) + R[3 * r + 2] * (double)sp[5];
  }
  const double tn[3] = {tp[3], tp[4], tp[5]};
  const double dv[3] = {pi[0] - (double)tp[0], pi[1] - (double)tp[1], pi[2] - (double)tp[2]};
  const double ninc = btc_norm3(ni[0] - tn[0], ni[1] - tn[1], ni[2] - tn[2]), nadd = btc_norm3(ni[0] + tn[0], ni[1] + tn[1], ni[2] + tn[2]);
  const double p2p = btc_norm3(dv[0], dv[1], dv[2]);
  const double rr = (tn[0] * dv[0] + tn[1] * dv[1]) + tn[2] * dv[2];
  if (!((ninc < pa[0] || nadd < pa[1]) && fabs(rr) < pa[2] && p2p < pa[3])) return false;
  // jac.head(3) = hat(plocal) R^T tni, jac.tail(3) = tni
  double H[9];   // hat(p) R^T
  const double hp[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) H[3 * r + c] = (hp[3 * r] * R[3 * c] + hp[3 * r + 1] * R[3 * c + 1]) + hp[3 * r + 2] * R[3 * c + 2];
  double j[6];
  for (int r = 0; r < 3; r++) j[r] = (H[3 * r] * tn[0] + H[3 * r + 1] * tn[1]) + H[3 * r + 2] * tn[2];
  j[3] = tn[0]; j[4] = tn[1]; j[5] = tn[2];
  int idx = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) s[idx++] = j[r] * j[c];
  for (int r = 0; r < 6; r++) s[21 + r] = j[r] * rr;
  s[27] = 0.5 * rr * rr;
  s[28] = 1.0;
  s[29] = tn[0] * tn[0]; s[30] = tn[0] * tn[1]; s[31] = tn[0] * tn[2];
  s[32] = tn[1] * tn[1]; s[33] = tn[1] * tn[2]; s[34] = tn[2] * tn[2];
  return true;
}

// Hess dxi = -JacT on the 35 sums, pose = (R Exp(dxi.head), t + dxi.tail), mat_norm kept (loop_refine.hpp:115-117)
BTC_HD __attribute__((always_inline)) void btc_icp_solve_update(const double *acc, double *R, double *t, double *mat, double *dx) {
  BTC_NOCONTRACT
  double H[36], g[6];
  int idx = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) { H[6 * r + c] = acc[idx]; H[6 * c + r] = acc[idx]; idx++; }
  for (int r = 0; r < 6; r++) g[r] = -acc[21 + r];
  vbh::ldlt_solve_fixed<6>(H, g, dx);
  double E[9], Rn[9];
  vbh::so3_exp(dx, E);
  vbh::m3_mul(R, E, Rn);
  for (int k = 0; k < 9; k++) R[k] = Rn[k];
  for (int k = 0; k < 3; k++) t[k] = t[k] + dx[3 + k];
  for (int k = 0; k < 6; k++) mat[k] = acc[29 + k];
}

// the state table after a step (loop_refine.hpp:69, 121-130): a small step switches the thresholds the first time and ends the loop
// the second time; BTC_ICP_ITERS iterations end it whatever the step
BTC_HD __attribute__((always_inline)) void btc_icp_transition(const double *dx, double *paras, int *is_conv, int *done, int *iters) {
  BTC_NOCONTRACT
  (*iters)++;
  if (btc_norm3(dx[0], dx[1], dx[2]) < 1e-3 && btc_norm3(dx[3], dx[4], dx[5]) < 1e-3) {
    if (*is_conv) *done = 1;
    else { paras[0] = 0.1; paras[1] = 0.1; paras[2] = 0.1; paras[3] = 1; *is_conv = 1; }
  }
  if (*iters >= BTC_ICP_ITERS) *done = 1;
}

}  // namespace vba
