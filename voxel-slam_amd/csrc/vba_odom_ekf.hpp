// The 15 x 15 algebra of one iterated-EKF scan-to-map update (VOXEL_SLAM::lio_state_estimation, voxelslam.cpp:1053-1086) on the 34
// sums of one point loop: [HTH upper (21) | HTz (6) | nnt upper (6) | match_num].  Nothing here knows about the voxel map.
//
// Every function is written for `nl` cooperating lanes: lane `lane` computes the elements e = lane, lane + nl, ... of each stage
// and calls sync() between stages.  The device-resident loop (vba_kernels_odom.hpp) runs it with the lanes of one workgroup on a
// work area in the LDS and a barrier as sync(); a host caller passes lane 0 of 1, a plain array and a sync() that does nothing
// (tests/host/odom_ekf_host.cpp).  An element is computed by one lane in one fixed order whatever nl is, so the two give the same
// bits up to sin / cos / acos of the two math libraries when both are compiled without floating-point contraction.
//
// K_1(:,0:6), the only columns of (H_T_H + cov_inv)^-1 that the step reads, comes from a Gauss-Jordan elimination with partial
// pivoting on the 15 x 21 system [A | I(:,0:6)].  Rows are not exchanged: the row taken by column k is remembered in four bits of a
// 64-bit word that every lane keeps for itself, so a pivot step reads column k, the pivot row and its own element, writes its own
// element, and needs ONE sync().  The pivots are those of vbh::inverse_pplu (largest magnitude among the rows not yet taken, the first
// one on a tie).
#pragma once
#include "vba_hostmath.hpp"

// the functions below are compiled without floating-point contraction wherever they are compiled (g++ takes -ffp-contract=off)
#if defined(__clang__)
#define VBE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VBE_NO_CONTRACT
#endif

namespace vbh {

// The state of one call.  On the device it lives in HBM between the launches: the host writes the whole image once (parameter
// block filled in, x_curr = x_prop, the rest zero) and reads the result block back once.
struct OdomEkf {
  // ---- parameter block (read only after the upload)
  State x_prop;                 // VS:965
  double P[225];                // x_curr.cov on entry; unchanged until the stop (VS:999-1000 read it in every iteration)
  double cov_inv[225];          // P^-1 (VS:987), computed by the caller
  // ---- result block
  State x_curr;
  double P_out[225];            // (I - G) P, written at the stop (VS:1082-1086)
  double nnt[9];                // of the last iteration run
  double rot_add[4], tra_add[4];
  int match_num[4];
  int iterations;               // iterations run so far
  int rematch_num;
  int done;                     // the stop rule has fired: later launches return at once
  int n_map;                    // kd mode: points of the re-sampled map, written by the down-sampler's scan after the loop
  // ---- what the next point loop reads: pose of x_curr, rotation and translation blocks of P
  double R[9], t[3], rot_var[9], tsl_var[9];
  // ---- kd mode only (lio_state_estimation_kdtree, VS:1159, VS:1216-1227): whether the next iteration searches its neighbours again
  // (the caller sets it to 1 after odom_ekf_begin), whether an iteration has converged yet
  int refind, converged_once;
};
static const int ODOM_EKF_MAX_ITER = 4;

// work area, in doubles
enum {
  OE_S34 = 0,                   // the 34 sums
  OE_HTH = OE_S34 + 34,         // 6 x 6
  OE_HTZ = OE_HTH + 36,         // 6
  OE_AUG = OE_HTZ + 6,          // 15 x 21: [H_T_H + cov_inv | I(:,0:6)], row stride 21 (odd: no LDS bank pattern)
  OE_K = OE_AUG + 15 * 21,      // K_1(:,0:6), 15 x 6
  OE_G = OE_K + 90,             // G(:,0:6), 15 x 6
  OE_KH = OE_G + 90,            // K_1(:,0:6) HTz, 15
  OE_VEC = OE_KH + 15,          // x_prop - x_curr, 15
  OE_SOL = OE_VEC + 15,         // solution, 15
  OE_FLAG = OE_SOL + 15,        // 1.0 when this iteration is the last
  OE_WORK = OE_FLAG + 1
};

// row that column k took, from the packed table
VBH_HD inline int oe_row_of(unsigned long long perm, int k) { return (int)((perm >> (4 * k)) & 15ull); }

// Stages 3-4 of the update: from w[OE_S34..] and (x_prop, x_curr, cov_inv) to w[OE_SOL..], w[OE_G..].  WP is a pointer to double in
// whatever address space the work area lives in.
template <class WP, class Sync>
VBH_HD inline void odom_ekf_solve(WP w, const double *cov_inv, const State &x_prop, const State &x_curr, int lane, int nl, Sync sync) {
  VBE_NO_CONTRACT
  // HTH, HTz from the packed sums; vec = x_prop - x_curr (TL:164-173)
  for (int e = lane; e < 36; e += nl) {
    const int r = e / 6, c = e % 6, a = r < c ? r : c, b = r < c ? c : r;
    w[OE_HTH + e] = w[OE_S34 + a * 6 - a * (a - 1) / 2 + (b - a)];
  }
  for (int e = lane; e < 6; e += nl) w[OE_HTZ + e] = w[OE_S34 + 21 + e];
  if (lane == 0) {
    double RtR[9], lg[3];
    m3_Tmul(x_curr.R, x_prop.R, RtR);
    so3_log(RtR, lg);
    for (int k = 0; k < 3; k++) {
      w[OE_VEC + k] = lg[k]; w[OE_VEC + 3 + k] = x_prop.p[k] - x_curr.p[k]; w[OE_VEC + 6 + k] = x_prop.v[k] - x_curr.v[k];
      w[OE_VEC + 9 + k] = x_prop.bg[k] - x_curr.bg[k]; w[OE_VEC + 12 + k] = x_prop.ba[k] - x_curr.ba[k];
    }
  }
  sync();
  for (int e = lane; e < 15 * 21; e += nl) {
    const int r = e / 21, c = e % 21;
    double v;
    if (c < 15) { v = cov_inv[r * 15 + c]; if (r < 6 && c < 6) v += w[OE_HTH + r * 6 + c]; }
    else v = (r == c - 15) ? 1.0 : 0.0;
    w[OE_AUG + e] = v;
  }
  sync();
  // Gauss-Jordan, one sync per pivot
  unsigned long long perm = 0;
  unsigned int used = 0;
  for (int k = 0; k < 15; k++) {
    int p = -1;
    double big = -1.0;
    for (int r = 0; r < 15; r++) {
      const double a = std::fabs(w[OE_AUG + r * 21 + k]);
      if (!((used >> r) & 1u) && (a > big || p < 0)) { big = a; p = r; }
    }
    used |= 1u << p;
    perm |= (unsigned long long)p << (4 * k);
    const double piv = w[OE_AUG + p * 21 + k];
    for (int e = lane; e < 15 * 21; e += nl) {
      const int r = e / 21, c = e % 21;
      if (r == p || c <= k) continue;
      const double l = w[OE_AUG + r * 21 + k] / piv;
      w[OE_AUG + e] -= l * w[OE_AUG + p * 21 + c];
    }
    sync();
  }
  for (int e = lane; e < 90; e += nl) {
    const int r = e / 6, j = e % 6, row = oe_row_of(perm, r);
    w[OE_K + e] = w[OE_AUG + row * 21 + 15 + j] / w[OE_AUG + row * 21 + r];
  }
  sync();
  // G(:,0:6) = K_1(:,0:6) HTH ; K_1(:,0:6) HTz                                                VS:1056-1058
  for (int e = lane; e < 105; e += nl) {
    const int r = e / 7, k = e % 7;
    double s = 0;
    if (k < 6) { for (int j = 0; j < 6; j++) s += w[OE_K + r * 6 + j] * w[OE_HTH + j * 6 + k]; w[OE_G + r * 6 + k] = s; }
    else { for (int j = 0; j < 6; j++) s += w[OE_K + r * 6 + j] * w[OE_HTZ + j]; w[OE_KH + r] = s; }
  }
  sync();
  // solution = K_1(:,0:6) HTz + vec - G(:,0:6) vec(0:6)                                        VS:1060
  for (int r = lane; r < 15; r += nl) {
    double b = 0;
    for (int j = 0; j < 6; j++) b += w[OE_G + r * 6 + j] * w[OE_VEC + j];
    w[OE_SOL + r] = w[OE_KH + r] + w[OE_VEC + r] - b;
  }
  sync();
}

// One whole iteration `iter` on the sums in w[OE_S34..]: the step, the trace row, the stop rule, on a stop the covariance, and the
// pose and covariance blocks of the next point loop.  The caller has already found S->done clear.
// kd != 0 is the stop rule of lio_state_estimation_kdtree (VS:1216-1233) on the same step: only a converged iteration counts as a
// rematch, the refind that iteration MAX - 2 forces when none has converged does not (VS:1224-1227), and S->refind tells the next
// iteration's neighbour search whether to run.  The stop iteration is the same expression in both modes.  (In kd mode the caller has
// divided cov_inv by 1000, VS:1213, and columns 27-32 of the sums are zero: there is no nnt.)
template <class WP, class Sync>
VBH_HD inline void odom_ekf_iterate(WP w, OdomEkf *S, int iter, int lane, int nl, Sync sync, int kd = 0) {
  VBE_NO_CONTRACT
  odom_ekf_solve(w, S->cov_inv, S->x_prop, S->x_curr, lane, nl, sync);
  if (lane == 0) {
    double sol[15], E[9], Rn[9];
    for (int k = 0; k < 15; k++) sol[k] = w[OE_SOL + k];
    State x = S->x_curr;                                                   // x_curr += solution  TL:154-162
    so3_exp(sol, E);
    m3_mul(x.R, E, Rn);
    for (int k = 0; k < 9; k++) x.R[k] = Rn[k];
    for (int k = 0; k < 3; k++) { x.p[k] += sol[3 + k]; x.v[k] += sol[6 + k]; x.bg[k] += sol[9 + k]; x.ba[k] += sol[12 + k]; }
    S->x_curr = x;
    const double rot_add = norm3(sol), tra_add = norm3(sol + 3);
    S->rot_add[iter] = rot_add; S->tra_add[iter] = tra_add;
    S->match_num[iter] = (int)w[OE_S34 + 33];
    S->nnt[0] = w[OE_S34 + 27]; S->nnt[1] = S->nnt[3] = w[OE_S34 + 28]; S->nnt[2] = S->nnt[6] = w[OE_S34 + 29];
    S->nnt[4] = w[OE_S34 + 30]; S->nnt[5] = S->nnt[7] = w[OE_S34 + 31]; S->nnt[8] = w[OE_S34 + 32];
    S->iterations = iter + 1;
    const bool converged = (rot_add * 57.3 < 0.01) && (tra_add * 100 < 0.015);     // VS:1072
    int rematch = S->rematch_num;
    if (kd) {
      if (converged) { rematch++; S->converged_once = 1; }                         // VS:1218-1223
      S->refind = (converged || (iter == ODOM_EKF_MAX_ITER - 2 && !S->converged_once)) ? 1 : 0;
    } else if (converged || (rematch == 0 && iter == ODOM_EKF_MAX_ITER - 2)) rematch++;   // VS:1076-1079
    S->rematch_num = rematch;
    const bool stop = rematch >= 2 || iter == ODOM_EKF_MAX_ITER - 1;               // VS:1082
    if (stop) S->done = 1;
    w[OE_FLAG] = stop ? 1.0 : 0.0;
    for (int k = 0; k < 9; k++) S->R[k] = x.R[k];
    for (int k = 0; k < 3; k++) S->t[k] = x.p[k];
  }
  sync();
  if (w[OE_FLAG] != 0.0) {                                                 // x_curr.cov = (I - G) cov: G has six columns    VS:1083-1085
    for (int e = lane; e < 225; e += nl) {
      const int r = e / 15, k = e % 15;
      double s = 0;
      for (int j = 0; j < 6; j++) s += w[OE_G + r * 6 + j] * S->P[j * 15 + k];
      S->P_out[e] = S->P[e] - s;
    }
  }
}

// Fills the image of a call: parameter block from (state, cov, cov_inv), x_curr = x_prop, counters zero, P_out = P, the first point
// loop's pose and covariance blocks.
inline void odom_ekf_begin(OdomEkf &S, const double *state25, const double *cov225, const double *cov_inv225) {
  std::memset(&S, 0, sizeof(S));
  std::memcpy(&S.x_prop, state25, sizeof(State));
  S.x_curr = S.x_prop;
  std::memcpy(S.P, cov225, sizeof(S.P));
  std::memcpy(S.P_out, cov225, sizeof(S.P));
  std::memcpy(S.cov_inv, cov_inv225, sizeof(S.cov_inv));
  std::memcpy(S.R, S.x_curr.R, sizeof(S.R));
  std::memcpy(S.t, S.x_curr.p, sizeof(S.t));
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) { S.rot_var[3 * r + k] = cov225[r * 15 + k]; S.tsl_var[3 * r + k] = cov225[(3 + r) * 15 + 3 + k]; }   // VS:999-1000
}

// SelfAdjointEigenSolver(nnt).eigenvalues()[0] (VS:1090-1094) by cyclic Jacobi sweeps on the host
inline double odom_nnt_eig_min(const double *nnt) {
  double a[3][3] = {{nnt[0], nnt[1], nnt[2]}, {nnt[3], nnt[4], nnt[5]}, {nnt[6], nnt[7], nnt[8]}};
  for (int sweep = 0; sweep < 60; sweep++) {
    const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
    if (off == 0.0) break;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        if (a[p][q] == 0.0) continue;
        const double theta = 0.5 * (a[q][q] - a[p][p]) / a[p][q];
        double t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
        if (theta < 0) t = -t;
        const double cth = 1.0 / std::sqrt(1 + t * t), sth = t * cth, apq = a[p][q];
        const int r = 3 - p - q;
        const double arp = a[r][p], arq = a[r][q];
        a[p][p] -= t * apq; a[q][q] += t * apq; a[p][q] = a[q][p] = 0.0;
        a[r][p] = a[p][r] = cth * arp - sth * arq; a[r][q] = a[q][r] = sth * arp + cth * arq;
        if (std::fabs(a[r][p]) < 1e-300) a[r][p] = a[p][r] = 0.0;
        if (std::fabs(a[r][q]) < 1e-300) a[r][q] = a[q][r] = 0.0;
      }
    if (off < 1e-14 * (std::fabs(a[0][0]) + std::fabs(a[1][1]) + std::fabs(a[2][2]))) break;
  }
  return std::min(a[0][0], std::min(a[1][1], a[2][2]));
}

}  // namespace vbh
