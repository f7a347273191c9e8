// The IMU forward propagation of the odometry state and its covariance with the pose table that the undistortion reads
// (IMUEKF::motion_blur, ekf_imu.hpp:54-123, "EK"), and the 15 x 15 inverse of the covariance that the scan-to-map update starts from
// (VS:987), both in the manner of vba_odom_ekf.hpp: every function is written for `nl` cooperating lanes, lane `lane` computes the
// elements e = lane, lane + nl, ... of each stage and calls sync() between stages.  The device kernels (vba_kernels_imu_ekf.hpp) run
// them with the lanes of one workgroup on a work area in the LDS and a barrier as sync(); a host caller passes lane 0 of 1, plain arrays
// and a sync() that does nothing (vba_imu_ekf_propagate, tests/host/imu_ekf_host.cpp).  An element is computed by one lane in one fixed
// order whatever nl is, so the two give the same bits up to sin / cos of the two math libraries when both are compiled without
// floating-point contraction.
//
// F_x (EK:92-99) is the identity plus five 3 x 3 blocks: rows 0-2 hold Exp(w, -dt) at (0,0) and -dt I at (0,9), rows 3-5 dt I at (3,6),
// rows 6-8 -R hat(a) dt at (6,0) and -R dt at (6,12).  F P F^T is formed from these blocks alone, each sum in ascending column order of
// F_x: it is the dense product without its exact zeros.
#pragma once
#include "vba_odom_ekf.hpp"

namespace vbh {

// parameter block of one propagation, in doubles
enum {
  IE_LAST_END = 0,              // last_pcl_end_time
  IE_BEG = 1,                   // pcl_beg_time
  IE_END = 2,                   // pcl_end_time
  IE_SCALE = 3,                 // scale_gravity
  IE_NOISE = 4,                 // cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc (3 each)
  IE_PRM = 16
};
// per-interval row of the work area, in doubles: what does not depend on the recursion, and what the recursion leaves for the
// covariance update
enum {
  IE_IV_EXPF = 0,               // Exp(angvel_avr, dt)
  IE_IV_EXPM = 9,               // Exp(angvel_avr, -dt)
  IE_IV_W = 18,                 // angvel_avr
  IE_IV_A = 21,                 // acc_avr
  IE_IV_DT = 24,
  IE_IV_OFFT = 25,              // cur_time - pcl_beg_time
  IE_IV_LIVE = 26,              // 0.0: the interval lies before last_pcl_end_time (EK:64)
  IE_IV_R = 27,                 // R_imu before the interval's update (the pose row's)
  IE_IV_FA = 36,                // F_x(6,0) = -R hat(acc_avr) dt
  IE_IV_FB = 45,                // F_x(6,12) = -R dt
  IE_IV = 55                    // (odd: no LDS bank pattern)
};
// work area, in doubles: the intervals are taken IE_CHUNK at a time, so its size does not depend on m.  The lanes index it with
// values they compute (a row of a block, a noise entry): nothing of that kind is kept in a lane's own arrays.
static const int IE_CHUNK = 64;
enum {
  IE_P = 0,                     // the covariance, 15 x 15
  IE_T = IE_P + 225,            // F P
  IE_NZ = IE_T + 225,           // cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc
  IE_IVW = IE_NZ + 12,          // IE_CHUNK interval rows
  IE_WORK = IE_IVW + IE_CHUNK * IE_IV
};
static const int IE_ROW = 22;   // pose row: [offt, R(9), p(3), v(3), angvel(3), acc(3)], the row of vba_scan_undistort

// Intervals that EK:64 lets through = rows of the pose table.  Comparisons of time stamps only.
inline int imu_ekf_count(int m, const double *imu, double last_pcl_end_time) {
  int n = 0;
  for (int j = 0; j + 1 < m; j++) if (!(imu[7 * (j + 1)] < last_pcl_end_time)) n++;
  return n;
}
// What a propagation refuses (include/voxelba.h): fewer than two rows, no interval left (EK:120 would read uninitialised values), the
// "LiDAR time regress" exit of EK:45-49, a non-finite input.
inline bool imu_ekf_args_ok(int m, const double *imu, const double *prm) {
  if (m < 2 || !imu || !prm) return false;
  for (int k = 0; k < IE_PRM; k++) if (!std::isfinite(prm[k])) return false;
  for (int k = 0; k < 7 * m; k++) if (!std::isfinite(imu[k])) return false;
  if (prm[IE_LAST_END] - prm[IE_BEG] > 0.01) return false;
  return imu_ekf_count(m, imu, prm[IE_LAST_END]) > 0;
}

// EK:54-123 on the deque rows imu[m][7] = [t, gyr, acc] as they are after push_front(last_imu).  x and P (global or host memory) are
// read and rewritten; poses receives one row per live interval, end_pose (xc.R, xc.p) after it, and the row count is returned.  w is a
// work area of IE_WORK doubles in whatever address space: everything an interval reads more than once lies there.  The caller has
// checked imu_ekf_args_ok.  bg, ba and g are not written.
template <class WP, class Sync>
VBH_HD inline int imu_ekf_propagate(WP w, int m, const double *imu, const double *prm, State *x, double *P, double *poses, double *end_pose,
                                    int lane, int nl, Sync sync) {
  VBE_NO_CONTRACT
  const double last_end = prm[IE_LAST_END], beg = prm[IE_BEG], end = prm[IE_END], sg = prm[IE_SCALE];
  double bg[3], ba[3];
  for (int k = 0; k < 3; k++) { bg[k] = x->bg[k]; ba[k] = x->ba[k]; }
  for (int e = lane; e < 225; e += nl) w[IE_P + e] = P[e];
  for (int e = lane; e < 12; e += nl) w[IE_NZ + e] = prm[IE_NOISE + e];
  // the recursion's state, kept by lane 0 from one chunk to the next
  double R[9], p[3], v[3], g[3], acc[3] = {0, 0, 0}, wl[3] = {0, 0, 0};
  if (lane == 0) {
    for (int k = 0; k < 9; k++) R[k] = x->R[k];
    for (int k = 0; k < 3; k++) { p[k] = x->p[k]; v[k] = x->v[k]; g[k] = x->g[k]; }
  }
  int rows = 0;
  for (int j0 = 0; j0 < m - 1; j0 += IE_CHUNK) {
    const int jn = (m - 1 - j0 < IE_CHUNK) ? m - 1 - j0 : IE_CHUNK;
    // what an interval needs of the IMU rows alone: averages, dt, the two exponentials                       EK:64-90, EK:95
    for (int jj = lane; jj < jn; jj += nl) {
      const double *head = imu + 7 * (size_t)(j0 + jj), *tail = head + 7;
      const int q = IE_IVW + IE_IV * jj;
      double wv[3], av[3], Ef[9], Em[9];
      for (int k = 0; k < 3; k++) {
        wv[k] = 0.5 * (head[1 + k] + tail[1 + k]) - bg[k];
        av[k] = 0.5 * (head[4 + k] + tail[4 + k]) * sg - ba[k];
      }
      double cur = head[0];
      if (cur < last_end) cur = last_end;                                                                    // EK:81-84
      const double dt = tail[0] - cur;
      so3_exp_dt(wv, dt, Ef);
      so3_exp_dt(wv, -dt, Em);
      for (int k = 0; k < 9; k++) { w[q + IE_IV_EXPF + k] = Ef[k]; w[q + IE_IV_EXPM + k] = Em[k]; }
      for (int k = 0; k < 3; k++) { w[q + IE_IV_W + k] = wv[k]; w[q + IE_IV_A + k] = av[k]; }
      w[q + IE_IV_DT] = dt; w[q + IE_IV_OFFT] = cur - beg;
      w[q + IE_IV_LIVE] = (tail[0] < last_end) ? 0.0 : 1.0;
    }
    sync();
    // the state recursion, which does not read P: pose rows (EK:87), then position, velocity, rotation in that order (EK:108-110)
    if (lane == 0) {
      int r = rows;
      for (int jj = 0; jj < jn; jj++) {
        const int q = IE_IVW + IE_IV * jj;
        if (w[q + IE_IV_LIVE] == 0.0) continue;
        const double dt = w[q + IE_IV_DT];
        double av[3], Ef[9], Rn[9];
        for (int k = 0; k < 3; k++) { wl[k] = w[q + IE_IV_W + k]; av[k] = w[q + IE_IV_A + k]; }
        for (int k = 0; k < 9; k++) Ef[k] = w[q + IE_IV_EXPF + k];
        m3_vec(R, av, acc);
        for (int k = 0; k < 3; k++) acc[k] += g[k];
        double *row = poses + (size_t)IE_ROW * r++;
        row[0] = w[q + IE_IV_OFFT];
        for (int k = 0; k < 9; k++) row[1 + k] = w[q + IE_IV_R + k] = R[k];
        for (int k = 0; k < 3; k++) { row[10 + k] = p[k]; row[13 + k] = v[k]; row[16 + k] = wl[k]; row[19 + k] = acc[k]; }
        // F_x(6,0) = -R hat(a) dt and F_x(6,12) = -R dt (EK:98-99), for the covariance update below
        double H[9];
        hat(av, H);
        for (int i = 0; i < 3; i++)
          for (int c = 0; c < 3; c++) {
            w[q + IE_IV_FA + 3 * i + c] = ((-R[3 * i]) * H[c] + (-R[3 * i + 1]) * H[3 + c] + (-R[3 * i + 2]) * H[6 + c]) * dt;
            w[q + IE_IV_FB + 3 * i + c] = (-R[3 * i + c]) * dt;
          }
        for (int k = 0; k < 3; k++) p[k] = p[k] + v[k] * dt + 0.5 * acc[k] * dt * dt;
        for (int k = 0; k < 3; k++) v[k] = v[k] + acc[k] * dt;
        m3_mul(R, Ef, Rn);
        for (int k = 0; k < 9; k++) R[k] = Rn[k];
      }
    }
    sync();
    // P <- F P F^T + cov_w (EK:92-105), interval by interval: T = F P, then P = T F^T + cov_w
    for (int jj = 0; jj < jn; jj++) {
      const int q = IE_IVW + IE_IV * jj;
      if (w[q + IE_IV_LIVE] == 0.0) continue;
      rows++;
      const double dt = w[q + IE_IV_DT];
      const int Em = q + IE_IV_EXPM, Rj = q + IE_IV_R;
      for (int e = lane; e < 225; e += nl) {
        const int i = e / 15, c = e % 15;
        double s;
        if (i < 3) s = w[Em + 3 * i] * w[IE_P + c] + w[Em + 3 * i + 1] * w[IE_P + 15 + c] + w[Em + 3 * i + 2] * w[IE_P + 30 + c] + (-dt) * w[IE_P + (9 + i) * 15 + c];
        else if (i < 6) s = w[IE_P + e] + dt * w[IE_P + (i + 3) * 15 + c];
        else if (i < 9) {
          const int Ai = q + IE_IV_FA + 3 * (i - 6), Bi = q + IE_IV_FB + 3 * (i - 6);
          s = w[Ai] * w[IE_P + c] + w[Ai + 1] * w[IE_P + 15 + c] + w[Ai + 2] * w[IE_P + 30 + c] + w[IE_P + e];
          s = s + w[Bi] * w[IE_P + 12 * 15 + c] + w[Bi + 1] * w[IE_P + 13 * 15 + c] + w[Bi + 2] * w[IE_P + 14 * 15 + c];
        } else s = w[IE_P + e];
        w[IE_T + e] = s;
      }
      sync();
      for (int e = lane; e < 225; e += nl) {
        const int i = e / 15, c = e % 15;
        const int t = IE_T + 15 * i;
        double s;
        if (c < 3) s = w[t] * w[Em + 3 * c] + w[t + 1] * w[Em + 3 * c + 1] + w[t + 2] * w[Em + 3 * c + 2] + w[t + 9 + c] * (-dt);
        else if (c < 6) s = w[t + c] + w[t + c + 3] * dt;
        else if (c < 9) {
          const int Ac = q + IE_IV_FA + 3 * (c - 6), Bc = q + IE_IV_FB + 3 * (c - 6);
          s = w[t] * w[Ac] + w[t + 1] * w[Ac + 1] + w[t + 2] * w[Ac + 2] + w[t + c];
          s = s + w[t + 12] * w[Bc] + w[t + 13] * w[Bc + 1] + w[t + 14] * w[Bc + 2];
        } else s = w[t + c];
        // cov_w, EK:100-103
        if (i < 3 && c == i) s += w[IE_NZ + i] * dt * dt;
        else if (i >= 6 && i < 9 && c >= 6 && c < 9) {
          const int ra = Rj + 3 * (i - 6), rb = Rj + 3 * (c - 6);
          s += (w[ra] * w[IE_NZ + 3] * w[rb] + w[ra + 1] * w[IE_NZ + 4] * w[rb + 1] + w[ra + 2] * w[IE_NZ + 5] * w[rb + 2]) * dt * dt;
        } else if (i >= 9 && c == i) s += w[IE_NZ + 6 + (i - 9)] * dt * dt;
        w[IE_P + e] = s;
      }
      sync();
    }
    sync();                     // the next chunk writes over the interval rows
  }
  // the tail extrapolation (EK:117-123)
  if (lane == 0) {
    const double imu_end = imu[7 * (size_t)(m - 1)];
    const double note = end > imu_end ? 1.0 : -1.0;
    const double dt = note * (end - imu_end);
    double wn[3], E[9], Rn[9];
    for (int k = 0; k < 3; k++) wn[k] = note * wl[k];
    so3_exp_dt(wn, dt, E);
    m3_mul(R, E, Rn);
    x->t = end;
    for (int k = 0; k < 9; k++) x->R[k] = end_pose[k] = Rn[k];
    for (int k = 0; k < 3; k++) {
      x->v[k] = v[k] + note * acc[k] * dt;
      x->p[k] = end_pose[9 + k] = p[k] + note * v[k] * dt + note * 0.5 * acc[k] * dt * dt;
    }
  }
  for (int e = lane; e < 225; e += nl) P[e] = w[IE_P + e];
  return rows;
}

// vbh::inverse_pplu for n = 15 by nl lanes: the same pivots (the first row of the largest magnitude among the rows not yet taken, in
// the order the exchanges have left them), the same operations in the same order for every element, so the same bits without
// contraction.  Rows are not moved: every lane keeps the table "logical row -> row of lu" in four bits per entry of a 64-bit word,
// which is inverse_pplu's perm.  w is a work area of INV15_WORK doubles: the LU factors, and per column of the inverse its y and its
// solution, which the lane that owns the column reads back as it goes.  Ainv is written at the end.
static const int INV15_WORK = 3 * 225;
template <class WP, class Sync>
VBH_HD inline void inverse15_pplu(WP w, const double *A, double *Ainv, int lane, int nl, Sync sync) {
  VBE_NO_CONTRACT
  const int n = 15, Y = 225, X = 450;
  for (int e = lane; e < 225; e += nl) w[e] = A[e];
  sync();
  unsigned long long perm = 0;
  for (int i = 0; i < n; i++) perm |= (unsigned long long)i << (4 * i);
  for (int k = 0; k < n; k++) {
    int piv = k;
    double big = std::fabs(w[oe_row_of(perm, k) * n + k]);
    for (int i = k + 1; i < n; i++) {
      const double a = std::fabs(w[oe_row_of(perm, i) * n + k]);
      if (a > big) { big = a; piv = i; }
    }
    if (piv != k) {
      const unsigned long long rk = (perm >> (4 * k)) & 15ull, rp = (perm >> (4 * piv)) & 15ull;
      perm &= ~((15ull << (4 * k)) | (15ull << (4 * piv)));
      perm |= (rp << (4 * k)) | (rk << (4 * piv));
    }
    const int pk = oe_row_of(perm, k), rem = n - 1 - k;
    const double d = w[pk * n + k];
    for (int e = lane; e < rem * rem; e += nl) {
      const int pi = oe_row_of(perm, k + 1 + e / rem), j = k + 1 + e % rem;
      const double l = w[pi * n + k] / d;
      w[pi * n + j] -= l * w[pk * n + j];
    }
    sync();
    // the multipliers: column k is read again only by the solves
    for (int i = k + 1 + lane; i < n; i += nl) { const int pi = oe_row_of(perm, i); w[pi * n + k] = w[pi * n + k] / d; }
  }
  sync();
  for (int c = lane; c < n; c += nl) {
    for (int i = 0; i < n; i++) {
      const int pi = oe_row_of(perm, i);
      double s = (pi == c) ? 1.0 : 0.0;
      for (int j = 0; j < i; j++) s -= w[pi * n + j] * w[Y + c * n + j];
      w[Y + c * n + i] = s;
    }
    for (int i = n - 1; i >= 0; i--) {
      const int pi = oe_row_of(perm, i);
      double s = w[Y + c * n + i];
      for (int j = i + 1; j < n; j++) s -= w[pi * n + j] * w[X + c * n + j];
      w[X + c * n + i] = s / w[pi * n + i];
    }
    for (int i = 0; i < n; i++) Ainv[i * n + c] = w[X + c * n + i];
  }
  sync();
}

}  // namespace vbh
