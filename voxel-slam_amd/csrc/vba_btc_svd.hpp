// The Kabsch step of triangle_solver (BTC.cpp:1398-1420): a restatement of Eigen's JacobiSVD for a square 3x3 and V U^T with the
// det < 0 branch.  Host-compilable (tests/test_btc_cpu.py compares it with numpy); the device kernels in vba_kernels_btc.hpp use it.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BTC_HD __host__ __device__ inline
#else
#define BTC_HD inline
#endif
#if defined(__clang__)
#define BTC_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define BTC_NOCONTRACT
#endif

namespace vba {

struct BtcRot { double c, s; };
BTC_HD BtcRot btc_make_jacobi(double x, double y, double z) {   // JacobiRotation::makeJacobi(x, y, z), real
  BTC_NOCONTRACT
  BtcRot j;
  const double deno = 2 * fabs(y);
  if (deno < DBL_MIN) { j.c = 1; j.s = 0; return j; }
  const double tau = (x - z) / deno, w = sqrt(tau * tau + 1);
  const double t = tau > 0 ? 1 / (tau + w) : 1 / (tau - w);
  const double sign_t = t > 0 ? 1 : -1, nn = 1 / sqrt(t * t + 1);
  j.s = -sign_t * (y / fabs(y)) * fabs(t) * nn;
  j.c = nn;
  return j;
}
BTC_HD void btc_svd3(const double *A /*row-major*/, double *U, double *S, double *V) {
  BTC_NOCONTRACT
  double M[9];
  double scale = 0;
  for (int k = 0; k < 9; k++) scale = fabs(A[k]) > scale ? fabs(A[k]) : scale;
  if (scale == 0) scale = 1;
  for (int k = 0; k < 9; k++) { M[k] = A[k] / scale; U[k] = V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
  const double precision = 2 * DBL_EPSILON, zero = DBL_MIN;
  double maxd = fmax(fmax(fabs(M[0]), fabs(M[4])), fabs(M[8]));
  bool finished = false;
  for (int sweep = 0; !finished && sweep < 64; sweep++) {
    finished = true;
    for (int p = 1; p < 3; p++)
      for (int q = 0; q < p; q++) {
        const double thr = fmax(zero, precision * maxd);
        if (!(fabs(M[3 * p + q]) > thr || fabs(M[3 * q + p]) > thr)) continue;
        finished = false;
        // real_2x2_jacobi_svd(M, p, q)
        double m00 = M[3 * p + p], m01 = M[3 * p + q], m10 = M[3 * q + p], m11 = M[3 * q + q];
        BtcRot r1;
        const double t = m00 + m11, d = m10 - m01;
        if (fabs(d) < DBL_MIN) { r1.s = 0; r1.c = 1; }
        else { const double u = t / d, tmp = sqrt(1 + u * u); r1.s = 1 / tmp; r1.c = u / tmp; }
        {   // m.applyOnTheLeft(0, 1, r1)
          const double a0 = m00, a1 = m01, b0 = m10, b1 = m11;
          m00 = r1.c * a0 + r1.s * b0; m01 = r1.c * a1 + r1.s * b1;
          m10 = -r1.s * a0 + r1.c * b0; m11 = -r1.s * a1 + r1.c * b1;
        }
        const BtcRot jr = btc_make_jacobi(m00, m01, m11);
        BtcRot jl;                                                   // r1 * jr^T
        jl.c = r1.c * jr.c - r1.s * (-jr.s);
        jl.s = r1.c * (-jr.s) + r1.s * jr.c;
        for (int k = 0; k < 3; k++) {                                // M.applyOnTheLeft(p, q, jl): rows p, q
          const double x = M[3 * p + k], y = M[3 * q + k];
          M[3 * p + k] = jl.c * x + jl.s * y; M[3 * q + k] = -jl.s * x + jl.c * y;
        }
        for (int k = 0; k < 3; k++) {                                // U.applyOnTheRight(p, q, jl^T): columns p, q
          const double x = U[3 * k + p], y = U[3 * k + q];
          U[3 * k + p] = jl.c * x + jl.s * y; U[3 * k + q] = -jl.s * x + jl.c * y;
        }
        for (int k = 0; k < 3; k++) {                                // M.applyOnTheRight(p, q, jr)
          const double x = M[3 * k + p], y = M[3 * k + q];
          M[3 * k + p] = jr.c * x - jr.s * y; M[3 * k + q] = jr.s * x + jr.c * y;
        }
        for (int k = 0; k < 3; k++) {                                // V.applyOnTheRight(p, q, jr)
          const double x = V[3 * k + p], y = V[3 * k + q];
          V[3 * k + p] = jr.c * x - jr.s * y; V[3 * k + q] = jr.s * x + jr.c * y;
        }
        maxd = fmax(maxd, fmax(fabs(M[3 * p + p]), fabs(M[3 * q + q])));
      }
  }
  for (int i = 0; i < 3; i++) {
    const double a = M[4 * i];
    S[i] = fabs(a) * scale;
    if (a < 0) for (int k = 0; k < 3; k++) U[3 * k + i] = -U[3 * k + i];
  }
  for (int i = 0; i < 3; i++) {                                      // sort descending (first maximum), columns follow
    int pos = i;
    for (int k = i + 1; k < 3; k++) if (S[k] > S[pos]) pos = k;
    if (S[pos] == 0) break;
    if (pos != i) {
      double s = S[i]; S[i] = S[pos]; S[pos] = s;
      for (int k = 0; k < 3; k++) {
        s = U[3 * k + i]; U[3 * k + i] = U[3 * k + pos]; U[3 * k + pos] = s;
        s = V[3 * k + i]; V[3 * k + i] = V[3 * k + pos]; V[3 * k + pos] = s;
      }
    }
  }
}

// R = V U^T; when det R < 0, R = V diag(1, 1, -1) U^T (row-major 3x3)
BTC_HD void btc_kabsch(const double *U, const double *V, double *R) {
  BTC_NOCONTRACT
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = (V[3 * r] * U[3 * c] + V[3 * r + 1] * U[3 * c + 1]) + V[3 * r + 2] * U[3 * c + 2];
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (det < 0)
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R[3 * r + c] = (V[3 * r] * U[3 * c] + V[3 * r + 1] * U[3 * c + 1]) - V[3 * r + 2] * U[3 * c + 2];
}

}  // namespace vba
