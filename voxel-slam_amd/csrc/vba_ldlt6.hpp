// Fixed-size twin of vbh::ldlt_solve_inplace (vba_hostmath.hpp) for the 6x6 point-to-plane system of icp_normal
// (loop_refine.hpp:115, Eigen `Hess.ldlt().solve(-JacT)`).  The host function keeps its std::vector scratch and stays as it is;
// this copy runs the same operations in the same order on plain arrays, so it compiles for the device and, on the host, returns
// the same bits (tests/test_btc_cpu.py compiles both with g++ and compares them).
#pragma once
#include <cmath>
#include <cfloat>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBL6_HD __host__ __device__ __forceinline__
#else
#define VBL6_HD inline
#endif
#if defined(__clang__)
#define VBL6_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define VBL6_NOCONTRACT
#endif

namespace vbh {

template <int N>
VBL6_HD void ldlt_solve_fixed(double *A /*[N][N], destroyed*/, const double *b, double *x) {
  VBL6_NOCONTRACT   // (the host build contracts nothing: baseline x86-64 has no FMA)
  int tr[N];
  double tmp[N];
#define AT(r, c) A[(r) * N + (c)]
  for (int k = 0; k < N; k++) {
    int piv = k;
    double big = fabs(AT(k, k));
    for (int i = k + 1; i < N; i++)
      if (fabs(AT(i, i)) > big) { big = fabs(AT(i, i)); piv = i; }
    tr[k] = piv;
    if (piv != k) {
      double s;
      for (int j = 0; j < k; j++) { s = AT(k, j); AT(k, j) = AT(piv, j); AT(piv, j) = s; }
      for (int i = piv + 1; i < N; i++) { s = AT(i, k); AT(i, k) = AT(i, piv); AT(i, piv) = s; }
      s = AT(k, k); AT(k, k) = AT(piv, piv); AT(piv, piv) = s;
      for (int i = k + 1; i < piv; i++) { s = AT(i, k); AT(i, k) = AT(piv, i); AT(piv, i) = s; }
    }
    if (k > 0) {
      for (int j = 0; j < k; j++) tmp[j] = AT(j, j) * AT(k, j);
      double s = 0;
      for (int j = 0; j < k; j++) s += AT(k, j) * tmp[j];
      AT(k, k) -= s;
      for (int i = k + 1; i < N; i++) {
        double t = 0;
        for (int j = 0; j < k; j++) t += AT(i, j) * tmp[j];
        AT(i, k) -= t;
      }
    }
    const double akk = AT(k, k);
    const bool valid = fabs(akk) > 0.0;
    if (k == 0 && !valid) { for (int j = 0; j < N; j++) tr[j] = j; break; }
    if (valid) for (int i = k + 1; i < N; i++) AT(i, k) /= akk;
  }
  for (int i = 0; i < N; i++) x[i] = b[i];
  for (int k = 0; k < N; k++) if (tr[k] != k) { const double s = x[k]; x[k] = x[tr[k]]; x[tr[k]] = s; }
  for (int i = 0; i < N; i++) { double s = x[i]; for (int j = 0; j < i; j++) s -= AT(i, j) * x[j]; x[i] = s; }
  for (int i = 0; i < N; i++) { const double d = AT(i, i); x[i] = (fabs(d) > DBL_MIN) ? x[i] / d : 0.0; }
  for (int i = N - 1; i >= 0; i--) { double s = x[i]; for (int j = i + 1; j < N; j++) s -= AT(j, i) * x[j]; x[i] = s; }
  for (int k = N - 1; k >= 0; k--) if (tr[k] != k) { const double s = x[k]; x[k] = x[tr[k]]; x[tr[k]] = s; }
#undef AT
}

}  // namespace vbh
