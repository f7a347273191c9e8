// The fit of one surfel record (vba_kf_surfel_export, include/voxelba.h): covariance -> ascending eigenvalues, the
// oriented normal and the 12-float record.  The project's symmetric 3x3 solver in its IEEE variant with the Jacobi fallback of the
// descriptor generator's plane fit (vba_btcgen_fit.hpp), so that this header compiled by g++ and by hipcc gives the same bits.  Both
// builds must run with floating-point contraction off (vba_surfel.hip is compiled with -ffp-contract=off;
// tests/host/export_surfel_host.cpp likewise).
#pragma once
#include <cmath>
#include "vba_btcgen_fit.hpp"

namespace vba {

// C = M (1 / cnt): the covariance from the centred moment sums xx xy xz yy yz zz
VBE_HD void sf_cov(const double M[6], int cnt, double C[6]) {
  const double inv = 1.0 / (double)cnt;
  for (int k = 0; k < 6; k++) C[k] = M[k] * inv;
}

// c = the voxel's mean, C = its covariance (xx xy xz yy yz zz), cnt = its records, sensor = x0.p of the keyframe of its first
// record, inten = that record's intensity.  rec: c | inten | normal | sqrt l0, l1, l2 | l0 / trace | cnt; every double is narrowed
// to float once.
VBE_HD void sf_fit(const double c[3], const double C[6], int cnt, const double sensor[3], float inten, float rec[12]) {
  Eig3 o;
  if (!eig3_direct<true>(C[0], C[1], C[2], C[3], C[4], C[5], o)) o = btcg_jacobi(C[0], C[1], C[2], C[3], C[4], C[5]);
  const double l0 = o.w0 < 0.0 ? 0.0 : o.w0, l1 = o.w1 < 0.0 ? 0.0 : o.w1, l2 = o.w2 < 0.0 ? 0.0 : o.w2;   // rounding residue
  double nx = o.v00, ny = o.v10, nz = o.v20;
  const double dot = (nx * (sensor[0] - c[0]) + ny * (sensor[1] - c[1])) + nz * (sensor[2] - c[2]);
  if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }              // toward the sensor
  if (cnt < 3) { nx = 0.0; ny = 0.0; nz = 0.0; }                // one or two records span no surface
  const double tr = (l0 + l1) + l2;
  rec[0] = (float)c[0]; rec[1] = (float)c[1]; rec[2] = (float)c[2]; rec[3] = inten;
  rec[4] = (float)nx; rec[5] = (float)ny; rec[6] = (float)nz;
  rec[7] = (float)sqrt(l0); rec[8] = (float)sqrt(l1); rec[9] = (float)sqrt(l2);
  rec[10] = tr > 0.0 ? (float)(l0 / tr) : 0.0f;
  rec[11] = (float)cnt;
}

}  // namespace vba
