// Plane fit of BTC descriptor generation (BTCOctoTree::init_plane, BTC.cpp:96-138, and the merged planes of get_project_plane /
// merge_plane, BTC.cpp:327-350 / :436-459): the project's symmetric 3x3 solver (vba_eig3.hpp, direct path, with cyclic Jacobi
// sweeps as the fallback the other plane fits use) in its IEEE variant, so that this header compiled by g++ and by hipcc gives
// the same bits.  Both builds must run with floating-point contraction off (vba_btcgen.hip is compiled with -ffp-contract=off;
// tests/host/btcgen_host.cpp likewise).
//
// Deviation from the reference: Eigen::EigenSolver's eigenvector sign cannot be reproduced without Eigen.  The normal's sign is
// fixed instead: its component of largest magnitude is positive (the lowest index wins a tie).  DESIGN.md §11.
#pragma once
#include <cmath>
#include "vba_eig3.hpp"

namespace vba {

// one Jacobi rotation in the (p, q) plane, correctly rounded primitives only (the algorithm of jacobi_rot, vba_kernels_factor.hpp)
VBE_HD void btcg_jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
                            double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq);
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { apq = 0.0; return; }
  const double a = 0.5 * (aqq - app);
  int ex;
  (void)frexp(fmax(fabs(a), fabs(apq)), &ex);
  const float af = (float)ldexp(a, -ex), bf = (float)ldexp(apq, -ex);
  const float tf = bf / (fabsf(af) + sqrtf(af * af + bf * bf));
  const double t = (af < 0.0f) ? -(double)tf : (double)tf;
  const double c = 1.0 / sqrt(1.0 + t * t);
  const double s = t * c;
  const double cc = c * c, ss = s * s, cs = c * s;
  const double npp = cc * app - 2.0 * cs * apq + ss * aqq;
  const double nqq = ss * app + 2.0 * cs * apq + cc * aqq;
  const double npq = cs * (app - aqq) + (cc - ss) * apq;
  app = npp; aqq = nqq; apq = npq;
  double x1 = arp, y1 = arq;
  arp = c * x1 - s * y1; arq = s * x1 + c * y1;
  x1 = v0p; y1 = v0q; v0p = c * x1 - s * y1; v0q = s * x1 + c * y1;
  x1 = v1p; y1 = v1q; v1p = c * x1 - s * y1; v1q = s * x1 + c * y1;
  x1 = v2p; y1 = v2q; v2p = c * x1 - s * y1; v2q = s * x1 + c * y1;
}

// cyclic Jacobi sweeps (eig3_jacobi_dev's algorithm): ascending eigenvalues, eigenvectors in the columns
VBE_HD Eig3 btcg_jacobi(double a00, double a01, double a02, double a11, double a12, double a22) {
  int e = 0;
  {
    const double s = fmax(fmax(fmax(fabs(a00), fabs(a11)), fabs(a22)), fmax(fmax(fabs(a01), fabs(a02)), fabs(a12)));
    if (s > 0.0 && s <= 1.7976931348623157e308) (void)frexp(s, &e);
  }
  a00 = ldexp(a00, -e); a01 = ldexp(a01, -e); a02 = ldexp(a02, -e); a11 = ldexp(a11, -e); a12 = ldexp(a12, -e); a22 = ldexp(a22, -e);
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
  for (int sweep = 0; sweep < 30; sweep++) {
    if (fabs(a01) + fabs(a02) + fabs(a12) == 0.0) break;
    btcg_jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    btcg_jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    btcg_jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  double t;
  if (a11 < a00) { t = a00; a00 = a11; a11 = t; t = v00; v00 = v01; v01 = t; t = v10; v10 = v11; v11 = t; t = v20; v20 = v21; v21 = t; }
  if (a22 < a00) { t = a00; a00 = a22; a22 = t; t = v00; v00 = v02; v02 = t; t = v10; v10 = v12; v12 = t; t = v20; v20 = v22; v22 = t; }
  if (a22 < a11) { t = a11; a11 = a22; a22 = t; t = v01; v01 = v02; v02 = t; t = v11; v11 = v12; v12 = t; t = v21; v21 = v22; v22 = t; }
  Eig3 o;
  o.w0 = ldexp(a00, e); o.w1 = ldexp(a11, e); o.w2 = ldexp(a22, e);
  o.v00 = v00; o.v01 = v01; o.v02 = v02; o.v10 = v10; o.v11 = v11; o.v12 = v12; o.v20 = v20; o.v21 = v21; o.v22 = v22;
  return o;
}

// covariance (lower triangle a00 a10 a20 a11 a21 a22) -> smallest eigenvalue, its unit eigenvector with the sign rule; returns
// whether the direct path solved it (0: the Jacobi fallback did)
VBE_HD int btcg_plane_eig(double a00, double a01, double a02, double a11, double a12, double a22, double &wmin, double n[3]) {
  Eig3 o;
  int direct = 1;
  if (!eig3_direct<true>(a00, a01, a02, a11, a12, a22, o)) { o = btcg_jacobi(a00, a01, a02, a11, a12, a22); direct = 0; }
  wmin = o.w0;
  double x = o.v00, y = o.v10, z = o.v20;
  int k = 0;
  double m = fabs(x);
  if (fabs(y) > m) { k = 1; m = fabs(y); }
  if (fabs(z) > m) { k = 2; }
  const double lead = k == 0 ? x : (k == 1 ? y : z);
  if (lead < 0.0) { x = -x; y = -y; z = -z; }
  n[0] = x; n[1] = y; n[2] = z;
  return direct;
}

}  // namespace vba
