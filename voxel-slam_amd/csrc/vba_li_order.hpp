// Elimination order and structure mask of the LI_BA solve (k_li_solve, vba_kernels_li.hpp).  Host-compilable: the CPU tests
// (tests/test_solve_cpu.py) check the mask against the symbolic fill of the permuted system.
//
// Order = the STRUCTURE of the system ("eliminate the 9W velocity / bias block first"): the v, bg, ba of frame 0, 1,
// ... W-1 (block-tridiagonal through the IMU factors, VM:551-567), then the 6W pose scalars (dense through the lidar part), then
// gravity.  Column c of frame i's block then reaches only the rest of its block, frame i+1's block, the poses of frames 0..i+1
// (i-1, i, i+1 directly, the older ones as fill of the chain), gravity and the right-hand side: the trailing update of most tiles
// is skipped (li_live).  This departs from Eigen's LDLT, which pivots by the largest remaining diagonal (VM:659): the damped
// system is symmetric positive definite, for which every order is backward stable, so the results move in the last digits only.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LIO_HD __host__ __device__ inline
#else
#define LIO_HD inline
#endif

namespace vba {

// state index (15 per frame: pose 0..5, v 6..8, bg 9..11, ba 12..14; gravity 15W..15W+2) eliminated at position k
LIO_HD int li_ord(int k, int W) {
  if (k < 9 * W) { const int i = k / 9; return 15 * i + 6 + (k - 9 * i); }
  if (k < 15 * W) { const int q = k - 9 * W, i = q / 6; return 15 * i + (q - 6 * i); }
  return k;
}

// bit b set: rows [16 b, 16 b + 16) of the permuted (n+1)-row system (row n = the right-hand side, NP = padded size) can hold a
// non-zero of L in the columns [8 kb, 8 kb + 8).  A superset of the structure is fine; ldlt_mfma skips the rank-8 update of every
// tile whose row block or column block is dead for the panel.
LIO_HD unsigned li_live(int kb, int W, int n, int NP) {
  const int c0 = 8 * kb, c1 = c0 + 7;
  auto span = [](int a, int b) -> unsigned { return (a < b) ? ((2u << ((b - 1) >> 4)) - 1u) & ~((1u << (a >> 4)) - 1u) : 0u; };   // rows [a, b)
  if (c0 >= 9 * W) return span(c0, NP);
  const int ihi = (c1 < 9 * W ? c1 : 9 * W - 1) / 9;                                   // last frame the panel touches
  unsigned m = span(c0, (9 * (ihi + 2) < 9 * W) ? 9 * (ihi + 2) : 9 * W);            // its own blocks and the next frame's
  m |= span(9 * W, (6 * (ihi + 2) < 6 * W) ? 9 * W + 6 * (ihi + 2) : 15 * W);        // poses of frames 0 .. ihi + 1
  m |= span(15 * W, n + 1);                                                            // gravity, right-hand side row
  if (c1 >= 9 * W) m |= span(9 * W, NP);                                               // a panel that straddles into the pose block
  return m;
}

// compact IMU Hessian layout: [pair (a, b), |a - b| <= 1][15][15] | (R, g col k) [15W][3] | (g row k, C) [3][15W] | corner [3][3]
LIO_HD int li_hb_pair(int a, int b) { return (3 * a + (b - a)) * 225; }
LIO_HD int li_hb_ne1(int W) { return (3 * W - 2) * 225; }
LIO_HD int li_hb_size(int W, int grav) { return li_hb_ne1(W) + (grav ? 90 * W + 9 : 0); }
LIO_HD double li_hb_get(const double *hb, int W, int n, int R, int C) {   // dense (R, C) from the compact image
  const int nw = 15 * W;
  if (R < nw && C < nw) { const int a = R / 15, b = C / 15; if (a - b > 1 || b - a > 1) return 0.0; return hb[li_hb_pair(a, b) + (R - 15 * a) * 15 + (C - 15 * b)]; }
  const int ne1 = li_hb_ne1(W);
  if (R < nw) return hb[ne1 + R * 3 + (C - nw)];
  if (C < nw) return hb[ne1 + 45 * W + (R - nw) * nw + C];
  return hb[ne1 + 90 * W + (R - nw) * 3 + (C - nw)];
}

}  // namespace vba

#undef LIO_HD
