// Shape of the dense-tile Hessian pass k_hessian2<W> (vba_kernels_factor.hpp): tile sizes, LDS budget, the table that deals the
// (16x16 output tile, k-split) MFMA units to the four waves, and the fixed tree of its 8-lane sums.  Plain C++17 without the runtime's
// headers, so host code (and tests/host/hess_units_host.cpp under g++) sees exactly what the kernel is compiled from.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define VBA_HESS_HD __host__ __device__
#else
#define VBA_HESS_HD
#endif

namespace vba {

constexpr int hess2_tv(int W) {   // voxels per tile: ~256 / W slot threads = exactly 4 waves, multiple of 8, K-split divisible
  return W == 2 ? 128 : W == 3 ? 80 : W == 4 ? 64 : W == 5 ? 48 : W == 6 ? 40 : (W == 7 || W == 8) ? 32 : (W == 9 || W == 10) ? 24 : 16;
}
constexpr int gcd_i(int a, int b) { return b == 0 ? a : gcd_i(b, a % b); }

// One MFMA unit: the upper-triangle tile u = (ta, tb), ta <= tb, in row-major order of the triangle, and the k-split it contracts.
struct HessUnit { int u, ta, tb, ks; };

template <int W>
struct HessCfg2 {
  static constexpr int TV = hess2_tv(W);
  static constexpr int NT = 256;                         // 4 waves: one per SIMD (5 waves measured 2x slower per tile)
  static constexpr int NC = 6 * W;
  static constexpr int NT16 = (NC + 15) / 16;
  static constexpr int NCP = 16 * NT16;
  // row stride of the LDS images in doubles.  ODD: the slot threads of one frame write rows 3 vl, 3 vl + 1, 3 vl + 2 — with the earlier
  // stride = 16 (mod 32) their stores all fell on two bank groups (12-way conflicts); an odd stride spreads them, and the MFMA operand
  // reads (4 rows x 16 consecutive doubles per wave) stay at 2-3 passes, far from binding
  static constexpr int GS = ((NCP % 32 == 16) ? NCP : NCP + 16) + 1;
  static constexpr int NK = 3 * TV;
  static constexpr int NWV = NT / 64;
  static constexpr int NU = NT16 * (NT16 + 1) / 2;       // upper-triangle 16x16 tiles
  static constexpr int KS = NWV / gcd_i(NU, NWV);        // K-splits so that NU*KS units divide evenly over the waves
  static constexpr int UPW = NU * KS / NWV;              // (tile, k-split) units per wave
  static constexpr int KSTEPS = NK / 4 / KS;             // MFMAs per unit
  static constexpr int NOUT = NC * NC + NC + 1;           // full layout [H | g | r]
  static constexpr int EB = NU * 256;                     // tile layout: offset of the per-frame E blocks
  static constexpr int GB = EB + 21 * W;                  //              offset of the gradient
  static constexpr int RB = GB + 6 * W;                   //              offset of the residual
  static constexpr int NOUT2 = RB + 1;
  static_assert(TV * W <= NT && TV % 8 == 0 && (NK / 4) % KS == 0 && (NU * KS) % NWV == 0, "tile shape");
  // PRESCALE: a second LDS image holds c_k * G, so the MFMA loop carries no f64 VALU multiply (f64 VALU and f64 MFMA share the issue on
  // gfx950: one multiply per MFMA cost 21 of 95 cycles, tools/micro/mfma_lds.hip); every window except W = 3 has the LDS for it
  static constexpr bool PRESCALE = ((size_t)2 * NK * GS + NK + W * 12 + 8) * sizeof(double) <= (size_t)150 * 1024;
  static constexpr size_t LDS_MAIN = (size_t)NK * GS * (PRESCALE ? 2 : 1) + NK + W * 12 + 8;
  // epilogue: [NU][256] staging of the k-splits | [28][SS] the threads' E / gradient / residual terms, one column per thread.  SS is odd:
  // the stores of a wave are 64 consecutive doubles, and the 28 rows a wave reads side by side in the frame sums fall on different banks
  static constexpr int SS = NT + 1;
  static constexpr size_t LDS_EPI = (size_t)(KS > 1 ? NU * 256 : 0) + (size_t)28 * SS + 8;
  static constexpr size_t LDS_BYTES = (LDS_MAIN > LDS_EPI ? LDS_MAIN : LDS_EPI) * sizeof(double);
  static_assert(LDS_BYTES <= (size_t)150 * 1024, "the launch opts in to 150 KB of LDS at most");

  // Unit t of wave `wave`: the NU * KS units are dealt in order, UPW to a wave, k-split major (unit = ks * NU + u).
  static constexpr HessUnit unit(int wave, int t) {
    const int n = wave * UPW + t, u = n % NU;
    int p = u, ta = 0;
    while (p >= NT16 - ta) { p -= NT16 - ta; ta++; }
    return HessUnit{u, ta, ta + p, n / NU};
  }
  // NU is a multiple of UPW, so the units of a wave are consecutive tiles of one k-split
  static constexpr bool wave_units_are_a_run() {
    for (int w = 0; w < NWV; w++)
      for (int t = 0; t < UPW; t++)
        if (unit(w, t).ks != unit(w, 0).ks || unit(w, t).u != unit(w, 0).u + t) return false;
    return true;
  }
};

// Sum of eight consecutive doubles in the association of the pass's 8-lane sums, ((x0+x1)+(x2+x3)) + ((x4+x5)+(x6+x7)): what lane 0
// of an aligned 8-lane group holds after the three data-parallel-primitive steps quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror with an add each (the other lanes hold commuted forms of it, bit-equal).
VBA_HESS_HD inline double group8_tree(const double *x) { return ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7])); }

}  // namespace vba
