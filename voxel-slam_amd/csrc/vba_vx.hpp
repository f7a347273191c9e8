// What the voxel passes over the global map share (vba_kf_voxel_export; vba_kf_surfel_export, §25): the per-keyframe
// table, the table slot, and the record of the sequence S recomputed from the store.  Device helpers only, no kernel: the k_vx_*
// kernels are vba_kernels_kf.hpp (compiled by vba_kf.hip), the k_sf_* kernels vba_kernels_surfel.hpp (compiled by vba_surfel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "vba_common.hpp"

namespace vba {

// One table row per NON-EMPTY keyframe of all stores in publication order: the records of S before it, the address of its point 0,
// its current x0, its store's intensity.  Record i of keyframe k is the point  pnt + 3 (i - first) jump.
struct VxKf { long long first; const double *pnt; double T[12]; float inten; int pad; };     // 120 bytes
// The table has >= 2 |S| slots, so the slot is lean: the sums live in an array of their own ([slots][3] doubles, indexed as the table).
struct alignas(16) VxSlot { unsigned long long key; int cnt, first; };                    // key DS_EMPTY when free
// A count or emit workgroup owns `per` consecutive records (a multiple of 256) and walks them tile by tile; at most kVxBlocks
// workgroups, so that the exclusive scan of their counts is k_ds_scan at the size it was written for.
static constexpr int kVxBlocks = 2048;

// last j in [lo, hi] with tab[j].first <= i
__device__ __forceinline__ int vx_kf_of(long long i, int lo, int hi, const VxKf *__restrict__ tab) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// record i of S, a record of keyframe *e: x0.R p + x0.p in kf_apply's order, each coordinate narrowed to float once
__device__ __forceinline__ void vx_world(const VxKf *__restrict__ e, long long i, int jump, float &x, float &y, float &z) {
  const double *__restrict__ p = e->pnt + 3 * (size_t)((i - e->first) * (long long)jump);
  double qx, qy, qz;
  kf_apply(e->T, p[0], p[1], p[2], qx, qy, qz);
  x = (float)qx; y = (float)qy; z = (float)qz;
}

}  // namespace vba
