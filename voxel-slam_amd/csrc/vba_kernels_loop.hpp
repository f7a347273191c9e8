// Loop-closure map rebuild (vba_loop_map_*, vba_loop_update): fixed-point insertion of an EXPANDED sequence of
// clouds that are already in HBM (the keyframe store, the buf_lba2loop scans), with their covariances.
//
// The reference inserts  kf0 | kf0 kf1 | kf0 kf1 kf2 | ...  (VS:2601-2625) and then one scan after the other (VS:1338-1347), every
// call at jour = 0.  Fixed-point cut_voxel (VM:2108-2152) is a per-point loop whose only per-call state is jour, so each of the two
// sequences is ONE insertion of the concatenation.  A small segment table describes the concatenation; no expanded copy of the
// source is made: k_loop_gather forms the world points, the shared insert kernels find root and leaf and sort by leaf, and
// k_fix_accum_ord<COV> fetches each point's covariance from the SOURCE row when it writes the point's pool entry.  (The pool keeps
// a leaf's points as one contiguous block in arrival order, so an entry's position is only known after the sort: the covariance
// cannot be put in place by the gather.  Fetching it at that moment moves it once, source -> pool row.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vba_common.hpp"
#include "vba_kernels_map.hpp"

namespace vba {

// One thread per OUTPUT point, lanes on consecutive points.  seg[j] = (first output index, first source row, pose index, -) for
// j < nseg, ascending in the first field; a thread finds its segment as k_kf_merge does.  pw = R p + t in k_kf_world's order
// ((a x + b y) + c z) + t, no contraction.  Writes the world point to `world` [n][3] (what k_fix_accum_ord reads, input order), to
// the pool tail fx[base + i] (what the root and leaf searches read) with fnode = -1, and the source row to srcrow[i].
__global__ __launch_bounds__(256) void k_loop_gather(MapView m, int base, int n, int nseg, const int4 *__restrict__ seg, const double *__restrict__ poses,
                                                     const double *__restrict__ src, double *__restrict__ world, int *__restrict__ srcrow) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = nseg - 1;                                // last j with seg[j].x <= i (empty segments are skipped by the <=)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid].x <= i) lo = mid; else hi = mid - 1;
  }
  const int4 sg = seg[lo];
  const int row = sg.y + (i - sg.x);
  const size_t b = 3 * (size_t)row, o = 3 * (size_t)i, q = 3 * ((size_t)base + (size_t)i);
  double x, y, z;
  kf_apply(poses + 12 * sg.z, src[b], src[b + 1], src[b + 2], x, y, z);
  world[o] = x; world[o + 1] = y; world[o + 2] = z;
  m.fx[q] = x; m.fx[q + 1] = y; m.fx[q + 2] = z;
  m.fnode[base + i] = -1;
  srcrow[i] = row;
}

}  // namespace vba
