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

// bytes of the map's staging buffer one insertion of n points needs: world points, source rows and the seven per-point temporaries
// of the insert kernels.  The temporaries live here, not in the map's [max_pts] arrays: those are sized for ONE scan and come in
// [W] rows, and an expanded keyframe sequence is 10-40 scans long.
inline size_t fix_source_stage_bytes(size_t n) { return ((n * 24 + 255) & ~(size_t)255) + 8 * ((n * 4 + 255) & ~(size_t)255); }

inline int map_sort_reserve_n(MapStore &s, hipStream_t st, size_t n, std::string &err) {
  size_t need = 0;
  MAPCHK(sort_pairs_u32(nullptr, need, nullptr, nullptr, nullptr, nullptr, n, 32u, st));
  if (need + 256 > s.sort_tmp_bytes) {
    MAPCHK(hipStreamSynchronize(st));
    if (s.d_sort_tmp) hipFree(s.d_sort_tmp);
    s.d_sort_tmp = nullptr; s.sort_tmp_bytes = 0;
    MAPCHK(hipMalloc(&s.d_sort_tmp, need + 256));
    s.sort_tmp_bytes = need + 256;
  }
  return VBA_OK;
}

// room for an insertion of n fixed points on top of what the map holds (counters current): nodes, pool, root table, staging, sort
int map_fix_source_ensure(MapStore &s, hipStream_t st, size_t nodes, size_t fix, size_t n, std::string &err) {
  int r = map_ensure(s, st, nodes, 0, fix, err);
  if (r) return r;
  if (2 * ((size_t)s.ub_used + n) > (size_t)s.hcap) {       // as map_ensure keeps the table under ~50 % load, for n possible new roots
    unsigned int nc = s.hcap;
    while ((size_t)nc < 2 * ((size_t)s.ub_roots + n) && nc < (1u << 30)) nc *= 2;
    r = map_hash_alloc(s, nc, st, err);
    if (r) return r;
  }
  if (fix_source_stage_bytes(n) > s.stage_bytes) MAPCHK(hipStreamSynchronize(st));
  r = map_stage(s, fix_source_stage_bytes(n), err);
  if (r) return r;
  return map_sort_reserve_n(s, st, n, err);
}

// map_cut_voxel_fix for a FixSource: n = points of the expanded sequence.  Same kernels after the staging, same single counter
// read-back at the end; k_fix_to_soa does not run (k_loop_gather writes the pool tail itself).
int map_cut_voxel_fix_source(MapStore &s, hipStream_t st, int n, const FixSource &src, double jour, std::string &err) {
  if (n < 0 || (n > 0 && (!src.d_pnt || !src.d_seg || !src.d_poses || src.nseg < 1)) || src.cov_kind == FIXCOV_KEEP || (src.cov_kind != FIXCOV_ZERO && !src.d_cov)) return VBA_ERR_BAD_ARG;
  if (n == 0) return VBA_OK;
  int r = map_base(s, st, err);
  if (r) return r;
  if (s.cnt_stale) { r = map_read_counters(s, st, err); if (r) return r; }
  if ((size_t)s.h_cnt[CNT_FIX] + (size_t)n > (size_t)INT32_MAX / 16) { err = "fixed-point pool: too many points"; return VBA_ERR_CAPACITY; }
  r = map_fix_source_ensure(s, st, (size_t)s.h_cnt[CNT_NODES] + (size_t)n + 64, (size_t)s.h_cnt[CNT_FIX] + (size_t)n, (size_t)n, err);
  if (r) return r;
  const size_t bi = ((size_t)n * 4 + 255) & ~(size_t)255;
  char *stg = (char *)s.d_stage;
  double *world = (double *)stg; stg += ((size_t)n * 24 + 255) & ~(size_t)255;
  int *srcrow = (int *)stg; stg += bi;
  // the insert kernels take their per-point temporaries from the view: for this call they point into the staging buffer
  struct Tmp {
    MapView &v; MapView keep;
    explicit Tmp(MapView &vv) : v(vv), keep(vv) {}
    ~Tmp() { v.phash = keep.phash; v.newslots = keep.newslots; v.skey_a = keep.skey_a; v.skey_b = keep.skey_b; v.sval_a = keep.sval_a; v.sval_b = keep.sval_b; v.wl = keep.wl; }
  } tmp(s.v);
  s.v.phash = (int *)stg; s.v.newslots = (int *)(stg + bi); s.v.skey_a = (unsigned int *)(stg + 2 * bi); s.v.skey_b = (unsigned int *)(stg + 3 * bi);
  s.v.sval_a = (int *)(stg + 4 * bi); s.v.sval_b = (int *)(stg + 5 * bi); s.v.wl = (int *)(stg + 6 * bi);
  const MapParams P = map_params(s);
  const int base = s.h_cnt[CNT_FIX];
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_loop_gather, dim3(nb), dim3(256), 0, st, s.v, base, n, src.nseg, src.d_seg, src.d_poses, src.d_pnt, world, srcrow);
  r = map_set_counter(s, st, CNT_NEWSLOTS, 0, err); if (r) return r;
  r = map_set_counter(s, st, CNT_FIX, base + n, err); if (r) return r;
  map_ins_roots(s, st, P, base, n, 1, jour, 0);
  r = map_set_counter(s, st, CNT_WL, 0, err); if (r) return r;
  hipLaunchKernelGGL(k_fix_leaf, dim3(nb), dim3(256), 0, st, s.v, P, base, n);
  {
    size_t tb = s.sort_tmp_bytes;
    MAPCHK(sort_pairs_u32(s.d_sort_tmp, tb, s.v.skey_a, s.v.skey_b, s.v.sval_a, s.v.sval_b, (size_t)n, map_key_bits(s), st));
  }
  hipLaunchKernelGGL(k_fix_heads, dim3(nb), dim3(256), 0, st, s.v, n);
  const dim3 ga(n < 4096 ? n : 4096), ba(64);
  if (src.cov_kind == FIXCOV_DIAG_F32) hipLaunchKernelGGL((k_fix_accum_ord<FIXCOV_DIAG_F32>), ga, ba, 0, st, s.v, P, base, n, (const double *)world, (const int *)srcrow, src.d_cov);
  else if (src.cov_kind == FIXCOV_FULL_F64) hipLaunchKernelGGL((k_fix_accum_ord<FIXCOV_FULL_F64>), ga, ba, 0, st, s.v, P, base, n, (const double *)world, (const int *)srcrow, src.d_cov);
  else hipLaunchKernelGGL((k_fix_accum_ord<FIXCOV_ZERO>), ga, ba, 0, st, s.v, P, base, n, (const double *)world, (const int *)srcrow, (const void *)nullptr);
  MAPCHK(hipGetLastError());
  if (src.cov_kind != FIXCOV_ZERO) s.have_var = true;       // the recut reads fvar (k_recut_push<true>)
  r = map_read_counters(s, st, err);
  if (r) return r;
  if (s.h_cnt[CNT_OVERFLOW]) { err = "voxel map capacity exceeded during fixed-point insert"; return VBA_ERR_CAPACITY; }
  return VBA_OK;
}

}  // namespace vba
