// Keyframe store (vba_kf_*): the merge of K clouds into the frame of the last one's pose (VS:2354-2371, VS:348-372,
// VS:384-398), the emit of the kept cloud into the store, and the keyframe -> world transform of keyframe_loading (VS:1418-1427).
// One thread per point, lanes on consecutive points.  Every product and sum below is rounded on its own (no contraction): the
// order of operations is part of the interface (include/voxelba.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vba_common.hpp"
#include "vba_kernels_scan.hpp"

namespace vba {

// Merge: point i of the concatenated input belongs to scan j with off[j] <= i < off[j + 1] and moves by xf[j] ([k][12]).
//   out   double [n][3]  the merged cloud (down-sampler input), may be nullptr
//   outf  float  [n][3]  the same narrowed to float (the descriptor generator's point buffer), may be nullptr
//   var / vout           covariance rows (vrow doubles apart, diagonal entries vstep apart) -> double [n][3] diagonals, unrotated
// the scan of merged point i: the last j with off[j] <= i (empty scans are skipped by the <=)
__device__ __forceinline__ int kf_merge_scan(int i, int k, const int *__restrict__ off) {
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// merged point i from source row `row`, moved by T
__device__ __forceinline__ void kf_merge_point(int i, size_t row, const double *__restrict__ T, const double *__restrict__ pnt, const double *__restrict__ var,
                                               int vrow, int vstep, double *__restrict__ out, float *__restrict__ outf, double *__restrict__ vout) {
  const size_t b = 3 * (size_t)i, sb = 3 * row;
  double qx, qy, qz;
  kf_apply(T, pnt[sb], pnt[sb + 1], pnt[sb + 2], qx, qy, qz);
  if (out) { out[b] = qx; out[b + 1] = qy; out[b + 2] = qz; }
  if (outf) { outf[b] = (float)qx; outf[b + 1] = (float)qy; outf[b + 2] = (float)qz; }
  if (vout) {
    const double *v = var + (size_t)vrow * row;
    vout[b] = v[0]; vout[b + 1] = v[vstep]; vout[b + 2] = v[2 * vstep];
  }
}
__global__ __launch_bounds__(256) void k_kf_merge(int n, int k, const int *__restrict__ off, const double *__restrict__ xf, const double *__restrict__ pnt,
                                                  const double *__restrict__ var, int vrow, int vstep, double *__restrict__ out, float *__restrict__ outf,
                                                  double *__restrict__ vout) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int lo = kf_merge_scan(i, k, off);
  kf_merge_point(i, (size_t)i, xf + 12 * lo, pnt, var, vrow, vstep, out, outf, vout);
}
// The merge from a scan log (vba_kf_build_from_log): the scans are whole but not contiguous, scan j starts at arena row start[j],
// so merged point i is row start[j] + (i - off[j]) of pnt and of var.
__global__ __launch_bounds__(256) void k_kf_merge_rows(int n, int k, const int *__restrict__ off, const int *__restrict__ start, const double *__restrict__ xf,
                                                       const double *__restrict__ pnt, const double *__restrict__ var, int vrow, int vstep,
                                                       double *__restrict__ out, float *__restrict__ outf, double *__restrict__ vout) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int lo = kf_merge_scan(i, k, off);
  kf_merge_point(i, (size_t)start[lo] + (size_t)(i - off[lo]), xf + 12 * lo, pnt, var, vrow, vstep, out, outf, vout);
}

// keyframe_loading: world = x0.R p + x0.p in the same operation order, T = the keyframe's x0 ([12])
__global__ __launch_bounds__(256) void k_kf_world(int n, const double *__restrict__ T, const double *__restrict__ pnt, double *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t b = 3 * (size_t)i;
  double qx, qy, qz;
  kf_apply(T, pnt[b], pnt[b + 1], pnt[b + 2], qx, qy, qz);
  out[b] = qx; out[b + 1] = qy; out[b + 2] = qz;
}

// k_ds_emit for the store: centroid rounded once to float and carried in doubles, the mean covariance diagonal as float (zero
// without covariances), the voxel's point count; first-occurrence order
__global__ __launch_bounds__(256) void k_kf_emit(int n, const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, const int *__restrict__ blk,
                                                 double *__restrict__ out, float *__restrict__ vout, int *__restrict__ count, int have_var) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  DsSlot s;
  int f = 0;
  if (i < n) { s = tab[slot_of[i]]; f = (s.first == i) ? 1 : 0; }
  const unsigned long long m = __ballot(f);
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  if (!f) return;
  int pos = blk[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; k++) pos += wsum[k];
  const double inv = 1.0 / (double)s.cnt;
  const size_t b = 3 * (size_t)pos;
  out[b] = (double)(float)(s.sx * inv); out[b + 1] = (double)(float)(s.sy * inv); out[b + 2] = (double)(float)(s.sz * inv);
  vout[b] = have_var ? (float)(s.vx * inv) : 0.0f; vout[b + 1] = have_var ? (float)(s.vy * inv) : 0.0f; vout[b + 2] = have_var ? (float)(s.vz * inv) : 0.0f;
  count[pos] = s.cnt;
}

// pub_globalmap (VS:110-154): the strided gather of the stores' keyframes into 16-byte x y z intensity records.
// One table row per keyframe, in publication order: the exported points before it (`first`, counted over the whole export), the
// store row of its first point, its current x0.  Keyframe k contributes rows row, row + jump, ... (the stride restarts at every
// keyframe, VS:133), so exported point i of keyframe k is store row  row + (i - first) * jump.
struct ExpKf { long long first; long long row; double T[12]; };   // 112 bytes

// One output record per lane, lanes on consecutive records; the grid is capped and strides over the rest.  Outputs i0 .. i0 + n - 1
// of the export, out = the record of i0; tab[0 .. nkf) = the keyframes of ONE store that these outputs can touch (tab[0].first <= i0),
// pnt = that store's point array.  A workgroup's 256 consecutive outputs touch the keyframes between the one of its first and the
// one of its last output: two lanes find those two in the table, every lane then searches only between them (as k_kf_merge does
// over its whole table; empty keyframes are skipped by the <=).  world = x0.R p + x0.p in kf_apply's order, each coordinate narrowed
// to float once (pp.x = vv[0], VS:139-141); one 16-byte store per record.  Every index into pnt and out is formed in 64 bits.
__global__ __launch_bounds__(256) void k_kf_export(long long i0, long long n, int nkf, const ExpKf *__restrict__ tab, const double *__restrict__ pnt,
                                                   int jump, float intensity, float4 *__restrict__ out) {
  __shared__ int s_k[2];
  const long long step = (long long)gridDim.x * 256;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += step) {        // (uniform per workgroup: the barriers below are safe)
    const long long rem = n - base, cnt = rem < 256 ? rem : 256;
    if (threadIdx.x < 2) {
      const long long t = i0 + base + (threadIdx.x ? cnt - 1 : 0);
      int lo = 0, hi = nkf - 1;                               // last j with tab[j].first <= t
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first <= t) lo = mid; else hi = mid - 1;
      }
      s_k[threadIdx.x] = lo;
    }
    __syncthreads();
    int lo = s_k[0], hi = s_k[1];
    __syncthreads();                                          // s_k is rewritten by the next round
    if ((long long)threadIdx.x < cnt) {
      const long long o = base + threadIdx.x, i = i0 + o;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first <= i) lo = mid; else hi = mid - 1;
      }
      const ExpKf *__restrict__ e = tab + lo;
      const long long row = e->row + (i - e->first) * (long long)jump;
      const size_t b = 3 * (size_t)row;
      double x, y, z;
      kf_apply(e->T, pnt[b], pnt[b + 1], pnt[b + 2], x, y, z);
      out[o] = make_float4((float)x, (float)y, (float)z, intensity);
    }
  }
}

}  // namespace vba
