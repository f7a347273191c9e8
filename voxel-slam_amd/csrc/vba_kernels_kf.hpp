// Keyframe store (vba_kf_*): the merge of K clouds into the frame of the last one's pose (VS:2354-2371, VS:348-372,
// VS:384-398), the emit of the kept cloud into the store, and the keyframe -> world transform of keyframe_loading (VS:1418-1427).
// One thread per point, lanes on consecutive points.  Every product and sum below is rounded on its own (no contraction): the
// order of operations is part of the interface (include/voxelba.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vba_common.hpp"
#include "vba_kernels_scan.hpp"
#include "vba_vx.hpp"

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
  const int i = blockIdx.x * 256 + threadIdx.x;
  DsSlot s;
  bool f = false;
  if (i < n) { s = tab[slot_of[i]]; f = s.first == i; }
  int tot;
  const int pos = blk[blockIdx.x] + wg_rank(f, wsum, tot);
  if (!f) return;
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

// Voxel-down-sampled global map (vba_kf_voxel_export): the gather of k_kf_export fused with the voxel filter of
// down_sampling_voxel (TL:201-238) over the whole sequence S of exported records; S itself is never written.
// The per-keyframe table VxKf, the slot VxSlot and the record of S (vx_kf_of, vx_world) are vba_vx.hpp, shared with the surfel passes.

__global__ __launch_bounds__(256) void k_vx_clear(VxSlot *__restrict__ tab, size_t cap) {
  VxSlot s; s.key = DS_EMPTY; s.cnt = 0; s.first = 0x7fffffff;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (size_t)gridDim.x * 256) tab[i] = s;
}

// One record of S per lane over a capped, strided grid, the keyframe found as k_kf_export finds it (two lanes search the table for
// the workgroup's first and last record, every lane between them); then the key of TL:209-216 on the FLOAT coordinates, the
// open-addressing insert, the voxel's count and first record, the record's slot.  mask = slots - 1 (a power of two >= 2 n: the
// probe always ends).  DET: no f64 atomics, k_vx_sum_det forms the sums.
template <bool DET>
__global__ __launch_bounds__(256) void k_vx_insert(long long n, int nkf, const VxKf *__restrict__ kft, int jump, double voxel_size, VxSlot *__restrict__ tab,
                                                   unsigned int mask, unsigned int *__restrict__ slot_of, double *__restrict__ sum) {
  __shared__ int s_k[2];
  const long long step = (long long)gridDim.x * 256;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += step) {        // (uniform per workgroup: the barriers below are safe)
    const long long rem = n - base, cnt = rem < 256 ? rem : 256;
    if (threadIdx.x < 2) s_k[threadIdx.x] = vx_kf_of(base + (threadIdx.x ? cnt - 1 : 0), 0, nkf - 1, kft);
    __syncthreads();
    const int lo = s_k[0], hi = s_k[1];
    __syncthreads();                                          // s_k is rewritten by the next round
    if ((long long)threadIdx.x < cnt) {
      const long long i = base + threadIdx.x;
      float x, y, z;
      vx_world(kft + vx_kf_of(i, lo, hi, kft), i, jump, x, y, z);
      const unsigned long long key = ds_pack(ds_axis_key((double)x, voxel_size), ds_axis_key((double)y, voxel_size), ds_axis_key((double)z, voxel_size));
      unsigned int h = ds_hash(key) & mask;
      for (;;) {
        const unsigned long long old = atomicCAS(&tab[h].key, DS_EMPTY, key);
        if (old == DS_EMPTY || old == key) break;
        h = (h + 1) & mask;
      }
      atomicAdd(&tab[h].cnt, 1);
      atomicMin(&tab[h].first, (int)i);
      slot_of[i] = h;
      if (!DET) {
        double *__restrict__ s = sum + 3 * (size_t)h;
        atomicAdd(s, (double)x); atomicAdd(s + 1, (double)y); atomicAdd(s + 2, (double)z);
      }
    }
  }
}

// Deterministic mode: (slot, record) pairs sorted by slot with the stable radix sort, so a voxel's records are one run of skey in
// ascending record index.  The lane on the first position of a run adds the run's float coordinates in that order,
// ((0 + a_0) + a_1) + ..., recomputing each from the store (24 bytes read against the 16 written and 16 read of a kept record, §23).
__global__ __launch_bounds__(256) void k_vx_sum_det(long long n, const unsigned int *__restrict__ skey, const int *__restrict__ sidx, const VxSlot *__restrict__ tab,
                                                    int nkf, const VxKf *__restrict__ kft, int jump, double *__restrict__ sum) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const unsigned int h = skey[j];
  if (j > 0 && skey[j - 1] == h) return;
  const long long end = j + tab[h].cnt;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int k = 0;                                                  // the records ascend, and so do their keyframes
  for (long long t = j; t < end; t++) {
    const long long q = sidx[t];
    k = vx_kf_of(q, k, nkf - 1, kft);
    float x, y, z;
    vx_world(kft + k, q, jump, x, y, z);
    sx += (double)x; sy += (double)y; sz += (double)z;
  }
  double *__restrict__ s = sum + 3 * (size_t)h;
  s[0] = sx; s[1] = sy; s[2] = sz;
}

// kept voxel = the first record of a voxel with at least min_count records; blk[b] = kept voxels among workgroup b's records
__global__ __launch_bounds__(256) void k_vx_count(long long n, long long per, const VxSlot *__restrict__ tab, const unsigned int *__restrict__ slot_of,
                                                  int min_count, int *__restrict__ blk) {
  __shared__ int wsum[4];
  const long long a = (long long)blockIdx.x * per, e = a + per < n ? a + per : n;
  int c = 0;
  for (long long i = a + threadIdx.x; i < e; i += 256) {
    const VxSlot s = tab[slot_of[i]];
    c += (s.first == (int)i && s.cnt >= min_count) ? 1 : 0;
  }
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// stable compaction of the kept voxels in the order of their first records (k_ds_emit's order); blk = the exclusive scan of
// k_vx_count's counts.  x y z = (float)(sum * (1 / cnt)), the intensity of the first record's store, counts[pos] = cnt.
__global__ __launch_bounds__(256) void k_vx_emit(long long n, long long per, const VxSlot *__restrict__ tab, const unsigned int *__restrict__ slot_of,
                                                 const double *__restrict__ sum, int min_count, const int *__restrict__ blk, int nkf,
                                                 const VxKf *__restrict__ kft, float4 *__restrict__ out, int *__restrict__ counts) {
  __shared__ int wsum[4];
  const long long a = (long long)blockIdx.x * per, e = a + per < n ? a + per : n;
  int pos0 = blk[blockIdx.x];
  for (long long b0 = a; b0 < e; b0 += 256) {                 // (uniform per workgroup)
    const long long i = b0 + threadIdx.x;
    VxSlot s;
    unsigned int h = 0;
    bool f = false;
    if (i < e) { h = slot_of[i]; s = tab[h]; f = s.first == (int)i && s.cnt >= min_count; }
    int tot;
    const int r = wg_rank(f, wsum, tot);
    if (f) {
      const size_t pos = (size_t)(pos0 + r);
      const double inv = 1.0 / (double)s.cnt;
      const double *__restrict__ q = sum + 3 * (size_t)h;
      out[pos] = make_float4((float)(q[0] * inv), (float)(q[1] * inv), (float)(q[2] * inv), kft[vx_kf_of(i, 0, nkf - 1, kft)].inten);
      if (counts) counts[pos] = s.cnt;
    }
    pos0 += tot;
    __syncthreads();                                          // wsum is rewritten by the next tile
  }
}

}  // namespace vba
