// Decode of a raw sensor message: Features::process (feature_point.hpp:103-366) + pcl_handler (voxelslam.hpp:77-103).
//   k_scan_decode   raw records -> decoded record + sort key per candidate slot, kept points counted per workgroup
//   k_scan_pairs    stable compaction of the kept candidates into the sort's (key, index) pairs; unused slots get the empty key
//   k_scan_finish   the 0.11 s cut on the sorted keys, the two-point rule, the gathered cloud in the stored form
// Between k_scan_decode and k_scan_pairs runs k_ds_scan (vba_kernels_scan.hpp), between k_scan_pairs and k_scan_finish the stable
// radix sort of vba_sort.hip.  No kernel here uses an atomic: the order of the kept points is part of the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/voxelba.h"
#include "vba_common.hpp"

namespace vba {

struct ScanLayoutDev { int step, ox, oy, oz, oi, itype, ot, ttype, filter; };

static constexpr unsigned int SCAN_KEY_EMPTY = 0xFFFFFFFFu;   // as a curvature: a NaN, unsupported input
static constexpr int SCAN_LDS_STEP = 64;                       // largest point_step staged through the LDS (16 KiB image)

// order-preserving float -> u32 map; -0 is +0 first (a comparison sort sees them equal)
__host__ __device__ inline unsigned int scan_time_key(float c) {
  unsigned int u;
  __builtin_memcpy(&u, &c, 4);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

// One thread per raw record, 256 consecutive records per workgroup.  LDS: the workgroup's byte range [256 b step, 256 (b + 1) step)
// - a multiple of 16 bytes long, 16-byte aligned because the frame owns the buffer - goes to the LDS with 16-byte loads, and every
// lane assembles its fields from LDS bytes (a 26-byte stride leaves them unaligned).  !LDS (point_step > 64): the same byte-wise
// assembly straight from global memory.  Record i is a candidate when the decimation keeps it; candidate slot j = i / pfn (i without
// the filter) receives rec[5 j] = x y z intensity curvature and key[j] (SCAN_KEY_EMPTY when the blind test drops it).
template <bool LDS>
__global__ __launch_bounds__(256) void k_scan_decode(const unsigned char *__restrict__ raw, size_t raw_bytes, int n_raw, ScanLayoutDev L, int pfn, double blind2,
                                                     float *__restrict__ rec, unsigned int *__restrict__ key, int *__restrict__ blk) {
#pragma clang fp contract(off)
  __shared__ uint4 img[LDS ? 16 * SCAN_LDS_STEP : 1];
  __shared__ int wsum[4];
  __shared__ double t0s;
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  const unsigned char *r;
  if (LDS) {
    const size_t base = (size_t)blockIdx.x * 256 * (size_t)L.step;
    const int nvec = 16 * L.step;
    for (int v = t; v < nvec; v += 256) {
      const size_t off = base + 16 * (size_t)v;
      if (off < raw_bytes) img[v] = *(const uint4 *)(raw + off);    // raw_bytes is a multiple of 16: the last load ends inside the padding
    }
    r = (const unsigned char *)img + t * L.step;
  } else {
    r = raw + (size_t)i * (size_t)L.step;
  }
  if (t == 0 && L.ttype == VBA_SCAN_TIME_F64_REL_FIRST) { double d; __builtin_memcpy(&d, raw + L.ot, 8); t0s = d; }   // record 0: a broadcast
  __syncthreads();
  const bool cand = i < n_raw && (!L.filter || i % pfn == 0);
  bool keep = false;
  if (cand) {
    float x, y, z, in = 0.f, cv = 0.f;
    __builtin_memcpy(&x, r + L.ox, 4); __builtin_memcpy(&y, r + L.oy, 4); __builtin_memcpy(&z, r + L.oz, 4);
    if (L.itype == VBA_SCAN_INTENSITY_F32) __builtin_memcpy(&in, r + L.oi, 4);
    else if (L.itype == VBA_SCAN_INTENSITY_U8) in = (float)r[L.oi];
    if (L.ttype == VBA_SCAN_TIME_F32) __builtin_memcpy(&cv, r + L.ot, 4);
    else if (L.ttype == VBA_SCAN_TIME_U32_DIV1E9) { unsigned int u; __builtin_memcpy(&u, r + L.ot, 4); cv = (float)u / 1e9f; }   // one IEEE division (FP:155)
    else if (L.ttype == VBA_SCAN_TIME_F64_REL_FIRST) { double d; __builtin_memcpy(&d, r + L.ot, 8); cv = (float)(d - t0s); }
    const float r2 = (x * x + y * y) + z * z;
    keep = !L.filter || (double)r2 > blind2;
    const size_t j = (size_t)(L.filter ? i / pfn : i);
    rec[5 * j] = x; rec[5 * j + 1] = y; rec[5 * j + 2] = z; rec[5 * j + 3] = in; rec[5 * j + 4] = cv;
    key[j] = keep ? scan_time_key(cv) : SCAN_KEY_EMPTY;
  }
  wg_count(keep, wsum, blk);
}

// Same grid as k_scan_decode, after k_ds_scan: blk holds the exclusive scan of the workgroup counts, *total the kept points.  The kept
// candidates go to kin / vin [0, total) in message order, the slots [total, n_sort) get the empty key and sort to the end.
__global__ __launch_bounds__(256) void k_scan_pairs(int n_raw, int filter, int pfn, int n_sort, const unsigned int *__restrict__ key, const int *__restrict__ blk,
                                                    const int *__restrict__ total, unsigned int *__restrict__ kin, int *__restrict__ vin) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool cand = i < n_raw && (!filter || i % pfn == 0);
  const int j = filter ? i / pfn : i;
  const unsigned int k = cand ? key[j] : SCAN_KEY_EMPTY;
  const bool f = k != SCAN_KEY_EMPTY;
  int tot;
  const int rank = wg_rank(f, wsum, tot);
  if (f) { const int pos = blk[blockIdx.x] + rank; kin[pos] = k; vin[pos] = j; }
  if (i < n_sort && i >= *total) { kin[i] = SCAN_KEY_EMPTY; vin[i] = 0; }
}

// kout / vout: the sorted pairs, the first *total of them points.  n = the points whose curvature is <= 0.11 as a double (kcut is the key
// of the largest such float): VH:96-97.  No kept point at all: the two points of VH:82-90.  res = {n, bits of the last curvature}.
__global__ __launch_bounds__(256) void k_scan_finish(const unsigned int *__restrict__ kout, const int *__restrict__ vout, const float *__restrict__ rec,
                                                     const int *__restrict__ total, unsigned int kcut, double *__restrict__ pnt, double *__restrict__ curv,
                                                     float *__restrict__ inten, int *__restrict__ res) {
  __shared__ int ns;
  if (threadIdx.x == 0) {
    const int tot = *total;
    int lo = 0, hi = tot;                      // first position whose key is > kcut
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (kout[mid] <= kcut) lo = mid + 1; else hi = mid; }
    ns = tot == 0 ? -1 : lo;
  }
  __syncthreads();
  const int n = ns, g = blockIdx.x * 256 + threadIdx.x;
  if (n < 0) {
    if (g < 2) {
      const float c = g ? 0.09f : 0.f;
      pnt[3 * g] = 0.0; pnt[3 * g + 1] = 0.0; pnt[3 * g + 2] = 0.0; inten[g] = 0.f; curv[g] = (double)c;
      if (g == 1) { res[0] = 2; res[1] = __float_as_int(c); }
    }
    return;
  }
  if (g == 0) { res[0] = n; res[1] = n > 0 ? __float_as_int(rec[5 * (size_t)vout[n - 1] + 4]) : 0; }
  if (g >= n) return;
  const float *q = rec + 5 * (size_t)vout[g];
  pnt[3 * (size_t)g] = (double)q[0]; pnt[3 * (size_t)g + 1] = (double)q[1]; pnt[3 * (size_t)g + 2] = (double)q[2];
  inten[g] = q[3]; curv[g] = (double)q[4];
}

}  // namespace vba
