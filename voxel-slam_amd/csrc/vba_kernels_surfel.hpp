// Surfel / NDT export of the global map (vba_kf_surfel_export): the passes that follow the voxel export's insert,
// count and scan (vba_kernels_kf.hpp).  The table, the sums s, every record's slot and, in deterministic mode, the sorted runs are
// those of that front half; these kernels add the row of every kept voxel, the centred moments M = sum (a - c)(a - c)^T with
// c = s (1 / cnt), and the fit.  What they allocate against is the KEPT voxels: a 48-byte moment row and a 4-byte slot index each.
// Compiled without floating-point contraction (vba_surfel.hip): every product and sum below is rounded on its own, and the fit
// (vba_surfel_fit.hpp) gives the bits of its host build.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vba_common.hpp"
#include "vba_vx.hpp"
#include "vba_surfel_fit.hpp"

namespace vba {

// k_vx_emit's stable compaction, writing no record: the kept voxel of output row pos gets slot_of_row[pos] = its slot, and its
// slot's key, which nothing reads after the insert, becomes pos (the table is cleared by the next call's front half).
__global__ __launch_bounds__(256) void k_sf_rank(long long n, long long per, VxSlot *__restrict__ tab, const unsigned int *__restrict__ slot_of,
                                                 int min_count, const int *__restrict__ blk, int *__restrict__ slot_of_row) {
  __shared__ int wsum[4];
  const long long a = (long long)blockIdx.x * per, e = a + per < n ? a + per : n;
  int pos0 = blk[blockIdx.x];
  for (long long b0 = a; b0 < e; b0 += 256) {                 // (uniform per workgroup)
    const long long i = b0 + threadIdx.x;
    unsigned int h = 0;
    bool f = false;
    if (i < e) { h = slot_of[i]; f = tab[h].first == (int)i && tab[h].cnt >= min_count; }
    int tot;
    const int r = wg_rank(f, wsum, tot);
    if (f) {
      slot_of_row[pos0 + r] = (int)h;
      tab[h].key = (unsigned long long)(pos0 + r);
    }
    pos0 += tot;
    __syncthreads();                                          // wsum is rewritten by the next tile
  }
}

// the six products of d = a - c in the order xx xy xz yy yz zz
__device__ __forceinline__ void sf_products(float x, float y, float z, double cx, double cy, double cz, double p[6]) {
  const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
  p[0] = dx * dx; p[1] = dx * dy; p[2] = dx * dz; p[3] = dy * dy; p[4] = dy * dz; p[5] = dz * dz;
}

// Default mode: one record of S per lane over a capped, strided grid, the keyframe found as k_vx_insert finds it.  A record of a
// kept voxel adds its six products to the voxel's row of mom (zeroed before the launch) with f64 atomics.
__global__ __launch_bounds__(256) void k_sf_mom(long long n, int nkf, const VxKf *__restrict__ kft, int jump, const VxSlot *__restrict__ tab,
                                                const unsigned int *__restrict__ slot_of, const double *__restrict__ sum, int min_count,
                                                double *__restrict__ mom) {
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
      const unsigned int h = slot_of[i];
      const VxSlot s = tab[h];
      if (s.cnt >= min_count) {
        float x, y, z;
        vx_world(kft + vx_kf_of(i, lo, hi, kft), i, jump, x, y, z);
        const double inv = 1.0 / (double)s.cnt;
        const double *__restrict__ q = sum + 3 * (size_t)h;
        double p[6];
        sf_products(x, y, z, q[0] * inv, q[1] * inv, q[2] * inv, p);
        double *__restrict__ m = mom + 6 * (size_t)s.key;
#pragma unroll
        for (int k = 0; k < 6; k++) atomicAdd(m + k, p[k]);
      }
    }
  }
}

// Deterministic mode: the walk of k_vx_sum_det over the sorted runs.  The lane on the first position of a kept voxel's run adds
// the products of the run's records in ascending record index, ((0 + t_0) + t_1) + ..., and writes the row whole: no atomic.
__global__ __launch_bounds__(256) void k_sf_mom_det(long long n, const unsigned int *__restrict__ skey, const int *__restrict__ sidx,
                                                    const VxSlot *__restrict__ tab, int nkf, const VxKf *__restrict__ kft, int jump,
                                                    const double *__restrict__ sum, int min_count, double *__restrict__ mom) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const unsigned int h = skey[j];
  if (j > 0 && skey[j - 1] == h) return;
  const VxSlot s = tab[h];
  if (s.cnt < min_count) return;
  const long long end = j + s.cnt;
  const double inv = 1.0 / (double)s.cnt;
  const double *__restrict__ q = sum + 3 * (size_t)h;
  const double cx = q[0] * inv, cy = q[1] * inv, cz = q[2] * inv;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 0.0;
  int k = 0;                                                  // the records ascend, and so do their keyframes
  for (long long t = j; t < end; t++) {
    const long long r = sidx[t];
    k = vx_kf_of(r, k, nkf - 1, kft);
    float x, y, z;
    vx_world(kft + k, r, jump, x, y, z);
    double p[6];
    sf_products(x, y, z, cx, cy, cz, p);
    m0 += p[0]; m1 += p[1]; m2 += p[2]; m3 += p[3]; m4 += p[4]; m5 += p[5];
  }
  double *__restrict__ m = mom + 6 * (size_t)s.key;
  m[0] = m0; m[1] = m1; m[2] = m2; m[3] = m3; m[4] = m4; m[5] = m5;
}

// One kept voxel per lane, in output order: the mean, C = M (1 / cnt), the fit, the record as three 16-byte stores.  cov (may be
// mom itself: a lane reads its row before it writes it) and counts may be nullptr.
__global__ __launch_bounds__(256) void k_sf_fit(int m, const int *__restrict__ slot_of_row, const VxSlot *__restrict__ tab, const double *__restrict__ sum,
                                                const double *mom, int nkf, const VxKf *__restrict__ kft, float4 *__restrict__ out, double *cov,
                                                int *__restrict__ counts) {
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= m) return;
  const unsigned int h = (unsigned int)slot_of_row[pos];
  const VxSlot s = tab[h];
  const double inv = 1.0 / (double)s.cnt;
  const double *__restrict__ q = sum + 3 * (size_t)h;
  const double c[3] = {q[0] * inv, q[1] * inv, q[2] * inv};
  double M[6], C[6];
#pragma unroll
  for (int k = 0; k < 6; k++) M[k] = mom[6 * (size_t)pos + k];
  sf_cov(M, s.cnt, C);
  const VxKf *__restrict__ e = kft + vx_kf_of((long long)s.first, 0, nkf - 1, kft);
  const double sensor[3] = {e->T[9], e->T[10], e->T[11]};
  float r[12];
  sf_fit(c, C, s.cnt, sensor, e->inten, r);
  float4 *__restrict__ o = out + 3 * (size_t)pos;
  o[0] = make_float4(r[0], r[1], r[2], r[3]); o[1] = make_float4(r[4], r[5], r[6], r[7]); o[2] = make_float4(r[8], r[9], r[10], r[11]);
  if (cov) {
#pragma unroll
    for (int k = 0; k < 6; k++) cov[6 * (size_t)pos + k] = C[k];
  }
  if (counts) counts[pos] = s.cnt;
}

}  // namespace vba
