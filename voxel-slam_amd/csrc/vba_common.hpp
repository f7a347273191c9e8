// Inline host/device helpers that the kernel headers of more than one translation unit use: voxel keys, the plane fit's eigen-solver,
// the exact cluster transform, the workgroup rank, count, append and scan bodies of the compactions, var_world, the keyframe transform.  Nothing here is a kernel, so
// including it from several units compiles no kernel twice ("source layout").
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "vba_eig3.hpp"

namespace vba {

// vba_sort.hip (rocPRIM): stable radix sort of (key, value) pairs on key bits [0, end_bit); tmp == nullptr queries tmp_bytes
hipError_t sort_pairs_u32(void *tmp, size_t &tmp_bytes, const unsigned int *keys_in, unsigned int *keys_out, const int *vals_in, int *vals_out,
                          size_t n, unsigned int end_bit, hipStream_t stream);

// 16-bit bucket of a root voxel key; ranks own contiguous bucket ranges
__host__ __device__ inline uint64_t shard_bucket(int64_t kx, int64_t ky, int64_t kz) {
  uint64_t h = (uint64_t)kx * 0x9E3779B97F4A7C15ull;
  h ^= (uint64_t)ky * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
  h ^= (uint64_t)kz * 0x165667B19E3779F9ull + (h << 6) + (h >> 2);
  h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
  return h & 0xFFFFull;
}

static constexpr unsigned long long KEY_EMPTY = ~0ull;
static constexpr unsigned long long KEY_TOMB = ~0ull - 1;   // erased root (map pruning): probes walk past it
static constexpr int KEY_BITS = 21, KEY_OFF = 1 << 20;

__host__ __device__ inline unsigned long long pack_key(long long kx, long long ky, long long kz) {
  return ((unsigned long long)(kx + KEY_OFF) << 42) | ((unsigned long long)(ky + KEY_OFF) << 21) | (unsigned long long)(kz + KEY_OFF);
}
__host__ __device__ inline void unpack_key(unsigned long long k, long long &kx, long long &ky, long long &kz) {
  kx = (long long)((k >> 42) & 0x1FFFFF) - KEY_OFF; ky = (long long)((k >> 21) & 0x1FFFFF) - KEY_OFF; kz = (long long)(k & 0x1FFFFF) - KEY_OFF;
}
// The reference's key quirk VM:1907-1918: float narrowing, -1 if negative, truncation toward zero.
__host__ __device__ inline long long key_axis(double pw, double voxel_size) {
  float loc = (float)(pw / voxel_size);
  if (loc < 0) loc -= 1.0f;
  return (long long)loc;
}

// Rank of an occupancy mask of `nb` frames in the store order: popcount DESCENDING, masks of one popcount in ascending numeric order
// (colexicographic rank).  Equal masks share a bucket, so the counting sort of the extraction keeps them adjacent.
__host__ __device__ inline int mask_bucket(unsigned int m, int nb) {
  constexpr int C[11][11] = {{1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 3, 3, 1, 0, 0, 0, 0, 0, 0, 0},
                             {1, 4, 6, 4, 1, 0, 0, 0, 0, 0, 0}, {1, 5, 10, 10, 5, 1, 0, 0, 0, 0, 0}, {1, 6, 15, 20, 15, 6, 1, 0, 0, 0, 0},
                             {1, 7, 21, 35, 35, 21, 7, 1, 0, 0, 0}, {1, 8, 28, 56, 70, 56, 28, 8, 1, 0, 0}, {1, 9, 36, 84, 126, 126, 84, 36, 9, 1, 0},
                             {1, 10, 45, 120, 210, 252, 210, 120, 45, 10, 1}};
  int p = 0;
  for (int b = 0; b < nb; b++) p += (m >> b) & 1u;
  int off = 0;
  for (int q = nb; q > p; q--) off += C[nb][q];
  int r = 0, k = 0;
  for (int b = 0; b < nb; b++)
    if ((m >> b) & 1u) { k++; r += C[b][k]; }
  return off + r;
}

// ------------------------------------------------------------------------------------------------
// Symmetric 3x3 eigen-decomposition, ascending eigenvalues, orthonormal eigenvectors in columns.
// Cyclic Jacobi in registers (no indexed arrays -> no scratch).  Replaces Eigen::SelfAdjointEigenSolver
// at voxel_map.hpp:312 / :1416 / :1525 (result equal up to rounding and eigenvector sign).
// One Jacobi rotation in the (p,q) plane.  The rotation only has to be ORTHOGONAL to full precision, not optimal: the
// tangent t is computed in f32 (v_rcp_f32 / v_sqrt_f32, ~1e-7 relative), c = rsqrt(1 + t^2) in f64 (v_rsq_f64 + two
// Newton steps), s = t c, so c^2 + s^2 = 1 to rounding while the annihilated element is left at ~1e-7 |a_pq| and dies
// in the next sweep.  Measured on MI355X (K4, one wave per SIMD): the textbook form (f64 div, sqrt, div, sqrt, div per
// rotation) cost 10.3k cycles per eigen-solve, 45 % of the residual pass.
__device__ __forceinline__ void jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq,
                                           double &v0p, double &v0q, double &v1p, double &v1q, double &v2p, double &v2q,
                                           int sweep) {
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq);
  // an off-diagonal below ulp/200 of both diagonals cannot change them any more: drop it (at any sweep)
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { apq = 0.0; return; }
  // t = sgn(a) b / (|a| + sqrt(a^2 + b^2)),  a = (aqq - app) / 2, b = apq   (the smaller root of t^2 + 2 theta t - 1 = 0);
  // operands are scaled by the exponent of the larger magnitude first (exact, and defined for subnormal operands, where a
  // reciprocal overflows) so that the f32 range cannot over/underflow
  const double a = 0.5 * (aqq - app);
  int ex;
  (void)frexp(fmax(fabs(a), fabs(apq)), &ex);
  const float af = (float)ldexp(a, -ex), bf = (float)ldexp(apq, -ex);
  const float tf = bf * __builtin_amdgcn_rcpf(fabsf(af) + __builtin_amdgcn_sqrtf(af * af + bf * bf));   // raw v_sqrt_f32 / v_rcp_f32
  const double t = (af < 0.0f) ? -(double)tf : (double)tf;
  const double x = 1.0 + t * t;
  double c = __builtin_amdgcn_rsq(x);            // ~26 good bits
  c = c * (1.5 - 0.5 * x * c * c);
  c = c * (1.5 - 0.5 * x * c * c);
  const double s = t * c;
  // A <- J^T A J:  a_pp' = c^2 a_pp - 2 c s a_pq + s^2 a_qq, a_qq' likewise, a_pq' = c s (a_pp - a_qq) + (c^2 - s^2) a_pq
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

#define VBA_SWAP(a, b) { double _t = a; a = b; b = _t; }

// in: lower triangle a00,a10,a20,a11,a21,a22.  out: w0<=w1<=w2, V (row-major, columns = eigenvectors).  Plain cyclic sweeps in f64:
// this is the fallback of eig3_sym_dev below (near-double eigenvalue pairs — every line-like covariance among them —, multiples of
// the identity, degenerate input), written for few registers, not for speed (the sweep loop is not unrolled).
__device__ __forceinline__ Eig3 eig3_jacobi_dev(double a00, double a01, double a02, double a11, double a12, double a22) {
  // exact power-of-two scaling of the largest entry into [0.5, 1), as the direct path does: subnormal and huge matrices run in the
  // normal range (NaN input stays NaN)
  int e = 0;
  {
    const double s = fmax(fmax(fmax(fabs(a00), fabs(a11)), fabs(a22)), fmax(fmax(fabs(a01), fabs(a02)), fabs(a12)));
    if (s > 0.0 && s <= 1.7976931348623157e308) (void)frexp(s, &e);
  }
  a00 = ldexp(a00, -e); a01 = ldexp(a01, -e); a02 = ldexp(a02, -e); a11 = ldexp(a11, -e); a12 = ldexp(a12, -e); a22 = ldexp(a22, -e);
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
#pragma unroll 1
  for (int sweep = 0; sweep < 30; sweep++) {
    if (fabs(a01) + fabs(a02) + fabs(a12) == 0.0) break;
    jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21, sweep);  // (p,q)=(0,1), r=2
    jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22, sweep);  // (0,2), r=1
    jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22, sweep);  // (1,2), r=0
  }
  if (a11 < a00) { VBA_SWAP(a00, a11); VBA_SWAP(v00, v01); VBA_SWAP(v10, v11); VBA_SWAP(v20, v21); }
  if (a22 < a00) { VBA_SWAP(a00, a22); VBA_SWAP(v00, v02); VBA_SWAP(v10, v12); VBA_SWAP(v20, v22); }
  if (a22 < a11) { VBA_SWAP(a11, a22); VBA_SWAP(v01, v02); VBA_SWAP(v11, v12); VBA_SWAP(v21, v22); }
  Eig3 o;
  o.w0 = ldexp(a00, e); o.w1 = ldexp(a11, e); o.w2 = ldexp(a22, e);
  o.v00 = v00; o.v01 = v01; o.v02 = v02; o.v10 = v10; o.v11 = v11; o.v12 = v12; o.v20 = v20; o.v21 = v21; o.v22 = v22;
  return o;
}

// The plane fit's eigen-solver: direct (vba_eig3.hpp: trigonometric seed + Newton for the isolated root, its eigenvector from cross
// products, the pair by one Jacobi rotation of the 2x2 complement problem); matrices with a near-double eigenvalue pair, multiples of the identity and
// non-finite input take the Jacobi sweeps above.
__device__ __forceinline__ void eig3_sym_dev(double a00, double a01, double a02, double a11, double a12, double a22,
                                             double &w0, double &w1, double &w2, double *V) {
  Eig3 o;
  if (!eig3_direct(a00, a01, a02, a11, a12, a22, o)) o = eig3_jacobi_dev(a00, a01, a02, a11, a12, a22);
  w0 = o.w0; w1 = o.w1; w2 = o.w2;
  V[0] = o.v00; V[1] = o.v01; V[2] = o.v02; V[3] = o.v10; V[4] = o.v11; V[5] = o.v12; V[6] = o.v20; V[7] = o.v21; V[8] = o.v22;
}

// PointCluster::transform (tools.hpp:357-363) in the reference's operation order, every operation rounded separately (the
// reference targets baseline x86-64: no FMA contraction):  v' = R v + p N ;  rp = (R v) p^T ;  P' = ((R P R^T + rp) + rp^T) + (p p^T) N,
// matrix products as left-to-right dot products.  The six P scalars of a cluster are its LOWER triangle (what the eigen-solver of the
// reference reads, and what the pushes make symmetric anyway).  With the frames added in frame order (VM:297-305) pcr_adds — which
// margi copies into the map (VM:1498-1500) — comes out bit-identical to the CPU restatement's, so the map's sums stay exact over a session.
struct Cl10 { double p00, p10, p20, p11, p21, p22, v0, v1, v2, n; };
__device__ __forceinline__ Cl10 cluster_transform_exact(double c0, double c1, double c2, double c3, double c4, double c5, double v0, double v1, double v2, double n,
                                                        const double *R) {
#pragma clang fp contract(off)
  const double R0 = R[0], R1 = R[1], R2 = R[2], R3 = R[3], R4 = R[4], R5 = R[5], R6 = R[6], R7 = R[7], R8 = R[8];
  const double tx = R[9], ty = R[10], tz = R[11];
  const double rv0 = (R0 * v0 + R1 * v1) + R2 * v2, rv1 = (R3 * v0 + R4 * v1) + R5 * v2, rv2 = (R6 * v0 + R7 * v1) + R8 * v2;
  // M = R P (P symmetric: P01 = c1, P02 = c2, P12 = c4)
  const double m00 = (R0 * c0 + R1 * c1) + R2 * c2, m01 = (R0 * c1 + R1 * c3) + R2 * c4, m02 = (R0 * c2 + R1 * c4) + R2 * c5;
  const double m10 = (R3 * c0 + R4 * c1) + R5 * c2, m11 = (R3 * c1 + R4 * c3) + R5 * c4, m12 = (R3 * c2 + R4 * c4) + R5 * c5;
  const double m20 = (R6 * c0 + R7 * c1) + R8 * c2, m21 = (R6 * c1 + R7 * c3) + R8 * c4, m22 = (R6 * c2 + R7 * c4) + R8 * c5;
  Cl10 o;
  o.p00 = ((((m00 * R0 + m01 * R1) + m02 * R2) + rv0 * tx) + rv0 * tx) + (tx * tx) * n;
  o.p10 = ((((m10 * R0 + m11 * R1) + m12 * R2) + rv1 * tx) + rv0 * ty) + (ty * tx) * n;
  o.p20 = ((((m20 * R0 + m21 * R1) + m22 * R2) + rv2 * tx) + rv0 * tz) + (tz * tx) * n;
  o.p11 = ((((m10 * R3 + m11 * R4) + m12 * R5) + rv1 * ty) + rv1 * ty) + (ty * ty) * n;
  o.p21 = ((((m20 * R3 + m21 * R4) + m22 * R5) + rv2 * ty) + rv1 * tz) + (tz * ty) * n;
  o.p22 = ((((m20 * R6 + m21 * R7) + m22 * R8) + rv2 * tz) + rv2 * tz) + (tz * tz) * n;
  o.v0 = rv0 + tx * n; o.v1 = rv1 + ty * n; o.v2 = rv2 + tz * n;
  o.n = n;
  return o;
}

__device__ __forceinline__ void cluster_transform_dev(const double *c /*10*/, const double *R /*12*/, double *o /*10*/) {
  const Cl10 w = cluster_transform_exact(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], R);   // the reference's operation order
  o[0] = w.p00; o[1] = w.p10; o[2] = w.p20; o[3] = w.p11; o[4] = w.p21; o[5] = w.p22; o[6] = w.v0; o[7] = w.v1; o[8] = w.v2; o[9] = w.n;
}

__device__ __forceinline__ double wave_sum(double x) {
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// Sum over the 64 lanes of a wave, result valid in LANE 63 only.  Data-parallel-primitive moves instead of ds_bpermute
// (__shfl_xor goes through the LDS crossbar: ~100+ cycles per step, six dependent steps): quad swaps, row mirrors, then the
// two row broadcasts of gfx9.  Fixed summation tree, so the result does not depend on the launch.
__device__ __forceinline__ double dpp_mov_f64(double x, double old, const int ctrl, const int row_mask) {
  const long long xi = __double_as_longlong(x), oi = __double_as_longlong(old);
  int lo = (int)xi, hi = (int)(xi >> 32);
  const int olo = (int)oi, ohi = (int)(oi >> 32);
  switch (ctrl) {   // (the control word is an immediate operand)
    case 0xB1: lo = __builtin_amdgcn_update_dpp(olo, lo, 0xB1, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(ohi, hi, 0xB1, 0xF, 0xF, false); break;
    case 0x4E: lo = __builtin_amdgcn_update_dpp(olo, lo, 0x4E, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(ohi, hi, 0x4E, 0xF, 0xF, false); break;
    case 0x141: lo = __builtin_amdgcn_update_dpp(olo, lo, 0x141, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(ohi, hi, 0x141, 0xF, 0xF, false); break;
    case 0x140: lo = __builtin_amdgcn_update_dpp(olo, lo, 0x140, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(ohi, hi, 0x140, 0xF, 0xF, false); break;
    case 0x142: lo = __builtin_amdgcn_update_dpp(olo, lo, 0x142, 0xA, 0xF, false); hi = __builtin_amdgcn_update_dpp(ohi, hi, 0x142, 0xA, 0xF, false); break;
    default: lo = __builtin_amdgcn_update_dpp(olo, lo, 0x143, 0xC, 0xF, false); hi = __builtin_amdgcn_update_dpp(ohi, hi, 0x143, 0xC, 0xF, false); break;
  }
  (void)row_mask;
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_sum_to_lane63(double x) {
  x += dpp_mov_f64(x, x, 0xB1, 0xF);      // quad_perm [1,0,3,2]
  x += dpp_mov_f64(x, x, 0x4E, 0xF);      // quad_perm [2,3,0,1]
  x += dpp_mov_f64(x, x, 0x141, 0xF);     // row_half_mirror
  x += dpp_mov_f64(x, x, 0x140, 0xF);     // row_mirror: every lane of a 16-lane row holds the row's sum
  x += dpp_mov_f64(x, 0.0, 0x142, 0xA);   // row_bcast15 into rows 1 and 3 (the others add 0)
  x += dpp_mov_f64(x, 0.0, 0x143, 0xC);   // row_bcast31 into rows 2 and 3
  return x;
}

// a double every lane loaded from the same address, made wave-uniform for the compiler too
__device__ __forceinline__ double odom_uniform(double x) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
  return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------- workgroup compaction and scan ("Source layout")
// The LDS arrays are the calling kernel's.  Every thread of the workgroup must call these (they synchronise): a kernel returns its
// unflagged threads after the call, not before.
// rank of a flagged thread among the flagged threads of its 256-thread workgroup (lane order) and the workgroup's count
__device__ __forceinline__ int wg_rank(bool f, int *wsum /*[4]*/, int &tot) {
  const unsigned long long mask = __ballot(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = __popcll(mask);
  __syncthreads();
  int before = 0;
  tot = 0;
  for (int w = 0; w < 4; w++) { const int c = wsum[w]; before += w < wave ? c : 0; tot += c; }
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}
// the count pass of a stable compaction: blk[workgroup] = flagged threads of the workgroup
__device__ __forceinline__ void wg_count(bool f, int *wsum /*[4]*/, int *blk) {
  int tot;
  wg_rank(f, wsum, tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}
// Append the flagged threads of a 256-thread workgroup to a list whose length is *counter: the list position of a flagged thread
// (lane order inside the workgroup; the workgroups in the order their atomics land).  ONE returning atomic per workgroup, none when
// no thread is flagged.
__device__ __forceinline__ int wg_append(bool f, int *wbase /*[4]*/, int *counter) {
  const unsigned long long mask = __ballot(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wbase[wave] = __popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < 4; w++) { const int c = wbase[w]; wbase[w] = tot; tot += c; }
    const int base = tot ? atomicAdd(counter, tot) : 0;
    for (int w = 0; w < 4; w++) wbase[w] += base;
  }
  __syncthreads();
  return wbase[wave] + __popcll(mask & ((1ull << lane) - 1ull));
}
// Exclusive scan of a[0 .. n) in place by ONE workgroup of 1024, any n: chunks of 8192 entries go through LDS (coalesced loads and
// stores; thread t scans entries 8t .. 8t+7 of the chunk, wave shuffles and LDS combine the 1024 runs, a carry links the chunks).
// Returns the total in every thread.  k_det_scan and k_bg_scan are its wrappers.
constexpr int WG_SCAN_CHUNK = 1024 * 8;
__device__ __forceinline__ int wg_scan_chunked(int *a, int n, int *buf /*[WG_SCAN_CHUNK]*/, int *wsum /*[16]*/) {
  constexpr int K = 8, CH = WG_SCAN_CHUNK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int c0 = 0; c0 < n; c0 += CH) {
#pragma unroll
    for (int j = 0; j < K; j++) { const int i = c0 + j * 1024 + tid; buf[j * 1024 + tid] = i < n ? a[i] : 0; }
    __syncthreads();
    int v[K], loc = 0;
#pragma unroll
    for (int j = 0; j < K; j++) { v[j] = buf[tid * K + j]; loc += v[j]; }
    int incl = loc;
    for (int off = 1; off < 64; off <<= 1) { const int u = __shfl_up(incl, off, 64); if (lane >= off) incl += u; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int run = carry + incl - loc, tot = 0;
    for (int w = 0; w < 16; w++) { const int c = wsum[w]; run += w < wave ? c : 0; tot += c; }
#pragma unroll
    for (int j = 0; j < K; j++) { buf[tid * K + j] = run; run += v[j]; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; j++) { const int i = c0 + j * 1024 + tid; if (i < n) a[i] = buf[j * 1024 + tid]; }
    carry += tot;
    __syncthreads();   // (buf and wsum are rewritten by the next chunk)
  }
  return carry;
}
// Exclusive scan of in[0 .. n) into out[0 .. n) by ONE workgroup of 256 (n <= a few thousand; out may be in): thread t owns the
// ceil(n / 256) consecutive entries from t * per, thread 0 scans the 256 partial sums.  Returns the total to THREAD 0 (other threads: 0).
// k_ds_scan and k_big_scan are its wrappers.
__device__ __forceinline__ int wg_scan_strided(int n, const int *in, int *out, int *part /*[256]*/) {
  const int t = threadIdx.x, per = (n + 255) / 256;
  int s = 0, tot = 0;
  for (int k = 0; k < per; k++) { const int i = t * per + k; if (i < n) s += in[i]; }
  part[t] = s;
  __syncthreads();
  if (t == 0) { for (int k = 0; k < 256; k++) { const int v = part[k]; part[k] = tot; tot += v; } }
  __syncthreads();
  int acc = part[t];
  for (int k = 0; k < per; k++) { const int i = t * per + k; if (i < n) { const int v = in[i]; out[i] = acc; acc += v; } }
  return tot;
}

// pvec_update (voxelslam.hpp:242-265): var_world = R var R^T + phat rot_var phat^T + tsl_var for the body point (bx, by, bz), in the
// reference's operation order, every operation rounded separately.  R row-major (9), cov6 = [rot_var(9) | tsl_var(9)]; out may not
// alias var.
__device__ __forceinline__ void var_world(const double *R, const double *cov6, double bx, double by, double bz, const double *var /*9*/, double *out /*9*/) {
#pragma clang fp contract(off)
  double RV[9], PR[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) RV[3 * r + c] = (R[3 * r] * var[c] + R[3 * r + 1] * var[3 + c]) + R[3 * r + 2] * var[6 + c];
  const double ph[9] = {0, -bz, by, bz, 0, -bx, -by, bx, 0};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) PR[3 * r + c] = (ph[3 * r] * cov6[c] + ph[3 * r + 1] * cov6[3 + c]) + ph[3 * r + 2] * cov6[6 + c];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++)
      out[3 * r + c] = (((RV[3 * r] * R[3 * c] + RV[3 * r + 1] * R[3 * c + 1]) + RV[3 * r + 2] * R[3 * c + 2]) +
                        ((PR[3 * r] * ph[3 * c] + PR[3 * r + 1] * ph[3 * c + 1]) + PR[3 * r + 2] * ph[3 * c + 2])) + cov6[9 + 3 * r + c];
}

// q = ((T[0] x + T[1] y) + T[2] z) + T[9], ... with T = [dR row-major (9), dp (3)]
__device__ __forceinline__ void kf_apply(const double *__restrict__ T, double x, double y, double z, double &qx, double &qy, double &qz) {
#pragma clang fp contract(off)
  qx = ((T[0] * x + T[1] * y) + T[2] * z) + T[9];
  qy = ((T[3] * x + T[4] * y) + T[5] * z) + T[10];
  qz = ((T[6] * x + T[7] * y) + T[8] * z) + T[11];
}

}  // namespace vba
