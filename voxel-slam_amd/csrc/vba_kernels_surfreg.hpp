// Kernels of the surfel map, of the registration against it (vba_surfel_map_*, vba_surfel_register) and of the point
// loop of the odometry update against it (vba_odom_surfel_update, §27), compiled by vba_surfreg.hip without contraction.  The
// arithmetic is vba_surfreg_math.hpp (shared with the g++ build of the tests); the kernels below own the table build, which
// workgroup owns which points, and the order of the sums.
//
// Order contract of an iteration over n points with nb = min(ceil(n / 256), SREG_MAX_BLOCKS) workgroups of 256: lane l of workgroup
// b adds its points b * 256 + l, (b + nb) * 256 + l, ... in ascending order into 29 chains; a wave adds its 64 lanes by the xor
// butterfly (32, 16, ..., 1); a workgroup adds its waves as (w0 + w1) + (w2 + w3); the step adds the nb partials in ascending order.
// Nothing adds floating point with atomics: every result is a function of n and the inputs alone.
#pragma once
#include <hip/hip_runtime.h>
#include "vba_common.hpp"
#include "vba_surfreg_math.hpp"
#include "vba_odom_ekf.hpp"

namespace vba {

constexpr int SREG_MAX_BLOCKS = 1024;

// status words of a build: the cells inserted, and whether two records met in one key
struct SregBuildStatus { int n_cells, dup; };

__global__ __launch_bounds__(256) void k_sreg_clear(SregSlot *__restrict__ tab, unsigned int slots, SregBuildStatus *__restrict__ status) {
  const unsigned int i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) { status->n_cells = 0; status->dup = 0; }
  if (i >= slots) return;
  SregSlot s; s.key = DS_EMPTY; s.row = -1; s.pad = 0;
  tab[i] = s;
}

// record i with [11] >= min_count becomes cell i: its slot is claimed by a compare-and-swap on the key (which slot a key lands in
// depends on the order of the claims, what a lookup returns does not), the payload is written by the claimant alone
__global__ __launch_bounds__(256) void k_sreg_insert(int n, const float *__restrict__ rec, const double *__restrict__ cov, double voxel, double sigma,
                                                    int min_count, SregSlot *__restrict__ tab, unsigned int mask, SregCell *__restrict__ cell,
                                                    SregBuildStatus *__restrict__ status) {
  BTC_NOCONTRACT
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float *r = rec + 12 * (size_t)i;
  if (!(r[11] >= (float)min_count)) return;
  const unsigned long long key = sreg_key(r, voxel);
  unsigned int h = ds_hash(key) & mask;
  bool mine = false;
  for (unsigned int probe = 0; probe <= mask; probe++) {    // the table has >= 2 n slots: always terminates
    const unsigned long long old = atomicCAS(&tab[h].key, DS_EMPTY, key);
    if (old == DS_EMPTY) { mine = true; break; }
    if (old == key) break;
    h = (h + 1) & mask;
  }
  if (!mine) { atomicOr(&status->dup, 1); return; }
  tab[h].row = i;
  SregCell c;
  sreg_make_cell(r, cov + 6 * (size_t)i, sigma, &c);
  cell[i] = c;
  atomicAdd(&status->n_cells, 1);
}

// The point loop and the first two levels of the order contract above, written once for k_sreg_accum and k_sodom_accum: the lane
// chains over this workgroup's points at the pose and gate of st, the butterfly of each wave, the four wave sums in red, and the
// barrier behind them.  Taps as in k_sreg_accum.  sreg_wg_sum then gives (w0 + w1) + (w2 + w3) of sum k to whichever lane asks.
__device__ __forceinline__ void sreg_accum_waves(int n, const double *__restrict__ pnt, const SregTable &T, const SregState &st,
                                                 int *__restrict__ cellrow, unsigned char *__restrict__ gate, double (*red)[SREG_PART]) {
  BTC_NOCONTRACT
  double s[SREG_PART];
#pragma unroll
  for (int k = 0; k < SREG_PART; k++) s[k] = 0.0;
  const int stride = (int)gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const double p[3] = {pnt[3 * (size_t)i], pnt[3 * (size_t)i + 1], pnt[3 * (size_t)i + 2]};
    bool pass;
    const int row = sreg_point(T, st, p, s, &pass);
    if (cellrow) cellrow[i] = row;
    if (gate) gate[i] = pass ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < SREG_PART; k++) s[k] = wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < SREG_PART; k++) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
}
__device__ __forceinline__ double sreg_wg_sum(const double (*red)[SREG_PART], int k) {
  BTC_NOCONTRACT
  return (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// One iteration's sums: per-workgroup partials [nb][29].  Taps (null in vba_surfel_register): cellrow[n] the chosen row or -1,
// gate[n] 1 where the point entered the sums.
__global__ __launch_bounds__(256) void k_sreg_accum(int n, const double *__restrict__ pnt, SregTable T, const SregState *__restrict__ st,
                                                   double *__restrict__ part, int *__restrict__ cellrow, unsigned char *__restrict__ gate) {
  BTC_NOCONTRACT
  __shared__ double red[4][SREG_PART];
  if (st->done) return;
  sreg_accum_waves(n, pnt, T, *st, cellrow, gate, red);
  if (threadIdx.x < SREG_PART) part[(size_t)blockIdx.x * SREG_PART + threadIdx.x] = sreg_wg_sum(red, threadIdx.x);
}

// The point loop of one iteration of the prior-map odometry update (vba_odom_surfel_update): the same points, cells,
// gate, terms and sums at the pose S->R, S->t of the EKF image, returning at once when the image's stop rule has fired.  One row [34]
// per workgroup in the layout k_odom_update reduces (vba_odom_ekf.hpp): columns 0..20 the sums 0..20 (J^T W J), 21..26 the negated
// sums 21..26 (HTz = -J^T W d), 27..32 the sums 15..20 again (the sum of W where the voxel map puts n n^T), 33 the count.  Sum 27
// (m / 2) goes to cost[workgroup], a tap like cellrow and gate: null in the loop.
constexpr int SODOM_ROW = 34;
__global__ __launch_bounds__(256) void k_sodom_accum(int n, const double *__restrict__ pnt, SregTable T, const vbh::OdomEkf *__restrict__ S,
                                                    double gate2, int neighbors, double *__restrict__ part, double *__restrict__ cost,
                                                    int *__restrict__ cellrow, unsigned char *__restrict__ gate) {
  BTC_NOCONTRACT
  __shared__ double red[4][SREG_PART];
  if (__builtin_amdgcn_readfirstlane(S->done)) return;
  SregState X;                                             // what sreg_point reads of a state: pose, gate, candidates
#pragma unroll
  for (int k = 0; k < 9; k++) X.R[k] = S->R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) X.t[k] = S->t[k];
  X.gate2 = gate2; X.neighbors = neighbors;
  sreg_accum_waves(n, pnt, T, X, cellrow, gate, red);
  const int c = threadIdx.x;
  if (c < SODOM_ROW) {
    const int k = c < 27 ? c : (c < 33 ? c - 12 : 28);
    const double v = sreg_wg_sum(red, k);
    part[(size_t)blockIdx.x * SODOM_ROW + c] = (c >= 21 && c < 27) ? -v : v;
  }
  if (cost && c == 0) cost[blockIdx.x] = sreg_wg_sum(red, 27);
}

// reduce the partials in workgroup order, step (vba_surfreg_math.hpp), and at the end of the loop the eigenvalues of the
// translation block.  Taps: sums[29] the reduced partials, dxo[6] the step.
__global__ __launch_bounds__(64) void k_sreg_step(int nb, const double *__restrict__ part, SregState *st, double *sums, double *dxo) {
  BTC_NOCONTRACT
  __shared__ double acc[SREG_PART], work[36];
  if (st->done) return;
  const int tid = threadIdx.x;
  if (tid < SREG_PART) {
    // the chain ((0 + p_0) + p_1) + ... in workgroup order; the loads of 16 partials are issued before their 16 additions
    double a = 0;
    int b = 0;
    for (; b + 16 <= nb; b += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; u++) v[u] = part[(size_t)(b + u) * SREG_PART + tid];
#pragma unroll
      for (int u = 0; u < 16; u++) a += v[u];
    }
    for (; b < nb; b++) a += part[(size_t)b * SREG_PART + tid];
    acc[tid] = a;
    if (sums) sums[tid] = a;
  }
  __syncthreads();
  if (tid != 0) return;
  double dx[6];
  sreg_step(acc, st, dx, work);
  if (dxo) for (int k = 0; k < 6; k++) dxo[k] = dx[k];
  if (st->done) {
    Eig3 e;
    if (!eig3_direct(acc[15], acc[16], acc[17], acc[18], acc[19], acc[20], e)) e = eig3_jacobi_dev(acc[15], acc[16], acc[17], acc[18], acc[19], acc[20]);
    st->rep.eig_tt[0] = e.w0; st->rep.eig_tt[1] = e.w1; st->rep.eig_tt[2] = e.w2;
  }
}

}  // namespace vba
