// Pose-graph optimisation on the device (vba_pgo_optimize): the ISAM2 schedule of build_graph + update() x U
// (VS:2078-2156, VS:2550-2561, VS:2769-2777) as U Gauss-Newton solves with per-node relinearisation gating.
//   * k_pgo_linearize  one thread per factor (between or prior): whitened residual, both 6x6 Jacobians, J^T Lambda J blocks,
//                      J^T Lambda e and the cost into the factor's slot;
//   * k_pgo_cost       one workgroup sums the factor costs in a fixed tree (bit-identical run to run);
//   * k_pgo_assemble   one thread per Hessian block: the block's factor contributions in CSR (factor) order, no atomics;
//   * k_pgo_seg_elim   one thread per segment (a maximal run of prior-free nodes with <= 2 neighbours): block-tridiagonal
//                      elimination along the run, 6x6 LDL^T in registers; the Schur complement goes to per-segment slots;
//   * k_pgo_skel_fill / k_pgo_skel_scatter  the dense skeleton system in the layout of k_bigl_panel / k_bigl_update (identity
//                      order, no gauge rows, no damping), each skeleton block summing its segment slots in a fixed order;
//   * k_pgo_pivots     a pivot <= 0 or not finite marks the system singular (k_bigl_panel itself skips zero pivots);
//   * k_bigl_bs_*      back substitution through the dense factor on the device; k_pgo_skel_dx / k_pgo_seg_back then solve
//                      the segments backwards; k_pgo_relin gates, retracts and counts per node.
// The arithmetic of every kernel (the chart, a factor, a block, a segment) is in vba_pgo_math.hpp, which also compiles for the host.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "vba_pgo_math.hpp"

namespace vba {

__global__ __launch_bounds__(256) void k_pgo_linearize(PgoView v) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= v.F) return;
  pgo_linearize_factor(v, f);
}

__global__ __launch_bounds__(256) void k_pgo_cost(PgoView v, int u) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int f = threadIdx.x; f < v.F; f += 256) acc += v.slot[(size_t)f * PGO_SLOT + 120];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) v.cost[u] = red[0];
}

__global__ __launch_bounds__(256) void k_pgo_assemble(PgoView v) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= v.NB) return;
  pgo_assemble_block(v, b);
}

__global__ __launch_bounds__(64) void k_pgo_seg_elim(PgoView v) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= v.S) return;
  if (!pgo_seg_elim(v, s)) *v.status = PGO_SINGULAR;
}

__global__ __launch_bounds__(256) void k_pgo_skel_fill(PgoView v) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long tot = (long long)(v.NP + 1) * v.NP;
  if (t >= tot) return;
  const int i = (int)(t / v.NP), j = (int)(t - (long long)i * v.NP);
  v.Ab[(size_t)i * v.ld + j] = (i == j && j >= 6 * v.K) ? 1.0 : 0.0;   // identity on the padding, zero elsewhere
}

__global__ __launch_bounds__(256) void k_pgo_skel_scatter(PgoView v) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= v.NSB) return;
  pgo_skel_scatter_block(v, b);
}

__global__ __launch_bounds__(256) void k_pgo_pivots(PgoView v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * v.K) return;
  const double d = v.Ab[(size_t)i * v.ld + i];
  if (!(d > 0.0) || !isfinite(d)) *v.status = PGO_SINGULAR;
}

__global__ __launch_bounds__(256) void k_pgo_skel_dx(PgoView v) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.K) return;
  const double *z = v.Ab + (size_t)v.NP * v.ld + 6 * p;
  for (int k = 0; k < 6; k++) v.dx[(size_t)v.skel_node[p] * 6 + k] = z[k];
}

__global__ __launch_bounds__(64) void k_pgo_seg_back(PgoView v) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= v.S) return;
  pgo_seg_back(v, s);
}

// After update u: max |delta|_inf into mx[u]; then either the gate of update u + 1 (retract where |delta|_inf >= thr, count) or,
// after the last update, theta (+) delta for every node (calculateEstimate).
__global__ __launch_bounds__(256) void k_pgo_relin(PgoView v, int u) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= v.n) return;
  const double *d = v.dx + (size_t)k * 6;
  double m = 0.0;
  for (int q = 0; q < 6; q++) m = fmax(m, fabs(d[q]));
  if (m != m) m = INFINITY;
  atomicMax(&v.mx[u], (unsigned long long)__double_as_longlong(m));
  const bool last = u + 1 == v.U;
  if (!last && !(m >= v.thr)) return;
  pgo_retract(d, v.theta + (size_t)k * 12);
  if (!last) atomicAdd(&v.cnt[u + 1], 1);
}

}  // namespace vba
