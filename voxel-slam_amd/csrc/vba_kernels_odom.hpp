// The device-resident iterated EKF of the odometry scan-to-map update (VOXEL_SLAM::lio_state_estimation,
// voxelslam.cpp:962-1098):
//   k_odom_match_dev   the point loop (odom_match_body, vba_kernels_map.hpp) with the pose and the covariance blocks read from the
//                      device state of the loop
//   k_odom_update      ONE workgroup: sums the workgroup partials in a fixed order and runs one iteration of vba_odom_ekf.hpp on them
//   k_odom_sums        ONE workgroup: the same sums, stored (the diagnostic entry vba_debug_odom_sums)
// Both read the state's `done` flag first and return at once when the stop rule has fired, so the host queues all four iterations
// without waiting for any of them (the pattern of LmDev::stop in vba_kernels_lm.hpp).  No atomics.  Included after vba_kernels_map.hpp.
#pragma once
#include "vba_odom_ekf.hpp"

namespace vba {

typedef __attribute__((address_space(3))) double odom_lds_f64;

__global__ __launch_bounds__(256) void k_odom_match_dev(MapView m, MapParams P, const vbh::OdomEkf *__restrict__ S, int n,
                                                        const double *__restrict__ pts, const double *__restrict__ var,
                                                        double *__restrict__ partial) {
  if (__builtin_amdgcn_readfirstlane(S->done)) return;
  OdomState X;
#pragma unroll
  for (int k = 0; k < 9; k++) { X.R[k] = odom_uniform(S->R[k]); X.rot_var[k] = odom_uniform(S->rot_var[k]); X.tsl_var[k] = odom_uniform(S->tsl_var[k]); }
#pragma unroll
  for (int k = 0; k < 3; k++) X.t[k] = odom_uniform(S->t[k]);
  odom_match_body(m, P, X, n, pts, var, partial);
}

struct OdomWgSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };

// Column c of the nb x 34 partials is summed by the seven lanes c, c + 34, ..., c + 204: lane t adds the elements t, t + 238,
// t + 476, ... of the flat array (rows t / 34, t / 34 + 7, ... of its column: consecutive lanes read consecutive doubles) in that
// order, then lane c adds the seven group sums in group order.  The order depends on nb alone.
static constexpr int ODOM_RED_LANES = 7 * 34;
// That reduction, by the first 238 lanes of one 256-lane workgroup: rd is the workgroup's ODOM_RED_LANES doubles of LDS, out[0..33]
// (LDS or global memory) receives the sums from lanes 0..33.  One barrier inside, none after the store.  Additions only, and they are
// not to be fused with anything a caller computes next to them.
template <class OP>
__device__ __forceinline__ void odom_sum_partials(const double *__restrict__ partial, int nb, odom_lds_f64 *rd, OP out) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t < ODOM_RED_LANES) {
    const size_t tot = (size_t)nb * 34;
    double s = 0.0;
    for (size_t i = t; i < tot; i += ODOM_RED_LANES) s += partial[i];
    rd[t] = s;
  }
  __syncthreads();
  if (t < 34) {
    double s = rd[t];
    for (int g = 1; g < 7; g++) s += rd[t + 34 * g];
    out[t] = s;
  }
}
// kd: the stop rule of the kd-tree variant (vba_odom_ekf.hpp), whose loop in vba_odom.hip launches this kernel too.
__global__ __launch_bounds__(256) void k_odom_update(vbh::OdomEkf *S, const double *__restrict__ partial, int nb, int iter, int kd) {
#pragma clang fp contract(off)
  __shared__ double wsm[vbh::OE_WORK];
  __shared__ double red[ODOM_RED_LANES];
  if (__builtin_amdgcn_readfirstlane(S->done)) return;
  odom_lds_f64 *w = (odom_lds_f64 *)wsm;
  odom_sum_partials(partial, nb, (odom_lds_f64 *)red, w + vbh::OE_S34);
  __syncthreads();
  vbh::odom_ekf_iterate(w, S, iter, threadIdx.x, 256, OdomWgSync(), kd);
}
// The sums alone, as k_odom_update forms them, stored for vba_debug_odom_sums: ONE workgroup of 256 lanes, whatever S->done says.
__global__ __launch_bounds__(256) void k_odom_sums(const double *__restrict__ partial, int nb, double *__restrict__ sums /*[34]*/) {
  __shared__ double red[ODOM_RED_LANES];
  odom_sum_partials(partial, nb, (odom_lds_f64 *)red, sums);
}

}  // namespace vba
