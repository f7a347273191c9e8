// The odometry state resident in HBM from one scan to the next: a block [state 25 | P 225] that
//   k_imu_propagate     ONE workgroup: IMUEKF::motion_blur's propagation (vba_imu_ekf.hpp, ekf_imu.hpp:54-123) on the block, the pose
//                       table and end_pose written where k_undistort reads them
//   k_odom_begin_dev    ONE workgroup: the image of a scan-to-map update (vbh::odom_ekf_begin) built from the block, P^-1 by
//                       inverse15_pplu, in place of the host inverse and the image upload
//   k_odom_commit_dev   x_curr and P_out of the image back into the block after the loop
//   k_odom_state_pose   the map's pose image poses[0..12) and [16..34) (pose, rot_var, tsl_var) from the block, in place of the pinned
//                       ring upload of map_cut_voxel
//   k_odom_begin_kd_dev the same for a kd-tree update of the initialisation odometry: P^-1 / 1000, refind = 1
//   k_odom_state_export the published scan of pub_localtraj (VS:37-45): world = x_curr.R p + x_curr.p in kf_apply's order with the
//                       pose read from the block, one 16-byte record x y z intensity per lane
// read and rewrite.  No atomics.  Compiled by vba_odom.hip.
#pragma once
#include "vba_common.hpp"
#include "vba_imu_ekf.hpp"

namespace vba {

typedef __attribute__((address_space(3))) double imu_lds_f64;
struct ImuWgSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };

static constexpr int ODOM_STATE_BLOCK = 256;       // doubles: state 25 | P 225 | 6 unused

// up: [parameter block IE_PRM | imu m x 7]; blk: the state block; tab: the pose table, end_pose behind its `rows` rows (the host's
// count of the live intervals, which is the one the propagation returns: comparisons of the same doubles)
__global__ __launch_bounds__(256) void k_imu_propagate(int m, int rows, const double *up, double *blk, double *tab) {
#pragma clang fp contract(off)
  __shared__ double wsm[vbh::IE_WORK];
  vbh::imu_ekf_propagate((imu_lds_f64 *)wsm, m, up + vbh::IE_PRM, up, (vbh::State *)blk, blk + 25, tab, tab + (size_t)vbh::IE_ROW * rows, threadIdx.x, 256,
                         ImuWgSync());
}

// KD: the image of a kd-tree update (odom_image_begin with kd = true): cov_inv = P^-1 / 1000 entry by entry, a division as at VS:1135 /
// VS:1207, and the first iteration searching
template <bool KD>
__device__ __forceinline__ void odom_begin_body(vbh::OdomEkf *S, const double *blk, imu_lds_f64 *wsm) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  unsigned int *z = (unsigned int *)S;
  for (int e = t; e < (int)(sizeof(vbh::OdomEkf) / 4); e += 256) z[e] = 0u;
  __syncthreads();
  const double *P = blk + 25;
  double *xp = (double *)&S->x_prop, *xc = (double *)&S->x_curr;
  for (int e = t; e < 25; e += 256) xp[e] = xc[e] = blk[e];
  for (int e = t; e < 225; e += 256) S->P[e] = S->P_out[e] = P[e];
  for (int e = t; e < 9; e += 256) {                                                            // VS:999-1000
    const int r = e / 3, k = e % 3;
    S->R[e] = blk[1 + e]; S->rot_var[e] = P[r * 15 + k]; S->tsl_var[e] = P[(3 + r) * 15 + 3 + k];
  }
  for (int e = t; e < 3; e += 256) S->t[e] = blk[10 + e];
  if (KD && t == 0) S->refind = 1;
  vbh::inverse15_pplu(wsm, P, S->cov_inv, t, 256, ImuWgSync());
  if (KD)                                                                                       // (the inverse ends in a barrier)
    for (int e = t; e < 225; e += 256) S->cov_inv[e] = S->cov_inv[e] / 1000;
}
__global__ __launch_bounds__(256) void k_odom_begin_dev(vbh::OdomEkf *S, const double *blk) {
  __shared__ double wsm[vbh::INV15_WORK];
  odom_begin_body<false>(S, blk, (imu_lds_f64 *)wsm);
}
__global__ __launch_bounds__(256) void k_odom_begin_kd_dev(vbh::OdomEkf *S, const double *blk) {
  __shared__ double wsm[vbh::INV15_WORK];
  odom_begin_body<true>(S, blk, (imu_lds_f64 *)wsm);
}

__global__ __launch_bounds__(256) void k_odom_commit_dev(const vbh::OdomEkf *S, double *blk) {
  const int t = threadIdx.x;
  const double *xc = (const double *)&S->x_curr;
  if (t < 25) blk[t] = xc[t];
  if (t < 225) blk[25 + t] = S->P_out[t];
}

__global__ __launch_bounds__(64) void k_odom_state_pose(const double *blk, double *poses) {
  const int t = threadIdx.x;
  if (t < 12) poses[t] = blk[1 + t];
  if (t < 9) {
    const int r = t / 3, k = t % 3;
    poses[16 + t] = blk[25 + r * 15 + k]; poses[25 + t] = blk[25 + (3 + r) * 15 + 3 + k];
  }
}

// one point per lane; the pose is the block's x_curr, wave-uniform; every product and sum rounded on its own (kf_apply), each
// coordinate narrowed once
__global__ __launch_bounds__(256) void k_odom_state_export(int n, const double *__restrict__ pts, const double *__restrict__ blk, float intensity,
                                                           float4 *__restrict__ out) {
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = odom_uniform(blk[1 + k]);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  kf_apply(T, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], x, y, z);
  out[i] = make_float4((float)x, (float)y, (float)z, intensity);
}

}  // namespace vba
