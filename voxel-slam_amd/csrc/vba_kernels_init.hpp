// LiDAR-inertial initialisation (Initialization::motion_init, voxelslam.cpp:617-819): the two pieces no other entry point offers.
//   k_init_blur           the initialisation variant of motion blur (VS:506-601) over all W scans of the window in one launch:
//                         backward-propagated pose table, points pushed from last to first, drops and the repeated point 0
//   k_init_nnt_part/_fin  Σ v0 v0ᵀ over the factor store's plane normals (VS:737-741) and its eigenvalues (VS:744-745)
//   k_initw_count/_gather the initialisation window (vba_init_window_push, VS:1499-1511): order-preserving compaction of the points
//                         that down_sampling_close keeps, from the frame's stage 0 into the window at its append offset
//   k_init_walk           per scan of a resident window, what the host walk of vba_motion_init reads from the curvatures
// plus the host side of the same call: the pose-table propagation (VS:508-544) and align_gravity (VS:470-497).
#pragma once
#include <hip/hip_runtime.h>
#include "vba_eig3.hpp"
#include "vba_hostmath.hpp"
#include "vba_types.hpp"

namespace vba {

constexpr int INIT_POSE_LEN = 22;   // pose-table row: t, R[9], p[3], v[3], angvel[3], acc[3] (the layout of k_undistort's table)

// Per-scan description of one blur launch (host-built every round, one copy for the whole window).
struct InitScan {
  int pt_off, n_pts;       // raw points of the scan in the uploaded cloud
  int out_off, n_out;      // its rows in the blurred output (pvec_buf[i])
  int pose_off, n_pose;    // its rows in the pose table (descending time)
  int j_min;               // first point the walk pushes (points below it are dropped)
  int k0;                  // pose that pushes point 0 (j_min == 0), else -1; point 0 is repeated for every later pose
  int notime, conv;        // point_notime (VS:550-559) / converge_flag == 1 (var from calcBodyVar + pvec_update, VS:675-681)
  float range_inc, degree_inc;
  double R[9], p[3];       // x_buf[i]: xc of the blur and the pose of pvec_update
  double Rx[9], tx[3];     // extrin_para
  double cov6[18];         // x_buf[i].cov rot block (0,0), translation block (3,3)
};

// What the walk of motion_blur (VS:562-599) needs from one scan's curvatures: the number of leading points at or before the oldest
// pose (the walk drops them) and the curvature of point 0 (which pose pushes it).  Host-fed clouds: read on the host; resident ones:
// k_init_walk from InitWalkIn.
struct InitWalk { int j_min, pad; double cv0; };
struct InitWalkIn { long long off; int n, pad; double t_last; };   // the scan's rows in the window (n = 0: no walk), oldest pose time

// ---------------------------------------------------------------- host side
// Backward IMU propagation of motion_blur (VS:508-544) from xc = state_c (biases of state_l), m samples rows [t, gyr(3), acc(3)]:
// m - 1 pose-table rows in push order (time descending).
inline int init_imu_poses(int m, const double *imu, const double *xc, const double *xl, double beg_time, double scale_gravity, double *out) {
  if (m < 2) return 0;
  const double *bg = xl + 16, *ba = xl + 19, *g = xc + 22;
  double R[9], pos[3], vel[3];
  for (int k = 0; k < 9; k++) R[k] = xc[1 + k];
  for (int k = 0; k < 3; k++) { pos[k] = xc[10 + k]; vel[k] = xc[13 + k]; }
  int row = 0;
  for (int it = m - 1; it > 0; it--, row++) {
    const double *head = imu + 7 * (size_t)(it - 1), *tail = imu + 7 * (size_t)it;
    double w[3], a[3], acc_imu[3], E[9], Rn[9];
    for (int k = 0; k < 3; k++) {
      w[k] = 0.5 * (head[1 + k] + tail[1 + k]);
      a[k] = 0.5 * (head[4 + k] + tail[4 + k]);
    }
    for (int k = 0; k < 3; k++) { w[k] -= bg[k]; a[k] = a[k] * scale_gravity - ba[k]; }
    const double dt = head[0] - tail[0];
    vbh::so3_exp_dt(w, dt, E);
    vbh::m3_vec(R, a, acc_imu);
    for (int k = 0; k < 3; k++) acc_imu[k] += g[k];
    for (int k = 0; k < 3; k++) pos[k] = pos[k] + vel[k] * dt + 0.5 * acc_imu[k] * dt * dt;
    for (int k = 0; k < 3; k++) vel[k] = vel[k] + acc_imu[k] * dt;
    vbh::m3_mul(R, E, Rn);
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
    double *o = out + (size_t)INIT_POSE_LEN * row;
    o[0] = head[0] - beg_time;
    for (int k = 0; k < 9; k++) o[1 + k] = R[k];
    for (int k = 0; k < 3; k++) { o[10 + k] = pos[k]; o[13 + k] = vel[k]; o[16 + k] = w[k]; o[19 + k] = acc_imu[k]; }
  }
  return row;
}

// Initialization::align_gravity (VS:470-497) on n states [25]: rotation taking g of state 0 onto ±z (Eigen::AngleAxisd::toRotationMatrix).
inline void init_align_gravity(int n, double *xs) {
  if (n < 1) return;
  const double *g0 = xs + 22;
  const double gn = vbh::norm3(g0);
  const double n0[3] = {g0[0] / gn, g0[1] / gn, g0[2] / gn};
  const double n1[3] = {0.0, 0.0, n0[2] < 0 ? -1.0 : 1.0};
  double ax[3] = {n0[1] * n1[2] - n0[2] * n1[1], n0[2] * n1[0] - n0[0] * n1[2], n0[0] * n1[1] - n0[1] * n1[0]};
  const double rnorm = vbh::norm3(ax);
  for (int k = 0; k < 3; k++) ax[k] = ax[k] / rnorm;
  const double ang = std::asin(rnorm), s = std::sin(ang), c = std::cos(ang);
  const double sa[3] = {s * ax[0], s * ax[1], s * ax[2]}, ca[3] = {(1.0 - c) * ax[0], (1.0 - c) * ax[1], (1.0 - c) * ax[2]};
  double rot[9];
  double t = ca[0] * ax[1]; rot[1] = t - sa[2]; rot[3] = t + sa[2];
  t = ca[0] * ax[2];        rot[2] = t + sa[1]; rot[6] = t - sa[1];
  t = ca[1] * ax[2];        rot[5] = t - sa[0]; rot[7] = t + sa[0];
  rot[0] = ca[0] * ax[0] + c; rot[4] = ca[1] * ax[1] + c; rot[8] = ca[2] * ax[2] + c;
  double gr[3];
  vbh::m3_vec(rot, g0, gr);
  const double p0[3] = {xs[10], xs[11], xs[12]};
  for (int i = 0; i < n; i++) {
    double *x = xs + (size_t)VBA_STATE_LEN * i, d[3], o[3], Rn[9];
    for (int k = 0; k < 3; k++) d[k] = x[10 + k] - p0[k];
    vbh::m3_vec(rot, d, o);
    for (int k = 0; k < 3; k++) x[10 + k] = o[k] + p0[k];
    vbh::m3_mul(rot, x + 1, Rn);
    for (int k = 0; k < 9; k++) x[1 + k] = Rn[k];
    vbh::m3_vec(rot, x + 13, o);
    for (int k = 0; k < 3; k++) x[13 + k] = o[k];
    for (int k = 0; k < 3; k++) x[22 + k] = gr[k];
  }
}

// ---------------------------------------------------------------- device side
// One thread per OUTPUT row of the window: the scan from the output offsets, the point and its pose from the push order of the
// reference walk.  Rows [0, n_pts - j_min) are points n_pts-1 .. j_min, each compensated with the FIRST pose (time descending) whose
// time is below its curvature; rows after them repeat point 0 with poses k0+1, k0+2, ... (the `break` at VS:597-598 leaves the
// iterator on point 0 while the pose loop goes on).  No atomics: the row index alone decides where a point goes.
__global__ __launch_bounds__(256) void k_init_blur(int W, int n_out, const InitScan *__restrict__ scans, const double *__restrict__ poses,
                                                   const double *__restrict__ pnt, const double *__restrict__ curv, double *__restrict__ pb,
                                                   double *__restrict__ var) {
#pragma clang fp contract(off)      // the reference's operation order, separately rounded
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_out) return;
  int i = 0;
  while (i + 1 < W && scans[i + 1].out_off <= o) i++;
  const InitScan &S = scans[i];
  const int s = o - S.out_off;
  double x, y, z;
  const double *Rx = S.Rx, *tx = S.tx;
  if (S.notime) {                                   // VS:550-559: the extrinsic alone, input order
    const double *P = pnt + 3 * (size_t)(S.pt_off + s);
    x = Rx[0] * P[0] + Rx[1] * P[1] + Rx[2] * P[2] + tx[0];
    y = Rx[3] * P[0] + Rx[4] * P[1] + Rx[5] * P[2] + tx[1];
    z = Rx[6] * P[0] + Rx[7] * P[1] + Rx[8] * P[2] + tx[2];
  } else {
    const double *tab = poses + (size_t)INIT_POSE_LEN * S.pose_off;
    const int n_main = S.n_pts - S.j_min;
    int j, k;
    if (s < n_main) {
      j = S.n_pts - 1 - s;
      const double cv = curv[S.pt_off + j];
      int lo = 0, hi = S.n_pose;                    // first pose with t < cv (times descend)
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (tab[(size_t)INIT_POSE_LEN * mid] < cv) hi = mid; else lo = mid + 1; }
      k = lo < S.n_pose ? lo : S.n_pose - 1;        // (the host checked the deque times ascend: lo < n_pose holds)
    } else {
      j = 0;
      k = S.k0 + 1 + (s - n_main);
    }
    const double *q = tab + (size_t)INIT_POSE_LEN * k;
    const double *R = q + 1, *p = q + 10, *v = q + 13, *w = q + 16, *a = q + 19;
    const double dt = curv[S.pt_off + j] - q[0];
    double E[9], Ri[9];
    vbh::so3_exp_dt(w, dt, E);
    vbh::m3_mul(R, E, Ri);
    double T[3], b[3], u[3];
    for (int c = 0; c < 3; c++) T[c] = p[c] + v[c] * dt + 0.5 * a[c] * dt * dt - S.p[c];
    const double *P = pnt + 3 * (size_t)(S.pt_off + j);
    for (int c = 0; c < 3; c++) b[c] = Rx[3 * c] * P[0] + Rx[3 * c + 1] * P[1] + Rx[3 * c + 2] * P[2] + tx[c];
    for (int c = 0; c < 3; c++) u[c] = Ri[3 * c] * b[0] + Ri[3 * c + 1] * b[1] + Ri[3 * c + 2] * b[2] + T[c];
    x = S.R[0] * u[0] + S.R[3] * u[1] + S.R[6] * u[2];   // xc.R^T (...)
    y = S.R[1] * u[0] + S.R[4] * u[1] + S.R[7] * u[2];
    z = S.R[2] * u[0] + S.R[5] * u[1] + S.R[8] * u[2];
  }
  double *vo = var + 9 * (size_t)o;
  if (!S.conv) {                                    // pv.var = I (VS:547)
    for (int k = 0; k < 9; k++) vo[k] = (k % 4 == 0) ? 1.0 : 0.0;
  } else {
    // calcBodyVar (VH:180-200) on the compensated body point (no extrinsic), then pvec_update (VH:242-265) with x_buf[i]
    if (z == 0) z = 0.0001;
    const float range = (float)sqrt(x * x + y * y + z * z);
    const float range_var = S.range_inc * S.range_inc;
    const double sn = sin((S.degree_inc) * 0.017453293), dv = sn * sn;
    const double nrm = sqrt(x * x + y * y + z * z);
    const double d0 = x / nrm, d1 = y / nrm, d2 = z / nrm;
    double b1x = 1, b1y = 1, b1z = -(d0 + d1) / d2;
    const double n1 = sqrt(b1x * b1x + b1y * b1y + b1z * b1z);
    b1x /= n1; b1y /= n1; b1z /= n1;
    double b2x = b1y * d2 - b1z * d1, b2y = b1z * d0 - b1x * d2, b2z = b1x * d1 - b1y * d0;
    const double n2 = sqrt(b2x * b2x + b2y * b2y + b2z * b2z);
    b2x /= n2; b2y /= n2; b2z /= n2;
    const double r = (double)range;
    const double a1[3] = {r * (d1 * b1z - d2 * b1y), r * (d2 * b1x - d0 * b1z), r * (d0 * b1y - d1 * b1x)};
    const double a2[3] = {r * (d1 * b2z - d2 * b2y), r * (d2 * b2x - d0 * b2z), r * (d0 * b2y - d1 * b2x)};
    const double rv = (double)range_var, d[3] = {d0, d1, d2};
    double vb[9];
    for (int ii = 0; ii < 3; ii++)
      for (int jj = 0; jj < 3; jj++) vb[3 * ii + jj] = d[ii] * rv * d[jj] + (a1[ii] * dv * a1[jj] + a2[ii] * dv * a2[jj]);
    var_world(S.R, S.cov6, x, y, z, vb, vo);
  }
  pb[3 * (size_t)o] = x; pb[3 * (size_t)o + 1] = y; pb[3 * (size_t)o + 2] = z;
}

// ---------------------------------------------------------------- initialisation window
// The point that down_sampling_close keeps of a voxel, from the table ds_core leaves in mode 2: `best`, or `first` when no distance
// competed (TL:281-295; what k_ds_emit writes to first[] in mode 2).  Point i is kept iff it is that point of its own voxel, so the
// mark is a predicate of the table and no pass writes it.
__device__ __forceinline__ int initw_kept(const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, int i) {
  const DsSlot *s = tab + slot_of[i];
  const int b = s->best;
  return ((b != 0x7fffffff) ? b : s->first) == i;
}
// kept points per 256-point block; k_ds_scan turns blk into the exclusive scan and the total
__global__ __launch_bounds__(256) void k_initw_count(int n, const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, int *__restrict__ blk) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  wg_count(i < n && initw_kept(tab, slot_of, i), wsum, blk);
}
// Kept point i goes to row row0 + (kept points below i): ascending stage-0 index, i.e. ascending curvature with ties in message
// order.  The row is copied as it is (xyz and curvature, bit for bit).  No atomics.
__global__ __launch_bounds__(256) void k_initw_gather(int n, const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, const int *__restrict__ blk,
                                                      const double *__restrict__ pnt, const double *__restrict__ curv, double *__restrict__ wpnt,
                                                      double *__restrict__ wcurv, long long row0) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool f = i < n && initw_kept(tab, slot_of, i);
  int tot;
  const int pos = blk[blockIdx.x] + wg_rank(f, wsum, tot);
  if (!f) return;
  const long long r = row0 + (long long)pos;
  wpnt[3 * r] = pnt[3 * (size_t)i]; wpnt[3 * r + 1] = pnt[3 * (size_t)i + 1]; wpnt[3 * r + 2] = pnt[3 * (size_t)i + 2];
  wcurv[r] = curv[i];
}
// One thread per scan: curvature ascends, so the points the walk drops are a prefix, found by binary search (first row with
// curv > t_last).
__global__ __launch_bounds__(64) void k_init_walk(int W, const InitWalkIn *__restrict__ in, const double *__restrict__ curv, InitWalk *__restrict__ out) {
  const int i = threadIdx.x;
  if (i >= W) return;
  const int n = in[i].n;
  const double *cv = curv + in[i].off, t = in[i].t_last;
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (cv[mid] <= t) lo = mid + 1; else hi = mid; }
  InitWalk o; o.j_min = lo; o.pad = 0; o.cv0 = n > 0 ? cv[0] : 0.0;
  out[i] = o;
}

// Σ v0 v0ᵀ (VS:737-741), first level: workgroup b sums voxels b*256 + t, (b + nb)*256 + t, ... per lane, then the wave sums (DPP, fixed
// tree) and the four waves in order through LDS -> part[b][6] (upper triangle xx xy xz yy yz zz).  nb depends on the voxel count only.
constexpr int INIT_NNT_WG = 64;     // workgroups of the first level (at most)
__global__ __launch_bounds__(256) void k_init_nnt_part(FactorView f, int nvox, double *__restrict__ part) {
  __shared__ double ws[4][6];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int v = blockIdx.x * 256 + threadIdx.x; v < nvox; v += gridDim.x * 256) {
    const double x = f.eigvec[(size_t)0 * f.vs + v], y = f.eigvec[(size_t)3 * f.vs + v], z = f.eigvec[(size_t)6 * f.vs + v];   // column 0
    acc[0] += x * x; acc[1] += x * y; acc[2] += x * z; acc[3] += y * y; acc[4] += y * z; acc[5] += z * z;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < 6; k++) {
    const double s = wave_sum_to_lane63(acc[k]);
    if (lane == 63) ws[wv][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6) part[6 * (size_t)blockIdx.x + threadIdx.x] = ((ws[0][threadIdx.x] + ws[1][threadIdx.x]) + ws[2][threadIdx.x]) + ws[3][threadIdx.x];
}
// Second level: one wave sums the nb partials (lane l takes l, l + 64, ...), then the 3x3 eigenvalues (SelfAdjointEigenSolver at
// VS:744-745): out = [w0, w1, w2, nnt upper triangle (6)].
__global__ __launch_bounds__(64) void k_init_nnt_fin(int nb, const double *__restrict__ part, double *__restrict__ out) {
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < nb; b += 64)
    for (int k = 0; k < 6; k++) acc[k] += part[6 * (size_t)b + k];
  for (int k = 0; k < 6; k++) acc[k] = wave_sum_to_lane63(acc[k]);
  if (threadIdx.x != 63) return;
  Eig3 e;
  if (!eig3_direct(acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], e)) e = eig3_jacobi_dev(acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]);
  out[0] = e.w0; out[1] = e.w1; out[2] = e.w2;
  for (int k = 0; k < 6; k++) out[3 + k] = acc[k];
}

}  // namespace vba
