// Scan pre-processing that feeds K1, one thread per point:
//   down_sampling_voxel   tools.hpp:201-238    voxel-grid centroid filter (hash grid + f64 sums; the reference's running mean
//                                              in float is order dependent, the centroid is the same up to float rounding)
//   undistortion          ekf_imu.hpp:137-163  per-point motion compensation against the IMU-propagated poses
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vba_types.hpp"
#include "vba_voxel_key.hpp"   // DS_EMPTY, ds_axis_key, ds_pack, ds_hash

namespace vba {

__global__ void k_ds_clear(DsSlot *__restrict__ tab, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  DsSlot s; s.key = DS_EMPTY; s.sx = s.sy = s.sz = 0.0; s.vx = s.vy = s.vz = 0.0; s.mind = ~0ull; s.cnt = 0; s.first = 0x7fffffff; s.best = 0x7fffffff; s.pad = 0;
  tab[i] = s;
}

// point -> slot (open addressing, linear probing), sums, count, first point of the voxel
// the covariance diagonal of point i is var[vrow * i + {0, vstep, 2 vstep}]: (9, 4) for [n][9] matrices, (3, 1) for gathered diagonals
// var != nullptr: pointVar input (down_sampling_pvec, VM:39-83): double coordinates, the covariance diagonal is averaged too
// DET (deterministic mode): no f64 atomics; the sums are added by k_ds_sum_det in input order
template <bool DET>
__global__ void k_ds_insert(int n, const double *__restrict__ pnt, const double *__restrict__ var, double voxel_size, DsSlot *__restrict__ tab, int cap_mask,
                            int *__restrict__ slot_of, int vrow = 9, int vstep = 4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int dbl = var != nullptr;
  const double x = pnt[3 * (size_t)i], y = pnt[3 * (size_t)i + 1], z = pnt[3 * (size_t)i + 2];
  const unsigned long long key = ds_pack(ds_axis_key(x, voxel_size, dbl), ds_axis_key(y, voxel_size, dbl), ds_axis_key(z, voxel_size, dbl));
  unsigned int h = ds_hash(key) & cap_mask;
  for (int probe = 0; probe <= cap_mask; probe++) {          // the table has >= 2n slots: always terminates
    const unsigned long long old = atomicCAS(&tab[h].key, DS_EMPTY, key);
    if (old == DS_EMPTY || old == key) break;
    h = (h + 1) & cap_mask;
  }
  if (!DET) {
    atomicAdd(&tab[h].sx, dbl ? x : (double)(float)x);
    atomicAdd(&tab[h].sy, dbl ? y : (double)(float)y);
    atomicAdd(&tab[h].sz, dbl ? z : (double)(float)z);
    if (dbl) { const double *v = var + (size_t)vrow * (size_t)i; atomicAdd(&tab[h].vx, v[0]); atomicAdd(&tab[h].vy, v[vstep]); atomicAdd(&tab[h].vz, v[2 * vstep]); }
  }
  atomicAdd(&tab[h].cnt, 1);
  atomicMin(&tab[h].first, i);
  slot_of[i] = h;
}

// Deterministic mode: the points are grouped by voxel with a stable radix sort of (slot, index) pairs (index order survives inside a
// group); k_ds_segstart marks where each voxel's group starts (in DsSlot::pad), k_ds_sum_det lets the voxel's first point add the
// group's coordinates (and covariance diagonals) in index order, as the chains the host replays: ((0 + a_0) + a_1) + ...
__global__ void k_iota(int *__restrict__ a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = i;
}
__global__ void k_ds_segstart(int n, const unsigned int *__restrict__ skey, DsSlot *__restrict__ tab) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (j == 0 || skey[j] != skey[j - 1]) tab[skey[j]].pad = j;
}
__global__ void k_ds_sum_det(int n, const double *__restrict__ pnt, const double *__restrict__ var, const int *__restrict__ sidx, DsSlot *__restrict__ tab,
                             const int *__restrict__ slot_of, int vrow = 9, int vstep = 4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  DsSlot *s = tab + slot_of[i];
  if (s->first != i) return;
  const int dbl = var != nullptr, a = s->pad, c = s->cnt;
  double sx = 0.0, sy = 0.0, sz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
  for (int j = a; j < a + c; j++) {
    const size_t q = (size_t)sidx[j];
    const double x = pnt[3 * q], y = pnt[3 * q + 1], z = pnt[3 * q + 2];
    sx += dbl ? x : (double)(float)x; sy += dbl ? y : (double)(float)y; sz += dbl ? z : (double)(float)z;
    if (dbl) { const double *v = var + (size_t)vrow * q; vx += v[0]; vy += v[vstep]; vz += v[2 * vstep]; }
  }
  s->sx = sx; s->sy = sy; s->sz = sz;
  if (dbl) { s->vx = vx; s->vy = vy; s->vz = vz; }
}

// block-level count of "first point of its voxel" flags; blk[b] = count of block b
__global__ __launch_bounds__(256) void k_ds_count(int n, const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, int *__restrict__ blk) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  wg_count(i < n && tab[slot_of[i]].first == i, wsum, blk);
}

// exclusive scan of the block counts by one workgroup (nb <= a few thousand), in place; total -> *n_out
__global__ __launch_bounds__(256) void k_ds_scan(int nb, int *blk, int *__restrict__ n_out) {
  __shared__ int part[256];
  const int tot = wg_scan_strided(nb, blk, blk, part);
  if (threadIdx.x == 0) *n_out = tot;
}

// stable compaction in first-occurrence order; centroid rounded to float like the PCL cloud it replaces
// mode 0: centroid (down_sampling_voxel); 1: centroid + mean covariance diagonal in vout (down_sampling_pvec);
// 2: first[] receives the index of the point closest to the centroid (down_sampling_close), out = that point's voxel centroid
__global__ __launch_bounds__(256) void k_ds_emit(int n, const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, const int *__restrict__ blk,
                                                 double *__restrict__ out, int *__restrict__ count, int *__restrict__ first, double *__restrict__ vout, int mode) {
  __shared__ int wsum[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  DsSlot s;
  bool f = false;
  if (i < n) { s = tab[slot_of[i]]; f = s.first == i; }
  int tot;
  const int pos = blk[blockIdx.x] + wg_rank(f, wsum, tot);
  if (!f) return;
  const double inv = 1.0 / (double)s.cnt;
  out[3 * (size_t)pos] = (double)(float)(s.sx * inv);
  out[3 * (size_t)pos + 1] = (double)(float)(s.sy * inv);
  out[3 * (size_t)pos + 2] = (double)(float)(s.sz * inv);
  count[pos] = s.cnt;
  first[pos] = (mode == 2) ? ((s.best != 0x7fffffff) ? s.best : i) : i;
  if (mode == 1) {
    vout[3 * (size_t)pos] = (double)(float)(s.vx * inv); vout[3 * (size_t)pos + 1] = (double)(float)(s.vy * inv); vout[3 * (size_t)pos + 2] = (double)(float)(s.vz * inv);
  }
}

// down_sampling_close (tools.hpp:240-298): per voxel the point with the smallest squared distance to the (float) centroid,
// first such point in input order, only distances < 100 compete (ndis = 100, mnum = 0 at TL:281-282).
__global__ void k_ds_close_min(int n, const double *__restrict__ pnt, DsSlot *__restrict__ tab, const int *__restrict__ slot_of, double *__restrict__ dist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  DsSlot *s = tab + slot_of[i];
  const double inv = 1.0 / (double)s->cnt;
  const float cx = (float)(s->sx * inv), cy = (float)(s->sy * inv), cz = (float)(s->sz * inv);
  const double xx = (double)(cx - (float)pnt[3 * (size_t)i]), yy = (double)(cy - (float)pnt[3 * (size_t)i + 1]), zz = (double)(cz - (float)pnt[3 * (size_t)i + 2]);
  const double d = xx * xx + yy * yy + zz * zz;
  dist[i] = d;
  if (d < 100.0) atomicMin(&s->mind, (unsigned long long)__double_as_longlong(d));
}
__global__ void k_ds_close_arg(int n, DsSlot *__restrict__ tab, const int *__restrict__ slot_of, const double *__restrict__ dist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  DsSlot *s = tab + slot_of[i];
  if ((unsigned long long)__double_as_longlong(dist[i]) == s->mind) atomicMin(&s->best, i);
}

// ---------------------------------------------------------------- undistortion
// prm: [m] imu poses x 22 doubles (t, R[9], p[3], v[3], angvel[3], acc[3]), then end pose R[9] p[3], then extrinsic R[9] t[3].
__device__ __forceinline__ void undist_one(const double *__restrict__ q, const double *__restrict__ Re, const double *__restrict__ pe,
                                           const double *__restrict__ Rx, const double *__restrict__ tx, double curv, double &x, double &y, double &z) {
  const double dt = curv - q[0];
  const double *R = q + 1, *p = q + 10, *v = q + 13, *w = q + 16, *a = q + 19;
  // Exp(angvel, dt)  tools.hpp:68-84 (threshold 1e-7)
  double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double nrm = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (nrm > 1e-7) {
    const double a0 = w[0] / nrm, a1 = w[1] / nrm, a2 = w[2] / nrm, th = nrm * dt;
    const double s = sin(th), c1 = 1.0 - cos(th);
    E[0] = 1.0 + c1 * (a0 * a0 - 1.0); E[1] = -s * a2 + c1 * a0 * a1;     E[2] = s * a1 + c1 * a0 * a2;
    E[3] = s * a2 + c1 * a1 * a0;      E[4] = 1.0 + c1 * (a1 * a1 - 1.0); E[5] = -s * a0 + c1 * a1 * a2;
    E[6] = -s * a1 + c1 * a2 * a0;     E[7] = s * a0 + c1 * a2 * a1;      E[8] = 1.0 + c1 * (a2 * a2 - 1.0);
  }
  double Ri[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Ri[3 * r + c] = R[3 * r] * E[c] + R[3 * r + 1] * E[3 + c] + R[3 * r + 2] * E[6 + c];
  double T[3], b[3], u[3], g[3];
#pragma unroll
  for (int k = 0; k < 3; k++) T[k] = p[k] + v[k] * dt + a[k] * (0.5 * dt * dt) - pe[k];
#pragma unroll
  for (int k = 0; k < 3; k++) b[k] = Rx[3 * k] * x + Rx[3 * k + 1] * y + Rx[3 * k + 2] * z + tx[k];           // Lid_rot_to_IMU * P_i + offset
#pragma unroll
  for (int k = 0; k < 3; k++) u[k] = Ri[3 * k] * b[0] + Ri[3 * k + 1] * b[1] + Ri[3 * k + 2] * b[2] + T[k];   // R_i * (...) + T_ei
#pragma unroll
  for (int k = 0; k < 3; k++) g[k] = Re[k] * u[0] + Re[3 + k] * u[1] + Re[6 + k] * u[2] - tx[k];               // xc.R^T * (...) - offset
  x = (double)(float)(Rx[0] * g[0] + Rx[3] * g[1] + Rx[6] * g[2]);                                            // Lid_rot_to_IMU^T * (...)
  y = (double)(float)(Rx[1] * g[0] + Rx[4] * g[1] + Rx[7] * g[2]);
  z = (double)(float)(Rx[2] * g[0] + Rx[5] * g[1] + Rx[8] * g[2]);
}

// var_init (voxelslam.hpp:210-234) = calcBodyVar (voxelslam.hpp:180-200) + extrinsic: one thread per point.
// DEG2RAD is PCL's macro ((x) * 0.017453293), see oracle/map_oracle.hpp.
__global__ void k_var_init(int n, const double *__restrict__ pin, double *__restrict__ pout, double *__restrict__ var, const double *__restrict__ ext,
                           float range_inc, float degree_inc) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  double x = pin[3 * (size_t)p], y = pin[3 * (size_t)p + 1], z = pin[3 * (size_t)p + 2];
  if (z == 0) z = 0.0001;
  const float range = (float)sqrt(x * x + y * y + z * z);
  const float range_var = range_inc * range_inc;
  const double sn = sin((degree_inc) * 0.017453293), dv = sn * sn;
  const double nrm = sqrt(x * x + y * y + z * z);
  const double d0 = x / nrm, d1 = y / nrm, d2 = z / nrm;
  double b1x = 1, b1y = 1, b1z = -(d0 + d1) / d2;
  const double n1 = sqrt(b1x * b1x + b1y * b1y + b1z * b1z);
  b1x /= n1; b1y /= n1; b1z /= n1;
  double b2x = b1y * d2 - b1z * d1, b2y = b1z * d0 - b1x * d2, b2z = b1x * d1 - b1y * d0;   // b1 x direction
  const double n2 = sqrt(b2x * b2x + b2y * b2y + b2z * b2z);
  b2x /= n2; b2y /= n2; b2z /= n2;
  // A = range * hat(direction) * [b1 b2]
  const double r = (double)range;
  const double a1x = r * (d1 * b1z - d2 * b1y), a1y = r * (d2 * b1x - d0 * b1z), a1z = r * (d0 * b1y - d1 * b1x);
  const double a2x = r * (d1 * b2z - d2 * b2y), a2y = r * (d2 * b2x - d0 * b2z), a2z = r * (d0 * b2y - d1 * b2x);
  const double rv = (double)range_var;
  const double d[3] = {d0, d1, d2}, a1[3] = {a1x, a1y, a1z}, a2[3] = {a2x, a2y, a2z};
  double vb[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) vb[3 * i + j] = d[i] * rv * d[j] + (a1[i] * dv * a1[j] + a2[i] * dv * a2[j]);
  // extrinsic: pnt = R p + t ; var = R var R^T
  const double *R = ext;
  pout[3 * (size_t)p] = R[0] * x + R[1] * y + R[2] * z + R[9];
  pout[3 * (size_t)p + 1] = R[3] * x + R[4] * y + R[5] * z + R[10];
  pout[3 * (size_t)p + 2] = R[6] * x + R[7] * y + R[8] * z + R[11];
  double RV[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) RV[3 * i + j] = R[3 * i] * vb[j] + R[3 * i + 1] * vb[3 + j] + R[3 * i + 2] * vb[6 + j];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) var[9 * (size_t)p + 3 * i + j] = RV[3 * i] * R[3 * j] + RV[3 * i + 1] * R[3 * j + 1] + RV[3 * i + 2] * R[3 * j + 2];
}

// Points are time-sorted (voxelslam.hpp:92-95), so the backwards walk of EK:138-163 assigns point i to the last pose with
// t < curvature_i; points at or before the first pose stay untouched.  The very first point is compensated once per
// remaining pose (the `break` at EK:161 leaves the iterator on it while the outer loop continues) — kept.
__global__ void k_undistort(int n, double *__restrict__ pnt, const double *__restrict__ curv, int m, const double *__restrict__ prm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double *Re = prm + 22 * (size_t)m, *pe = Re + 9, *Rx = pe + 3, *tx = Rx + 9;
  const double cv = (double)(float)curv[i];
  int lo = 0, hi = m;                       // first pose index with t >= cv
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (prm[22 * (size_t)mid] < cv) lo = mid + 1; else hi = mid; }
  int j = lo - 1;
  if (j < 0) return;
  double x = (double)(float)pnt[3 * (size_t)i], y = (double)(float)pnt[3 * (size_t)i + 1], z = (double)(float)pnt[3 * (size_t)i + 2];
  const int jend = (i == 0) ? 0 : j;
  for (; j >= jend; j--) undist_one(prm + 22 * (size_t)j, Re, pe, Rx, tx, cv, x, y, z);
  pnt[3 * (size_t)i] = x; pnt[3 * (size_t)i + 1] = y; pnt[3 * (size_t)i + 2] = z;
}

}  // namespace vba
