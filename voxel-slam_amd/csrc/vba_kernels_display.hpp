// The display export of the live local voxel map: OctoTree::tras_display (VM:1765-1827) over every root, the planar
// leaves as records and the window's points that sit in them at the caller's poses.  Count / k_det_scan / write, as every stable
// compaction of the map; the map is only read.  Compiled by vba_map_display.hip alone.
#pragma once
#include "vba_types.hpp"
#include "vba_common.hpp"

namespace vba {

// the window's frames laid end to end in 256-point workgroups: frame i owns workgroups [bb[i], bb[i + 1]) and reads ring slot slot[i]
struct DispFrames {
  int win_count;
  int slot[VBA_MAX_WIN], npts[VBA_MAX_WIN], bb[VBA_MAX_WIN + 1];
};

enum { DISP_N_PLANES = 0, DISP_N_POINTS = 1, DISP_FRAME0 = 2, DISP_CNT_N = DISP_FRAME0 + VBA_MAX_WIN + 1 };

// a live leaf (the rows of k_dump_leaves: not internal, not pruned, an octant that was touched) with plane.is_plane (VM:1780).  Node
// storage beyond the true node count is zero-filled, so an upper bound of the count as nn flags nothing more.
__device__ __forceinline__ bool disp_planar(const MapView &m, int id, int nn) {
  if (id >= nn) return false;
  if (m.nstate[id] != 0 || m.nlayer[id] < 0) return false;
  if (m.nlayer[id] > 0 && !m.f_touched[id]) return false;
  return m.f_plane[id] != 0;
}

// PASS 0: planar leaves per workgroup -> blk.  PASS 1 (blk scanned): nidx[node] = rank of the leaf in node-id order, or -1
template <int PASS>
__global__ __launch_bounds__(256) void k_disp_nodes(MapView m, int nn, int *__restrict__ blk, int *__restrict__ nidx) {
  __shared__ int wsum[4];
  const int id = blockIdx.x * 256 + threadIdx.x;
  const bool f = disp_planar(m, id, nn);
  int tot;
  const int r = wg_rank(f, wsum, tot);
  if (PASS == 0) { if (threadIdx.x == 0) blk[blockIdx.x] = tot; return; }
  if (id < nn) nidx[id] = f ? blk[blockIdx.x] + r : -1;
}

// one lane per planar leaf: the record is formed fresh from pcr_add as VM:1771-1773 does (center = v / N, cov = P / N - center center^T,
// the reference's operations, uncontracted), each double narrowed to float once.  64 bytes = four 16-byte stores, then the key.
__global__ __launch_bounds__(256) void k_disp_planes(MapView m, int nn, const int *__restrict__ nidx, int n_planes, float4 *__restrict__ planes,
                                                     long long *__restrict__ key) {
#pragma clang fp contract(off)
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= nn) return;
  const int i = nidx[id];
  if (i < 0 || i >= n_planes) return;
  const size_t cp = (size_t)m.cap;
  if (planes) {
    const double *a = m.nadd + (size_t)id * 10;
    const double N = a[9];
    const double cx = a[6] / N, cy = a[7] / N, cz = a[8] / N;
    double w0, w1, w2, V[9];
    eig3_sym_dev(a[0] / N - cx * cx, a[1] / N - cy * cx, a[2] / N - cz * cx, a[3] / N - cy * cy, a[4] / N - cz * cy, a[5] / N - cz * cz, w0, w1, w2, V);
    const double nfixN = m.nfix[(size_t)id * 10 + 9];
    float4 *o = planes + (size_t)i * 4;
    o[0] = make_float4((float)cx, (float)cy, (float)cz, 2.0f * m.nql[id]);
    o[1] = make_float4((float)V[0], (float)V[3], (float)V[6], (float)m.nlayer[id]);
    o[2] = make_float4((float)sqrt(fmax(w0, 0.0)), (float)sqrt(fmax(w1, 0.0)), (float)sqrt(fmax(w2, 0.0)), (float)N);
    o[3] = make_float4((float)m.ncenter[id], (float)m.ncenter[cp + id], (float)m.ncenter[2 * cp + id], (float)(N - nfixN));
  }
  if (key) {
    long long kx, ky, kz;
    unpack_key(m.nkey[id], kx, ky, kz);
    long long *k = key + (size_t)i * 5;
    k[0] = kx; k[1] = ky; k[2] = kz; k[3] = m.nlayer[id]; k[4] = m.npath[id];
  }
}

// The grids below run over (frame, 256 points) with the frames end to end; inv holds one int per thread of that grid.
__device__ __forceinline__ int disp_frame_of(const DispFrames &F, int b) {
  int fr = 0;
  while (fr + 1 < F.win_count && F.bb[fr + 1] <= b) fr++;
  return fr;
}

// pleaf tags the slot's ORDERED storage (the points grouped by insertion leaf, perm[position] = index in the scan), and the order of the
// groups is drawn by atomics in every mode.  The export runs in the scan's own order instead, which is the same in every run:
// inv[index in the scan] = position, -1 (the fill) for a point that holds no position.
__global__ __launch_bounds__(256) void k_disp_inverse(MapView m, DispFrames F, int *__restrict__ inv) {
  const int b = blockIdx.x, fr = disp_frame_of(F, b);
  const int pos = (b - F.bb[fr]) * 256 + threadIdx.x;
  if (pos >= F.npts[fr]) return;
  const size_t at = (size_t)F.slot[fr] * (size_t)m.max_pts + (size_t)pos;
  if (m.pleaf[at] < 0) return;
  const int p = m.perm[at];
  if (p >= 0 && p < F.npts[fr]) inv[(size_t)F.bb[fr] * 256 + p] = pos;
}

// A point is kept when its leaf is planar, with `all` when it has a leaf at all.  PASS 0: kept points per workgroup -> blk.  PASS 1 (blk
// scanned): record = x y z (poses[frame] applied in kf_apply's order, each coordinate narrowed once) and the frame index as intensity,
// one 16-byte store; pop = the leaf's plane index or -1.
template <int PASS>
__global__ __launch_bounds__(256) void k_disp_points(MapView m, DispFrames F, int nn, const int *__restrict__ nidx, const int *__restrict__ inv, int all,
                                                     int *__restrict__ blk, const double *__restrict__ poses, float4 *__restrict__ xyzi, int *__restrict__ pop) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, fr = disp_frame_of(F, b);
  const int p = (b - F.bb[fr]) * 256 + threadIdx.x;
  const size_t base = (size_t)F.slot[fr] * (size_t)m.max_pts;
  bool f = false;
  int pi = -1;
  if (p < F.npts[fr]) {
    const int pos = inv[(size_t)b * 256 + threadIdx.x];
    const int leaf = pos >= 0 && pos < F.npts[fr] ? m.pleaf[base + pos] : -1;
    if (leaf >= 0) { pi = leaf < nn ? nidx[leaf] : -1; f = all || pi >= 0; }
  }
  int tot;
  const int r = wg_rank(f, wsum, tot);
  if (PASS == 0) { if (threadIdx.x == 0) blk[b] = tot; return; }
  if (!f) return;
  const size_t j = (size_t)blk[b] + (size_t)r;
  const double *q = m.px + (base + (size_t)p) * 3;
  double x, y, z;
  kf_apply(poses + 12 * fr, q[0], q[1], q[2], x, y, z);
  xyzi[j] = make_float4((float)x, (float)y, (float)z, (float)fr);
  if (pop) pop[j] = pi;
}

// frame_begin from the scanned workgroup counts: the offset of a frame's first workgroup, the total for the frames behind the last one
__global__ void k_disp_frames(const int *__restrict__ blk, int nb, DispFrames F, int *__restrict__ cnt) {
  const int i = threadIdx.x;
  if (i <= F.win_count) cnt[DISP_FRAME0 + i] = (i < F.win_count && F.bb[i] < nb) ? blk[F.bb[i]] : cnt[DISP_N_POINTS];
}

}  // namespace vba
