// The display export of the live local voxel map: the kernels of vba_kernels_display.hpp, compiled here and nowhere
// else, the host function that launches them on the map's arrays and the three entry points of include/voxelba.h.  The work arrays are
// members of the MapStore; the map itself is only read.
#include "vba_ctx.hpp"
#include "vba_kernels_display.hpp"
#include <cstring>

namespace vba {
namespace {

constexpr size_t kDispPinPoses = (size_t)VBA_MAX_WIN * 12 * sizeof(double);           // the pinned block: poses, then the counts
constexpr size_t kDispPinBytes = kDispPinPoses + (size_t)DISP_CNT_N * sizeof(int);

template <class M>
int disp_grow(MapStore &s, M &m, size_t want, std::string &err) {
  if (want <= m.n) return VBA_OK;
  VBA_HIPCHK(err, m.ensure(want));
  s.disp_allocs++; s.disp_bytes += (int64_t)(want * sizeof(*m.p));
  return VBA_OK;
}

// `want` when nothing is there yet (or the caller reserves), else the current size doubled until it suffices
inline size_t disp_size(size_t have, size_t want, bool exact) {
  if (want <= have) return have;
  size_t m = (exact || !have) ? want : have;
  while (m < want) m *= 2;
  return m;
}

// bytes of the device staging of a host result: records, plane records, keys, plane indices
inline size_t disp_stage_bytes(size_t np, size_t npl) { return np * 16 + npl * 64 + npl * 40 + np * 4; }

// the work arrays for `nodes` nodes, `blocks` workgroup counts, `pts` threads of the point grid and a host result of `stage` bytes; a
// buffer that has to grow is replaced after a synchronise (the stream may still read the old one)
int disp_ensure(MapStore &s, hipStream_t st, size_t nodes, size_t blocks, size_t pts, size_t stage, bool exact, std::string &err) {
  const bool grow = nodes > s.disp_nidx.n || blocks > s.disp_blk.n || pts > s.disp_inv.n || stage > s.disp_stage.n || !s.disp_cnt.p || !s.disp_poses.p || !s.disp_pin.p;
  if (!grow) return VBA_OK;
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  int r;
  if ((r = disp_grow(s, s.disp_nidx, disp_size(s.disp_nidx.n, nodes, exact), err)) || (r = disp_grow(s, s.disp_blk, disp_size(s.disp_blk.n, blocks, exact), err)) ||
      (r = disp_grow(s, s.disp_inv, disp_size(s.disp_inv.n, pts, exact), err)) ||
      (r = disp_grow(s, s.disp_stage, disp_size(s.disp_stage.n, stage, exact), err)) || (r = disp_grow(s, s.disp_cnt, (size_t)DISP_CNT_N, err)) ||
      (r = disp_grow(s, s.disp_poses, (size_t)VBA_MAX_WIN * 12, err)) || (r = disp_grow(s, s.disp_pin, kDispPinBytes, err)))
    return r;
  return VBA_OK;
}

inline size_t disp_node_room(const MapStore &s) {
  size_t n = s.v.cap > 0 ? (size_t)s.v.cap : (size_t)1 << 18;     // (the map's first node allocation)
  if (s.opt.max_map_nodes > n) n = s.opt.max_map_nodes;
  return n;
}

int map_display_reserve(MapStore &s, hipStream_t st, int64_t max_points, int64_t max_planes, std::string &err) {
  const size_t nodes = disp_node_room(s);
  const size_t pblocks = ((size_t)max_points + 255) / 256 + VBA_MAX_WIN;            // (every frame may end in a ragged workgroup)
  return disp_ensure(s, st, nodes, (nodes + 255) / 256 + pblocks, pblocks * 256, disp_stage_bytes((size_t)max_points, (size_t)max_planes), true, err);
}

int map_display(MapStore &s, hipStream_t st, int win_count, const double *poses, int flags, int64_t cap_points, float *xyzi, int *plane_of_point,
                int64_t *frame_begin, int64_t cap_planes, float *planes, long long *plane_key, bool dev_out, int64_t *n_points, int64_t *n_planes,
                std::string &err) {
  *n_points = 0; *n_planes = 0;
  const bool query_pts = cap_points == 0 && !xyzi, query_pl = cap_planes == 0 && !planes;
  // the frames end to end
  DispFrames F;
  std::memset(&F, 0, sizeof(F));
  F.win_count = win_count;
  long long total = 0, nbp = 0;
  for (int i = 0; i < win_count; i++) {
    F.slot[i] = s.mp[i]; F.npts[i] = s.allocated ? s.npts[s.mp[i]] : 0; F.bb[i] = (int)nbp;
    total += F.npts[i]; nbp += (F.npts[i] + 255) / 256;
  }
  F.bb[win_count] = (int)nbp;
  if (total >= (1ll << 31)) return VBA_ERR_CAPACITY;
  // an upper bound of the node count (exact after the last read-back, plus the points inserted since): storage above the true count
  // reads as non-planar, so no read-back is needed before the pass
  const long long nn = !s.allocated ? 0 : (s.ub_nodes < (long long)s.v.cap ? s.ub_nodes : (long long)s.v.cap);
  if (nn == 0 && total == 0) {
    if (frame_begin) for (int i = 0; i <= win_count; i++) frame_begin[i] = 0;
    return VBA_OK;
  }
  const int nbn = (int)((nn + 255) / 256);
  int r = disp_ensure(s, st, (size_t)(nn > 0 ? s.v.cap : 0), (size_t)nbn + (size_t)nbp, (size_t)nbp * 256, 0, false, err);
  if (r) return r;
  double *h_poses = (double *)s.disp_pin.p;
  int *h_cnt = (int *)(s.disp_pin.p + kDispPinPoses);
  if (win_count > 0) {   // (every call ends drained, so the pinned block is free)
    std::memcpy(h_poses, poses, (size_t)win_count * 12 * sizeof(double));
    VBA_HIPCHK(err, hipMemcpyAsync(s.disp_poses.p, h_poses, (size_t)win_count * 12 * sizeof(double), hipMemcpyHostToDevice, st));
  }
  int *nblk = s.disp_blk.p, *pblk = s.disp_blk.p + nbn, *cnt = s.disp_cnt.p;
  const int all = flags & 1;
  if (nbn > 0) hipLaunchKernelGGL(k_disp_nodes<0>, dim3(nbn), dim3(256), 0, st, s.v, (int)nn, nblk, s.disp_nidx.p);
  hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, nblk, nbn, cnt, -1, 0, (int)DISP_N_PLANES);
  if (nbn > 0) hipLaunchKernelGGL(k_disp_nodes<1>, dim3(nbn), dim3(256), 0, st, s.v, (int)nn, nblk, s.disp_nidx.p);
  if (nbp > 0) {
    VBA_HIPCHK(err, hipMemsetAsync(s.disp_inv.p, 0xFF, (size_t)nbp * 256 * sizeof(int), st));
    hipLaunchKernelGGL(k_disp_inverse, dim3((unsigned)nbp), dim3(256), 0, st, s.v, F, s.disp_inv.p);
    hipLaunchKernelGGL(k_disp_points<0>, dim3((unsigned)nbp), dim3(256), 0, st, s.v, F, (int)nn, (const int *)s.disp_nidx.p, (const int *)s.disp_inv.p, all,
                       pblk, (const double *)s.disp_poses.p, (float4 *)nullptr, (int *)nullptr);
  }
  hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, pblk, (int)nbp, cnt, -1, 0, (int)DISP_N_POINTS);
  hipLaunchKernelGGL(k_disp_frames, dim3(1), dim3(64), 0, st, (const int *)pblk, (int)nbp, F, cnt);
  VBA_HIPCHK(err, hipGetLastError());
  // the one wait of the call: the host needs the counts
  VBA_HIPCHK(err, hipMemcpyAsync(h_cnt, cnt, (size_t)DISP_CNT_N * sizeof(int), hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  const long long np = h_cnt[DISP_N_POINTS], npl = h_cnt[DISP_N_PLANES];
  *n_points = np; *n_planes = npl;
  if ((!query_pts && np > cap_points) || (!query_pl && npl > cap_planes)) return VBA_ERR_CAPACITY;
  if (frame_begin) for (int i = 0; i <= win_count; i++) frame_begin[i] = h_cnt[DISP_FRAME0 + i];
  const bool want_pts = !query_pts && np > 0, want_pl = !query_pl && npl > 0 && (planes || plane_key);
  if (!want_pts && !want_pl) return VBA_OK;
  float4 *o_xyzi = (float4 *)xyzi, *o_planes = (float4 *)planes;
  long long *o_key = plane_key;
  int *o_pop = plane_of_point;
  if (!dev_out) {   // a host result is written to the staging buffer and copied from there
    const size_t wp = want_pts ? (size_t)np : 0, wl = want_pl ? (size_t)npl : 0;
    r = disp_ensure(s, st, 0, 0, 0, disp_stage_bytes(wp, wl), false, err);
    if (r) return r;
    char *b = s.disp_stage.p;
    o_xyzi = (float4 *)b; b += wp * 16;
    o_planes = planes ? (float4 *)b : nullptr; b += wl * 64;
    o_key = plane_key ? (long long *)b : nullptr; b += wl * 40;
    o_pop = plane_of_point ? (int *)b : nullptr;
  }
  if (want_pl) hipLaunchKernelGGL(k_disp_planes, dim3(nbn), dim3(256), 0, st, s.v, (int)nn, (const int *)s.disp_nidx.p, (int)npl, o_planes, o_key);
  if (want_pts)
    hipLaunchKernelGGL(k_disp_points<1>, dim3((unsigned)nbp), dim3(256), 0, st, s.v, F, (int)nn, (const int *)s.disp_nidx.p, (const int *)s.disp_inv.p, all,
                       pblk, (const double *)s.disp_poses.p, o_xyzi, o_pop);
  VBA_HIPCHK(err, hipGetLastError());
  if (!dev_out) {
    if (want_pts) {
      VBA_HIPCHK(err, hipMemcpyAsync(xyzi, o_xyzi, (size_t)np * 16, hipMemcpyDeviceToHost, st));
      if (plane_of_point) VBA_HIPCHK(err, hipMemcpyAsync(plane_of_point, o_pop, (size_t)np * 4, hipMemcpyDeviceToHost, st));
    }
    if (want_pl) {
      if (planes) VBA_HIPCHK(err, hipMemcpyAsync(planes, o_planes, (size_t)npl * 64, hipMemcpyDeviceToHost, st));
      if (plane_key) VBA_HIPCHK(err, hipMemcpyAsync(plane_key, o_key, (size_t)npl * 40, hipMemcpyDeviceToHost, st));
    }
    VBA_HIPCHK(err, hipStreamSynchronize(st));
  }
  return VBA_OK;
}

}  // namespace
}  // namespace vba

extern "C" {

int vba_map_display_reserve(vba_ctx *c, int64_t max_points, int64_t max_planes) {
  if (!c || max_points < 0 || max_planes < 0) return VBA_ERR_BAD_ARG;
  if (max_points >= ((int64_t)1 << 31) || max_planes >= ((int64_t)1 << 31)) return VBA_ERR_CAPACITY;
  HIPCHK(c, hipSetDevice(c->device));
  return map_display_reserve(c->map, c->stream, max_points, max_planes, c->err);
}

int vba_map_display_allocations(vba_ctx *c, int *n_allocs, int64_t *bytes) {
  if (!c || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = c->map.disp_allocs; *bytes = c->map.disp_bytes;
  return VBA_OK;
}

int vba_map_display(vba_ctx *c, int win_count, const double *poses, int flags, int64_t cap_points, float *xyzi, int *plane_of_point,
                    int64_t *frame_begin, int64_t cap_planes, float *planes, long long *plane_key, int64_t *n_points, int64_t *n_planes) {
  if (!c || !n_points || !n_planes || win_count < 0 || win_count > c->opt.win_size || (win_count > 0 && !poses) || cap_points < 0 ||
      cap_planes < 0 || (flags & ~1) || (cap_points > 0 && !xyzi) || (cap_planes > 0 && !planes && !plane_key))
    return VBA_ERR_BAD_ARG;
  // the four result arrays on one side
  const void *outs[4] = {xyzi, plane_of_point, planes, plane_key};
  int n_dev = 0, n_out = 0;
  for (const void *p : outs) if (p) { n_out++; n_dev += is_device_ptr(p) ? 1 : 0; }
  if (n_dev != 0 && n_dev != n_out) { c->set_error("vba_map_display: xyzi, plane_of_point, planes and plane_key must be all host or all device memory"); return VBA_ERR_BAD_ARG; }
  const bool dev_out = n_dev > 0;
  if (dev_out && ((((uintptr_t)xyzi) | ((uintptr_t)planes)) & 15)) { c->set_error("vba_map_display: a device xyzi / planes must be 16-byte aligned"); return VBA_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  return map_display(c->map, c->stream, win_count, poses, flags, cap_points, xyzi, plane_of_point, frame_begin, cap_planes, planes, plane_key,
                     dev_out, n_points, n_planes, c->err);
}

}  // extern "C"
