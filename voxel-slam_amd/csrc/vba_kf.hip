// Scan pre-processing (vba_scan_*), the keyframe store (vba_kf_*) and the global map export (vba_kf_export_*)
// of libvoxelba.so: host drivers of the kernels in vba_kernels_scan.hpp and vba_kernels_kf.hpp.
#include "vba_ctx.hpp"
#include "vba_sat.hpp"
#include "vba_kf_store.hpp"
#include "vba_btc_db.hpp"
#include "vba_scanlog.hpp"
#include "vba_kernels_scan.hpp"
#include "vba_kernels_kf.hpp"
#include "vba_surfel_decl.hpp"

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <map>
#include <functional>
#include <algorithm>

using namespace vba;

extern "C" {

int vba_scan_var_init(vba_ctx *c, int n, const double *pnt_in, const double *ext_pose, double dept_err, double beam_err, double *pnt_out,
                      double *var_out) {
  if (n < 0 || (n > 0 && (!pnt_in || !pnt_out || !var_out)) || !ext_pose) return VBA_ERR_BAD_ARG;
  if (n == 0) return VBA_OK;
  int st = ensure_stage(c, ((size_t)n * 15 + 16) * sizeof(double));
  if (st) return st;
  double *d_in = (double *)c->d_stage.p, *d_out = d_in + (size_t)n * 3, *d_var = d_out + (size_t)n * 3, *d_ext = d_var + (size_t)n * 9;
  HIPCHK(c, hipMemcpyAsync(d_in, pnt_in, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ext, ext_pose, 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_var_init, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d_in, d_out, d_var, d_ext, (float)dept_err, (float)beam_err);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(pnt_out, d_out, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(var_out, d_var, (size_t)n * 9 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}
}  // extern "C"
namespace vba {
// also the down-sampling pass of vba_scan_prepare (vba_scan.hip)
int ds_core(vba_ctx *c, hipStream_t stream, int mode, int n, const double *d_in, const double *d_var, int vrow, int vstep, double voxel_size,
            bool det, const DsWork &w) {
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_ds_clear, dim3((w.cap + 255) / 256), dim3(256), 0, stream, w.tab, w.cap);
  if (det) {
    hipLaunchKernelGGL(k_ds_insert<true>, dim3(nb), dim3(256), 0, stream, n, d_in, d_var, voxel_size, w.tab, w.cap - 1, w.slot, vrow, vstep);
    hipLaunchKernelGGL(k_iota, dim3(nb), dim3(256), 0, stream, w.idx, n);
    size_t tmp = w.tmp_bytes;
    HIPCHK(c, sort_pairs_u32(w.tmp, tmp, (const unsigned int *)w.slot, w.skey, w.idx, w.sidx, (size_t)n, w.key_bits, stream));
    hipLaunchKernelGGL(k_ds_segstart, dim3(nb), dim3(256), 0, stream, n, w.skey, w.tab);
    hipLaunchKernelGGL(k_ds_sum_det, dim3(nb), dim3(256), 0, stream, n, d_in, d_var, w.sidx, w.tab, w.slot, vrow, vstep);
  } else {
    hipLaunchKernelGGL(k_ds_insert<false>, dim3(nb), dim3(256), 0, stream, n, d_in, d_var, voxel_size, w.tab, w.cap - 1, w.slot, vrow, vstep);
  }
  if (mode == 2) {
    hipLaunchKernelGGL(k_ds_close_min, dim3(nb), dim3(256), 0, stream, n, d_in, w.tab, w.slot, w.dist);
    hipLaunchKernelGGL(k_ds_close_arg, dim3(nb), dim3(256), 0, stream, n, w.tab, w.slot, w.dist);
  }
  hipLaunchKernelGGL(k_ds_count, dim3(nb), dim3(256), 0, stream, n, w.tab, w.slot, w.blk);
  hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(256), 0, stream, nb, w.blk, w.n_out);
  return VBA_OK;
}
}  // namespace vba
extern "C" {
// mode 0 down_sampling_voxel, 1 down_sampling_pvec (var in, vout out), 2 down_sampling_close (first_out = chosen indices)
static int ds_common(vba_ctx *c, int mode, int n, const double *pnt, const double *var, double voxel_size, double *pnt_out, double *vout, int *count_out,
                     int *first_out, int *n_out) {
  if (n < 0 || !n_out || (n > 0 && (!pnt || !first_out)) || (mode != 2 && n > 0 && (!pnt_out || !count_out)) || (mode == 1 && n > 0 && (!var || !vout)))
    return VBA_ERR_BAD_ARG;
  *n_out = 0;
  if (n == 0) return VBA_OK;
  if (voxel_size < 0.001 && mode != 1) {                                // TL:203 / TL:242: the cloud is left untouched
    if (pnt_out) HIPCHK(c, hipMemcpyAsync(pnt_out, pnt, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    std::vector<int> z(n, 0), id(n);
    for (int i = 0; i < n; i++) id[i] = i;
    if (count_out) HIPCHK(c, hipMemcpyAsync(count_out, z.data(), (size_t)n * sizeof(int), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(first_out, id.data(), (size_t)n * sizeof(int), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = n;
    return VBA_OK;
  }
  int cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  const int nb = (n + 255) / 256;
  const bool det = c->opt.deterministic != 0;
  unsigned int key_bits = 1;
  while ((1u << key_bits) < (unsigned)cap) key_bits++;
  size_t b_sort = 0;   // deterministic mode: sorted slot keys, index values in / out, rocPRIM scratch
  if (det) {
    size_t tmp = 0;
    HIPCHK(c, sort_pairs_u32(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, (size_t)n, key_bits, c->stream));
    b_sort = 3 * ((((size_t)n * sizeof(int)) + 15) & ~(size_t)15) + ((tmp + 255) & ~(size_t)255);
  }
  const size_t b_tab = (size_t)cap * sizeof(DsSlot), b_pnt = (size_t)n * 3 * sizeof(double), b_i = (((size_t)n * sizeof(int)) + 15) & ~(size_t)15,
               b_blk = (((size_t)nb + 1) * sizeof(int) + 15) & ~(size_t)15, b_var = mode == 1 ? (size_t)n * 9 * sizeof(double) : 0,
               b_dist = mode == 2 ? (size_t)n * sizeof(double) : 0;
  int st = ensure_stage(c, b_tab + 3 * b_pnt + b_var + b_dist + 3 * b_i + b_blk + 64 + b_sort + 256);
  if (st) return st;
  char *base = (char *)c->d_stage.p;
  DsSlot *tab = (DsSlot *)base;
  double *d_in = (double *)(base + b_tab), *d_out = (double *)(base + b_tab + b_pnt), *d_vout = (double *)(base + b_tab + 2 * b_pnt),
         *d_var = (double *)(base + b_tab + 3 * b_pnt), *d_dist = (double *)(base + b_tab + 3 * b_pnt + b_var);
  int *d_slot = (int *)(base + b_tab + 3 * b_pnt + b_var + b_dist), *d_cnt = (int *)((char *)d_slot + b_i), *d_first = (int *)((char *)d_cnt + b_i),
      *d_blk = (int *)((char *)d_first + b_i), *d_n = d_blk + nb;
  HIPCHK(c, hipMemcpyAsync(d_in, pnt, b_pnt, hipMemcpyDefault, c->stream));
  if (mode == 1) HIPCHK(c, hipMemcpyAsync(d_var, var, b_var, hipMemcpyDefault, c->stream));
  TimedSpan sp{};
  span_begin(c, "downsample", sp);
  DsWork w{};
  w.tab = tab; w.cap = cap; w.key_bits = key_bits; w.slot = d_slot; w.blk = d_blk; w.n_out = d_n; w.dist = d_dist;
  if (det) {
    char *sb = (char *)(((uintptr_t)((char *)d_n + 64) + 255) & ~(uintptr_t)255);
    w.skey = (unsigned int *)sb; w.idx = (int *)(sb + b_i); w.sidx = (int *)(sb + 2 * b_i);
    w.tmp = sb + 3 * b_i; w.tmp_bytes = b_sort - 3 * b_i;
  }
  st = ds_core(c, c->stream, mode, n, d_in, mode == 1 ? d_var : nullptr, 9, 4, voxel_size, det, w);
  if (st) return st;
  hipLaunchKernelGGL(k_ds_emit, dim3(nb), dim3(256), 0, c->stream, n, tab, d_slot, d_blk, d_out, d_cnt, d_first, d_vout, mode);
  span_end(c, "downsample", sp);
  HIPCHK(c, hipGetLastError());
  int m = 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(&m, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (m > 0) {
    if (pnt_out) HIPCHK(c, hipMemcpyAsync(pnt_out, d_out, (size_t)m * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    if (count_out) HIPCHK(c, hipMemcpyAsync(count_out, d_cnt, (size_t)m * sizeof(int), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(first_out, d_first, (size_t)m * sizeof(int), hipMemcpyDefault, c->stream));
    if (mode == 1) HIPCHK(c, hipMemcpyAsync(vout, d_vout, (size_t)m * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *n_out = m;
  return VBA_OK;
}
int vba_scan_down_sampling_voxel(vba_ctx *c, int n, const double *pnt, double voxel_size, double *pnt_out, int *count_out, int *first_out,
                                 int *n_out) {
  return ds_common(c, 0, n, pnt, nullptr, voxel_size, pnt_out, nullptr, count_out, first_out, n_out);
}
int vba_scan_down_sampling_pvec(vba_ctx *c, int n, const double *pnt, const double *var, double voxel_size, double *pnt_out, double *vardiag_out,
                                int *count_out, int *n_out) {
  std::vector<int> first(n > 0 ? n : 1);
  return ds_common(c, 1, n, pnt, var, voxel_size, pnt_out, vardiag_out, count_out, first.data(), n_out);
}
int vba_scan_down_sampling_close(vba_ctx *c, int n, const double *pnt, double voxel_size, int *index_out, int *n_out) {
  return ds_common(c, 2, n, pnt, nullptr, voxel_size, nullptr, nullptr, nullptr, index_out, n_out);
}
int vba_scan_undistort(vba_ctx *c, int n, double *pnt, const double *curv, int m, const double *imu_poses, const double *end_pose,
                       const double *ext_pose) {
  if (n < 0 || m < 0 || (n > 0 && (!pnt || !curv)) || (m > 0 && !imu_poses) || !end_pose || !ext_pose) return VBA_ERR_BAD_ARG;
  if (n == 0 || m == 0) return VBA_OK;
  const size_t nprm = (size_t)22 * m + 24;
  int st = ensure_stage(c, ((size_t)n * 4 + nprm) * sizeof(double));
  if (st) return st;
  double *d_p = (double *)c->d_stage.p, *d_c = d_p + (size_t)n * 3, *d_prm = d_c + n;
  std::vector<double> prm(nprm);
  std::memcpy(prm.data(), imu_poses, (size_t)22 * m * sizeof(double));
  std::memcpy(prm.data() + (size_t)22 * m, end_pose, 12 * sizeof(double));
  std::memcpy(prm.data() + (size_t)22 * m + 12, ext_pose, 12 * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(d_p, pnt, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_c, curv, (size_t)n * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_prm, prm.data(), nprm * sizeof(double), hipMemcpyHostToDevice, c->stream));
  TimedSpan sp{};
  span_begin(c, "undistort", sp);
  hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d_p, d_c, m, d_prm);
  span_end(c, "undistort", sp);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(pnt, d_p, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // prm is a host temporary
  return VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ keyframe store (vba_kf_*)

namespace {

size_t kf_tab_off_bytes(int t) { return ((size_t)t + 1) * sizeof(int) + 15 & ~(size_t)15; }
// transforms [t][12] | offsets [t + 1] | source starts [t] (a build from a scan log)
size_t kf_tab_bytes(int t) { return (size_t)t * 12 * sizeof(double) + 2 * kf_tab_off_bytes(t); }

// a fresh device block of n elements, counted (vba_kf_allocations)
template <class T>
int kf_alloc(vba_kf_store *s, DevMem<T> &m, size_t n) {
  m.reset();
  HIPCHK(s->ctx, m.ensure(n ? n : 1));
  s->allocs++; s->bytes += (int64_t)(n * sizeof(T));
  return VBA_OK;
}

}  // namespace
namespace vba {
// layout of the down-sampler's work area for n points (also the scan frame's, vba_scan.hip)
size_t kf_ws_layout(vba_ctx *c, int n, bool det, char *base, DsWork *w, int *status) {
  int cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  unsigned int key_bits = 1;
  while ((1u << key_bits) < (unsigned)cap) key_bits++;
  const int nb = (n + 255) / 256;
  const size_t b_i = (((size_t)n * sizeof(int)) + 255) & ~(size_t)255, b_tab = (size_t)cap * sizeof(DsSlot),
               b_blk = (((size_t)nb + 2) * sizeof(int) + 255) & ~(size_t)255;
  size_t tmp = 0;
  if (det && sort_pairs_u32(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, (size_t)n, key_bits, c->stream) != hipSuccess) { *status = VBA_ERR_HIP; return 0; }
  tmp = (tmp + 255) & ~(size_t)255;
  if (w) {
    w->tab = (DsSlot *)base; w->cap = cap; w->key_bits = key_bits;
    w->slot = (int *)(base + b_tab); w->blk = (int *)(base + b_tab + b_i); w->n_out = w->blk + nb;
    if (det) {
      char *sb = base + b_tab + b_i + b_blk;
      w->skey = (unsigned int *)sb; w->idx = (int *)(sb + b_i); w->sidx = (int *)(sb + 2 * b_i); w->tmp = sb + 3 * b_i; w->tmp_bytes = tmp;
    }
  }
  *status = VBA_OK;
  return b_tab + b_i + b_blk + (det ? 3 * b_i + tmp : 0);
}
}  // namespace vba
namespace {

// grow-only: the keyframe arrays move (device-to-device copy, the old blocks are freed after a synchronise)
int kf_ensure_rows(vba_kf_store *s, size_t need) {
  if (need <= s->cap) return VBA_OK;
  vba_ctx *c = s->ctx;
  size_t m = s->cap ? s->cap : 65536;
  while (m < need) m *= 2;
  const size_t have = (size_t)s->off.back();
  HIPCHK(c, s->d_pnt.grow_keep(m * 3, have * 3, c->stream));
  HIPCHK(c, s->d_var.grow_keep(m * 3, have * 3, c->stream));
  s->cap = m;
  s->allocs += 2; s->bytes += (int64_t)(m * 3 * (sizeof(double) + sizeof(float)));
  return VBA_OK;
}

int kf_ensure_merge(vba_kf_store *s, size_t need) {
  if (need <= s->mcap) return VBA_OK;
  vba_ctx *c = s->ctx;
  size_t m = s->mcap ? s->mcap : 65536;
  while (m < need) m *= 2;
  if (m > ((size_t)1 << 28)) return VBA_ERR_CAPACITY;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int st = VBA_OK;
  const size_t ws = kf_ws_layout(c, (int)m, true, nullptr, nullptr, &st);
  if (st) return st;
  if ((st = kf_alloc(s, s->d_src, 3 * m)) || (st = kf_alloc(s, s->d_merge, 3 * m)) || (st = kf_alloc(s, s->d_mdiag, 3 * m)) ||
      (st = kf_alloc(s, s->d_cnt, m)) || (st = kf_alloc(s, s->d_ws, ws)))
    return st;
  HIPCHK(c, s->h_diag.ensure(3 * m));
  s->allocs++;
  s->mcap = m;
  return VBA_OK;
}

int kf_ensure_tab(vba_kf_store *s, int k) {
  if (k <= s->tcap) return VBA_OK;
  vba_ctx *c = s->ctx;
  int t = s->tcap ? s->tcap : 64;
  while (t < k) t *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, s->h_tab.ensure(kf_tab_bytes(t)));
  s->allocs++;
  int st = kf_alloc(s, s->d_tab, kf_tab_bytes(t));
  if (st) return st;
  s->tcap = t;
  return VBA_OK;
}

// Host half of the merge (include/voxelba.h, "order of operations"): T = [dR, dp] of a cloud at pose x into the frame of pose xc
void kf_delta(const double *xc, const double *x, double *T) {
  volatile double a, b, e;     // every product and sum rounded on its own, whatever the host compiler would contract
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) {
      a = xc[0 * 3 + r] * x[0 * 3 + cc]; b = xc[1 * 3 + r] * x[1 * 3 + cc]; a = a + b; e = xc[2 * 3 + r] * x[2 * 3 + cc];
      T[3 * r + cc] = a + e;
    }
  const double d0 = x[9] - xc[9], d1 = x[10] - xc[10], d2 = x[11] - xc[11];
  for (int r = 0; r < 3; r++) {
    a = xc[0 * 3 + r] * d0; b = xc[1 * 3 + r] * d1; a = a + b; e = xc[2 * 3 + r] * d2;
    T[9 + r] = a + e;
  }
}

// the transform table of k clouds with poses [k][12] (xc = the last), row offsets rel [k + 1] and, for clouds that lie apart in their
// source array, the source row of each cloud's first point (starts [k], else nullptr) -> pinned image -> device, on st
int kf_upload_tab(vba_kf_store *s, int k, const double *const *poses, const int *rel, hipStream_t st, const int *starts = nullptr) {
  vba_ctx *c = s->ctx;
  double *T = (double *)s->h_tab.p;
  int *o = (int *)(s->h_tab + (size_t)s->tcap * 12 * sizeof(double));
  int *b = (int *)((char *)o + kf_tab_off_bytes(s->tcap));
  for (int i = 0; i < k; i++) kf_delta(poses[k - 1], poses[i], T + 12 * i);
  for (int i = 0; i <= k; i++) o[i] = rel[i];
  if (starts) for (int i = 0; i < k; i++) b[i] = starts[i];
  HIPCHK(c, hipMemcpyAsync(s->d_tab, s->h_tab, kf_tab_bytes(s->tcap), hipMemcpyHostToDevice, st));
  return VBA_OK;
}
const double *kf_dev_xf(const vba_kf_store *s) { return (const double *)s->d_tab.p; }
const int *kf_dev_off(const vba_kf_store *s) { return (const int *)(s->d_tab + (size_t)s->tcap * 12 * sizeof(double)); }
const int *kf_dev_start(const vba_kf_store *s) { return (const int *)((const char *)kf_dev_off(s) + kf_tab_off_bytes(s->tcap)); }

bool kf_pose_ok(const double *p) { for (int i = 0; i < 12; i++) if (!std::isfinite(p[i])) return false; return true; }

}  // namespace

extern "C" {

int vba_kf_create(vba_ctx *c, vba_kf_store **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  vba_kf_store *s = new vba_kf_store();
  s->ctx = c;
  int st = kf_ensure_tab(s, 64);
  if (!st && s->h_n.ensure(16) != hipSuccess) st = VBA_ERR_HIP;
  if (!st && hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) != hipSuccess) st = VBA_ERR_HIP;
  if (st) { vba_kf_destroy(s); return st; }
  s->allocs++;
  *out = s;
  return VBA_OK;
}

void vba_kf_destroy(vba_kf_store *s) {
  if (!s) return;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  if (s->ev) hipEventDestroy(s->ev);
  delete s;
}

int vba_kf_reserve(vba_kf_store *s, int64_t points, int keyframes, int64_t merge_points) {
  if (!s || points < 0 || keyframes < 0 || merge_points < 0 || points > ((int64_t)1 << 30) || merge_points > ((int64_t)1 << 28) || keyframes > (1 << 24))
    return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if (merge_points > 0 && (st = kf_ensure_merge(s, (size_t)merge_points))) return st;
  // a build writes its kept cloud straight behind the last keyframe, and that cloud is bounded only by the merged one
  if (points + merge_points > 0 && (st = kf_ensure_rows(s, (size_t)(points + merge_points)))) return st;
  s->off.reserve((size_t)keyframes + 1); s->kf.reserve((size_t)keyframes); s->hist_pos.reserve(3 * (size_t)keyframes);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_kf_allocations(vba_kf_store *s, int *count, int64_t *bytes) {
  if (!s || !count || !bytes) return VBA_ERR_BAD_ARG;
  *count = s->allocs; *bytes = s->bytes;
  return VBA_OK;
}

int vba_kf_size(vba_kf_store *s) { return s ? (int)s->kf.size() : 0; }

}  // extern "C"
namespace {

// The k scans of a build: rel [k + 1] = the points before each scan among the k.  Without starts they are rows rel[i] .. rel[i + 1]
// of pnt / var (HOST or DEVICE); with starts [k] scan i begins at row starts[i] of the DEVICE arrays pnt / var (a scan log's arena).
struct KfScans { const int *rel; const double *pnt, *var; const int *starts; };

// vba_kf_build behind its argument checks: merge, down-sampling, descriptors, commit
int kf_build_scans(vba_kf_store *s, int k, const KfScans &in, const double *poses, double voxel_size, int id, double jour, vba_btc_db *db, int cap,
                   double *rows, uint64_t *bits, int *n_stds, int *n_points) {
  const int n = in.rel[k];
  const double *pnt = in.pnt, *var = in.var;
  vba_ctx *c = s->ctx;
  const size_t N = (size_t)s->off.back();
  if (N + (size_t)n > (size_t)INT32_MAX) return VBA_ERR_CAPACITY;
  int st;
  if (db) {
    if (db->ctx->device != c->device) return VBA_ERR_BAD_ARG;
    if ((st = btc_generate_check(db, n, cap, rows, bits, n_stds))) return st;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = kf_ensure_tab(s, k)) || (st = kf_ensure_merge(s, (size_t)n)) || (st = kf_ensure_rows(s, N + (size_t)n))) return st;
  if (db && n > 0 && (st = btc_gen_ensure(db, n, 0, 0))) return st;
  int m = 0;
  if (n > 0) {
    std::vector<const double *> pp(k);
    for (int i = 0; i < k; i++) pp[i] = poses + 12 * i;
    if ((st = kf_upload_tab(s, k, pp.data(), in.rel, c->stream, in.starts))) return st;
    const double *src = pnt, *dvar = nullptr;
    if (!in.starts && !is_device_ptr(pnt)) {
      HIPCHK(c, hipMemcpyAsync(s->d_src, src, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
      src = s->d_src;
    }
    if (var) {
      if (in.starts || is_device_ptr(var)) dvar = var;            // gathered by the merge kernel, 72 bytes apart
      else {                                                       // host array: only the three diagonal doubles per point cross
        const double *v = var;
        for (size_t i = 0; i < (size_t)n; i++) { s->h_diag[3 * i] = v[9 * i]; s->h_diag[3 * i + 1] = v[9 * i + 4]; s->h_diag[3 * i + 2] = v[9 * i + 8]; }
        HIPCHK(c, hipMemcpyAsync(s->d_mdiag, s->h_diag, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
      }
    }
    const int nb = (n + 255) / 256;
    if (in.starts)
      hipLaunchKernelGGL(k_kf_merge_rows, dim3(nb), dim3(256), 0, c->stream, n, k, kf_dev_off(s), kf_dev_start(s), kf_dev_xf(s), src, dvar, 9, 4,
                         s->d_merge, db ? db->gen->pts.xyz.p : (float *)nullptr, dvar ? s->d_mdiag : (double *)nullptr);
    else
      hipLaunchKernelGGL(k_kf_merge, dim3(nb), dim3(256), 0, c->stream, n, k, kf_dev_off(s), kf_dev_xf(s), src, dvar, 9, 4, s->d_merge,
                         db ? db->gen->pts.xyz.p : (float *)nullptr, dvar ? s->d_mdiag : (double *)nullptr);
    if (db && db->ctx->stream != c->stream) {                      // the generator runs on its database's stream, behind the merge
      HIPCHK(c, hipEventRecord(s->ev, c->stream));
      HIPCHK(c, hipStreamWaitEvent(db->ctx->stream, s->ev, 0));
    }
    const bool det = c->opt.deterministic != 0;
    DsWork w{};
    kf_ws_layout(c, n, det, s->d_ws, &w, &st);
    if (st) return st;
    TimedSpan sp{};
    span_begin(c, "downsample", sp);
    if ((st = ds_core(c, c->stream, var ? 1 : 0, n, s->d_merge, var ? s->d_mdiag : nullptr, 3, 1, voxel_size, det, w))) return st;
    hipLaunchKernelGGL(k_kf_emit, dim3(nb), dim3(256), 0, c->stream, n, w.tab, w.slot, w.blk, s->d_pnt + 3 * N, s->d_var + 3 * N, s->d_cnt, var ? 1 : 0);
    span_end(c, "downsample", sp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s->h_n, w.n_out, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  if (db) {
    st = btc_generate_impl(db, n, nullptr, id, cap, rows, bits, n_stds);
    if (st) { hipStreamSynchronize(c->stream); return st; }
  }
  if (n > 0) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m = s->h_n[0];
  }
  // commit
  vba_kf_store::Meta me{};
  std::memcpy(me.x0, poses + 12 * (size_t)(k - 1), 12 * sizeof(double));
  me.id = id; me.jour = jour; me.exist = 0;
  s->kf.push_back(me);
  s->off.push_back((int)(N + (size_t)m));
  s->last_m = m;
  *n_points = m;
  return VBA_OK;
}

}  // namespace
extern "C" {

int vba_kf_build(vba_kf_store *s, int k, const int *offsets, const double *pnt, const double *var, const double *poses, double voxel_size, int id,
                 double jour, vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds, int *n_points) {
  if (!s || k < 1 || !offsets || !poses || !n_points || !(voxel_size > 0) || (!var && voxel_size < 0.001)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < k; i++) if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
  const int off0 = offsets[0], n = offsets[k] - off0;
  if (n > (1 << 28) || (n > 0 && !pnt)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < k; i++) if (!kf_pose_ok(poses + 12 * i)) return VBA_ERR_BAD_ARG;
  std::vector<int> rel(k + 1);
  for (int i = 0; i <= k; i++) rel[i] = offsets[i] - off0;
  const KfScans in{rel.data(), pnt ? pnt + 3 * (size_t)off0 : nullptr, var ? var + 9 * (size_t)off0 : nullptr, nullptr};
  return kf_build_scans(s, k, in, poses, voxel_size, id, jour, db, cap, rows, bits, n_stds, n_points);
}

// vba_kf_build (var != NULL) on scans first .. first + k - 1 of a scan log, read at their own arena starts
int vba_kf_build_from_log(vba_kf_store *s, vba_scanlog *l, int64_t first, int k, const double *poses, double voxel_size, int id, double jour,
                          vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds, int *n_points) {
  if (!s || !l || k < 1 || !poses || !n_points || !(voxel_size > 0)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < k; i++) if (!kf_pose_ok(poses + 12 * i)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  if (l->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  ScanLogView v;
  int st = scanlog_view(l, first, k, 1ll << 28, c->stream, &v);     // the store's stream waits for the captures through an event
  if (st) return st;
  const KfScans in{v.rel.data(), v.d_pnt, v.d_var, v.starts.data()};
  return kf_build_scans(s, k, in, poses, voxel_size, id, jour, db, cap, rows, bits, n_stds, n_points);   // synchronises: nothing stays queued on the arena
}

int vba_kf_last_counts(vba_kf_store *s, int cap, int *counts, int *n) {
  if (!s || !n || cap < 0 || (cap > 0 && !counts)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  *n = s->last_m;
  const int w = s->last_m < cap ? s->last_m : cap;
  if (w > 0) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(counts, s->d_cnt, (size_t)w * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VBA_OK;
}

int vba_kf_generate_stds(vba_kf_store *s, int first, int count, vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds) {
  if (!s || !db || first < 0 || count < 1 || (size_t)first + (size_t)count > s->kf.size()) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  if (db->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  const int b = s->off[first], n = s->off[first + count] - b;
  int st;
  if ((st = btc_generate_check(db, n, cap, rows, bits, n_stds))) return st;
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = kf_ensure_tab(s, count))) return st;
  const int id = s->kf[first + count - 1].id;
  if (n > 0) {
    if ((st = btc_gen_ensure(db, n, 0, 0))) return st;
    std::vector<const double *> pp(count);
    std::vector<int> rel(count + 1);
    for (int i = 0; i < count; i++) pp[i] = s->kf[first + i].x0;
    for (int i = 0; i <= count; i++) rel[i] = s->off[first + i] - b;
    hipStream_t q = db->ctx->stream;                               // the store is quiescent between calls: everything on the database's stream
    if ((st = kf_upload_tab(s, count, pp.data(), rel.data(), q))) return st;
    hipLaunchKernelGGL(k_kf_merge, dim3((n + 255) / 256), dim3(256), 0, q, n, count, kf_dev_off(s), kf_dev_xf(s), s->d_pnt + 3 * (size_t)b,
                       (const double *)nullptr, 9, 4, (double *)nullptr, db->gen->pts.xyz.p, (double *)nullptr);
    HIPCHK(c, hipGetLastError());
  }
  st = btc_generate_impl(db, n, nullptr, id, cap, rows, bits, n_stds);
  if (st) hipStreamSynchronize(db->ctx->stream);
  return st;
}

int vba_kf_set_poses(vba_kf_store *s, int first, int n, const double *poses) {
  if (!s || first < 0 || n < 0 || (size_t)first + (size_t)n > s->kf.size() || (n > 0 && !poses)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < n; i++) if (!kf_pose_ok(poses + 12 * i)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < n; i++) std::memcpy(s->kf[first + i].x0, poses + 12 * (size_t)i, 12 * sizeof(double));
  return VBA_OK;
}

int vba_kf_get(vba_kf_store *s, int k, double *pose12, int *id, double *jour, int *exist, int *n_points) {
  if (!s || k < 0 || (size_t)k >= s->kf.size()) return VBA_ERR_BAD_ARG;
  const vba_kf_store::Meta &m = s->kf[k];
  if (pose12) std::memcpy(pose12, m.x0, 12 * sizeof(double));
  if (id) *id = m.id;
  if (jour) *jour = m.jour;
  if (exist) *exist = m.exist;
  if (n_points) *n_points = s->off[k + 1] - s->off[k];
  return VBA_OK;
}

int vba_kf_set_history(vba_kf_store *s, int n_hist) {
  if (!s || n_hist < 0 || (size_t)n_hist > s->kf.size()) return VBA_ERR_BAD_ARG;
  s->hist_pos.resize(3 * (size_t)n_hist);
  for (size_t i = 0; i < s->kf.size(); i++) {
    s->kf[i].exist = (int)i < n_hist ? 1 : 0;
    if ((int)i < n_hist) for (int j = 0; j < 3; j++) s->hist_pos[3 * i + j] = (float)s->kf[i].x0[9 + j];
  }
  s->hist = n_hist;
  return VBA_OK;
}

int vba_kf_history_size(vba_kf_store *s) { return s ? s->hist : 0; }

int vba_kf_load(vba_kf_store *s, int k, vba_ctx *mc, double jour) {
  if (!s || !mc || k < 0 || (size_t)k >= s->kf.size()) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  if (mc->device != c->device) return VBA_ERR_BAD_ARG;
  const int b = s->off[k], n = s->off[k + 1] - b;
  if (n > 0) {
    HIPCHK(c, hipSetDevice(c->device));
    int st;
    if ((st = kf_ensure_merge(s, (size_t)n))) return st;
    // the keyframe's x0 goes through the pinned table; the world points into the merge scratch, on the map context's stream
    std::memcpy(s->h_tab, s->kf[k].x0, 12 * sizeof(double));
    HIPCHK(mc, hipMemcpyAsync(s->d_tab, s->h_tab, 12 * sizeof(double), hipMemcpyHostToDevice, mc->stream));
    hipLaunchKernelGGL(k_kf_world, dim3((n + 255) / 256), dim3(256), 0, mc->stream, n, (const double *)s->d_tab.p, s->d_pnt + 3 * (size_t)b, s->d_merge);
    HIPCHK(mc, hipGetLastError());
    st = map_cut_voxel_fix(mc->map, mc->stream, n, s->d_merge, jour, mc->err);   // ends with the map's counter read-back: one synchronise
    if (st) { hipStreamSynchronize(mc->stream); return st; }
  }
  s->kf[k].exist = 0;
  return VBA_OK;
}

int vba_kf_load_nearby(vba_kf_store *s, vba_ctx *mc, const double *p3, double radius, double jour, int *loaded) {
  if (!s || !mc || !p3 || !loaded || !(radius >= 0)) return VBA_ERR_BAD_ARG;
  *loaded = -1;
  if (s->hist <= 0) return VBA_OK;                                   // VS:1382
  const float q[3] = {(float)p3[0], (float)p3[1], (float)p3[2]};
  const float r2 = (float)(radius * radius);
  std::vector<std::pair<float, int>> hit;
  const int nh = (int)(s->hist_pos.size() / 3);
  for (int i = 0; i < nh; i++) {
    volatile float d2 = 0.0f, t;                                     // x, then y, then z, each product and sum rounded to float
    for (int j = 0; j < 3; j++) { t = s->hist_pos[3 * (size_t)i + j] - q[j]; t = t * t; d2 = d2 + t; }
    if (d2 < r2) hit.emplace_back((float)d2, i);
  }
  std::sort(hit.begin(), hit.end());                                 // ascending distance, the lower index on a tie
  for (const auto &h : hit) {
    if (!s->kf[h.second].exist) continue;
    const int st = vba_kf_load(s, h.second, mc, jour);
    if (st) return st;
    s->hist--;
    *loaded = h.second;
    break;
  }
  return VBA_OK;
}

int vba_kf_read(vba_kf_store *s, int k, int cap, double *xyz, float *vardiag, int *n) {
  if (!s || !n || k < 0 || (size_t)k >= s->kf.size() || cap < 0) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  const int b = s->off[k], m = s->off[k + 1] - b;
  *n = m;
  const int w = m < cap ? m : cap;
  if (w > 0 && (xyz || vardiag)) {
    HIPCHK(c, hipSetDevice(c->device));
    if (xyz) HIPCHK(c, hipMemcpyAsync(xyz, s->d_pnt + 3 * (size_t)b, (size_t)w * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (vardiag) HIPCHK(c, hipMemcpyAsync(vardiag, s->d_var + 3 * (size_t)b, (size_t)w * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VBA_OK;
}

int vba_kf_clouds(vba_kf_store *s, const double **d_pnt, const int **offsets, int *n_kf) {
  if (!s || !d_pnt || !offsets || !n_kf) return VBA_ERR_BAD_ARG;
  *d_pnt = s->d_pnt; *offsets = s->off.data(); *n_kf = (int)s->kf.size();
  return VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ global map export (vba_kf_export_*)
namespace {

const long long kExpChunk = 1ll << 22;       // records per pass through the staging buffer of a host export (64 MiB)
const int kExpMaxBlocks = 2048;              // grid cap of the streaming kernel: 256 CUs x 8 workgroups, the rest is grid-strided

inline long long exp_count(long long size, long long jump) { return (size + jump - 1) / jump; }   // j = 0, jump, ... < size

// the table of `entries` keyframes: every image of the pinned ring and the device copy
int exp_ensure_tab(vba_ctx *c, size_t entries) {
  for (int i = 0; i < CtxSat::Exp::kRing; i++)
    if (!c->sat->exp.ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->sat->exp.ev[i], hipEventDisableTiming));
  const size_t have = c->sat->exp.d.n / sizeof(ExpKf);        // the device copy is made last
  if (entries <= have) return VBA_OK;
  size_t m = have ? have : 1024;
  while (m < entries) m *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sat->exp.d.reset();
  for (auto &h : c->sat->exp.h) h.reset();
  for (auto &h : c->sat->exp.h) HIPCHK(c, h.ensure(m * sizeof(ExpKf)));
  HIPCHK(c, c->sat->exp.d.ensure(m * sizeof(ExpKf)));
  return VBA_OK;
}

int exp_ensure_out(vba_ctx *c, size_t recs) {
  if (recs <= c->sat->exp.d_out.n) return VBA_OK;
  size_t m = c->sat->exp.d_out.n ? c->sat->exp.d_out.n : 65536;
  while (m < recs) m *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, c->sat->exp.d_out.ensure(m));
  return VBA_OK;
}

}  // namespace

extern "C" {

int vba_kf_export_plan(int n_kf, const int *sizes, int64_t interval_size, int jump, int *jump_out, int64_t *kf_begin, int cap_msgs, int *msg_end_kf,
                       int *n_msgs) {
  if (n_kf < 0 || (n_kf > 0 && !sizes) || interval_size < 1 || jump < 0 || !jump_out || !kf_begin || !n_msgs || cap_msgs < 0 ||
      (cap_msgs > 0 && !msg_end_kf))
    return VBA_ERR_BAD_ARG;
  uint64_t psize = 0;                                          // VS:117-123 in 64 bits: the reference's `uint psize` wraps at 2^32
  for (int k = 0; k < n_kf; k++) {
    if (sizes[k] < 0) return VBA_ERR_BAD_ARG;
    psize += (uint64_t)sizes[k];
  }
  if (jump == 0) {
    if (psize >= ((uint64_t)1 << 32)) return VBA_ERR_BAD_ARG;
    const uint64_t ten = interval_size > INT64_MAX / 10 ? (uint64_t)INT64_MAX : 10 * (uint64_t)interval_size;
    jump = (int)(psize / ten) + 1;                             // VS:124
  }
  *jump_out = jump;
  int64_t total = 0, pl = 0;
  int nm = 0;
  for (int k = 0; k < n_kf; k++) {
    kf_begin[k] = total;
    const int64_t cnt = exp_count(sizes[k], jump);             // VS:133
    total += cnt; pl += cnt;
    if (pl > interval_size) {                                  // VS:145-150
      if (nm < cap_msgs) msg_end_kf[nm] = k + 1;
      nm++; pl = 0;
    }
  }
  kf_begin[n_kf] = total;
  if (nm < cap_msgs) msg_end_kf[nm] = n_kf;                    // VS:153: published whatever it holds
  nm++;
  *n_msgs = nm;
  return VBA_OK;
}

int vba_kf_export_world(vba_ctx *c, int n_stores, vba_kf_store *const *stores, const float *intensity, int jump, int64_t begin, int64_t count,
                        float *xyzi) {
  if (!c || n_stores < 1 || !stores || !intensity || jump < 1 || begin < 0 || count < 0 || (count > 0 && !xyzi)) return VBA_ERR_BAD_ARG;
  for (int s = 0; s < n_stores; s++) if (!stores[s] || stores[s]->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  // exported points before every keyframe of the whole sequence (the plan's kf_begin), keyframes before every store
  std::vector<long long> &first = c->sat->exp.first;
  std::vector<int> &kbase = c->sat->exp.kbase;
  first.clear(); kbase.clear();
  long long total = 0;
  for (int s = 0; s < n_stores; s++) {
    const std::vector<int> &off = stores[s]->off;
    if (first.size() + stores[s]->kf.size() > (size_t)(1 << 30)) return VBA_ERR_CAPACITY;
    kbase.push_back((int)first.size());
    for (size_t k = 0; k + 1 < off.size(); k++) { first.push_back(total); total += exp_count((long long)off[k + 1] - off[k], jump); }
  }
  kbase.push_back((int)first.size());
  first.push_back(total);
  if (begin > total || count > total - begin) return VBA_ERR_BAD_ARG;
  if (count == 0) return VBA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev_out = is_device_ptr(xyzi);
  if (dev_out && ((uintptr_t)xyzi & 15)) { c->set_error("vba_kf_export_world: a device xyzi must be 16-byte aligned"); return VBA_ERR_BAD_ARG; }
  const long long end = begin + count;
  // the keyframes of the first and of the last exported point: the last k with first[k] <= i (never an empty keyframe)
  auto kf_of = [&](long long i) { return (int)(std::upper_bound(first.begin(), first.end() - 1, i) - first.begin()) - 1; };
  const int ka = kf_of(begin), kb = kf_of(end - 1), nk = kb - ka + 1;
  int st;
  if ((st = exp_ensure_tab(c, (size_t)nk))) return st;
  if (!dev_out && (st = exp_ensure_out(c, (size_t)(count < kExpChunk ? count : kExpChunk)))) return st;
  const int slot = c->sat->exp.next;
  c->sat->exp.next = (slot + 1) % CtxSat::Exp::kRing;
  HIPCHK(c, hipEventSynchronize(c->sat->exp.ev[slot]));             // the upload that last read this image (kRing calls ago): long done
  ExpKf *h = (ExpKf *)c->sat->exp.h[slot].p;
  for (int s = 0; s < n_stores; s++) {
    const vba_kf_store *S = stores[s];
    for (int g = std::max(ka, kbase[s]); g <= kb && g < kbase[s + 1]; g++) {
      const int k = g - kbase[s];
      ExpKf &e = h[g - ka];
      e.first = first[g]; e.row = S->off[k];
      std::memcpy(e.T, S->kf[k].x0, 12 * sizeof(double));
    }
  }
  HIPCHK(c, hipMemcpyAsync(c->sat->exp.d, h, (size_t)nk * sizeof(ExpKf), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->sat->exp.ev[slot], c->stream));
  const ExpKf *d_tab = (const ExpKf *)c->sat->exp.d.p;
  for (long long cb = begin; cb < end; cb += dev_out ? count : kExpChunk) {
    const long long ce = dev_out ? end : std::min(end, cb + kExpChunk);
    float4 *out = dev_out ? (float4 *)xyzi : c->sat->exp.d_out.p;                     // the record of cb
    for (int s = 0; s < n_stores; s++) {                       // one launch per store: its point array, its intensity, its rows of the table
      const long long a = std::max(cb, first[kbase[s]]), b = std::min(ce, first[kbase[s + 1]]);
      if (a >= b) continue;
      const int g0 = std::max(ka, kbase[s]), g1 = std::min(kb, kbase[s + 1] - 1);
      const long long nb = (b - a + 255) / 256;
      hipLaunchKernelGGL(k_kf_export, dim3((unsigned)std::min<long long>(nb, kExpMaxBlocks)), dim3(256), 0, c->stream, a, b - a, g1 - g0 + 1,
                         d_tab + (g0 - ka), (const double *)stores[s]->d_pnt, jump, intensity[s], out + (a - cb));
    }
    HIPCHK(c, hipGetLastError());
    if (!dev_out) HIPCHK(c, hipMemcpyAsync(xyzi + 4 * (size_t)(cb - begin), c->sat->exp.d_out, (size_t)(ce - cb) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  }
  if (!dev_out) HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

// pub_localmap's point loop (VS:63-76) over scans of a scan log: the same gather with one table row per scan, whose `row` is the
// scan's own arena start and whose T is the pose given for it
int vba_scanlog_export_world(vba_ctx *c, vba_scanlog *l, int64_t first_seq, int k, const double *poses, int stride, float intensity, int64_t cap,
                             float *xyzi, int64_t *n_out) {
  if (!c || !l || !n_out || k < 0 || stride < 1 || cap < 0 || (k > 0 && !poses)) return VBA_ERR_BAD_ARG;
  *n_out = 0;
  if (l->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < k; i++) if (!kf_pose_ok(poses + 12 * i)) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  ScanLogView v;
  int st = scanlog_view(l, first_seq, k, INT32_MAX, nullptr, &v);   // the sizes first: cap is checked before any device work
  if (st) return st;
  std::vector<long long> &first = c->sat->exp.first;
  first.clear();
  long long total = 0;
  for (int i = 0; i < k; i++) { first.push_back(total); total += exp_count((long long)v.rel[i + 1] - v.rel[i], stride); }
  *n_out = total;
  if (total > cap || (total > 0 && !xyzi)) return VBA_ERR_BAD_ARG;
  if (total == 0) return VBA_OK;
  const bool dev_out = is_device_ptr(xyzi);
  if (dev_out && ((uintptr_t)xyzi & 15)) { c->set_error("vba_scanlog_export_world: a device xyzi must be 16-byte aligned"); return VBA_ERR_BAD_ARG; }
  if ((st = exp_ensure_tab(c, (size_t)k))) return st;
  if (!dev_out && (st = exp_ensure_out(c, (size_t)(total < kExpChunk ? total : kExpChunk)))) return st;
  if ((st = scanlog_view(l, first_seq, k, INT32_MAX, c->stream, &v))) return st;   // again, now ordering ctx's stream behind the captures
  const int slot = c->sat->exp.next;
  c->sat->exp.next = (slot + 1) % CtxSat::Exp::kRing;
  HIPCHK(c, hipEventSynchronize(c->sat->exp.ev[slot]));
  ExpKf *h = (ExpKf *)c->sat->exp.h[slot].p;
  for (int i = 0; i < k; i++) {
    h[i].first = first[i]; h[i].row = v.starts[i];
    std::memcpy(h[i].T, poses + 12 * (size_t)i, 12 * sizeof(double));
  }
  HIPCHK(c, hipMemcpyAsync(c->sat->exp.d, h, (size_t)k * sizeof(ExpKf), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->sat->exp.ev[slot], c->stream));
  const ExpKf *d_tab = (const ExpKf *)c->sat->exp.d.p;
  for (long long cb = 0; cb < total; cb += dev_out ? total : kExpChunk) {
    const long long ce = dev_out ? total : std::min(total, cb + kExpChunk);
    float4 *out = dev_out ? (float4 *)xyzi : c->sat->exp.d_out.p;
    // the rows of the table that records cb .. ce - 1 can touch: from the last scan with first <= cb
    const int g0 = (int)(std::upper_bound(first.begin(), first.end(), cb) - first.begin()) - 1;
    const long long nb = (ce - cb + 255) / 256;
    hipLaunchKernelGGL(k_kf_export, dim3((unsigned)std::min<long long>(nb, kExpMaxBlocks)), dim3(256), 0, c->stream, cb, ce - cb, k - g0, d_tab + g0, v.d_pnt,
                       stride, intensity, out);
    HIPCHK(c, hipGetLastError());
    if (!dev_out) HIPCHK(c, hipMemcpyAsync(xyzi + 4 * (size_t)cb, c->sat->exp.d_out, (size_t)(ce - cb) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  }
  if (!dev_out) HIPCHK(c, hipStreamSynchronize(c->stream));
  else if ((st = scanlog_reader_queued(l, c->stream))) return st;   // the gather is still queued: the next push waits for it
  return VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ voxel-down-sampled global map (vba_kf_voxel_export)
namespace {

inline size_t vx_slots(size_t pts) {                         // a power of two >= 2 pts
  size_t cap = 1024;
  while (cap < 2 * pts) cap <<= 1;
  return cap;
}
inline unsigned int vx_key_bits(size_t slots) {
  unsigned int b = 1;
  while (((size_t)1 << b) < slots) b++;
  return b;
}

// what this feature adds to the export's table and staging counts as its own
struct VxShared {
  vba_ctx *c; size_t tab, out;
  explicit VxShared(vba_ctx *c_) : c(c_), tab(c_->sat->exp.d.n), out(c_->sat->exp.d_out.n) {}
  ~VxShared() {
    if (c->sat->exp.d.n != tab) { c->sat->vx.allocs += 1 + CtxSat::Exp::kRing; c->sat->vx.bytes += (int64_t)c->sat->exp.d.n * (1 + CtxSat::Exp::kRing); }
    if (c->sat->exp.d_out.n != out) { c->sat->vx.allocs++; c->sat->vx.bytes += (int64_t)(c->sat->exp.d_out.n * sizeof(float4)); }
  }
};

template <class M>
int vx_grow(vba_ctx *c, M &m, size_t want) {
  if (want <= m.n) return VBA_OK;
  HIPCHK(c, m.ensure(want));
  c->sat->vx.allocs++; c->sat->vx.bytes += (int64_t)(want * sizeof(*m.p));
  return VBA_OK;
}

// the work arrays for a sequence of n records: as they are when they suffice, else doubled until they do, after a synchronise
int vx_ensure(vba_ctx *c, size_t n, bool exact) {
  auto &w = c->sat->vx;
  const bool det = c->opt.deterministic != 0;
  int st;
  if (n > w.pts) {
    size_t m = (exact || !w.pts) ? n : w.pts;
    while (m < n) m *= 2;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t slots = vx_slots(m);
    if ((st = vx_grow(c, w.tab, slots * sizeof(VxSlot))) || (st = vx_grow(c, w.sum, slots * 3)) || (st = vx_grow(c, w.slot, m)) ||
        (st = vx_grow(c, w.blk, (size_t)kVxBlocks + 1)) || (st = vx_grow(c, w.h_n, 1)))
      return st;
    w.pts = m;
  }
  if (det) {
    size_t tmp = 0;
    HIPCHK(c, sort_pairs_u32(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, w.pts, vx_key_bits(vx_slots(w.pts)), c->stream));
    if (w.sort_pts < w.pts || w.tmp_bytes < tmp) {
      const size_t stride = (w.pts * sizeof(int) + 255) & ~(size_t)255;
      HIPCHK(c, hipStreamSynchronize(c->stream));
      w.sort.reset();
      w.sort_pts = 0;
      if ((st = vx_grow(c, w.sort, 3 * stride + tmp))) return st;
      w.sort_pts = w.pts; w.sort_stride = stride; w.tmp_bytes = tmp;
    }
  }
  return VBA_OK;
}

// The front half that vba_kf_voxel_export and vba_kf_surfel_export share: the sequence S, the per-keyframe table through the export's
// upload ring, the table clear, the insert (with the sort and the chain sums of a deterministic context), the count, the scan and the
// one wait of the call.  r.n == 0: nothing to export, no device work was done.
struct VxFront { long long n = 0, per = 0, m = 0; size_t nk = 0; int nblk = 0; const VxKf *d_kft = nullptr; };
int vx_front(vba_ctx *c, int n_stores, vba_kf_store *const *stores, const float *intensity, int jump, double voxel_size, int min_count, VxFront &r) {
  // the sequence S: its length and its non-empty keyframes
  long long total = 0;
  size_t nk = 0;
  for (int s = 0; s < n_stores; s++) {
    const std::vector<int> &off = stores[s]->off;
    for (size_t k = 0; k + 1 < off.size(); k++)
      if (off[k + 1] > off[k]) { total += exp_count((long long)off[k + 1] - off[k], jump); nk++; }
  }
  if (total >= (1ll << 31) || nk > (size_t)(1 << 30)) return VBA_ERR_CAPACITY;
  if (total == 0) return VBA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if ((st = vx_ensure(c, (size_t)total, false))) return st;
  if ((st = exp_ensure_tab(c, (nk * sizeof(VxKf) + sizeof(ExpKf) - 1) / sizeof(ExpKf)))) return st;
  // the per-keyframe table through the export's upload ring
  const int ring = c->sat->exp.next;
  c->sat->exp.next = (ring + 1) % CtxSat::Exp::kRing;
  HIPCHK(c, hipEventSynchronize(c->sat->exp.ev[ring]));
  VxKf *h = (VxKf *)c->sat->exp.h[ring].p;
  {
    long long first = 0;
    size_t g = 0;
    for (int s = 0; s < n_stores; s++) {
      const vba_kf_store *S = stores[s];
      for (size_t k = 0; k + 1 < S->off.size(); k++) {
        if (S->off[k + 1] <= S->off[k]) continue;
        VxKf &e = h[g++];
        e.first = first; e.pnt = (const double *)S->d_pnt + 3 * (size_t)S->off[k]; e.inten = intensity[s]; e.pad = 0;
        std::memcpy(e.T, S->kf[k].x0, 12 * sizeof(double));
        first += exp_count((long long)S->off[k + 1] - S->off[k], jump);
      }
    }
  }
  HIPCHK(c, hipMemcpyAsync(c->sat->exp.d, h, nk * sizeof(VxKf), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->sat->exp.ev[ring], c->stream));
  const VxKf *d_kft = (const VxKf *)c->sat->exp.d.p;
  auto &w = c->sat->vx;
  const bool det = c->opt.deterministic != 0;
  const long long n = total, nb = (n + 255) / 256;
  const size_t slots = vx_slots((size_t)n);
  const unsigned int mask = (unsigned int)(slots - 1);
  VxSlot *tab = (VxSlot *)w.tab.p;
  const unsigned grid = (unsigned)std::min<long long>(nb, kExpMaxBlocks);
  hipLaunchKernelGGL(k_vx_clear, dim3((unsigned)std::min<size_t>(slots / 256, 4 * kExpMaxBlocks)), dim3(256), 0, c->stream, tab, slots);
  if (det) {
    unsigned int *skey = (unsigned int *)w.sort.p;
    int *idx = (int *)(w.sort.p + w.sort_stride), *sidx = (int *)(w.sort.p + 2 * w.sort_stride);
    hipLaunchKernelGGL(k_vx_insert<true>, dim3(grid), dim3(256), 0, c->stream, n, (int)nk, d_kft, jump, voxel_size, tab, mask, w.slot.p, (double *)nullptr);
    hipLaunchKernelGGL(k_iota, dim3((unsigned)nb), dim3(256), 0, c->stream, idx, (int)n);
    size_t tmp = w.tmp_bytes;
    HIPCHK(c, sort_pairs_u32(w.sort.p + 3 * w.sort_stride, tmp, w.slot.p, skey, idx, sidx, (size_t)n, vx_key_bits(slots), c->stream));
    hipLaunchKernelGGL(k_vx_sum_det, dim3((unsigned)nb), dim3(256), 0, c->stream, n, skey, sidx, tab, (int)nk, d_kft, jump, w.sum.p);
  } else {
    HIPCHK(c, hipMemsetAsync(w.sum.p, 0, slots * 3 * sizeof(double), c->stream));
    hipLaunchKernelGGL(k_vx_insert<false>, dim3(grid), dim3(256), 0, c->stream, n, (int)nk, d_kft, jump, voxel_size, tab, mask, w.slot.p, w.sum.p);
  }
  // count, scan, and the one wait of the call: the host needs the number of kept voxels
  const long long tiles = (nb + kVxBlocks - 1) / kVxBlocks, per = tiles * 256;
  const int nblk = (int)((nb + tiles - 1) / tiles);
  int *d_n = w.blk.p + kVxBlocks;
  hipLaunchKernelGGL(k_vx_count, dim3(nblk), dim3(256), 0, c->stream, n, per, tab, w.slot.p, min_count, w.blk.p);
  hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(256), 0, c->stream, nblk, w.blk.p, d_n);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(w.h_n.p, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  r.n = n; r.per = per; r.m = *w.h_n.p; r.nk = nk; r.nblk = nblk; r.d_kft = d_kft;
  return VBA_OK;
}

}  // namespace

extern "C" {

int vba_kf_voxel_export_reserve(vba_ctx *c, int64_t max_points) {
  if (!c || max_points < 0) return VBA_ERR_BAD_ARG;
  if (max_points >= ((int64_t)1 << 31)) return VBA_ERR_CAPACITY;
  if (max_points == 0) return VBA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  VxShared shared(c);
  int st;
  if ((st = vx_ensure(c, (size_t)max_points, true))) return st;
  if ((st = exp_ensure_tab(c, 1))) return st;
  return exp_ensure_out(c, (size_t)max_points + ((size_t)max_points + 3) / 4);     // a host result of max_points voxels: records, then counts
}

int vba_kf_voxel_export_allocations(vba_ctx *c, int *n_allocs, int64_t *bytes) {
  if (!c || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = c->sat->vx.allocs; *bytes = c->sat->vx.bytes;
  return VBA_OK;
}

int vba_kf_voxel_export(vba_ctx *c, int n_stores, vba_kf_store *const *stores, const float *intensity, int jump, double voxel_size, int min_count,
                        int64_t cap, float *xyzi, int *counts, int64_t *n_out) {
  if (!c || n_stores < 1 || !stores || !intensity || jump < 1 || min_count < 1 || cap < 0 || !n_out || (cap > 0 && !xyzi) || !(voxel_size >= 0.001))
    return VBA_ERR_BAD_ARG;
  for (int s = 0; s < n_stores; s++) if (!stores[s] || stores[s]->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  const bool query = cap == 0 && !xyzi;
  const bool dev_out = xyzi && is_device_ptr(xyzi);
  if (dev_out && ((uintptr_t)xyzi & 15)) { c->set_error("vba_kf_voxel_export: a device xyzi must be 16-byte aligned"); return VBA_ERR_BAD_ARG; }
  if (xyzi && counts && is_device_ptr(counts) != dev_out) { c->set_error("vba_kf_voxel_export: counts must be on the side of xyzi"); return VBA_ERR_BAD_ARG; }
  VxShared shared(c);
  VxFront r;
  int st;
  if ((st = vx_front(c, n_stores, stores, intensity, jump, voxel_size, min_count, r))) return st;
  auto &w = c->sat->vx;
  const long long n = r.n, per = r.per, m = r.m;
  const size_t nk = r.nk;
  const int nblk = r.nblk;
  const VxKf *d_kft = r.d_kft;
  VxSlot *tab = (VxSlot *)w.tab.p;
  *n_out = m;
  if (query) return VBA_OK;
  if (m > cap) return VBA_ERR_CAPACITY;
  if (m == 0) return VBA_OK;
  float4 *out = (float4 *)xyzi;
  int *cnt = counts;
  if (!dev_out) {
    if ((st = exp_ensure_out(c, (size_t)m + ((size_t)m + 3) / 4))) return st;
    out = c->sat->exp.d_out.p;
    cnt = counts ? (int *)(out + m) : nullptr;
  }
  hipLaunchKernelGGL(k_vx_emit, dim3(nblk), dim3(256), 0, c->stream, n, per, tab, w.slot.p, w.sum.p, min_count, w.blk.p, (int)nk, d_kft, out, cnt);
  HIPCHK(c, hipGetLastError());
  if (!dev_out) {
    HIPCHK(c, hipMemcpyAsync(xyzi, out, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (counts) HIPCHK(c, hipMemcpyAsync(counts, cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ surfel / NDT export of the global map (vba_kf_surfel_export)
namespace {

// the moment rows and row slots of `vox` kept voxels: as they are when they suffice, else doubled until they do, after a synchronise
int sf_ensure(vba_ctx *c, size_t vox, bool exact) {
  auto &w = c->sat->vx;
  if (vox <= w.sf_vox) return VBA_OK;
  size_t m = (exact || !w.sf_vox) ? vox : w.sf_vox;
  while (m < vox) m *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, w.sf_mom.ensure(m * 6));
  HIPCHK(c, w.sf_row.ensure(m));
  w.sf_allocs += 2; w.sf_bytes += (int64_t)(m * (6 * sizeof(double) + sizeof(int)));
  w.sf_vox = m;
  return VBA_OK;
}

// float4 entries of the export's staging for a host result of m voxels: records, then counts
inline size_t sf_staging(size_t m) { return 3 * m + (m + 3) / 4; }

}  // namespace

extern "C" {

int vba_kf_surfel_export_reserve(vba_ctx *c, int64_t max_points, int64_t max_voxels) {
  if (!c || max_points < 0 || max_voxels < 0) return VBA_ERR_BAD_ARG;
  if (max_points >= ((int64_t)1 << 31) || max_voxels >= ((int64_t)1 << 31)) return VBA_ERR_CAPACITY;
  if (max_points == 0 && max_voxels == 0) return VBA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  VxShared shared(c);
  int st;
  if (max_points > 0 && (st = vx_ensure(c, (size_t)max_points, true))) return st;
  if ((st = exp_ensure_tab(c, 1))) return st;
  if (max_voxels == 0) return VBA_OK;
  if ((st = sf_ensure(c, (size_t)max_voxels, true))) return st;
  return exp_ensure_out(c, sf_staging((size_t)max_voxels));
}

int vba_kf_surfel_export_allocations(vba_ctx *c, int *n_allocs, int64_t *bytes) {
  if (!c || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = c->sat->vx.allocs + c->sat->vx.sf_allocs; *bytes = c->sat->vx.bytes + c->sat->vx.sf_bytes;
  return VBA_OK;
}

int vba_kf_surfel_export(vba_ctx *c, int n_stores, vba_kf_store *const *stores, const float *intensity, int jump, double voxel_size, int min_count,
                         int64_t cap, float *surfels, double *cov, int *counts, int64_t *n_out) {
  if (!c || n_stores < 1 || !stores || !intensity || jump < 1 || min_count < 1 || cap < 0 || !n_out || (cap > 0 && !surfels) || !(voxel_size >= 0.001))
    return VBA_ERR_BAD_ARG;
  for (int s = 0; s < n_stores; s++) if (!stores[s] || stores[s]->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  const bool query = cap == 0 && !surfels;
  const bool dev_out = surfels && is_device_ptr(surfels);
  if (dev_out && ((uintptr_t)surfels & 15)) { c->set_error("vba_kf_surfel_export: a device surfels must be 16-byte aligned"); return VBA_ERR_BAD_ARG; }
  if (surfels && cov && is_device_ptr(cov) != dev_out) { c->set_error("vba_kf_surfel_export: cov must be on the side of surfels"); return VBA_ERR_BAD_ARG; }
  if (dev_out && cov && ((uintptr_t)cov & 7)) { c->set_error("vba_kf_surfel_export: a device cov must be 8-byte aligned"); return VBA_ERR_BAD_ARG; }
  if (surfels && counts && is_device_ptr(counts) != dev_out) { c->set_error("vba_kf_surfel_export: counts must be on the side of surfels"); return VBA_ERR_BAD_ARG; }
  VxShared shared(c);
  VxFront r;
  int st;
  if ((st = vx_front(c, n_stores, stores, intensity, jump, voxel_size, min_count, r))) return st;
  const long long m = r.m;
  *n_out = m;
  if (query) return VBA_OK;
  if (m > cap) return VBA_ERR_CAPACITY;
  if (m == 0) return VBA_OK;
  if ((st = sf_ensure(c, (size_t)m, false))) return st;
  if (!dev_out && (st = exp_ensure_out(c, sf_staging((size_t)m)))) return st;
  auto &w = c->sat->vx;
  const bool det = c->opt.deterministic != 0;
  SfPass p;
  p.n = r.n; p.per = r.per; p.nblk = r.nblk; p.nkf = (int)r.nk; p.jump = jump; p.min_count = min_count; p.m = (int)m;
  p.kft = r.d_kft; p.tab = (VxSlot *)w.tab.p; p.slot_of = w.slot.p; p.sum = w.sum.p; p.blk = w.blk.p;
  p.skey = det ? (const unsigned int *)w.sort.p : nullptr;
  p.sidx = det ? (const int *)(w.sort.p + 2 * w.sort_stride) : nullptr;
  p.slot_of_row = w.sf_row.p; p.mom = w.sf_mom.p;
  // a host result: the records and counts through the export's staging, the covariances in place of the moment rows
  float4 *out = dev_out ? (float4 *)surfels : c->sat->exp.d_out.p;
  double *dcov = dev_out ? cov : (cov ? w.sf_mom.p : nullptr);
  int *cnt = dev_out ? counts : (counts ? (int *)(out + 3 * m) : nullptr);
  HIPCHK(c, (hipError_t)sf_run(p, kExpMaxBlocks, out, dcov, cnt, c->stream));
  if (!dev_out) {
    HIPCHK(c, hipMemcpyAsync(surfels, out, (size_t)m * 12 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (cov) HIPCHK(c, hipMemcpyAsync(cov, dcov, (size_t)m * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (counts) HIPCHK(c, hipMemcpyAsync(counts, cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VBA_OK;
}

}  // extern "C"
