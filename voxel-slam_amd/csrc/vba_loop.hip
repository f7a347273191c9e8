// Loop-closure map of libvoxelba.so (vba_loop_map_*, vba_loop_update): host code over the map's host API (vba_map.hip)
// and the keyframe store (vba_kf.hip).
#include "vba_ctx.hpp"
#include "vba_kf_store.hpp"
#include "vba_scanlog.hpp"

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

// ------------------------------------------------------------------------------------------------ loop-closure map (vba_loop_map_*, vba_loop_update)

struct vba_loop_map {
  vba_ctx *ctx = nullptr;
  MapStore map;                                  // map_loop; after vba_loop_update the map the context gave up (ping-pong)
  size_t res_fix = 0, res_nodes = 0;             // vba_loop_map_reserve: applied to whichever store the object owns
  // segment table int4 [tcap] + poses double [tcap][12]: pinned image and device copy
  int tcap = 0; PinMem<char> h_tab; DevMem<char> d_tab;
  DevMem<char> d_in;                             // host-memory scans of vba_loop_update on their way to the device
  int allocs = 0; int64_t bytes = 0;
};

namespace {

size_t lm_tab_bytes(int t) { return (size_t)t * (sizeof(int4) + 12 * sizeof(double)); }

// device bytes behind a MapStore, from its capacities (what grows when a call allocates)
int64_t lm_store_bytes(MapStore &s) {
  if (!s.allocated) return 0;
  const int W = s.opt.win_size;
  size_t b = 0;
  for (auto &a : node_arrays(s.v, W)) b += a.elem * a.rows * (size_t)s.v.cap;
  for (auto &a : scan_arrays(s.v, W)) b += a.elem * a.rows * (size_t)s.v.max_pts;
  for (auto &a : fix_arrays(s.v)) b += a.elem * a.rows * (size_t)s.v.cap_fix;
  b += (size_t)s.hcap * (s.det ? 16 : 12) + s.d_stage.n + s.d_sort_tmp.n + s.d_whist.n * sizeof(int);
  return (int64_t)b;
}

// allocations made by the calls on this object: every store the call may have grown is measured around it
struct LmAccount {
  vba_loop_map *lm; MapStore *a, *b; int64_t before;
  LmAccount(vba_loop_map *l, MapStore *x, MapStore *y = nullptr) : lm(l), a(x), b(y), before(lm_store_bytes(*x) + (y ? lm_store_bytes(*y) : 0)) {}
  ~LmAccount() {
    const int64_t after = lm_store_bytes(*a) + (b ? lm_store_bytes(*b) : 0);
    if (after != before) { lm->allocs++; lm->bytes += after - before; }
  }
};

int lm_ensure_tab(vba_loop_map *lm, int t) {
  if (t <= lm->tcap) return VBA_OK;
  vba_ctx *c = lm->ctx;
  int m = lm->tcap ? lm->tcap : 64;
  while (m < t) m *= 2;
  HIPCHK(c, hipDeviceSynchronize());
  lm->tcap = 0;
  HIPCHK(c, lm->h_tab.ensure(lm_tab_bytes(m)));
  HIPCHK(c, lm->d_tab.ensure(lm_tab_bytes(m)));
  lm->allocs += 2; lm->bytes += (int64_t)lm_tab_bytes(m);
  lm->tcap = m;
  return VBA_OK;
}
int lm_ensure_in(vba_loop_map *lm, size_t bytes) {
  if (bytes <= lm->d_in.n) return VBA_OK;
  vba_ctx *c = lm->ctx;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, lm->d_in.ensure(bytes));
  lm->allocs++; lm->bytes += (int64_t)bytes;
  return VBA_OK;
}
int4 *lm_h_seg(vba_loop_map *lm) { return (int4 *)lm->h_tab.p; }
double *lm_h_pose(vba_loop_map *lm) { return (double *)(lm->h_tab + (size_t)lm->tcap * sizeof(int4)); }
const int4 *lm_d_seg(vba_loop_map *lm) { return (const int4 *)lm->d_tab.p; }
const double *lm_d_pose(vba_loop_map *lm) { return (const double *)(lm->d_tab + (size_t)lm->tcap * sizeof(int4)); }

// the reservation on the store the object owns now
int lm_apply_reserve(vba_loop_map *lm, hipStream_t st, std::string &err) {
  if (!lm->res_fix && !lm->res_nodes) return VBA_OK;
  MapStore &s = lm->map;
  int r = map_base(s, st, err);
  if (r) return r;
  if (s.cnt_stale) { r = map_read_counters(s, st, err); if (r) return r; }
  return map_fix_source_ensure(s, st, lm->res_nodes, lm->res_fix, lm->res_fix, err);
}

bool lm_same_map_options(const vba_options &a, const vba_options &b) {
  if (a.win_size != b.win_size || a.voxel_size != b.voxel_size || a.max_layer != b.max_layer || a.max_points != b.max_points ||
      a.min_eigen_value != b.min_eigen_value || a.thread_num != b.thread_num || (a.deterministic != 0) != (b.deterministic != 0))
    return false;
  for (int i = 0; i < 4; i++) if (a.plane_eigen_value_thre[i] != b.plane_eigen_value_thre[i] || a.min_point[i] != b.min_point[i]) return false;
  return true;
}

// The two maps trade places.  What belongs to a context stays with it: its options, its shard and its all-reduce closure; buffers
// (arrays, staging, pose ring, pinned counters, sort scratch) travel with the store: they are memory of the device, not of a stream.
void lm_swap_stores(MapStore &a, MapStore &b) {
  std::swap(a, b);
  std::swap(a.opt, b.opt); std::swap(a.rank, b.rank); std::swap(a.n_ranks, b.n_ranks); std::swap(a.allreduce, b.allreduce);
}

bool lm_finite(const double *p, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; }

}  // namespace

extern "C" {

int vba_loop_map_create(vba_ctx *c, vba_loop_map **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  vba_loop_map *lm = new vba_loop_map();
  lm->ctx = c;
  map_init(lm->map, c->opt);
  const int st = lm_ensure_tab(lm, 64);
  if (st) { vba_loop_map_destroy(lm); return st; }
  *out = lm;
  return VBA_OK;
}

void vba_loop_map_destroy(vba_loop_map *lm) {
  if (!lm) return;
  hipSetDevice(lm->ctx->device);
  hipStreamSynchronize(lm->ctx->stream);
  map_free(lm->map);
  delete lm;
}

int vba_loop_map_reserve(vba_loop_map *lm, int64_t fix_points, int64_t nodes) {
  if (!lm || fix_points < 0 || nodes < 0 || fix_points > ((int64_t)1 << 27) || nodes > ((int64_t)1 << 28)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = lm->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if ((size_t)fix_points > lm->res_fix) lm->res_fix = (size_t)fix_points;
  if ((size_t)nodes > lm->res_nodes) lm->res_nodes = (size_t)nodes;
  int st;
  {
    LmAccount acc(lm, &lm->map);
    st = lm_apply_reserve(lm, c->stream, c->err);
  }
  if (!st) st = lm_ensure_in(lm, lm->res_fix * 96);
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_loop_map_allocations(vba_loop_map *lm, int *count, int64_t *bytes) {
  if (!lm || !count || !bytes) return VBA_ERR_BAD_ARG;
  *count = lm->allocs; *bytes = lm->bytes;
  return VBA_OK;
}

int vba_loop_map_build(vba_loop_map *lm, vba_kf_store *s, int init_num, int cumulative, int *n_inserted) {
  if (!lm || !s || !n_inserted || init_num < 1 || init_num > 64) return VBA_ERR_BAD_ARG;
  *n_inserted = 0;
  vba_ctx *c = lm->ctx;
  if (s->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int size = (int)s->kf.size();
  const int first = size - init_num > 0 ? size - init_num : 0, m = size - first;       // indices below zero are skipped (VS:2607-2608)
  const int nseg = cumulative ? m * (m + 1) / 2 : m;
  int st;
  if ((st = lm_ensure_tab(lm, nseg > m ? nseg : (m > 0 ? m : 1)))) return st;
  // pvec_tem is never cleared (VS:2602): call j inserts keyframes first .. first + j again
  int4 *seg = lm_h_seg(lm);
  double *hp = lm_h_pose(lm);
  long long n = 0;
  int ns = 0;
  for (int j = 0; j < m; j++)                               // insertion j of the reference: keyframes 0 .. j (corrected form: j alone)
    for (int i = cumulative ? 0 : j; i <= j; i++) {
      seg[ns++] = make_int4((int)n, s->off[first + i], i, 0);
      n += s->off[first + i + 1] - s->off[first + i];
    }
  for (int i = 0; i < m; i++) std::memcpy(hp + 12 * i, s->kf[first + i].x0, 12 * sizeof(double));
  if (n > ((long long)1 << 27)) return VBA_ERR_CAPACITY;
  LmAccount acc(lm, &lm->map);
  if ((st = map_reset(lm->map, c->stream, c->err))) return st;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(lm->d_tab, lm->h_tab, lm_tab_bytes(lm->tcap), hipMemcpyHostToDevice, c->stream));
    FixSource src;
    src.nseg = ns; src.d_seg = lm_d_seg(lm); src.d_poses = lm_d_pose(lm); src.d_pnt = s->d_pnt; src.cov_kind = FIXCOV_DIAG_F32; src.d_cov = s->d_var;
    st = map_cut_voxel_fix_source(lm->map, c->stream, (int)n, src, 0.0, c->err);       // ends with the counter read-back: the map is complete
    if (st) { hipStreamSynchronize(c->stream); map_reset(lm->map, c->stream, c->err); return st; }
  }
  for (int i = 0; i < m; i++) s->kf[first + i].exist = 0;                               // VS:2612
  *n_inserted = (int)n;
  return VBA_OK;
}

int vba_loop_map_num_roots(vba_loop_map *lm) { return lm ? map_num_roots(lm->map, lm->ctx->stream, false) : -1; }
int vba_loop_map_dump_leaves(vba_loop_map *lm, double *out, int max_leaves) { return lm ? map_dump_leaves(lm->map, lm->ctx->stream, out, max_leaves, lm->ctx->err) : -1; }
int vba_loop_map_dump_plane_var(vba_loop_map *lm, double *out, int max_leaves) { return lm ? map_dump_plane_var(lm->map, lm->ctx->stream, out, max_leaves, lm->ctx->err) : -1; }

}  // extern "C"
namespace {

// vba_loop_update.  log == nullptr: the buf_lba2loop scans are rows offsets[i] .. offsets[i + 1] of pnt / var.  Otherwise they are
// scans first .. first + k - 1 of the scan log, each read at its own arena start (vba_scanlog_loop_update).
int loop_update_scans(vba_ctx *c, vba_loop_map *lm, const double *dx12, int k, const int *offsets, const double *pnt, const double *var,
                      vba_scanlog *log, int64_t first, const double *poses_bl, int win_count, const double *win_pnt, const double *win_var,
                      const int *win_offsets, const double *poses_win, int *n_factors) {
  // ---- 1. arguments, before any device work
  if (!c || !lm || !n_factors || !poses_win || k < 0) return VBA_ERR_BAD_ARG;
  *n_factors = 0;
  const int W = c->opt.win_size;
  if (win_count < 1 || win_count > W) { c->set_error("vba_loop_update: win_count outside 1..win_size"); return VBA_ERR_BAD_ARG; }
  if (lm->ctx->device != c->device) { c->set_error("vba_loop_update: the loop map is on another device"); return VBA_ERR_BAD_ARG; }
  if (!lm_same_map_options(lm->map.opt, c->opt)) { c->set_error("vba_loop_update: the loop map was created with other map options"); return VBA_ERR_BAD_ARG; }
  if (c->n_ranks > 1 || c->map.n_ranks > 1 || lm->map.n_ranks > 1 || c->rank != 0) { c->set_error("vba_loop_update: sharded maps are not supported"); return VBA_ERR_UNSUPPORTED; }
  if (dx12 && !lm_finite(dx12, 12)) return VBA_ERR_BAD_ARG;
  if (!lm_finite(poses_win, 12 * (size_t)win_count)) return VBA_ERR_BAD_ARG;
  ScanLogView lv;
  if (log) {
    if (log->ctx->device != c->device) { c->set_error("vba_scanlog_loop_update: the scan log is on another device"); return VBA_ERR_BAD_ARG; }
    if (scanlog_view(log, first, k, 1ll << 27, nullptr, &lv)) { c->set_error("vba_scanlog_loop_update: the scans are not all live, or hold more than 2^27 points"); return VBA_ERR_BAD_ARG; }
    offsets = lv.rel.data(); pnt = lv.d_pnt; var = lv.d_var;
  }
  long long n_bl = 0;
  if (k > 0) {
    if (!offsets || !poses_bl || !lm_finite(poses_bl, 12 * (size_t)k)) return VBA_ERR_BAD_ARG;
    for (int i = 0; i < k; i++) if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
    n_bl = (long long)offsets[k] - offsets[0];
    if (n_bl > ((long long)1 << 27)) return VBA_ERR_CAPACITY;
    if (n_bl > 0 && !pnt) return VBA_ERR_BAD_ARG;
  }
  if (win_pnt) {
    if (!win_offsets) return VBA_ERR_BAD_ARG;
    for (int i = 0; i < win_count; i++) if (win_offsets[i] < 0 || win_offsets[i + 1] < win_offsets[i]) return VBA_ERR_BAD_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  int r;
  if ((r = lm_ensure_tab(lm, k > 0 ? k : 1))) { c->set_error(lm->ctx->err); return r; }
  const bool bl_host = n_bl > 0 && !log && !is_device_ptr(pnt);
  if (log && n_bl > 0 && (r = scanlog_view(log, first, k, 1ll << 27, st, &lv))) return r;     // this stream behind the captures
  if (bl_host && (r = lm_ensure_in(lm, (size_t)n_bl * (var ? 96 : 24)))) { c->set_error(lm->ctx->err); return r; }
  HIPCHK(c, hipStreamSynchronize(lm->ctx->stream));          // (the build ended with a synchronise; a dump on that stream may not have)
  LmAccount acc(lm, &lm->map, &c->map);
  // ---- 2. the context adopts map_loop (surf_map = map_loop, VS:1275-1276); the outgoing map stays readable until the end
  lm_swap_stores(c->map, lm->map);
  MapStore &old = lm->map;
  for (int i = 0; i < VBA_MAX_WIN; i++) c->map.mp[i] = i;    // VS:1334-1335
  auto fail = [&](int code) {                                // the context gets its map back untouched; the loop map has to be built again
    hipStreamSynchronize(st);
    const std::string why = c->err;
    lm_swap_stores(c->map, lm->map);
    std::string e2;
    map_reset(lm->map, st, e2);
    c->set_error(why + " (vba_loop_update: the context's map is unchanged, the loop map was reset)");
    return code;
  };
  // ---- 3. the buf_lba2loop scans: one fixed insertion with their covariances at jour = 0 (VS:1338-1347)
  if (n_bl > 0) {
    const int off0 = offsets[0];
    int4 *seg = lm_h_seg(lm);
    for (int i = 0; i < k; i++) seg[i] = make_int4(offsets[i] - off0, log ? lv.starts[i] : offsets[i] - off0, i, 0);
    std::memcpy(lm_h_pose(lm), poses_bl, 12 * sizeof(double) * (size_t)k);
    if (hipMemcpyAsync(lm->d_tab, lm->h_tab, lm_tab_bytes(lm->tcap), hipMemcpyHostToDevice, st) != hipSuccess) { c->set_error("vba_loop_update: table upload failed"); return fail(VBA_ERR_HIP); }
    const double *d_p = pnt + 3 * (size_t)off0, *d_v = var ? var + 9 * (size_t)off0 : nullptr;
    if (bl_host) {
      hipError_t e = hipMemcpyAsync(lm->d_in, d_p, (size_t)n_bl * 24, hipMemcpyHostToDevice, st);
      if (e == hipSuccess && var) e = hipMemcpyAsync(lm->d_in + (size_t)n_bl * 24, d_v, (size_t)n_bl * 72, hipMemcpyHostToDevice, st);
      if (e != hipSuccess) { c->set_error("vba_loop_update: scan upload failed"); return fail(VBA_ERR_HIP); }
      d_p = (const double *)lm->d_in.p; d_v = var ? (const double *)(lm->d_in + (size_t)n_bl * 24) : nullptr;
    }
    FixSource src;
    src.nseg = k; src.d_seg = lm_d_seg(lm); src.d_poses = lm_d_pose(lm); src.d_pnt = d_p;
    src.cov_kind = d_v ? FIXCOV_FULL_F64 : FIXCOV_ZERO; src.d_cov = d_v;
    if ((r = map_cut_voxel_fix_source(c->map, st, (int)n_bl, src, 0.0, c->err))) return fail(r);
  }
  // ---- 4. the window's scans again: cut_voxel at frame i with the moved pose (VS:1350-1359)
  for (int i = 0; i < win_count; i++) {
    const double *p, *v; int n;
    if (win_pnt) {
      n = win_offsets[i + 1] - win_offsets[i];
      p = win_pnt + 3 * (size_t)win_offsets[i]; v = win_var ? win_var + 9 * (size_t)win_offsets[i] : nullptr;
    } else {                                                  // the outgoing map's scan ring: raw body points and covariances as inserted
      const int slot = old.mp[i];
      n = old.npts[slot];
      p = n > 0 ? old.v.px + (size_t)slot * old.v.max_pts * 3 : nullptr;
      v = n > 0 && old.have_var ? old.v.pvar + (size_t)slot * old.v.max_pts * 9 : nullptr;
    }
    if ((r = map_cut_voxel(c->map, st, i, n, p, v, poses_win + 12 * (size_t)i, false, c->err))) return fail(r);
  }
  // ---- 5. recut over all roots (VS:1362-1363), with vba_map_recut's factor extraction
  if ((r = vba_map_recut(c, win_count, poses_win, 0))) return fail(r);
  *n_factors = c->nvox;
  // ---- 6. the outgoing map is emptied and keeps its allocations for the next loop closure
  std::string e2;
  r = map_reset(old, st, e2);
  if (!r) r = lm_apply_reserve(lm, st, e2);
  if (!r && old.hcap != c->map.hcap) {                         // both tables at the larger size: the capacities stop moving after one cycle
    MapStore &small = old.hcap < c->map.hcap ? old : c->map;
    const unsigned int big = old.hcap < c->map.hcap ? c->map.hcap : old.hcap;
    if (small.allocated) {
      if (small.cnt_stale) r = map_read_counters(small, st, e2);
      if (!r) r = map_hash_alloc(small, big, st, e2);
    }
  }
  if (r) { c->set_error("vba_loop_update: the context holds the new map; resetting the outgoing map failed: " + e2); return r; }
  return VBA_OK;
}

}  // namespace
extern "C" {

int vba_loop_update(vba_ctx *c, vba_loop_map *lm, const double *dx12, int k, const int *offsets, const double *pnt, const double *var, const double *poses_bl,
                    int win_count, const double *win_pnt, const double *win_var, const int *win_offsets, const double *poses_win, int *n_factors) {
  return loop_update_scans(c, lm, dx12, k, offsets, pnt, var, nullptr, 0, poses_bl, win_count, win_pnt, win_var, win_offsets, poses_win, n_factors);
}

int vba_scanlog_loop_update(vba_ctx *c, vba_loop_map *lm, const double *dx12, vba_scanlog *l, int64_t first, int k, const double *poses_bl,
                            int win_count, const double *poses_win, int *n_factors) {
  if (!l) return VBA_ERR_BAD_ARG;
  return loop_update_scans(c, lm, dx12, k, nullptr, nullptr, nullptr, l, first, poses_bl, win_count, nullptr, nullptr, nullptr, poses_win, n_factors);
}

}  // extern "C"
