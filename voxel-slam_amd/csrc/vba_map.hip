// The voxel map of libvoxelba.so: the kernels of vba_kernels_map.hpp, vba_kernels_loop.hpp and vba_kernels_odom.hpp (the resident EKF
// loop runs the map's point loop), compiled here and nowhere else, and the map_* host functions that launch them; the other units reach
// the map through the declarations in vba_ctx.hpp.
#include "vba_ctx.hpp"
#include "vba_odom_state_decl.hpp"
#include "vba_kernels_map.hpp"
#include "vba_kernels_loop.hpp"
#include "vba_kernels_odom.hpp"
#include <cstddef>

namespace vba {

// ================================================================================================ the map's host functions
void map_init(MapStore &s, const vba_options &o) {
  s.opt = o;
  s.det = o.deterministic != 0;
  for (int i = 0; i < VBA_MAX_WIN; i++) { s.mp[i] = i; s.npts[i] = 0; }   // VS:3158-3160
}

inline MapParams map_params(const MapStore &s) {
  MapParams P;
  P.W = s.opt.win_size; P.max_layer = s.opt.max_layer; P.max_points = s.opt.max_points; P.thread_num = s.opt.thread_num;
  P.voxel_size = s.opt.voxel_size; P.min_eigen_value = s.opt.min_eigen_value;
  for (int i = 0; i < 4; i++) { P.plane_thre[i] = s.opt.plane_eigen_value_thre[i]; P.min_point[i] = s.opt.min_point[i]; }
  if (s.thr_override) {
    P.min_eigen_value = s.ovr_min_eigen_value;
    for (int i = 0; i < 4; i++) P.plane_thre[i] = s.ovr_plane_thre[i];
  }
  for (int i = 0; i < VBA_MAX_WIN; i++) P.mp[i] = s.mp[i];
  P.rank = s.rank; P.n_ranks = s.n_ranks;
  return P;
}

std::vector<DevArr> node_arrays(MapView &v, int W) {
  return {
      {(void **)&v.nkey, 8, 1}, {(void **)&v.nroot, 4, 1}, {(void **)&v.nparent, 4, 1}, {(void **)&v.nchild, 4, 1}, {(void **)&v.npath, 4, 1},
      {(void **)&v.nopt, 4, 1}, {(void **)&v.nflist, 4, 1}, {(void **)&v.nfl2, 4, 1}, {(void **)&v.nfkey, 4, 1}, {(void **)&v.nlast, 4, 1}, {(void **)&v.nstamp, 4, 1}, {(void **)&v.nsplit, 4, 1}, {(void **)&v.ntake, 4, 1},
      {(void **)&v.nclear, 4, 1}, {(void **)&v.ndead, 4, 1}, {(void **)&v.nfree_root, 4, 1}, {(void **)&v.nfree_blk, 4, 1}, {(void **)&v.ndet, 4, 1}, {(void **)&v.dblk, 4, 1},
      {(void **)&v.nseg_a, 4, (size_t)W}, {(void **)&v.nseg_b, 4, (size_t)W}, {(void **)&v.nsl, 4, 1}, {(void **)&v.ncnt, 4, 1}, {(void **)&v.nfb_head, 4, 1}, {(void **)&v.nfb_tail, 4, 1}, {(void **)&v.nlayer, 1, 1}, {(void **)&v.nstate, 1, 1}, {(void **)&v.f_exist, 1, 1},
      {(void **)&v.f_sw, 1, 1}, {(void **)&v.f_plane, 1, 1}, {(void **)&v.f_touched, 1, 1}, {(void **)&v.f_slide, 4, 1}, {(void **)&v.nql, 4, 1},
      {(void **)&v.ncenter, 8, 3}, {(void **)&v.njour, 8, 1}, {(void **)&v.nadd, 80, 1}, {(void **)&v.nfix, 80, 1}, {(void **)&v.ncov, 360, 1},
      {(void **)&v.neval, 24, 1}, {(void **)&v.nevec, 72, 1}, {(void **)&v.nplane, 8, 43}, {(void **)&v.nlc, (size_t)80 * W, 1},
  };
}
std::vector<DevArr> scan_arrays(MapView &v, int W) {
  return {{(void **)&v.px, 24, (size_t)W}, {(void **)&v.pvar, 72, (size_t)W}, {(void **)&v.pnode, 4, (size_t)W}, {(void **)&v.phash, 4, 1}, {(void **)&v.newslots, 4, 1},
          {(void **)&v.perm, 4, (size_t)W}, {(void **)&v.sx, 24, (size_t)W}, {(void **)&v.svar, 72, (size_t)W}, {(void **)&v.pleaf, 4, (size_t)W}, {(void **)&v.skey_a, 4, 1}, {(void **)&v.skey_b, 4, 1}, {(void **)&v.sval_a, 4, 1}, {(void **)&v.sval_b, 4, 1}, {(void **)&v.wl, 4, 1}, {(void **)&v.wlb, 4, 1}, {(void **)&v.wl4, 16, 1}};
}
std::vector<DevArr> fix_arrays(MapView &v) {
  return {{(void **)&v.fx, 24, 1}, {(void **)&v.fvar, 72, 1}, {(void **)&v.fnode, 4, 1}, {(void **)&v.fb_base, 4, 1}, {(void **)&v.fb_len, 4, 1}, {(void **)&v.fb_next, 4, 1}};
}

// grow a family of [rows][cap] arrays from oldcap to newcap, keeping the first `used` columns; new space zero-filled.  All or nothing
// (grow_family, vba_mem.hpp): after a failure the owners and the view slots are as they were, under the capacity the caller still records
inline int grow_arrays(std::vector<DevMem<char>> &own, const std::vector<DevArr> &arrs, size_t oldcap, size_t newcap, size_t used, hipStream_t st, std::string &err) {
  VBA_HIPCHK(err, grow_family(own, arrs, oldcap, newcap, used, st));
  for (size_t i = 0; i < arrs.size(); i++) *arrs[i].slot = own[i].p;
  return VBA_OK;
}

int map_read_counters(MapStore &s, hipStream_t st, std::string &err) {
  hipLaunchKernelGGL(k_words_to_host, dim3(1), dim3(64), 0, st, s.v.cnt, s.h_cnt.p, (int)CNT_N);
  VBA_HIPCHK(err, hipGetLastError());
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  s.ub_nodes = s.h_cnt[CNT_NODES]; s.ub_roots = s.h_cnt[CNT_ROOTS]; s.ub_used = s.h_cnt[CNT_USED]; s.cnt_stale = false;
  return VBA_OK;
}

int map_hash_alloc(MapStore &s, unsigned int cap, hipStream_t st, std::string &err) {
  // the new table is built in locals and adopted at the end: an early return frees it and leaves the map on its old one
  DevMem<unsigned long long> nk; DevMem<int> nv; DevMem<unsigned int> nf;
  VBA_HIPCHK(err, nk.ensure(cap));
  VBA_HIPCHK(err, nv.ensure(cap));
  if (s.det) {   // (no insert is in flight between calls: every slot reads DET_NONE)
    VBA_HIPCHK(err, nf.ensure(cap));
    VBA_HIPCHK(err, hipMemsetAsync(nf.p, 0x7F, (size_t)cap * 4, st));
  }
  hipLaunchKernelGGL(k_fill_u64, dim3(1024), dim3(256), 0, st, nk.p, KEY_EMPTY, (size_t)cap);
  VBA_HIPCHK(err, hipMemsetAsync(nv.p, 0xFF, (size_t)cap * 4, st));
  if (s.hkeys) {
    hipLaunchKernelGGL(k_rehash, dim3((s.hcap + 255) / 256), dim3(256), 0, st, s.v.hkeys, s.v.hvals, s.v.hmask, nk.p, nv.p, cap - 1);
    hipLaunchKernelGGL(k_copy_counter, dim3(1), dim3(1), 0, st, s.v.cnt, (int)CNT_ROOTS, (int)CNT_USED);   // the tombstones are gone
    VBA_HIPCHK(err, hipStreamSynchronize(st));   // (before the moves below free the old table)
    s.ub_used = s.ub_roots;
  }
  s.hkeys = std::move(nk); s.hvals = std::move(nv); s.hfirst = std::move(nf);
  s.v.hkeys = s.hkeys; s.v.hvals = s.hvals; s.v.hfirst = s.hfirst; s.v.hmask = cap - 1; s.hcap = cap;
  return VBA_OK;
}

int map_base(MapStore &s, hipStream_t st, std::string &err) {
  if (s.allocated) return VBA_OK;
  VBA_HIPCHK(err, s.cnt.ensure(CNT_N));
  VBA_HIPCHK(err, s.fhist.ensure(EXTRACT_NB_MAX));
  VBA_HIPCHK(err, hipMemsetAsync(s.cnt.p, 0, CNT_N * sizeof(int), st));
  VBA_HIPCHK(err, s.poses.ensure(VBA_MAX_WIN * 12));
  VBA_HIPCHK(err, s.h_cnt.ensure(CNT_N + 16));
  std::memset(s.h_cnt.p, 0, CNT_N * sizeof(int) + 64);
  s.v.cnt = s.cnt; s.v.fhist = s.fhist; s.v.poses = s.poses;
  // initial root table: 2^20 slots, or (with the max_points_per_scan capacity hint) the power of two above 4x the hint
  unsigned int hc = 1u << 20;
  if (s.opt.max_points_per_scan) { hc = 1u << 10; while ((size_t)hc < 4 * s.opt.max_points_per_scan && hc < (1u << 30)) hc *= 2; }
  int st2 = map_hash_alloc(s, hc, st, err);
  if (st2) return st2;
  s.allocated = true;
  return VBA_OK;
}

inline int map_ensure(MapStore &s, hipStream_t st, size_t need_nodes, size_t need_pts, size_t need_fix, std::string &err) {
  const int W = s.opt.win_size;
  int rb = map_base(s, st, err);
  if (rb) return rb;
  // capacity hints of vba_options: taken at the first allocation of each array family
  if (s.v.cap == 0 && need_nodes > 0 && s.opt.max_map_nodes > need_nodes) need_nodes = s.opt.max_map_nodes;
  if (s.v.max_pts == 0 && need_pts > 0 && s.opt.max_points_per_scan > need_pts) need_pts = s.opt.max_points_per_scan;
  if (s.v.cap_fix == 0 && need_fix > 0 && s.opt.max_fix_points > need_fix) need_fix = s.opt.max_fix_points;
  if (need_nodes > (size_t)s.v.cap) {
    size_t nc = s.v.cap ? (size_t)s.v.cap : (size_t)1 << 18;
    while (nc < need_nodes) nc *= 2;
    int r = grow_arrays(s.node_mem, node_arrays(s.v, W), (size_t)s.v.cap, nc, (size_t)s.v.cap, st, err);
    if (r) return r;
    s.v.cap = (int)nc;
  }
  if (need_pts > (size_t)s.v.max_pts) {
    size_t nc = s.v.max_pts ? (size_t)s.v.max_pts : (size_t)1 << 16;
    while (nc < need_pts) nc *= 2;
    int r = grow_arrays(s.scan_mem, scan_arrays(s.v, W), (size_t)s.v.max_pts, nc, (size_t)s.v.max_pts, st, err);
    if (r) return r;
    if (s.v.max_pts == 0) { VBA_HIPCHK(err, hipMemsetAsync(s.v.pnode, 0xFF, (size_t)W * nc * 4, st)); VBA_HIPCHK(err, hipMemsetAsync(s.v.pleaf, 0xFF, (size_t)W * nc * 4, st)); }
    else {  // new tail of every slot must read "no node"
      for (int sl = 0; sl < W; sl++) {
        VBA_HIPCHK(err, hipMemsetAsync(s.v.pnode + (size_t)sl * nc + s.v.max_pts, 0xFF, (nc - s.v.max_pts) * 4, st));
        VBA_HIPCHK(err, hipMemsetAsync(s.v.pleaf + (size_t)sl * nc + s.v.max_pts, 0xFF, (nc - s.v.max_pts) * 4, st));
      }
    }
    s.v.max_pts = (int)nc;
  }
  if (need_fix > (size_t)s.v.cap_fix) {
    size_t nc = s.v.cap_fix ? (size_t)s.v.cap_fix : (size_t)1 << 20;
    while (nc < need_fix) nc *= 2;
    int r = grow_arrays(s.fix_mem, fix_arrays(s.v), (size_t)s.v.cap_fix, nc, (size_t)s.v.cap_fix, st, err);
    if (r) return r;
    s.v.cap_fix = (int)nc;
  }
  // keep the hash table under ~50 % load, counting the tombstones of pruned roots (insertion reuses them, lookups walk past
  // them): when the live roots alone would fit, the table is re-hashed at its current size, which drops the tombstones
  if (2 * ((size_t)s.ub_used + need_pts) > (size_t)s.hcap) {
    if (s.cnt_stale) { int r = map_read_counters(s, st, err); if (r) return r; }
    if (2 * ((size_t)s.ub_used + need_pts) > (size_t)s.hcap) {
      unsigned int nc = s.hcap;
      while ((size_t)nc < 2 * ((size_t)s.ub_roots + need_pts) && nc < (1u << 30)) nc *= 2;
      int r = map_hash_alloc(s, nc, st, err);
      if (r) return r;
    }
  }
  return VBA_OK;
}

// what is not memory (the pose ring's events), then the memory as a whole: the owners of MapMem free themselves
void map_free(MapStore &s) {
  for (hipEvent_t &e : s.pose_ev) { if (e) hipEventDestroy(e); e = nullptr; }
  static_cast<MapMem &>(s) = MapMem();
  s.v = MapView{};
  s.sort_tmp_for = 0;
  s.allocated = false;
}

bool is_device_ptr(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice;
}
inline int map_stage(MapStore &s, size_t bytes, std::string &err) {
  VBA_HIPCHK(err, s.d_stage.ensure(bytes));
  return VBA_OK;
}
inline int map_set_counter(MapStore &s, hipStream_t st, int which, int val, std::string &err) {   // stream-ordered, no host sync
  hipLaunchKernelGGL(k_set_counter, dim3(1), dim3(1), 0, st, s.v.cnt, which, val);
  VBA_HIPCHK(err, hipGetLastError());
  return VBA_OK;
}

// cnt[to] = sum over the ranks of cnt[from]  (no-op for an unsharded map)
inline int map_global_count(MapStore &s, hipStream_t st, int from, int to, std::string &err) {
  if (s.n_ranks <= 1 || !s.allreduce) return VBA_OK;
  VBA_HIPCHK(err, s.d_gc.ensure(2));
  hipLaunchKernelGGL(k_cnt_to_f64, dim3(1), dim3(1), 0, st, s.v.cnt, from, s.d_gc.p);
  if (s.allreduce(s.d_gc, 1)) { err = "collective failed while summing a map counter over the ranks"; return VBA_ERR_HIP; }
  hipLaunchKernelGGL(k_f64_to_cnt, dim3(1), dim3(1), 0, st, s.d_gc.p, s.v.cnt, to);
  VBA_HIPCHK(err, hipGetLastError());
  return VBA_OK;
}

// rocPRIM scratch for sorting up to max_pts (leaf, point) pairs
inline int map_sort_reserve(MapStore &s, hipStream_t st, std::string &err) {
  if (s.sort_tmp_for >= s.v.max_pts) return VBA_OK;
  size_t need = 0;
  VBA_HIPCHK(err, sort_pairs_u32(nullptr, need, s.v.skey_a, s.v.skey_b, s.v.sval_a, s.v.sval_b, (size_t)s.v.max_pts, 32u, st));
  if (need > s.d_sort_tmp.n) {
    VBA_HIPCHK(err, hipStreamSynchronize(st));
    VBA_HIPCHK(err, s.d_sort_tmp.ensure(need + 256));
  }
  s.sort_tmp_for = s.v.max_pts;
  return VBA_OK;
}
// sort key = node id < cap; "no leaf" = all ones, which must sort behind every id
inline unsigned int map_key_bits(const MapStore &s) {
  unsigned int bits = 1;
  while (bits < 32 && (1ull << bits) <= (unsigned long long)s.v.cap) bits++;
  return bits;
}

// phases 1-2 of an insertion of n points (root keys, new roots); deterministic mode ranks the new roots by their first point
inline void map_ins_roots(MapStore &s, hipStream_t st, const MapParams &P, int slot, int n, int is_fix, double jour, int stamp) {
  const int nb = (n + 255) / 256;
  if (!s.det) {
    hipLaunchKernelGGL(k_ins_keys<false>, dim3(nb), dim3(256), 0, st, s.v, P, slot, n, is_fix, stamp);
    hipLaunchKernelGGL(k_ins_newroots, dim3(nb), dim3(256), 0, st, s.v, P, is_fix, jour, stamp);
    return;
  }
  hipLaunchKernelGGL(k_ins_keys<true>, dim3(nb), dim3(256), 0, st, s.v, P, slot, n, is_fix, stamp);
  hipLaunchKernelGGL(k_ins_newroots_det<0>, dim3(nb), dim3(256), 0, st, s.v, P, n, is_fix, jour, stamp);
  hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.v.dblk, nb, s.v.cnt, -1, 0, (int)CNT_NEWSLOTS);
  hipLaunchKernelGGL(k_ins_newroots_det<1>, dim3(nb), dim3(256), 0, st, s.v, P, n, is_fix, jour, stamp);
  hipLaunchKernelGGL(k_det_commit, dim3(1), dim3(1), 0, st, s.v, (int)CNT_NEWSLOTS, (int)CNT_FREE_ROOTS, 1, is_fix);
}

// cut_voxel / cut_voxel_multi for one scan
int map_cut_voxel(MapStore &s, hipStream_t st, int win_count, int n, const double *pnt_body, const double *var, const double *pose,
                  bool multi, std::string &err, const double *cov6, const double *d_state_blk) {
  const int W = s.opt.win_size;
  if (win_count < 0 || win_count >= W || n < 0 || (!pose && !d_state_blk) || (n > 0 && !pnt_body)) return VBA_ERR_BAD_ARG;
  int r = map_base(s, st, err);
  if (r) return r;
  if (s.cnt_stale && (s.ub_nodes + n + 64 > (long long)s.v.cap || 2 * (s.ub_used + n) > (long long)s.hcap)) {
    r = map_read_counters(s, st, err);      // bounds too pessimistic for the current capacity: fetch the true counts
    if (r) return r;
  }
  r = map_ensure(s, st, (size_t)s.ub_nodes + (size_t)n + 64, (size_t)n, (size_t)1, err);
  if (r) return r;
  const int slot = s.mp[win_count];
  s.npts[slot] = n;
  if (n == 0) return VBA_OK;
  // stage the points into the slot's SoA arrays
  const double *d_pts = pnt_body, *d_var = var;
  if (!is_device_ptr(pnt_body)) {
    const size_t bytes = (size_t)n * 3 * 8 + (var ? (size_t)n * 9 * 8 : 0);
    r = map_stage(s, bytes, err);
    if (r) return r;
    VBA_HIPCHK(err, hipMemcpyAsync(s.d_stage, pnt_body, (size_t)n * 3 * 8, hipMemcpyHostToDevice, st));
    d_pts = (const double *)s.d_stage.p;
    if (var) {
      VBA_HIPCHK(err, hipMemcpyAsync(s.d_stage + (size_t)n * 3 * 8, var, (size_t)n * 9 * 8, hipMemcpyHostToDevice, st));
      d_var = (const double *)(s.d_stage + (size_t)n * 3 * 8);
    }
  }
  if (var) s.have_var = true;
  // pose and covariance blocks of a resident odometry state: written where they lie, nothing comes from the host
  if (d_state_blk) hipLaunchKernelGGL(k_odom_state_pose, dim3(1), dim3(64), 0, st, d_state_blk, s.v.poses);
  else {  // pose upload through a pinned ring: no implicit synchronisation of a pageable copy
    VBA_HIPCHK(err, s.h_pose_ring.ensure(8 * 40));
    const int k = s.pose_next; s.pose_next = (k + 1) & 7;
    if (!s.pose_ev[k]) VBA_HIPCHK(err, hipEventCreateWithFlags(&s.pose_ev[k], hipEventDisableTiming));
    else VBA_HIPCHK(err, hipEventSynchronize(s.pose_ev[k]));
    // entry = the device image poses[0 .. 34): pose (12) | 4 unused | rot_var, tsl_var (18) — one copy command
    std::memcpy(s.h_pose_ring + 40 * k, pose, 12 * sizeof(double));
    if (cov6) std::memcpy(s.h_pose_ring + 40 * k + 16, cov6, 18 * sizeof(double));
    VBA_HIPCHK(err, hipMemcpyAsync(s.v.poses, s.h_pose_ring + 40 * k, (cov6 ? 34 : 12) * sizeof(double), hipMemcpyHostToDevice, st));
    VBA_HIPCHK(err, hipEventRecord(s.pose_ev[k], st));
  }
  const MapParams P = map_params(s);
  const int nb = (n + 255) / 256;
  if ((cov6 || d_state_blk) && var) hipLaunchKernelGGL(k_scan_to_soa_pvec_update, dim3(nb), dim3(256), 0, st, s.v, W, slot, n, d_pts, d_var, s.v.poses, s.v.poses + 16);
  else hipLaunchKernelGGL(k_scan_to_soa, dim3(nb), dim3(256), 0, st, s.v, W, slot, n, d_pts, d_var);
  s.stamp++;
  map_ins_roots(s, st, P, slot, n, 0, 0.0, s.stamp);
  if (multi) { r = map_global_count(s, st, CNT_TOUCH, CNT_TOUCH_G, err); if (r) return r; }   // VM:2044 tests the whole scan's voxel count
  // order-preserving accumulation: leaf of every point + per-leaf counts -> segments (scan over the touched leaves) -> scatter ->
  // one wave (workgroup for big leaves) per leaf puts its segment into scan order and adds in that order
  hipLaunchKernelGGL(k_ins_leaf, dim3(nb), dim3(256), 0, st, s.v, P, slot, n, multi ? 1 : 0);
  {
    long long ubn = (long long)s.ub_nodes + n;               // the insert creates at most one node (a root) per point
    if (ubn > s.v.cap) ubn = s.v.cap;
    hipLaunchKernelGGL(k_ins_scan, dim3((unsigned)((ubn + 255) / 256)), dim3(256), 0, st, s.v, slot);
  }
  hipLaunchKernelGGL(k_ins_scatter, dim3(nb), dim3(256), 0, st, s.v, slot, n);
  {
    const int nwg = n < 8192 ? ((n + 7) & ~7) : 8192;   // grid-stride over the work list (its length stays on the device); a multiple of 8
    int win = 128; while (win < n && win < (1 << 19)) win *= 2;         // bitmap window of the big-leaf kernel (<= 96 KB of LDS)
    size_t lds_big = (size_t)(win / 64) * 12 + 16;
    if (lds_big < (size_t)4 * 64 * 33 * 8) lds_big = (size_t)4 * 64 * 33 * 8;             // bitmap + prefix, then the four term images in the same space
    static LdsOptIn opt_in_var, opt_in_novar;
    int dev = 0; hipGetDevice(&dev);
    VBA_HIPCHK(err, opt_in_var(dev, (const void *)k_ins_accum_big<true>, 160 * 1024 - 64));
    VBA_HIPCHK(err, opt_in_novar(dev, (const void *)k_ins_accum_big<false>, 160 * 1024 - 64));
    if (var) {
      hipLaunchKernelGGL((k_ins_accum_ord<true>), dim3(nwg), dim3(64), 0, st, s.v, P, slot);
      hipLaunchKernelGGL((k_ins_accum_big<true>), dim3(256), dim3(256), lds_big, st, s.v, P, slot, n, win);
    } else {
      hipLaunchKernelGGL((k_ins_accum_ord<false>), dim3(nwg), dim3(64), 0, st, s.v, P, slot);
      hipLaunchKernelGGL((k_ins_accum_big<false>), dim3(256), dim3(256), lds_big, st, s.v, P, slot, n, win);
    }
  }
  VBA_HIPCHK(err, hipGetLastError());
  // no read-back: capacity was reserved for the worst case (n new roots), so this call cannot overflow
  s.ub_nodes += n; s.ub_roots += n; s.ub_used += n; s.cnt_stale = true;
  if (!is_device_ptr(pnt_body)) VBA_HIPCHK(err, hipStreamSynchronize(st));   // the caller's host point buffers may go away (pose and covariance went through the pinned ring)
  return VBA_OK;
}

int map_cut_voxel_fix(MapStore &s, hipStream_t st, int n, const double *pnt_world, double jour, std::string &err) {
  if (n < 0 || (n > 0 && !pnt_world)) return VBA_ERR_BAD_ARG;
  if (n == 0) return VBA_OK;
  int r = map_base(s, st, err);
  if (r) return r;
  if (s.cnt_stale) { r = map_read_counters(s, st, err); if (r) return r; }
  r = map_ensure(s, st, (size_t)s.h_cnt[CNT_NODES] + (size_t)n + 64, (size_t)n, (size_t)s.h_cnt[CNT_FIX] + (size_t)n, err);
  if (r) return r;
  const double *d_pts = pnt_world;
  if (!is_device_ptr(pnt_world)) {
    r = map_stage(s, (size_t)n * 3 * 8, err);
    if (r) return r;
    VBA_HIPCHK(err, hipMemcpyAsync(s.d_stage, pnt_world, (size_t)n * 3 * 8, hipMemcpyHostToDevice, st));
    d_pts = (const double *)s.d_stage.p;
  }
  const MapParams P = map_params(s);
  const int base = s.h_cnt[CNT_FIX];
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_fix_to_soa, dim3(nb), dim3(256), 0, st, s.v, base, n, d_pts);
  r = map_set_counter(s, st, CNT_NEWSLOTS, 0, err); if (r) return r;
  r = map_set_counter(s, st, CNT_FIX, base + n, err); if (r) return r;
  map_ins_roots(s, st, P, base, n, 1, jour, 0);
  r = map_sort_reserve(s, st, err); if (r) return r;
  r = map_set_counter(s, st, CNT_WL, 0, err); if (r) return r;
  hipLaunchKernelGGL(k_fix_leaf, dim3(nb), dim3(256), 0, st, s.v, P, base, n);
  {
    size_t tb = s.d_sort_tmp.n;
    VBA_HIPCHK(err, sort_pairs_u32(s.d_sort_tmp.p, tb, s.v.skey_a, s.v.skey_b, s.v.sval_a, s.v.sval_b, (size_t)n, map_key_bits(s), st));
  }
  hipLaunchKernelGGL(k_fix_heads, dim3(nb), dim3(256), 0, st, s.v, n);
  hipLaunchKernelGGL((k_fix_accum_ord<FIXCOV_KEEP>), dim3(n < 4096 ? n : 4096), dim3(64), 0, st, s.v, P, base, n, d_pts, (const int *)nullptr, (const void *)nullptr);
  VBA_HIPCHK(err, hipGetLastError());
  r = map_read_counters(s, st, err);
  if (r) return r;
  if (s.h_cnt[CNT_OVERFLOW]) { err = "voxel map capacity exceeded during fixed-point insert"; return VBA_ERR_CAPACITY; }
  return VBA_OK;
}

// recut over the scope + factor index assignment; *n_factors = number of planar leaves selected by tras_opt
int map_recut(MapStore &s, hipStream_t st, int win_count, const double *poses, bool multi, std::string &err, int *n_factors) {
  const int W = s.opt.win_size;
  *n_factors = 0;
  if (win_count < 0 || win_count > W || !poses) return VBA_ERR_BAD_ARG;
  if (!s.allocated) return VBA_OK;
  if (multi) { int r0 = map_global_count(s, st, CNT_SLIDE, CNT_SLIDE_G, err); if (r0) return r0; }   // VS:1693 tests surf_map_slide.size() of the whole map
  for (int attempt = 0; attempt < 8; attempt++) {
    // The first attempt works from the host's upper bound of the node count (exact at the last read-back + the points inserted
    // since): no read-back, hence no drain of the stream, before the pass.  The pass ends with the one read-back that serves the
    // overflow check, the factor count and the next call's bounds.
    int r = VBA_OK;
    if (attempt > 0) { r = map_read_counters(s, st, err); if (r) return r; }
    const size_t nodes_ub = attempt ? (size_t)s.h_cnt[CNT_NODES] : (size_t)s.ub_nodes;
    // room for every current leaf to split once per level (checked again through the overflow flag)
    r = map_ensure(s, st, nodes_ub + 8 * (size_t)(attempt ? s.h_cnt[CNT_NODES] : 65536), 0, 0, err);
    if (r) return r;
    VBA_HIPCHK(err, hipMemcpyAsync(s.v.poses, poses, (size_t)(win_count > 0 ? win_count : 1) * 12 * sizeof(double), hipMemcpyHostToDevice, st));
    const MapParams P = map_params(s);
    int max_n = 0;
    for (int i = 0; i < win_count; i++) if (s.npts[s.mp[i]] > max_n) max_n = s.npts[s.mp[i]];
    const int grid_nodes = (s.v.cap + 255) / 256;
    if (nodes_ub > 0) {
      for (int L = 0; L <= s.opt.max_layer; L++) {
        s.epoch++;
        hipLaunchKernelGGL(k_recut_prep, dim3(1), dim3(1), 0, st, s.v.cnt, L == 0 ? 1 : 0, L == s.opt.max_layer ? 1 : 0);
        if (s.det) {
          hipLaunchKernelGGL(k_recut_leaf<true>, dim3(grid_nodes), dim3(256), 0, st, s.v, P, L, multi ? 1 : 0, s.epoch);
          hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.v.dblk, grid_nodes, s.v.cnt, (int)CNT_SNAP, s.v.cap, (int)CNT_SPLIT);
          hipLaunchKernelGGL(k_recut_split_det, dim3(grid_nodes), dim3(256), 0, st, s.v, P, L, s.epoch);
          hipLaunchKernelGGL(k_det_commit, dim3(1), dim3(1), 0, st, s.v, (int)CNT_SPLIT, (int)CNT_FREE_BLOCKS, 8, 0);
        } else {
          hipLaunchKernelGGL(k_recut_leaf<false>, dim3(grid_nodes), dim3(256), 0, st, s.v, P, L, multi ? 1 : 0, s.epoch);
        }
        if (L < s.opt.max_layer) {
          if (s.have_var) hipLaunchKernelGGL((k_recut_push<true>), dim3(4096), dim3(256), 0, st, s.v, P, win_count, L + 1);
          else hipLaunchKernelGGL((k_recut_push<false>), dim3(4096), dim3(256), 0, st, s.v, P, win_count, L + 1);
        }
#ifdef VBA_DIAG
        if (getenv("VBA_RECUT_STATS")) {
          int h[CNT_N];
          hipStreamSynchronize(st);
          hipMemcpy(h, s.v.cnt, sizeof(h), hipMemcpyDeviceToHost);
          fprintf(stderr, "[recut] level %d: nodes %d, split leaves %d, candidates scanned %d, matched %d, fix blocks walked %d (%d entries)\n", L, h[CNT_NODES], h[CNT_SPLIT], h[CNT_DBG0], h[CNT_DBG1], h[CNT_DBG2], h[CNT_DBG3]);
          const int z[4] = {0, 0, 0, 0};
          hipMemcpy(s.v.cnt + CNT_DBG0, z, sizeof(z), hipMemcpyHostToDevice);
        }
#endif
      }
      // tras_opt pass 1 rides in the same submission: one counter read-back serves the overflow check and the factor count
      if (s.det) {
        hipLaunchKernelGGL(k_extract_count<1>, dim3(grid_nodes), dim3(256), 0, st, s.v, P, multi ? 1 : 0);
        hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.v.dblk, grid_nodes, s.v.cnt, (int)CNT_NODES, s.v.cap, (int)CNT_FACTORS);
        hipLaunchKernelGGL(k_extract_count<2>, dim3(grid_nodes), dim3(256), 0, st, s.v, P, multi ? 1 : 0);
      } else {
        hipLaunchKernelGGL(k_extract_count<0>, dim3(grid_nodes), dim3(256), 0, st, s.v, P, multi ? 1 : 0);
      }
    }
    VBA_HIPCHK(err, hipGetLastError());
    r = map_read_counters(s, st, err);
    if (r) return r;
    if (s.h_cnt[CNT_OVERFLOW] == 4) { err = "root hash table full during scan insertion"; return VBA_ERR_CAPACITY; }
    if (!s.h_cnt[CNT_OVERFLOW]) break;
    // a leaf could not be split for lack of node space: clamp the counter, grow and run the pass again (idempotent)
    if (s.h_cnt[CNT_NODES] > s.v.cap) { r = map_set_counter(s, st, CNT_NODES, s.v.cap, err); if (r) return r; }
    if (attempt == 7) { err = "voxel map node capacity exceeded during recut"; return VBA_ERR_CAPACITY; }
  }
  if (s.h_cnt[CNT_NODES] == 0) s.h_cnt[CNT_FACTORS] = 0;
  *n_factors = s.h_cnt[CNT_FACTORS];
  s.h_cnt[CNT_N] = multi ? 1 : 0;   // remembered for map_extract_factors
  return VBA_OK;
}

int map_extract_factors(MapStore &s, hipStream_t st, FactorView f, std::string &err, int *n_factors) {
  *n_factors = 0;
  if (!s.allocated) return VBA_OK;
  const MapParams P = map_params(s);
  const int nfac = s.h_cnt[CNT_NODES] > 0 ? s.h_cnt[CNT_FACTORS] : 0;
  if (nfac > 1) {
    const int nbuckets = 1 << (s.opt.win_size < 10 ? s.opt.win_size : 10);
    const int nwg = (nfac + 255) / 256;
    if (s.det) {   // stable: (bucket, node id)
      const size_t need = (size_t)nbuckets * nwg;
      if (need > s.d_whist.n) {
        VBA_HIPCHK(err, hipStreamSynchronize(st));
        VBA_HIPCHK(err, s.d_whist.ensure(need));
      }
      hipLaunchKernelGGL(k_extract_key<true>, dim3(nwg), dim3(256), 0, st, s.v, P, nfac, nbuckets, s.d_whist.p);
      hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.d_whist.p, (int)need, s.v.cnt, -1, 0, -1);
      hipLaunchKernelGGL(k_extract_scatter_det, dim3(nwg), dim3(256), 0, st, s.v, (const int *)s.d_whist.p, nfac, nbuckets);
    } else {
      VBA_HIPCHK(err, hipMemsetAsync(s.v.fhist, 0, (size_t)nbuckets * sizeof(int), st));
      hipLaunchKernelGGL(k_extract_key<false>, dim3(nwg), dim3(256), 0, st, s.v, P, nfac, nbuckets, (int *)nullptr);
      hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(1024), 0, st, s.v, nbuckets);
      hipLaunchKernelGGL(k_extract_scatter, dim3(nwg), dim3(256), 0, st, s.v, nfac, nbuckets);
    }
  }
  if (nfac > 0) hipLaunchKernelGGL(k_extract_write, dim3((nfac + XW_F - 1) / XW_F), dim3(256), (size_t)(10 * s.opt.win_size + 33) * (XW_F + 1) * 8, st, s.v, P, f, nfac);
  VBA_HIPCHK(err, hipGetLastError());
  *n_factors = s.h_cnt[CNT_FACTORS];
  return VBA_OK;
}

int map_margi(MapStore &s, hipStream_t st, int win_count, const double *poses, double jour, FactorView f, int nfac, std::string &err) {
  const int W = s.opt.win_size;
  if (win_count < 1 || win_count > W || !poses) return VBA_ERR_BAD_ARG;
  if (!s.allocated) return VBA_OK;
  int r = VBA_OK;
  r = map_global_count(s, st, CNT_SLIDE, CNT_SLIDE_G, err); if (r) return r;   // VS:1616 tests the whole sliding map (every rank enters this collective)
  if (s.cnt_stale || s.n_ranks > 1) { r = map_read_counters(s, st, err); if (r) return r; }    // (the recut before the optimisation left them current)
  const int slot0 = s.mp[0];
  r = map_ensure(s, st, 0, 0, (size_t)s.h_cnt[CNT_FIX] + (size_t)s.npts[slot0] + 1, err);
  if (r) return r;
  hipLaunchKernelGGL(k_set_counter2, dim3(1), dim3(1), 0, st, s.v.cnt, (int)CNT_OVERFLOW, 0, (int)CNT_TAKE, 0);
  VBA_HIPCHK(err, hipMemcpyAsync(s.v.poses, poses, (size_t)win_count * 12 * sizeof(double), hipMemcpyHostToDevice, st));
  const MapParams P = map_params(s);
  const int nn = s.h_cnt[CNT_NODES] < s.v.cap ? s.h_cnt[CNT_NODES] : s.v.cap;
  const int n_slide_before = s.n_ranks > 1 ? s.h_cnt[CNT_SLIDE_G] : s.h_cnt[CNT_SLIDE];
  if (nn == 0) return VBA_OK;
  s.epoch++;
  const dim3 gn((nn + 255) / 256), b(256);
  hipLaunchKernelGGL(k_margi_leaf, gn, b, 0, st, s.v, P, f, nfac, win_count, s.epoch);
  if (n_slide_before >= s.opt.thread_num) {
    if (s.npts[slot0] > 0) {
      hipLaunchKernelGGL(k_margi_take, dim3(4096), dim3(64), 0, st, s.v, P, s.have_var ? 1 : 0);
      hipLaunchKernelGGL(k_margi_points, dim3((s.v.max_pts + 1023) / 1024), dim3(1024), 0, st, s.v, P);
    }
    if (s.h_cnt[CNT_FIX] > 0) hipLaunchKernelGGL(k_margi_fixclear, dim3((s.h_cnt[CNT_FIX] + 255) / 256), b, 0, st, s.v, s.epoch);
    for (int L = s.opt.max_layer - 1; L >= 0; L--) hipLaunchKernelGGL(k_margi_up, gn, b, 0, st, s.v, P, L);
    hipLaunchKernelGGL(k_margi_roots, gn, b, 0, st, s.v, P, jour, s.epoch, n_slide_before);
    hipLaunchKernelGGL(k_margi_clear_nodes, gn, b, 0, st, s.v, P, s.epoch);
    hipLaunchKernelGGL(k_margi_clear_points, dim3((s.v.max_pts + 255) / 256, W), b, 0, st, s.v, P, s.epoch);
    s.npts[slot0] = 0;
  }
  VBA_HIPCHK(err, hipGetLastError());
  r = map_read_counters(s, st, err);
  if (r) return r;
  if (s.h_cnt[CNT_OVERFLOW] == 2) { err = "Error: opt_state out of range"; return VBA_ERR_OPT_STATE; }
  if (s.h_cnt[CNT_OVERFLOW]) { err = "fixed-point pool capacity exceeded"; return VBA_ERR_CAPACITY; }
  return VBA_OK;
}

int map_slide(MapStore &s, int mgsize) {   // VS:2014-2019
  const int W = s.opt.win_size;
  if (mgsize < 0 || mgsize > W) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < W; i++) { s.mp[i] += mgsize; if (s.mp[i] >= W) s.mp[i] -= W; }
  return VBA_OK;
}

int map_reset(MapStore &s, hipStream_t st, std::string &err) {
  if (!s.allocated) return VBA_OK;
  const int W = s.opt.win_size;
  hipStreamSynchronize(st);
  for (auto &a : node_arrays(s.v, W)) VBA_HIPCHK(err, hipMemsetAsync(*a.slot, 0, a.elem * a.rows * (size_t)s.v.cap, st));
  if (s.v.pnode) VBA_HIPCHK(err, hipMemsetAsync(s.v.pnode, 0xFF, (size_t)W * s.v.max_pts * 4, st));
  if (s.v.pleaf) VBA_HIPCHK(err, hipMemsetAsync(s.v.pleaf, 0xFF, (size_t)W * s.v.max_pts * 4, st));
  if (s.v.fnode) VBA_HIPCHK(err, hipMemsetAsync(s.v.fnode, 0xFF, (size_t)s.v.cap_fix * 4, st));
  hipLaunchKernelGGL(k_fill_u64, dim3(1024), dim3(256), 0, st, s.v.hkeys, KEY_EMPTY, (size_t)s.hcap);
  VBA_HIPCHK(err, hipMemsetAsync(s.v.hvals, 0xFF, (size_t)s.hcap * 4, st));
  if (s.v.hfirst) VBA_HIPCHK(err, hipMemsetAsync(s.v.hfirst, 0x7F, (size_t)s.hcap * 4, st));
  VBA_HIPCHK(err, hipMemsetAsync(s.v.cnt, 0, CNT_N * sizeof(int), st));
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  std::memset(s.h_cnt, 0, CNT_N * sizeof(int));
  for (int i = 0; i < VBA_MAX_WIN; i++) { s.mp[i] = i; s.npts[i] = 0; }
  s.have_var = false; s.ub_nodes = 0; s.ub_roots = 0; s.ub_used = 0; s.cnt_stale = false;
  return VBA_OK;
}

int map_num_roots(MapStore &s, hipStream_t st, bool slide) {
  if (!s.allocated) return 0;
  std::string err;
  if (map_read_counters(s, st, err)) return -1;
  return slide ? s.h_cnt[CNT_SLIDE] : s.h_cnt[CNT_ROOTS];
}

// storage statistics: [node high-water mark, free root nodes, free child blocks, hash capacity, hash slots in use (roots +
// tombstones), roots, sliding-map roots, fixed points]
int map_stats(MapStore &s, hipStream_t st, long long *out8, std::string &err) {
  for (int k = 0; k < 8; k++) out8[k] = 0;
  if (!s.allocated) return VBA_OK;
  int r = map_read_counters(s, st, err);
  if (r) return r;
  out8[0] = s.h_cnt[CNT_NODES]; out8[1] = s.h_cnt[CNT_FREE_ROOTS]; out8[2] = s.h_cnt[CNT_FREE_BLOCKS]; out8[3] = s.hcap;
  out8[4] = s.h_cnt[CNT_USED]; out8[5] = s.h_cnt[CNT_ROOTS]; out8[6] = s.h_cnt[CNT_SLIDE]; out8[7] = s.h_cnt[CNT_FIX];
  return VBA_OK;
}

int map_dump_leaves(MapStore &s, hipStream_t st, double *out, int max_leaves, std::string &err) {
  if (!s.allocated) return 0;
  if (map_read_counters(s, st, err)) return -1;
  const int nn = s.h_cnt[CNT_NODES] < s.v.cap ? s.h_cnt[CNT_NODES] : s.v.cap;
  if (nn == 0) return 0;
  const int cap_out = out ? max_leaves : 0;
  DevMem<double> d_out;                         // a temporary of this call
  if (cap_out > 0 && d_out.ensure((size_t)cap_out * 39) != hipSuccess) return -1;
  if (map_set_counter(s, st, CNT_LEAVES, 0, err)) return -1;
  if (s.det) {   // rows in ascending node id
    hipLaunchKernelGGL(k_dump_leaves<1>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, d_out, cap_out);
    hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.v.dblk, (nn + 255) / 256, s.v.cnt, -1, 0, (int)CNT_LEAVES);
    hipLaunchKernelGGL(k_dump_leaves<2>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, d_out, cap_out);
  } else {
    hipLaunchKernelGGL(k_dump_leaves<0>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, d_out, cap_out);
  }
  if (map_read_counters(s, st, err)) return -1;
  const int n = s.h_cnt[CNT_LEAVES];
  if (cap_out > 0) hipMemcpy(out, d_out, (size_t)(n < cap_out ? n : cap_out) * 39 * 8, hipMemcpyDeviceToHost);
  return n;
}

int map_dump_plane_var(MapStore &s, hipStream_t st, double *out, int max_leaves, std::string &err) {
  if (!s.allocated) return 0;
  if (map_read_counters(s, st, err)) return -1;
  const int nn = s.h_cnt[CNT_NODES] < s.v.cap ? s.h_cnt[CNT_NODES] : s.v.cap;
  if (nn == 0) return 0;
  const int cap_out = out ? max_leaves : 0;
  DevMem<double> d_out;                         // a temporary of this call
  if (cap_out > 0 && d_out.ensure((size_t)cap_out * 86) != hipSuccess) return -1;
  if (map_set_counter(s, st, CNT_LEAVES, 0, err)) return -1;
  if (s.det) {   // rows in ascending node id
    hipLaunchKernelGGL(k_dump_plane_var<1>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, d_out, cap_out);
    hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.v.dblk, (nn + 255) / 256, s.v.cnt, -1, 0, (int)CNT_LEAVES);
    hipLaunchKernelGGL(k_dump_plane_var<2>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, d_out, cap_out);
  } else {
    hipLaunchKernelGGL(k_dump_plane_var<0>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, d_out, cap_out);
  }
  if (map_read_counters(s, st, err)) return -1;
  const int n = s.h_cnt[CNT_LEAVES];
  if (cap_out > 0) hipMemcpy(out, d_out, (size_t)(n < cap_out ? n : cap_out) * 86 * 8, hipMemcpyDeviceToHost);
  return n;
}

int map_prune(MapStore &s, hipStream_t st, double jour, int dist, std::string &err) {
  if (!s.allocated) return VBA_OK;
  int r = map_read_counters(s, st, err);
  if (r) return r;
  const int nn = s.h_cnt[CNT_NODES] < s.v.cap ? s.h_cnt[CNT_NODES] : s.v.cap;
  if (nn == 0) return VBA_OK;
  s.epoch++;
  hipLaunchKernelGGL(k_prune_roots, dim3((s.hcap + 255) / 256), dim3(256), 0, st, s.v, jour, dist, s.epoch);
  if (s.det) hipLaunchKernelGGL(k_prune_nodes<true>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, s.epoch);
  else hipLaunchKernelGGL(k_prune_nodes<false>, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, s.epoch);
  hipLaunchKernelGGL(k_prune_finish, dim3((nn + 255) / 256), dim3(256), 0, st, s.v, s.epoch);
  if (s.det) {   // both free stacks rebuilt in id order (descending, so that the pops come out ascending)
    const int nb = (nn + 255) / 256;
    hipLaunchKernelGGL((k_prune_free_det<0, 0>), dim3(nb), dim3(256), 0, st, s.v);
    hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.v.dblk, nb, s.v.cnt, -1, 0, (int)CNT_FREE_ROOTS);
    hipLaunchKernelGGL((k_prune_free_det<0, 1>), dim3(nb), dim3(256), 0, st, s.v);
    hipLaunchKernelGGL((k_prune_free_det<1, 0>), dim3(nb), dim3(256), 0, st, s.v);
    hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(1024), 0, st, s.v.dblk, nb, s.v.cnt, -1, 0, (int)CNT_FREE_BLOCKS);
    hipLaunchKernelGGL((k_prune_free_det<1, 1>), dim3(nb), dim3(256), 0, st, s.v);
  }
  hipLaunchKernelGGL(k_prune_zero, dim3((nn + 255) / 256, 130 + 10 * s.opt.win_size), dim3(256), 0, st, s.v, s.opt.win_size, s.epoch);
  if (s.h_cnt[CNT_FIX] > 0) hipLaunchKernelGGL(k_prune_fix, dim3((s.h_cnt[CNT_FIX] + 255) / 256), dim3(256), 0, st, s.v);
  VBA_HIPCHK(err, hipGetLastError());
  return map_read_counters(s, st, err);
}


// ================================================================================================ loop-closure map rebuild (vba_kernels_loop.hpp)
// bytes of the map's staging buffer one insertion of n points needs: world points, source rows and the seven per-point temporaries
// of the insert kernels.  The temporaries live here, not in the map's [max_pts] arrays: those are sized for ONE scan and come in
// [W] rows, and an expanded keyframe sequence is 10-40 scans long.
inline size_t fix_source_stage_bytes(size_t n) { return ((n * 24 + 255) & ~(size_t)255) + 8 * ((n * 4 + 255) & ~(size_t)255); }

inline int map_sort_reserve_n(MapStore &s, hipStream_t st, size_t n, std::string &err) {
  size_t need = 0;
  VBA_HIPCHK(err, sort_pairs_u32(nullptr, need, nullptr, nullptr, nullptr, nullptr, n, 32u, st));
  if (need + 256 > s.d_sort_tmp.n) {
    VBA_HIPCHK(err, hipStreamSynchronize(st));
    VBA_HIPCHK(err, s.d_sort_tmp.ensure(need + 256));
  }
  return VBA_OK;
}

// room for an insertion of n fixed points on top of what the map holds (counters current): nodes, pool, root table, staging, sort
int map_fix_source_ensure(MapStore &s, hipStream_t st, size_t nodes, size_t fix, size_t n, std::string &err) {
  int r = map_ensure(s, st, nodes, 0, fix, err);
  if (r) return r;
  if (2 * ((size_t)s.ub_used + n) > (size_t)s.hcap) {       // as map_ensure keeps the table under ~50 % load, for n possible new roots
    unsigned int nc = s.hcap;
    while ((size_t)nc < 2 * ((size_t)s.ub_roots + n) && nc < (1u << 30)) nc *= 2;
    r = map_hash_alloc(s, nc, st, err);
    if (r) return r;
  }
  if (fix_source_stage_bytes(n) > s.d_stage.n) VBA_HIPCHK(err, hipStreamSynchronize(st));
  r = map_stage(s, fix_source_stage_bytes(n), err);
  if (r) return r;
  return map_sort_reserve_n(s, st, n, err);
}

// map_cut_voxel_fix for a FixSource: n = points of the expanded sequence.  Same kernels after the staging, same single counter
// read-back at the end; k_fix_to_soa does not run (k_loop_gather writes the pool tail itself).
int map_cut_voxel_fix_source(MapStore &s, hipStream_t st, int n, const FixSource &src, double jour, std::string &err) {
  if (n < 0 || (n > 0 && (!src.d_pnt || !src.d_seg || !src.d_poses || src.nseg < 1)) || src.cov_kind == FIXCOV_KEEP || (src.cov_kind != FIXCOV_ZERO && !src.d_cov)) return VBA_ERR_BAD_ARG;
  if (n == 0) return VBA_OK;
  int r = map_base(s, st, err);
  if (r) return r;
  if (s.cnt_stale) { r = map_read_counters(s, st, err); if (r) return r; }
  if ((size_t)s.h_cnt[CNT_FIX] + (size_t)n > (size_t)INT32_MAX / 16) { err = "fixed-point pool: too many points"; return VBA_ERR_CAPACITY; }
  r = map_fix_source_ensure(s, st, (size_t)s.h_cnt[CNT_NODES] + (size_t)n + 64, (size_t)s.h_cnt[CNT_FIX] + (size_t)n, (size_t)n, err);
  if (r) return r;
  const size_t bi = ((size_t)n * 4 + 255) & ~(size_t)255;
  char *stg = s.d_stage;
  double *world = (double *)stg; stg += ((size_t)n * 24 + 255) & ~(size_t)255;
  int *srcrow = (int *)stg; stg += bi;
  // the insert kernels take their per-point temporaries from the view: for this call they point into the staging buffer
  struct Tmp {
    MapView &v; MapView keep;
    explicit Tmp(MapView &vv) : v(vv), keep(vv) {}
    ~Tmp() { v.phash = keep.phash; v.newslots = keep.newslots; v.skey_a = keep.skey_a; v.skey_b = keep.skey_b; v.sval_a = keep.sval_a; v.sval_b = keep.sval_b; v.wl = keep.wl; }
  } tmp(s.v);
  s.v.phash = (int *)stg; s.v.newslots = (int *)(stg + bi); s.v.skey_a = (unsigned int *)(stg + 2 * bi); s.v.skey_b = (unsigned int *)(stg + 3 * bi);
  s.v.sval_a = (int *)(stg + 4 * bi); s.v.sval_b = (int *)(stg + 5 * bi); s.v.wl = (int *)(stg + 6 * bi);
  const MapParams P = map_params(s);
  const int base = s.h_cnt[CNT_FIX];
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_loop_gather, dim3(nb), dim3(256), 0, st, s.v, base, n, src.nseg, src.d_seg, src.d_poses, src.d_pnt, world, srcrow);
  r = map_set_counter(s, st, CNT_NEWSLOTS, 0, err); if (r) return r;
  r = map_set_counter(s, st, CNT_FIX, base + n, err); if (r) return r;
  map_ins_roots(s, st, P, base, n, 1, jour, 0);
  r = map_set_counter(s, st, CNT_WL, 0, err); if (r) return r;
  hipLaunchKernelGGL(k_fix_leaf, dim3(nb), dim3(256), 0, st, s.v, P, base, n);
  {
    size_t tb = s.d_sort_tmp.n;
    VBA_HIPCHK(err, sort_pairs_u32(s.d_sort_tmp.p, tb, s.v.skey_a, s.v.skey_b, s.v.sval_a, s.v.sval_b, (size_t)n, map_key_bits(s), st));
  }
  hipLaunchKernelGGL(k_fix_heads, dim3(nb), dim3(256), 0, st, s.v, n);
  const dim3 ga(n < 4096 ? n : 4096), ba(64);
  if (src.cov_kind == FIXCOV_DIAG_F32) hipLaunchKernelGGL((k_fix_accum_ord<FIXCOV_DIAG_F32>), ga, ba, 0, st, s.v, P, base, n, (const double *)world, (const int *)srcrow, src.d_cov);
  else if (src.cov_kind == FIXCOV_FULL_F64) hipLaunchKernelGGL((k_fix_accum_ord<FIXCOV_FULL_F64>), ga, ba, 0, st, s.v, P, base, n, (const double *)world, (const int *)srcrow, src.d_cov);
  else hipLaunchKernelGGL((k_fix_accum_ord<FIXCOV_ZERO>), ga, ba, 0, st, s.v, P, base, n, (const double *)world, (const int *)srcrow, (const void *)nullptr);
  VBA_HIPCHK(err, hipGetLastError());
  if (src.cov_kind != FIXCOV_ZERO) s.have_var = true;       // the recut reads fvar (k_recut_push<true>)
  r = map_read_counters(s, st, err);
  if (r) return r;
  if (s.h_cnt[CNT_OVERFLOW]) { err = "voxel map capacity exceeded during fixed-point insert"; return VBA_ERR_CAPACITY; }
  return VBA_OK;
}

// ================================================================================================ resident odometry loop (vba_kernels_odom.hpp)
// ONE point loop of the resident update at the pose of the image d_S, the map's part of the frame that vba_odom.hip queues: the match
// launch over nb workgroups when there is anything to match, else nothing (every sum is zero: the reduction then runs on no
// partials).  Returns nb, the rows of d_partial the reduction is to read.
int map_odom_point_loop(MapStore &s, hipStream_t st, const vbh::OdomEkf *d_S, int n, const double *d_pts, const double *d_var,
                        double *d_partial) {
  if (!(n > 0 && s.allocated)) return 0;
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_odom_match_dev, dim3(nb), dim3(256), 0, st, s.v, map_params(s), d_S, n, d_pts, d_var, d_partial);
  return nb;
}

// vba_debug_plane_update: plane_update_dev on n caller-supplied leaves, one lane each, on a scratch view of this call (cap = n, ncov
// and nplane in a buffer the call owns): no array of the map is read or written.  in [n][67], out [n][43], host arrays.
int map_debug_plane_update(hipStream_t st, int n, const double *in, double *out, std::string &err) {
  const size_t N = (size_t)n;
  DevMem<double> buf;                           // [in 67 n | ncov 45 n | nplane 43 n | out 43 n]
  VBA_HIPCHK(err, buf.ensure(N * (67 + 45 + 43 + 43)));
  double *d_in = buf.p, *d_cov = d_in + N * 67, *d_plane = d_cov + N * 45, *d_out = d_plane + N * 43;
  VBA_HIPCHK(err, hipMemcpyAsync(d_in, in, N * 67 * sizeof(double), hipMemcpyHostToDevice, st));
  VBA_HIPCHK(err, hipMemsetAsync(d_cov, 0, N * (45 + 43 + 43) * sizeof(double), st));
  MapView v{};
  v.cap = n; v.ncov = d_cov; v.nplane = d_plane;
  hipLaunchKernelGGL(k_debug_plane_update, dim3((n + 255) / 256), dim3(256), 0, st, v, n, (const double *)d_in, d_out);
  VBA_HIPCHK(err, hipGetLastError());
  VBA_HIPCHK(err, hipMemcpyAsync(out, d_out, N * 43 * sizeof(double), hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  return VBA_OK;
}

}  // namespace vba
