// libvoxelba.so: the odometry EKF updates, both variants.  The initialisation odometry on a point-cloud map (vba_odom_kdtree_*,
// vba_odom_lio_state_estimation_kdtree*) with the kernels of vba_kernels_kd.hpp, compiled here and nowhere else, and
// the scan-to-map update on the voxel map (vba_odom_lio_state_estimation*, §17), whose kernels the map unit compiles
// (vba_kernels_odom.hpp) and whose point loop it queues (map_odom_point_loop).  And the odometry state resident in HBM (vba_odom_state_*, the
// IMU propagation vba_imu_ekf_propagate / vba_odom_state_propagate, the update and the insertion on a state object; the
// initialisation odometry and the published scan on a state object) with the kernels of vba_kernels_imu_ekf.hpp,
// compiled here and nowhere else.  And the update against a prior surfel map (vba_odom_surfel_update*), whose point
// loop the surfel-map unit compiles and queues (surfel_odom_queue).  All of them run in one frame, written once below ("the frame
// of an update"): a back-end supplies its point loop and its ok rule.
#include "vba_ctx.hpp"
#include "vba_sat.hpp"
#include "vba_odom_state.hpp"
#include "vba_kf_store_decl.hpp"
#include "vba_kernels_kd.hpp"
#include "vba_kernels_imu_ekf.hpp"
#include "vba_hostmath.hpp"
#include "vba_odom_ekf.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

extern "C" {

// ---------------------------------------------------------------- initialisation odometry on a point-cloud map (vba_kernels_kd.hpp)
static int kd_reserve(vba_ctx *c, size_t pts) {
  const size_t have = c->sat->kd.d_tree[1].n / 3;             // points; the second half grows last
  if (pts <= have) return VBA_OK;
  size_t cap = have ? have : 65536;
  while (cap < pts) cap *= 2;
  for (int i = 0; i < 2; i++) HIPCHK(c, c->sat->kd.d_tree[i].grow_keep(cap * 3, i == c->sat->kd.cur ? (size_t)c->sat->kd.n * 3 : 0, c->stream));
  c->sat->kd.allocs += 2; c->sat->kd.bytes += (int64_t)(2 * cap * 3 * sizeof(double));
  return VBA_OK;
}
// map slices of the 5-NN search for nb workgroups of scan points: enough workgroups to cover the chip
static int kd_slices_of(int nb) { return nb >= 512 ? 1 : (nb >= 128 ? 4 : 8); }
int vba_odom_kdtree_reset(vba_ctx *c) { c->sat->kd.n = 0; return VBA_OK; }
int vba_odom_kdtree_size(vba_ctx *c) { return c->sat->kd.n; }
int vba_odom_kdtree_points(vba_ctx *c, double *out) {
  if (!out && c->sat->kd.n > 0) return VBA_ERR_BAD_ARG;
  if (c->sat->kd.n == 0) return VBA_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(out, c->sat->kd.d_tree[c->sat->kd.cur], (size_t)c->sat->kd.n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

// ---------------------------------------------------------------- its EKF loop, resident on the device
// device state and pinned image of the resident EKF loops (this one and the voxel map's)
static int odom_image_ensure(vba_ctx *c) {
  if (c->sat->odom.h) return VBA_OK;                         // the pinned image is made last: complete or empty
  HIPCHK(c, c->sat->odom.d.ensure(1));
  const hipError_t e = c->sat->odom.h.ensure(1);
  if (e != hipSuccess) c->sat->odom.d.reset();
  HIPCHK(c, e);
  c->sat->kd.allocs += 2; c->sat->kd.bytes += (int64_t)(2 * sizeof(vbh::OdomEkf));
  return VBA_OK;
}
// what a resident entry point reports of the loop's result block
static void odom_report_fill(vba_odom_report *report, const vbh::OdomEkf &S, double nnt_eig_min) {
  report->iterations = S.iterations;
  for (int k = 0; k < 4; k++) { report->match_num[k] = S.match_num[k]; report->rot_add[k] = S.rot_add[k]; report->tra_add[k] = S.tra_add[k]; }
  report->nnt_eig_min = nnt_eig_min;
}
static size_t kd_up(size_t b) { return (b + 255) & ~(size_t)255; }
// scratch sized by a scan of up to p points: planes [p][4] | partials [ceil(p / 256)][34] | candidates at the slice count that
// needs the most of them among the scans of up to p points
struct KdScanLayout { size_t o_part, o_cand, bytes; };
static KdScanLayout kd_scan_layout(size_t p) {
  const size_t a = 8 * std::min<size_t>(p, 127 * 256), b = 4 * std::min<size_t>(p, 511 * 256);
  KdScanLayout L;
  L.o_part = kd_up(p * 4 * sizeof(double));
  L.o_cand = L.o_part + kd_up(((p + 255) / 256) * 34 * sizeof(double));
  L.bytes = L.o_cand + kd_up(std::max(std::max(a, b), p) * 5 * sizeof(unsigned long long));
  return L;
}
static int kd_scan_ensure(vba_ctx *c, size_t pts) {
  if (pts <= c->sat->kd.scan_pts) return VBA_OK;
  size_t cap = c->sat->kd.scan_pts ? c->sat->kd.scan_pts : 16384;
  while (cap < pts) cap *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sat->kd.d_scan.reset(); c->sat->kd.scan_pts = 0;
  const size_t b = kd_scan_layout(cap).bytes;
  HIPCHK(c, c->sat->kd.d_scan.ensure(b));
  c->sat->kd.scan_pts = cap; c->sat->kd.allocs++; c->sat->kd.bytes += (int64_t)b;
  return VBA_OK;
}
// scratch sized by map + scan of up to p points: the re-sampler's count [p] | first [p] | work area (the deterministic layout, the larger)
static int kd_ws_ensure(vba_ctx *c, size_t pts) {
  if (pts <= c->sat->kd.ws_pts) return VBA_OK;
  if (pts > ((size_t)1 << 28)) return VBA_ERR_CAPACITY;
  size_t cap = c->sat->kd.ws_pts ? c->sat->kd.ws_pts : 65536;
  while (cap < pts) cap *= 2;
  int st = VBA_OK;
  const size_t ws = kf_ws_layout(c, (int)cap, true, nullptr, nullptr, &st);
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sat->kd.d_ws.reset(); c->sat->kd.ws_pts = 0;
  const size_t b = 2 * kd_up(cap * sizeof(int)) + ws;
  HIPCHK(c, c->sat->kd.d_ws.ensure(b));
  c->sat->kd.ws_pts = cap; c->sat->kd.allocs++; c->sat->kd.bytes += (int64_t)b;
  return VBA_OK;
}

int vba_odom_kdtree_reserve(vba_ctx *c, int max_map_points, int max_scan_points) {
  if (!c || max_map_points < 0 || max_scan_points < 0 || max_map_points > (1 << 28) || max_scan_points > (1 << 28)) return VBA_ERR_BAD_ARG;
  int st = odom_image_ensure(c);
  if (st || (st = kd_reserve(c, (size_t)max_map_points + 16)) || (st = kd_scan_ensure(c, (size_t)max_scan_points)) ||
      (st = kd_ws_ensure(c, (size_t)max_map_points)))
    return st;
  return VBA_OK;
}
int vba_odom_kdtree_allocations(vba_ctx *c, int *n_allocs, int64_t *bytes) {
  if (!c || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = c->sat->kd.allocs; *bytes = c->sat->kd.bytes;
  return VBA_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the frame of an update (DESIGN.md "Source layout", §17)
// Every update, on any map and in either state form, is begin / odom_loop_queue / [what the back-end queues behind the loop] / end on
// the context's stream, image (c->sat->odom.d), pinned block (c->sat->odom.h) and partials.  A back-end supplies `loop`: queue ONE
// point loop at the pose of the image, return the rows [34] of partials it wrote.
//
// The image of a call: odom_ekf_begin on (state, cov) with cov_inv = P^-1 (VS:987), or in kd mode P^-1 / 1000 entry by entry (VS:1134,
// VS:1213) and the first iteration searching
static void odom_image_begin(vbh::OdomEkf &S, const double *state, const double *cov, bool kd) {
  double cov_inv[225];
  vbh::inverse_pplu(cov, cov_inv, VBA_DIM);
  if (kd) for (int k = 0; k < 225; k++) cov_inv[k] = cov_inv[k] / 1000;
  vbh::odom_ekf_begin(S, state, cov, cov_inv);
  if (kd) S.refind = 1;
}
static int odom_image_upload(vba_ctx *c) {
  HIPCHK(c, hipMemcpyAsync(c->sat->odom.d.p, c->sat->odom.h.p, sizeof(vbh::OdomEkf), hipMemcpyHostToDevice, c->stream));
  return VBA_OK;
}
// The four (point loop, update) pairs on an image that is on the device by then; which of them do any work is decided by the `done`
// flag in the image.  A loop that returns 0 rows (n == 0, a map never allocated) leaves the update alone, on no partials: d_part may
// then be NULL.  kd: the stop rule of the initialisation odometry.
template <class Loop>
static int odom_loop_queue(vba_ctx *c, const double *d_part, int kd, Loop loop) {
  for (int iter = 0; iter < vbh::ODOM_EKF_MAX_ITER; iter++) {
    const int nb = loop();
    hipLaunchKernelGGL(k_odom_update, dim3(1), dim3(256), 0, c->stream, c->sat->odom.d.p, d_part, nb, iter, kd);
  }
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}
// the one download of a call: the result block of the image into the pinned block
static int odom_result_download(vba_ctx *c) {
  const size_t r0 = offsetof(vbh::OdomEkf, x_curr), r1 = offsetof(vbh::OdomEkf, R);
  HIPCHK(c, hipMemcpyAsync((char *)c->sat->odom.h.p + r0, (const char *)c->sat->odom.d.p + r0, r1 - r0, hipMemcpyDeviceToHost, c->stream));
  return VBA_OK;
}
// The host form: the host inverts P once, writes one image and uploads it; the end downloads the result block, waits once and
// updates state and cov.  The call has completed on return and c->sat->odom.h holds the loop's result block.  Nothing here touches
// c->d_stage: a caller may keep the scan there.
static int odom_begin_host(vba_ctx *c, const double *state, const double *cov, bool kd) {
  odom_image_begin(*c->sat->odom.h, state, cov, kd);
  return odom_image_upload(c);
}
static int odom_end_host(vba_ctx *c, double *state, double *cov) {
  const int r = odom_result_download(c);
  if (r) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const vbh::OdomEkf &S = *c->sat->odom.h;
  std::memcpy(state, &S.x_curr, sizeof(S.x_curr));
  std::memcpy(cov, S.P_out, sizeof(S.P_out));
  return VBA_OK;
}
// The form on a state resident in HBM: the image is made from the state block by a kernel behind the block's last
// user.  The wait of the end is for the download alone: the copy back into the state block runs behind it, ordered before whatever
// reads the block next.
static int odom_begin_state(vba_ctx *c, vba_odom_state *st, bool kd) {
  const int r = odom_state_order(st, c->stream, c->err);
  if (r) return r;
  if (kd) hipLaunchKernelGGL(k_odom_begin_kd_dev, dim3(1), dim3(256), 0, c->stream, c->sat->odom.d.p, (const double *)st->d_blk.p);
  else hipLaunchKernelGGL(k_odom_begin_dev, dim3(1), dim3(256), 0, c->stream, c->sat->odom.d.p, (const double *)st->d_blk.p);
  return VBA_OK;
}
static int odom_end_state(vba_ctx *c, vba_odom_state *st, double *state_out) {
  const int r = odom_result_download(c);
  if (r) return r;
  HIPCHK(c, hipEventRecord(st->res_ev, c->stream));
  hipLaunchKernelGGL(k_odom_commit_dev, dim3(1), dim3(256), 0, c->stream, (const vbh::OdomEkf *)c->sat->odom.d.p, st->d_blk.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventSynchronize(st->res_ev));
  if (state_out) std::memcpy(state_out, &c->sat->odom.h->x_curr, sizeof(c->sat->odom.h->x_curr));
  return VBA_OK;
}
// The diagnostic tail: the pinned image uploaded as the caller left it, ONE point loop as odom_loop_queue queues it, the reduction of
// k_odom_update stored by k_odom_sums into d_sums [34], the stream drained.
template <class Loop>
static int odom_sums_run(vba_ctx *c, const double *d_part, double *d_sums, Loop loop) {
  const int r = odom_image_upload(c);
  if (r) return r;
  const int nb = loop();
  hipLaunchKernelGGL(k_odom_sums, dim3(1), dim3(256), 0, c->stream, d_part, nb, d_sums);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}
// the partials of a point loop of up to n points in workgroups of 256 (the voxel map's and, through sodom_part_ensure, the surfel map's)
static int odom_part_ensure(vba_ctx *c, int n) {
  const size_t need = (size_t)((n + 255) / 256) * 34;
  if (need > c->sat->odom.d_part.n) {
    size_t cap = 256 * 34;
    while (cap < need) cap *= 2;
    HIPCHK(c, c->sat->odom.d_part.ensure(cap));               // idle: the call that used it ended in a synchronise
  }
  return VBA_OK;
}

extern "C" {

// One point loop of the kd-tree update, as queued: search per slice, merge + fit, the 28 sums per workgroup.  n > 0.
static void kd_point_loop(hipStream_t s, const vbh::OdomEkf *d_S, int n, int kd_slices, const double *d_pts, int m, const double *tree,
                          unsigned long long *d_cand, double *d_pl, double *d_part) {
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_kd_match_dev, dim3(nb, kd_slices), dim3(256), 0, s, d_S, n, d_pts, m, tree, d_cand);
  hipLaunchKernelGGL(k_kd_fit_dev, dim3(nb), dim3(256), 0, s, d_S, n, kd_slices, (const unsigned long long *)d_cand, tree, d_pl);
  hipLaunchKernelGGL(k_kd_accum_dev, dim3(nb), dim3(256), 0, s, d_S, n, d_pts, (const double *)d_pl, d_part);
}

// One update on a scan in device memory, c->sat->kd.n + n <= 2^28, in three parts that the host-fed form (kd_odom_core) and the form on a
// state resident in HBM (vba_odom_lio_state_estimation_kdtree_on_state) share: kd_odom_ensure sizes the map halves and
// the scratch and says whether the scan only seeds the map (fewer than 100 map points, VS:1105-1118); kd_odom_queue queues the loop
// of the frame and behind it the append and the re-sampling; kd_odom_finish takes the new map size from the downloaded result block.
struct KdPlan {
  int nb, kd_slices;
  size_t tot;
  bool seed, det;
  int *d_cnt, *d_first;
  double *d_pl, *d_part;
  unsigned long long *d_cand;
  DsWork w;
};
static int kd_odom_ensure(vba_ctx *c, int n, KdPlan &p) {
  p = KdPlan{};
  p.nb = (n + 255) / 256; p.kd_slices = kd_slices_of(p.nb);
  p.tot = (size_t)c->sat->kd.n + (size_t)n;
  int st = kd_reserve(c, p.tot + 16);
  if (st) return st;
  p.seed = c->sat->kd.n < 100;
  if (p.seed) return VBA_OK;
  if ((st = odom_image_ensure(c)) || (st = kd_scan_ensure(c, (size_t)n)) || (st = kd_ws_ensure(c, p.tot))) return st;
  p.det = c->opt.deterministic != 0;
  p.d_cnt = (int *)c->sat->kd.d_ws.p; p.d_first = (int *)(c->sat->kd.d_ws + kd_up(c->sat->kd.ws_pts * sizeof(int)));
  char *ws = c->sat->kd.d_ws + 2 * kd_up(c->sat->kd.ws_pts * sizeof(int));
  if (2 * kd_up(c->sat->kd.ws_pts * sizeof(int)) + kf_ws_layout(c, (int)p.tot, p.det, ws, &p.w, &st) > c->sat->kd.d_ws.n || st) return st ? st : VBA_ERR_CAPACITY;
  const KdScanLayout L = kd_scan_layout(c->sat->kd.scan_pts);
  p.d_pl = (double *)c->sat->kd.d_scan.p; p.d_part = (double *)(c->sat->kd.d_scan + L.o_part);
  p.d_cand = (unsigned long long *)(c->sat->kd.d_scan + L.o_cand);
  return VBA_OK;
}
static int kd_odom_queue(vba_ctx *c, int n, const double *d_pts, KdPlan &p) {
  vbh::OdomEkf *d_S = c->sat->odom.d;
  hipStream_t s = c->stream;
  double *tree = c->sat->kd.d_tree[c->sat->kd.cur], *tree_out = c->sat->kd.d_tree[c->sat->kd.cur ^ 1];
  // n == 0: the point loop is skipped, nb == 0 and d_part may be NULL (no scan scratch was ever needed)
  int st = odom_loop_queue(c, p.d_part, 1, [&] {
    if (n > 0) kd_point_loop(s, d_S, n, p.kd_slices, d_pts, c->sat->kd.n, tree, p.d_cand, p.d_pl, p.d_part);
    return p.nb;
  });
  if (st) return st;
  // map update VS:1238-1250: the scan appended in the refined pose, map + scan re-sampled on a 0.5 m grid into the other half; the
  // voxel count lands in the result block
  if (n > 0) hipLaunchKernelGGL(k_kd_append_dev, dim3(p.nb), dim3(256), 0, s, (const vbh::OdomEkf *)d_S, n, d_pts, tree + (size_t)c->sat->kd.n * 3);
  p.w.n_out = &d_S->n_map;
  if ((st = ds_core(c, s, 0, (int)p.tot, tree, nullptr, 9, 4, 0.5, p.det, p.w))) return st;
  hipLaunchKernelGGL(k_ds_emit, dim3(((int)p.tot + 255) / 256), dim3(256), 0, s, (int)p.tot, (const DsSlot *)p.w.tab, (const int *)p.w.slot, (const int *)p.w.blk, tree_out,
                     p.d_cnt, p.d_first, (double *)nullptr, 0);
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}
// c->sat->odom.h holds the result block of the loop that kd_odom_queue queued
static int kd_odom_finish(vba_ctx *c, const KdPlan &p) {
  const vbh::OdomEkf &S = *c->sat->odom.h;
  if (S.n_map < 1 || (size_t)S.n_map > p.tot) { c->set_error("kd-tree odometry: voxel count of the re-sampled map out of range"); return VBA_ERR_HIP; }
  c->sat->kd.cur ^= 1; c->sat->kd.n = S.n_map;
  return VBA_OK;
}

// The host-fed form.  When the scan only seeds the map the append is enqueued, *ran stays false and nothing is waited for.  Otherwise
// the host form of the frame.
static int kd_odom_core(vba_ctx *c, int n, const double *d_pts, double *state, double *cov, bool *ran) {
  *ran = false;
  KdPlan p;
  int st = kd_odom_ensure(c, n, p);
  if (st) return st;
  if (p.seed) {
    if (n > 0) {
      KdPose X;
      std::memcpy(X.R, state + 1, sizeof(X.R)); std::memcpy(X.t, state + 10, sizeof(X.t));
      hipLaunchKernelGGL(k_kd_append, dim3(p.nb), dim3(256), 0, c->stream, n, d_pts, X, c->sat->kd.d_tree[c->sat->kd.cur] + (size_t)c->sat->kd.n * 3);
      HIPCHK(c, hipGetLastError());
    }
    c->sat->kd.n += n;
    return VBA_OK;
  }
  if ((st = odom_begin_host(c, state, cov, true)) || (st = kd_odom_queue(c, n, d_pts, p)) || (st = odom_end_host(c, state, cov)) ||
      (st = kd_odom_finish(c, p)))
    return st;
  *ran = true;
  return VBA_OK;
}

int vba_odom_lio_state_estimation_kdtree_resident(vba_ctx *c, int n, const double *d_pnt_body, double *state, double *cov, int *iterations,
                                                  vba_odom_report *report) {
  if (!c || n < 0 || (n > 0 && !d_pnt_body) || !state || !cov) return VBA_ERR_BAD_ARG;
  if (iterations) *iterations = 0;
  if (report) std::memset(report, 0, sizeof(*report));
  if ((size_t)c->sat->kd.n + (size_t)n > ((size_t)1 << 28)) return VBA_ERR_CAPACITY;
  bool ran;
  const int st = kd_odom_core(c, n, d_pnt_body, state, cov, &ran);
  if (st || !ran) return st;
  const vbh::OdomEkf &S = *c->sat->odom.h;
  if (iterations) *iterations = S.iterations;
  if (report) odom_report_fill(report, S, 0.0);
  return VBA_OK;
}

// The staging front end of the same update: the scan may be in host or device memory and the call has completed when it returns.
int vba_odom_lio_state_estimation_kdtree(vba_ctx *c, int n, const double *pnt_body, double *state, double *cov, int *iterations) {
  if (n < 0 || (n > 0 && !pnt_body) || !state || !cov) return VBA_ERR_BAD_ARG;
  if (iterations) *iterations = 0;
  if ((size_t)c->sat->kd.n + (size_t)n > ((size_t)1 << 28)) return VBA_ERR_CAPACITY;
  int st = ensure_stage(c, (size_t)n * 3 * sizeof(double));
  if (st) return st;
  if (n > 0) HIPCHK(c, hipMemcpyAsync(c->d_stage, pnt_body, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  bool ran;
  if ((st = kd_odom_core(c, n, (const double *)c->d_stage.p, state, cov, &ran))) return st;
  if (!ran) HIPCHK(c, hipStreamSynchronize(c->stream));                    // seeded: the core only enqueued the append
  else if (iterations) *iterations = c->sat->odom.h->iterations;
  return VBA_OK;
}

// ---------------------------------------------------------------- odometry scan-to-map (VS:962-1098)
// One update on a scan in device memory: the host form of the frame on the map's point loop.  Runs on this rank's map, whatever
// n_ranks is.
static int voxel_point_loop(vba_ctx *c, int n, const double *d_pts, const double *d_var, double *d_part) {
  return map_odom_point_loop(c->map, c->stream, c->sat->odom.d, n, d_pts, d_var, d_part);
}
static int voxel_odom_queue(vba_ctx *c, int n, const double *d_pts, const double *d_var) {
  double *d_part = c->sat->odom.d_part;
  return odom_loop_queue(c, d_part, 0, [=] { return voxel_point_loop(c, n, d_pts, d_var, d_part); });
}
// ok and the report from the downloaded result block: SelfAdjointEigenSolver(nnt).eigenvalues()[0] < 14 -> false  (VS:1090-1097)
static void voxel_odom_finish(const vbh::OdomEkf &S, int *ok, vba_odom_report *report) {
  const double emin = vbh::odom_nnt_eig_min(S.nnt);
  if (ok) *ok = (emin < 14) ? 0 : 1;
  if (report) odom_report_fill(report, S, emin);
}
static int odom_core(vba_ctx *c, int n, const double *d_pts, const double *d_var, double *state, double *cov) {
  int st = odom_image_ensure(c);
  if (st || (st = odom_part_ensure(c, n)) || (st = odom_begin_host(c, state, cov, false)) || (st = voxel_odom_queue(c, n, d_pts, d_var))) return st;
  return odom_end_host(c, state, cov);
}

int vba_odom_lio_state_estimation_resident(vba_ctx *c, int n, const double *d_pnt_body, const double *d_var_body, double *state, double *cov,
                                           int *ok, vba_odom_report *report) {
  if (n < 0 || (n > 0 && (!d_pnt_body || !d_var_body)) || !state || !cov) return VBA_ERR_BAD_ARG;
  if (c->n_ranks > 1) { c->set_error("the resident odometry loop has no all-reduce step between its iterations: unsharded contexts only"); return VBA_ERR_UNSUPPORTED; }
  const int st = odom_core(c, n, d_pnt_body, d_var_body, state, cov);
  if (st) return st;
  voxel_odom_finish(*c->sat->odom.h, ok, report);
  return VBA_OK;
}

// The staging front end of the same update: the scan may be in host or device memory, and a sharded context is accepted.
int vba_odom_lio_state_estimation(vba_ctx *c, int n, const double *pnt_body, const double *var_body, double *state, double *cov, int *ok) {
  if (n < 0 || (n > 0 && (!pnt_body || !var_body)) || !state || !cov) return VBA_ERR_BAD_ARG;
  int st = ensure_stage(c, (size_t)n * 12 * sizeof(double));             // [pts n*3 | var n*9]
  if (st) return st;
  double *d_pts = (double *)c->d_stage.p, *d_var = d_pts + (size_t)n * 3;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(d_pts, pnt_body, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_var, var_body, (size_t)n * 9 * sizeof(double), hipMemcpyDefault, c->stream));
  }
  if ((st = odom_core(c, n, d_pts, d_var, state, cov))) return st;
  voxel_odom_finish(*c->sat->odom.h, ok, nullptr);
  return VBA_OK;
}

// ---------------------------------------------------------------- diagnostic: one point loop of either variant (include/voxelba.h)
static bool all_finite(const double *a, size_t n) {
  for (size_t i = 0; i < n; i++) if (!std::isfinite(a[i])) return false;
  return true;
}
int vba_debug_odom_sums(vba_ctx *c, int kind, int n, const double *pnt_body, const double *var_body, const double *state, const double *cov,
                        int slices, double *partial, double *sums, unsigned long long *cand, double *planes, int *slices_used) {
  if (!c || !pnt_body || !state || !cov || !partial || !sums || n < 1 || n > (1 << 28)) return VBA_ERR_BAD_ARG;
  if (kind != VBA_ODOM_SUMS_VOXEL && kind != VBA_ODOM_SUMS_KD) return VBA_ERR_BAD_ARG;
  const bool kd = kind == VBA_ODOM_SUMS_KD;
  if (kd ? (!cand || !planes || slices < 0 || slices > 8 || c->sat->kd.n < 100) : (!var_body || slices != 0)) return VBA_ERR_BAD_ARG;
  if (!all_finite(state, 25) || !all_finite(cov, 225)) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (!is_device_ptr(pnt_body) && !all_finite(pnt_body, (size_t)n * 3)) return VBA_ERR_BAD_ARG;
  if (!kd && !is_device_ptr(var_body) && !all_finite(var_body, (size_t)n * 9)) return VBA_ERR_BAD_ARG;
  if (c->n_ranks > 1) { c->set_error("vba_debug_odom_sums runs the resident odometry loops: unsharded contexts only"); return VBA_ERR_UNSUPPORTED; }
  const int nb = (n + 255) / 256, ns = kd ? (slices ? slices : kd_slices_of(nb)) : 0;
  if (slices_used) *slices_used = ns;
  // the scan staged as the host-fed calls stage it; the outputs of the loop in buffers of this call: [sums 34 | partial nb * 34 |
  // planes n * 4], candidates [ns][n][5]
  int st = ensure_stage(c, (size_t)n * 12 * sizeof(double));
  if (st || (st = odom_image_ensure(c))) return st;
  double *d_pts = (double *)c->d_stage.p, *d_var = d_pts + (size_t)n * 3;
  DevMem<double> d_out;
  DevMem<unsigned long long> d_cand;
  HIPCHK(c, d_out.ensure(34 + (size_t)nb * 34 + (size_t)n * 4));
  if (kd) HIPCHK(c, d_cand.ensure((size_t)ns * n * 5));
  double *d_sums = d_out.p, *d_part = d_sums + 34, *d_pl = d_part + (size_t)nb * 34;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemsetAsync(d_out.p, 0, d_out.n * sizeof(double), s));
  HIPCHK(c, hipMemcpyAsync(d_pts, pnt_body, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, s));
  if (!kd) HIPCHK(c, hipMemcpyAsync(d_var, var_body, (size_t)n * 9 * sizeof(double), hipMemcpyDefault, s));
  odom_image_begin(*c->sat->odom.h, state, cov, kd);
  st = odom_sums_run(c, d_part, d_sums, [&] {
    if (!kd) return voxel_point_loop(c, n, d_pts, d_var, d_part);
    kd_point_loop(s, c->sat->odom.d, n, ns, d_pts, c->sat->kd.n, c->sat->kd.d_tree[c->sat->kd.cur], d_cand, d_pl, d_part);
    return nb;
  });
  if (st) { hipStreamSynchronize(s); return st; }                           // (nothing of this call is left in flight behind a status)
  hipError_t e = hipMemcpy(sums, d_sums, 34 * sizeof(double), hipMemcpyDefault);
  if (e == hipSuccess) e = hipMemcpy(partial, d_part, (size_t)nb * 34 * sizeof(double), hipMemcpyDefault);
  if (e == hipSuccess && kd) e = hipMemcpy(planes, d_pl, (size_t)n * 4 * sizeof(double), hipMemcpyDefault);
  if (e == hipSuccess && kd) e = hipMemcpy(cand, d_cand.p, (size_t)ns * n * 5 * sizeof(unsigned long long), hipMemcpyDefault);
  HIPCHK(c, e);
  return VBA_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the odometry state resident in HBM (vba_kernels_imu_ekf.hpp)
namespace vba {
int odom_state_order(vba_odom_state *st, hipStream_t stream, std::string &err) {
  if (st->last && st->last != stream) {
    // up_ev serves: recorded again on the same stream it only moves later, and the host waits for it before it writes a pinned block
    VBA_HIPCHK(err, hipEventRecord(st->up_ev, st->last));
    VBA_HIPCHK(err, hipStreamWaitEvent(stream, st->up_ev, 0));
    st->up_pending = true;
  }
  st->last = stream;
  return VBA_OK;
}
}  // namespace vba
static size_t ost_tab_doubles(int cap) { return (size_t)vbh::IE_ROW * (cap - 1) + 24; }
static size_t ost_up_doubles(int cap) { return (size_t)vbh::IE_PRM + (size_t)7 * cap; }
// the pinned blocks are free again once the copy (or the event of another stream's reader) recorded behind their last use has passed
static int ost_pinned_free(vba_odom_state *st) {
  if (st->up_pending) { HIPCHK(st->ctx, hipEventSynchronize(st->up_ev)); st->up_pending = false; }
  return VBA_OK;
}
static int ost_drain(vba_odom_state *st) {
  vba_ctx *c = st->ctx;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (st->last && st->last != c->stream) HIPCHK(c, hipDeviceSynchronize());
  st->up_pending = false;
  return VBA_OK;
}
// grow-only by doubling; the table's contents do not survive (a propagation rewrites all of them)
static int ost_ensure(vba_odom_state *st, int rows) {
  if (rows <= st->cap) return VBA_OK;
  vba_ctx *c = st->ctx;
  int cap = st->cap ? st->cap : 64;
  while (cap < rows) cap *= 2;
  int r = ost_drain(st);
  if (r) return r;
  st->cap = 0; st->n_poses = 0;
  const size_t tab = ost_tab_doubles(cap), up = ost_up_doubles(cap), pin = std::max<size_t>(ODOM_STATE_BLOCK, tab);
  HIPCHK(c, st->d_tab.ensure(tab)); HIPCHK(c, st->d_up.ensure(up));
  HIPCHK(c, st->h_up.ensure(up)); HIPCHK(c, st->h_blk.ensure(pin));
  st->cap = cap; st->allocs += 4; st->bytes += (int64_t)((tab + 2 * up + pin) * sizeof(double));
  return VBA_OK;
}

extern "C" {

int vba_imu_ekf_propagate(int m, const double *imu, const double *noise, double scale_gravity, double last_pcl_end_time, double pcl_beg_time,
                          double pcl_end_time, double *state, double *cov, double *imu_poses, double *end_pose, int *n_poses) {
  if (!imu || !noise || !state || !cov || !imu_poses || !end_pose || !n_poses || m < 2) return VBA_ERR_BAD_ARG;
  double prm[vbh::IE_PRM] = {last_pcl_end_time, pcl_beg_time, pcl_end_time, scale_gravity};
  std::memcpy(prm + vbh::IE_NOISE, noise, 12 * sizeof(double));
  if (!vbh::imu_ekf_args_ok(m, imu, prm) || !all_finite(state, 25) || !all_finite(cov, 225)) return VBA_ERR_BAD_ARG;
  std::vector<double> w(vbh::IE_WORK);
  vbh::State x;
  std::memcpy(&x, state, sizeof(x));
  *n_poses = vbh::imu_ekf_propagate(w.data(), m, imu, prm, &x, cov, imu_poses, end_pose, 0, 1, [] {});
  std::memcpy(state, &x, sizeof(x));
  return VBA_OK;
}

int vba_odom_state_create(vba_ctx *c, vba_odom_state **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  vba_odom_state *st = new vba_odom_state();
  st->ctx = c;
  int r = ost_ensure(st, 64);
  if (!r && st->d_blk.ensure(ODOM_STATE_BLOCK) != hipSuccess) r = VBA_ERR_HIP;
  if (!r && hipMemsetAsync(st->d_blk.p, 0, ODOM_STATE_BLOCK * sizeof(double), c->stream) != hipSuccess) r = VBA_ERR_HIP;
  if (!r && hipEventCreateWithFlags(&st->up_ev, hipEventDisableTiming) != hipSuccess) r = VBA_ERR_HIP;
  if (!r && hipEventCreateWithFlags(&st->res_ev, hipEventDisableTiming) != hipSuccess) r = VBA_ERR_HIP;
  if (r) { vba_odom_state_destroy(st); return r; }
  st->allocs++; st->bytes += (int64_t)(ODOM_STATE_BLOCK * sizeof(double));
  st->last = c->stream;
  *out = st;
  return VBA_OK;
}

void vba_odom_state_destroy(vba_odom_state *st) {
  if (!st) return;
  hipSetDevice(st->ctx->device);
  hipStreamSynchronize(st->ctx->stream);
  if (st->last && st->last != st->ctx->stream) hipDeviceSynchronize();
  if (st->up_ev) hipEventDestroy(st->up_ev);
  if (st->res_ev) hipEventDestroy(st->res_ev);
  delete st;
}

int vba_odom_state_reserve(vba_odom_state *st, int max_imu_rows) {
  if (!st || max_imu_rows < 0 || max_imu_rows > (1 << 20)) return VBA_ERR_BAD_ARG;
  HIPCHK(st->ctx, hipSetDevice(st->ctx->device));
  return ost_ensure(st, max_imu_rows);
}

int vba_odom_state_allocations(vba_odom_state *st, int *n_allocs, int64_t *bytes) {
  if (!st || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = st->allocs; *bytes = st->bytes;
  return VBA_OK;
}

int vba_odom_state_set(vba_odom_state *st, const double *state, const double *cov) {
  if (!st || !state || !cov || !all_finite(state, 25) || !all_finite(cov, 225)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = st->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int r = ost_pinned_free(st);
  if (r || (r = odom_state_order(st, c->stream, c->err))) return r;
  std::memcpy(st->h_blk.p, state, 25 * sizeof(double));
  std::memcpy(st->h_blk.p + 25, cov, 225 * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(st->d_blk.p, st->h_blk.p, 250 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(st->up_ev, c->stream));
  st->up_pending = true;
  return VBA_OK;
}

int vba_odom_state_get(vba_odom_state *st, double *state, double *cov) {
  if (!st) return VBA_ERR_BAD_ARG;
  vba_ctx *c = st->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int r = ost_pinned_free(st);
  if (r || (r = odom_state_order(st, c->stream, c->err))) return r;
  HIPCHK(c, hipMemcpyAsync(st->h_blk.p, st->d_blk.p, 250 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  st->up_pending = false;
  if (state) std::memcpy(state, st->h_blk.p, 25 * sizeof(double));
  if (cov) std::memcpy(cov, st->h_blk.p + 25, 225 * sizeof(double));
  return VBA_OK;
}

int vba_odom_state_poses(vba_odom_state *st, int max_rows, double *imu_poses, double *end_pose, int *n_poses) {
  if (!st || max_rows < 0) return VBA_ERR_BAD_ARG;
  if (n_poses) *n_poses = st->n_poses;
  if (imu_poses && st->n_poses > max_rows) return VBA_ERR_CAPACITY;
  vba_ctx *c = st->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int r = ost_pinned_free(st);
  if (r || (r = odom_state_order(st, c->stream, c->err))) return r;
  const size_t nd = (size_t)vbh::IE_ROW * st->n_poses + 12;
  HIPCHK(c, hipMemcpyAsync(st->h_blk.p, st->d_tab.p, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  st->up_pending = false;
  if (imu_poses) std::memcpy(imu_poses, st->h_blk.p, (nd - 12) * sizeof(double));
  if (end_pose) std::memcpy(end_pose, st->h_blk.p + nd - 12, 12 * sizeof(double));
  return VBA_OK;
}

int vba_odom_state_propagate(vba_odom_state *st, const double *noise, double scale_gravity, int m, const double *imu, double last_pcl_end_time,
                             double pcl_beg_time, double pcl_end_time, int *n_poses) {
  if (!st || !noise || !imu || !n_poses || m < 2 || m > (1 << 20)) return VBA_ERR_BAD_ARG;
  double prm[vbh::IE_PRM] = {last_pcl_end_time, pcl_beg_time, pcl_end_time, scale_gravity};
  std::memcpy(prm + vbh::IE_NOISE, noise, 12 * sizeof(double));
  if (!vbh::imu_ekf_args_ok(m, imu, prm)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = st->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int r = ost_ensure(st, m);
  if (r || (r = ost_pinned_free(st)) || (r = odom_state_order(st, c->stream, c->err))) return r;
  std::memcpy(st->h_up.p, prm, sizeof(prm));
  std::memcpy(st->h_up.p + vbh::IE_PRM, imu, (size_t)7 * m * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(st->d_up.p, st->h_up.p, ost_up_doubles(m) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(st->up_ev, c->stream));
  st->up_pending = true;
  const int rows = vbh::imu_ekf_count(m, imu, last_pcl_end_time);
  hipLaunchKernelGGL(k_imu_propagate, dim3(1), dim3(256), 0, c->stream, m, rows, (const double *)st->d_up.p, st->d_blk.p, st->d_tab.p);
  HIPCHK(c, hipGetLastError());
  *n_poses = st->n_poses = rows;
  return VBA_OK;
}

int vba_odom_lio_state_estimation_on_state(vba_ctx *c, vba_odom_state *st, int n, const double *d_pnt_body, const double *d_var_body, int *ok,
                                           vba_odom_report *report, double *state_out) {
  if (!c || !st || n < 0 || (n > 0 && (!d_pnt_body || !d_var_body)) || c->device != st->ctx->device) return VBA_ERR_BAD_ARG;
  if (c->n_ranks > 1) { c->set_error("the resident odometry loop has no all-reduce step between its iterations: unsharded contexts only"); return VBA_ERR_UNSUPPORTED; }
  HIPCHK(c, hipSetDevice(c->device));
  int r = odom_image_ensure(c);
  if (r || (r = odom_part_ensure(c, n)) || (r = odom_begin_state(c, st, false)) || (r = voxel_odom_queue(c, n, d_pnt_body, d_var_body)) ||
      (r = odom_end_state(c, st, state_out)))
    return r;
  voxel_odom_finish(*c->sat->odom.h, ok, report);
  return VBA_OK;
}

int vba_map_pvec_update_cut_voxel_on_state(vba_ctx *c, vba_odom_state *st, int win_count, int n, const double *d_pnt_body, const double *d_var_body,
                                           int multi) {
  if (!c || !st || !d_var_body || c->device != st->ctx->device) return VBA_ERR_BAD_ARG;
  if (c->n_ranks > 1) { c->set_error("the insertion on a resident odometry state runs on one rank's map: unsharded contexts only"); return VBA_ERR_UNSUPPORTED; }
  HIPCHK(c, hipSetDevice(c->device));
  const int r = odom_state_order(st, c->stream, c->err);
  if (r) return r;
  return map_cut_voxel(c->map, c->stream, win_count, n, d_pnt_body, d_var_body, nullptr, multi != 0, c->err, nullptr, st->d_blk.p);
}

// ---------------------------------------------------------------- the initialisation odometry on a state object
int vba_odom_lio_state_estimation_kdtree_on_state(vba_ctx *c, vba_odom_state *st, int n, const double *d_pnt_body, int *iterations,
                                                  vba_odom_report *report, double *state_out) {
  if (!c || !st || !iterations || n < 0 || (n > 0 && !d_pnt_body) || c->device != st->ctx->device) return VBA_ERR_BAD_ARG;
  *iterations = 0;
  if (report) std::memset(report, 0, sizeof(*report));
  if ((size_t)c->sat->kd.n + (size_t)n > ((size_t)1 << 28)) return VBA_ERR_CAPACITY;
  HIPCHK(c, hipSetDevice(c->device));
  KdPlan p;
  int r = kd_odom_ensure(c, n, p);
  if (r) return r;
  hipStream_t s = c->stream;
  if (p.seed) {
    // the scan only seeds the map: the block is read and not written.  The download of state_out goes ahead of the append, which it
    // does not depend on, and is all that the host waits for
    if (state_out && (r = ost_pinned_free(st))) return r;
    if ((r = odom_state_order(st, s, c->err))) return r;
    if (state_out) {
      HIPCHK(c, hipMemcpyAsync(st->h_blk.p, st->d_blk.p, 25 * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipEventRecord(st->res_ev, s));
    }
    if (n > 0) {
      hipLaunchKernelGGL(k_kd_append_blk, dim3(p.nb), dim3(256), 0, s, (const double *)st->d_blk.p, n, d_pnt_body, c->sat->kd.d_tree[c->sat->kd.cur] + (size_t)c->sat->kd.n * 3);
      HIPCHK(c, hipGetLastError());
    }
    c->sat->kd.n += n;
    if (state_out) {
      HIPCHK(c, hipEventSynchronize(st->res_ev));
      std::memcpy(state_out, st->h_blk.p, 25 * sizeof(double));
    }
    return VBA_OK;
  }
  if ((r = odom_begin_state(c, st, true)) || (r = kd_odom_queue(c, n, d_pnt_body, p)) || (r = odom_end_state(c, st, state_out)) ||
      (r = kd_odom_finish(c, p)))
    return r;
  *iterations = c->sat->odom.h->iterations;
  if (report) odom_report_fill(report, *c->sat->odom.h, 0.0);
  return VBA_OK;
}

// pub_localtraj's point loop (VS:37-45) on the scan that the insertion would transform: the pose is read from the state block
int vba_odom_state_export_scan(vba_ctx *c, vba_odom_state *st, int n, const double *d_pnt_body, float intensity, int64_t cap, float *xyzi,
                               int64_t *n_out) {
  if (!c || !st || !n_out || n < 0 || cap < n || (n > 0 && (!d_pnt_body || !xyzi)) || c->device != st->ctx->device) return VBA_ERR_BAD_ARG;
  *n_out = n;
  if (n == 0) return VBA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev_out = is_device_ptr(xyzi);
  if (dev_out && ((uintptr_t)xyzi & 15)) { c->set_error("vba_odom_state_export_scan: a device xyzi must be 16-byte aligned"); return VBA_ERR_BAD_ARG; }
  int r;
  if (!dev_out && (r = ensure_stage(c, (size_t)n * sizeof(float4)))) return r;
  if ((r = odom_state_order(st, c->stream, c->err))) return r;
  float4 *out = dev_out ? (float4 *)xyzi : (float4 *)c->d_stage.p;
  hipLaunchKernelGGL(k_odom_state_export, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d_pnt_body, (const double *)st->d_blk.p, intensity, out);
  HIPCHK(c, hipGetLastError());
  if (!dev_out) {
    HIPCHK(c, hipMemcpyAsync(xyzi, out, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VBA_OK;
}

// ---------------------------------------------------------------- the update against a prior map
// The iterated-EKF update of the 15-state against the cells of a surfel map: the point loop is k_sodom_accum (vba_surfreg.hip queues
// it), whose rows k_odom_update reduces and steps on with kd = 0 as it does for the voxel map.  Image, pinned block and partials are
// the context's (c->sat->odom).
void vba_surfel_odom_default_params(vba_surfel_odom_params *p) {
  if (!p) return;
  p->gate = 3.0; p->neighbors = 7; p->min_matches = 30; p->min_eig = 0.0;
}
static bool sodom_params_ok(const vba_surfel_odom_params *p) {
  return p && (p->neighbors == 1 || p->neighbors == 7) && p->gate > 0.0 && std::isfinite(p->gate) && p->min_matches >= 0 && p->min_eig >= 0.0;
}
static int sodom_unsharded(vba_ctx *c, const char *who) {
  if (c->n_ranks > 1 || c->rank != 0) { c->set_error(std::string(who) + ": sharded contexts are not supported"); return VBA_ERR_UNSUPPORTED; }
  return VBA_OK;
}
// the rows of the context's partials that a point loop of n points writes
static int sodom_part_ensure(vba_ctx *c, int n) { return odom_part_ensure(c, 256 * surfel_odom_blocks(n)); }
// the loop of the frame on the surfel map's point loop; n == 0 launches the updates alone, on no partials
static int sodom_queue(vba_ctx *c, vba_surfel_map *m, int n, const double *d_pnt, const vba_surfel_odom_params *p) {
  double *d_part = c->sat->odom.d_part;
  return odom_loop_queue(c, d_part, 0, [=] {
    return n > 0 ? surfel_odom_queue(m, c->stream, c->sat->odom.d, n, d_pnt, p->gate, p->neighbors, d_part, nullptr, nullptr, nullptr) : 0;
  });
}
// ok and the report from the downloaded result block
static void sodom_finish(const vbh::OdomEkf &S, const vba_surfel_odom_params *p, int *ok, vba_odom_report *report) {
  const double emin = vbh::odom_nnt_eig_min(S.nnt);
  const int last = S.iterations > 0 ? S.match_num[S.iterations - 1] : 0;
  if (ok) *ok = (last >= p->min_matches && emin >= p->min_eig) ? 1 : 0;
  if (report) odom_report_fill(report, S, emin);
}

int vba_odom_surfel_update(vba_ctx *c, vba_surfel_map *m, int n, const double *pnt_body, const vba_surfel_odom_params *p, double *state,
                           double *cov, int *ok, vba_odom_report *report) {
  if (!c || !m || !state || !cov || n < 0 || (n > 0 && !pnt_body) || !sodom_params_ok(p) || !surfel_odom_args_ok(m, c, n, pnt_body)) return VBA_ERR_BAD_ARG;
  int st = sodom_unsharded(c, "vba_odom_surfel_update");
  if (st) return st;
  HIPCHK(c, hipSetDevice(c->device));
  const double *d_pnt;
  if ((st = odom_image_ensure(c)) || (st = sodom_part_ensure(c, n)) || (st = surfel_odom_stage(m, n, pnt_body, &d_pnt))) return st;
  if ((st = odom_begin_host(c, state, cov, false)) || (st = sodom_queue(c, m, n, d_pnt, p)) || (st = odom_end_host(c, state, cov))) return st;
  sodom_finish(*c->sat->odom.h, p, ok, report);
  return VBA_OK;
}

int vba_odom_surfel_update_on_state(vba_ctx *c, vba_odom_state *st, vba_surfel_map *m, int n, const double *d_pnt_body,
                                    const vba_surfel_odom_params *p, int *ok, vba_odom_report *report, double *state_out) {
  if (!c || !st || !m || n < 0 || (n > 0 && !d_pnt_body) || !sodom_params_ok(p) || c->device != st->ctx->device ||
      !surfel_odom_args_ok(m, c, n, d_pnt_body))
    return VBA_ERR_BAD_ARG;
  int r = sodom_unsharded(c, "vba_odom_surfel_update_on_state");
  if (r) return r;
  HIPCHK(c, hipSetDevice(c->device));
  const double *d_pnt;
  if ((r = odom_image_ensure(c)) || (r = sodom_part_ensure(c, n)) || (r = surfel_odom_stage(m, n, d_pnt_body, &d_pnt)) ||
      (r = odom_begin_state(c, st, false)) || (r = sodom_queue(c, m, n, d_pnt, p)) || (r = odom_end_state(c, st, state_out)))
    return r;
  sodom_finish(*c->sat->odom.h, p, ok, report);
  return VBA_OK;
}

int vba_debug_odom_surfel_sums(vba_ctx *c, vba_surfel_map *m, int n, const double *pnt_body, const vba_surfel_odom_params *p, const double *R,
                               const double *t, int cap_rows, double *partial, double *cost, double *sums, int *cell, unsigned char *gate, int *nb_out) {
  if (!c || !m || !R || !t || n < 1 || !pnt_body || cap_rows < 0 || !sodom_params_ok(p) || !all_finite(R, 9) || !all_finite(t, 3) ||
      !surfel_odom_args_ok(m, c, n, pnt_body))
    return VBA_ERR_BAD_ARG;
  int st = sodom_unsharded(c, "vba_debug_odom_surfel_sums");
  if (st) return st;
  const int nb = surfel_odom_blocks(n);
  if (nb_out) *nb_out = nb;
  if ((partial || cost) && cap_rows < nb) return VBA_ERR_CAPACITY;
  HIPCHK(c, hipSetDevice(c->device));
  const double *d_pnt;
  if ((st = odom_image_ensure(c)) || (st = sodom_part_ensure(c, n)) || (st = surfel_odom_stage(m, n, pnt_body, &d_pnt))) return st;
  // the taps in buffers of this call: [sums 34 | cost nb] doubles, [cell n] ints, [gate n] bytes
  DevMem<double> d_out; DevMem<int> d_cell; DevMem<unsigned char> d_gate;
  HIPCHK(c, d_out.ensure(34 + (size_t)nb));
  HIPCHK(c, d_cell.ensure((size_t)n));
  HIPCHK(c, d_gate.ensure((size_t)n));
  // an image of which the point loop reads the pose and the flag alone
  vbh::OdomEkf &S = *c->sat->odom.h;
  std::memset(&S, 0, sizeof(S));
  std::memcpy(S.R, R, sizeof(S.R)); std::memcpy(S.t, t, sizeof(S.t));
  double *d_part = c->sat->odom.d_part.p;
  if ((st = odom_sums_run(c, d_part, d_out.p, [&] {
        return surfel_odom_queue(m, c->stream, c->sat->odom.d, n, d_pnt, p->gate, p->neighbors, d_part, d_out.p + 34, d_cell.p, d_gate.p);
      })))
    return st;
  hipError_t e = hipSuccess;
  if (sums) e = hipMemcpy(sums, d_out.p, 34 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && cost) e = hipMemcpy(cost, d_out.p + 34, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && partial) e = hipMemcpy(partial, d_part, (size_t)nb * 34 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && cell) e = hipMemcpy(cell, d_cell.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess && gate) e = hipMemcpy(gate, d_gate.p, (size_t)n, hipMemcpyDeviceToHost);
  HIPCHK(c, e);
  return VBA_OK;
}

}  // extern "C"
