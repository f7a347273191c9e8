// libvoxelba.so: LiDAR-inertial initialisation (vba_init_imu_poses, vba_init_align_gravity, vba_motion_init, and the device-resident
// window of raw clouds: vba_init_window_*, vba_motion_init_resident).  The kernels of vba_kernels_init.hpp, compiled
// here and nowhere else; the map is reached through map_* (vba_ctx.hpp) and the down-sampler's pass through ds_core (vba_kf_store_decl.hpp), the LI-BA and
// the IMU pre-integration of the BA core (voxelba.hip) through the C ABI.
#include "vba_ctx.hpp"
#include "vba_sat.hpp"
#include "vba_kf_store_decl.hpp"
#include "vba_scan_frame.hpp"
#include "vba_kernels_init.hpp"
#include "vba_hostmath.hpp"
#include "vba_init_window.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

extern "C" {

// ---------------------------------------------------------------- LiDAR-inertial initialisation (VS:617-819)
int vba_init_imu_poses(int m, const double *imu, const double *state_c, const double *state_l, double beg_time, double scale_gravity,
                       double *out) {
  if (m < 0 || (m > 0 && !imu) || !state_c || !state_l || (m > 1 && !out)) return VBA_ERR_BAD_ARG;
  init_imu_poses(m, imu, state_c, state_l, beg_time, scale_gravity, out);
  return VBA_OK;
}
int vba_init_align_gravity(int n, double *states) {
  if (n < 1 || !states) return VBA_ERR_BAD_ARG;
  init_align_gravity(n, states);
  return VBA_OK;
}

namespace {
// Restores the map's own thresholds however vba_motion_init returns (the context's options are never written).
struct ThrOverride {
  MapStore &s;
  explicit ThrOverride(MapStore &m) : s(m) {}
  void set(bool on) {
    s.thr_override = on;
    s.ovr_min_eigen_value = 0.02;                              // VS:624-627
    for (int k = 0; k < 4; k++) s.ovr_plane_thre[k] = 1.0 / 4; // VS:628-630 (stored inverted)
  }
  ~ThrOverride() { s.thr_override = false; }
};
}

// Argument checks of both entry points (pnt / curv: the host arrays, or the window's device arrays).
static int motion_init_check(vba_ctx *c, int W, const int *pt_offsets, const double *pnt, const double *curv, const int *imu_offsets, const double *imu,
                             const double *beg_times, const double *ext_pose, const double *nm6, const double *nw6, double *states, const double *covs,
                             double *imus, int *converged, double *eigvalue3, int *iterations, int *thresholds_left_relaxed, double *round_log,
                             int max_rounds, double *pnt_out, double *var_out, int *pvec_offsets) {
  if (!c || W != c->opt.win_size || W < 2 || !pt_offsets || !imu_offsets || !beg_times || !ext_pose || !nm6 || !nw6 || !states || !covs || !imus ||
      !converged || !eigvalue3 || !iterations || !thresholds_left_relaxed || (round_log && max_rounds < 0) || (pnt_out && (!var_out || !pvec_offsets)))
    return VBA_ERR_BAD_ARG;
  if (!li_device_supported(W)) return VBA_ERR_UNSUPPORTED_WINDOW;
  const int np = pt_offsets[W];
  if (pt_offsets[0] != 0 || np < 0 || (np > 0 && (!pnt || !curv)) || imu_offsets[0] != 0 || imu_offsets[W] < 0 || (imu_offsets[W] > 0 && !imu))
    return VBA_ERR_BAD_ARG;
  for (int i = 0; i < W; i++)
    if (pt_offsets[i + 1] < pt_offsets[i] || imu_offsets[i + 1] < imu_offsets[i]) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < W; i++) {                   // each deque's times ascend (the blur's binary search needs descending pose times)
    for (int k = imu_offsets[i] + 1; k < imu_offsets[i + 1]; k++)
      if (imu[7 * (size_t)k] < imu[7 * (size_t)(k - 1)]) return VBA_ERR_BAD_ARG;
    if (i > 0 && imu_offsets[i + 1] == imu_offsets[i]) return VBA_ERR_BAD_ARG;   // IMU_PRE::push_imu needs samples (VS:729)
  }
  return VBA_OK;
}

// Does scan i walk its curvatures (VS:562-599)?  Not with point_notime, without poses or without points.
static bool init_scan_walks(int i, const int *pt_offsets, const int *imu_offsets, int point_notime) {
  return !point_notime && imu_offsets[i + 1] - imu_offsets[i] > 1 && pt_offsets[i + 1] > pt_offsets[i];
}

// The body both entry points share, after motion_init_check.  The clouds are host arrays that are uploaded once into sat->init.d
// (vba_motion_init), or, with h_pnt == nullptr, the device arrays d_pnt / d_cv read in place (vba_motion_init_resident).  walk [W]
// holds the walk's two inputs for every scan that init_scan_walks.
static int motion_init_impl(vba_ctx *c, int W, const int *pt_offsets, const double *h_pnt, const double *h_curv, const double *d_pnt, const double *d_cv,
                    const InitWalk *walk, const int *imu_offsets, const double *imu,
                    const double *beg_times, const double *ext_pose, double dept_err, double beam_err, double scale_gravity, int point_notime,
                    const double *nm6, const double *nw6, double *states, const double *covs, double *imus, double *hess, int *converged,
                    double *eigvalue3, int *iterations, int *thresholds_left_relaxed, double *round_log, int max_rounds, double *pnt_out,
                    double *var_out, int *pvec_offsets, int pvec_cap, bool &started) {
  const int np = pt_offsets[W];
  const bool upload = h_pnt != nullptr;

  // The walk's shape depends on the curvatures and the IMU / scan times only, not on the states: rows per scan are fixed for the call.
  std::vector<InitScan> scans(W);
  int n_out = 0, n_pose = 0;
  for (int i = 0; i < W; i++) {
    InitScan &S = scans[i];
    std::memset(&S, 0, sizeof(S));
    S.pt_off = pt_offsets[i]; S.n_pts = pt_offsets[i + 1] - pt_offsets[i];
    const int m = imu_offsets[i + 1] - imu_offsets[i];
    S.pose_off = n_pose; S.n_pose = m > 1 ? m - 1 : 0;
    S.notime = point_notime != 0;
    S.k0 = -1;
    if (S.notime) { S.j_min = 0; S.n_out = S.n_pts; }
    else if (S.n_pose == 0 || S.n_pts == 0) { S.j_min = S.n_pts; S.n_out = 0; }
    else {
      const double *im = imu + 7 * (size_t)imu_offsets[i];
      const int j = walk[i].j_min;                                                  // the walk stops at the first point at or before the oldest pose
      const double cv0 = walk[i].cv0;
      S.j_min = j;
      int dups = 0;
      if (j == 0) {
        int k = 0;                                                                  // pose that pushes point 0: first with t < curvature
        while (k < S.n_pose && !((im[7 * (size_t)(m - 2 - k)] - beg_times[i]) < cv0)) k++;
        S.k0 = k;
        dups = S.n_pose - 1 - k;
      }
      S.n_out = S.n_pts - j + dups;
    }
    S.out_off = n_out;
    n_out += S.n_out;
    n_pose += S.n_pose;
    S.range_inc = (float)dept_err; S.degree_inc = (float)beam_err;
    for (int k = 0; k < 9; k++) S.Rx[k] = ext_pose[k];
    for (int k = 0; k < 3; k++) S.tx[k] = ext_pose[9 + k];
  }
  if (pvec_offsets) for (int i = 0; i <= W; i++) pvec_offsets[i] = i < W ? scans[i].out_off : n_out;
  if (pnt_out && n_out > pvec_cap) return VBA_ERR_CAPACITY;

  // the IMU deques split once for the re-preintegration (VS:724-730)
  std::vector<std::vector<double>> it(W), ig(W), ia(W);
  for (int i = 0; i < W; i++) {
    const int m = imu_offsets[i + 1] - imu_offsets[i];
    const double *im = imu + 7 * (size_t)imu_offsets[i];
    it[i].resize(m); ig[i].resize(3 * (size_t)m); ia[i].resize(3 * (size_t)m);
    for (int k = 0; k < m; k++) {
      it[i][k] = im[7 * k];
      for (int q = 0; q < 3; q++) { ig[i][3 * k + q] = im[7 * k + 1 + q]; ia[i][3 * k + q] = im[7 * k + 4 + q]; }
    }
  }
  // device buffer: raw cloud + curvatures (uploaded once; absent with resident clouds), blurred rows + their var, pose tables, scan
  // table, Σ n nᵀ partials and result
  const size_t b_pnt = upload ? (size_t)np * 24 : 0, b_cv = upload ? (size_t)np * 8 : 0, b_pb = (size_t)n_out * 24, b_var = (size_t)n_out * 72,
               b_pose = (size_t)n_pose * INIT_POSE_LEN * 8, b_sc = (size_t)W * sizeof(InitScan), b_nnt = (size_t)(INIT_NNT_WG * 6 + 16) * 8;
  const size_t need = b_pnt + b_cv + b_pb + b_var + b_pose + b_sc + b_nnt + 64;
  HIPCHK(c, c->sat->init.d.ensure(need));
  char *base = c->sat->init.d;
  if (upload) { d_pnt = (double *)base; d_cv = (double *)(base + b_pnt); }
  double *d_pb = (double *)(base + b_pnt + b_cv), *d_var = (double *)(base + b_pnt + b_cv + b_pb), *d_pose = (double *)(base + b_pnt + b_cv + b_pb + b_var);
  InitScan *d_sc = (InitScan *)(base + b_pnt + b_cv + b_pb + b_var + b_pose);
  double *d_part = (double *)(base + b_pnt + b_cv + b_pb + b_var + b_pose + b_sc), *d_nnt = d_part + INIT_NNT_WG * 6;
  if (upload && np > 0) {
    HIPCHK(c, hipMemcpyAsync(base, h_pnt, b_pnt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + b_pnt, h_curv, b_cv, hipMemcpyHostToDevice, c->stream));
  }

  ThrOverride thr(c->map);
  thr.set(true);
  started = true;                                 // from here on a failure leaves device state behind
  bool relaxed = true;
  std::vector<double> ptab((size_t)n_pose * INIT_POSE_LEN + 1);
  std::vector<double> poses((size_t)W * 12);
  double last_nnt[9] = {0};
  int converge_flag = 0, rounds = 0, st = VBA_OK;
  double converge_thre = 0.05;
  bool is_degrade = true;
  double eig[3] = {0, 0, 0};
  for (int iterCnt = 0; iterCnt < 10; iterCnt++) {
    rounds = iterCnt + 1;
    if (converge_flag == 1 && relaxed) { thr.set(false); relaxed = false; }    // VS:643-647
    st = map_reset(c->map, c->stream, c->err); if (st) return st;              // VS:650-661
    for (int i = 0; i < W; i++) {
      InitScan &S = scans[i];
      const double *xc = states + (size_t)VBA_STATE_LEN * i, *xl = states + (size_t)VBA_STATE_LEN * (i == 0 ? 0 : i - 1);
      if (!S.notime && S.n_pose > 0)
        init_imu_poses(S.n_pose + 1, imu + 7 * (size_t)imu_offsets[i], xc, xl, beg_times[i], scale_gravity, ptab.data() + (size_t)INIT_POSE_LEN * S.pose_off);
      for (int k = 0; k < 9; k++) S.R[k] = xc[1 + k];
      for (int k = 0; k < 3; k++) S.p[k] = xc[10 + k];
      const double *cv = covs + (size_t)VBA_DIM * VBA_DIM * i;
      for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) { S.cov6[3 * r + k] = cv[r * VBA_DIM + k]; S.cov6[9 + 3 * r + k] = cv[(3 + r) * VBA_DIM + 3 + k]; }
      S.conv = converge_flag;
      for (int k = 0; k < 9; k++) poses[12 * i + k] = xc[1 + k];
      for (int k = 0; k < 3; k++) poses[12 * i + 9 + k] = xc[10 + k];
    }
    if (n_pose > 0) HIPCHK(c, hipMemcpyAsync(d_pose, ptab.data(), b_pose, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_sc, scans.data(), b_sc, hipMemcpyHostToDevice, c->stream));
    if (n_out > 0) {
      TimedSpan sp{};
      span_begin(c, "init", sp);
      hipLaunchKernelGGL(k_init_blur, dim3((n_out + 255) / 256), dim3(256), 0, c->stream, W, n_out, d_sc, d_pose, d_pnt, d_cv, d_pb, d_var);
      span_end(c, "init", sp);
      HIPCHK(c, hipGetLastError());
    }
    // cut_voxel (VM:1896) per scan with win_count = i, straight from the blurred rows in HBM
    for (int i = 0; i < W; i++) {
      TimedSpan sp{};
      span_begin(c, "insert", sp);
      st = map_cut_voxel(c->map, c->stream, i, scans[i].n_out, d_pb + 3 * (size_t)scans[i].out_off, d_var + 9 * (size_t)scans[i].out_off,
                         poses.data() + 12 * i, false, c->err);
      span_end(c, "insert", sp);
      if (st) return st;
    }
    st = vba_map_recut(c, W, poses.data(), 0); if (st) return st;               // recut + tras_opt over surf_map (VS:695-703)
    const int nf = c->nvox;
    double resis[2] = {0, 0};
    double *log = (round_log && iterCnt < max_rounds) ? round_log + 5 * iterCnt : nullptr;
    if (log) { log[0] = nf; log[1] = log[2] = 0.0; log[3] = vbh::norm3(states + 22); log[4] = converge_flag; }
    if (nf < 10) break;                                                         // VS:706-707
    st = vba_li_ba_damping_iter(c, states, imus, 1, 3, hess, resis); if (st) return st;   // LI_BA_OptimizerGravity::damping_iter(.., 3)
    for (int i = 1; i < W; i++) {                                               // VS:719-730
      const double *xp = states + (size_t)VBA_STATE_LEN * (i - 1);
      st = vba_imu_preintegrate((int)it[i].size(), it[i].data(), ig[i].data(), ia[i].data(), xp + 16, xp + 19, nm6, nw6, scale_gravity,
                                imus + (size_t)VBA_IMU_PRE_LEN * (i - 1));
      if (st) return st;
    }
    bool stop = false;
    if (std::fabs(resis[0] - resis[1]) / resis[0] < converge_thre && iterCnt >= 2) {   // VS:733-758
      TimedSpan sp{};
      span_begin(c, "init", sp);
      const int nb = std::min(INIT_NNT_WG, (nf + 255) / 256);
      hipLaunchKernelGGL(k_init_nnt_part, dim3(nb), dim3(256), 0, c->stream, c->fv, nf, d_part);
      hipLaunchKernelGGL(k_init_nnt_fin, dim3(1), dim3(64), 0, c->stream, nb, d_part, d_nnt);
      span_end(c, "init", sp);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(last_nnt, d_nnt, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (int k = 0; k < 3; k++) eig[k] = last_nnt[k];
      is_degrade = eig[0] < 15;
      converge_thre = 0.01;
      if (converge_flag == 0) { init_align_gravity(W, states); converge_flag = 1; }
      else stop = true;
    }
    if (log) { log[1] = resis[0]; log[2] = resis[1]; log[3] = vbh::norm3(states + 22); log[4] = converge_flag; }
    if (stop) break;
  }
  const double gnm = vbh::norm3(states + (size_t)VBA_STATE_LEN * (W - 1) + 22);  // x_curr = x_buf[win_size - 1] (VS:761-762)
  if (is_degrade || gnm < 9.6 || gnm > 10.0) converge_flag = 0;
  if (converge_flag == 0) { st = map_reset(c->map, c->stream, c->err); if (st) return st; }   // VS:771-786
  if (pnt_out && n_out > 0) {
    HIPCHK(c, hipMemcpyAsync(pnt_out, d_pb, b_pb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(var_out, d_var, b_var, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *converged = converge_flag;
  for (int k = 0; k < 3; k++) eigvalue3[k] = eig[k];
  *iterations = rounds;
  *thresholds_left_relaxed = relaxed ? 1 : 0;
  return VBA_OK;
}

// A failing device step leaves no half-built window behind: the map is torn down and the factor store emptied (states / imus
// are undefined then, as the header says).
static int motion_init_cleanup(vba_ctx *c, int st, bool started) {
  if (st != VBA_OK && started) {
    const std::string why = c->err;
    map_reset(c->map, c->stream, c->err);
    c->nvox = 0;
    c->err = why;
  }
  return st;
}

int vba_motion_init(vba_ctx *c, int W, const int *pt_offsets, const double *pnt, const double *curv, const int *imu_offsets, const double *imu,
                    const double *beg_times, const double *ext_pose, double dept_err, double beam_err, double scale_gravity, int point_notime,
                    const double *nm6, const double *nw6, double *states, const double *covs, double *imus, double *hess, int *converged,
                    double *eigvalue3, int *iterations, int *thresholds_left_relaxed, double *round_log, int max_rounds, double *pnt_out,
                    double *var_out, int *pvec_offsets, int pvec_cap) {
  int st = motion_init_check(c, W, pt_offsets, pnt, curv, imu_offsets, imu, beg_times, ext_pose, nm6, nw6, states, covs, imus, converged, eigvalue3,
                             iterations, thresholds_left_relaxed, round_log, max_rounds, pnt_out, var_out, pvec_offsets);
  if (st) return st;
  std::vector<InitWalk> walk(W);
  for (int i = 0; i < W; i++) {
    InitWalk &K = walk[i];
    K.j_min = 0; K.pad = 0; K.cv0 = 0.0;
    if (!init_scan_walks(i, pt_offsets, imu_offsets, point_notime)) continue;
    const double *cv = curv + pt_offsets[i];
    const double t_last = imu[7 * (size_t)imu_offsets[i]] - beg_times[i];           // oldest pose: head = the deque's first sample
    int j = pt_offsets[i + 1] - pt_offsets[i];
    while (j > 0 && cv[j - 1] > t_last) j--;                                        // the walk stops at the first point at or before it
    K.j_min = j; K.cv0 = cv[0];
  }
  bool started = false;
  st = motion_init_impl(c, W, pt_offsets, pnt, curv, nullptr, nullptr, walk.data(), imu_offsets, imu, beg_times, ext_pose, dept_err, beam_err, scale_gravity,
                        point_notime, nm6, nw6, states, covs, imus, hess, converged, eigvalue3, iterations, thresholds_left_relaxed, round_log, max_rounds,
                        pnt_out, var_out, pvec_offsets, pvec_cap, started);
  return motion_init_cleanup(c, st, started);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ initialisation window
// pl_origs of initialization() (VS:1499-1516) in HBM: the scans' rows one after the other in the form k_init_blur reads.
struct vba_init_window {
  vba_ctx *ctx = nullptr;
  DevMem<double> d_pnt, d_curv; size_t cap = 0;             // [cap][3], [cap]: PCL floats carried in doubles
  InitWindowIndex idx;                                      // rows before every scan, and their total (host)
  // one push of up to pcap points: the down-sampler's work area (deterministic layout, the larger one) and its distances
  DevMem<char> d_ws; DevMem<double> d_dist; size_t pcap = 0;
  PinMem<int> h_n;                                          // pinned: the kept count
  // vba_motion_init_resident: kWalkRows InitWalkIn up, then kWalkRows InitWalk down (pinned image, device copy)
  DevMem<char> d_walk; PinMem<char> h_walk;
  int allocs = 0; int64_t bytes = 0;
};

namespace {

const int kWalkRows = 64;                                   // one wave of k_init_walk
const size_t kWalkBytes = kWalkRows * (sizeof(InitWalkIn) + sizeof(InitWalk));

// grow-only by doubling; the scans already in the window move with the block (device-to-device copy, one synchronise)
int iw_ensure_rows(vba_init_window *w, size_t need) {
  if (need <= w->cap) return VBA_OK;
  vba_ctx *c = w->ctx;
  const size_t m = init_window_grow(w->cap, 65536, need, (size_t)INT_MAX);      // vba_motion_init's body indexes rows with int
  if (!m) return VBA_ERR_CAPACITY;
  const size_t have = (size_t)w->idx.rows();
  HIPCHK(c, w->d_pnt.grow_keep(m * 3, have * 3, c->stream));
  HIPCHK(c, w->d_curv.grow_keep(m, have, c->stream));
  w->cap = m;
  w->allocs += 2; w->bytes += (int64_t)(m * 4 * sizeof(double));
  return VBA_OK;
}

// grow-only by doubling after a synchronise; nothing in it outlives a push
int iw_ensure_scratch(vba_init_window *w, size_t need) {
  if (need <= w->pcap) return VBA_OK;
  vba_ctx *c = w->ctx;
  const size_t m = init_window_grow(w->pcap, 65536, need, (size_t)1 << 28);
  if (!m) return VBA_ERR_CAPACITY;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int st = VBA_OK;
  const size_t ws = kf_ws_layout(c, (int)m, true, nullptr, nullptr, &st);
  if (st) return st;
  w->pcap = 0;
  HIPCHK(c, w->d_ws.ensure(ws));
  HIPCHK(c, w->d_dist.ensure(m));
  w->pcap = m;
  w->allocs += 2; w->bytes += (int64_t)(ws + m * sizeof(double));
  return VBA_OK;
}

}  // namespace

extern "C" {

int vba_init_window_create(vba_ctx *c, vba_init_window **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  vba_init_window *w = new vba_init_window();
  w->ctx = c;
  if (w->h_n.ensure(16) != hipSuccess || w->h_walk.ensure(kWalkBytes) != hipSuccess || w->d_walk.ensure(kWalkBytes) != hipSuccess) {
    c->set_error("vba_init_window_create: allocation failed");
    delete w;
    return VBA_ERR_HIP;
  }
  w->allocs = 3; w->bytes = (int64_t)kWalkBytes;
  *out = w;
  return VBA_OK;
}

void vba_init_window_destroy(vba_init_window *w) {
  if (!w) return;
  hipSetDevice(w->ctx->device);
  hipStreamSynchronize(w->ctx->stream);
  delete w;
}

int vba_init_window_reserve(vba_init_window *w, int max_scans, int max_points_per_scan) {
  if (!w || !init_window_reserve_args_ok(max_scans, max_points_per_scan)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = w->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st = iw_ensure_rows(w, (size_t)max_scans * (size_t)max_points_per_scan);
  if (st) return st;
  return iw_ensure_scratch(w, (size_t)max_points_per_scan);
}

int vba_init_window_allocations(vba_init_window *w, int *n_allocs, int64_t *bytes) {
  if (!w || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = w->allocs; *bytes = w->bytes;
  return VBA_OK;
}

int vba_init_window_clear(vba_init_window *w) {
  if (!w) return VBA_ERR_BAD_ARG;
  w->idx.clear();
  return VBA_OK;
}

int vba_init_window_size(vba_init_window *w, int *n_scans, int64_t *offsets) {
  if (!w || !n_scans) return VBA_ERR_BAD_ARG;
  *n_scans = w->idx.scans();
  w->idx.copy_to(offsets);
  return VBA_OK;
}

int vba_init_window_push(vba_init_window *w, vba_scan_frame *f, double down_size, int min_points, int *n_kept, int *retried) {
  if (!w || !f || !n_kept || !retried || !(down_size == down_size)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = w->ctx;
  ScanStage0 s0{};
  if (!scan_frame_stage0(f, nullptr, &s0) || s0.ctx->device != c->device) return VBA_ERR_BAD_ARG;
  *n_kept = 0; *retried = 0;
  const int n = s0.n;
  if (n == 0) { w->idx.append(0); return VBA_OK; }                  // the decode's documented deviation: an empty scan
  HIPCHK(c, hipSetDevice(c->device));
  const size_t row0 = (size_t)w->idx.rows();
  int st = iw_ensure_rows(w, row0 + (size_t)n);                     // every point may be kept
  if (st || (st = iw_ensure_scratch(w, (size_t)n))) return st;
  hipStream_t s = c->stream;
  if (!scan_frame_stage0(f, s, &s0)) { c->set_error("vba_init_window_push: cannot order the read behind the decode"); return VBA_ERR_HIP; }
  const bool det = c->opt.deterministic != 0;
  DsWork wk{};
  if (kf_ws_layout(c, n, det, w->d_ws, &wk, &st) > w->d_ws.n || st) return st ? st : VBA_ERR_CAPACITY;
  wk.dist = w->d_dist;
  const int nb = (n + 255) / 256;
  double *wp = w->d_pnt + 3 * row0, *wc = w->d_curv + row0;
  int kept = 0;
  // down_sampling_close(orig, vs) + the sort of VS:1510-1511, which the ascending-index compaction of a curvature-sorted cloud is
  auto pass = [&](double vs) -> int {
    if (vs < 0.001) {                                               // TL:242: the cloud as it is
      HIPCHK(c, hipMemcpyAsync(wp, s0.pnt, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
      HIPCHK(c, hipMemcpyAsync(wc, s0.curv, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
      HIPCHK(c, hipStreamSynchronize(s));
      kept = n;
      return VBA_OK;
    }
    int e = ds_core(c, s, 2, n, s0.pnt, nullptr, 9, 4, vs, det, wk);
    if (e) return e;
    TimedSpan sp{};
    span_begin(c, "init", sp);
    hipLaunchKernelGGL(k_initw_count, dim3(nb), dim3(256), 0, s, n, (const DsSlot *)wk.tab, (const int *)wk.slot, wk.blk);
    hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(256), 0, s, nb, wk.blk, wk.n_out);
    hipLaunchKernelGGL(k_initw_gather, dim3(nb), dim3(256), 0, s, n, (const DsSlot *)wk.tab, (const int *)wk.slot, (const int *)wk.blk, s0.pnt, s0.curv, w->d_pnt.p,
                       w->d_curv.p, (long long)row0);
    span_end(c, "init", sp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(w->h_n, wk.n_out, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    kept = w->h_n[0];
    return VBA_OK;
  };
  if ((st = pass(down_size))) return st;
  if (min_points > 0 && kept < min_points) {                        // VS:1503-1507: from the full cloud, kept whatever its count
    if ((st = pass(down_size / 2))) return st;
    *retried = 1;
  }
  if (kept < 1 || kept > n) { c->set_error("vba_init_window_push: kept count out of range"); return VBA_ERR_HIP; }
  w->idx.append(kept);
  *n_kept = kept;
  return VBA_OK;
}

int vba_init_window_push_points(vba_init_window *w, int n, const double *pnt, const double *curv) {
  if (!w || !init_window_points_args_ok(n, pnt, curv)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = w->ctx;
  if (n == 0) { w->idx.append(0); return VBA_OK; }
  HIPCHK(c, hipSetDevice(c->device));
  if (!is_device_ptr(curv) && !init_window_ascends(n, curv)) return VBA_ERR_BAD_ARG;   // device arrays: the caller answers for the order
  const size_t row0 = (size_t)w->idx.rows();
  int st = iw_ensure_rows(w, row0 + (size_t)n);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(w->d_pnt + 3 * row0, pnt, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(w->d_curv + row0, curv, (size_t)n * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  w->idx.append(n);
  return VBA_OK;
}

int vba_init_window_read(vba_init_window *w, int scan, double *pnt, double *curv) {
  int64_t first = 0, rows = 0;
  if (!w || !w->idx.range(scan, &first, &rows)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = w->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t a = (size_t)first, n = (size_t)rows;
  if (n > 0) {
    if (pnt) HIPCHK(c, hipMemcpyAsync(pnt, w->d_pnt + 3 * a, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (curv) HIPCHK(c, hipMemcpyAsync(curv, w->d_curv + a, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

// vba_motion_init on the window's clouds in place: the walk's inputs come from k_init_walk (one W-row download, one synchronise),
// everything after that is motion_init_impl.
int vba_motion_init_resident(vba_ctx *c, int W, vba_init_window *w, const int *imu_offsets, const double *imu, const double *beg_times,
                             const double *ext_pose, double dept_err, double beam_err, double scale_gravity, int point_notime, const double *nm6,
                             const double *nw6, double *states, const double *covs, double *imus, double *hess, int *converged, double *eigvalue3,
                             int *iterations, int *thresholds_left_relaxed, double *round_log, int max_rounds, double *pnt_out, double *var_out,
                             int *pvec_offsets, int pvec_cap) {
  std::vector<int> pto;
  if (!c || !w || w->ctx->device != c->device || W < 2 || W > kWalkRows || !w->idx.as_int(W, &pto)) return VBA_ERR_BAD_ARG;
  int st = motion_init_check(c, W, pto.data(), w->d_pnt, w->d_curv, imu_offsets, imu, beg_times, ext_pose, nm6, nw6, states, covs, imus, converged,
                             eigvalue3, iterations, thresholds_left_relaxed, round_log, max_rounds, pnt_out, var_out, pvec_offsets);
  if (st) return st;
  std::vector<InitWalk> walk(W);
  InitWalkIn *in = (InitWalkIn *)w->h_walk.p;
  InitWalk *res = (InitWalk *)(w->h_walk.p + kWalkRows * sizeof(InitWalkIn));
  bool any = false;
  for (int i = 0; i < W; i++) {
    const bool walks = init_scan_walks(i, pto.data(), imu_offsets, point_notime);
    in[i].off = w->idx.off[i]; in[i].n = walks ? pto[i + 1] - pto[i] : 0; in[i].pad = 0;
    in[i].t_last = walks ? imu[7 * (size_t)imu_offsets[i]] - beg_times[i] : 0.0;
    walk[i].j_min = 0; walk[i].pad = 0; walk[i].cv0 = 0.0;
    any = any || walks;
  }
  if (any) {
    HIPCHK(c, hipSetDevice(c->device));
    InitWalkIn *d_in = (InitWalkIn *)w->d_walk.p;
    InitWalk *d_res = (InitWalk *)(w->d_walk.p + kWalkRows * sizeof(InitWalkIn));
    HIPCHK(c, hipMemcpyAsync(d_in, in, (size_t)W * sizeof(InitWalkIn), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_init_walk, dim3(1), dim3(64), 0, c->stream, W, (const InitWalkIn *)d_in, (const double *)w->d_curv, d_res);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(res, d_res, (size_t)W * sizeof(InitWalk), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < W; i++) walk[i] = res[i];
  }
  bool started = false;
  st = motion_init_impl(c, W, pto.data(), nullptr, nullptr, w->d_pnt, w->d_curv, walk.data(), imu_offsets, imu, beg_times, ext_pose, dept_err, beam_err,
                        scale_gravity, point_notime, nm6, nw6, states, covs, imus, hess, converged, eigvalue3, iterations, thresholds_left_relaxed, round_log,
                        max_rounds, pnt_out, var_out, pvec_offsets, pvec_cap, started);
  return motion_init_cleanup(c, st, started);
}

}  // extern "C"
