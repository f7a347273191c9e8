// libvoxelba.so: LiDAR-inertial initialisation (vba_init_imu_poses, vba_init_align_gravity, vba_motion_init).  The kernels of
// vba_kernels_init.hpp, compiled here and nowhere else; the map is reached through map_* (vba_ctx.hpp), the LI-BA and the IMU
// pre-integration of the BA core (voxelba.hip) through the C ABI.
#include "vba_ctx.hpp"
#include "vba_kernels_init.hpp"
#include "vba_hostmath.hpp"

#include <algorithm>
#include <cmath>
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

static int motion_init_impl(vba_ctx *c, int W, const int *pt_offsets, const double *pnt, const double *curv, const int *imu_offsets, const double *imu,
                    const double *beg_times, const double *ext_pose, double dept_err, double beam_err, double scale_gravity, int point_notime,
                    const double *nm6, const double *nw6, double *states, const double *covs, double *imus, double *hess, int *converged,
                    double *eigvalue3, int *iterations, int *thresholds_left_relaxed, double *round_log, int max_rounds, double *pnt_out,
                    double *var_out, int *pvec_offsets, int pvec_cap, bool &started) {
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
      const double *cv = curv + S.pt_off;
      const double t_last = im[0] - beg_times[i];                                 // oldest pose: head = the deque's first sample
      int j = S.n_pts;
      while (j > 0 && cv[j - 1] > t_last) j--;                                      // the walk stops at the first point at or before it
      S.j_min = j;
      int dups = 0;
      if (j == 0) {
        int k = 0;                                                                  // pose that pushes point 0: first with t < curvature
        while (k < S.n_pose && !((im[7 * (size_t)(m - 2 - k)] - beg_times[i]) < cv[0])) k++;
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
  // device buffer: raw cloud + curvatures (uploaded once), blurred rows + their var, pose tables, scan table, Σ n nᵀ partials and result
  const size_t b_pnt = (size_t)np * 24, b_cv = (size_t)np * 8, b_pb = (size_t)n_out * 24, b_var = (size_t)n_out * 72,
               b_pose = (size_t)n_pose * INIT_POSE_LEN * 8, b_sc = (size_t)W * sizeof(InitScan), b_nnt = (size_t)(INIT_NNT_WG * 6 + 16) * 8;
  const size_t need = b_pnt + b_cv + b_pb + b_var + b_pose + b_sc + b_nnt + 64;
  HIPCHK(c, c->d_init.ensure(need));
  char *base = c->d_init;
  double *d_pnt = (double *)base, *d_cv = (double *)(base + b_pnt), *d_pb = (double *)(base + b_pnt + b_cv), *d_var = (double *)(base + b_pnt + b_cv + b_pb),
         *d_pose = (double *)(base + b_pnt + b_cv + b_pb + b_var);
  InitScan *d_sc = (InitScan *)(base + b_pnt + b_cv + b_pb + b_var + b_pose);
  double *d_part = (double *)(base + b_pnt + b_cv + b_pb + b_var + b_pose + b_sc), *d_nnt = d_part + INIT_NNT_WG * 6;
  if (np > 0) {
    HIPCHK(c, hipMemcpyAsync(d_pnt, pnt, b_pnt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_cv, curv, b_cv, hipMemcpyHostToDevice, c->stream));
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
int vba_motion_init(vba_ctx *c, int W, const int *pt_offsets, const double *pnt, const double *curv, const int *imu_offsets, const double *imu,
                    const double *beg_times, const double *ext_pose, double dept_err, double beam_err, double scale_gravity, int point_notime,
                    const double *nm6, const double *nw6, double *states, const double *covs, double *imus, double *hess, int *converged,
                    double *eigvalue3, int *iterations, int *thresholds_left_relaxed, double *round_log, int max_rounds, double *pnt_out,
                    double *var_out, int *pvec_offsets, int pvec_cap) {
  bool started = false;
  const int st = motion_init_impl(c, W, pt_offsets, pnt, curv, imu_offsets, imu, beg_times, ext_pose, dept_err, beam_err, scale_gravity, point_notime,
                                  nm6, nw6, states, covs, imus, hess, converged, eigvalue3, iterations, thresholds_left_relaxed, round_log, max_rounds,
                                  pnt_out, var_out, pvec_offsets, pvec_cap, started);
  if (st != VBA_OK && started) {
    const std::string why = c->err;
    map_reset(c->map, c->stream, c->err);
    c->nvox = 0;
    c->err = why;
  }
  return st;
}

}  // extern "C"
