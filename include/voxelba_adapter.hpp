// voxelba_adapter.hpp — header-only C++ adapter that gives libvoxelba.so (include/voxelba.h) the class/method
// surface of the reference so that it drops in behind the ROS odometry node:
//
//   reference (VoxelSLAM/src/voxel_map.hpp)                         adapter
//   -------------------------------------------------------------   -----------------------------------------
//   class LidarFactor            VM:124-339                         vba::LidarFactor
//   class Lidar_BA_Optimizer     VM:342-498  (damping_iter :422)    vba::Lidar_BA_Optimizer
//   class LI_BA_Optimizer        VM:504-714  (damping_iter :624)    vba::LI_BA_Optimizer
//   class LI_BA_OptimizerGravity VM:717-976  (damping_iter :878)    vba::LI_BA_OptimizerGravity
//   cut_voxel / cut_voxel_multi / cut_voxel(fix)  VM:1896/1964/2108 vba::VoxelMap::cut_voxel[_multi|_fix]
//   multi_recut / multi_margi    VS:1682 / VS:1590                  vba::VoxelMap::multi_recut / multi_margi
//   OctoTree::tras_display       VM:1765-1827                       vba::VoxelMap::tras_display / display, vba::pub_voxelmap
//   Initialization::motion_init  VS:617-819                         vba::Initialization::motion_init
//   initialization(), pl_origs   VS:1499-1516                       vba::InitWindow::push + the InitWindow overload of motion_init
//   build_graph + gtsam::ISAM2   VS:2078-2156, VS:2550-2561          vba::PoseGraph (add_edge LR:147-161, set_state LR:36-43)
//   ResultOutput::pub_globalmap  VS:110-154                         vba::pub_globalmap
//   pcl_handler VH:77-103; motion_blur's loop + VS:1877-1888        vba::ScanFrame::decode / prepare (ScanView feeds the odometry and the map)
//   class IMUEKF (IMU_init, process, motion_blur) EK:8-216          vba::ImuEkf, on the host or on a vba::OdomState resident in HBM
//
// The reference's types are Eigen-based (tools.hpp:4).  This header compiles without Eigen (plain-array structs that
// mirror PointCluster / IMUST / IMU_PRE field for field); when <Eigen/Core> is available the Eigen-typed overloads
// below are enabled so call sites such as voxelslam.cpp:1969-1970 compile unchanged after `using namespace vba;`.
#pragma once
#include "voxelba.h"
#include <cstring>
#include <deque>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#if defined(__has_include)
#if __has_include(<Eigen/Core>)
#include <Eigen/Core>
#define VBA_ADAPTER_HAVE_EIGEN 1
#endif
#endif

namespace vba {

struct PointCluster {  // tools.hpp:304-365 (P symmetric 3x3 row-major, v, N)
  double P[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double v[3] = {0, 0, 0};
  int N = 0;
  void pack(double *c) const { c[0] = P[0]; c[1] = P[3]; c[2] = P[6]; c[3] = P[4]; c[4] = P[7]; c[5] = P[8]; c[6] = v[0]; c[7] = v[1]; c[8] = v[2]; c[9] = N; }
  void unpack(const double *c) {
    P[0] = c[0]; P[1] = P[3] = c[1]; P[2] = P[6] = c[2]; P[4] = c[3]; P[5] = P[7] = c[4]; P[8] = c[5];
    v[0] = c[6]; v[1] = c[7]; v[2] = c[8]; N = (int)c[9];
  }
};

struct IMUST {  // tools.hpp:135-199: exactly the `state` layout of voxelba.h followed by cov
  double t = 0, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0}, v[3] = {0, 0, 0}, bg[3] = {0, 0, 0}, ba[3] = {0, 0, 0}, g[3] = {0, 0, 0};
  double cov[225] = {0};
};

struct IMU_PRE {  // preintegration.hpp:11-331: exactly the `imu_pre` layout of voxelba.h
  double f[VBA_IMU_PRE_LEN];
  double bg0[3] = {0, 0, 0}, ba0[3] = {0, 0, 0};
  IMU_PRE(const double *bg1 = nullptr, const double *ba1 = nullptr) {   // IMU_PRE(bg, ba) PI:32-48
    std::memset(f, 0, sizeof(f));
    f[0] = f[4] = f[8] = 1.0;
    if (bg1) { std::memcpy(f + 15, bg1, 24); std::memcpy(bg0, bg1, 24); }
    if (ba1) { std::memcpy(f + 18, ba1, 24); std::memcpy(ba0, ba1, 24); }
  }
  // push_imu(deque<sensor_msgs::Imu::Ptr>&) PI:50-73 with the samples as arrays t[n], gyr[n][3], acc[n][3] and the noise globals
  // noiseMeas / noiseWalk (PI:8) as diagonals
  void push_imu(int n, const double *t, const double *gyr, const double *acc, const double *noise_meas6, const double *noise_walk6,
                double scale_gravity = 1.0) {
    const int st = vba_imu_preintegrate(n, t, gyr, acc, bg0, ba0, noise_meas6, noise_walk6, scale_gravity, f);
    if (st != VBA_OK) throw std::runtime_error(std::string("libvoxelba: push_imu: ") + vba_status_string(st));
  }
};

inline void check(vba_ctx *c, int st) {
  if (st != VBA_OK) throw std::runtime_error(std::string("libvoxelba: ") + vba_status_string(st) + " | " + (c ? vba_last_error(c) : ""));
}

// One context = one HIP stream + HBM factor store + device voxel map.  The reference's globals (VM:98-104, VM:500) are
// the fields of vba_options.
class Context {
 public:
  explicit Context(const vba_options &o) { check(nullptr, vba_create(&o, &c_)); }
  ~Context() { vba_destroy(c_); }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  vba_ctx *get() const { return c_; }
 private:
  vba_ctx *c_ = nullptr;
};

// class LidarFactor (VM:124-339).  The voxel data lives in HBM; eig_values / eig_vectors / pcr_adds are fetched on demand.
class LidarFactor {
 public:
  int win_size;
  LidarFactor(Context &ctx, int w) : win_size(w), c_(ctx.get()) {}
  void push_voxel(const std::vector<PointCluster> &vec_orig, const PointCluster &fix, double coe, const double *eig_value3,
                  const double *eig_vector9, const PointCluster &pcr_add) {   // VM:139-147
    std::vector<double> cl((size_t)win_size * 10);
    for (int i = 0; i < win_size; i++) vec_orig[i].pack(&cl[(size_t)i * 10]);
    double fx[10], pa[10];
    fix.pack(fx); pcr_add.pack(pa);
    check(c_, vba_factor_push_voxels(c_, 1, cl.data(), fx, &coe, eig_value3, eig_vector9, pa));
  }
  size_t size() const { return (size_t)vba_factor_size(c_); }   // plvec_voxels.size()
  void acc_evaluate2(const std::vector<IMUST> &xs, int head, int end, double *Hess, double *JacT, double &residual) {   // VM:150-282
    std::vector<double> poses = poses_of(xs);
    check(c_, vba_factor_acc_evaluate2(c_, poses.data(), head, end, Hess, JacT, &residual));
  }
  void evaluate_only_residual(const std::vector<IMUST> &xs, int head, int end, double &residual) {   // VM:285-325
    std::vector<double> poses = poses_of(xs);
    check(c_, vba_factor_evaluate_only_residual(c_, poses.data(), head, end, &residual));
  }
  void read_back(std::vector<double> &eig_values, std::vector<double> &eig_vectors, std::vector<PointCluster> &pcr_adds) {
    const size_t n = size();
    eig_values.resize(n * 3); eig_vectors.resize(n * 9);
    std::vector<double> pa(n * 10);
    check(c_, vba_factor_read_back(c_, eig_values.data(), eig_vectors.data(), pa.data()));
    pcr_adds.resize(n);
    for (size_t a = 0; a < n; a++) pcr_adds[a].unpack(&pa[a * 10]);
  }
  void clear() { check(c_, vba_factor_clear(c_)); }   // VM:328-336
  vba_ctx *ctx() const { return c_; }
  static std::vector<double> poses_of(const std::vector<IMUST> &xs) {
    std::vector<double> p(xs.size() * 12);
    for (size_t i = 0; i < xs.size(); i++) { std::memcpy(&p[i * 12], xs[i].R, 72); std::memcpy(&p[i * 12 + 9], xs[i].p, 24); }
    return p;
  }
 private:
  vba_ctx *c_;
};

// class Lidar_BA_Optimizer (VM:342-498)
class Lidar_BA_Optimizer {
 public:
  int win_size = 0, jac_leng = 0, thd_num = 2;
  // bool damping_iter(vector<IMUST>&, LidarFactor&, MatrixXd *hess, vector<double> &resis, int max_iter = 3, bool is_display = false)  VM:422
  bool damping_iter(std::vector<IMUST> &x_stats, LidarFactor &voxhess, std::vector<double> *hess, std::vector<double> &resis, int max_iter = 3,
                    bool /*is_display*/ = false) {
    win_size = voxhess.win_size; jac_leng = 6 * win_size;
    std::vector<double> poses = LidarFactor::poses_of(x_stats);
    if (hess) hess->assign((size_t)jac_leng * jac_leng, 0.0);
    double r2[2] = {0, 0};
    int conv = 0;
    check(voxhess.ctx(), vba_lidar_ba_damping_iter(voxhess.ctx(), poses.data(), hess ? hess->data() : nullptr, r2, max_iter, thd_num, &conv));
    for (size_t i = 0; i < x_stats.size(); i++) { std::memcpy(x_stats[i].R, &poses[i * 12], 72); std::memcpy(x_stats[i].p, &poses[i * 12 + 9], 24); }
    resis.push_back(r2[0]); resis.push_back(r2[1]);
    return conv != 0;
  }
};

namespace detail {
inline void li_call(std::vector<IMUST> &x_stats, LidarFactor &voxhess, std::deque<IMU_PRE *> &imus_factor, std::vector<double> *resis,
                    std::vector<double> *hess, int gravity, int max_iter) {
  const int W = voxhess.win_size, n = 15 * W + (gravity ? 3 : 0);
  std::vector<double> st((size_t)W * 25), im((size_t)(W - 1) * VBA_IMU_PRE_LEN);
  for (int i = 0; i < W; i++) std::memcpy(&st[(size_t)i * 25], &x_stats[i].t, 25 * sizeof(double));
  for (int i = 0; i < W - 1; i++) std::memcpy(&im[(size_t)i * VBA_IMU_PRE_LEN], imus_factor[i]->f, sizeof(imus_factor[i]->f));
  if (hess) hess->assign((size_t)n * n, 0.0);
  double r2[2] = {0, 0};
  check(voxhess.ctx(), vba_li_ba_damping_iter(voxhess.ctx(), st.data(), im.data(), gravity, max_iter, hess ? hess->data() : nullptr, r2));
  for (int i = 0; i < W; i++) std::memcpy(&x_stats[i].t, &st[(size_t)i * 25], 25 * sizeof(double));
  for (int i = 0; i < W - 1; i++) std::memcpy(imus_factor[i]->f, &im[(size_t)i * VBA_IMU_PRE_LEN], sizeof(imus_factor[i]->f));
  if (gravity && resis) { resis->push_back(r2[0]); resis->push_back(r2[1]); }
}
}  // namespace detail

// class LI_BA_Optimizer (VM:504-714): void damping_iter(x_stats, voxhess, imus_factor, MatrixXd *hess)  VM:624
class LI_BA_Optimizer {
 public:
  void damping_iter(std::vector<IMUST> &x_stats, LidarFactor &voxhess, std::deque<IMU_PRE *> &imus_factor, std::vector<double> *hess) {
    detail::li_call(x_stats, voxhess, imus_factor, nullptr, hess, 0, 3);
  }
};
// class LI_BA_OptimizerGravity (VM:717-976): void damping_iter(x_stats, voxhess, imus_factor, resis, hess, max_iter = 2)  VM:878
class LI_BA_OptimizerGravity {
 public:
  void damping_iter(std::vector<IMUST> &x_stats, LidarFactor &voxhess, std::deque<IMU_PRE *> &imus_factor, std::vector<double> &resis,
                    std::vector<double> *hess, int max_iter = 2) {
    detail::li_call(x_stats, voxhess, imus_factor, &resis, hess, 1, max_iter);
  }
};

// Voxel map: unordered_map<VOXEL_LOC, OctoTree*> surf_map / surf_map_slide + the free functions that operate on them.
struct pointVar { double pnt[3]; double var[9]; };   // VM:18-34
typedef std::vector<pointVar> PVec;

// ---- scan front end: pcl_handler VH:77-103, then odom_ekf.process's point loop + VS:1877-1888, resident in HBM
struct ScanView { int n = 0; const double *pnt = nullptr; const double *var = nullptr; };   // DEVICE arrays [n][3], [n][9] owned by a ScanFrame
class ScanFrame {
 public:
  explicit ScanFrame(Context &ctx) : ctx_(ctx.get()) { check(ctx_, vba_scan_frame_create(ctx_, &f_)); }
  ~ScanFrame() { vba_scan_frame_destroy(f_); }
  ScanFrame(const ScanFrame &) = delete;
  ScanFrame &operator=(const ScanFrame &) = delete;
  void reserve(int max_raw_points, int max_point_step) { check(ctx_, vba_scan_frame_reserve(f_, max_raw_points, max_point_step)); }
  // feat.process(msg, *pl_ptr) + the rest of pcl_handler: data = &msg->data[0] (PointCloud2) or &msg->points[0] (livox CustomMsg).
  // Returns pl_ptr->back().curvature, the end-time offset that sync_packages adds to the message stamp (VH:129); size() = pl_ptr->size()
  double decode(const void *data, int n_raw, const vba_scan_layout &layout, int point_filter_num, double blind) {
    double last = 0;
    check(ctx_, vba_scan_decode(f_, &layout, data, n_raw, point_filter_num, blind * blind, &n_, &last));
    return last;
  }
  int size() const { return n_; }
  // imu_poses [m][22], end = xc after the propagation (EK:121-123), ext = extrin_para; min_points 500 (VS:1880), 0 while initialising
  ScanView prepare(Context &ctx, int m, const double *imu_poses, const IMUST &end, const IMUST &ext, bool point_notime, double down_size,
                   double dept_err, double beam_err, int min_points = 500) {
    double e[12], x[12];
    std::memcpy(e, end.R, 72); std::memcpy(e + 9, end.p, 24); std::memcpy(x, ext.R, 72); std::memcpy(x + 9, ext.p, 24);
    ScanView v;
    check(ctx.get(), vba_scan_prepare(ctx.get(), f_, m, imu_poses, e, x, point_notime ? 1 : 0, down_size, min_points, dept_err, beam_err, &v.n, &v.pnt, &v.var));
    return v;
  }
  vba_scan_frame *get() const { return f_; }
 private:
  vba_ctx *ctx_;
  vba_scan_frame *f_ = nullptr;
  int n_ = 0;
};

class LoopMap;
class ScanLog;
struct ScanPose;
class VoxelMap {
 public:
  explicit VoxelMap(Context &ctx) : c_(ctx.get()) {}
  // cut_voxel(feat_map, pvec, win_count, feat_tem_map, wdsize, pwld, sws) VM:1896 — pwld = R p + t is recomputed on the device from `x`
  void cut_voxel(const PVec &pvec, int win_count, const IMUST &x, bool with_var = true) { insert(pvec, win_count, x, with_var, 0); }
  // cut_voxel_multi(...) VM:1964
  void cut_voxel_multi(const PVec &pvec, int win_count, const IMUST &x, bool with_var = true) { insert(pvec, win_count, x, with_var, 1); }
  // pvec_update(pptr, x_curr, pwld) VH:242-265 + cut_voxel_multi VM:1964 fused on the device: pvec holds BODY-frame points and
  // covariances (as var_init leaves them), x.cov the state covariance whose rotation / translation blocks inflate them
  void pvec_update_cut_voxel_multi(const PVec &pvec, int win_count, const IMUST &x) {
    const size_t n = pvec.size();
    std::vector<double> p(n * 3), v(n * 9);
    for (size_t i = 0; i < n; i++) { std::memcpy(&p[i * 3], pvec[i].pnt, 24); std::memcpy(&v[i * 9], pvec[i].var, 72); }
    double pose[12];
    std::memcpy(pose, x.R, 72); std::memcpy(pose + 9, x.p, 24);
    check(c_, vba_map_pvec_update_cut_voxel(c_, win_count, (int)n, p.data(), v.data(), pose, x.cov, 1));
  }
  // the same on a prepared scan frame: the device arrays are consumed in place, on the context that prepared them
  void pvec_update_cut_voxel_multi(const ScanView &scan, int win_count, const IMUST &x) {
    double pose[12];
    std::memcpy(pose, x.R, 72); std::memcpy(pose + 9, x.p, 24);
    check(c_, vba_map_pvec_update_cut_voxel(c_, win_count, scan.n, scan.pnt, scan.var, pose, x.cov, 1));
  }
  // cut_voxel(feat_map, PVec&, wdsize, jour) VM:2108
  void cut_voxel_fix(const PVec &pvec, double jour) {
    std::vector<double> p(pvec.size() * 3);
    for (size_t i = 0; i < pvec.size(); i++) std::memcpy(&p[i * 3], pvec[i].pnt, 24);
    check(c_, vba_map_cut_voxel_fix(c_, (int)pvec.size(), p.data(), jour));
  }
  // multi_recut(feat_map, win_count, xs, voxopt, sws) VS:1682 (fills the context's LidarFactor store)
  void multi_recut(int win_count, const std::vector<IMUST> &xs, bool multi = true) {
    std::vector<double> poses = LidarFactor::poses_of(xs);
    check(c_, vba_map_recut(c_, win_count, poses.data(), multi ? 1 : 0));
  }
  // multi_margi(feat_map, jour, win_count, xs, voxopt, sw) VS:1590
  void multi_margi(double jour, int win_count, const std::vector<IMUST> &xs) {
    std::vector<double> poses = LidarFactor::poses_of(xs);
    check(c_, vba_map_margi(c_, win_count, poses.data(), jour));
  }
  void slide(int mgsize) { check(c_, vba_map_slide(c_, mgsize)); }   // VS:2014-2019
  void reset() { check(c_, vba_map_reset(c_)); }
  // loop_update() VS:1255-1373 (defined below, after LoopMap): returns the factor count of the closing recut
  inline int loop_update(LoopMap &map_loop, const IMUST &dx, std::vector<ScanPose *> &buf_lba2loop, std::vector<IMUST> &x_buf, int win_count,
                         IMUST &x_curr, int &g_update, const std::vector<const PVec *> *pvec_buf = nullptr);
  // the same with the buf_lba2loop scans in a ScanLog (scans first .. first + bl_states.size() - 1; bl_states are their ScanPose::x,
  // moved by dx here) and the window from the outgoing map's scan ring: no point crosses the host boundary
  inline int loop_update(LoopMap &map_loop, const IMUST &dx, ScanLog &log, int64_t first, std::vector<IMUST> &bl_states, std::vector<IMUST> &x_buf,
                         int win_count, IMUST &x_curr, int &g_update);
  // The view of the live map (vba_map_display): what tras_display collects, with the planes it walks as records
  struct Display {
    std::vector<float> xyzi;                 // [n][4] x y z intensity (= the frame's index in the window)
    std::vector<int> plane_of_point;         // [n] index into planes, -1: the point's leaf is no plane (flags & 1 only)
    std::vector<int64_t> frame_begin;        // [win_count + 1]
    std::vector<float> planes;               // [m][16]
    std::vector<long long> plane_key;        // [m][5] kx ky kz layer path
    int64_t n_points() const { return (int64_t)(xyzi.size() / 4); }
    int64_t n_planes() const { return (int64_t)(planes.size() / 16); }
  };
  // the first win_count states of x_buf are the window's poses; flags & 1 keeps the points of non-planar leaves too
  Display display(int win_count, const std::vector<IMUST> &x_buf, int flags = 0) {
    if (win_count < 0 || (size_t)win_count > x_buf.size()) throw std::invalid_argument("VoxelMap::display: win_count");
    const std::vector<double> poses = LidarFactor::poses_of(std::vector<IMUST>(x_buf.begin(), x_buf.begin() + win_count));
    const double *ps = win_count > 0 ? poses.data() : nullptr;
    Display d;
    int64_t n = 0, m = 0;
    d.frame_begin.assign((size_t)win_count + 1, 0);
    check(c_, vba_map_display(c_, win_count, ps, flags, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &n, &m));     // the size query
    d.xyzi.resize((size_t)n * 4); d.plane_of_point.resize((size_t)n); d.planes.resize((size_t)m * 16); d.plane_key.resize((size_t)m * 5);
    if (n > 0 || m > 0)
      check(c_, vba_map_display(c_, win_count, ps, flags, n, n > 0 ? d.xyzi.data() : nullptr, n > 0 ? d.plane_of_point.data() : nullptr,
                                d.frame_begin.data(), m, m > 0 ? d.planes.data() : nullptr, m > 0 ? d.plane_key.data() : nullptr, &n, &m));
    return d;
  }
  // OctoTree::tras_display(win_count, pl_fixd, pl_wind, x_buf) over every root of surf_map (VM:1765-1827):
  // the window's points that sit in planar leaves are appended to pl_wind as x y z intensity.  pl_fixd is not produced: its loop is
  // commented out in the reference, which leaves it empty.
  void tras_display(int win_count, std::vector<float> &pl_wind, const std::vector<IMUST> &x_buf) {
    const Display d = display(win_count, x_buf, 0);
    pl_wind.insert(pl_wind.end(), d.xyzi.begin(), d.xyzi.end());
  }
  vba_ctx *get() const { return c_; }
  size_t size() const { return (size_t)vba_map_num_roots(c_); }
  size_t slide_size() const { return (size_t)vba_map_num_slide_roots(c_); }
 private:
  void insert(const PVec &pvec, int win_count, const IMUST &x, bool with_var, int multi) {
    const size_t n = pvec.size();
    std::vector<double> p(n * 3), v(with_var ? n * 9 : 0);
    for (size_t i = 0; i < n; i++) { std::memcpy(&p[i * 3], pvec[i].pnt, 24); if (with_var) std::memcpy(&v[i * 9], pvec[i].var, 72); }
    double pose[12];
    std::memcpy(pose, x.R, 72); std::memcpy(pose + 9, x.p, 24);
    check(c_, vba_map_cut_voxel(c_, win_count, (int)n, p.data(), with_var ? v.data() : nullptr, pose, multi));
  }
  vba_ctx *c_;
};

// ---- the initialisation window: pl_origs of initialization() (VS:1499-1516), resident in HBM
class InitWindow {
 public:
  explicit InitWindow(Context &ctx) : ctx_(ctx.get()) { check(ctx_, vba_init_window_create(ctx_, &w_)); }
  ~InitWindow() { vba_init_window_destroy(w_); }
  InitWindow(const InitWindow &) = delete;
  InitWindow &operator=(const InitWindow &) = delete;
  void reserve(int max_scans, int max_points_per_scan) { check(ctx_, vba_init_window_reserve(w_, max_scans, max_points_per_scan)); }
  // pl_down = orig; down_sampling_close(pl_down, down_size); the `< 1000` retry at down_size / 2; sort(curvature <);
  // pl_origs.push_back(pl_down)  (VS:1499-1512) on the frame's decoded cloud (`orig`, VS:1458).  Returns the points kept.
  int push(ScanFrame &orig, double down_size, int min_points = 1000, bool *retried = nullptr) {
    int n = 0, r = 0;
    check(ctx_, vba_init_window_push(w_, orig.get(), down_size, min_points, &n, &r));
    if (retried) *retried = r != 0;
    return n;
  }
  // a cloud the caller holds (host or device arrays [n][3], [n]; curvature ascending), appended as it is
  void push_points(int n, const double *pnt, const double *curv) { check(ctx_, vba_init_window_push_points(w_, n, pnt, curv)); }
  int size() const { int n = 0; vba_init_window_size(w_, &n, nullptr); return n; }                  // pl_origs.size()
  long long points() const {                                                                       // points of all scans
    std::vector<int64_t> off((size_t)size() + 1);
    int n = 0;
    vba_init_window_size(w_, &n, off.data());
    return (long long)off.back();
  }
  void clear() { check(ctx_, vba_init_window_clear(w_)); }                                          // pl_origs.clear() (VS:795)
  vba_init_window *get() const { return w_; }
 private:
  vba_ctx *ctx_;
  vba_init_window *w_ = nullptr;
};

// ---- LiDAR-inertial initialisation: class Initialization (voxelslam.cpp:460-820)
struct PointXYZC { float x, y, z, curvature; };   // the fields of a PointType (pcl::PointXYZINormal) that motion_init reads
struct ImuSample { double t, gyr[3], acc[3]; };   // one sensor_msgs::Imu of a deque: stamp, angular_velocity, linear_acceleration

class Initialization {
 public:
  // the reference's globals that motion_init reads: dept_err / beam_err (VH:179), imupre_scale_gravity / noiseMeas / noiseWalk (PI:8-9),
  // point_notime (VS:550)
  double dept_err = 0.02, beam_err = 0.05, scale_gravity = 1.0;
  double noise_meas[6] = {0, 0, 0, 0, 0, 0}, noise_walk[6] = {0, 0, 0, 0, 0, 0};
  int point_notime = 0;
  // filled by each call: eigvalue (VS:744), outer rounds run, and whether the reference would leave its relaxed thresholds in force
  double eigvalue[3] = {0, 0, 0};
  int iterations = 0, thresholds_left_relaxed = 0;

  // int motion_init(pl_origs, vec_imus, beg_times, hess, voxhess, x_buf, surf_map, surf_map_slide, pvec_buf, win_size, sws, x_curr,
  //                 imu_pre_buf, extrin_para)  VS:617.  surf_map stands for surf_map + surf_map_slide (one device map); sws has no
  // counterpart (the device map recycles its own nodes).  imu_pre_buf must hold win_size - 1 factors; they are rebuilt in place
  // (VS:719-730).  As in the reference, pl_origs / vec_imus / beg_times are cleared on return (VS:795-797).
  int motion_init(std::vector<std::vector<PointXYZC>> &pl_origs, std::vector<std::vector<ImuSample>> &vec_imus, std::vector<double> &beg_times,
                  std::vector<double> *hess, LidarFactor &voxhess, std::vector<IMUST> &x_buf, VoxelMap &surf_map,
                  std::vector<std::shared_ptr<PVec>> &pvec_buf, int win_size, IMUST &x_curr, std::deque<IMU_PRE *> &imu_pre_buf,
                  const IMUST &extrin_para) {
    const int W = win_size;
    if ((int)pl_origs.size() < W || (int)vec_imus.size() < W || (int)beg_times.size() < W || (int)x_buf.size() < W ||
        (int)imu_pre_buf.size() < W - 1)
      throw std::runtime_error("libvoxelba: motion_init: fewer than win_size scans / states / IMU factors");
    std::vector<int> pto(W + 1, 0);
    for (int i = 0; i < W; i++) pto[i + 1] = pto[i] + (int)pl_origs[i].size();
    std::vector<double> pnt((size_t)pto[W] * 3 + 3), curv((size_t)pto[W] + 1);
    for (int i = 0; i < W; i++)
      for (size_t k = 0; k < pl_origs[i].size(); k++) {
        const PointXYZC &a = pl_origs[i][k];
        const size_t r = (size_t)pto[i] + k;
        pnt[3 * r] = a.x; pnt[3 * r + 1] = a.y; pnt[3 * r + 2] = a.z; curv[r] = a.curvature;
      }
    const int converged = run(pto[W], vec_imus, beg_times, hess, voxhess, x_buf, pvec_buf, W, x_curr, imu_pre_buf, extrin_para, [&](const Call &a) {
      return vba_motion_init(voxhess.ctx(), W, pto.data(), pnt.data(), curv.data(), a.imo, a.imu, beg_times.data(), a.ext, dept_err, beam_err, scale_gravity,
                             point_notime, noise_meas, noise_walk, a.st, a.cov, a.im, a.hess, a.converged, eigvalue, &iterations, &thresholds_left_relaxed,
                             nullptr, 0, a.po, a.vo, a.pvo, a.cap);
    });
    (void)surf_map;   // the map (and voxhess) stay on the context, as surf_map / voxhess in the reference
    pl_origs.clear(); vec_imus.clear(); beg_times.clear();         // VS:795-797
    return converged;
  }

  // The same with pl_origs resident in HBM: the window the node filled with InitWindow::push, one scan at a time, in
  // place of VS:1499-1512.  The clouds are read where they are; the window is cleared on return, as the vectors are.
  int motion_init(InitWindow &pl_origs, std::vector<std::vector<ImuSample>> &vec_imus, std::vector<double> &beg_times, std::vector<double> *hess,
                  LidarFactor &voxhess, std::vector<IMUST> &x_buf, VoxelMap &surf_map, std::vector<std::shared_ptr<PVec>> &pvec_buf, int win_size,
                  IMUST &x_curr, std::deque<IMU_PRE *> &imu_pre_buf, const IMUST &extrin_para) {
    const int W = win_size;
    if (pl_origs.size() != W || (int)vec_imus.size() < W || (int)beg_times.size() < W || (int)x_buf.size() < W || (int)imu_pre_buf.size() < W - 1)
      throw std::runtime_error("libvoxelba: motion_init: the window does not hold win_size scans, or fewer than win_size states / IMU factors");
    const int converged = run((int)pl_origs.points(), vec_imus, beg_times, hess, voxhess, x_buf, pvec_buf, W, x_curr, imu_pre_buf, extrin_para, [&](const Call &a) {
      return vba_motion_init_resident(voxhess.ctx(), W, pl_origs.get(), a.imo, a.imu, beg_times.data(), a.ext, dept_err, beam_err, scale_gravity,
                                      point_notime, noise_meas, noise_walk, a.st, a.cov, a.im, a.hess, a.converged, eigvalue, &iterations,
                                      &thresholds_left_relaxed, nullptr, 0, a.po, a.vo, a.pvo, a.cap);
    });
    (void)surf_map;
    pl_origs.clear(); vec_imus.clear(); beg_times.clear();         // VS:795-797
    return converged;
  }

 private:
  // what both overloads hand to the library besides the clouds
  struct Call { const int *imo; const double *imu, *ext; double *st; const double *cov; double *im, *hess; int *converged; double *po, *vo; int *pvo, cap; };
  // packs the deques, states and factors, calls `call`, and unpacks states, factors and pvec_buf; n_pts = points of the whole window
  template <class F>
  int run(int n_pts, std::vector<std::vector<ImuSample>> &vec_imus, std::vector<double> &beg_times, std::vector<double> *hess, LidarFactor &voxhess,
          std::vector<IMUST> &x_buf, std::vector<std::shared_ptr<PVec>> &pvec_buf, int W, IMUST &x_curr, std::deque<IMU_PRE *> &imu_pre_buf,
          const IMUST &extrin_para, F &&call) {
    (void)beg_times;
    std::vector<int> imo(W + 1, 0);
    for (int i = 0; i < W; i++) imo[i + 1] = imo[i] + (int)vec_imus[i].size();
    std::vector<double> imu((size_t)imo[W] * 7 + 7);
    for (int i = 0; i < W; i++)
      for (size_t k = 0; k < vec_imus[i].size(); k++) std::memcpy(&imu[((size_t)imo[i] + k) * 7], &vec_imus[i][k], 7 * sizeof(double));
    std::vector<double> st((size_t)W * 25), cov((size_t)W * 225), im((size_t)(W - 1) * VBA_IMU_PRE_LEN);
    for (int i = 0; i < W; i++) { std::memcpy(&st[(size_t)i * 25], &x_buf[i].t, 25 * sizeof(double)); std::memcpy(&cov[(size_t)i * 225], x_buf[i].cov, 225 * sizeof(double)); }
    for (int i = 0; i < W - 1; i++) std::memcpy(&im[(size_t)i * VBA_IMU_PRE_LEN], imu_pre_buf[i]->f, sizeof(imu_pre_buf[i]->f));
    double ext[12];
    std::memcpy(ext, extrin_para.R, 72); std::memcpy(ext + 9, extrin_para.p, 24);
    const int nh = 15 * W + 3;
    if (hess) hess->assign((size_t)nh * nh, 0.0);
    const int cap = n_pts + imo[W];
    std::vector<double> po((size_t)cap * 3 + 3), vo((size_t)cap * 9 + 9);
    std::vector<int> pvo(W + 1);
    int converged = 0;
    const Call a{imo.data(), imu.data(), ext, st.data(), cov.data(), im.data(), hess ? hess->data() : nullptr, &converged, po.data(), vo.data(), pvo.data(), cap};
    check(voxhess.ctx(), call(a));
    for (int i = 0; i < W; i++) std::memcpy(&x_buf[i].t, &st[(size_t)i * 25], 25 * sizeof(double));
    for (int i = 1; i < W; i++) {                                  // IMU_PRE(x_buf[i-1].bg, x_buf[i-1].ba) + push_imu (VS:724-730)
      IMU_PRE *f = imu_pre_buf[i - 1];
      std::memcpy(f->f, &im[(size_t)(i - 1) * VBA_IMU_PRE_LEN], sizeof(f->f));
      std::memcpy(f->bg0, x_buf[i - 1].bg, 24); std::memcpy(f->ba0, x_buf[i - 1].ba, 24);
    }
    if ((int)pvec_buf.size() < W) pvec_buf.resize(W);
    for (int i = 0; i < W; i++) {
      if (!pvec_buf[i]) pvec_buf[i].reset(new PVec);
      PVec &pv = *pvec_buf[i];
      pv.resize((size_t)(pvo[i + 1] - pvo[i]));
      for (size_t k = 0; k < pv.size(); k++) {
        std::memcpy(pv[k].pnt, &po[((size_t)pvo[i] + k) * 3], 24);
        std::memcpy(pv[k].var, &vo[((size_t)pvo[i] + k) * 9], 72);
      }
    }
    x_curr = x_buf[W - 1];                                         // VS:761
    return converged;
  }
};

// ---- scan pre-processing and hierarchical global BA (free functions of the reference: tools.hpp / voxelslam.cpp)
struct XYZ { float x, y, z; };   // the coordinates of a pcl::PointXYZINormal

// down_sampling_voxel(pl_feat, voxel_size) TL:201-238: pl is replaced by the centroids; counts[i] = the `curvature` field
// after the call, first[i] = index (in the input) of the point whose other fields the reference keeps.
inline void down_sampling_voxel(Context &ctx, std::vector<XYZ> &pl, double voxel_size, std::vector<int> *counts = nullptr,
                                std::vector<int> *first = nullptr) {
  const int n = (int)pl.size();
  std::vector<double> in((size_t)n * 3), out((size_t)n * 3);
  std::vector<int> cnt(n), fst(n);
  for (int i = 0; i < n; i++) { in[3 * i] = pl[i].x; in[3 * i + 1] = pl[i].y; in[3 * i + 2] = pl[i].z; }
  int m = 0;
  check(ctx.get(), vba_scan_down_sampling_voxel(ctx.get(), n, in.data(), voxel_size, out.data(), cnt.data(), fst.data(), &m));
  pl.resize(m);
  for (int i = 0; i < m; i++) { pl[i].x = (float)out[3 * i]; pl[i].y = (float)out[3 * i + 1]; pl[i].z = (float)out[3 * i + 2]; }
  cnt.resize(m); fst.resize(m);
  if (counts) *counts = cnt;
  if (first) *first = fst;
}

struct GbaEdge { int i, j; double rot[9], tra[3], v6[6]; };   // the arguments of PGO_Edges::push, LR:247

// The optimisation part of VOXEL_SLAM::HBA_add_edge (VS:2858-2951) for one connected keyframe set: xs in/out,
// clouds[i] = keyframe i's points in its own frame.  submap (optional) receives the cloud of VS:2954-2989.
inline std::vector<GbaEdge> HBA_add_edge(Context &ctx, std::vector<IMUST> &xs, const std::vector<std::vector<XYZ>> &clouds, double gba_voxel_size,
                                         double gba_min_eigen_value, const std::vector<double> &gba_eigen_value_array, int max_iter, int thread_num,
                                         std::vector<XYZ> *submap = nullptr) {
  const int W = (int)xs.size();
  std::vector<int> off(W + 1, 0);
  for (int i = 0; i < W; i++) off[i + 1] = off[i] + (int)clouds[i].size();
  std::vector<double> pts((size_t)off[W] * 3), poses = LidarFactor::poses_of(xs), edges((size_t)(W * (W - 1) / 2 + 1) * 20);
  for (int i = 0; i < W; i++)
    for (size_t k = 0; k < clouds[i].size(); k++) {
      double *q = &pts[((size_t)off[i] + k) * 3];
      q[0] = clouds[i][k].x; q[1] = clouds[i][k].y; q[2] = clouds[i][k].z;
    }
  double eig[4] = {0, 0, 0, 0};
  for (size_t k = 0; k < 4 && k < gba_eigen_value_array.size(); k++) eig[k] = gba_eigen_value_array[k];
  std::vector<double> cloud(submap ? pts.size() : 0);
  std::vector<int> ccnt(submap ? (size_t)off[W] : 0);
  int ne = 0, nc = 0;
  check(ctx.get(), vba_hba_add_edge(ctx.get(), W, off.data(), pts.data(), poses.data(), gba_voxel_size, gba_min_eigen_value, eig, max_iter, thread_num,
                                    edges.data(), &ne, submap ? cloud.data() : nullptr, submap ? ccnt.data() : nullptr, submap ? &nc : nullptr, nullptr, nullptr));
  for (int i = 0; i < W; i++) { std::memcpy(xs[i].R, &poses[12 * i], 72); std::memcpy(xs[i].p, &poses[12 * i + 9], 24); }
  std::vector<GbaEdge> out(ne);
  for (int e = 0; e < ne; e++) {
    const double *q = &edges[(size_t)e * 20];
    out[e].i = (int)q[0]; out[e].j = (int)q[1];
    std::memcpy(out[e].rot, q + 2, 72); std::memcpy(out[e].tra, q + 11, 24); std::memcpy(out[e].v6, q + 14, 48);
  }
  if (submap) { submap->resize(nc); for (int k = 0; k < nc; k++) (*submap)[k] = XYZ{(float)cloud[3 * k], (float)cloud[3 * k + 1], (float)cloud[3 * k + 2]}; }
  return out;
}

// The pose graph of build_graph (VS:2078-2156) and topDownProcess (VS:2717-2812): gtsam::Values initial + NonlinearFactorGraph
// graph, solved by vba_pgo_optimize with the ISAM2 schedule of VS:2550-2561.  Keys are the node ids 0..n-1 the
// reference uses (stepsizes[..] + scan index).  Variances take the place of noiseModel::Diagonal::Variances(v6).
class PoseGraph {
 public:
  void insert(int key, const IMUST &x) {                                            // initial.insert(j, Pose3(Rot3(x.R), x.p))
    if (key < 0) throw std::runtime_error("libvoxelba: PoseGraph::insert: negative key");
    if ((size_t)key >= have_.size()) { poses_.resize(12 * (size_t)(key + 1), 0.0); have_.resize(key + 1, 0); }
    std::memcpy(&poses_[12 * (size_t)key], x.R, 72); std::memcpy(&poses_[12 * (size_t)key + 9], x.p, 24);
    have_[key] = 1;
  }
  // add_edge(pos1, pos2, x1, x2, graph, noise) LR:147-153: the relative pose of x2 seen from x1
  void add_edge(int pos1, int pos2, const IMUST &x1, const IMUST &x2, const double *v6) {
    double rot[9], tra[3], d[3] = {x2.p[0] - x1.p[0], x2.p[1] - x1.p[1], x2.p[2] - x1.p[2]};
    for (int i = 0; i < 3; i++) {
      tra[i] = x1.R[i] * d[0] + x1.R[3 + i] * d[1] + x1.R[6 + i] * d[2];
      for (int j = 0; j < 3; j++) rot[3 * i + j] = x1.R[i] * x2.R[j] + x1.R[3 + i] * x2.R[3 + j] + x1.R[6 + i] * x2.R[6 + j];
    }
    add_edge(pos1, pos2, rot, tra, v6);
  }
  // add_edge(pos1, pos2, rot, tra, graph, noise) LR:155-161
  void add_edge(int pos1, int pos2, const double *rot, const double *tra, const double *v6) {
    edges_.push_back(pos1); edges_.push_back(pos2);
    edges_.insert(edges_.end(), rot, rot + 9); edges_.insert(edges_.end(), tra, tra + 3); edges_.insert(edges_.end(), v6, v6 + 6);
  }
  // graph.add(PriorFactor<Pose3>(key, Pose3(x.R, x.p), Variances(v6))) VS:2122-2133
  void add_prior(int key, const IMUST &x, const double *v6) {
    priors_.push_back(key);
    priors_.insert(priors_.end(), x.R, x.R + 9); priors_.insert(priors_.end(), x.p, x.p + 3); priors_.insert(priors_.end(), v6, v6 + 6);
  }
  // ISAM2 {relinearizeThreshold thr, relinearizeSkip 1}: update(graph, initial) + (updates - 1) x update(); calculateEstimate()
  // replaces the inserted poses.  Returns results.size().
  int optimize(Context &ctx, int updates = 6, double thr = 0.01) {
    for (size_t k = 0; k < have_.size(); k++)
      if (!have_[k]) throw std::runtime_error("libvoxelba: PoseGraph::optimize: key " + std::to_string(k) + " was never inserted");
    stats.assign(3 * (size_t)(updates > 0 ? updates : 1), 0.0);
    check(ctx.get(), vba_pgo_optimize(ctx.get(), (int)have_.size(), poses_.data(), (int)num_edges(), edges_.data(), (int)num_priors(),
                                      priors_.data(), updates, thr, stats.data()));
    return (int)have_.size();
  }
  const double *pose(int key) const { return &poses_.at(12 * (size_t)key); }   // results.at(key): [R(9) row-major, p(3)]
  size_t size() const { return have_.size(); }
  size_t num_edges() const { return edges_.size() / 20; }
  size_t num_priors() const { return priors_.size() / 19; }
  const std::vector<double> &edges() const { return edges_; }
  void clear() { poses_.clear(); have_.clear(); edges_.clear(); priors_.clear(); }   // initial.clear(); graph = NonlinearFactorGraph()
  std::vector<double> stats;   // [updates][3] of the last optimize: relinearised nodes, cost, max |delta|_inf
 private:
  std::vector<double> poses_, edges_, priors_;
  std::vector<char> have_;
};

// ScanPose::set_state(const gtsam::Pose3 &) LR:36-43: the velocity turns with the rotation change R_new R_old^T.
inline void set_state(IMUST &x, const double *pose12) {
  double rot[9], v[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) rot[3 * i + j] = pose12[3 * i] * x.R[3 * j] + pose12[3 * i + 1] * x.R[3 * j + 1] + pose12[3 * i + 2] * x.R[3 * j + 2];
  std::memcpy(x.R, pose12, 72); std::memcpy(x.p, pose12 + 9, 24);
  for (int i = 0; i < 3; i++) v[i] = rot[3 * i] * x.v[0] + rot[3 * i + 1] * x.v[1] + rot[3 * i + 2] * x.v[2];
  std::memcpy(x.v, v, 24);
}

// VOXEL_SLAM::lio_state_estimation(pptr) VS:962-1098 on a prepared scan frame (device arrays, consumed in place): x_curr in/out
inline bool lio_state_estimation(Context &ctx, const ScanView &scan, IMUST &x_curr) {
  int ok = 0;
  check(ctx.get(), vba_odom_lio_state_estimation(ctx.get(), scan.n, scan.pnt, scan.var, &x_curr.t, x_curr.cov, &ok));
  return ok != 0;
}

// The same with the EKF iterations resident on the device: one upload, one download, one wait.  report, when
// given, receives the iteration count, the matches and step norms per iteration and the smallest eigenvalue of nnt.
inline bool lio_state_estimation_resident(Context &ctx, const ScanView &scan, IMUST &x_curr, vba_odom_report *report = nullptr) {
  int ok = 0;
  check(ctx.get(), vba_odom_lio_state_estimation_resident(ctx.get(), scan.n, scan.pnt, scan.var, &x_curr.t, x_curr.cov, &ok, report));
  return ok != 0;
}

// VOXEL_SLAM::lio_state_estimation_kdtree(pptr) VS:1102-1252: x_curr (state + cov) in/out, the point-cloud map (pl_tree) lives in
// the context.  Returns the number of EKF iterations (0 while the map is only being seeded).
inline int lio_state_estimation_kdtree(Context &ctx, const std::vector<pointVar> &pvec, IMUST &x_curr) {
  const int n = (int)pvec.size();
  std::vector<double> p((size_t)n * 3);
  for (int i = 0; i < n; i++) { p[3 * i] = (float)pvec[i].pnt[0]; p[3 * i + 1] = (float)pvec[i].pnt[1]; p[3 * i + 2] = (float)pvec[i].pnt[2]; }   // PointType is float (VS:1143-1146)
  int iters = 0;
  check(ctx.get(), vba_odom_lio_state_estimation_kdtree(ctx.get(), n, p.data(), &x_curr.t, x_curr.cov, &iters));
  return iters;
}

// The same on a prepared scan frame: the frame's device points are read in place, as the doubles they are
// (pv.pnt is a Vector3d, VS:1155-1157; the overload above rounds them to float first), and the iterations, the map append and the
// re-sampling stay on the device: one upload, one download, one wait.  report, when given, receives the iteration count and the
// valid points and step norms per iteration.
inline int lio_state_estimation_kdtree(Context &ctx, const ScanView &scan, IMUST &x_curr, vba_odom_report *report = nullptr) {
  int iters = 0;
  check(ctx.get(), vba_odom_lio_state_estimation_kdtree_resident(ctx.get(), scan.n, scan.pnt, &x_curr.t, x_curr.cov, &iters, report));
  return iters;
}

// ---- the odometry state resident in HBM: x_curr and its covariance stay on the device from one scan to the next;
// the per-scan chain odom_ekf.process -> prepare -> lio_state_estimation -> pvec_update + cut_voxel_multi (VS:1873-1922) reads and
// writes them where they lie
class SurfelMap;
class OdomState {
 public:
  explicit OdomState(Context &ctx) : ctx_(ctx.get()) { check(ctx_, vba_odom_state_create(ctx_, &s_)); }
  ~OdomState() { vba_odom_state_destroy(s_); }
  OdomState(const OdomState &) = delete;
  OdomState &operator=(const OdomState &) = delete;
  void reserve(int max_imu_rows) { check(ctx_, vba_odom_state_reserve(s_, max_imu_rows)); }
  void set(const IMUST &x) { check(ctx_, vba_odom_state_set(s_, &x.t, x.cov)); }
  void get(IMUST &x) { check(ctx_, vba_odom_state_get(s_, &x.t, x.cov)); }
  // the pose table [n][22] of the last propagation and, when asked for, end_pose [12]
  std::vector<double> poses(double *end_pose12 = nullptr) {
    int n = 0;
    check(ctx_, vba_odom_state_poses(s_, 0, nullptr, nullptr, &n));
    std::vector<double> rows((size_t)22 * n);
    check(ctx_, vba_odom_state_poses(s_, n, rows.data(), end_pose12, &n));
    return rows;
  }
  // imu [m][7] = [t, gyr, acc] after push_front(last_imu); noise12 = cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc.  Returns the rows of the table.
  int propagate(const double *noise12, double scale_gravity, int m, const double *imu, double last_pcl_end_time, double pcl_beg_time, double pcl_end_time) {
    int n = 0;
    check(ctx_, vba_odom_state_propagate(s_, noise12, scale_gravity, m, imu, last_pcl_end_time, pcl_beg_time, pcl_end_time, &n));
    return n;
  }
  // ScanFrame::prepare with the table and end_pose of the last propagation read in place
  ScanView prepare(Context &ctx, ScanFrame &frame, const IMUST &ext, bool point_notime, double down_size, double dept_err, double beam_err,
                   int min_points = 500) {
    double x[12];
    std::memcpy(x, ext.R, 72); std::memcpy(x + 9, ext.p, 24);
    ScanView v;
    check(ctx.get(), vba_scan_prepare_on_state(ctx.get(), frame.get(), s_, x, point_notime ? 1 : 0, down_size, min_points, dept_err, beam_err, &v.n, &v.pnt, &v.var));
    return v;
  }
  // lio_state_estimation (VS:962-1098) on the resident state; x_out, when given, receives the updated state (not its covariance)
  bool lio_state_estimation(Context &ctx, const ScanView &scan, vba_odom_report *report = nullptr, IMUST *x_out = nullptr) {
    int ok = 0;
    check(ctx.get(), vba_odom_lio_state_estimation_on_state(ctx.get(), s_, scan.n, scan.pnt, scan.var, &ok, report, x_out ? &x_out->t : nullptr));
    return ok != 0;
  }
  // the same update against a prior map (vba::lio_state_estimation_prior below) on the resident state
  inline bool lio_state_estimation_prior(Context &ctx, SurfelMap &map, const ScanView &scan, const vba_surfel_odom_params &params,
                                         vba_odom_report *report = nullptr, IMUST *x_out = nullptr);
  // pvec_update + cut_voxel_multi (VS:1903-1920) with the pose and covariance blocks of the resident state
  void pvec_update_cut_voxel_multi(Context &ctx, const ScanView &scan, int win_count) {
    check(ctx.get(), vba_map_pvec_update_cut_voxel_on_state(ctx.get(), s_, win_count, scan.n, scan.pnt, scan.var, 1));
  }
  // lio_state_estimation_kdtree (VS:1102-1252) on the resident state and ctx's point-cloud map: returns the iterations,
  // 0 while the scan only seeds the map; x_out, when given, receives the state (not its covariance) after a seeding scan as well
  int lio_state_estimation_kdtree(Context &ctx, const ScanView &scan, vba_odom_report *report = nullptr, IMUST *x_out = nullptr) {
    int iters = 0;
    check(ctx.get(), vba_odom_lio_state_estimation_kdtree_on_state(ctx.get(), s_, scan.n, scan.pnt, &iters, report, x_out ? &x_out->t : nullptr));
    return iters;
  }
  // the scan that pub_localtraj publishes (VS:37-45): pvec_update's pwld in the pose of the resident state, records x y z intensity
  void export_scan(Context &ctx, const ScanView &scan, float intensity, std::vector<float> &xyzi) {
    int64_t n = 0;
    xyzi.resize((size_t)scan.n * 4);
    check(ctx.get(), vba_odom_state_export_scan(ctx.get(), s_, scan.n, scan.pnt, intensity, scan.n, xyzi.data(), &n));
  }
  vba_odom_state *get() const { return s_; }
 private:
  vba_ctx *ctx_;
  vba_odom_state *s_ = nullptr;
};

// ResultOutput::pub_localtraj (VS:32-58) on a state object: publish_scan(const float *xyzi, int64_t n) receives the scan in world
// coordinates (VS:37-46), then the path point of VS:48-56 is built from x_curr (the state_out of the update: host bookkeeping) and
// appended to pcl_path, which publish_path receives whole (VS:57).
struct PathPoint { float x, y, z, intensity, curvature; };
template <class PublishScan, class PublishPath>
inline void pub_localtraj(Context &ctx, OdomState &st, const ScanView &scan, double jour, const IMUST &x_curr, int cur_session,
                          std::vector<PathPoint> &pcl_path, PublishScan &&publish_scan, PublishPath &&publish_path) {
  std::vector<float> pl;
  st.export_scan(ctx, scan, 0.0f, pl);
  publish_scan((const float *)pl.data(), (int64_t)scan.n);
  PathPoint ap;
  ap.x = (float)x_curr.p[0]; ap.y = (float)x_curr.p[1]; ap.z = (float)x_curr.p[2];
  ap.curvature = (float)jour; ap.intensity = (float)cur_session;
  pcl_path.push_back(ap);
  publish_path(pcl_path);
}

// class IMUEKF (ekf_imu.hpp, "EK"): its fields and call surface without the point loop of the undistortion (EK:135-163), which is
// ScanFrame::prepare.  A deque holds ImuSample values where the reference holds sensor_msgs::Imu::Ptr.
class ImuEkf {
 public:
  bool init_flag = false;
  double pcl_beg_time = 0, pcl_end_time = 0, last_pcl_end_time = 0;
  int init_num = 0;
  double mean_acc[3] = {0, 0, 0}, mean_gyr[3] = {0, 0, 0};
  ImuSample last_imu{};
  int min_init_num = 30;
  double cov_acc[3] = {0, 0, 0}, cov_gyr[3] = {0, 0, 0}, cov_bias_gyr[3] = {0, 0, 0}, cov_bias_acc[3] = {0, 0, 0};
  double scale_gravity = 1.0;
  std::vector<double> imu_poses;     // [n][22], the rows of vba_scan_undistort (host propagation only; on a state the table stays on the device)
  int n_poses = 0;
  double end_pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  std::string imu_topic = "/livox/imu";
  int point_notime = 0;

  void IMU_init(std::deque<ImuSample> &imus) {                                                    // EK:167-195
    for (const ImuSample &imu : imus) {
      if (init_num != 0) {
        for (int k = 0; k < 3; k++) { mean_acc[k] += (imu.acc[k] - mean_acc[k]) / init_num; mean_gyr[k] += (imu.gyr[k] - mean_gyr[k]) / init_num; }
      } else {
        for (int k = 0; k < 3; k++) { mean_acc[k] = imu.acc[k]; mean_gyr[k] = imu.gyr[k]; }
        init_num = 1;
      }
      init_num++;
    }
    last_imu = imus.back();
  }
  // process(x_curr, pcl_in, imus) EK:197-214 with the propagation on the host: 0 while initialising, then 1
  int process(IMUST &x_curr, std::deque<ImuSample> &imus) {
    if (!init_flag) return init_step(x_curr, imus);
    std::vector<double> rows = begin_blur(imus);
    imu_poses.assign((size_t)22 * (imus.size() - 1), 0.0);
    double noise[12];
    noise12(noise);
    const int st = vba_imu_ekf_propagate((int)imus.size(), rows.data(), noise, scale_gravity, last_pcl_end_time, pcl_beg_time, pcl_end_time, &x_curr.t,
                                         x_curr.cov, imu_poses.data(), end_pose, &n_poses);
    if (st != VBA_OK) { imus.pop_front(); check(nullptr, st); }
    imu_poses.resize((size_t)22 * n_poses);
    end_blur(imus);
    return 1;
  }
  // the same on a resident state: x_curr is written only while initialising (the caller sets the state once that has ended); the
  // table and end_pose stay on the device for OdomState::prepare
  int process(OdomState &state, IMUST &x_curr, std::deque<ImuSample> &imus) {
    if (!init_flag) return init_step(x_curr, imus);
    std::vector<double> rows = begin_blur(imus);
    double noise[12];
    noise12(noise);
    try { n_poses = state.propagate(noise, scale_gravity, (int)imus.size(), rows.data(), last_pcl_end_time, pcl_beg_time, pcl_end_time); }
    catch (...) { imus.pop_front(); throw; }
    end_blur(imus);
    return 1;
  }

 private:
  void noise12(double *n) const { std::memcpy(n, cov_gyr, 24); std::memcpy(n + 3, cov_acc, 24); std::memcpy(n + 6, cov_bias_gyr, 24); std::memcpy(n + 9, cov_bias_acc, 24); }
  int init_step(IMUST &x_curr, std::deque<ImuSample> &imus) {                                     // EK:199-210
    IMU_init(imus);
    double norm = 0;
    for (int k = 0; k < 3; k++) norm += mean_acc[k] * mean_acc[k];
    if (norm < 4 && imu_topic == "/livox/imu") scale_gravity = 9.8;                               // G_m_s2, TL:15
    for (int k = 0; k < 3; k++) x_curr.g[k] = -mean_acc[k] * scale_gravity;
    if (init_num > min_init_num) init_flag = true;
    last_pcl_end_time = pcl_end_time;
    return 0;
  }
  // EK:43-49: push_front(last_imu), the "LiDAR time regress" exit as an exception; the deque as rows [m][7]
  std::vector<double> begin_blur(std::deque<ImuSample> &imus) {
    if (last_pcl_end_time - pcl_beg_time > 0.01) throw std::runtime_error("LiDAR time regress. Please check data");
    imus.push_front(last_imu);
    std::vector<double> rows(imus.size() * 7);
    for (size_t i = 0; i < imus.size(); i++) { rows[7 * i] = imus[i].t; std::memcpy(&rows[7 * i + 1], imus[i].gyr, 24); std::memcpy(&rows[7 * i + 4], imus[i].acc, 24); }
    return rows;
  }
  // EK:125-133: last_imu keeps the back as it came, front and back become copies re-stamped to the scan's ends (push_imu reads them, VS:1913)
  void end_blur(std::deque<ImuSample> &imus) {
    ImuSample imu1 = imus.front(), imu2 = imus.back();
    imu1.t = last_pcl_end_time; imu2.t = pcl_end_time;
    last_imu = imus.back();
    last_pcl_end_time = pcl_end_time;
    imus.front() = imu1; imus.back() = imu2;
  }
};

// FileReaderWriter::save_pcd / save_pose (VS:166-204), pcl::io::loadPCDFile (VS:340), read_lidarstate (VH:268-307)
inline void save_pcd(const std::vector<pointVar> &pvec, int count, const std::string &savename) {
  std::vector<double> p(pvec.size() * 3);
  for (size_t i = 0; i < pvec.size(); i++) std::memcpy(&p[3 * i], pvec[i].pnt, 24);
  const std::string path = savename + "/" + std::to_string(count) + ".pcd";
  if (vba_io_save_pcd(path.c_str(), (int)pvec.size(), p.data())) throw std::runtime_error("save_pcd: " + path);
}
inline std::vector<XYZ> load_pcd(const std::string &path) {
  int n = 0;
  int st = vba_io_load_pcd(path.c_str(), 0, nullptr, nullptr, &n);
  if (st != VBA_OK && st != VBA_ERR_CAPACITY) throw std::runtime_error("load_pcd: " + path);
  std::vector<double> p((size_t)(n > 0 ? n : 1) * 3);
  if (vba_io_load_pcd(path.c_str(), n, p.data(), nullptr, &n)) throw std::runtime_error("load_pcd: " + path);
  std::vector<XYZ> out(n);
  for (int i = 0; i < n; i++) out[i] = XYZ{(float)p[3 * i], (float)p[3 * i + 1], (float)p[3 * i + 2]};
  return out;
}
struct ScanPoseRec { IMUST x; double v6[6]; };   // ScanPose (LR:17-27) without the point pointer
inline void save_pose(const std::vector<ScanPoseRec> &bbuf, const std::string &path) {
  std::vector<double> st(bbuf.size() * 25), v6(bbuf.size() * 6);
  for (size_t i = 0; i < bbuf.size(); i++) { std::memcpy(&st[25 * i], &bbuf[i].x.t, 200); std::memcpy(&v6[6 * i], bbuf[i].v6, 48); }
  if (vba_io_save_pose(path.c_str(), (int)bbuf.size(), st.data(), v6.data())) throw std::runtime_error("save_pose: " + path);
}
inline std::vector<ScanPoseRec> read_lidarstate(const std::string &filename) {
  int n = 0;
  int st = vba_io_read_lidarstate(filename.c_str(), 0, nullptr, nullptr, &n);
  if (st != VBA_OK && st != VBA_ERR_CAPACITY) throw std::runtime_error("read_lidarstate: " + filename);   // the reference exits (VH:271-275)
  std::vector<double> s((size_t)(n > 0 ? n : 1) * 25), v6((size_t)(n > 0 ? n : 1) * 6);
  if (vba_io_read_lidarstate(filename.c_str(), n, s.data(), v6.data(), &n)) throw std::runtime_error("read_lidarstate: " + filename);
  std::vector<ScanPoseRec> out(n);
  for (int i = 0; i < n; i++) {
    std::memcpy(&out[i].x.t, &s[25 * (size_t)i], 200); std::memcpy(out[i].v6, &v6[6 * (size_t)i], 48);
    for (int k = 0; k < 225; k++) out[i].x.cov[k] = 0.0;
    for (int k = 0; k < 15; k++) out[i].x.cov[16 * k] = k < 9 ? 1e-4 : 1e-5;       // IMUST::setZero (TL:188-197)
  }
  return out;
}

// ---- loop retrieval: the database half of STDescManager (BTC.h:228-300; AddSTDescs / SearchLoop, BTC.cpp:205-277) and icp_normal
// (loop_refine.hpp:47-139), and descriptor generation (GenerateSTDescs, BTC.cpp:156-203) on the device.  The structs below mirror STD and
// BinaryDescriptor (BTC.h:59-84) with the occupancy array as a bit mask (entry k = bit k) and angle_ left out (retrieval never
// reads it).  A loop transform is (t, R row-major), the pair<Vector3d, Matrix3d> of the reference.
struct BinaryDescriptor {
  uint64_t occupy_bits = 0;        // occupy_array_
  unsigned char summary_ = 0;
  double location_[3] = {0, 0, 0};
};
struct STD {
  double triangle_[3] = {0, 0, 0};
  double center_[3] = {0, 0, 0};
  int frame_number_ = 0;
  BinaryDescriptor binary_A_, binary_B_, binary_C_;
};
struct LoopTransform { double t[3] = {0, 0, 0}; double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; };

inline void pack_stds(const std::vector<STD> &v, std::vector<double> &rows, std::vector<uint64_t> &bits) {
  rows.assign(v.size() * VBA_BTC_ROW_LEN, 0.0);
  bits.assign(v.size() * 3, 0);
  for (size_t i = 0; i < v.size(); i++) {
    double *r = rows.data() + i * VBA_BTC_ROW_LEN;
    const BinaryDescriptor *b[3] = {&v[i].binary_A_, &v[i].binary_B_, &v[i].binary_C_};
    for (int k = 0; k < 3; k++) { r[k] = v[i].triangle_[k]; r[3 + k] = v[i].center_[k]; }
    r[6] = v[i].frame_number_;
    for (int e = 0; e < 3; e++) {
      for (int k = 0; k < 3; k++) r[7 + 3 * e + k] = b[e]->location_[k];
      r[16 + e] = b[e]->summary_;
      bits[3 * i + e] = b[e]->occupy_bits;
    }
  }
}

inline void unpack_stds(const std::vector<double> &rows, const std::vector<uint64_t> &bits, int n, std::vector<STD> &stds_vec) {
  stds_vec.assign(n, STD{});
  for (int i = 0; i < n; i++) {
    const double *r = rows.data() + (size_t)i * VBA_BTC_ROW_LEN;
    STD &d = stds_vec[i];
    BinaryDescriptor *b[3] = {&d.binary_A_, &d.binary_B_, &d.binary_C_};
    for (int u = 0; u < 3; u++) { d.triangle_[u] = r[u]; d.center_[u] = r[3 + u]; }
    d.frame_number_ = (int)r[6];
    for (int e = 0; e < 3; e++) {
      for (int u = 0; u < 3; u++) b[e]->location_[u] = r[7 + 3 * e + u];
      b[e]->summary_ = (unsigned char)r[16 + e];
      b[e]->occupy_bits = bits[3 * (size_t)i + e];
    }
  }
}

// STDescManager's database: one per session, on the loop-closure thread's context.  Destroy it before its Context.
class BtcDatabase {
 public:
  struct ConfigSetting { int skip_near_num_; };   // the field the node writes to close a session (VS:410, VS:2242)
  ConfigSetting config_setting_;
  BtcDatabase(Context &ctx, const vba_btc_config &cfg, const vba_btc_gen_config *gen_cfg = nullptr) : ctx_(ctx.get()) {
    check(ctx_, vba_btc_create(ctx_, &cfg, &db_));
    config_setting_.skip_near_num_ = cfg.skip_near_num;
    if (gen_cfg) check(ctx_, vba_btc_set_gen_config(db_, gen_cfg));
    vba_btc_gen_config g;
    check(ctx_, vba_btc_get_gen_config(db_, &g));
    const int k1 = (int)g.descriptor_near_num - 1;
    gen_cap_ = g.useful_corner_num * (k1 * (k1 - 1) / 2);
  }
  ~BtcDatabase() { vba_btc_destroy(db_); }
  BtcDatabase(const BtcDatabase &) = delete;
  BtcDatabase &operator=(const BtcDatabase &) = delete;
  vba_btc_db *get() const { return db_; }
  // plane_cloud_vec_.push_back(plane_cloud) with header.seq = seq (BTC.cpp:156-168); xyz_normal: n x 6 floats
  void push_plane_cloud(const std::vector<float> &xyz_normal, int seq) {
    check(ctx_, vba_btc_push_plane_cloud(db_, (int)(xyz_normal.size() / 6), xyz_normal.data(), seq));
  }
  int plane_cloud_num() const { return vba_btc_num_frames(db_); }      // plane_cloud_vec_.size()
  // GenerateSTDescs(input_cloud, stds_vec, id) (BTC.cpp:156-203): xyz = the PointXYZI cloud's x y z (n x 3 floats); pushes the plane
  // cloud with header.seq = id; frame_number_ = current_frame_id_ (the AddSTDescs count)
  void GenerateSTDescs(const std::vector<float> &xyz, std::vector<STD> &stds_vec, int id) {
    std::vector<double> rows((size_t)(gen_cap_ > 0 ? gen_cap_ : 1) * VBA_BTC_ROW_LEN);
    std::vector<uint64_t> bits((size_t)(gen_cap_ > 0 ? gen_cap_ : 1) * 3);
    int n = 0;
    check(ctx_, vba_btc_generate_stds(db_, (int)(xyz.size() / 3), xyz.data(), id, gen_cap_, rows.data(), bits.data(), &n));
    unpack_stds(rows, bits, n, stds_vec);
  }
  int gen_cap() const { return gen_cap_; }
  int plane_cloud_seq(int frame) const { int s = 0; check(ctx_, vba_btc_frame_seq(db_, frame, &s)); return s; }
  void AddSTDescs(const std::vector<STD> &stds) {                          // BTC.cpp:258-277
    std::vector<double> rows; std::vector<uint64_t> bits;
    pack_stds(stds, rows, bits);
    check(ctx_, vba_btc_add_stds(db_, (int)stds.size(), rows.data(), bits.data()));
  }
  // SearchLoop(stds_vec, loop_result, loop_transform, loop_std_pair, pl_cur) (BTC.cpp:205-256) with pl_cur = plane cloud cur_frame
  // of cur (VS:2421 passes std_manager->plane_cloud_vec_.back()).  loop_std_pair is cleared: it is always empty in the reference.
  void SearchLoop(const std::vector<STD> &stds, std::pair<int, double> &loop_result, LoopTransform &loop_transform,
                  std::vector<std::pair<STD, STD>> &loop_std_pair, const BtcDatabase &cur, int cur_frame) {
    std::vector<BtcDatabase *> one{this};
    std::vector<vba_btc_result> r;
    search_loop_sessions(one, stds, cur, cur_frame, r);
    loop_std_pair.clear();
    loop_result = std::make_pair(r[0].loop_id, r[0].score);
    if (r[0].loop_id >= 0) { std::memcpy(loop_transform.t, r[0].t, 24); std::memcpy(loop_transform.R, r[0].R, 72); }
  }
  // the loop over sessions `for (id = 0; id <= cur_id; id++) SearchLoop(...)` (VS:2417-2421) as one batched call
  static void search_loop_sessions(const std::vector<BtcDatabase *> &dbs, const std::vector<STD> &stds, const BtcDatabase &cur, int cur_frame,
                                   std::vector<vba_btc_result> &results) {
    std::vector<double> rows; std::vector<uint64_t> bits;
    pack_stds(stds, rows, bits);
    std::vector<vba_btc_db *> h(dbs.size());
    for (size_t k = 0; k < dbs.size(); k++) { h[k] = dbs[k]->db_; vba_btc_set_skip_near_num(h[k], dbs[k]->config_setting_.skip_near_num_); }
    results.assign(dbs.size(), vba_btc_result{});
    check(cur.ctx_, vba_btc_search_loop_sessions((int)dbs.size(), h.data(), (int)stds.size(), rows.data(), bits.data(), cur.db_, cur_frame,
                                                 results.data()));
  }
 private:
  vba_ctx *ctx_ = nullptr;
  vba_btc_db *db_ = nullptr;
  int gen_cap_ = 0;                // row capacity GenerateSTDescs needs: useful_corner_num * C(K - 1, 2)
};

// icp_normal(pl_src, pl_tar, pose, icp_eigval) (loop_refine.hpp:47-139) at its call site VS:2434, both clouds resident: pose
// updated in place, the return value of the reference; eig / iters optional.
inline bool icp_normal(BtcDatabase &src, int src_frame, BtcDatabase &tar, int tar_frame, LoopTransform &pose, double icp_eigval,
                       double *eig = nullptr, int *iters = nullptr) {
  int ok = 0;
  const int st = vba_btc_icp_normal(src.get(), src_frame, tar.get(), tar_frame, pose.t, pose.R, icp_eigval, &ok, eig, iters);
  if (st != VBA_OK) throw std::runtime_error(std::string("libvoxelba: icp_normal: ") + vba_status_string(st));
  return ok != 0;
}

// `vector<Keyframe*> *keyframes` of one session, resident in HBM (voxelba.h "Keyframe store").  The caller's
// mtx_keyframe excludes readers while build / reserve / keyframe_loading run: growing the store moves its arrays.  Destroy it
// before its Context.
struct ScanPoseRef { const IMUST *x; const PVec *pvec; };   // what VS:2357-2371 reads of a ScanPose: bl.x and *bl.pvec
class KeyframeStore {
 public:
  explicit KeyframeStore(Context &ctx) : ctx_(ctx.get()) { check(ctx_, vba_kf_create(ctx_, &s_)); }
  ~KeyframeStore() { vba_kf_destroy(s_); }
  KeyframeStore(const KeyframeStore &) = delete;
  KeyframeStore &operator=(const KeyframeStore &) = delete;
  vba_kf_store *get() const { return s_; }
  void reserve(int64_t points, int keyframes, int64_t merge_points) { check(ctx_, vba_kf_reserve(s_, points, keyframes, merge_points)); }
  int size() const { return vba_kf_size(s_); }                                  // keyframes->size()
  // VS:2354-2406: the scans of bl_local merged into the frame of the last one (its x becomes the keyframe's x0),
  // down_sampling_pvec(voxel_size / 10) kept as the keyframe's cloud, and, with a database, GenerateSTDescs(plbtc, stds_vec, id) on
  // the merged cloud.  Returns the size of the kept cloud.
  int build(const std::vector<ScanPoseRef> &bl_local, double voxel_size_10, int id, double jour, BtcDatabase *db = nullptr,
            std::vector<STD> *stds_vec = nullptr) {
    const int k = (int)bl_local.size();
    std::vector<int> off(k + 1, 0);
    for (int i = 0; i < k; i++) off[i + 1] = off[i] + (int)bl_local[i].pvec->size();
    std::vector<double> pnt((size_t)off[k] * 3), var((size_t)off[k] * 9), poses((size_t)k * 12);
    for (int i = 0; i < k; i++) {
      std::memcpy(&poses[(size_t)i * 12], bl_local[i].x->R, 72); std::memcpy(&poses[(size_t)i * 12 + 9], bl_local[i].x->p, 24);
      size_t r = (size_t)off[i];
      for (const pointVar &pv : *bl_local[i].pvec) { std::memcpy(&pnt[3 * r], pv.pnt, 24); std::memcpy(&var[9 * r], pv.var, 72); r++; }
    }
    const int cap = db ? db->gen_cap() : 0;
    std::vector<double> rows((size_t)(cap > 0 ? cap : 1) * VBA_BTC_ROW_LEN);
    std::vector<uint64_t> bits((size_t)(cap > 0 ? cap : 1) * 3);
    int n = 0, kept = 0;
    check(ctx_, vba_kf_build(s_, k, off.data(), pnt.data(), var.data(), poses.data(), voxel_size_10, id, jour, db ? db->get() : nullptr, cap,
                             rows.data(), bits.data(), &n, &kept));
    if (db && stds_vec) unpack_stds(rows, bits, n, *stds_vec);
    return kept;
  }
  // the same from a ScanLog (defined below, after ScanLog): scans first .. first + bl_poses.size() - 1 at bl_poses (their bl.x),
  // merged from the log's arena in place
  inline int build(ScanLog &log, int64_t first, const std::vector<IMUST> &bl_poses, double voxel_size_10, int id, double jour,
                   BtcDatabase *db = nullptr, std::vector<STD> *stds_vec = nullptr);
  // VS:384-409: descriptors of keyframes [first, first + count) merged into the last one's frame, from the store
  void GenerateSTDescs(int first, int count, BtcDatabase &db, std::vector<STD> &stds_vec) {
    const int cap = db.gen_cap();
    std::vector<double> rows((size_t)(cap > 0 ? cap : 1) * VBA_BTC_ROW_LEN);
    std::vector<uint64_t> bits((size_t)(cap > 0 ? cap : 1) * 3);
    int n = 0;
    check(ctx_, vba_kf_generate_stds(s_, first, count, db.get(), cap, rows.data(), bits.data(), &n));
    unpack_stds(rows, bits, n, stds_vec);
  }
  // kf->x0 = scanPoses[kf->id]->x (VS:2582-2587): xs[i] is the new pose of keyframe first + i
  void set_poses(int first, const std::vector<IMUST> &xs) {
    const std::vector<double> p = LidarFactor::poses_of(xs);
    check(ctx_, vba_kf_set_poses(s_, first, (int)xs.size(), p.data()));
  }
  void set_history(int n_hist) { check(ctx_, vba_kf_set_history(s_, n_hist)); }  // VS:2628-2647
  int history_kfsize() const { return vba_kf_history_size(s_); }
  // keyframe_loading(jour) (VS:1379-1438) into the map of `map` around x_curr.p; returns the loaded keyframe or -1
  int keyframe_loading(Context &map, const IMUST &x_curr, double jour, double radius = 10) {
    int k = -1;
    check(ctx_, vba_kf_load_nearby(s_, map.get(), x_curr.p, radius, jour, &k));
    return k;
  }
  // the (offsets, pnt_local) arguments of vba_hba_add_edge / vba_hba_global / vba_gba_build, zero copy: pnt_local is DEVICE memory
  void clouds(const double *&d_pnt, const int *&offsets, int &n_kf) const { check(ctx_, vba_kf_clouds(s_, &d_pnt, &offsets, &n_kf)); }
  // smps[i]->plptr->size() for every keyframe: the `sizes` of vba_kf_export_plan
  std::vector<int> sizes() const {
    const double *d_pnt; const int *off; int n = 0;
    clouds(d_pnt, off, n);
    std::vector<int> out((size_t)n);
    for (int i = 0; i < n; i++) out[i] = off[i + 1] - off[i];
    return out;
  }
  // keyframe k's plptr on the host (save_pcd, tests): x y z and normal_x/y/z
  void read(int k, std::vector<XYZ> &xyz, std::vector<XYZ> *normal = nullptr) const {
    int n = 0;
    check(ctx_, vba_kf_read(s_, k, 0, nullptr, nullptr, &n));
    std::vector<double> p((size_t)(n > 0 ? n : 1) * 3);
    std::vector<float> v((size_t)(n > 0 ? n : 1) * 3);
    check(ctx_, vba_kf_read(s_, k, n, p.data(), v.data(), &n));
    xyz.resize(n);
    if (normal) normal->resize(n);
    for (int i = 0; i < n; i++) {
      xyz[i] = XYZ{(float)p[3 * (size_t)i], (float)p[3 * (size_t)i + 1], (float)p[3 * (size_t)i + 2]};
      if (normal) (*normal)[i] = XYZ{v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]};
    }
  }
 private:
  vba_ctx *ctx_ = nullptr;
  vba_kf_store *s_ = nullptr;
};

// ResultOutput::pub_globalmap (VS:110-154) from the stores: relc_submaps[id] is session id's store, `ids` the sessions to publish in
// order, publish(const float *xyzi, int64_t n) receives one message of n records x y z intensity (intensity = id), the final one
// included even when it is empty (VS:153).  The empty publish that clears the display first (VS:113) stays with the caller.  The
// work runs on ctx's stream; the caller holds mtx_keyframe as for any reader of the stores.  Returns the jump in force.
template <class Publish>
inline int pub_globalmap(Context &ctx, const std::vector<KeyframeStore *> &relc_submaps, const std::vector<int> &ids, Publish &&publish,
                         int64_t interval_size = 5000000, int jump = 0) {
  std::vector<vba_kf_store *> stores;
  std::vector<float> intensity;
  std::vector<int> sizes;
  for (int id : ids) {
    KeyframeStore &smps = *relc_submaps.at((size_t)id);
    stores.push_back(smps.get());
    intensity.push_back((float)id);                                             // pp.intensity = id, VS:128
    const std::vector<int> sz = smps.sizes();
    sizes.insert(sizes.end(), sz.begin(), sz.end());
  }
  const int n_kf = (int)sizes.size();
  std::vector<int64_t> kf_begin((size_t)n_kf + 1);
  std::vector<int> msg_end((size_t)n_kf + 1);
  int n_msgs = 0;
  check(ctx.get(), vba_kf_export_plan(n_kf, sizes.data(), interval_size, jump, &jump, kf_begin.data(), n_kf + 1, msg_end.data(), &n_msgs));
  std::vector<float> pl;
  int k0 = 0;
  for (int m = 0; m < n_msgs; m++) {
    const int64_t begin = kf_begin[(size_t)k0], n = kf_begin[(size_t)msg_end[(size_t)m]] - begin;
    pl.resize((size_t)n * 4);
    if (n > 0) check(ctx.get(), vba_kf_export_world(ctx.get(), (int)stores.size(), stores.data(), intensity.data(), jump, begin, n, pl.data()));
    publish((const float *)pl.data(), n);
    k0 = msg_end[(size_t)m];
  }
  return jump;
}

// Where a result of n records is cut into messages of at most interval_size records: ends[m] = one past the last record of message
// m.  One final message always follows the full ones; it is empty only when n == 0 (a cloud is published whatever it holds, VS:153).
inline std::vector<int64_t> voxel_message_ends(int64_t n, int64_t interval_size) {
  if (n < 0 || interval_size < 1) throw std::invalid_argument("voxel_message_ends");
  std::vector<int64_t> ends;
  int64_t b = 0;
  while (n - b > interval_size) { b += interval_size; ends.push_back(b); }
  ends.push_back(n);
  return ends;
}

// The global map voxel-down-sampled (vba_kf_voxel_export): the records pub_globalmap would publish at `jump`, one per
// voxel of voxel_size (the centroid; intensity = the id of the voxel's first record), voxels of fewer than min_count records left
// out, in messages of at most interval_size records (voxel_message_ends).  publish(const float *xyzi, int64_t n) as pub_globalmap;
// the caller holds mtx_keyframe.  Two device passes: the size query, then the result.  Returns the number of records.
template <class Publish>
inline int64_t pub_globalmap_voxel(Context &ctx, const std::vector<KeyframeStore *> &relc_submaps, const std::vector<int> &ids, double voxel_size,
                                   Publish &&publish, int min_count = 1, int64_t interval_size = 5000000, int jump = 1) {
  std::vector<vba_kf_store *> stores;
  std::vector<float> intensity;
  for (int id : ids) {
    stores.push_back(relc_submaps.at((size_t)id)->get());
    intensity.push_back((float)id);                                             // pp.intensity = id, VS:128
  }
  int64_t n = 0;
  std::vector<float> pl;
  if (!stores.empty()) {
    check(ctx.get(), vba_kf_voxel_export(ctx.get(), (int)stores.size(), stores.data(), intensity.data(), jump, voxel_size, min_count, 0, nullptr, nullptr, &n));
    pl.resize((size_t)n * 4);
    if (n > 0)
      check(ctx.get(), vba_kf_voxel_export(ctx.get(), (int)stores.size(), stores.data(), intensity.data(), jump, voxel_size, min_count, n, pl.data(), nullptr, &n));
  }
  int64_t b = 0;
  for (int64_t e : voxel_message_ends(n, interval_size)) {
    publish((const float *)pl.data() + 4 * b, e - b);
    b = e;
  }
  return n;
}

// The global map as surfels (vba_kf_surfel_export): one record of 12 floats per voxel of pub_globalmap_voxel (mean,
// intensity = the id of the voxel's first record, normal toward the sensor, sqrt of the eigenvalues, l0 / trace, count) and its
// covariance of 6 doubles, voxels of fewer than min_count records left out, cut into messages as pub_globalmap_voxel cuts them.
// publish(const float *records, const double *cov, int64_t n) receives one message; the caller holds mtx_keyframe.  Two device
// passes: the size query, then the result.  Returns the number of records.
template <class Publish>
inline int64_t pub_globalmap_surfel(Context &ctx, const std::vector<KeyframeStore *> &relc_submaps, const std::vector<int> &ids, double voxel_size,
                                    Publish &&publish, int min_count = 3, int64_t interval_size = 5000000, int jump = 1) {
  std::vector<vba_kf_store *> stores;
  std::vector<float> intensity;
  for (int id : ids) {
    stores.push_back(relc_submaps.at((size_t)id)->get());
    intensity.push_back((float)id);                                             // pp.intensity = id, VS:128
  }
  int64_t n = 0;
  std::vector<float> pl;
  std::vector<double> cov;
  if (!stores.empty()) {
    check(ctx.get(), vba_kf_surfel_export(ctx.get(), (int)stores.size(), stores.data(), intensity.data(), jump, voxel_size, min_count, 0, nullptr, nullptr,
                                          nullptr, &n));
    pl.resize((size_t)n * 12);
    cov.resize((size_t)n * 6);
    if (n > 0)
      check(ctx.get(), vba_kf_surfel_export(ctx.get(), (int)stores.size(), stores.data(), intensity.data(), jump, voxel_size, min_count, n, pl.data(),
                                            cov.data(), nullptr, &n));
  }
  int64_t b = 0;
  for (int64_t e : voxel_message_ends(n, interval_size)) {
    publish((const float *)pl.data() + 12 * b, (const double *)cov.data() + 6 * b, e - b);
    b = e;
  }
  return n;
}

// ---- prior-map localisation (voxelba.h "Registration of a scan against the surfel map").  No reference counterpart:
// the cells of an earlier session's finished map in HBM, and the registration of a scan or a keyframe against them.  Works on ctx's
// stream; the caller holds mtx_keyframe while a map is built from stores.  Destroy it before its Context.
class SurfelMap {
 public:
  explicit SurfelMap(Context &ctx) : ctx_(ctx.get()) { check(ctx_, vba_surfel_map_create(ctx_, &m_)); }
  ~SurfelMap() { vba_surfel_map_destroy(m_); }
  SurfelMap(const SurfelMap &) = delete;
  SurfelMap &operator=(const SurfelMap &) = delete;
  vba_surfel_map *get() const { return m_; }
  vba_ctx *ctx() const { return ctx_; }
  void reserve(int64_t max_cells, int64_t max_points) { check(ctx_, vba_surfel_map_reserve(m_, max_cells, max_points)); }
  // from the messages of pub_globalmap_surfel: records [n][12], cov [n][6] (host or device arrays).  Returns the cells.
  int64_t build(int64_t n, const float *records, const double *cov, double voxel_size, double sigma = 0.02, int min_count = 5) {
    int64_t cells = 0;
    check(ctx_, vba_surfel_map_build(m_, n, records, cov, voxel_size, sigma, min_count, &cells));
    return cells;
  }
  // from the stores, as pub_globalmap_surfel reads them: relc_submaps[id] for every id of `ids`
  int64_t build(const std::vector<KeyframeStore *> &relc_submaps, const std::vector<int> &ids, double voxel_size, double sigma = 0.02, int min_count = 5,
                int jump = 1) {
    std::vector<vba_kf_store *> stores;
    for (int id : ids) stores.push_back(relc_submaps.at((size_t)id)->get());
    int64_t cells = 0;
    check(ctx_, vba_surfel_map_build_from_kf(m_, (int)stores.size(), stores.data(), jump, voxel_size, sigma, min_count, &cells));
    return cells;
  }
  int64_t size() const {
    int64_t cells = 0;
    check(ctx_, vba_surfel_map_size(m_, &cells, nullptr, nullptr));
    return cells;
  }
 private:
  vba_ctx *ctx_ = nullptr;
  vba_surfel_map *m_ = nullptr;
};

inline vba_surfel_reg_params surfel_reg_defaults() { vba_surfel_reg_params p; vba_surfel_reg_default_params(&p); return p; }

namespace detail {
inline bool relocalize_points(SurfelMap &map, int64_t n, const double *d_pnt, IMUST &x, vba_surfel_reg_report *rep, const vba_surfel_reg_params &params) {
  double R[9], t[3];
  std::memcpy(R, x.R, 72); std::memcpy(t, x.p, 24);
  vba_surfel_reg_report local;
  vba_surfel_reg_report *r = rep ? rep : &local;
  check(map.ctx(), vba_surfel_register(map.get(), n, d_pnt, &params, R, t, r));
  const bool ok = r->converged && !r->lost && !r->singular;
  if (ok) { std::memcpy(x.R, R, 72); std::memcpy(x.p, t, 24); }
  return ok;
}
}  // namespace detail

// x.R, x.p = the pose of the scan in the map's frame, from x as the first guess.  Written only when the registration converged and
// was neither lost nor singular, which is what it returns; rep->eig_tt[0] is the degeneracy figure to threshold.
inline bool relocalize(SurfelMap &map, const ScanView &scan, IMUST &x, vba_surfel_reg_report *rep = nullptr,
                       const vba_surfel_reg_params &params = surfel_reg_defaults()) {
  return detail::relocalize_points(map, scan.n, scan.pnt, x, rep, params);
}
// the same for keyframe kf of a store (of this or another session), read in place
inline bool relocalize(SurfelMap &map, KeyframeStore &store, int kf, IMUST &x, vba_surfel_reg_report *rep = nullptr,
                       const vba_surfel_reg_params &params = surfel_reg_defaults()) {
  const double *d_pnt; const int *off; int n_kf = 0;
  store.clouds(d_pnt, off, n_kf);
  if (kf < 0 || kf >= n_kf) throw std::runtime_error("libvoxelba: relocalize: no such keyframe");
  return detail::relocalize_points(map, off[kf + 1] - off[kf], d_pnt + 3 * (size_t)off[kf], x, rep, params);
}

// ---- localisation mode (voxelba.h "Odometry update against a prior map"): lio_state_estimation with the cells of a
// prior map in the place of the live voxel map.  x_curr (state + cov) in/out; returns ok (enough matches, no degenerate direction
// by params.min_eig); the state is updated either way, as in lio_state_estimation.  The start must lie within the gate (relocalize).
inline vba_surfel_odom_params surfel_odom_defaults() { vba_surfel_odom_params p; vba_surfel_odom_default_params(&p); return p; }
inline bool lio_state_estimation_prior(Context &ctx, SurfelMap &map, const ScanView &scan, IMUST &x_curr,
                                       const vba_surfel_odom_params &params = surfel_odom_defaults(), vba_odom_report *report = nullptr) {
  int ok = 0;
  check(ctx.get(), vba_odom_surfel_update(ctx.get(), map.get(), scan.n, scan.pnt, &params, &x_curr.t, x_curr.cov, &ok, report));
  return ok != 0;
}
inline bool OdomState::lio_state_estimation_prior(Context &ctx, SurfelMap &map, const ScanView &scan, const vba_surfel_odom_params &params,
                                                  vba_odom_report *report, IMUST *x_out) {
  int ok = 0;
  check(ctx.get(), vba_odom_surfel_update_on_state(ctx.get(), s_, map.get(), scan.n, scan.pnt, &params, &ok, report, x_out ? &x_out->t : nullptr));
  return ok != 0;
}

// ---- loop closure -> local mapping (voxelba.h "Loop-closure map").  The pose algebra runs here, on the host, one
// separately rounded product and sum after the other in the order  s = a0*b0; s += a1*b1; s += a2*b2  (compile without contraction
// to keep it so); the device sees poses that are already moved.
namespace detail {
inline void mat3_mul(const double *A, const double *B, double *C) {          // C = A B, may alias neither
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double s = A[3 * r] * B[c]; s += A[3 * r + 1] * B[3 + c]; s += A[3 * r + 2] * B[6 + c]; C[3 * r + c] = s; }
}
inline void mat3_vec(const double *A, const double *v, double *o) {          // o = A v, may not alias
  for (int r = 0; r < 3; r++) { double s = A[3 * r] * v[0]; s += A[3 * r + 1] * v[1]; s += A[3 * r + 2] * v[2]; o[r] = s; }
}
}  // namespace detail

// VS:2597-2598: dx.R = x3.R x1.R^T, dx.p = x3.p - (x3.R x1.R^T) x1.p, with x1 the pose before and x3 after the optimisation
inline IMUST loop_dx(const IMUST &x1, const IMUST &x3) {
  IMUST dx;
  double Rt[9], q[3];
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rt[3 * r + c] = x1.R[3 * c + r];
  detail::mat3_mul(x3.R, Rt, dx.R);
  detail::mat3_vec(dx.R, x1.p, q);
  for (int k = 0; k < 3; k++) dx.p[k] = x3.p[k] - q[k];
  return dx;
}
// x.v = dx.R x.v; x.p = dx.R x.p + dx.p; x.R = dx.R x.R  (LR:29-34, VS:1299-1305)
inline void apply_dx(IMUST &x, const IMUST &dx) {
  double v[3], p[3], R[9];
  detail::mat3_vec(dx.R, x.v, v); detail::mat3_vec(dx.R, x.p, p); detail::mat3_mul(dx.R, x.R, R);
  for (int k = 0; k < 3; k++) { x.v[k] = v[k]; x.p[k] = p[k] + dx.p[k]; }
  std::memcpy(x.R, R, 72);
}
struct ScanPose {   // LR:17-34
  IMUST x; std::shared_ptr<PVec> pvec; double v6[6] = {0, 0, 0, 0, 0, 0};
  ScanPose(const IMUST &x_, std::shared_ptr<PVec> pvec_) : x(x_), pvec(std::move(pvec_)) {}
  void update(const IMUST &dx) { apply_dx(x, dx); }
};

// ResultOutput::pub_global_path (VS:90-108), host only: one record x y z intensity per ScanPose of every session in `ids`, in that
// order; x y z = bl->x.p narrowed to float, intensity = the session's id.  (*relc_bl_buf[id]) are session id's scan poses.
// publish(const float *xyzi, int64_t n) receives the one message.  Returns the number of records.
template <class Publish>
inline int64_t pub_global_path(const std::vector<std::vector<ScanPose *> *> &relc_bl_buf, const std::vector<int> &ids, Publish &&publish) {
  std::vector<float> pl;
  for (int id : ids)
    for (const ScanPose *bl : *relc_bl_buf.at((size_t)id)) {
      pl.push_back((float)bl->x.p[0]); pl.push_back((float)bl->x.p[1]); pl.push_back((float)bl->x.p[2]);
      pl.push_back((float)id);
    }
  publish((const float *)pl.data(), (int64_t)(pl.size() / 4));
  return (int64_t)(pl.size() / 4);
}

// `map_loop` (VS:2601-2625): a second voxel map in HBM.  Destroy it before its Context.
class LoopMap {
 public:
  explicit LoopMap(Context &ctx) : ctx_(ctx.get()) { check(ctx_, vba_loop_map_create(ctx_, &lm_)); }
  ~LoopMap() { vba_loop_map_destroy(lm_); }
  LoopMap(const LoopMap &) = delete;
  LoopMap &operator=(const LoopMap &) = delete;
  vba_loop_map *get() const { return lm_; }
  void reserve(int64_t fix_points, int64_t nodes) { check(ctx_, vba_loop_map_reserve(lm_, fix_points, nodes)); }
  // the block VS:2601-2625 from the store's last init_num keyframes at their current x0 (run KeyframeStore::set_poses first; hold
  // mtx_keyframe).  cumulative = true is the reference: pvec_tem is never cleared, keyframe 0 goes in init_num times.
  int build(KeyframeStore &keyframes, int init_num = 5, bool cumulative = true) {
    int n = 0;
    check(ctx_, vba_loop_map_build(lm_, keyframes.get(), init_num, cumulative ? 1 : 0, &n));
    return n;
  }
  size_t size() const { return (size_t)vba_loop_map_num_roots(lm_); }
 private:
  vba_ctx *ctx_ = nullptr;
  vba_loop_map *lm_ = nullptr;
};

// loop_update() on the local-mapping thread (VS:1255-1373) without its publishing code: the host part VS:1296-1331 (the
// buf_lba2loop poses, the window states with x.g while g_update == 1, x_curr) and VS:1366-1367 (g_update 1 -> 2) here, the map part
// in ONE call.  pvec_buf == nullptr re-inserts the window from the outgoing map's own scan ring (device to device); otherwise
// (*pvec_buf)[i] is the scan of frame i.
inline void loop_update_states(const IMUST &dx, std::vector<ScanPose *> &buf_lba2loop, std::vector<IMUST> &x_buf, int win_count, IMUST &x_curr,
                               int g_update) {
  if (win_count < 1 || (size_t)win_count > x_buf.size()) throw std::invalid_argument("loop_update: win_count");
  for (ScanPose *bl : buf_lba2loop) bl->update(dx);                         // VS:1286-1294
  for (int i = 0; i < win_count; i++) {                                     // VS:1296-1311
    apply_dx(x_buf[i], dx);
    if (g_update == 1) { double g[3]; detail::mat3_vec(dx.R, x_buf[i].g, g); std::memcpy(x_buf[i].g, g, 24); }
  }
  double v[3];                                                              // VS:1327-1331
  detail::mat3_vec(dx.R, x_curr.v, v);
  std::memcpy(x_curr.R, x_buf[win_count - 1].R, 72); std::memcpy(x_curr.p, x_buf[win_count - 1].p, 24);
  std::memcpy(x_curr.v, v, 24); std::memcpy(x_curr.g, x_buf[win_count - 1].g, 24);
}
inline void loop_update_finish(int &g_update) { if (g_update == 1) g_update = 2; }   // VS:1366-1367

inline int VoxelMap::loop_update(LoopMap &map_loop, const IMUST &dx, std::vector<ScanPose *> &buf_lba2loop, std::vector<IMUST> &x_buf, int win_count,
                                 IMUST &x_curr, int &g_update, const std::vector<const PVec *> *pvec_buf) {
  loop_update_states(dx, buf_lba2loop, x_buf, win_count, x_curr, g_update);
  const int k = (int)buf_lba2loop.size();
  std::vector<int> off(k + 1, 0);
  for (int i = 0; i < k; i++) off[i + 1] = off[i] + (int)buf_lba2loop[i]->pvec->size();
  std::vector<double> pnt((size_t)off[k] * 3), var((size_t)off[k] * 9), poses_bl((size_t)k * 12);
  for (int i = 0; i < k; i++) {
    std::memcpy(&poses_bl[(size_t)i * 12], buf_lba2loop[i]->x.R, 72); std::memcpy(&poses_bl[(size_t)i * 12 + 9], buf_lba2loop[i]->x.p, 24);
    size_t r = (size_t)off[i];
    for (const pointVar &pv : *buf_lba2loop[i]->pvec) { std::memcpy(&pnt[3 * r], pv.pnt, 24); std::memcpy(&var[9 * r], pv.var, 72); r++; }
  }
  std::vector<IMUST> xw(x_buf.begin(), x_buf.begin() + win_count);
  const std::vector<double> poses_win = LidarFactor::poses_of(xw);
  std::vector<int> woff;
  std::vector<double> wp, wv;
  if (pvec_buf) {
    woff.assign(win_count + 1, 0);
    for (int i = 0; i < win_count; i++) woff[i + 1] = woff[i] + (int)(*pvec_buf)[i]->size();
    wp.resize((size_t)woff[win_count] * 3 + 1); wv.resize((size_t)woff[win_count] * 9 + 1);
    size_t r = 0;
    for (int i = 0; i < win_count; i++)
      for (const pointVar &pv : *(*pvec_buf)[i]) { std::memcpy(&wp[3 * r], pv.pnt, 24); std::memcpy(&wv[9 * r], pv.var, 72); r++; }
  }
  double dx12[12];
  std::memcpy(dx12, dx.R, 72); std::memcpy(dx12 + 9, dx.p, 24);
  int nf = 0;
  check(c_, vba_loop_update(c_, map_loop.get(), dx12, k, off.data(), pnt.data(), var.data(), poses_bl.data(), win_count,
                            pvec_buf ? wp.data() : nullptr, pvec_buf ? wv.data() : nullptr, pvec_buf ? woff.data() : nullptr, poses_win.data(), &nf));
  loop_update_finish(g_update);
  return nf;
}

// ---- the marginalised scans of a session, resident in HBM (voxelba.h "Scan log"): the counterpart of the live
// ScanPose::pvec pointers.  push(map, frame) stands where the reference creates the ScanPose (VS:1974-1980), after the BA and BEFORE
// multi_margi; the number it returns is win_base + frame for a session that pushes every marginalised scan.  The producer thread
// (push) and one consumer thread (everything else) may overlap while no push has to grow the arena: reserve() first.  Destroy it
// before its Context.
class ScanLog {
 public:
  explicit ScanLog(Context &ctx) : ctx_(ctx.get()) { check(ctx_, vba_scanlog_create(ctx_, &l_)); }
  ~ScanLog() { vba_scanlog_destroy(l_); }
  ScanLog(const ScanLog &) = delete;
  ScanLog &operator=(const ScanLog &) = delete;
  vba_scanlog *get() const { return l_; }
  void reserve(int64_t points, int scans) { check(ctx_, vba_scanlog_reserve(l_, points, scans)); }
  // frame `frame` of the window, from the map's scan ring, device to device (the map must be the one of the log's Context)
  int64_t push(VoxelMap &map, int frame) {
    if (map.get() != ctx_) throw std::invalid_argument("ScanLog::push: the map belongs to another Context");
    int64_t seq = -1;
    check(ctx_, vba_scanlog_push_window(l_, frame, &seq));
    return seq;
  }
  // a scan the caller holds (offline sessions)
  int64_t push(const PVec &pvec) {
    const size_t n = pvec.size();
    std::vector<double> p(n * 3 + 1), v(n * 9 + 1);
    for (size_t i = 0; i < n; i++) { std::memcpy(&p[i * 3], pvec[i].pnt, 24); std::memcpy(&v[i * 9], pvec[i].var, 72); }
    int64_t seq = -1;
    check(ctx_, vba_scanlog_push_points(l_, (int)n, p.data(), v.data(), &seq));
    return seq;
  }
  void release(int64_t upto) { check(ctx_, vba_scanlog_release(l_, upto)); }     // pvec = nullptr for every scan below upto
  int64_t first() const { int64_t a = 0, b = 0; check(ctx_, vba_scanlog_range(l_, &a, &b, 0, nullptr)); return a; }
  int64_t end() const { int64_t a = 0, b = 0; check(ctx_, vba_scanlog_range(l_, &a, &b, 0, nullptr)); return b; }
  int size(int64_t seq) const {
    int n = 0;
    check(ctx_, vba_scanlog_read(l_, seq, 0, nullptr, nullptr, nullptr, &n));
    return n;
  }
  // scan seq on the host: the PVec as it was inserted, and / or its points narrowed to float on the device (pl_save, VS:172-174)
  void read(int64_t seq, PVec *pvec, std::vector<XYZ> *xyz = nullptr) const {
    const int n = size(seq);
    std::vector<double> p(pvec ? (size_t)n * 3 + 1 : 0), v(pvec ? (size_t)n * 9 + 1 : 0);
    std::vector<float> f(xyz ? (size_t)n * 3 + 1 : 0);
    int m = 0;
    check(ctx_, vba_scanlog_read(l_, seq, n, pvec ? p.data() : nullptr, pvec ? v.data() : nullptr, xyz ? f.data() : nullptr, &m));
    if (m < n) throw std::runtime_error("ScanLog::read: the scan changed under the reader");
    if (pvec) {
      pvec->resize((size_t)n);
      for (int i = 0; i < n; i++) { std::memcpy((*pvec)[i].pnt, &p[3 * (size_t)i], 24); std::memcpy((*pvec)[i].var, &v[9 * (size_t)i], 72); }
    }
    if (xyz) {
      xyz->resize((size_t)n);
      for (int i = 0; i < n; i++) (*xyz)[i] = XYZ{f[3 * (size_t)i], f[3 * (size_t)i + 1], f[3 * (size_t)i + 2]};
    }
  }
 private:
  vba_ctx *ctx_ = nullptr;
  vba_scanlog *l_ = nullptr;
};

inline int KeyframeStore::build(ScanLog &log, int64_t first, const std::vector<IMUST> &bl_poses, double voxel_size_10, int id, double jour,
                                BtcDatabase *db, std::vector<STD> *stds_vec) {
  const std::vector<double> poses = LidarFactor::poses_of(bl_poses);
  const int cap = db ? db->gen_cap() : 0;
  std::vector<double> rows((size_t)(cap > 0 ? cap : 1) * VBA_BTC_ROW_LEN);
  std::vector<uint64_t> bits((size_t)(cap > 0 ? cap : 1) * 3);
  int n = 0, kept = 0;
  check(ctx_, vba_kf_build_from_log(s_, log.get(), first, (int)bl_poses.size(), poses.data(), voxel_size_10, id, jour, db ? db->get() : nullptr, cap,
                                    rows.data(), bits.data(), &n, &kept));
  if (db && stds_vec) unpack_stds(rows, bits, n, *stds_vec);
  return kept;
}

inline int VoxelMap::loop_update(LoopMap &map_loop, const IMUST &dx, ScanLog &log, int64_t first, std::vector<IMUST> &bl_states, std::vector<IMUST> &x_buf,
                                 int win_count, IMUST &x_curr, int &g_update) {
  std::vector<ScanPose *> none;
  loop_update_states(dx, none, x_buf, win_count, x_curr, g_update);
  for (IMUST &x : bl_states) apply_dx(x, dx);                                   // ScanPose::update, VS:1286-1294
  const std::vector<double> poses_bl = LidarFactor::poses_of(bl_states);
  std::vector<IMUST> xw(x_buf.begin(), x_buf.begin() + win_count);
  const std::vector<double> poses_win = LidarFactor::poses_of(xw);
  double dx12[12];
  std::memcpy(dx12, dx.R, 72); std::memcpy(dx12 + 9, dx.p, 24);
  int nf = 0;
  check(c_, vba_scanlog_loop_update(c_, map_loop.get(), dx12, log.get(), first, (int)bl_states.size(), poses_bl.data(), win_count, poses_win.data(), &nf));
  loop_update_finish(g_update);
  return nf;
}

// ResultOutput::pub_localmap's point loop (VS:63-76) from the log: the mgsize scans first .. first + mgsize - 1 (the outgoing frames,
// pushed before multi_margi) at x_buf[0 .. mgsize), every third point, intensity = cur_session; publish(const float *xyzi, int64_t n)
// receives the records x y z intensity.  The path update VS:78-84 reads x_buf alone and stays with the caller.
template <class Publish>
inline int64_t pub_localmap(Context &ctx, ScanLog &log, int64_t first, int mgsize, const std::vector<IMUST> &x_buf, int cur_session, Publish &&publish,
                            int stride = 3) {
  if (mgsize < 0 || (size_t)mgsize > x_buf.size()) throw std::invalid_argument("pub_localmap: mgsize");
  std::vector<IMUST> xs(x_buf.begin(), x_buf.begin() + mgsize);
  const std::vector<double> poses = LidarFactor::poses_of(xs);
  int64_t cap = 0, n = 0;
  for (int i = 0; i < mgsize; i++) cap += (log.size(first + i) + stride - 1) / stride;
  std::vector<float> pl((size_t)cap * 4 + 4);
  check(ctx.get(), vba_scanlog_export_world(ctx.get(), log.get(), first, mgsize, poses.data(), stride, (float)cur_session, cap, pl.data(), &n));
  publish((const float *)pl.data(), n);
  return n;
}

// The live local map for display, shaped like pub_localmap: what OctoTree::tras_display (VM:1765-1827) collects for /map_wind and
// what the /avoxel marker of rviz_cfg/back_voxel.rviz shows.  publish_points(const float *xyzi, int64_t n) receives the records
// x y z intensity (intensity = the frame's index in the window), publish_planes(const float *planes, const long long *keys, int64_t m)
// the plane records [m][16] and their keys [m][5] (voxelba.h, vba_map_display).  Returns the number of points.
template <class PublishPoints, class PublishPlanes>
inline int64_t pub_voxelmap(VoxelMap &vmap, int win_count, const std::vector<IMUST> &x_buf, PublishPoints &&publish_points, PublishPlanes &&publish_planes) {
  const VoxelMap::Display d = vmap.display(win_count, x_buf, 0);
  publish_points((const float *)d.xyzi.data(), d.n_points());
  publish_planes((const float *)d.planes.data(), (const long long *)d.plane_key.data(), d.n_planes());
  return d.n_points();
}

// FileReaderWriter::save_pcd (VS:166-179) of scan seq: savename/seq.pcd from the float form read off the device
inline void save_pcd(ScanLog &log, int64_t seq, const std::string &savename) {
  std::vector<XYZ> xyz;
  log.read(seq, nullptr, &xyz);
  std::vector<double> p(xyz.size() * 3 + 1);
  for (size_t i = 0; i < xyz.size(); i++) { p[3 * i] = xyz[i].x; p[3 * i + 1] = xyz[i].y; p[3 * i + 2] = xyz[i].z; }
  const std::string path = savename + "/" + std::to_string(seq) + ".pcd";
  if (vba_io_save_pcd(path.c_str(), (int)xyz.size(), p.data())) throw std::runtime_error("save_pcd: " + path);
}

#ifdef VBA_ADAPTER_HAVE_EIGEN
// Eigen-typed conveniences so reference call sites keep their argument types (Eigen is column-major: converted here).
inline void to_rowmajor3(const Eigen::Matrix3d &M, double *r) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r[3 * i + j] = M(i, j); }
inline Eigen::MatrixXd to_eigen(const std::vector<double> &h, int n) {
  Eigen::MatrixXd M(n, n);
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) M(i, j) = h[(size_t)i * n + j];
  return M;
}
#endif

}  // namespace vba
