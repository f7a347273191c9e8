// C++ harness that drives libvoxelba.so through include/voxelba_adapter.hpp in the call order of the reference's
// thd_odometry_localmapping (voxelslam.cpp:1899-1927 and 1951-2043): the class names and call sites below are the
// reference's (LidarFactor voxhess; cut_voxel_multi; multi_recut; LI_BA_Optimizer::damping_iter; multi_margi; the mp[]
// rotation; the x_buf / pvec_buf / imu_pre_buf slide) with the ROS / PCL / Eigen containers replaced by the adapter's
// plain-array ones.  Input and output are flat files of doubles written / read by tests/test_gpu_harness.py, which runs
// the same sequence on the CPU oracle and compares.
//
//   input : [magic 20241004, win_size, n_scans, mode (0 lidar-only | 1 LI | 2 LI + gravity on the first full window),
//            voxel_size, max_layer, max_points, min_eigen_value, plane_thre[4], min_point[4], imu_coef, thread_num]
//           per scan : [n, x_curr (25 state doubles), x_curr.cov (225), n_imu] points[n][3] var_body[n][9]
//                      imu samples of the interval BEFORE this scan: t[n_imu] gyr[n_imu][3] acc[n_imu][3]
//           noise_meas[6] noise_walk[6]
//   mode 3 (motion_init, VS:1524, then the steady-state loop of mode 1): after the header an initialisation block
//           [point_notime, dept_err, beam_err, scale_gravity, extrin_para R(9) p(3)]
//           per scan of the first win_size : [n, n_imu, beg_time, x_buf state (25), cov (225)] pnt[n][3] curvature[n] imu[n_imu][7]
//           then the remaining n_scans - win_size scans in the per-scan layout above (their IMU samples use scale_gravity);
//           output starts with [-2, converge_flag, iterations, thresholds_left_relaxed, eigvalue(3), W x 25 states], then as above
//           (the first window record is the initialised window's step, VS:1951 reached with win_count = win_size)
//   mode 4 (loop detection, VS:2404-2541, through vba::BtcDatabase / vba::icp_normal): the header is only
//           [magic, 0, n_keyframes, 4, is_high_fly, icp_eigval, n_sessions, juds[n_sessions]], then per keyframe
//           [session, n_desc, n_pts] rows[n_desc][19] bits[n_desc][3] (occupancy masks as doubles, < 2^53) cloud[n_pts][6];
//           sessions come in order; a new session closes the previous one (skip_near_num_ = -(clouds + 10), VS:2242).
//           output per keyframe and per session id <= cur: [cur session, keyframe, id, loop_id, score, icp_ran, icp_ok, iters,
//           t(3), R(9), eig(3)] (23 doubles; the pose is the ICP result when icp_ran, else SearchLoop's transform)
//   mode 5 (the same step with descriptor generation, VS:2404-2541: GenerateSTDescs -> SearchLoop over sessions -> icp_normal ->
//           AddSTDescs, through vba::BtcDatabase::GenerateSTDescs): the header of mode 4 with mode 5, then per keyframe
//           [session, n_pts] cloud[n_pts][3] (the keyframe's merged cloud); GenerateSTDescs gets id = the keyframe's index in its
//           session; output as mode 4
//   mode 6 (pose-graph optimisation, build_graph VS:2078-2156 + topDownProcess VS:2717-2812 + ISAM2, through vba::PoseGraph):
//           header [magic, 0, n_sessions, 6, lpedge_enable, n_updates, relin_threshold], per session [n_scans] states[n][25] v6[n][6],
//           then [n_loop] rows [m1, m2, id1, id2, rot(9), tra(3)] (noise v6_init = 1e-4), then [n_gba] rows [m1, m2, id1, id2, rot(9),
//           tra(3), v6(6)] (gba_edges1 + gba_edges2 with scan ids); output: the states of every session after set_state, then the
//           stats [n_updates][3]
//   mode 7 (a loop closure carried back into local mapping, VS:2582-2625 + loop_update() VS:1255-1373, through vba::KeyframeStore,
//           vba::LoopMap and vba::VoxelMap::loop_update): the lidar-only session of mode 0 with [n_loop, kf_every, dx(12)] after the
//           header.  Every marginalised scan joins buf_lba2loop with its refined pose; every kf_every of them become a keyframe
//           (KeyframeStore::build at voxel_size / 10).  Before scan n_loop is read: set_poses with the keyframes' x0 moved by dx,
//           LoopMap::build, loop_update (window from the outgoing map's scan ring), and every later x_curr of the input is moved by
//           dx.  (The device formed the scans' world covariances when it inserted them; buf_lba2loop keeps the covariances of the
//           input, which is what both sides of the test use for the marginalised scans.)  The record written at that point:
//           [-3, points inserted by the build, factor count, n_kf, per keyframe {n, x0(12), xyz[n][3], diag[n][3]},
//            k, per buf_lba2loop scan {scan index, state(25)}, win_count, per frame {state(25)}]
//   mode 9 (mode 7 with the marginalised scans resident in HBM, DESIGN.md §20, through vba::ScanLog): input and output layouts are
//           mode 7's.  A vba::ScanLog takes the place of the host ScanPose::pvec: the outgoing frame is pushed from the map's scan
//           ring before multi_margi, keyframes are built from the log (KeyframeStore::build(ScanLog&, ...)) and released after each
//           build, loop_update takes the buf_lba2loop scans from the log.  (The log holds the map's world covariances, mode 7's host
//           route the covariances of the input: the keyframes' diag rows and what derives from them differ between the two modes.)
//   mode 8 (the initialisation window resident in HBM, VS:1450-1534 through vba::ScanFrame::decode, vba::InitWindow::push and the
//           InitWindow overload of motion_init): the header and the initialisation block of mode 3 with n_scans = win_size,
//           then [down_size, min_points, point_filter_num, blind, layout (point_step, off_x, off_y, off_z, off_intensity, intensity_type,
//           off_time, time_type, filter)], per scan [n_raw, n_words, n_imu, beg_time, x_buf state (25), cov (225)] then the raw message in
//           n_words doubles (its bytes, padded) and imu[n_imu][7]; output: the initialisation record of mode 3, then per scan
//           [points kept, retried], then the final map as below
//   mode 10 (mode 8 with the window's states PRODUCED by the initialisation odometry on a vba::OdomState, VS:1450-1534):
//           the header and the blocks of mode 8 up to the layout, then ekf noise [12] (cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc),
//           x_curr state (25) and cov (225) before the first scan, per scan [n_raw, n_words, n_imu, last_pcl_end_time, pcl_beg_time,
//           pcl_end_time] then the raw message and imu[n_imu][7].  Per scan: OdomState::propagate, OdomState::prepare at
//           max(down_size, 0.5) with min_points 0, OdomState::lio_state_estimation_kdtree (x_out -> x_buf), vba::pub_localtraj,
//           IMU_PRE::push_imu, InitWindow::push; then the InitWindow overload of motion_init and OdomState::set(x_buf.back()).
//           output: the initialisation record of mode 3 (converge_flag is recorded, not required), then per scan [iterations,
//           state (25), points kept, retried, records published, sum of their float bits as integers], then the final map as below
//   output: per optimised window [scan index, W x 25 states, v6[6]] ... then [-1, n_leaves] leaf dump [n][39] plane_var dump [n][86]
#include "../../include/voxelba_adapter.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <vector>

using namespace vba;

static std::vector<double> read_all(const char *path) {
  FILE *f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "harness: cannot open %s\n", path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> v((size_t)bytes / 8);
  if (std::fread(v.data(), 8, v.size(), f) != v.size()) { std::fprintf(stderr, "harness: short read\n"); std::exit(2); }
  std::fclose(f);
  return v;
}

// VS:2404-2541 over a multi-session stream: push the keyframe's plane cloud, SearchLoop against every session (one batched call),
// icp_normal where score > juds[id], AddSTDescs; a new session closes the previous database
static int run_loop_detection(const std::vector<double> &in, size_t q, int n_kf, const char *out_path, bool generate) {
  auto next = [&]() { return in.at(q++); };
  const int is_high_fly = (int)next();
  const double icp_eigval = next();
  const int n_sessions = (int)next();
  std::vector<double> juds(n_sessions);
  for (double &j : juds) j = next();
  vba_options opt;
  vba_default_options(&opt);
  opt.device = 0;
  std::vector<double> out;
  {
    Context ctx(opt);
    vba_btc_config cfg;
    vba_btc_default_config(is_high_fly, &cfg);
    vba_btc_gen_config gcfg;
    vba_btc_default_gen_config(is_high_fly, &gcfg);
    std::vector<std::unique_ptr<BtcDatabase>> managers;
    int cur_session = -1, kf_in_session = 0;
    for (int k = 0; k < n_kf; k++) {
      const int session = (int)next(), nd = generate ? 0 : (int)next(), np = (int)next();
      if (session != cur_session) {
        if (!managers.empty()) managers.back()->config_setting_.skip_near_num_ = -(managers.back()->plane_cloud_num() + 10);   // VS:2242
        managers.emplace_back(new BtcDatabase(ctx, cfg, &gcfg));
        cur_session = session; kf_in_session = 0;
      }
      BtcDatabase &cur = *managers.back();
      std::vector<STD> stds(nd);
      for (int i = 0; i < nd; i++) {
        STD &d = stds[i];
        double r[19];
        for (int u = 0; u < 19; u++) r[u] = next();
        BinaryDescriptor *b[3] = {&d.binary_A_, &d.binary_B_, &d.binary_C_};
        for (int u = 0; u < 3; u++) { d.triangle_[u] = r[u]; d.center_[u] = r[3 + u]; }
        d.frame_number_ = (int)r[6];
        for (int e = 0; e < 3; e++) { for (int u = 0; u < 3; u++) b[e]->location_[u] = r[7 + 3 * e + u]; b[e]->summary_ = (unsigned char)r[16 + e]; }
      }
      for (int i = 0; i < nd; i++) {
        stds[i].binary_A_.occupy_bits = (uint64_t)next(); stds[i].binary_B_.occupy_bits = (uint64_t)next(); stds[i].binary_C_.occupy_bits = (uint64_t)next();
      }
      if (generate) {
        std::vector<float> xyz((size_t)np * 3);
        for (float &f : xyz) f = (float)next();
        cur.GenerateSTDescs(xyz, stds, kf_in_session);                                     // VS:2406
      } else {
        std::vector<float> cloud((size_t)np * 6);
        for (float &f : cloud) f = (float)next();
        cur.push_plane_cloud(cloud, kf_in_session);                                        // GenerateSTDescs' push (BTC.cpp:164-165)
      }
      const int last = cur.plane_cloud_num() - 1;
      std::vector<BtcDatabase *> dbs;
      for (auto &m : managers) dbs.push_back(m.get());
      std::vector<vba_btc_result> res;
      BtcDatabase::search_loop_sessions(dbs, stds, cur, last, res);                          // VS:2417-2421
      for (size_t id = 0; id < dbs.size(); id++) {
        LoopTransform pose;
        std::memcpy(pose.t, res[id].t, 24); std::memcpy(pose.R, res[id].R, 72);
        double eig[3] = {0, 0, 0};
        int iters = 0, ran = 0, ok = 0;
        if (res[id].loop_id >= 0 && res[id].score > juds[id]) {                              // VS:2431-2434
          ran = 1;
          ok = icp_normal(cur, last, *dbs[id], res[id].loop_id, pose, icp_eigval, eig, &iters) ? 1 : 0;
        }
        const double rec[8] = {(double)session, (double)kf_in_session, (double)id, (double)res[id].loop_id, res[id].score, (double)ran, (double)ok, (double)iters};
        out.insert(out.end(), rec, rec + 8);
        out.insert(out.end(), pose.t, pose.t + 3);
        out.insert(out.end(), pose.R, pose.R + 9);
        out.insert(out.end(), eig, eig + 3);
      }
      cur.AddSTDescs(stds);                                                                  // VS:2541
      kf_in_session++;
    }
  }
  FILE *f = std::fopen(out_path, "wb");
  if (!f) return 2;
  std::fwrite(out.data(), 8, out.size(), f);
  std::fclose(f);
  return 0;
}

// build_graph (VS:2078-2156) over all sessions (ids = 0..n_sessions-1, stepsizes from their sizes), the gba_edges of
// topDownProcess (VS:2733-2764), ISAM2 (VS:2766-2773) and the set_state write-back (VS:2778-2786)
static int run_pose_graph(const std::vector<double> &in, size_t q, int n_sessions, const char *out_path) {
  auto next = [&]() { return in.at(q++); };
  const int lpedge_enable = (int)next(), n_updates = (int)next();
  const double relin = next();
  std::vector<std::vector<ScanPoseRec>> scans(n_sessions);
  std::vector<int> stepsizes(1, 0);
  for (int s = 0; s < n_sessions; s++) {
    const int n = (int)next();
    scans[s].resize(n);
    for (int k = 0; k < n; k++) { double *st = &scans[s][k].x.t; for (int f = 0; f < VBA_STATE_LEN; f++) st[f] = next(); }
    for (int k = 0; k < n; k++) for (int f = 0; f < 6; f++) scans[s][k].v6[f] = next();
    stepsizes.push_back(stepsizes.back() + n);
  }
  vba_options opt;
  vba_default_options(&opt);
  std::vector<double> out;
  try {
    Context ctx(opt);
    PoseGraph graph;
    for (int ii = 0; ii < n_sessions; ii++) {                          // VS:2099-2118
      const int bsize = stepsizes[ii];
      for (int j = bsize; j < stepsizes[ii + 1]; j++) {
        graph.insert(j, scans[ii][j - bsize].x);
        if (j > bsize) graph.add_edge(j - 1, j, scans[ii][j - 1 - bsize].x, scans[ii][j - bsize].x, scans[ii][j - 1 - bsize].v6);
      }
    }
    if (n_sessions > 0 && !scans[0].empty()) {                          // VS:2121-2134
      const double v6_fixd[6] = {1e-9, 1e-9, 1e-9, 1e-9, 1e-9, 1e-9};
      graph.add_prior(0, scans[0][0].x, v6_fixd);
    }
    const int n_loop = (int)next();
    const double v6_init[6] = {1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4};
    for (int e = 0; e < n_loop; e++) {                                 // VS:2137-2154 (default_noise)
      double r[16];
      for (int f = 0; f < 16; f++) r[f] = next();
      if (lpedge_enable == 1) graph.add_edge(stepsizes[(int)r[0]] + (int)r[2], stepsizes[(int)r[1]] + (int)r[3], r + 4, r + 13, v6_init);
    }
    const int n_gba = (int)next();
    for (int e = 0; e < n_gba; e++) {                                  // VS:2733-2764
      double r[22];
      for (int f = 0; f < 22; f++) r[f] = next();
      graph.add_edge(stepsizes[(int)r[0]] + (int)r[2], stepsizes[(int)r[1]] + (int)r[3], r + 4, r + 13, r + 16);
    }
    graph.optimize(ctx, n_updates, relin);                             // VS:2766-2773
    for (int ii = 0; ii < n_sessions; ii++)                            // VS:2778-2786
      for (int j = stepsizes[ii]; j < stepsizes[ii + 1]; j++) {
        IMUST &x = scans[ii][j - stepsizes[ii]].x;
        set_state(x, graph.pose(j));
        const double *st = &x.t;
        out.insert(out.end(), st, st + VBA_STATE_LEN);
      }
    out.insert(out.end(), graph.stats.begin(), graph.stats.end());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "harness: %s\n", e.what());
    return 1;
  }
  FILE *f = std::fopen(out_path, "wb");
  if (!f) return 2;
  std::fwrite(out.data(), 8, out.size(), f);
  std::fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  // optional third argument --deterministic: vba_options::deterministic = 1 (bit-identical output run to run)
  const bool det = argc == 4 && std::strcmp(argv[3], "--deterministic") == 0;
  if (argc < 3 || (argc == 4 && !det) || argc > 4) { std::fprintf(stderr, "usage: %s <input.bin> <output.bin> [--deterministic]\n", argv[0]); return 2; }
  const std::vector<double> in = read_all(argv[1]);
  size_t q = 0;
  auto next = [&]() { return in.at(q++); };
  if (next() != 20241004.0) { std::fprintf(stderr, "harness: bad magic\n"); return 2; }
  const int win_size = (int)next(), n_scans = (int)next(), mode = (int)next();
  if (mode == 4 || mode == 5) return run_loop_detection(in, q, n_scans, argv[2], mode == 5);
  if (mode == 6) return run_pose_graph(in, q, n_scans, argv[2]);
  vba_options opt;
  vba_default_options(&opt);
  opt.win_size = win_size;
  opt.voxel_size = next(); opt.max_layer = (int)next(); opt.max_points = (int)next(); opt.min_eigen_value = next();
  for (int i = 0; i < 4; i++) opt.plane_eigen_value_thre[i] = next();
  for (int i = 0; i < 4; i++) opt.min_point[i] = next();
  opt.imu_coef = next(); opt.thread_num = (int)next();
  opt.deterministic = det ? 1 : 0;
  const bool loop_mode = mode == 7 || mode == 9, use_log = mode == 9;
  const bool lidar_only = mode == 0 || loop_mode;
  int n_loop = -1, kf_every = 1;
  IMUST dx;
  if (loop_mode) {
    n_loop = (int)next(); kf_every = (int)next();
    for (int i = 0; i < 9; i++) dx.R[i] = next();
    for (int i = 0; i < 3; i++) dx.p[i] = next();
  }

  std::vector<double> out;
  try {
    Context ctx(opt);
    VoxelMap surf_map(ctx);                      // surf_map + surf_map_slide
    LidarFactor voxhess(ctx, win_size);          // VS:1758
    std::vector<IMUST> x_buf;                    // VS:1760
    std::vector<std::shared_ptr<PVec>> pvec_buf;
    std::deque<IMU_PRE *> imu_pre_buf;
    std::vector<double> hess;                    // Eigen::MatrixXd hess (VS:1762)
    int win_count = 0, win_base = 0, g_update = (mode == 2) ? 2 : 0;
    const int mgsize = 1, DIM = VBA_DIM;
    double jour = 0;
    // the noise globals of preintegration.hpp:8-9 travel at the end of the file
    const double *noise = &in[in.size() - 12];
    double scale_gravity = 1.0;                  // imupre_scale_gravity (PI:9)
    // mode 7: keyframes, map_loop and the scans marginalised since the last keyframe (buf_lba2loop) with their scan indices
    std::unique_ptr<KeyframeStore> keyframes;
    std::unique_ptr<LoopMap> map_loop;
    std::vector<std::unique_ptr<ScanPose>> buf_lba2loop;
    std::vector<int> bl_index;
    std::vector<IMUST> kf_x0;
    std::vector<int> scan_of_frame;              // scan index of every frame of the window
    bool moved = false;
    if (loop_mode) { keyframes.reset(new KeyframeStore(ctx)); map_loop.reset(new LoopMap(ctx)); }
    // mode 9: the same scans in a ScanLog; bl_states are their ScanPose::x, scan bl_first of the log is the first of them
    std::unique_ptr<ScanLog> scan_log;
    std::vector<IMUST> bl_states;
    int64_t bl_first = 0;
    if (use_log) scan_log.reset(new ScanLog(ctx));

    // VS:1951-2043: optimise the full window, then marginalise and slide
    auto window_step = [&](int k) {
        if (lidar_only) {                                        // lidar-only windows (what HBA_add_edge runs, VS:2895-2899)
          Lidar_BA_Optimizer opt_lsv;
          std::vector<double> resis;
          opt_lsv.damping_iter(x_buf, voxhess, &hess, resis, 3);
        } else if (g_update == 2) {                              // VS:1955-1964
          LI_BA_OptimizerGravity opt_lsv;
          std::vector<double> resis;
          opt_lsv.damping_iter(x_buf, voxhess, imu_pre_buf, resis, &hess, 5);
          g_update = 0;
        } else {                                                 // VS:1967-1970
          LI_BA_Optimizer opt_lsv;
          opt_lsv.damping_iter(x_buf, voxhess, imu_pre_buf, &hess);
        }
        // VS:1973-1977: v6 = 1 / |diag(hess.block<6,6>(0, DIM))|
        const int nh = lidar_only ? 6 * win_size : DIM * win_size + ((int)hess.size() == (DIM * win_size + 3) * (DIM * win_size + 3) ? 3 : 0);
        const int col0 = lidar_only ? 6 : DIM;
        double v6[6];
        for (int i = 0; i < 6; i++) v6[i] = 1.0 / std::fabs(hess[(size_t)i * nh + col0 + i]);
        out.push_back((double)k);
        for (int i = 0; i < win_size; i++) out.insert(out.end(), &x_buf[i].t, &x_buf[i].t + 25);
        out.insert(out.end(), v6, v6 + 6);

        if (use_log && scan_log->push(surf_map, 0) != win_base)  // VS:1974-1980: where the ScanPose is created, before the margi
          throw std::runtime_error("mode 9: the scan's number is not win_base");
        surf_map.multi_margi(jour, win_count, x_buf);            // VS:1991
        jour += 0.1;
        surf_map.slide(mgsize);                                  // mp[] rotation VS:2014-2019
        if (use_log) {                                           // VS:2001-2010 and VS:2354-2397 with the scans in the log
          bl_states.push_back(x_buf[0]);
          bl_index.push_back(scan_of_frame[0]);
          scan_of_frame.erase(scan_of_frame.begin());
          if ((int)bl_states.size() >= kf_every) {
            const std::vector<IMUST> bl_local(bl_states.begin(), bl_states.begin() + kf_every);
            keyframes->build(*scan_log, bl_first, bl_local, opt.voxel_size / 10, keyframes->size(), jour);
            kf_x0.push_back(bl_local.back());
            bl_states.erase(bl_states.begin(), bl_states.begin() + kf_every);
            bl_index.erase(bl_index.begin(), bl_index.begin() + kf_every);
            bl_first += kf_every;
            scan_log->release(bl_first);                           // pvec = nullptr, VS:2375
          }
        }
        if (mode == 7) {                                         // VS:2001-2010: the marginalised scan goes to the loop-closure thread
          buf_lba2loop.emplace_back(new ScanPose(x_buf[0], pvec_buf[0]));
          bl_index.push_back(scan_of_frame[0]);
          scan_of_frame.erase(scan_of_frame.begin());
          if ((int)buf_lba2loop.size() >= kf_every) {            // VS:2354-2397
            std::vector<ScanPoseRef> bl_local;
            for (int i = 0; i < kf_every; i++) bl_local.push_back(ScanPoseRef{&buf_lba2loop[i]->x, buf_lba2loop[i]->pvec.get()});
            keyframes->build(bl_local, opt.voxel_size / 10, keyframes->size(), jour);
            kf_x0.push_back(buf_lba2loop[kf_every - 1]->x);
            buf_lba2loop.erase(buf_lba2loop.begin(), buf_lba2loop.begin() + kf_every);
            bl_index.erase(bl_index.begin(), bl_index.begin() + kf_every);
          }
        }
        for (int i = mgsize; i < win_count; i++) {               // VS:2022-2028
          x_buf[i - mgsize] = x_buf[i];
          std::swap(pvec_buf[i - mgsize], pvec_buf[i]);
        }
        for (int i = win_count - mgsize; i < win_count; i++) {   // VS:2031-2038
          x_buf.pop_back();
          pvec_buf.pop_back();
          delete imu_pre_buf.front();
          imu_pre_buf.pop_front();
        }
        win_base += mgsize;
        win_count -= mgsize;
    };

    int k_first = 0;
    if (mode == 3) {                                             // VS:1450-1534: the window the initialisation collected
      Initialization init;
      init.point_notime = (int)next(); init.dept_err = next(); init.beam_err = next(); init.scale_gravity = scale_gravity = next();
      std::memcpy(init.noise_meas, noise, 48); std::memcpy(init.noise_walk, noise + 6, 48);
      IMUST extrin_para;
      for (int i = 0; i < 9; i++) extrin_para.R[i] = next();
      for (int i = 0; i < 3; i++) extrin_para.p[i] = next();
      std::vector<std::vector<PointXYZC>> pl_origs(win_size);
      std::vector<std::vector<ImuSample>> vec_imus(win_size);
      std::vector<double> beg_times(win_size);
      for (int i = 0; i < win_size; i++) {
        const int n = (int)next(), n_imu = (int)next();
        beg_times[i] = next();
        IMUST x;
        std::memcpy(&x.t, &in.at(q), 25 * sizeof(double)); q += 25;
        std::memcpy(x.cov, &in.at(q), 225 * sizeof(double)); q += 225;
        x_buf.push_back(x);
        pl_origs[i].resize((size_t)n);
        for (int j = 0; j < n; j++) { pl_origs[i][j].x = (float)next(); pl_origs[i][j].y = (float)next(); pl_origs[i][j].z = (float)next(); }
        for (int j = 0; j < n; j++) pl_origs[i][j].curvature = (float)next();
        vec_imus[i].resize((size_t)n_imu);
        for (int j = 0; j < n_imu; j++) { std::memcpy(&vec_imus[i][j], &in.at(q), 7 * sizeof(double)); q += 7; }
      }
      for (int i = 1; i < win_size; i++) {                       // imu_pre_buf as the accumulation leaves it (VS:1505-1509)
        std::vector<double> t, g, a;
        for (const ImuSample &m : vec_imus[i]) { t.push_back(m.t); g.insert(g.end(), m.gyr, m.gyr + 3); a.insert(a.end(), m.acc, m.acc + 3); }
        imu_pre_buf.push_back(new IMU_PRE(x_buf[i - 1].bg, x_buf[i - 1].ba));
        imu_pre_buf.back()->push_imu((int)t.size(), t.data(), g.data(), a.data(), noise, noise + 6, scale_gravity);
      }
      IMUST x_curr;
      const int ok = init.motion_init(pl_origs, vec_imus, beg_times, &hess, voxhess, x_buf, surf_map, pvec_buf, win_size, x_curr, imu_pre_buf,
                                      extrin_para);
      out.push_back(-2.0); out.push_back(ok); out.push_back(init.iterations); out.push_back(init.thresholds_left_relaxed);
      out.insert(out.end(), init.eigvalue, init.eigvalue + 3);
      for (int i = 0; i < win_size; i++) out.insert(out.end(), &x_buf[i].t, &x_buf[i].t + 25);
      if (!ok) throw std::runtime_error("motion_init did not converge");
      win_count = win_size;
      window_step(win_size - 1);                                 // VS:1951 with the initialised window
      k_first = win_size;
    }

    if (mode == 8) {                                             // the same window, collected on the device (VS:1458, VS:1499-1516)
      Initialization init;
      init.point_notime = (int)next(); init.dept_err = next(); init.beam_err = next(); init.scale_gravity = scale_gravity = next();
      std::memcpy(init.noise_meas, noise, 48); std::memcpy(init.noise_walk, noise + 6, 48);
      IMUST extrin_para;
      for (int i = 0; i < 9; i++) extrin_para.R[i] = next();
      for (int i = 0; i < 3; i++) extrin_para.p[i] = next();
      const double down_size = next();
      const int min_points = (int)next(), point_filter_num = (int)next();
      const double blind = next();
      vba_scan_layout layout;
      layout.point_step = (int)next(); layout.off_x = (int)next(); layout.off_y = (int)next(); layout.off_z = (int)next();
      layout.off_intensity = (int)next(); layout.intensity_type = (int)next(); layout.off_time = (int)next(); layout.time_type = (int)next();
      layout.filter = (int)next();
      ScanFrame frame(ctx);
      InitWindow pl_origs(ctx);
      std::vector<std::vector<ImuSample>> vec_imus(win_size);
      std::vector<double> beg_times(win_size), kept;
      for (int i = 0; i < win_size; i++) {
        const int n_raw = (int)next();
        const size_t n_words = (size_t)next();
        const int n_imu = (int)next();
        beg_times[i] = next();
        IMUST x;
        std::memcpy(&x.t, &in.at(q), 25 * sizeof(double)); q += 25;
        std::memcpy(x.cov, &in.at(q), 225 * sizeof(double)); q += 225;
        x_buf.push_back(x);
        if (n_raw < 0 || (size_t)n_raw * (size_t)layout.point_step > n_words * 8 || q + n_words > in.size())
          throw std::runtime_error("mode 8: the raw message does not fit its words");
        frame.decode(n_words ? &in[q] : nullptr, n_raw, layout, point_filter_num, blind);     // pcl_handler; `orig` = its cloud (VS:1458)
        q += n_words;
        bool retried = false;
        kept.push_back(pl_origs.push(frame, down_size, min_points, &retried));                // VS:1499-1512
        kept.push_back(retried ? 1.0 : 0.0);
        vec_imus[i].resize((size_t)n_imu);
        for (int j = 0; j < n_imu; j++) { std::memcpy(&vec_imus[i][j], &in.at(q), 7 * sizeof(double)); q += 7; }
      }
      for (int i = 1; i < win_size; i++) {
        std::vector<double> t, g, a;
        for (const ImuSample &m : vec_imus[i]) { t.push_back(m.t); g.insert(g.end(), m.gyr, m.gyr + 3); a.insert(a.end(), m.acc, m.acc + 3); }
        imu_pre_buf.push_back(new IMU_PRE(x_buf[i - 1].bg, x_buf[i - 1].ba));
        imu_pre_buf.back()->push_imu((int)t.size(), t.data(), g.data(), a.data(), noise, noise + 6, scale_gravity);
      }
      IMUST x_curr;
      const int ok = init.motion_init(pl_origs, vec_imus, beg_times, &hess, voxhess, x_buf, surf_map, pvec_buf, win_size, x_curr, imu_pre_buf,
                                      extrin_para);
      out.push_back(-2.0); out.push_back(ok); out.push_back(init.iterations); out.push_back(init.thresholds_left_relaxed);
      out.insert(out.end(), init.eigvalue, init.eigvalue + 3);
      for (int i = 0; i < win_size; i++) out.insert(out.end(), &x_buf[i].t, &x_buf[i].t + 25);
      out.insert(out.end(), kept.begin(), kept.end());
      k_first = n_scans;                                         // the steady-state continuation is mode 3's
    }

    if (mode == 10) {                                            // initialization() per scan on a state object (VS:1450-1534)
      Initialization init;
      init.point_notime = (int)next(); init.dept_err = next(); init.beam_err = next(); init.scale_gravity = scale_gravity = next();
      std::memcpy(init.noise_meas, noise, 48); std::memcpy(init.noise_walk, noise + 6, 48);
      IMUST extrin_para;
      for (int i = 0; i < 9; i++) extrin_para.R[i] = next();
      for (int i = 0; i < 3; i++) extrin_para.p[i] = next();
      const double down_size = next();
      const int min_points = (int)next(), point_filter_num = (int)next();
      const double blind = next();
      vba_scan_layout layout;
      layout.point_step = (int)next(); layout.off_x = (int)next(); layout.off_y = (int)next(); layout.off_z = (int)next();
      layout.off_intensity = (int)next(); layout.intensity_type = (int)next(); layout.off_time = (int)next(); layout.time_type = (int)next();
      layout.filter = (int)next();
      double ekf_noise[12];
      for (int i = 0; i < 12; i++) ekf_noise[i] = next();
      IMUST x0;                                                  // x_curr before the first scan
      std::memcpy(&x0.t, &in.at(q), 25 * sizeof(double)); q += 25;
      std::memcpy(x0.cov, &in.at(q), 225 * sizeof(double)); q += 225;
      ScanFrame frame(ctx);
      InitWindow pl_origs(ctx);
      OdomState x_dev(ctx);
      x_dev.set(x0);
      std::vector<std::vector<ImuSample>> vec_imus(win_size);
      std::vector<double> beg_times(win_size), per_scan;
      std::vector<PathPoint> pcl_path;
      const double downkd = down_size >= 0.5 ? down_size : 0.5;  // VS:1470
      for (int i = 0; i < win_size; i++) {
        const int n_raw = (int)next();
        const size_t n_words = (size_t)next();
        const int n_imu = (int)next();
        const double last_end = next(), beg = next(), end = next();
        if (n_raw < 0 || n_imu < 0 || (size_t)n_raw * (size_t)layout.point_step > n_words * 8 || q + n_words + (size_t)n_imu * 7 > in.size())
          throw std::runtime_error("mode 10: the raw message or the IMU rows do not fit the input");
        frame.decode(n_words ? &in[q] : nullptr, n_raw, layout, point_filter_num, blind);     // pcl_handler; `orig` = its cloud (VS:1458)
        q += n_words;
        const double *imu = &in[q];
        vec_imus[i].resize((size_t)n_imu);
        for (int j = 0; j < n_imu; j++) { std::memcpy(&vec_imus[i][j], &in.at(q), 7 * sizeof(double)); q += 7; }
        x_dev.propagate(ekf_noise, scale_gravity, n_imu, imu, last_end, beg, end);            // odom_ekf.process (VS:1460)
        const ScanView scan = x_dev.prepare(ctx, frame, extrin_para, init.point_notime != 0, downkd, init.dept_err, init.beam_err, 0);   // VS:1470-1474
        IMUST x_curr = x0;                                       // (x_buf keeps the covariance of x0: the state's stays on the device)
        const int iters = x_dev.lio_state_estimation_kdtree(ctx, scan, nullptr, &x_curr);     // VS:1476
        int64_t n_pub = 0;
        unsigned long long sum = 0;
        pub_localtraj(ctx, x_dev, scan, 0, x_curr, 0, pcl_path, [&](const float *xyzi, int64_t n) {   // VS:1480-1488
          n_pub = n;
          for (int64_t e = 0; e < 4 * n; e++) { uint32_t b; std::memcpy(&b, xyzi + e, 4); sum += b; }
        }, [](const std::vector<PathPoint> &) {});
        x_buf.push_back(x_curr);
        if (i > 0) {                                             // VS:1491-1496
          std::vector<double> t, g, a;
          for (const ImuSample &m : vec_imus[i]) { t.push_back(m.t); g.insert(g.end(), m.gyr, m.gyr + 3); a.insert(a.end(), m.acc, m.acc + 3); }
          imu_pre_buf.push_back(new IMU_PRE(x_buf[i - 1].bg, x_buf[i - 1].ba));
          imu_pre_buf.back()->push_imu((int)t.size(), t.data(), g.data(), a.data(), noise, noise + 6, scale_gravity);
        }
        bool retried = false;
        const int kept = pl_origs.push(frame, down_size, min_points, &retried);               // VS:1499-1512
        beg_times[i] = beg;
        per_scan.push_back(iters);
        per_scan.insert(per_scan.end(), &x_curr.t, &x_curr.t + 25);
        per_scan.push_back(kept); per_scan.push_back(retried ? 1.0 : 0.0);
        per_scan.push_back((double)n_pub); per_scan.push_back((double)sum);
      }
      IMUST x_curr;
      const int ok = init.motion_init(pl_origs, vec_imus, beg_times, &hess, voxhess, x_buf, surf_map, pvec_buf, win_size, x_curr, imu_pre_buf,
                                      extrin_para);                // whether it converges on odometry-produced states is recorded, not required
      x_dev.set(x_buf.back());
      out.push_back(-2.0); out.push_back(ok); out.push_back(init.iterations); out.push_back(init.thresholds_left_relaxed);
      out.insert(out.end(), init.eigvalue, init.eigvalue + 3);
      for (int i = 0; i < win_size; i++) out.insert(out.end(), &x_buf[i].t, &x_buf[i].t + 25);
      out.insert(out.end(), per_scan.begin(), per_scan.end());
      k_first = n_scans;
    }

    for (int k = k_first; k < n_scans; k++) {
      if (loop_mode && k == n_loop) {                            // loop_detect == 1 (VS:1768-1773)
        if (keyframes->size() < 2 || win_count < 1) throw std::runtime_error("mode 7 / 9: the session built fewer than two keyframes");
        for (IMUST &x0 : kf_x0) apply_dx(x0, dx);                // VS:2582-2587 with a synthetic correction
        keyframes->set_poses(0, kf_x0);
        const int n_ins = map_loop->build(*keyframes);           // VS:2601-2625
        std::vector<ScanPose *> bl;
        for (auto &b : buf_lba2loop) bl.push_back(b.get());
        IMUST x_now = x_buf[win_count - 1];
        int g_upd = 0;
        const int nf = use_log ? surf_map.loop_update(*map_loop, dx, *scan_log, bl_first, bl_states, x_buf, win_count, x_now, g_upd)
                               : surf_map.loop_update(*map_loop, dx, bl, x_buf, win_count, x_now, g_upd);
        out.push_back(-3.0); out.push_back(n_ins); out.push_back(nf); out.push_back(keyframes->size());
        for (int i = 0; i < keyframes->size(); i++) {
          std::vector<XYZ> xyz, nrm;
          keyframes->read(i, xyz, &nrm);
          out.push_back((double)xyz.size());
          out.insert(out.end(), kf_x0[i].R, kf_x0[i].R + 9); out.insert(out.end(), kf_x0[i].p, kf_x0[i].p + 3);
          for (const XYZ &a : xyz) { out.push_back(a.x); out.push_back(a.y); out.push_back(a.z); }
          for (const XYZ &a : nrm) { out.push_back(a.x); out.push_back(a.y); out.push_back(a.z); }
        }
        out.push_back((double)(use_log ? bl_states.size() : bl.size()));
        for (size_t i = 0; i < bl.size(); i++) { out.push_back(bl_index[i]); out.insert(out.end(), &bl[i]->x.t, &bl[i]->x.t + 25); }
        for (size_t i = 0; i < bl_states.size(); i++) { out.push_back(bl_index[i]); out.insert(out.end(), &bl_states[i].t, &bl_states[i].t + 25); }
        out.push_back(win_count);
        for (int i = 0; i < win_count; i++) out.insert(out.end(), &x_buf[i].t, &x_buf[i].t + 25);
        buf_lba2loop.clear(); bl_index.clear();
        if (use_log) { bl_first += (int64_t)bl_states.size(); bl_states.clear(); scan_log->release(bl_first); }   // VS:2342
        moved = true;
      }
      const int n = (int)next();
      IMUST x_curr;
      std::memcpy(&x_curr.t, &in.at(q), 25 * sizeof(double)); q += 25;
      if (moved) apply_dx(x_curr, dx);
      scan_of_frame.push_back(k);
      std::memcpy(x_curr.cov, &in.at(q), 225 * sizeof(double)); q += 225;
      const int n_imu = (int)next();
      std::shared_ptr<PVec> pptr(new PVec((size_t)n));
      for (int i = 0; i < n; i++) { std::memcpy((*pptr)[i].pnt, &in.at(q), 24); q += 3; }
      for (int i = 0; i < n; i++) { std::memcpy((*pptr)[i].var, &in.at(q), 72); q += 9; }
      const double *imu_t = &in[q]; q += (size_t)n_imu;
      const double *imu_g = &in[q]; q += (size_t)n_imu * 3;
      const double *imu_a = &in[q]; q += (size_t)n_imu * 3;

      // VS:1905-1913
      win_count++;
      x_buf.push_back(x_curr);
      pvec_buf.push_back(pptr);
      if (win_count > 1) {
        imu_pre_buf.push_back(new IMU_PRE(x_buf[win_count - 2].bg, x_buf[win_count - 2].ba));
        imu_pre_buf[win_count - 2]->push_imu(n_imu, imu_t, imu_g, imu_a, noise, noise + 6, scale_gravity);
      }
      // VS:1918-1926: pvec_update (VS:1901) rides in the insert, as the device path fuses the two
      voxhess.clear();
      surf_map.pvec_update_cut_voxel_multi(*pvec_buf[win_count - 1], win_count - 1, x_curr);
      surf_map.multi_recut(win_count, x_buf);

      if (win_count >= win_size) window_step(k);                // VS:1951
    }
    while (!imu_pre_buf.empty()) { delete imu_pre_buf.front(); imu_pre_buf.pop_front(); }
    // final map: leaves + plane covariances
    const int nl = vba_map_dump_leaves(ctx.get(), nullptr, 0);
    out.push_back(-1.0);
    out.push_back((double)nl);
    std::vector<double> leaves((size_t)(nl > 0 ? nl : 1) * 39), pv((size_t)(nl > 0 ? nl : 1) * 86);
    if (nl > 0) { vba_map_dump_leaves(ctx.get(), leaves.data(), nl); vba_map_dump_plane_var(ctx.get(), pv.data(), nl); }
    out.insert(out.end(), leaves.begin(), leaves.begin() + (size_t)nl * 39);
    out.insert(out.end(), pv.begin(), pv.begin() + (size_t)nl * 86);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "harness: %s\n", e.what());
    return 1;
  }
  FILE *f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) { std::fprintf(stderr, "harness: cannot write %s\n", argv[2]); return 2; }
  std::fclose(f);
  return 0;
}
