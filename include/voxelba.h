/*
 * voxelba.h — C ABI of the MI355X-native Voxel-SLAM local-mapping hot path (libvoxelba.so).
 *
 * The reference (Wangshihu12/Voxel-SLAM, /root/reference/VoxelSLAM/src) has no FFI/plugin boundary: the
 * path is reached through C++ member calls on header-only classes.  Each entry point
 * below names the reference interface it replaces (VM = voxel_map.hpp, VS = voxelslam.cpp,
 * TL = tools.hpp, PI = preintegration.hpp).  include/voxelba_adapter.hpp wraps these calls back into
 * the reference's class/method names (LidarFactor, Lidar_BA_Optimizer, LI_BA_Optimizer, ...).
 *
 * Conventions
 *   - All numeric arrays are IEEE double, caller-owned, HOST memory unless a name ends in _dev.
 *   - Every function returns an int status (VBA_OK = 0) where the reference would printf+exit(0)
 *     (VM:401-402, VM:1490-1491) or silently return; no function throws.
 *   - A context is re-entrant per handle: one HIP stream per vba_ctx, no process-wide mutable state
 *     (the reference's globals VM:98-104, VM:500, VM:1046 are fields of vba_options / the context).
 *   - The library has NO CPU compute fallback: without a HIP device vba_create fails with
 *     VBA_ERR_NO_DEVICE.
 *
 * Flat layouts
 *   cluster : [Pxx,Pxy,Pxz,Pyy,Pyz,Pzz, vx,vy,vz, N]    (10)   PointCluster TL:304-310 (P symmetric)
 *   pose    : [R(9) row-major, p(3)]                    (12)   IMUST::R, IMUST::p  TL:139-140
 *   state   : [t, R(9), p(3), v(3), bg(3), ba(3), g(3)] (25)   IMUST TL:135-144 (cov passed separately)
 *   imu_pre : [R_delta(9) p_delta(3) v_delta(3) bg(3) ba(3) R_bg(9) p_bg(9) p_ba(9) v_bg(9) v_ba(9)
 *              dtime dbg(3) dba(3) dbg_buf(3) dba_buf(3) cov(225)]  (304)   IMU_PRE PI:15-28
 *   3x3 / NxN matrices are row-major; eigenvector matrices hold eigenvectors in COLUMNS (VM:193).
 */
#ifndef VOXELBA_H
#define VOXELBA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBA_CLUSTER_LEN 10
#define VBA_POSE_LEN 12
#define VBA_STATE_LEN 25
#define VBA_IMU_PRE_LEN 304
#define VBA_DIM 15 /* TL:16 */
#define VBA_MAX_WIN 16

enum vba_status {
  VBA_OK = 0,
  VBA_ERR_NO_DEVICE = 1,       /* no HIP device / kernel image: the product has no CPU path */
  VBA_ERR_BAD_ARG = 2,
  VBA_ERR_UNSUPPORTED_WINDOW = 3,
  VBA_ERR_TOO_FEW_VOXELS = 4,  /* Lidar_BA_Optimizer::only_residual "Too Less Voxel" exit(0), VM:399-403 */
  VBA_ERR_OPT_STATE = 5,       /* OctoTree::margi "Error: opt_state" exit(0), VM:1488-1492 */
  VBA_ERR_HIP = 6,
  VBA_ERR_CAPACITY = 7,
  VBA_ERR_IO = 8,              /* file missing / malformed (read_lidarstate prints "not found" and exits, VH:271-275) */
  VBA_ERR_UNSUPPORTED = 9,     /* the in-library RCCL exchange step was asked for but librccl.so.1 cannot be resolved in this process */
  VBA_ERR_SINGULAR = 10        /* vba_pgo_optimize: a connected component without a prior, or a non-positive pivot */
};

typedef struct vba_ctx vba_ctx;

/* Replaces the process-wide configuration of the reference: voxel_size, min_eigen_value, max_layer,
 * max_points, plane_eigen_value_thre, min_point (VM:98-104), imu_coef (VM:500), LocalBA/win_size and
 * thread_num (VS:875-931).  plane_eigen_value_thre is passed ALREADY INVERTED as the reference stores
 * it (VS:930-931). */
typedef struct vba_options {
  int win_size;                     /* LocalBA/win_size */
  double voxel_size;                /* Odometry/voxel_size */
  int max_layer;                    /* VM:100 */
  int max_points;                   /* VM:101 */
  double min_eigen_value;           /* VM:99 */
  double plane_eigen_value_thre[4]; /* VM:104, inverted */
  double min_point[4];              /* VM:98 */
  double imu_coef;                  /* VM:500 */
  int thread_num;                   /* only for the "#voxels < thread_num" early-return quirks (VM:2044, VS:1616, VS:1693) */
  int device;                       /* HIP device ordinal, -1 = current */
  void *stream;                     /* hipStream_t to run on, NULL = the context creates its own */
  size_t max_voxels;                /* factor capacity hint (0 = grow on demand) */
  size_t max_points_per_scan;       /* map capacity hint (0 = grow on demand) */
  /* execution knobs (no reference counterpart; 0 = default).  They replace the environment switches of earlier builds. */
  int lm_spec;                      /* damping candidates per solve launch, 1..4 (default 4; 1 = the plain sequential solve) */
  int force_collective;             /* != 0: take the exchange step of the sharded LM flow with ONE rank too (rehearsals) */
  int hessian_workgroups;           /* persistent workgroups of the Hessian pass, 2..256 (default 256 = one per CU) */
  int residual_vpl_from;            /* residual pass: stores with more voxels use the voxel-per-lane kernel (default 45000) */
  int hessian_compact_tiles;        /* != 0: Hessian pass on occupancy-compact tiles (k_hessian3, W <= 10) instead of dense fixed-size ones; measured slower at the bench size */
  /* (this field occupies what was alignment padding behind the five ints above: no other field moves, the size is unchanged)
     Lidar LM iteration on one rank: 0 (default) = the solve and the residual pass of the trial poses share ONE launch (k_lm_trial) where
     the window's kernel allows it; 2 = always the two launches k_lm_solve_m + k_residual_s.  Results are bit-identical.
     A residual workgroup of the fused launch waits for the solve's poses for at most 20 ms; one that gives up rejects the step and marks the
     LM state, and the next call that fetches that state (vba_lm_end with an output, vba_lm_iterate with accepted / stop,
     vba_lidar_ba_damping_iter) returns VBA_ERR_HIP with vba_last_error naming k_lm_trial. */
  int lm_trial_launches;
  size_t max_map_nodes;             /* map capacity hints (0 = grow on demand): octree nodes and fixed (marginalised) points the map is */
  size_t max_fix_points;            /* sized for at the first insertion — a session that stays below them never re-allocates (no stalls) */
  int hba_workers;                  /* vba_hba_global on one rank: bottom-layer windows optimised side by side by this many worker contexts (0 = default 4, 1 = one after the other) */
  /* != 0: deterministic mode.  Given identical inputs, options, call sequence and hessian_workgroups, every call
     below returns bit-identical results in every run: node ids are handed out in a canonical order (new roots by the first input
     point of their voxel, child blocks by parent id, free ids ascending), the factor store is ordered by (occupancy bucket, node
     id), dumps list leaves by node id, down-sampling adds each voxel's points in input order; hessian_compact_tiles is ignored.
     Covered: map insert / fixed insert / recut / extraction / margi / slide / prune / reset / dumps, acc_evaluate2,
     evaluate_only_residual, the lidar, LI and LI-gravity damping_iter and lm_* entry points, both odometry variants, scan var_init /
     down-sampling / undistortion, vba_motion_init.  NOT covered: vba_gba_build, vba_hba_* and the large-window store (they add with
     f64 atomics), and multi-rank runs (the collective's order belongs to RCCL or the hook).  0 (default): today's kernels. */
  int deterministic;
} vba_options;

void vba_default_options(vba_options *opt); /* values of config/avia.yaml:26-47 */
int vba_create(const vba_options *opt, vba_ctx **out);
void vba_destroy(vba_ctx *ctx);
const char *vba_status_string(int status);
const char *vba_last_error(vba_ctx *ctx);
int vba_synchronize(vba_ctx *ctx);

/* ------------------------------------------------------------------------------------------------
 * Factor level — drop-in for class LidarFactor (VM:124-339).
 * The factor store lives in HBM as SoA [field][frame][voxel].                        */

/* LidarFactor::clear (VM:328-336) */
int vba_factor_clear(vba_ctx *ctx);
/* LidarFactor::push_voxel (VM:139-147), batched: n voxels appended.
 * clusters [n][W][10], fix [n][10], coe [n], eig_val [n][3], eig_vec [n][9], pcr_add [n][10]. */
int vba_factor_push_voxels(vba_ctx *ctx, int n, const double *clusters, const double *fix, const double *coe,
                           const double *eig_val, const double *eig_vec, const double *pcr_add);
/* plvec_voxels.size() (read by callers at VS:706) */
int vba_factor_size(vba_ctx *ctx);
/* LidarFactor::acc_evaluate2 (VM:150-282) over voxels [head,end): Hess (6W x 6W), JacT (6W), residual. */
int vba_factor_acc_evaluate2(vba_ctx *ctx, const double *poses, int head, int end, double *Hess, double *JacT,
                             double *residual);
/* LidarFactor::evaluate_only_residual (VM:285-325) over [head,end); updates the device-side
 * eig_values / eig_vectors / pcr_adds exactly as the reference does (VM:317-319). */
int vba_factor_evaluate_only_residual(vba_ctx *ctx, const double *poses, int head, int end, double *residual);
/* Public data members eig_values / eig_vectors / pcr_adds read by OctoTree::margi (VM:1495-1501) and
 * motion_init (VS:737).  Any pointer may be NULL. */
int vba_factor_read_back(vba_ctx *ctx, double *eig_val, double *eig_vec, double *pcr_add);

/* Number of occupied (voxel, frame) slots (clusters with N != 0) in the factor store — the "slots" that the
 * algorithmic-traffic figures of DESIGN.md are priced on. */
int vba_factor_occupied_slots(vba_ctx *ctx, long long *slots);
/* Occupancy mask of every stored voxel (bit i = frame i of the window sees it), in store order: `masks` holds vba_factor_size()
 * entries.  After vba_map_recut the store is in non-decreasing order of the mask's low 10 bits. */
int vba_factor_occupancy_masks(vba_ctx *ctx, unsigned int *masks);

/* ------------------------------------------------------------------------------------------------
 * Optimizers — drop-in for the three LM classes.                                                  */

/* bool Lidar_BA_Optimizer::damping_iter(x_stats, voxhess, hess, resis, max_iter, is_display) (VM:422-497).
 * poses [W][12] in/out; hess (6W)^2 out (may be NULL); resis2[2] = {first, last} appended values;
 * thd_num = Lidar_BA_Optimizer::thd_num (VM:345) — only used for the V < thd_num check (VM:399).
 * *is_converge receives the bool return value. */
int vba_lidar_ba_damping_iter(vba_ctx *ctx, double *poses, double *hess, double *resis2, int max_iter, int thd_num,
                              int *is_converge);

/* void LI_BA_Optimizer::damping_iter(x_stats, voxhess, imus_factor, hess) (VM:624-713) when gravity == 0;
 * void LI_BA_OptimizerGravity::damping_iter(x_stats, voxhess, imus_factor, resis, hess, max_iter) (VM:878-975)
 * when gravity != 0.  states [W][25] in/out, imus [W-1][304] in/out (dbg/dba/dbg_buf/dba_buf are updated,
 * PI:296-303), hess ((15W + 3*gravity)^2) out (may be NULL), resis2 out (gravity variant only, may be NULL). */
int vba_li_ba_damping_iter(vba_ctx *ctx, double *states, double *imus, int gravity, int max_iter, double *hess,
                           double *resis2);

/* Optional iteration trace of the last damping_iter on this context: rows [r1, r2, u, v, q1] as used in each
 * executed iteration.  Returns the number of rows written (<= max_rows). */
int vba_last_lm_trace(vba_ctx *ctx, double *rows, int max_rows);

/* IMU_PRE(bg, ba) + IMU_PRE::push_imu (PI:32-73) with the noise globals noiseMeas / noiseWalk /
 * imupre_scale_gravity (PI:8-9) passed as diagonals: samples t[n], gyr[n][3], acc[n][3] -> imu_pre[304]. */
int vba_imu_preintegrate(int n, const double *t, const double *gyr, const double *acc, const double *bg,
                         const double *ba, const double *noise_meas_diag6, const double *noise_walk_diag6,
                         double scale_gravity, double *imu_pre_out);
/* IMU_PRE::give_evaluate (PI:137-212) / give_evaluate_g (PI:214-294): returns r^T cov^-1 r in *resid;
 * jtj ((30|33)^2) and gg (30|33) are written when jac_enable != 0. */
int vba_imu_give_evaluate(const double *imu_pre, const double *state1, const double *state2, int with_gravity,
                          int jac_enable, double *jtj, double *gg, double *resid);

/* ------------------------------------------------------------------------------------------------
 * Map level — drop-in for the voxel hash map + octree of local mapping.                           */

/* cut_voxel (VM:1896-1949) / cut_voxel_multi (VM:1964-2096) for one scan: pnt_body [n][3] body-frame
 * points (pointVar::pnt), var [n][9] per-point covariance as produced by pvec_update (VH:242-265) or NULL,
 * pose [12] = the scan's pose used for pw = R p + t (the pwld argument), win_count = frame index in the window.
 * multi != 0 applies cut_voxel_multi's "#touched voxels < thread_num -> scan dropped" rule (VM:2044-2045).
 * pnt_body / var may point to HOST or DEVICE (HBM) memory; device buffers are consumed in place. */
int vba_map_cut_voxel(vba_ctx *ctx, int win_count, int n, const double *pnt_body, const double *var,
                      const double *pose, int multi);
/* pvec_update (VH:242-265) fused with cut_voxel[_multi]: var_body [n][9] is the BODY-frame covariance of the scan's
 * points (from var_init); the world-frame covariance var = R var R^T + phat rot_var phat^T + tsl_var is formed on the
 * device from the scan state's covariance cov [225] (x_curr.cov: rot block (0,0), translation block (3,3)). */
int vba_map_pvec_update_cut_voxel(vba_ctx *ctx, int win_count, int n, const double *pnt_body, const double *var_body,
                                  const double *pose, const double *cov, int multi);
/* var_init (VH:210-234) = calcBodyVar (VH:180-200) + extrinsic ext_pose [12]: pnt_in [n][3] -> pnt_out [n][3],
 * var_out [n][9] (host buffers; pnt_out may alias pnt_in). */
int vba_scan_var_init(vba_ctx *ctx, int n, const double *pnt_in, const double *ext_pose, double dept_err, double beam_err,
                      double *pnt_out, double *var_out);
/* down_sampling_voxel (tools.hpp:201-238): voxel-grid centroid filter.  pnt [n][3] (PCL float coordinates carried in
 * doubles) -> pnt_out [<=n][3] centroids rounded to float, count_out = points per voxel (the `curvature` field after the
 * call, TL:221/230), first_out = index of the voxel's first input point (whose intensity/normal fields the reference
 * keeps); *n_out = number of voxels.  Output order = first occurrence (the reference's is unordered_map order).
 * voxel_size < 0.001 returns the input unchanged (TL:203), counts 0.  Buffers may be HOST or DEVICE memory. */
int vba_scan_down_sampling_voxel(vba_ctx *ctx, int n, const double *pnt, double voxel_size, double *pnt_out, int *count_out,
                                 int *first_out, int *n_out);
/* down_sampling_pvec (voxel_map.hpp:39-83): the pointVar form used when a keyframe cloud is made (VS:2385): double
 * coordinates pnt [n][3] and covariances var [n][9] -> per voxel the mean point and the mean covariance DIAGONAL
 * (stored by the reference in normal_x/y/z), both narrowed to float like the PCL points they become. */
int vba_scan_down_sampling_pvec(vba_ctx *ctx, int n, const double *pnt, const double *var, double voxel_size,
                                double *pnt_out, double *vardiag_out, int *count_out, int *n_out);
/* down_sampling_close (tools.hpp:240-298): per voxel the index of the input point closest to the voxel's centroid
 * (first such point; only squared distances < 100 compete, else the voxel's first point — TL:281-295). */
int vba_scan_down_sampling_close(vba_ctx *ctx, int n, const double *pnt, double voxel_size, int *index_out, int *n_out);
/* Undistortion inner loop of IMUEKF::motion_blur (ekf_imu.hpp:137-163).  pnt [n][3] in/out, curv [n] = per-point time
 * offset (PointType::curvature), ascending as pcl_handler leaves them (VH:92-95); imu_poses [m][22] = the imu_poses
 * vector (EK:87): t, R[9], p[3], v[3], angvel_avr[3], acc_imu[3]; end_pose [12] = xc.R, xc.p after propagation
 * (EK:121-123); ext_pose [12] = Lid_rot_to_IMU, Lid_offset_to_IMU. */
int vba_scan_undistort(vba_ctx *ctx, int n, double *pnt, const double *curv, int m, const double *imu_poses,
                       const double *end_pose, const double *ext_pose);
/* cut_voxel(feat_map, PVec&, wdsize, jour) for fixed (already-world) points (VM:2108-2152). */
int vba_map_cut_voxel_fix(vba_ctx *ctx, int n, const double *pnt_world, double jour);
/* multi_recut (VS:1682-1737) when multi != 0, or the loop "recut + tras_opt over surf_map" of motion_init
 * (VS:699-703) when multi == 0: OctoTree::recut (VM:1396-1456) on every root, then OctoTree::tras_opt
 * (VM:1605-1638) fills the context's factor store (voxhess.clear() + win_size, VS:1918-1919, is implied). */
int vba_map_recut(vba_ctx *ctx, int win_count, const double *poses, int multi);
/* multi_margi (VS:1590-1679): OctoTree::margi (VM:1465-1598, mgsize = 1) on every root of the sliding map
 * using the factor store's refined eig/pcr_add, then drops roots with !isexist from the sliding map.
 * jour is stamped on every sliding-map root (VS:1628). */
int vba_map_margi(vba_ctx *ctx, int win_count, const double *poses, double jour);
/* Ring-map rotation mp[i] = (mp[i] + mgsize) mod W (VS:2014-2019). */
int vba_map_slide(vba_ctx *ctx, int mgsize);
/* "Release the features not used for a long time" (VS:1800-1823): roots with int(jour - root.jour) >= dist (700 in
 * the reference) leave surf_map with their subtrees. */
int vba_map_prune(vba_ctx *ctx, double jour, int dist);
/* Destroys the map (system_reset / motion_init teardown, VS:650-661). */
int vba_map_reset(vba_ctx *ctx);
int vba_map_num_roots(vba_ctx *ctx);       /* surf_map.size() */
int vba_map_num_slide_roots(vba_ctx *ctx); /* surf_map_slide.size() */
/* Storage statistics of the device map (the reference new/deletes OctoTree nodes, VS:1787-1823; here pruned roots hand their
 * node storage and hash slots back for reuse): out8 = [node high-water mark, free root nodes, free 8-node child blocks, root
 * table capacity, root table slots in use (live roots + tombstones), live roots, sliding-map roots, fixed points]. */
int vba_map_stats(vba_ctx *ctx, long long *out8);
/* Leaf dump for inspection / parity tests: 39 doubles per leaf
 * [kx,ky,kz, layer, path, N_add, N_fix, is_plane, isexist, opt_state, eig_value(3), eig_vector(9), pcr_add(10),
 *  plane.center(3), plane.normal(3), plane.radius].  out == NULL returns the leaf count. */
int vba_map_dump_leaves(vba_ctx *ctx, double *out, int max_leaves);
/* The two covariance outputs of the map that the leaf dump does not carry: plane.plane_var (6x6; plane_update VM:1344-1388,
 * consumed by OctoTree::match VM:1667-1672) and cov_add (9x9 symmetric; Bf_var VM:106-121 summed by push VM:1138-1140).
 * 86 doubles per leaf: [kx,ky,kz, layer, path, plane_var(36 row-major), cov_add upper triangle (45, row by row)];
 * same leaf set as vba_map_dump_leaves (order not defined).  out == NULL returns the leaf count. */
int vba_map_dump_plane_var(vba_ctx *ctx, double *out, int max_leaves);
/* The view of the live local voxel map: OctoTree::tras_display (VM:1765-1827) over every root of surf_map, what the
 * topics /map_wind and /avoxel show.  The planar leaves come out as records, and with them the window's points that sit in planar
 * leaves, at the poses given (x_buf).  pl_fixd is not produced (its loop is commented out in the reference).  The map is only read.
 *
 * Planes: one record per live leaf with plane.is_plane (VM:1780; the leaves whose column 7 of vba_map_dump_leaves is 1), 16 floats,
 * formed fresh from the leaf's pcr_add as VM:1771-1773 does (center = v / N, cov = P / N - center center^T, uncontracted), each double
 * narrowed to float once:
 *   [0..2] center   [3] half edge of the leaf's cube (2 quater_length)
 *   [4..6] unit eigenvector of the smallest eigenvalue (sign as the solver leaves it)   [7] layer
 *   [8..10] sqrt of the eigenvalues, ascending, negative rounding residue clamped to 0   [11] pcr_add.N
 *   [12..14] voxel_center   [15] pcr_add.N - pcr_fix.N
 * (the commented-out attributes of VM:1794-1797 are floats 8, 10 / 8, 11 and 15).  plane_key[i] = {kx, ky, kz, layer, path}, the
 * first five columns of vba_map_dump_leaves.  Order: ascending node id (a stable compaction over the nodes), hence a function of the
 * map bit for bit under vba_options::deterministic and an unspecified permutation otherwise.
 * Points: for i = 0 .. win_count - 1 in this order, the points of ring slot mp[i] that sit in a planar leaf, in the order the scan
 * was inserted with (the slot's own storage groups them by leaf in an order that differs from run to run; the export undoes that, so
 * the point records are the same bytes in every run and every mode); with flags & 1 every point that sits in a leaf.  Record = x y z intensity: xyz = poses[i].R pnt + poses[i].p in the uncontracted order
 * ((R0 x + R1 y) + R2 z) + p, each coordinate narrowed to float once (VM:1807-1810), intensity = (float)i.  plane_of_point[j] = index
 * of the record of that point's leaf in `planes`, -1 for a point of a non-planar leaf (flags & 1 only).  frame_begin[i] = first
 * record of frame i, frame_begin[win_count] = *n_points: frames are contiguous, a stable compaction of the scan inside each.
 * xyzi, plane_of_point, planes and plane_key are all HOST or all DEVICE memory (a device xyzi / planes 16-byte aligned); poses,
 * frame_begin and the counts are host memory.  The work runs on ctx's stream.  The host needs the counts, so every call waits for
 * the stream once; a device result is then written stream-ordered, without a second wait; a host result passes through the map's
 * staging buffer and the call returns when it has arrived.
 * cap_points == 0 with xyzi == NULL, and cap_planes == 0 with planes == NULL, form the size query of their side: the counts (and
 * frame_begin) are set, nothing of that side is written and no capacity is checked for it.  planes == NULL with plane_of_point !=
 * NULL is allowed: the indices refer to the order a full call returns.  A result larger than its cap is VBA_ERR_CAPACITY with
 * *n_points and *n_planes set and every buffer (frame_begin too) untouched; so is a window of 2^31 points or more.
 * Work arrays: an int per node, an int per 256 nodes and per 256-point workgroup, an int per window point (scan index -> position
 * in the slot), the counts, and the staging of a host result (20 bytes per point, 104 per plane).  They belong to the context's map, _reserve(max_points, max_planes) sizes them for the map's
 * current node capacity (or vba_options::max_map_nodes) and a host result of that size, a call that needs more doubles them after
 * a synchronise, and nothing is allocated per call.  _allocations: allocations made and bytes requested for this feature so far.
 * VBA_ERR_BAD_ARG before any device work, outputs untouched: a NULL ctx, n_points or n_planes; win_count < 0 or > win_size; NULL
 * poses with win_count > 0; a negative cap; cap_points > 0 with a NULL xyzi; cap_planes > 0 with planes and plane_key both NULL;
 * flag bits other than 1; result arrays on different sides; a misaligned device xyzi or planes.  A context without a map, an empty
 * map or win_count == 0 give zero points and the planes that exist.  A sharded context exports its own leaves, with no collective. */
int vba_map_display_reserve(vba_ctx *ctx, int64_t max_points, int64_t max_planes);
int vba_map_display_allocations(vba_ctx *ctx, int *n_allocs, int64_t *bytes);
int vba_map_display(vba_ctx *ctx, int win_count, const double *poses /* [win_count][12], host: x_buf */, int flags,
                    int64_t cap_points, float *xyzi /* [cap_points][4] */, int *plane_of_point /* [cap_points] or NULL */,
                    int64_t *frame_begin /* host, [win_count + 1], or NULL */,
                    int64_t cap_planes, float *planes /* [cap_planes][16] or NULL */, long long *plane_key /* [cap_planes][5] or NULL */,
                    int64_t *n_points, int64_t *n_planes);

/* ------------------------------------------------------------------------------------------------
 * Odometry scan-to-map ("next #1").
 * bool VOXEL_SLAM::lio_state_estimation(PVecPtr pptr) (VS:962-1098): iterated EKF update of x_curr against the voxel map
 * with match() (VM:2167-2205) / OctoTree::match (VM:1649-1721).  pnt_body [n][3] and var_body [n][9] are the scan's
 * body-frame points and covariances (pointVar as produced by var_init, VH:210-234); state [25] and cov [225] = x_curr
 * (IMUST incl. its 15x15 covariance) in/out; *ok receives the bool result (false = degenerate, VS:1090-1097).
 * pnt_body / var_body may be host or device arrays.  The call is a staging front end of vba_odom_lio_state_estimation_resident
 * below: it copies the scan into the context's staging buffer (device to device when handed device arrays), runs that call's loop on
 * the copy and returns its bits; the call has completed when it returns.  n == 0 or a map that was never allocated: state and cov
 * come back bit-identical, *ok = 0.  Unlike the call below it accepts a sharded context and runs on the local map. */
int vba_odom_lio_state_estimation(vba_ctx *ctx, int n, const double *pnt_body, const double *var_body, double *state,
                                  double *cov, int *ok);

/* The same update with its 2-4 iterations resident on the device: no host round trip between them.
 * d_pnt_body [n][3] and d_var_body [n][9] are DEVICE arrays (what vba_scan_prepare hands out), read in place and never copied;
 * state [25] and cov [225] are host arrays, in/out, in the layout of vba_odom_lio_state_estimation; *ok (may be NULL) as there.
 * Call shape: cov^-1 is computed on the host; ONE host-to-device copy of one parameter block; for each
 * of the four possible iterations a point-loop launch and an update launch (one workgroup: fixed-order sum of the workgroup
 * partials, the 15x15 EKF step, the stop rule rematch_num >= 2 || iter == 3 of VS:1073-1086, and at the stop cov <- (I - G) cov);
 * after the stop the remaining launches find a flag in device memory and return at once; ONE device-to-host copy of one result
 * block and ONE stream synchronise.  No atomics: the call is bit-reproducible with and without vba_options::deterministic.
 * Scratch (device state, pinned image, partials) belongs to the context and only grows: a steady-state call allocates nothing.
 * report (may be NULL) receives what the loop saw; entries of iterations that did not run are zero.
 * n == 0 or a map that was never allocated: no point loop runs, all sums are zero, which the algebra takes as it is: the solution
 * is exactly zero, iterations == 2, state and cov come back bit-identical, *ok = 0.
 * VBA_ERR_BAD_ARG: NULL state / cov, n < 0, n > 0 with a NULL array.  VBA_ERR_UNSUPPORTED: a sharded context (n_ranks > 1) - the
 * all-reduce hook cannot run between iterations that the host never sees. */
typedef struct vba_odom_report {
  int iterations;                  /* EKF iterations run, 2..4 (VS:990-1087) */
  int match_num[4];                /* per iteration, VS:1048 */
  double rot_add[4], tra_add[4];   /* |solution(0:3)|, |solution(3:6)| per iteration, VS:1061-1062 */
  double nnt_eig_min;              /* evalue[0] of the last iteration's nnt, VS:1090-1094 */
} vba_odom_report;
int vba_odom_lio_state_estimation_resident(vba_ctx *ctx, int n, const double *d_pnt_body, const double *d_var_body,
                                           double *state, double *cov, int *ok, vba_odom_report *report /* may be NULL */);

/* void VOXEL_SLAM::lio_state_estimation_kdtree(PVecPtr pptr) (VS:1102-1252), the odometry used while the system initialises:
 * scan points against a point-cloud map (pl_tree, kept by the context) through an exact 5-nearest-neighbour plane fit.
 * While the map holds fewer than 100 points the scan only seeds it (VS:1105-1118, *iterations = 0); otherwise state / cov
 * are updated in place, the scan is appended in the refined pose and the map re-sampled on a 0.5 m grid (VS:1238-1250).
 * pnt_body may be a host or a device array.  The call is a staging front end of vba_odom_lio_state_estimation_kdtree_resident
 * below: it copies the points into the context's staging buffer, runs that call on the copy and returns its bits (state, cov,
 * iterations, map); unlike that call it has completed when it returns, after a seeding call too.  It shares that call's scratch,
 * allocated on first use and counted by vba_odom_kdtree_allocations, and its limit: VBA_ERR_CAPACITY when map + scan exceed 2^28
 * points. */
int vba_odom_lio_state_estimation_kdtree(vba_ctx *ctx, int n, const double *pnt_body, double *state, double *cov,
                                         int *iterations);
int vba_odom_kdtree_reset(vba_ctx *ctx);   /* pl_tree->clear() */
int vba_odom_kdtree_size(vba_ctx *ctx);    /* pl_tree->size() */
int vba_odom_kdtree_points(vba_ctx *ctx, double *xyz_out /* [size][3] */);

/* lio_state_estimation_kdtree (VS:1102-1252) on DEVICE points, read in place; iterations, map append and 0.5 m re-sampling stay on
 * the device.  d_pnt_body [n][3] is a DEVICE array of doubles (what vba_scan_prepare hands out), used as the
 * doubles it holds: only the 5-NN query and the appended map point are rounded to float (VS:1155-1157, VH:223-229).  state [25] and
 * cov [225] are host arrays, in/out; *iterations (may be NULL) as in the call above.  The map is the one the call above keeps: the two
 * calls may alternate on one context.
 * Call shape, map below 100 points (seeding, VS:1105-1118): ONE append launch with the pose passed by value; *iterations = 0, state
 * and cov untouched; no copy and no wait - the call is stream-ordered (vba_odom_kdtree_points and every later call follow it on the
 * context's stream).
 * Call shape, estimation: cov^-1 / 1000 is computed on the host; ONE host-to-device copy of one parameter
 * block; for each of the four possible iterations four launches - 5-NN candidates per map slice, slice merge + plane fit, the 28 sums
 * per workgroup, and the one-workgroup update of vba_odom_lio_state_estimation_resident under the kd stop rule (only a converged
 * iteration counts as a rematch; refind = converged || (iter == 2 && none converged yet)), 16 launches in all; one append launch
 * that reads its pose from the device state; the 0.5 m re-sampling of map + scan into the other half of the map's ping-pong; ONE
 * device-to-host copy of one result block, which carries the new map size; ONE stream synchronise.  Every launch of the loop reads a
 * `done` flag in device memory first and returns at once when the stop rule has fired; the search and fit launches also return when
 * the device-side refind flag is clear, so the planes of the last search stay in place for the sums.  The re-sampling's count and
 * first-index arrays are not downloaded.
 * n == 0 on a map of 100 points or more: no search, fit, sum or append launch; the update runs on zero sums (the solution is exactly
 * zero, *iterations = 2, state and cov come back bit-identical) and the map is still re-sampled, as the call above does.
 * No atomics except the ones of the re-sampling's non-deterministic mode: with vba_options::deterministic = 1 two contexts given the
 * same call sequence return identical bits for state, cov, report and map.
 * report (may be NULL): iterations, match_num[i] = points with an accepted plane, rot_add, tra_add; nnt_eig_min = 0 (this variant has
 * no nnt); all zero after a seeding call.
 * Scratch belongs to the context and grows by doubling after a synchronise.  After vba_odom_kdtree_reserve(max_map_points,
 * max_scan_points) no call allocates while size + n <= max_map_points and n <= max_scan_points: the reservation covers both halves of
 * the map, the candidates at the largest slice count, planes, partial sums, the re-sampler's work area and the pinned block.
 * vba_odom_kdtree_allocations counts the allocations of all of these and the bytes they asked for, cumulatively, as
 * vba_scan_frame_allocations does: a block that grows is counted again at its new size and the freed one is not subtracted, so a
 * counter that does not move means that nothing was allocated.  The map's halves are counted whichever of the two kd-tree calls grew
 * them; the loop state and its pinned block are shared with vba_odom_lio_state_estimation_resident and counted here whichever call
 * allocated them first.
 * VBA_ERR_BAD_ARG: NULL state / cov, n < 0, n > 0 with a NULL array, a negative reservation.  VBA_ERR_CAPACITY: map + scan exceed
 * 2^28 points. */
int vba_odom_lio_state_estimation_kdtree_resident(vba_ctx *ctx, int n, const double *d_pnt_body, double *state, double *cov,
                                                  int *iterations, vba_odom_report *report /* may be NULL */);
int vba_odom_kdtree_reserve(vba_ctx *ctx, int max_map_points, int max_scan_points);
int vba_odom_kdtree_allocations(vba_ctx *ctx, int *n_allocs, int64_t *bytes);

/* ------------------------------------------------------------------------------------------------
 * LiDAR-inertial initialisation: int Initialization::motion_init(pl_origs, vec_imus, beg_times, hess, voxhess, x_buf, surf_map,
 * surf_map_slide, pvec_buf, win_size, sws, x_curr, imu_pre_buf, extrin_para) (VS:617-819, called from initialization at VS:1524).
 * Up to 10 rounds of {map teardown (VS:650-661), motion blur of every scan with its own IMU deque (VS:506-601, VS:668), cut_voxel
 * with win_count = i (VM:1896, VS:688), recut + tras_opt with multi = 0 (VS:695-703), break if fewer than 10 factors (VS:706-707),
 * LI_BA_OptimizerGravity::damping_iter(.., 3) (VS:711), re-preintegration of scan i's deque with x_buf[i-1].bg/ba (VS:719-730),
 * convergence / degeneracy test (VS:733-758, align_gravity on the first hit)}; failure (VS:764-786) tears the map down, success
 * leaves map and factor store on the context as surf_map / voxhess are left for the first steady-state step.
 * The clouds are uploaded once per call and stay in HBM; per round only the factor count, resis, the states and eigvalue3 cross.
 * The relaxed thresholds of VS:624-630 (min_eigen_value 0.02, plane_eigen_value_thre 1/4) apply through a per-call override of the
 * map's parameters until the round after the first convergence (VS:643-647); the context's vba_options are never written.
 *   win_size                   W = vba_options::win_size (win_size)
 *   pt_offsets [W+1], pnt [][3], curv []   pl_origs: ragged raw clouds, rows pt_offsets[i]..pt_offsets[i+1] of scan i, lidar-frame
 *                              xyz (PCL float values in doubles) and PointType::curvature, ascending per scan (VS:1510-1512)
 *   imu_offsets [W+1], imu [][7]   vec_imus: ragged deques, rows [t, gyr(3), acc(3)] as the deques hold them (VS:1513)
 *   beg_times [W]              beg_times (odom_ekf.pcl_beg_time per scan, VS:1514)
 *   ext_pose [12]              extrin_para (R row-major, p)
 *   dept_err, beam_err         globals of calcBodyVar (VH:179), applied after the first convergence (VS:675-681)
 *   scale_gravity              imupre_scale_gravity (PI:9): motion_blur (VS:522) and the re-preintegration
 *   point_notime               global point_notime (VS:550)
 *   noise_meas_diag6, noise_walk_diag6   noiseMeas / noiseWalk diagonals as for vba_imu_preintegrate
 *   states [W][25] in/out      x_buf;  covs [W][225] in: x_buf[i].cov (pvec_update, VS:680)
 *   imus [W-1][304] in/out     imu_pre_buf
 *   hess ((15W+3)^2) out       hess: the last damping_iter's Hessian (may be NULL)
 *   *converged                 the int return value of motion_init (converge_flag)
 *   eigvalue3 [3]              eigvalue of VS:744-745 (ascending; zeros if the convergence test never passed)
 *   *iterations                outer rounds started (iterCnt + 1 at the exit of the loop)
 *   *thresholds_left_relaxed   1 if the reference would leave the relaxed thresholds in its globals (the loop ended before the
 *                              round after the first convergence); the context keeps its own options either way
 *   round_log [max_rounds][5]  per round: [factor count, resis[0], resis[1], |x_buf[0].g|, converge_flag] after the round (may be
 *                              NULL; resis stay 0 in a round that breaks before the LM)
 *   pnt_out [pvec_cap][3], var_out [pvec_cap][9], pvec_offsets [W+1]   pvec_buf after the last round: compensated body points in the
 *                              reference's push order and their var (identity before the first convergence, world-frame pvec_update
 *                              after it); NULL pnt_out skips them.  pvec_offsets is always written when given; VBA_ERR_CAPACITY
 *                              when the rows exceed pvec_cap (checked before any work).
 * Argument errors are found before any device work and leave the context untouched.  Any other non-zero return leaves states, imus
 * and the other outputs undefined and the context with an empty map and factor store. */
int vba_motion_init(vba_ctx *ctx, int win_size, const int *pt_offsets, const double *pnt, const double *curv, const int *imu_offsets,
                    const double *imu, const double *beg_times, const double *ext_pose, double dept_err, double beam_err,
                    double scale_gravity, int point_notime, const double *noise_meas_diag6, const double *noise_walk_diag6,
                    double *states, const double *covs, double *imus, double *hess, int *converged, double *eigvalue3, int *iterations,
                    int *thresholds_left_relaxed, double *round_log, int max_rounds, double *pnt_out, double *var_out, int *pvec_offsets,
                    int pvec_cap);
/* Host only, no context.  The backward IMU propagation of Initialization::motion_blur (VS:508-544): xc = state_c with the biases of
 * state_l (VS:508-509), m deque rows imu [m][7] -> out [m-1][22] rows [offt, R(9), p(3), v(3), angvel_avr(3), acc_imu(3)] in push
 * order (time descending, offt = head time - beg_time): the table the initialisation blur reads. */
int vba_init_imu_poses(int m, const double *imu, const double *state_c, const double *state_l, double beg_time, double scale_gravity,
                       double *out);
/* Host only.  Initialization::align_gravity (VS:470-497) on states [n][25] in place. */
int vba_init_align_gravity(int n, double *states);

/* ------------------------------------------------------------------------------------------------
 * Hierarchical global BA ("next #3"), one keyframe window per call.  vba_hba_add_edge accepts any
 * wdsize >= 2: a window of the context's win_size (the bottom layers use 10, VS:3033) runs on the templated device
 * kernels; any other size — the top-level BA over all submaps, VS:3103-3113 — takes the sparse path (hashed per-keyframe
 * clusters, atomics Hessian, LM loop and dense LDL^T on the host).  vba_gba_build requires wdsize == win_size.
 * Keyframe clouds are passed ragged: pnt_local [offsets[wdsize]][3] holds keyframe i's points (its own frame, PCL float
 * values in doubles) in rows offsets[i]..offsets[i+1]; HOST or DEVICE memory.  gba_eigen_value_array is ALREADY INVERTED
 * (VS:3022-3024).
 *
 * vba_gba_build = OctreeGBA::cut_voxel for every keyframe (LR:439-479) + OctreeGBA_multi_recut (LR:483-537): fills the
 * context's factor store (what `LidarFactor voxhess(wdsize)` holds at VS:2889-2890).
 *
 * vba_hba_add_edge = VOXEL_SLAM::HBA_add_edge (VS:2822-3015) on an already filtered keyframe set: up to max_iter
 * rounds of {octree rebuild, Lidar_BA_Optimizer::damping_iter(xs, voxhess, &hess, resis, 4)} with the convergence
 * ladder of VS:2871-2915 (the last round uses the context's voxel_size / plane_eigen_value_thre / min_eigen_value),
 * poses [wdsize][12] in/out, then one edge per keyframe pair whose six diagonal Hessian entries are all >= 1e-6
 * (VS:2926-2951): edges_out rows = i, j, rot[9] = R_i^T R_j, tra[3] = R_i^T (p_j - p_i), v6[6] = 1/|H| — the arguments
 * of PGO_Edges::push (LR:247).  cloud_out (optional, capacity offsets[wdsize] rows) receives the submap cloud of
 * VS:2954-2989 (all points in keyframe 0's frame, down_sampling_voxel(voxel_size / 8)), cloud_count its per-voxel
 * counts.  resis_log (optional, [max_iter][2]) receives resis[0], resis[1] of every round.
 * Returns VBA_ERR_TOO_FEW_VOXELS where the reference prints "Too Less Voxel" and exits. */
int vba_gba_build(vba_ctx *ctx, int wdsize, const int *offsets, const double *pnt_local, const double *poses,
                  double gba_voxel_size, double gba_min_eigen_value, const double *gba_eigen_value_array);
int vba_hba_add_edge(vba_ctx *ctx, int wdsize, const int *offsets, const double *pnt_local, double *poses,
                     double gba_voxel_size, double gba_min_eigen_value, const double *gba_eigen_value_array, int max_iter,
                     int thread_num, double *edges_out, int *n_edges, double *cloud_out, int *cloud_count, int *n_cloud,
                     double *resis_log, int *n_log);

/* The optimisation work of thd_globalmapping (VS:3018-3141) over one map: bottom-layer windows of wdsize keyframes every
 * mgsize keyframes (10 / 5 in the reference, VS:3033-3034) on the poses x0, each yielding edges (edges1, the reference's
 * gba_edges1) and one submap (first keyframe's x0, the window's down-sampled cloud in that frame, VS:3084-3089); then the
 * top-level HBA_add_edge over all submaps with the keyframes' CURRENT poses poses_now (VS:3096-3110) -> edges2.  Rows as in
 * vba_hba_add_edge with global keyframe indices; cap1 / cap2 = row capacities of the outputs.  Queues, map switching and
 * the GTSAM graph stay with the caller. */
int vba_hba_global(vba_ctx *ctx, int n_kf, const int *offsets, const double *pnt_local, const double *poses_x0,
                   const double *poses_now, double gba_voxel_size, double gba_min_eigen_value,
                   const double *gba_eigen_value_array, int total_max_iter, int wdsize, int mgsize, double *edges1_out, int cap1,
                   int *n_edges1, double *edges2_out, int cap2, int *n_edges2);

/* ------------------------------------------------------------------------------------------------
 * Pose-graph optimisation: the two GTSAM call sites of the loop-closure thread on the device.
 * build_graph (VS:2078-2156) + ISAM2 {relinearizeThreshold, relinearizeSkip 1}: update(graph, initial) + (n_updates - 1) x update()
 * + calculateEstimate() (VS:2550-2561, VS:2769-2777), with the semantics of DESIGN.md §12.  poses [n][12] in/out (initial -> result).
 * edges [m][20] = i, j, rot[9], tra[3], var[6]: the row layout vba_hba_add_edge / vba_hba_global emit (indices remapped by the
 * caller to node ids, stepsizes[..] + id as VS:2144-2147).  priors [n_prior][19] = k, R[9], p[3], var[6].
 * stats (optional) [n_updates][3] = relinearised nodes, cost at θ before the solve, max ‖δ‖∞.
 * VBA_ERR_BAD_ARG: index out of range, i == j, var <= 0 or not finite, n_updates < 1.  VBA_ERR_SINGULAR: a connected component
 * without a prior, or a non-positive pivot (GTSAM throws IndeterminantLinearSystemException).  On any error poses are untouched.
 * Bit-identical run to run whatever vba_options::deterministic says (no floating-point atomics).
 * Device memory: the dense skeleton system over the K prior-holding or branching nodes takes 8 (6K)^2 bytes (1.15 GB at K = 2000,
 * 29 GB at K = 10000) on top of O(n + m) for the graph; both buffers are grow-only and stay with the context until vba_destroy.
 * VBA_ERR_CAPACITY (context still usable) when the device cannot hold them. */
int vba_pgo_optimize(vba_ctx *ctx, int n, double *poses, int m, const double *edges, int n_prior, const double *priors,
                     int n_updates, double relin_threshold, double *stats);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: voxels are sharded by root-voxel hash bucket; each rank evaluates its
 * shard and the packed [H | g | r] buffer is summed across ranks (the thread-sum of VM:571-581).
 * The reduction is RCCL inside the library (vba_rccl_init) or, for rehearsals without RCCL, a hook
 * supplied by the host program; both are stream-ordered on the context's stream.                  */
typedef int (*vba_allreduce_fn)(void *user, void *buf_dev, size_t n_doubles, void *stream);
int vba_set_allreduce(vba_ctx *ctx, vba_allreduce_fn fn, void *user);
/* RCCL inside the library: the context owns (vba_rccl_init) or adopts (vba_set_rccl_comm, an ncclComm_t) a communicator and issues
 * ncclAllReduce(ncclDouble, ncclSum) / ncclAllGather on its own stream — no host code in the LM loop.  Rank 0 calls
 * vba_rccl_get_unique_id (128 bytes, ncclUniqueId), the host program hands the bytes to every rank (any transport), every rank
 * calls vba_rccl_init, which also applies vba_set_shard(rank, n_ranks).  The hook above stays for CPU-side rehearsals (gloo). */
int vba_rccl_get_unique_id(void *out128);
int vba_rccl_init(vba_ctx *ctx, const void *unique_id128, int rank, int n_ranks);
int vba_set_rccl_comm(vba_ctx *ctx, void *nccl_comm);
/* Which rank owns root voxel (kx,ky,kz) out of n_ranks (pure function, usable without a device). */
int vba_shard_owner(int64_t kx, int64_t ky, int64_t kz, int n_ranks);
int vba_set_shard(vba_ctx *ctx, int rank, int n_ranks);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): average device time in microseconds of the named kernel family since
 * the last reset, from hipEvents recorded on the context's stream around each launch.             */
int vba_timing_enable(vba_ctx *ctx, int on);
/* Measurement aid for the rocprofv3 PMC passes: one launch that reads exactly (n_bytes rounded down to 32 KiB) bytes with the
 * factor store's access shape; its FETCH_SIZE calibrates the read-side counter correction (tools/prof_summary.py). */
int vba_timing_calibration_read(vba_ctx *ctx, size_t n_bytes);
/* Restrict the event bracketing to one kernel family (NULL / "" = all): two hipEventRecord calls per launch cost host
 * time, so the headline timed region brackets only the kernel whose roofline is reported. */
int vba_timing_select(vba_ctx *ctx, const char *name);
/* Bracket only every n-th launch of the selected family (n <= 1: every launch).  An event pair costs ~5 us of stream time on
 * this runtime, more than the kernel it brackets: the headline timed region samples instead of bracketing every launch. */
int vba_timing_sample_every(vba_ctx *ctx, int n);
/* Records an event pair around no work under the name "null": the overhead that every bracketed launch carries. */
int vba_timing_null_span(vba_ctx *ctx);
int vba_timing_reset(vba_ctx *ctx);
/* name in {"residual","hessian","reduce","solve","insert","recut","margi","init","loop"} ("init": the blur and normal-scatter launches of
 * vba_motion_init; "loop": one span per vba_btc_search_loop[_sessions] call and per vba_btc_icp_normal call); returns launches in *count. */
int vba_timing_get(vba_ctx *ctx, const char *name, double *total_us, int *count);

/* LM building blocks on device state (used by bench.py to time exactly K LM iterations, and by the
 * damping_iter entry points themselves): begin loads the poses, iterate runs one trip through the
 * loop body VM:441-494 / VM:643-710, end copies the refined poses back (all-NULL outputs: no synchronisation). */
int vba_lm_begin(vba_ctx *ctx, const double *poses, int thd_num);
int vba_lm_refresh_eigen(vba_ctx *ctx); /* device-side residual pass at the begin poses (re-creates eig/pcr_add state) */
/* Measurement aid: enqueues exactly one launch of the Hessian pass kernel (all voxels, at the begin poses, no reduction) on the
 * context's stream.  bench.py replays a batch of them from a HIP graph between one event pair. */
int vba_timing_launch_hessian(vba_ctx *ctx);
int vba_lm_iterate(vba_ctx *ctx, int *accepted, int *stop); /* NULL, NULL: enqueue only (no host synchronisation) */
int vba_lm_end(vba_ctx *ctx, double *poses, double *hess, double *resis2);
/* Diagnostic: one linear solve of an LM iteration on a system of the caller's choosing (tests/test_gpu_solve.py).  H (n x n,
 * row-major, exactly symmetric) and g (n) are the Hessian and gradient before the gauge; the production kernel solves
 * (H + u diag(H)) dx = -g with the loop's gauge rows (identity, zero right-hand side) and returns dx and the model decrease
 * q1 = 0.5 dx^T (u diag(H) dx - g) of every damping candidate b, candidate b using the damping b consecutive rejections lead to
 * (u <- u v, v <- 2 v): dx[b n + i], q1[b].
 *   VBA_SOLVE_LIDAR  k_lm_solve_m, n = 6W (W = 2..16), gauge rows 0..5, lm_spec candidates.  The system goes into the tile image
 *                    of the Hessian pass: every entry in the tiles, or (VBA_SOLVE_E_PACKED) each frame's 6 x 6 diagonal block in
 *                    the per-frame remainders only.
 *   VBA_SOLVE_LI     k_li_solve, n = 15W (+3 with VBA_SOLVE_GRAVITY), W = 2..16, gauge rows 0..14 (0..5 with gravity), lm_spec
 *                    candidates.  Pose-pose entries go into the lidar tiles, the rest into the compact IMU image (coefficient 1);
 *                    an entry coupling frames more than one apart that is not pose-pose is VBA_ERR_BAD_ARG.
 *                    VBA_SOLVE_DENSE_MASK updates every tile in every panel instead of skipping by structure.
 *   VBA_SOLVE_DENSE  big_damping_iter's solve (host pivot order, k_bigl_* on the device), n = 6W (W = 2..1024), gauge rows 0..5,
 *                    one candidate.
 * VBA_SOLVE_COPY_RAW launches the multi-rank form of the lidar / LI kernel (system read from the reduced buffer and saved), with
 * VBA_SOLVE_FROM_RAW the form that reads the saved copy after a rejected step.  The lidar and LI kernels end the factorisation
 * with the panel of the last live pivot (behind it lie only decoupled gauge rows, the right-hand-side row and padding; the solution
 * there is written as 0); VBA_SOLVE_ALL_PANELS runs every panel instead, the two must agree by value.  Non-finite input, a W out of range or an
 * asymmetric H: VBA_ERR_BAD_ARG with nothing launched.  The context's LM state is not touched. */
#define VBA_SOLVE_LIDAR 0
#define VBA_SOLVE_LI 1
#define VBA_SOLVE_DENSE 2
#define VBA_SOLVE_E_PACKED 1
#define VBA_SOLVE_COPY_RAW 2
#define VBA_SOLVE_FROM_RAW 4
#define VBA_SOLVE_GRAVITY 8
#define VBA_SOLVE_DENSE_MASK 16
#define VBA_SOLVE_ALL_PANELS 32
int vba_debug_solve(vba_ctx *ctx, int kind, int W, int flags, const double *H, const double *g, double u, double v, double *dx, double *q1);
/* Diagnostic: the IMU factor pass of the LI-BA loop (li_imu_body; with VBA_IMU_TRIAL also the trial-state residual of k_li_update)
 * once, on the caller's window (tests/test_gpu_imu.py).  states[W][25] and imus[W-1][304] are those of vba_li_ba_damping_iter; the
 * set-up (LM state, LiDev, the factor image with the host-inverted cov) is the code that call runs.  W must be the context's
 * win_size (2..16), gravity 0 or 1, n = 15W + 3 gravity.  The pass is launched in the form flags selects:
 *   0                 alone, as k_li_imu;
 *   VBA_IMU_RIDE_H2   as the extra workgroup of k_hessian2 over the context's factor store;
 *   VBA_IMU_RIDE_H3   as the extra workgroup of k_hessian3 (contexts with hessian_compact_tiles, W <= 10).
 * A riding form needs a pushed store and must be the lidar kernel the context selects for this window (k_hessian3 where it exists
 * for the context, else k_hessian2); otherwise VBA_ERR_BAD_ARG, so the caller knows which form ran.  Outputs, after the stream is
 * drained: h_dense[n * n] = the compact IMU image read through li_hb_get (no imu_coef, no lidar part, no gauge), g[n], rimu[0] =
 * sum_f r^T cov^-1 r at the states.  VBA_IMU_TRIAL launches k_li_update afterwards with the states in the trial slots, a zero lidar
 * residual and the fresh LM bookkeeping, and returns its sum in rimu[1] (0 without the flag).  covinv_out (may be NULL):
 * [W-1][225], the cov^-1 blocks the kernels read.  VBA_ERR_BAD_ARG with nothing launched: a NULL pointer other than covinv_out,
 * W not the context's, gravity not 0 / 1, an unknown flag, both riding flags, a non-finite input.  VBA_ERR_UNSUPPORTED: a sharded
 * context.  A pending LM call of the context is dropped. */
#define VBA_IMU_RIDE_H2 1
#define VBA_IMU_RIDE_H3 2
#define VBA_IMU_TRIAL 4
int vba_debug_li_imu(vba_ctx *ctx, int W, int gravity, int flags, const double *states, const double *imus, double *h_dense, double *g,
                     double *rimu, double *covinv_out);
/* Diagnostic: ONE point loop of a resident odometry update, and what it left in device memory (tests/test_gpu_odom_sums.py).  The
 * image is built by the code the real calls run (odom_ekf_begin on state [25] and cov [225], host arrays; done = 0, refind = 1), the
 * launches are those one iteration of the loop queues, the stream is drained, nothing of the context's state, covariance or map changes.
 *   VBA_ODOM_SUMS_VOXEL  the scan-to-map loop of vba_odom_lio_state_estimation_resident on the context's voxel map: pnt_body [n][3]
 *                        and var_body [n][9], host or device arrays; slices must be 0, cand and planes are not touched.
 *   VBA_ODOM_SUMS_KD     the loop of vba_odom_lio_state_estimation_kdtree_resident on the context's current point-cloud map, which is
 *                        not appended to: pnt_body [n][3]; var_body is not read.  slices = 0: the slice count the loop takes for a scan
 *                        of n points; 1..8: that many.  cand [slices][n][5]: the raw 64-bit candidates of the sliced search (float
 *                        distance bits << 32 | map index; index 0xFFFFFFFF = unfilled slot), so 8 * n * 5 words cover every choice;
 *                        planes [n][4]: (unit normal, distance) of the fit, (0, 0, 0, -1) = rejected.
 * Outputs of both, host arrays: partial [ceil(n / 256)][34], the per-workgroup sums [HTH upper (21) | HTz (6) | nnt upper (6) |
 * match_num] (kd: columns 27-32 zero), and sums [34], the reduction of k_odom_update over them stored by a one-workgroup launch of
 * the same code: column c by the seven lanes c + 34 g, lane t adding the elements t, t + 238, ... of the flat partials in that order,
 * then the seven group sums in group order.  On a voxel map never allocated the loop matches nothing: partial and sums are zero.
 * *slices_used (may be NULL): the slice count that ran (0 for VOXEL).  VBA_ERR_BAD_ARG with nothing launched: a NULL pointer that the
 * kind reads or writes, n < 1, a non-finite state, cov or host-array input, an unknown kind or slice count, KD on a map of fewer than
 * 100 points (the loop never searches one).  VBA_ERR_UNSUPPORTED: a sharded context. */
#define VBA_ODOM_SUMS_VOXEL 0
#define VBA_ODOM_SUMS_KD 1
int vba_debug_odom_sums(vba_ctx *ctx, int kind, int n, const double *pnt_body, const double *var_body, const double *state,
                        const double *cov, int slices, double *partial, double *sums, unsigned long long *cand, double *planes,
                        int *slices_used);
/* Diagnostic: plane_update (the centre, normal, radius and 6x6 covariance of a leaf's plane) alone, on caller-supplied leaves
 * (tests/test_gpu_plane.py).  The device function that the marginalisation runs is launched with one lane per leaf on scratch
 * buffers of this call; the context's map is neither read nor written.  Host arrays:
 *   in  [n][67]  pcr_add (Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N) | eig_value (3) | eig_vector (9, row-major, columns = eigenvectors) |
 *                cov_add (45: the upper triangle of the symmetric 9x9, row by row)
 *   out [n][43]  centre (3) | normal (3) | radius | plane_var (36, row-major)
 * The stream is drained.  VBA_ERR_BAD_ARG with nothing launched: a NULL pointer, n < 1 or n > 2^20. */
int vba_debug_plane_update(vba_ctx *ctx, int n, const double *in, double *out);
/* Diagnostic: one update of vba_pgo_optimize with n_updates = 1, every pass read back (tests/test_gpu_pgo_passes.py).  The plan, the
 * upload and the launches are the functions the production call runs; arguments, validation and error codes are those of
 * vba_pgo_optimize, and the caller's input arrays are left as given.  Host outputs, each may be NULL:
 *   slot [m + n_prior][121]  as k_pgo_linearize left them: Hii (36) | Hjj (36) | Hij (36) | gi (6) | gj (6) | cost
 *   *n_pairs, pairs [<= m][2]  the distinct node pairs (lower id, higher id), in the order of their blocks
 *   blk [n + n_pairs][36]    the assembled blocks: the n diagonal ones, then one per pair, rows = the lower node id
 *   g [n][6], dx [n][6]      the assembled gradient and the solved step
 *   *cost                    k_pgo_cost's sum
 *   poses_out [n][12]        theta (+) delta (k_pgo_relin as the last update)
 * The stream is drained. */
int vba_debug_pgo_step(vba_ctx *ctx, int n, const double *poses, int m, const double *edges, int n_prior, const double *priors,
                       double *slot, int *n_pairs, int *pairs, double *blk, double *g, double *dx, double *cost, double *poses_out);
/* Diagnostic: the passes of the any-window path (csrc/vba_kernels_big.hpp) one at a time on the context's sparse store, the store that
 * vba_hba_add_edge builds and optimises whenever wdsize != win_size (tests/test_gpu_big.py).  The store is CSR over voxels, one entry
 * per occupied (voxel, frame).  Every call drains the stream; none touches the context's LM state, its dense factor store or its map.
 *   vba_debug_big_load      replaces the store by the caller's: W frames (2..1024, the range of VBA_SOLVE_DENSE), V voxels, vptr[V + 1],
 *                           efr[E] (frame of every entry), ecl[E][10] (body cluster sums Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N), and per voxel
 *                           eig_val[V][3], eig_vec[V][9] (row-major, columns = eigenvectors), pcr_add[V][10].  Sizing and allocation are
 *                           the code big_build ends with; evox is the CSR row of each entry, eidx comes from k_big_eidx.  V = 0 is an
 *                           empty store (only vptr is read).  VBA_ERR_BAD_ARG with nothing launched and the previous store intact: a NULL
 *                           pointer, W out of range, V < 0, vptr not starting at 0 or not increasing (a voxel without an entry would make
 *                           the residual pass divide by N = 0; the build cannot produce one), efr not strictly increasing within a voxel
 *                           or outside [0, W), a non-finite input.
 *   vba_debug_big_build     big_build on the caller's clouds with the arguments of vba_hba_add_edge (points staged as that call stages
 *                           them); *V, *E = the size of the store it left.
 *   vba_debug_big_size      W, V, E of the current store (zeros when there is none).
 *   vba_debug_big_read      the store as it stands: vptr[V + 1], efr[E], evox[E], eidx[V][W] (entry of (voxel, frame) or -1), ecl[E][10],
 *                           eig_val, eig_vec, pcr_add as above.  Any pointer may be NULL.  After a residual pass the last three are what
 *                           that pass stored.
 *   vba_debug_big_hessian   big_hessian at poses[W][12] (R row-major | p): H[(6W)^2], g[6W], *r, and blockdiag[W][W][6], the output of
 *                           big_block_diagonals (the six diagonal entries of every 6 x 6 block; all vba_hba_add_edge reads of H).  slices:
 *                           voxel slices of k_big_syrk, 0 = the pass's own choice (what vba_hba_add_edge runs), k >= 1 = k; at most one
 *                           per chunk of 16 voxels either way.
 *   vba_debug_big_residual  big_residual at poses: *r; the eigen-data and sums it stored are read through vba_debug_big_read.
 * Read and the two passes return VBA_ERR_BAD_ARG without a store (no load or build yet); the passes also for a NULL pointer, a negative
 * slice count or non-finite poses.  All: VBA_ERR_UNSUPPORTED on a sharded context. */
int vba_debug_big_load(vba_ctx *ctx, int W, int V, const int *vptr, const int *efr, const double *ecl, const double *eig_val,
                       const double *eig_vec, const double *pcr_add);
int vba_debug_big_build(vba_ctx *ctx, int W, const int *offsets, const double *pnt_local, const double *poses, double gba_voxel_size,
                        double gba_min_eigen_value, const double *gba_eigen_value_array, int *V, int *E);
int vba_debug_big_size(vba_ctx *ctx, int *W, int *V, int *E);
int vba_debug_big_read(vba_ctx *ctx, int *vptr, int *efr, int *evox, int *eidx, double *ecl, double *eig_val, double *eig_vec,
                       double *pcr_add);
int vba_debug_big_hessian(vba_ctx *ctx, const double *poses, int slices, double *H, double *g, double *r, double *blockdiag);
int vba_debug_big_residual(vba_ctx *ctx, const double *poses, double *r);

/* ------------------------------------------------------------------------------------------------
 * Session-store formats either side of the path.  Host only, no context.
 *   FileReaderWriter::save_pcd (VS:166-179): <session>/<count>.pcd, pcl::io::savePCDFileBinary of PointXYZI (x y z from the
 *     scan's body-frame points, intensity 0); read back with pcl::io::loadPCDFile (VS:337-340).  vba_io_load_pcd reads
 *     DATA binary and DATA ascii files with x y z [intensity] among their fields; *n_out is the point count also when
 *     VBA_ERR_CAPACITY is returned (call with cap 0 to size the buffers).
 *   FileReaderWriter::save_pose (VS:181-204) / read_lidarstate (VH:268-307): alidarState.txt, one line per scan:
 *     t px py pz qx qy qz qw vx vy vz bgx bgy bgz bax bay baz gx gy gz v6[0..5], fixed notation, 6 decimals for t, 7 for the
 *     rest; nothing is written for fewer than 100 scans (VS:183-184); the reader accepts 8-, 20- and 26-column lines.
 *   states: n x 25 doubles (t, R row-major, p, v, bg, ba, g — the layout of vba_odom_*), v6: n x 6. */
int vba_io_save_pcd(const char *path, int n, const double *xyz);
int vba_io_load_pcd(const char *path, int cap, double *xyz, double *intensity /* may be NULL */, int *n_out);
int vba_io_save_pose(const char *path, int n, const double *states, const double *v6);
int vba_io_read_lidarstate(const char *path, int cap, double *states, double *v6 /* may be NULL */, int *n_out);

/* ------------------------------------------------------------------------------------------------
 * Loop retrieval and verification of the loop-closure thread (VS:2404-2541): the database half of
 * STDescManager (BTC.h, BTC.cpp) and icp_normal (loop_refine.hpp = LR).  Descriptors and plane clouds come from the caller or
 * from vba_btc_generate_stds below (GenerateSTDescs on the device).  A database hangs off a context
 * and runs on its stream; the loop-closure thread owns its own context.  Every result is the same bits
 * in every run; vba_options::deterministic plays no part here.  DESIGN.md §11.
 *
 * Descriptor row (STD, BTC.h:73-84), VBA_BTC_ROW_LEN doubles:
 *   [triangle_(3) center_(3) frame_number_ A.location_(3) B.location_(3) C.location_(3) A.summary_ B.summary_ C.summary_]
 * with the occupy_array_ of A, B, C as three 64-bit masks (bit k = entry k) in a separate uint64 [n][3] array.  angle_ is
 * not read by retrieval and is not passed.  summary_ must be an integer in [0, 255] (unsigned char), a mask may not set a bit
 * at or above vba_btc_config::occupy_len.
 * Plane cloud (PointXYZINormal): float [n][6] = x y z normal_x normal_y normal_z.
 * loop_std_pair is not returned: it is always empty in the reference (the push at BTC.cpp:1370-1388 is commented out). */
#define VBA_BTC_ROW_LEN 19

typedef struct vba_btc_config {   /* the fields of ConfigSetting (BTC.h:22-57) that retrieval reads, with their types */
  int skip_near_num;              /* skip_near_num_ */
  int candidate_num;              /* candidate_num_ (1..256; vba_btc_create refuses anything else) */
  float rough_dis_threshold;      /* rough_dis_threshold_ */
  float similarity_threshold;     /* similarity_threshold_ */
  float icp_threshold;            /* icp_threshold_ */
  float normal_threshold;         /* normal_threshold_ */
  float dis_threshold;            /* dis_threshold_ */
  int occupy_len;                 /* entries of occupy_array_ ((proj_dis_max_ - proj_dis_min_) / proj_image_high_inc_ = 50), <= 64 */
} vba_btc_config;

typedef struct vba_btc_db vba_btc_db;

typedef struct vba_btc_result {   /* SearchLoop's out-parameters */
  int loop_id;                    /* loop_result.first: the matched frame, -1 = none */
  double score;                   /* loop_result.second (0 with loop_id -1) */
  double t[3];                    /* loop_transform.first  (valid when loop_id >= 0) */
  double R[9];                    /* loop_transform.second, row-major */
} vba_btc_result;

typedef struct vba_btc_candidate {/* one entry of candidate_matcher_vec of the last search, for tests */
  int frame;                      /* match_id_.second */
  int votes;                      /* match_array[frame] */
  int match_len;                  /* match_list_.size() (equals votes) */
  int max_vote_index;             /* winning sampled index of candidate_verify */
  int max_vote;
  double score;                   /* verify_score (-1 when max_vote < 4) */
} vba_btc_candidate;

/* read_parameters (BTC.cpp:3-68), the retrieval fields only.  Host only. */
int vba_btc_default_config(int is_high_fly, vba_btc_config *cfg);
/* new STDescManager(config_setting).  VBA_ERR_NO_DEVICE without a HIP device; VBA_ERR_BAD_ARG for occupy_len > 64. */
int vba_btc_create(vba_ctx *ctx, const vba_btc_config *cfg, vba_btc_db **out);
/* A database belongs to its context: destroy every database of a context before vba_destroy(ctx). */
void vba_btc_destroy(vba_btc_db *db);
/* Capacity hint (no reference counterpart): size the database for `stds` descriptors (rows, cell table, chunks), `frames` plane
 * clouds of `cloud_points` points in all and a match list of `matches` pairs, so that a session that stays below them never
 * re-allocates.  Results do not depend on it.  Databases grow by doubling without it. */
int vba_btc_reserve(vba_btc_db *db, int stds, int frames, int64_t cloud_points, int matches);
/* config_setting_.skip_near_num_ = v: the writes that close a session (VS:410, VS:2242) */
int vba_btc_set_skip_near_num(vba_btc_db *db, int v);
/* plane_cloud_vec_.push_back + header.seq inside GenerateSTDescs (BTC.cpp:156-168).  Frame index = number pushed before. */
int vba_btc_push_plane_cloud(vba_btc_db *db, int n, const float *xyz_normal, int seq);
int vba_btc_num_frames(vba_btc_db *db);
int vba_btc_frame_seq(vba_btc_db *db, int frame, int *seq);
/* AddSTDescs (BTC.cpp:258-277).  A frame_number_ outside [0, frames pushed) is VBA_ERR_BAD_ARG. */
int vba_btc_add_stds(vba_btc_db *db, int n, const double *rows, const uint64_t *bits);
/* SearchLoop (BTC.cpp:205-256) of the n query rows against db; pl_cur = plane cloud cur_frame of cur_db (VS:2421 passes
 * std_manager->plane_cloud_vec_.back()).  n == 0 gives (-1, 0). */
int vba_btc_search_loop(vba_btc_db *db, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur_db, int cur_frame,
                        vba_btc_result *result);
/* the loop `for (id = 0; id <= cur_id; id++) SearchLoop(...)` (VS:2417-2421): one query upload, every database enqueued, one host
 * synchronisation; results[k] is the result of dbs[k].  All databases must hang off the same context. */
int vba_btc_search_loop_sessions(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits,
                                 const vba_btc_db *cur_db, int cur_frame, vba_btc_result *results);
/* icp_normal(pl_src, pl_tar, pose, icp_eigval) (LR:47-139) at its call site VS:2434, both clouds resident: t, R (row-major) are
 * the pose, updated in place; *ok = the return value, eig = eigenvalues of mat_norm (ascending), *iters = iterations run. */
int vba_btc_icp_normal(vba_btc_db *src_db, int src_frame, vba_btc_db *tar_db, int tar_frame, double *t, double *R, double icp_eigval,
                       int *ok, double *eig, int *iters);
/* Diagnostic: ONE iteration of vba_btc_icp_normal, every pass read back (tests/test_gpu_icp_passes.py; declared here, not with the
 * other vba_debug_* entries, because it takes database handles).  The 1-NN launch, the gate-and-accumulate launch and the step
 * launch are queued by the host function the loop of vba_btc_icp_normal calls twenty times; the outputs leave the production
 * kernels through pointers that are null in that loop.  *state is the iteration's state, in and out: vba_btc_icp_normal starts
 * from (R, t, paras = {0.2, 0.2, 0.5, 3}, everything else 0), and chaining this call from there reproduces it bit for bit.
 * slices: runs of 256-point tiles the target is cut into for the 1-NN launch; 0 = the call's own choice (what the loop runs),
 * k >= 1 = k.  With ntile = ceil(nt / 256) and nb = max(ceil(ns / 256), 1), k > max(ntile, 1) or nb * k > 1024 is refused.
 * Host outputs, each may be NULL, each left as the caller gave it when state->done is set on entry (the launches return at once):
 *   key [ns]           the merged 1-NN word of every source point: float distance bits << 32 | index in the target cloud, ~0 = none
 *   gate [ns]          1 where the point passed the four gates and entered the sums
 *   partial [nb][35]   per workgroup of 256 points: Hess upper (21) | JacT (6) | resi | match_num | mat_norm upper (6)
 *   sums [35]          the column sums of partial in workgroup order, as the step forms them
 *   dx [6]             the solved step (rotation | translation)
 *   *slices_used       the slice count that ran
 * The stream is drained.  VBA_ERR_BAD_ARG with nothing launched and *state untouched: a NULL database or state, databases of two
 * contexts, a frame out of range, a slice count outside the plan.  VBA_ERR_UNSUPPORTED: a sharded context. */
typedef struct vba_btc_icp_state {
  double R[9], t[3], paras[4];    /* pose (R row-major), thresholds: normal_inc, normal_add, point_to_plane, point_to_point */
  int is_conv, done, iters, pad;  /* is_converge; the loop has ended; iterations run */
  double mat[6], eig[3];          /* mat_norm of the last iteration (xx xy xz yy yz zz); its eigenvalues once done is set */
} vba_btc_icp_state;
int vba_debug_btc_icp_pass(vba_btc_db *src_db, int src_frame, vba_btc_db *tar_db, int tar_frame, vba_btc_icp_state *state, int slices,
                           unsigned long long *key, unsigned char *gate, double *partial, double *sums, double *dx, int *slices_used);
/* candidates of the last search on db (*n = how many; at most cap written) */
int vba_btc_last_candidates(vba_btc_db *db, int cap, vba_btc_candidate *out, int *n);

/* ------------------------------------------------------------------------------------------------
 * Descriptor generation (GenerateSTDescs, BTC.cpp:156-203, with BTC.cpp:279-1126) on the device.  The input is the keyframe's
 * merged cloud (PointXYZI x y z as float [n][3], host memory, finite).  One call is one stream-ordered sequence with a single host
 * synchronisation at the end (unless it outgrows its buffers: vba_btc_gen_reserve); the plane cloud goes straight into the
 * database's cloud storage.  DESIGN.md §11a.
 *
 * Order contract (the reference iterates unordered_maps; this fixes the order, and results are the same bits in every run):
 *  1. voxel key (int64_t)(p / voxel_size - (p / voxel_size < 0 ? 1 : 0)) in double from the float point (|key| < 2^20, else
 *     VBA_ERR_BAD_ARG); voxels ordered by the index of their first point; a voxel's points in input order; centre and covariance
 *     are the sequential sums in that order (sum p p^T / N - c c^T); a voxel is fitted when it has MORE than voxel_init_num points.
 *  2. plane fit: the project's symmetric 3x3 solver (direct path + Jacobi fallback, correctly rounded primitives); normal sign:
 *     the component of largest magnitude is positive, the lowest index wins a tie (Eigen's EigenSolver sign is not reproduced:
 *     a deviation; the sign decides the projection image's y axis).
 *  3. plane cloud and origin_list in voxel order; get_project_plane / merge_plane replay the greedy id assignment (iter
 *     descending, iter2 ascending); each group folds its members in ascending index from its first; both sorts by points_size_
 *     are stable.
 *  4. extract_binary: per-cell sums in the order of the kept points; the first strict maximum of a 5x5 segment in x-then-y
 *     order; corners in (x segment, y segment) order.  A point whose height index equals cut_num (dis near proj_dis_max) counts
 *     in the cell but sets no occupancy bit.
 *  5. neighbours (NMS radius search, generate_std kNN) exact in float: squared L2 over x then y then z, ties to the earlier index,
 *     radius test d^2 < (float)(r r); kNN takes min(K, corners) neighbours.
 *  6. triangles: the key is (int64_t)(float)(side * 1000); the first in (i, m, n) order wins; output in emission order.
 * An empty origin_list takes the single_plane branch (normal (0, 0, 1) through the first point); n == 0 pushes an empty plane
 * cloud and gives no descriptors.  angle_ is not produced. */
typedef struct vba_btc_gen_config {   /* the ConfigSetting fields (BTC.h:22-46) GenerateSTDescs reads, with the reference's types */
  int useful_corner_num;
  float plane_merge_normal_thre, plane_merge_dis_thre, plane_detection_thre, voxel_size;
  int voxel_init_num, proj_plane_num;
  float proj_image_resolution, proj_image_high_inc, proj_dis_min, proj_dis_max, summary_min_thre;
  int line_filter_enable, touch_filter_enable;
  float descriptor_near_num, descriptor_min_len, descriptor_max_len, non_max_suppression_radius, std_side_resolution;
} vba_btc_gen_config;

/* read_parameters (BTC.cpp:3-68), the generation fields.  Host only. */
int vba_btc_default_gen_config(int is_high_fly, vba_btc_gen_config *cfg);
/* vba_btc_get_gen_config reads the current one back.  A database starts with vba_btc_default_gen_config(0).  VBA_ERR_BAD_ARG outside the supported range: useful_corner_num >= 1,
 * voxel_size > 0, voxel_init_num >= 0, 1 <= proj_plane_num <= 8, proj_image_resolution > 0, proj_image_high_inc > 0,
 * 3 <= (int)descriptor_near_num <= 32, 0 <= descriptor_min_len, descriptor_max_len <= 2000, std_side_resolution > 0. */
int vba_btc_set_gen_config(vba_btc_db *db, const vba_btc_gen_config *cfg);
int vba_btc_get_gen_config(const vba_btc_db *db, vba_btc_gen_config *cfg);
/* GenerateSTDescs(input_cloud, stds_vec, id): pushes the plane cloud with seq = id (as vba_btc_push_plane_cloud would) and writes
 * *n_stds descriptor rows and masks in the layout vba_btc_add_stds / vba_btc_search_loop* take, frame_number_ = current_frame_id_
 * = the number of vba_btc_add_stds calls on db so far.  cap (rows) must be >= useful_corner_num * C(K - 1, 2), K =
 * (int)descriptor_near_num, and cut_num = (int)((proj_dis_max - proj_dis_min) / proj_image_high_inc) (49 for both shipped
 * configurations) must be <= the database's occupy_len; otherwise VBA_ERR_BAD_ARG with no side effect (no plane cloud pushed). */
int vba_btc_generate_stds(vba_btc_db *db, int n, const float *xyz, int id, int cap, double *rows, uint64_t *bits, int *n_stds);
/* read back plane cloud `frame` (float [n][6]); *n = its size, at most cap points written */
int vba_btc_plane_cloud(vba_btc_db *db, int frame, int cap, float *xyz_normal, int *n);
/* binary_list of the last vba_btc_generate_stds (for tests): loc_summary [n][4] = location_ x y z, summary_; bits [n] */
int vba_btc_last_corners(vba_btc_db *db, int cap, double *loc_summary, uint64_t *bits, int *n);
/* Capacity hint for generation (no reference counterpart): buffers for clouds of up to `points` points (voxel buffers are bounded
 * by it), projection images of `cells` cells (<= 2^24), and database room for the plane clouds and offsets of `frames` more calls,
 * so that such calls make no device or pinned-host allocation.  Results do not depend on it.  Without it buffers grow by doubling;
 * a call whose projection image or corner list outgrows its buffer grows it and runs its sequence once more (a second
 * synchronisation).  A projection image above 2^24 cells (points far out in the plane within proj_dis_max of it) is refused with
 * VBA_ERR_CAPACITY before anything is allocated for it. */
int vba_btc_gen_reserve(vba_btc_db *db, int64_t points, int64_t cells, int frames);
/* device and pinned-host allocations made by generation on db so far (its own buffers and the growth of the database's plane-cloud
 * storage and offset table in vba_btc_generate_stds), and the bytes of the generator's device buffers */
int vba_btc_gen_allocations(vba_btc_db *db, int *count, int64_t *bytes);

/* ------------------------------------------------------------------------------------------------
 * Keyframe store: the counterpart of `vector<Keyframe*> *keyframes`, one store per session, resident in HBM.
 * A keyframe is built on the device from the scans of its window, kept there, and read from there by keyframe_loading
 * (VS:1379-1438), descriptor generation (VS:2387-2406, VS:384-409) and the hierarchical BA (VS:2888): points cross the host
 * boundary once, as scans.
 *
 * Layout: one contiguous ragged array double [N][3] of keyframe points in the keyframe's own frame (PCL float values carried in
 * doubles: the form vba_hba_* and vba_map_cut_voxel_fix take), a parallel float [N][3] of covariance diagonals (normal_x/y/z);
 * on the host int offsets[n_kf + 1] and per keyframe x0 (pose layout), id, jour, exist.
 *
 * Growth and locking: the device arrays are grow-only; growing allocates new blocks, copies device to device and frees the old
 * ones after a synchronise, so THE ARRAYS MOVE.  A store is not synchronised internally: calls on one store, and any reader of
 * the pointers vba_kf_clouds returned, must be excluded from vba_kf_build / vba_kf_reserve / vba_kf_load* by the caller's lock,
 * as mtx_keyframe does for the reference's vector.  After vba_kf_reserve(points, keyframes, merge_points) no call below
 * allocates device or pinned-host memory of the store while the session holds at most `points` kept points in `keyframes`
 * keyframes, no merge (a build's scans, a window of vba_kf_generate_stds, a keyframe of vba_kf_load) exceeds `merge_points`
 * points and no build merges more than 64 scans (vba_kf_allocations counts them, as vba_btc_gen_allocations does).  The store
 * owns its buffers and nothing else; destroy it before its context.
 *
 * Order of operations of the merge (part of the interface; no product below is fused with a sum, on either side).
 * With xc = the pose of the last cloud, on the host per cloud i:
 *   dR[r][c] = (xcR[0][r]*R_i[0][c] + xcR[1][r]*R_i[1][c]) + xcR[2][r]*R_i[2][c]
 *   d_k = p_i[k] - xc_p[k];   dp[r] = (xcR[0][r]*d_0 + xcR[1][r]*d_1) + xcR[2][r]*d_2
 * on the device per point: q[r] = ((dR[r][0]*x + dR[r][1]*y) + dR[r][2]*z) + dp[r].  The covariance is carried over unrotated,
 * as the reference does (VS:2366-2370); clouds are concatenated in order i = 0..k-1. */
typedef struct vba_kf_store vba_kf_store;
int vba_kf_create(vba_ctx *ctx, vba_kf_store **out);
void vba_kf_destroy(vba_kf_store *s);
int vba_kf_reserve(vba_kf_store *s, int64_t points, int keyframes, int64_t merge_points);
int vba_kf_allocations(vba_kf_store *s, int *count, int64_t *bytes);
int vba_kf_size(vba_kf_store *s);   /* keyframes->size() */
/* The keyframe of VS:2354-2397 (online, var != NULL) or VS:348-372 (offline, var == NULL) from k scans: rows offsets[i]..offsets[i+1]
 * of pnt [][3] (and var [][9]) are scan i, body frame, HOST or DEVICE memory as for vba_map_cut_voxel; poses [k][12], xc = poses[k-1]
 * becomes the keyframe's x0.  Of a host var only the three diagonal doubles per point are uploaded.
 * Kept cloud: var != NULL: down_sampling_pvec (VM:39-81) of the merged doubles at voxel_size (the caller passes voxel_size / 10);
 * var == NULL: down_sampling_voxel (TL:201) of the merged points narrowed to float, diagonals zero (voxel_size >= 0.001).  Both
 * follow the contract of vba_scan_down_sampling_*: float-narrowed key, voxels in first-occurrence order, mean rounded once to
 * float, vba_options::deterministic of the store's context honoured.  The result is written straight into the store; *n_points =
 * its size.
 * Descriptors: with db != NULL (same device) the merged cloud is narrowed to float (VS:2390-2397) straight into the generator's
 * point buffer and vba_btc_generate_stds(db, n, ., id, cap, rows, bits, n_stds) runs on it: outputs, side effects, capacity rules
 * and errors are that call's.  The merged cloud never reaches the host.
 * Stream-ordered; synchronises once before returning (twice when a generator buffer has to grow; once more when db hangs off
 * another context, whose stream waits for the merge through an event).  After it returns other contexts on the device may read the
 * keyframe.  The keyframe is committed (offset, x0, id, jour, exist = 0) only after success; argument errors (k < 1, offsets not
 * non-decreasing, a non-finite pose, cap below the generator's bound) are found before any device work, and any error leaves
 * the store and db as they were. */
int vba_kf_build(vba_kf_store *s, int k, const int *offsets, const double *pnt, const double *var, const double *poses, double voxel_size,
                 int id, double jour, vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds, int *n_points);
/* per-voxel point counts of the last vba_kf_build, in the kept cloud's order (for tests); *n = their number, at most cap written */
int vba_kf_last_counts(vba_kf_store *s, int cap, int *counts, int *n);
/* Descriptors of a window of stored keyframes (VS:384-409): keyframes [first, first + count) merged from the store into the frame of
 * keyframe first+count-1's x0 (the arithmetic above, on the stored float values), narrowed to float and generated with that
 * keyframe's id.  No point crosses the host boundary.  Otherwise as vba_btc_generate_stds. */
int vba_kf_generate_stds(vba_kf_store *s, int first, int count, vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds);
/* kf->x0 = scanPoses[kf->id]->x for keyframes [first, first + n) (VS:2582-2587, VS:2798-2803) */
int vba_kf_set_poses(vba_kf_store *s, int first, int n, const double *poses /* [n][12] */);
int vba_kf_get(vba_kf_store *s, int k, double *pose12, int *id, double *jour, int *exist, int *n_points);   /* any output may be NULL */
/* VS:2628-2647: exist = 1 for keyframes below n_hist and 0 for the rest, the positions x0.p of the first n_hist keyframes
 * snapshot as floats (pl_kdmap), history_kfsize = n_hist.  n_hist = 0 switches loading off (the subsize <= init_num case). */
int vba_kf_set_history(vba_kf_store *s, int n_hist);
int vba_kf_history_size(vba_kf_store *s);   /* history_kfsize */
/* The body of keyframe_loading for keyframe k (VS:1407-1432): world = x0.R p + x0.p in the operation order above from the stored
 * values, inserted in stored order as fixed points with vba_map_cut_voxel_fix's semantics into map_ctx's map, from HBM; exist = 0.
 * map_ctx may be another context on the same device (VBA_ERR_BAD_ARG for another device); the work runs on ITS stream and the call
 * synchronises it once (the map's counter read-back). */
int vba_kf_load(vba_kf_store *s, int k, vba_ctx *map_ctx, double jour);
/* keyframe_loading(jour) (VS:1379-1438) around p3 = x_curr.p: returns at once while history_kfsize <= 0; otherwise the snapshot
 * positions within `radius` (10 in the reference), nearest first, and the first one whose keyframe has exist != 0 is loaded
 * (vba_kf_load) and history_kfsize decremented: at most one load per call.  *loaded = its index, -1 = none.
 * Rule chosen here (the reference leaves it to FLANN, which is not restated): the squared distance is accumulated x, y, z in float
 * between the float snapshot and (float)p3; a position is inside when d2 < (float)(radius * radius), so a point exactly on the
 * sphere is outside; equal distances are taken in ascending keyframe index.  The search runs on the host, the load on the device. */
int vba_kf_load_nearby(vba_kf_store *s, vba_ctx *map_ctx, const double *p3, double radius, double jour, int *loaded);
/* keyframe k to the host (tests, save_pcd): xyz [cap][3], vardiag [cap][3] (either may be NULL); *n = its size */
int vba_kf_read(vba_kf_store *s, int k, int cap, double *xyz, float *vardiag, int *n);
/* Zero copy: the store's device array and host offsets are the (offsets, pnt_local) arguments of vba_gba_build / vba_hba_add_edge /
 * vba_hba_global, which accept a device pnt_local: vba_hba_global(ctx, n, offsets, d_pnt, ...) on these pointers replaces the
 * upload of the keyframe clouds.  For a window starting at keyframe f pass d_pnt + 3 * offsets[f] and offsets rebased to
 * offsets[f].  The pointers are valid until the next call that may grow the store (see "Growth and locking"). */
int vba_kf_clouds(vba_kf_store *s, const double **d_pnt, const int **offsets, int *n_kf);

/* ---- ResultOutput::pub_globalmap (VS:110-154): the global map of one or more sessions, from the stores.
 *
 * vba_kf_export_plan is HOST ONLY (no context, no device, like vba_io_*): which points are exported and where the messages are cut.
 *   sizes[k]      point count of keyframe k of the sequence "all keyframes of all exported sessions in publication order" (the loop
 *                 over ids at VS:126): the differences of the offsets vba_kf_clouds returns, store after store.
 *   jump == 0     the reference's rule (VS:116-124): psize = sum of sizes, jump = psize / (10 * interval_size) + 1 in integer
 *                 division; interval_size is 5e6 there.  The reference holds psize in a 32-bit unsigned, which wraps; here the sum is
 *                 formed in 64 bits and a sum of 2^32 or more is VBA_ERR_BAD_ARG.  jump >= 1 is used as given (no limit on the sum).
 *   *jump_out     the jump in force.
 *   kf_begin      [n_kf + 1]: keyframe k contributes its points j = 0, jump, 2 jump, ... < sizes[k] (VS:133; the stride restarts
 *                 at every keyframe), that is ceil(sizes[k] / jump) points; kf_begin[k] = exported points before keyframe k,
 *                 kf_begin[n_kf] = the total.
 *   messages      VS:145-153: after each keyframe a message ends when the points accumulated since the last cut are STRICTLY MORE than
 *                 interval_size; one final message always follows and may be empty (pl is published unconditionally at VS:153).
 *                 msg_end_kf[m] = one past the last keyframe of message m: message m is exactly the exported points
 *                 [kf_begin[msg_end_kf[m-1]], kf_begin[msg_end_kf[m]]) (msg_end_kf[-1] = 0).  *n_msgs = the number of messages,
 *                 always; at most cap_msgs entries are written (n_kf + 1 always suffices).
 * The empty publish that clears the display (VS:113) stays with the node.
 * VBA_ERR_BAD_ARG, with nothing written: n_kf < 0, a negative size, interval_size < 1, jump < 0, a NULL output (msg_end_kf may be
 * NULL when cap_msgs == 0). */
int vba_kf_export_plan(int n_kf, const int *sizes, int64_t interval_size, int jump, int *jump_out, int64_t *kf_begin /* [n_kf + 1] */,
                       int cap_msgs, int *msg_end_kf /* [cap_msgs] */, int *n_msgs);
/* Exported points [begin, begin + count) of the sequence the plan defines for the keyframes of stores[0], then stores[1], ... (the
 * loop over ids, VS:126-151), as records x y z intensity of four floats; intensity[s] takes the place of pp.intensity = id (VS:128).
 * world = x0.R p + x0.p with the store's CURRENT x0 (what vba_kf_set_poses last wrote) in the operation order stated above for the
 * merge and used by vba_kf_load: q[r] = ((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + p[r], every product and sum rounded on its own,
 * nothing contracted; each coordinate is then narrowed to float once (pp.x = vv[0], VS:139-141).  This order is part of the interface.
 * xyzi [count][4] is HOST or DEVICE memory (a device buffer 16-byte aligned).  The work runs on ctx's stream; the stores may hang
 * off other contexts on the same device (another device: VBA_ERR_BAD_ARG).  Host memory: the records pass through a staging buffer
 * of the context in passes of at most 2^22 records and the call synchronises once, at its end.  Device memory: stream-ordered, no
 * synchronisation, the buffer may be consumed by later work on that stream.  (The per-keyframe table goes up through a ring of four
 * pinned images; a call waits for the upload of the fourth call before it only if that is still pending.)  The table and the
 * staging buffer belong to the context, grow by doubling when an export needs more and are never allocated per call.
 * The stores are read and nothing in them changes: no exist flag, no pose, no point.  The caller excludes vba_kf_build /
 * vba_kf_reserve / vba_kf_load* on these stores for the duration of the call ("Growth and locking").  With a DEVICE xyzi the call
 * returns while the gather is still queued: the exclusion then lasts until that work on ctx's stream has completed (vba_synchronize
 * (ctx), or an event the caller recorded behind the call), because a build or reserve that grows a store waits only for the store's
 * own context before it frees the old arrays.
 * VBA_ERR_BAD_ARG before any device work, xyzi untouched: n_stores < 1, a NULL store or intensity, jump < 1, begin < 0, count < 0,
 * begin + count beyond the plan's total, count > 0 with a NULL xyzi.  count == 0 is a success that does nothing. */
int vba_kf_export_world(vba_ctx *ctx, int n_stores, vba_kf_store *const *stores, const float *intensity /* [n_stores] */, int jump,
                        int64_t begin, int64_t count, float *xyzi /* [count][4], HOST or DEVICE */);

/* ---- The global map voxel-down-sampled: down_sampling_voxel (TL:201-238) over the exported records, at the
 * stores' current poses, without the records leaving the device.  Overlap between keyframes is removed: one record per voxel.
 *
 * The sequence S is exactly the records vba_kf_export_world(ctx, n_stores, stores, intensity, jump, 0, total, ...) would write:
 * stores in order, every keyframe's stride restarting at its point 0, world = x0.R p + x0.p at the CURRENT x0 in the uncontracted
 * order stated there, each coordinate narrowed once to float.  S is never written to memory.
 * Voxel of a record: TL:209-216 on the FLOAT coordinates: per axis loc = (float)(v / voxel_size), loc < 0 -> loc - 1, truncated
 * toward zero; 21 bits per axis are kept (the packing of every down-sampler of this library; both quirks are the reference's).
 * Output: one record per voxel, in ascending index of the voxel's FIRST record in S (first-occurrence order):
 *   x y z      = (float)(s * (1.0 / (double)cnt)), s the f64 sum of the voxel's float coordinates, cnt their number
 *   intensity  = that of the voxel's first record
 *   counts[i]  = cnt                                             (counts may be NULL)
 * Voxels with cnt < min_count (min_count >= 1) are left out, the order of the rest is unchanged; *n_out = the number kept.
 * Sum order.  vba_options::deterministic = 1: every sum is the chain ((0 + a_0) + a_1) + ... in the order of S, no f64 atomic is
 * on the path, and the result of a call is a function of its inputs bit for bit.  Default: f64 atomics form the sums, as in every
 * other down-sampler here, and two calls may differ.  After the narrowing the order is visible only at a float rounding boundary:
 * two f64 sums of the same cnt < 2^26 floats differ by less than 2 cnt 2^-53 sum|a|, far below half a float ulp, so the two
 * results are the same float or adjacent floats.
 * Capacity: more kept voxels than `cap` is VBA_ERR_CAPACITY with *n_out = the number needed, xyzi and counts untouched;
 * cap == 0 with xyzi == NULL is the size query (VBA_OK, *n_out set).  An S of 2^31 records or more is VBA_ERR_CAPACITY before any
 * device work (indices into S are 32-bit in the work arrays; indices into the stores and the output are 64-bit).
 * xyzi [cap][4] and counts [cap] are both HOST or both DEVICE memory (a device xyzi 16-byte aligned).  The work runs on ctx's
 * stream.  The host needs the count, so every call waits for the stream once; a device result is then written stream-ordered,
 * without a second wait; a host result passes through the context's staging buffer (whole, 20 bytes per voxel) and the call returns
 * when it has arrived.
 * Work arrays: a table of 16-byte slots and the sums (24 bytes per slot), a power of two >= 2 |S| slots of each (no overflow
 * path), 4 bytes per record, a deterministic context 12 bytes per record and the sort's scratch more.  They belong to the context,
 * _reserve(max_points) sizes them, the per-keyframe table and the host staging for an S (and a result) of that length, a call that
 * needs more doubles them after a synchronise, and nothing is allocated per call.  _allocations: allocations made and bytes
 * requested for this feature so far (cumulative, as vba_scan_frame_allocations); more than 1024 non-empty keyframes grow the
 * export's table by doubling, which is counted too.
 * The stores are only read; the locking rule is that of vba_kf_export_world (a device xyzi: until the work on ctx's stream is done).
 * VBA_ERR_BAD_ARG before any device work, outputs untouched: the argument errors of vba_kf_export_world (n_stores < 1, a NULL
 * store or intensity, a store of another device), jump < 1, min_count < 1, cap < 0, a NULL n_out, cap > 0 with a NULL xyzi,
 * voxel_size < 0.001 (the reference leaves such a cloud alone, TL:203: that caller wants vba_kf_export_world), a misaligned device
 * xyzi, counts on the other side.  Stores without keyframes and empty keyframes are valid: *n_out = 0. */
int vba_kf_voxel_export_reserve(vba_ctx *ctx, int64_t max_points);
int vba_kf_voxel_export_allocations(vba_ctx *ctx, int *n_allocs, int64_t *bytes);
int vba_kf_voxel_export(vba_ctx *ctx, int n_stores, vba_kf_store *const *stores, const float *intensity /* [n_stores] */, int jump,
                        double voxel_size, int min_count, int64_t cap, float *xyzi /* [cap][4], HOST or DEVICE */,
                        int *counts /* [cap], same side as xyzi, may be NULL */, int64_t *n_out);

/* ---- The global map as surfels / NDT cells: per voxel of the map above a mean, a covariance and a normal that
 * points to the sensor, fitted on the device.  What a mesher, a surfel renderer, an NDT registration against a prior map reads.
 *
 * Sequence, voxels, order, filter: exactly vba_kf_voxel_export's.  The same sequence S of float records, the same voxel key with
 * both inherited quirks, one output per voxel in ascending index of the voxel's first record in S, voxels with cnt < min_count left
 * out, counts[i] = cnt.  For the same arguments *n_out, counts and the order are identical to vba_kf_voxel_export.
 * Mean: c = s * (1.0 / (double)cnt), s the f64 sum of the voxel's float coordinates; c stays a double.
 * Covariance, two passes, centred on c: for every member a of the voxel d = (double)a - c; the six products d_i d_j (i <= j, order
 * xx xy xz yy yz zz) are each rounded on their own, nothing contracted, and summed into M; C = M * (1.0 / (double)cnt);
 * cov[i] = C as doubles (cov may be NULL).  No raw moment sum(a a^T) / cnt - c c^T is formed anywhere: at the coordinates a long
 * session reaches it cancels.
 * Fit: the ascending eigenvalues l0 <= l1 <= l2 of C and the eigenvector of l0, by the library's symmetric 3x3 solver built from
 * correctly rounded operations only (csrc/vba_eig3.hpp in its IEEE form with cyclic Jacobi sweeps as the fallback, the plane fit of
 * vba_btc_generate_stds); negative rounding residue in an eigenvalue is clamped to 0.  A host build of csrc/vba_surfel_fit.hpp
 * without contraction gives the same bits from the same C.
 * Record, 12 floats (48 bytes), each double narrowed to float once:
 *   [0..2]  c: the x y z of vba_kf_voxel_export            [3]     intensity of the voxel's first record
 *   [4..6]  unit eigenvector of l0, the normal             [7..9]  sqrt l0, sqrt l1, sqrt l2
 *   [10]    l0 / (l0 + l1 + l2), 0 when the trace is 0     [11]    (float)cnt
 * Orientation: the normal n points toward the sensor, that is toward x0.p of the keyframe of the voxel's FIRST record: when
 * (n_x (p_x - c_x) + n_y (p_y - c_y)) + n_z (p_z - c_z) < 0, in double and uncontracted, n is negated.  An exactly zero dot product
 * leaves the sign unspecified.  For cnt < 3 the normal is (0, 0, 0); the other fields are as defined.
 * Sum order.  vba_options::deterministic = 1: s and M are the chains ((0 + t_0) + t_1) + ... in the order of S, no f64 atomic is on
 * the path, and the result of a call is a function of its inputs bit for bit.  Default: f64 atomics form s and M, and two calls may
 * differ in the last bits of c and C and in what the fit makes of those.
 * Capacity, size query, limits, waits, locking: as vba_kf_voxel_export.  More kept voxels than `cap` is VBA_ERR_CAPACITY with
 * *n_out = the number needed and every output untouched; cap == 0 with surfels == NULL is the size query; an S of 2^31 records or
 * more is VBA_ERR_CAPACITY before any device work.  surfels [cap][12], cov [cap][6] and counts [cap] are all HOST or all DEVICE
 * memory; a device surfels is 16-byte aligned, a device cov 8-byte aligned.  Every call waits for the stream once, for the count; a
 * device result is then written stream-ordered without a second wait, a host result passes through the context's staging (whole)
 * and the call returns when it has arrived.
 * Work memory: the work arrays of vba_kf_voxel_export, shared with it (the two calls may alternate on one context: each call clears
 * and refills them), and beyond them 52 bytes per KEPT voxel: a row of six f64 moment sums, which become the covariance in place,
 * and the slot of every output row; nothing of this feature's own is proportional to the table's slots.  A host result adds 52
 * bytes of staging per kept voxel.  _reserve(max_points, max_voxels) sizes all of it for an S of max_points records and a result of
 * max_voxels voxels; a call that needs more doubles what is short after a synchronise, and nothing is allocated per call.
 * _allocations: allocations made and bytes requested so far for the shared work arrays and this feature's own together, cumulative.
 * VBA_ERR_BAD_ARG before any device work, outputs untouched: the refusals of vba_kf_voxel_export (with surfels in the place of
 * xyzi), a misaligned device cov, cov on the other side. */
int vba_kf_surfel_export_reserve(vba_ctx *ctx, int64_t max_points, int64_t max_voxels);
int vba_kf_surfel_export_allocations(vba_ctx *ctx, int *n_allocs, int64_t *bytes);
int vba_kf_surfel_export(vba_ctx *ctx, int n_stores, vba_kf_store *const *stores, const float *intensity /* [n_stores] */, int jump,
                         double voxel_size, int min_count, int64_t cap, float *surfels /* [cap][12], HOST or DEVICE */,
                         double *cov /* [cap][6], same side as surfels, may be NULL */,
                         int *counts /* [cap], same side as surfels, may be NULL */, int64_t *n_out);

/* ---- Registration of a scan against the surfel map: prior-map localisation.  No reference counterpart.
 *
 * A vba_surfel_map holds the cells of a surfel export in HBM and works on its context's stream, like a vba_loop_map; sharded
 * contexts are VBA_ERR_UNSUPPORTED.
 * Cell: a record of the surfel export with [11] >= min_count.  Mean c = (double)record[0..2] (the floats, so that both build
 * paths define one map); weight W = (C + sigma^2 I)^-1 from the record's cov, six doubles xx xy xz yy yz zz, by the cofactor
 * formula of csrc/vba_surfreg_math.hpp (sreg_weight: nothing contracted, the order written there is the definition).
 * Key: the down-samplers' voxel key of record[0..2] at voxel_size (both inherited quirks, 21 bits per axis), which is the key of
 * the voxel the record came from.  Two records with one key were not made at this voxel_size: VBA_ERR_BAD_ARG, the map is empty.
 * Storage: an open-addressing table (ds_hash, linear probing) of the smallest power of two >= 2 n slots of 16 bytes (key, row),
 * n the records given, and one 64-byte line per cell (float c[3], float cnt, double W[6]) at the record's row.
 * _build: surfels [n][12] and cov [n][6] both HOST (staged once) or both DEVICE memory of the map's device (read in place, not
 * kept); n == 0 empties the map.  _build_from_kf runs the surfel export into arrays the map owns (the stores' intensity is not
 * read; refusals and locking are the export's) and builds from them.  A build waits for the stream once for its status words
 * (cells, duplicate flag); _build_from_kf before that once for the export's count.  voxel_size >= 0.001, sigma >= 1e-4,
 * min_count >= 1, n <= 2^30, else VBA_ERR_BAD_ARG with *n_cells untouched.
 * _reserve(max_cells, max_points): table, cells and record staging for max_cells records, scan staging for max_points points and
 * the state and partial blocks; afterwards no build or registration within those sizes allocates.  Beyond them a call doubles
 * what is short after a synchronise.  _allocations: allocations made and bytes requested so far, cumulative. */
typedef struct vba_surfel_map vba_surfel_map;
int vba_surfel_map_create(vba_ctx *ctx, vba_surfel_map **m);
int vba_surfel_map_destroy(vba_surfel_map *m);
int vba_surfel_map_reserve(vba_surfel_map *m, int64_t max_cells, int64_t max_points);
int vba_surfel_map_allocations(vba_surfel_map *m, int *n_allocs, int64_t *bytes);
int vba_surfel_map_build(vba_surfel_map *m, int64_t n, const float *surfels /* [n][12] */, const double *cov /* [n][6] */,
                         double voxel_size, double sigma, int min_count, int64_t *n_cells);
int vba_surfel_map_build_from_kf(vba_surfel_map *m, int n_stores, vba_kf_store *const *stores, int jump, double voxel_size,
                                 double sigma, int min_count, int64_t *n_cells);
int vba_surfel_map_size(vba_surfel_map *m, int64_t *n_cells, double *voxel_size /* may be NULL */, double *sigma /* may be NULL */);
/* Diagnostic: the occupied slots of the table in slot order, to HOST arrays of cap entries (each may be NULL): the slot, its key,
 * the cell's row in the build arrays, the cell's c and cnt (4 floats) and W (6 doubles).  *n_out = the cells, *n_slots = the
 * table's slots; cap == 0 is the size query, fewer than the cells is VBA_ERR_CAPACITY.  Waits for the stream. */
int vba_debug_surfel_map_read(vba_surfel_map *m, int64_t cap, int64_t *slot, unsigned long long *key, int *row, float *c4, double *W,
                              int64_t *n_out, int64_t *n_slots);

/* Gauss-Newton registration of n body-frame points against the map, from the pose (R row-major, t) to the pose it ends at.
 * pnt [n][3] is HOST memory (staged once) or DEVICE memory of the map's device, read in place: the points of a prepared scan
 * frame, a slice of a keyframe store's clouds, any array.
 * Per iteration and point: q[r] = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r] in double, uncontracted; the voxel index of
 * (float)q; candidates: that cell and, for neighbors == 7, its six face neighbours (+-1 on the integer axis index before
 * packing) in the order own, -x, +x, -y, +y, -z, +z; for each existing candidate d = q - c and m = d^T W d, the smallest m wins,
 * ties go to the earlier candidate; the point enters the sums when m < gate^2.  With J = [-R hat(p) | I] for the update
 * R <- R Exp(dphi), t <- t + dt the 29 sums are the upper triangle of J^T W J (21, row-major), J^T W d (6), m / 2 and 1.
 * Then H delta = -g by the library's 6x6 LDLT, the pose update, and the report slots of the iteration.
 * End: converged (|dphi| < eps_rot and |dt| < eps_tra after a step); iters == max_iter; lost (fewer than min_matches points
 * entered the sums: the pose is as it was before that iteration); singular (a non-finite step: the pose is unchanged).  iters
 * counts the evaluated iterations, the one that ended lost or singular included; matches[i], cost[i] (the sum of m / 2) belong
 * to iteration i at the pose BEFORE its step, step_rot[i], step_tra[i] are that step's norms (0 where none was taken); H, g are
 * those of the last evaluated iteration; eig_tt the ascending eigenvalues of its translation block (the sum of W), the degeneracy
 * figure a caller thresholds.
 * Order of the sums: a function of n and the inputs alone; no f64 atomic is on the path; two calls return the
 * same bytes in every mode.  One upload, max_iter gated launch pairs queued at once, one download, one wait.
 * VBA_ERR_BAD_ARG before any device work, outputs untouched: a NULL m, pnt, p, R or t (rep may be NULL), n < 1, neighbors not 1
 * or 7, max_iter outside 1..32, gate <= 0, an empty map, pnt on another device.
 * vba_debug_surfel_reg_pass runs ONE iteration of the same launches with taps that are null in the loop: cell [n] the chosen
 * cell's row in the build arrays or -1, gate [n] 1 where the point entered the sums, sums [29], dx [6] the step (zeros when none
 * was taken); R, t leave as the loop would hold them after that iteration.  Every tap is HOST memory and may be NULL. */
#define VBA_SURFEL_REG_MAX_ITER 32
typedef struct {
  double gate;
  int neighbors, max_iter, min_matches;
  double eps_rot, eps_tra;
} vba_surfel_reg_params;
typedef struct {
  int iters, converged, lost, singular;
  int matches[VBA_SURFEL_REG_MAX_ITER];
  double cost[VBA_SURFEL_REG_MAX_ITER], step_rot[VBA_SURFEL_REG_MAX_ITER], step_tra[VBA_SURFEL_REG_MAX_ITER];
  double H[21], g[6], eig_tt[3];
} vba_surfel_reg_report;
void vba_surfel_reg_default_params(vba_surfel_reg_params *p);   /* 3.0, 7, 30, 50, 1e-5, 1e-5 */
int vba_surfel_register(vba_surfel_map *m, int64_t n, const double *pnt /* [n][3], HOST or DEVICE */, const vba_surfel_reg_params *p,
                        double *R /* [9] in/out */, double *t /* [3] in/out */, vba_surfel_reg_report *rep /* may be NULL */);
int vba_debug_surfel_reg_pass(vba_surfel_map *m, int64_t n, const double *pnt, const vba_surfel_reg_params *p, double *R, double *t,
                              int *cell, unsigned char *gate, double *sums, double *dx);

/* ------------------------------------------------------------------------------------------------
 * Loop-closure map: the counterpart of `map_loop` (VS:2601-2625) and loop_update() (VS:1255-1373), the step that
 * carries a loop closure back into local mapping.  A vba_loop_map owns one second voxel map, created from its context's options
 * and working on that context's stream; like the keyframe store it may hang off the loop-closure thread's context.
 *
 * Both halves are fixed-point insertions of clouds that are in HBM already.  Fixed-point cut_voxel (VM:2108-2152) is a per-point
 * loop whose only per-call state is jour, so the reference's sequence of calls at jour = 0 is ONE insertion of the concatenated
 * clouds; the device runs it as one, with one counter read-back.  Unlike vba_map_cut_voxel_fix these insertions carry the points'
 * covariances into point_fix (push_fix_novar stores pv whole, VM:1168; push_fix adds Bf_var(pv) to cov_add at the first recut,
 * VM:1149-1162): the keyframes' normal_x/y/z as a diagonal (VS:2620-2621), the buf_lba2loop scans' full 3x3 rows unrotated
 * (VS:1341-1344).
 *
 * Order of operations (part of the interface): pw[r] = ((R[r][0]*x + R[r][1]*y) + R[r][2]*z) + t[r], no product fused with a sum.
 *
 * Residency: after vba_loop_map_reserve(fix_points, nodes) no call below allocates for the loop map while one insertion and the
 * map's fixed-point pool stay within fix_points points and the map within `nodes` octree nodes.  vba_loop_update trades the two
 * maps: the object then owns the map the context gave up, with that map's allocations (ping-pong); the reservation is applied to
 * it and both root tables are brought to the larger size, so from the second loop closure on nothing is allocated.
 * vba_loop_map_allocations: count = calls on this object that allocated (vba_loop_update counts growth of either map), bytes =
 * what they allocated. */
typedef struct vba_loop_map vba_loop_map;
int vba_loop_map_create(vba_ctx *ctx, vba_loop_map **out);
void vba_loop_map_destroy(vba_loop_map *lm);   /* before its context */
int vba_loop_map_reserve(vba_loop_map *lm, int64_t fix_points, int64_t nodes);
int vba_loop_map_allocations(vba_loop_map *lm, int *count, int64_t *bytes);
/* The block VS:2601-2625.  The loop map is reset; keyframes max(0, size - init_num) .. size - 1 of `store` (same device) are moved
 * to the world with their CURRENT x0 (the caller has run vba_kf_set_poses) and inserted as fixed points with their covariance
 * diagonals at jour = 0; their exist flags are cleared (VS:2612).
 * cumulative = 1 is THE REFERENCE: pvec_tem (VS:2602) is never cleared, so insertion j holds keyframes 0 .. j again; with five
 * keyframes the oldest goes in five times and the newest once.  cumulative = 0 is the corrected form: every keyframe once.
 * *n_inserted = points of the expanded sequence.  One gather over the store's arrays, one fixed insertion; the call ends with that
 * insertion's counter read-back (one synchronise of the loop map's stream), so the map is complete when it returns.  The caller
 * holds the store's lock (mtx_keyframe) around the call.  An empty store gives an empty map.  On error the loop map is empty. */
int vba_loop_map_build(vba_loop_map *lm, vba_kf_store *store, int init_num /* 5 */, int cumulative, int *n_inserted);
/* row formats of vba_map_num_roots / vba_map_dump_leaves / vba_map_dump_plane_var */
int vba_loop_map_num_roots(vba_loop_map *lm);
int vba_loop_map_dump_leaves(vba_loop_map *lm, double *out, int max_leaves);
int vba_loop_map_dump_plane_var(vba_loop_map *lm, double *out, int max_leaves);
/* loop_update() on the local-mapping context: VS:1262-1277 and VS:1334-1363.  The pose algebra of VS:1296-1331 stays with the caller
 * (vba::VoxelMap::loop_update in voxelba_adapter.hpp): every pose below is ALREADY moved by dx; dx12 (may be NULL) is only checked
 * to be finite.
 *  1. Arguments are checked before any device work: VBA_ERR_BAD_ARG for win_count outside 1..win_size, a loop map whose map
 *     options (win_size, voxel_size, max_layer, max_points, min_eigen_value, plane thresholds, min_point, thread_num,
 *     deterministic) differ from ctx's or that lives on another device, bad offsets, non-finite poses; VBA_ERR_UNSUPPORTED when ctx
 *     is sharded (vba_set_shard with n_ranks > 1): sharded maps are not covered.
 *  2. ctx adopts the loop map (surf_map = map_loop) with mp[i] = i; lm takes the outgoing map, which stays readable until step 6.
 *  3. The k buf_lba2loop scans, rows offsets[i] .. offsets[i+1] of pnt [][3] (body frame) and var [][9] (NULL: zeros), HOST or
 *     DEVICE memory as for vba_kf_build, at poses_bl [k][12]: one fixed insertion with covariances at jour = 0.  k = 0 skips it.
 *  4. For i < win_count the sliding insert (vba_map_cut_voxel, multi = 0) at frame i with poses_win[i].  win_pnt == NULL: the
 *     source is the OUTGOING map's own scan ring (the raw body points, the world covariances and the count of frame i exactly as
 *     they were inserted, including covariances formed on the device by vba_map_pvec_update_cut_voxel): device to device, no point
 *     crosses the host boundary.  Otherwise rows win_offsets[i] .. win_offsets[i+1] of win_pnt / win_var (NULL: none), host or
 *     device.
 *  5. vba_map_recut(ctx, win_count, poses_win, 0) over all roots; *n_factors = its factor count.  The reference's loop (VS:1362-1363)
 *     does not run tras_opt; filling the factor store here is unobservable, because the next step's multi_recut clears and
 *     refills it.
 *  6. The outgoing map is reset and kept by lm with its allocations.
 * On an error return after step 1 the context's map is the one it had before the call (the maps are traded back; the loop map is
 * reset and has to be built again), unless vba_last_error says otherwise (only a failure of step 6 leaves the new map in place).
 * Synchronises as its parts do: once per fixed insertion, once for the recut, plus the reset. */
int vba_loop_update(vba_ctx *ctx, vba_loop_map *lm, const double *dx12, int k, const int *offsets, const double *pnt, const double *var,
                    const double *poses_bl, int win_count, const double *win_pnt, const double *win_var, const int *win_offsets,
                    const double *poses_win, int *n_factors);

/* ------------------------------------------------------------------------------------------------
 * Scan log: the counterpart of the live `ScanPose::pvec` pointers of one session (pvec_buf[0] -> ScanPose::pvec ->
 * buf_lba2loop -> bl_local, VS:1974-1980 .. VS:2342), resident in HBM.  A scan enters the log from the map's scan ring by a
 * device-to-device capture before it is marginalised, and the keyframe store, the loop update, pub_localmap and save_pcd read it
 * in place: between leaving the window and becoming part of a keyframe no point crosses the host boundary.
 *
 * Layout: one arena double pnt [cap][3] (body points) and double var [cap][9] (the covariance rows as the map's ring held them: the
 * world covariances of pvec_update, VH:259), used as a ring of WHOLE scans.  A scan never straddles the arena's end: when the tail
 * is too short it is skipped, so consecutive scans need not be contiguous and every reader addresses a scan by its own start.
 * Scans are numbered 0, 1, 2, ... in push order (64 bits); a session that pushes every marginalised scan has seq = win_base + i,
 * the `count` of save_pcd's file name.  Release is first in, first out.
 *
 * Growth: the arena grows by doubling; growing allocates new blocks, copies the live scans device to device in order (packed from
 * row 0), and frees the old blocks after a synchronise.  Numbers are kept.  After vba_scanlog_reserve(points, scans) no call on the
 * log allocates device memory while, AT EVERY PUSH of n points,
 *     live points + gap + n <= points   and   live scans + 1 <= scans,
 * where gap = the rows at the arena's end that a wrap leaves unused: 0 while the scans lie in ascending order and the new one fits
 * behind the newest; points - (end of the newest scan) when this push has to skip the tail; points - (end of the last scan before
 * the skip) for as long as the oldest live scan still lies above the newest.  (A session of scans of at most m points that holds at
 * most s of them live is safe with points = (s + 1) * m.)  This is exactly the test of the ring bookkeeping
 * (csrc/vba_scanlog_ring.hpp, place), which is what decides when a push grows the arena.  vba_scanlog_allocations counts the
 * calls that allocated and their bytes, as vba_kf_allocations does.
 *
 * Ordering and threads: the log works on its context's stream.  It is not locked internally beyond its bookkeeping: the producer
 * thread (the push calls) and ONE consumer thread (release and the readers: range, read, export, the keyframe build, the loop
 * update) may overlap as long as no push has to grow the arena; a push that grows must be excluded from every reader by the
 * caller, because the arrays move.  A reader on another stream of the device is ordered behind the captures by an event, nothing
 * waits on the host.  The one reader that returns with its device work still queued is the export into device memory: it leaves
 * an event in the log, and the next push waits for that event on its own stream before it may write over released rows.
 * Destroy the log before its context. */
typedef struct vba_scanlog vba_scanlog;
int vba_scanlog_create(vba_ctx *ctx, vba_scanlog **out);
void vba_scanlog_destroy(vba_scanlog *l);
int vba_scanlog_reserve(vba_scanlog *l, int64_t points, int scans);   /* points <= 2^30; also the float staging of vba_scanlog_read */
int vba_scanlog_allocations(vba_scanlog *l, int *count, int64_t *bytes);
/* Captures frame `frame` (0 .. win_size-1, slot mp[frame]) of the window of the log's context: the slot's body points and covariance
 * rows exactly as they were inserted (zeros when the map holds no covariances), by one kernel on the context's stream.  No host
 * synchronise: the count is the host's.  CALL IT WHERE THE REFERENCE CREATES THE ScanPose (VS:1974-1980): after the BA and BEFORE
 * vba_map_margi, which clears the outgoing slot's count; after it the pushed scan is empty.  An empty frame is pushed as an empty
 * scan and still gets a number.  *seq = the scan's number.  VBA_ERR_UNSUPPORTED: the context is sharded (its ring holds only the
 * rank's share of a scan).  VBA_ERR_BAD_ARG: a frame outside the window. */
int vba_scanlog_push_window(vba_scanlog *l, int frame, int64_t *seq);
/* Pushes a scan the caller holds: pnt [n][3], var [n][9] (NULL: zeros), HOST or DEVICE memory as for vba_map_cut_voxel (host arrays
 * are the caller's again on return).  For offline sessions and tests. */
int vba_scanlog_push_points(vba_scanlog *l, int n, const double *pnt, const double *var, int64_t *seq);
/* the live numbers [*first, *end) and the sizes of up to cap scans from *first */
int vba_scanlog_range(vba_scanlog *l, int64_t *first, int64_t *end, int cap, int *sizes);
/* drops every scan with seq < upto (pvec = nullptr, VS:2342 / VS:2375 / VS:2227-2228); their rows may be written by later pushes */
int vba_scanlog_release(vba_scanlog *l, int64_t upto);
/* Scan seq to the host (tests, save_pcd): pnt [cap][3], var [cap][9], xyz [cap][3] = the body point narrowed once to float ON THE
 * DEVICE (pl_save, VS:172-174: 12 bytes per point cross); any output may be NULL.  *n = the scan's size, at most cap points are
 * written.  Synchronises once.  VBA_ERR_BAD_ARG: seq is not live. */
int vba_scanlog_read(vba_scanlog *l, int64_t seq, int cap, double *pnt, double *var, float *xyz, int *n);
/* pub_localmap's point loop (VS:63-76) from the log: for scans first .. first+k-1 at poses [k][12] the points j = 0, stride,
 * 2 stride, ... < size (the stride restarts at every scan: ceil(size / stride) points each) as records x y z intensity of four
 * floats.  world = R p + t in the order stated for vba_kf_export_world, every product and sum rounded on its own, each coordinate
 * narrowed to float once.  xyzi [cap][4] is HOST or DEVICE memory with that call's rules: host output passes through ctx's
 * staging and the call synchronises once; device output (16-byte aligned) is stream-ordered on ctx's stream and the call returns
 * with the gather queued (see "Ordering and threads").  ctx may be another context of the log's device.  *n_out = the record count,
 * always; VBA_ERR_BAD_ARG with nothing queued and xyzi untouched when cap is smaller than it, when the range is not wholly live,
 * for stride < 1, a non-finite pose or another device. */
int vba_scanlog_export_world(vba_ctx *ctx, vba_scanlog *l, int64_t first, int k, const double *poses, int stride, float intensity,
                             int64_t cap, float *xyzi, int64_t *n_out);
/* vba_kf_build with var != NULL on scans first .. first+k-1 of the log: the merge reads scan j at its own arena start; everything
 * after it (the transforms and their order of operations, the covariance diagonal taken unrotated, down_sampling_pvec, the
 * descriptors, the commit rule, the errors) is vba_kf_build's own code.  The store may hang off another context of the log's
 * device (another device: VBA_ERR_BAD_ARG): its stream waits for the captures through an event.  VBA_ERR_BAD_ARG, store and db
 * untouched: a range that is not wholly live, or more than 2^28 points. */
int vba_kf_build_from_log(vba_kf_store *s, vba_scanlog *l, int64_t first, int k, const double *poses, double voxel_size, int id,
                          double jour, vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds, int *n_points);
/* vba_loop_update with steps 3 and 4 fed from the device: the buf_lba2loop scans are scans first .. first+k-1 of the log with their
 * full covariance rows (each read at its own arena start), the window is the outgoing map's scan ring (the win_pnt == NULL form).
 * Checks, the trade of the maps, the failure path and the synchronisation are that call's: one body serves both.  Additionally
 * VBA_ERR_BAD_ARG for a range that is not wholly live or a log on another device. */
int vba_scanlog_loop_update(vba_ctx *ctx, vba_loop_map *lm, const double *dx12, vba_scanlog *l, int64_t first, int k,
                            const double *poses_bl, int win_count, const double *poses_win, int *n_factors);

/* ------------------------------------------------------------------------------------------------
 * Scan front end: the node's per-scan path from the raw sensor message to the points and covariances that the
 * odometry and the map read, resident in HBM.  A frame owns the device buffers of one scan.
 *   decode:  Features::process + pcl_handler (FP:103-366, VH:77-103): raw message bytes -> decoded, filtered, time-sorted, cut cloud.
 *   prepare: motion_blur's point loop + down_sampling_voxel + the retry + var_init (EK:135-163, VS:1877-1888), stream-ordered; returns
 *            DEVICE pointers that vba_odom_lio_state_estimation and vba_map_pvec_update_cut_voxel consume in place.
 * Between the two the node runs sync_packages (it needs the last curvature, VH:129) and the host IMU propagation (EK:55-123) that
 * produces imu_poses.
 *
 * A record of the message is point_step bytes; the fields are read at byte offsets that need not be aligned:
 *   x, y, z     float32.
 *   intensity   by intensity_type; NONE gives 0 (velodyne FP:185, tartanair).
 *   curvature   by time_type.  U32_DIV1E9: the u32 converted to float (round to nearest), then ONE float division by float(1e9).
 *               F64_REL_FIRST: t[i] - t[0] in double, t[0] read from raw record 0 whether or not it is kept, narrowed once.
 * filter == 1: record i is kept iff i % point_filter_num == 0 and (double)((x*x + y*y) + z*z) > blind2, products and sums in float in
 * that order, not contracted (a point exactly on the blind sphere is dropped).  filter == 0: every record is kept.
 * Kept points keep message order.  No kept point (or n_raw == 0): two points at the origin, intensity 0, curvatures 0 and 0.09f
 * (VH:82-90).  Then the sort on the float curvature, ascending (VH:92-95), and the cut of trailing points with
 * (double)curvature > 0.11 (VH:96-97).
 *
 * TIES: the sort is STABLE, points of equal curvature keep message order (-0.0f and +0.0f are equal).  The reference's std::sort
 * leaves their order undefined.
 * Deviations from the reference: (1) a message whose points are ALL beyond 0.11 ends with n = 0, *last_curvature = 0 and VBA_OK
 * (the reference pops from an empty vector), and prepare on such a frame returns n = 0; (2) NaN times are unsupported input
 * (undefined behaviour in the reference; here their position after the sort is unspecified); (3) time_type F32 (velodyne): when the
 * last raw record's time is not inside (0.01, 0.12) the reference takes its yaw-angle branch (FP:200-252), which is not built:
 * VBA_ERR_UNSUPPORTED, read on the host from `raw`.
 *
 * Stored form: coordinates and curvature as PCL floats carried in doubles ([n][3], [n]), the convention of the vba_scan_* calls
 * above; intensity as float. */
typedef struct vba_scan_frame vba_scan_frame;

enum { VBA_SCAN_TIME_NONE = 0,         /* curvature = 0                                          tartanair FP:356 */
       VBA_SCAN_TIME_F32 = 1,          /* curvature = the float field as it is                   velodyne  FP:188 */
       VBA_SCAN_TIME_U32_DIV1E9 = 2,   /* (float)u32 / float(1e9), one float division            livox FP:155, ouster FP:271 */
       VBA_SCAN_TIME_F64_REL_FIRST = 3 /* (float)(t[i] - t[0]), the subtraction in double        hesai FP:304, robosense FP:335 */ };
enum { VBA_SCAN_INTENSITY_NONE = 0, VBA_SCAN_INTENSITY_F32 = 1, VBA_SCAN_INTENSITY_U8 = 2 /* livox reflectivity FP:153 */ };

typedef struct vba_scan_layout {
  int point_step;                  /* bytes from one record to the next (any value >= 1; 26 for the Hesai driver) */
  int off_x, off_y, off_z;         /* float32 fields */
  int off_intensity, intensity_type;
  int off_time, time_type;
  int filter;                      /* 1: decimation + blind test apply; 0: every point is kept (tartanair FP:350-366) */
} vba_scan_layout;

/* livox_ros_driver::CustomPoint as it lies in memory: step 20, time u32 @0, xyz @4/8/12, reflectivity u8 @16 */
int vba_scan_layout_livox(vba_scan_layout *l);
/* Host only (no device needed): VBA_OK when point_step >= 1, the type codes are known, filter is 0 or 1 and every field that its type
 * code selects lies inside [0, point_step); VBA_ERR_BAD_ARG otherwise. */
int vba_scan_layout_check(const vba_scan_layout *l);

/* A frame belongs to the device of ctx; decode runs on ctx's stream.  The buffers are grow-only, by doubling after a synchronise;
 * after vba_scan_frame_reserve no call allocates while n_raw <= max_raw_points, n_raw * point_step <= max_raw_points * max_point_step
 * and m <= 64 IMU poses (vba_scan_frame_allocations counts allocations and bytes, as vba_kf_allocations does).  Growing discards the
 * frame's contents.  A frame is not synchronised internally; destroy it before its context. */
int vba_scan_frame_create(vba_ctx *ctx, vba_scan_frame **out);
void vba_scan_frame_destroy(vba_scan_frame *f);
int vba_scan_frame_reserve(vba_scan_frame *f, int max_raw_points, int max_point_step);
int vba_scan_frame_allocations(vba_scan_frame *f, int *n_allocs, int64_t *bytes);

/* raw: n_raw records in HOST memory, uploaded once.  blind2 = blind * blind (VS:906).  *n_out = points of the frame's cloud,
 * *last_curvature = pl_ptr->back().curvature (VH:129; 0 when n = 0).  Complete when it returns (one synchronise).
 * VBA_ERR_BAD_ARG: a layout that fails vba_scan_layout_check, n_raw < 0, point_filter_num < 1. */
int vba_scan_decode(vba_scan_frame *f, const vba_scan_layout *l, const void *raw, int n_raw, int point_filter_num, double blind2,
                    int *n_out, double *last_curvature);

/* On ctx's stream (ctx may be another context of the frame's device), from the frame's decoded cloud:
 *  1. undistortion as vba_scan_undistort (imu_poses [m][22], end_pose [12], ext_pose [12]), skipped when point_notime != 0 (EK:135);
 *  2. down_sampling_voxel at down_size; if min_points > 0 and fewer than min_points voxels result, once more at down_size / 2 from
 *     the UNDISTORTED cloud, that result kept whatever its count (VS:1880-1884; the node passes 500, and 0 with
 *     down_size = max(down_size, 0.5) for VS:1470-1474).  A size < 0.001 leaves the cloud as it is (TL:203).
 *     vba_options::deterministic of ctx selects the deterministic summation;
 *  3. var_init with ext_pose, dept_err, beam_err into *d_pnt_body [n][3] and *d_var_body [n][9].
 * The two pointers are DEVICE pointers owned by the frame, valid until the frame's next decode, prepare, reserve or destroy; the
 * call may return before var_init has finished, consumers on ctx's stream are ordered behind it.  One synchronise per call, two when
 * the retry runs.  Preparing a frame again repeats the work from the decoded cloud.
 * VBA_ERR_BAD_ARG when the frame has not been decoded (or lost its contents by growing), or lives on another device. */
int vba_scan_prepare(vba_ctx *ctx, vba_scan_frame *f, int m, const double *imu_poses, const double *end_pose, const double *ext_pose,
                     int point_notime, double down_size, int min_points, double dept_err, double beam_err, int *n_out,
                     const double **d_pnt_body, const double **d_var_body);

/* Inspection (synchronises).  stage 0 = decoded + sorted: pnt [n][3], intensity [n], curvature [n]; 1 = undistorted: the same with the
 * moved points; 2 = down-sampled: pnt [m][3], count [m], first [m] as vba_scan_down_sampling_voxel; 3 = var_init: pnt [m][3],
 * var [m][9].  n and m are the counts that decode and prepare returned.  NULL outputs, and outputs that a stage does not have, are
 * skipped.  Stages 1-3 need a prepared frame (VBA_ERR_BAD_ARG). */
int vba_scan_frame_read(vba_scan_frame *f, int stage, double *pnt, float *intensity, double *curvature, int *count, int *first,
                        double *var);

/* ------------------------------------------------------------------------------------------------
 * Initialisation window: pl_origs of initialization() (VS:1499-1516) resident in HBM.  Per scan of the window the
 * node does  pl_down = orig; down_sampling_close(pl_down, down_size); if (size < 1000) { pl_down = orig; down_sampling_close(pl_down,
 * down_size / 2) }; sort(curvature <); pl_origs.push_back(pl_down)  with orig the copy of pcl_curr taken before odom_ekf.process
 * (VS:1458): the frame's stage 0, which vba_scan_prepare leaves alone.  The window holds the ragged clouds in the form
 * vba_motion_init reads (pnt [n][3], curv [n], PCL floats carried in doubles); the offsets stay on the host.
 *
 * Stage 0 is sorted by curvature with a STABLE sort and down_sampling_close keeps a subset of it, so the reference's sort, with ties
 * resolved as the scan front end resolves them (message order), is that subset in ascending stage-0 index: push runs no sort, it
 * compacts in index order.
 *
 * A window belongs to the device of ctx and works on ctx's stream.  Its buffers grow by doubling and keep their contents; after
 * vba_init_window_reserve(w, max_scans, max_points_per_scan) no call allocates while the window holds at most max_scans scans and
 * every pushed frame's decoded cloud (or pushed array) has at most max_points_per_scan points; vba_init_window_allocations counts
 * allocations and bytes as vba_scan_frame_allocations does.  Destroy it before its context. */
typedef struct vba_init_window vba_init_window;
int vba_init_window_create(vba_ctx *ctx, vba_init_window **out);
void vba_init_window_destroy(vba_init_window *w);
int vba_init_window_reserve(vba_init_window *w, int max_scans, int max_points_per_scan);
int vba_init_window_allocations(vba_init_window *w, int *n_allocs, int64_t *bytes);
int vba_init_window_clear(vba_init_window *w);   /* pl_origs.clear() (VS:795); the storage is kept */
/* *n_scans = pl_origs.size(); offsets [n_scans + 1] (may be NULL): rows before every scan, and their total */
int vba_init_window_size(vba_init_window *w, int *n_scans, int64_t *offsets);
/* Appends one scan from the frame's stage 0, read in place on the window's stream (the frame may have been decoded or prepared on
 * another context of the same device; the read is ordered behind the decode).  The selection is vba_scan_down_sampling_close at
 * down_size (float centroid, first point in input order among equal distances, only distances < 100 compete; vba_options::deterministic
 * of the window's context selects the summation).  If min_points > 0 and fewer than min_points points are kept (strict, VS:1503; the
 * node passes 1000), once more from the full decoded cloud at down_size / 2, that result kept whatever its count, *retried = 1.  A
 * size < 0.001 leaves the cloud as it is (TL:242), on either pass.  The kept rows are written in ascending stage-0 index, xyz and
 * curvature bit for bit.  A frame with n = 0 appends an empty scan.  Complete when it returns: one synchronise, two when the retry
 * runs.  VBA_ERR_BAD_ARG, window unchanged: an undecoded frame, a frame on another device, a NULL output pointer. */
int vba_init_window_push(vba_init_window *w, vba_scan_frame *frame, double down_size, int min_points, int *n_kept, int *retried);
/* Appends pnt [n][3], curv [n] as they are (HOST or DEVICE arrays; one synchronise).  The curvatures must ascend: HOST arrays are
 * checked (VBA_ERR_BAD_ARG), DEVICE arrays are NOT, the caller answers for them. */
int vba_init_window_push_points(vba_init_window *w, int n, const double *pnt, const double *curv);
/* Inspection (synchronises): the rows of one scan; NULL outputs are skipped. */
int vba_init_window_read(vba_init_window *w, int scan, double *pnt, double *curv);

/* vba_motion_init with pl_origs taken from a window: the arguments of vba_motion_init with pt_offsets, pnt, curv replaced by w.  The
 * clouds are read in place, no copy of them is made on the host or the device.  What the host walk of vba_motion_init reads from the
 * curvatures (per scan the number of leading points at or before the oldest pose, and the curvature of point 0) is found by one small
 * kernel (binary search; curvature ascends) and crosses in one W-row download with one synchronise; everything after that is the code
 * of vba_motion_init, and the results are the same bit for bit.  The window must hold exactly win_size scans and live on ctx's device
 * (it may belong to another context of it): VBA_ERR_BAD_ARG before any device work otherwise.  The window is not cleared.  Errors and
 * what they leave behind: as vba_motion_init. */
int vba_motion_init_resident(vba_ctx *ctx, int win_size, vba_init_window *w, const int *imu_offsets, const double *imu,
                             const double *beg_times, const double *ext_pose, double dept_err, double beam_err, double scale_gravity,
                             int point_notime, const double *noise_meas_diag6, const double *noise_walk_diag6, double *states,
                             const double *covs, double *imus, double *hess, int *converged, double *eigvalue3, int *iterations,
                             int *thresholds_left_relaxed, double *round_log, int max_rounds, double *pnt_out, double *var_out,
                             int *pvec_offsets, int pvec_cap);

/* ------------------------------------------------------------------------------------------------
 * IMU forward propagation and the odometry state resident in HBM: IMUEKF::motion_blur's propagation of state and
 * covariance (ekf_imu.hpp, "EK", EK:54-123) with the pose table the undistortion reads, and the per-scan chain
 * odom_ekf.process -> vba_scan_prepare -> lio_state_estimation -> pvec_update + cut_voxel (VS:1873-1922) on a state that stays on the
 * device from one scan to the next.
 *
 * imu [m][7] = [t, gyr(3), acc(3)]: the deque rows as they are after imus.push_front(last_imu) (EK:43).  noise [12] = cov_gyr, cov_acc,
 * cov_bias_gyr, cov_bias_acc.  Intervals whose tail lies before last_pcl_end_time are skipped (EK:64), cur_time is clamped (EK:81-84),
 * a pose row [offt, R(9), p(3), v(3), angvel_avr(3), acc_imu(3)] (the row of vba_scan_undistort) is pushed before the update (EK:87),
 * cov <- F_x cov F_x^T + cov_w (EK:92-105, not symmetrised), position, velocity, rotation move in that order (EK:108-110), the tail is
 * extrapolated with note = +-1 (EK:117-123), state.t = pcl_end_time; bg, ba, g are not written.  *n_poses = the rows written, at most
 * m - 1: it depends on comparisons of the time stamps alone.  end_pose [12] = (xc.R, xc.p) after the propagation.
 * VBA_ERR_BAD_ARG with state and covariance untouched: m < 2; no interval left after the EK:64 skip (the reference reads
 * uninitialised values at EK:120); last_pcl_end_time - pcl_beg_time > 0.01 (the "LiDAR time regress" exit(0) of EK:45-49); a
 * non-finite input; a NULL pointer. */

/* Host only (no context, no device): state [25] and cov [225] in / out, imu_poses [m - 1][22] (rows beyond *n_poses are not written). */
int vba_imu_ekf_propagate(int m, const double *imu, const double *noise, double scale_gravity, double last_pcl_end_time,
                          double pcl_beg_time, double pcl_end_time, double *state, double *cov, double *imu_poses, double *end_pose,
                          int *n_poses);

/* A state object belongs to the device of ctx and is created with room for 64 IMU rows; its pose table grows by doubling after a
 * synchronise, and after vba_odom_state_reserve(st, max_imu_rows) no call on it allocates while m <= max_imu_rows
 * (vba_odom_state_allocations counts allocations and bytes as vba_scan_frame_allocations does).  Destroy it before its context. */
typedef struct vba_odom_state vba_odom_state;
int vba_odom_state_create(vba_ctx *ctx, vba_odom_state **out);
void vba_odom_state_destroy(vba_odom_state *st);
int vba_odom_state_reserve(vba_odom_state *st, int max_imu_rows);
int vba_odom_state_allocations(vba_odom_state *st, int *n_allocs, int64_t *bytes);
/* state [25], cov [225]: stream-ordered through a pinned block (the arrays may go away on return).  Non-finite values: VBA_ERR_BAD_ARG. */
int vba_odom_state_set(vba_odom_state *st, const double *state, const double *cov);
/* Synchronises.  NULL outputs are skipped. */
int vba_odom_state_get(vba_odom_state *st, double *state, double *cov);
/* Inspection (synchronises): the table of the last propagation, imu_poses [max_rows][22] (VBA_ERR_CAPACITY when it has more rows),
 * and end_pose [12]; NULL outputs are skipped. */
int vba_odom_state_poses(vba_odom_state *st, int max_rows, double *imu_poses, double *end_pose, int *n_poses);
/* The propagation above on the device state (EK:54-123): one upload of the IMU rows and the parameters, one launch, no wait.  The
 * table and end_pose stay on the device for vba_scan_prepare_on_state.  *n_poses is computed by the host from the same doubles. */
int vba_odom_state_propagate(vba_odom_state *st, const double *noise, double scale_gravity, int m, const double *imu,
                             double last_pcl_end_time, double pcl_beg_time, double pcl_end_time, int *n_poses);
/* vba_scan_prepare with imu_poses and end_pose read in place from the table that the last propagation of st left (EK:135-163). */
int vba_scan_prepare_on_state(vba_ctx *ctx, vba_scan_frame *f, vba_odom_state *st, const double *ext_pose, int point_notime,
                              double down_size, int min_points, double dept_err, double beam_err, int *n_out, const double **d_pnt_body,
                              const double **d_var_body);
/* vba_odom_lio_state_estimation_resident (VS:962-1098) on the state of st: the image of the call is built on the device (P^-1 of VS:987
 * by the device restatement of the host inverse, bit for bit), no host inverse and no image upload; one download of the result block
 * and one synchronise.  st holds the updated state and covariance afterwards; state_out [25] (may be NULL) receives the state.
 * VBA_ERR_UNSUPPORTED on a sharded context. */
int vba_odom_lio_state_estimation_on_state(vba_ctx *ctx, vba_odom_state *st, int n, const double *d_pnt_body, const double *d_var_body,
                                           int *ok, vba_odom_report *report, double *state_out);
/* vba_map_pvec_update_cut_voxel (VS:1903-1920) with the pose and the two covariance blocks read from st on the device: nothing but
 * the arguments comes from the host.  VBA_ERR_UNSUPPORTED on a sharded context. */
int vba_map_pvec_update_cut_voxel_on_state(vba_ctx *ctx, vba_odom_state *st, int win_count, int n, const double *d_pnt_body,
                                           const double *d_var_body, int multi);

/* The initialisation odometry on a state object: VOXEL_SLAM::initialization (VS:1450-1534) per scan, after
 * vba_odom_state_propagate and vba_scan_prepare_on_state. */

/* vba_odom_lio_state_estimation_kdtree_resident (VS:1102-1252) on the state of st and the point-cloud map of ctx.  The image of the
 * call is built on the device from the state block (P^-1 by the device restatement of the host inverse, every entry divided by 1000,
 * VS:1135; the first iteration searches): no vba_odom_state_get, no host inverse, no image upload, no vba_odom_state_set.  The
 * launches behind it are the resident call's.  Crosses the boundary: the arguments in, one download of the result block out; ONE wait,
 * for that download alone (the copy of x_curr and P back into the state block runs behind it, ordered before whatever reads the block
 * next).  st holds the updated state and covariance afterwards, state_out [25] (may be NULL) receives the state, the results equal
 * the resident call's on the values of the block bit for bit.
 * While the map holds fewer than 100 points the scan only seeds it (VS:1105-1118): the append reads its pose from the block, the
 * block is not written, *iterations = 0, *report is zeroed; with state_out the 25 doubles of the block are downloaded and that copy
 * alone is waited for, with state_out == NULL the call returns with everything queued.  n == 0 on a map of 100 points or more:
 * *iterations = 2, state and covariance keep their bits, the map is re-sampled.
 * ctx may be another context of the state's device, sharded or not (the point-cloud map is not sharded).  VBA_ERR_BAD_ARG before any
 * device work, st untouched: a NULL ctx, st or iterations; n < 0; n > 0 with a NULL array; a state on another device.
 * VBA_ERR_CAPACITY as the resident call.  The scratch is the resident call's: vba_odom_kdtree_reserve and
 * vba_odom_kdtree_allocations cover this call. */
int vba_odom_lio_state_estimation_kdtree_on_state(vba_ctx *ctx, vba_odom_state *st, int n, const double *d_pnt_body, int *iterations,
                                                  vba_odom_report *report, double *state_out);
/* The published scan of pub_localtraj (VS:37-45): for the n DEVICE points world = x_curr.R p + x_curr.p with the pose read from the
 * state block on the device, in the order of vba_kf_export_world, ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r], every product and
 * sum rounded on its own, each coordinate narrowed to float once; xyzi receives n records x y z intensity of 16 bytes.  *n_out = n.
 * xyzi is HOST memory (the records pass through ctx's staging buffer, ONE synchronise) or DEVICE memory (16-byte aligned; the call
 * is stream-ordered and returns with the work queued, no wait).  Crosses the boundary: nothing but the arguments and, to a host
 * xyzi, the records.  n == 0 succeeds and does nothing.  VBA_ERR_BAD_ARG, nothing queued and xyzi untouched: cap < n, a NULL
 * argument with n > 0, a NULL ctx, st or n_out, n < 0, a state on another device, a misaligned device xyzi. */
int vba_odom_state_export_scan(vba_ctx *ctx, vba_odom_state *st, int n, const double *d_pnt_body, float intensity, int64_t cap,
                               float *xyzi, int64_t *n_out);

/* ------------------------------------------------------------------------------------------------
 * Odometry update against a prior map: localisation mode.  No reference counterpart: the iterated-EKF update of
 * VOXEL_SLAM::lio_state_estimation (VS:962-1098) with the point-to-distribution residuals of vba_surfel_register in the place of
 * the point-to-plane residuals of the live voxel map.  After vba::relocalize has found the pose in an earlier session's map, this
 * call tracks in it: the IMU prediction and its 15 x 15 covariance are the prior, v, bg and ba move through the correlations of
 * P, and the covariance is updated, none of which vba_surfel_register does.
 *
 * Per iteration the point loop is that of vba_surfel_register at the pose of x_curr (query, own cell or own cell and six face
 * neighbours, smallest m, ties to the earlier candidate, gate m < gate^2, the 29 sums in the same order, bit for bit), and the
 * step is vba_odom_ekf's on the 34 sums  HTH = sum J^T W J (21),  HTz = -sum J^T W d (6),  sum W (6, where the voxel map has
 * n n^T),  the count:  the MAP step of the 15-state, with the retraction R <- R Exp(dphi), t <- t + dt both sides assume.  Stop
 * rule, iteration limit (4) and covariance update are those of VS:1072-1086, unchanged.
 *   state [25], cov [225]: in/out as in vba_odom_lio_state_estimation.  pnt_body [n][3]: HOST memory (staged once in the map's scan
 *   staging) or DEVICE memory of the context's device, read in place.
 *   report: the struct of the voxel-map call; nnt_eig_min is the smallest eigenvalue of the last iteration's sum of W, the
 *   degeneracy figure.  *ok = 1 iff the last iteration matched at least min_matches points and nnt_eig_min >= min_eig.  State and
 *   covariance are updated either way, as in the reference; with no match at all the algebra returns the prediction bit for bit.
 *   n == 0: no point loop is launched, state and covariance keep their bits, iterations == 2, *ok = 0 unless min_matches is 0.
 * The start must lie within the gate: from 0.05 m / 0.5 deg the four iterations end within the estimator's bias (1e-4 .. 1e-3 m) of
 * the pose; from 0.2 m / 2 deg only a small part of a scan passes a 3 sigma gate and four iterations do not converge.  That start is
 * vba_surfel_register's (vba::relocalize), not this call's.
 * Crosses the boundary: vba_odom_surfel_update uploads the image once (the host inverts P) and downloads the result block once;
 * _on_state builds the image on the device from the state object (bit for bit the same) and only downloads.  Four gated launch
 * pairs queued at once, ONE wait.  Order of the sums: a function of n and the inputs alone; no f64 atomic; two calls return the same
 * bytes in every mode.  Scratch: the context's EKF image and partials (vba_odom_kdtree_allocations counts the image) and the map's
 * scan staging (vba_surfel_map_reserve); after a first call within the reserved sizes nothing allocates.
 * VBA_ERR_BAD_ARG before any device work, outputs and the state object untouched: a NULL ctx, m, p, state, cov or st; n < 0;
 * n > 0 with NULL points; neighbors not 1 or 7; gate <= 0; min_matches < 0; min_eig < 0; an empty map; a map of another context;
 * points on another device; a state object on another device.  VBA_ERR_UNSUPPORTED: a sharded context.
 * vba_debug_odom_surfel_sums runs ONE point loop at the pose (R, t) and the reduction of the update launch, with taps to HOST
 * arrays, each of which may be NULL: partial [nb][34] the workgroups' rows, cost [nb] their sums of m / 2, sums [34], cell [n] the
 * chosen cell's row or -1, gate [n].  *nb = min(ceil(n / 256), 1024); cap_rows < nb with partial or cost given: VBA_ERR_CAPACITY. */
typedef struct {
  double gate;
  int neighbors, min_matches;
  double min_eig;
} vba_surfel_odom_params;
void vba_surfel_odom_default_params(vba_surfel_odom_params *p);   /* 3.0, 7, 30, 0.0 */
int vba_odom_surfel_update(vba_ctx *ctx, vba_surfel_map *m, int n, const double *pnt_body /* [n][3], HOST or DEVICE */,
                           const vba_surfel_odom_params *p, double *state /* [25] in/out */, double *cov /* [225] in/out */, int *ok,
                           vba_odom_report *report /* may be NULL */);
int vba_odom_surfel_update_on_state(vba_ctx *ctx, vba_odom_state *st, vba_surfel_map *m, int n, const double *d_pnt_body,
                                    const vba_surfel_odom_params *p, int *ok, vba_odom_report *report, double *state_out);
int vba_debug_odom_surfel_sums(vba_ctx *ctx, vba_surfel_map *m, int n, const double *pnt_body, const vba_surfel_odom_params *p,
                               const double *R, const double *t, int cap_rows, double *partial /* [cap_rows][34] */,
                               double *cost /* [cap_rows] */, double *sums /* [34] */, int *cell, unsigned char *gate, int *nb);

#ifdef __cplusplus
}
#endif
#endif /* VOXELBA_H */
