// Private header of libvoxelba.so's translation units ("source layout"): the context, the handle structs that more than one
// unit reads, and the declarations of the host functions and kernels that one unit defines and another calls.  It defines no kernel.
#pragma once
#include "../../include/voxelba.h"
#include "vba_types.hpp"
#include "vba_common.hpp"
#include "vba_mem.hpp"
#include "vba_stores.hpp"
#include "vba_launch.hpp"
#include "vba_btcgen.hpp"
#include "vba_scanlog_ring.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // TYPES only: the entry points are resolved at run time (rccl_api in voxelba.hip), the library does not link librccl
#include <array>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

using namespace vba;

// The one check of a runtime call: a failure leaves "<the call as written>: <the runtime's text>" in `err`, the error string itself or the
// context that holds it (hipchk_err), and returns VBA_ERR_HIP.  HIPCHK(ctx, expr) is an alias, not a wrapper: an argument handed on through
// a second macro is expanded before it is stringified, and the message would spell hipEventDisableTiming as 0x2.
#define VBA_HIPCHK(err, expr)                                                                    \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      hipchk_err(err) = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
      return VBA_ERR_HIP;                                                                        \
    }                                                                                            \
  } while (0)
#define HIPCHK VBA_HIPCHK

namespace vba {
struct TimedSpan { hipEvent_t a, b; };

// Layout of vba_ctx::h_pin in doubles: poses [W][12] (upload_poses), the download stage (fetch: n doubles, reserving n + kPinFixed; *hess of
// vba_lm_end: (6W)^2), this rank's voxel count on its way through the all-reduce of vba_lm_begin (device partner: d_scal + kScalCount), the end
// of the fixed part; vba_create reserves kPinCreate + nout_of(W), vba_lm_end kPinCreate + (6W)^2
constexpr size_t kPinPoses = 0, kPinStage = 32768, kPinCount = 60000, kPinFixed = 65536, kPinCreate = kPinFixed + 1024;
constexpr int kScalCount = 8;
static_assert(kPinPoses + (size_t)VBA_MAX_WIN_DEV * 12 <= kPinStage, "the pose region ends before the stage");
static_assert(kPinStage + (size_t)36 * VBA_MAX_WIN_DEV * VBA_MAX_WIN_DEV <= kPinCount, "the *hess stage of vba_lm_end ends before the count slot");
static_assert(kPinCount < kPinFixed && kPinFixed <= kPinCreate, "the fixed part fits inside what vba_create reserves");

// Diagnostic switches (in-kernel stamps, host-side phase timers, ablation forms) exist only in a -DVBA_DIAG build (make diag ->
// libvoxelba_diag.so, tools/README.md); the shipped library reads no environment variable.  Internal linkage: the diagnostic library links
// -DVBA_DIAG objects of the units that call this (csrc/Makefile, DIAG_UNITS) with plain objects of the others.
static inline const char *diag_env(const char *name) {
#ifdef VBA_DIAG
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
}
namespace vbh { struct OdomEkf; }   // vba_odom_ekf.hpp

struct vba_ctx {
  vba_options opt;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;

  // factor store (HBM, SoA): fv is the view the kernels take, refreshed from its owners by factor_reserve
  FactorView fv{};
  DevMem<double> fv_rows[6];      // cl, fix, coe, eigval, eigvec, pcr
  DevMem<unsigned int> fv_occ;
  DevMem<int> fv_tiles;
  int nvox = 0;   // voxels stored
  int nvox_global = 0;   // the same summed over the ranks (set by vba_lm_begin when the factor store is sharded)
  int cap = 0;    // capacity = stride
  DevMem<double> d_poses;        // [W][12]
  DevMem<double> d_partial;      // workgroup partials
  DevMem<double> d_out;          // reduced Hessian pass, tile layout (vba_kernels_factor.hpp)
  DevMem<double> d_full;         // the same in full layout [H | g | r] for host consumers
  DevMem<double> d_scal;         // reduced residual scalar
  PinMem<double> h_pin;          // pinned host staging
  DevMem<char> d_stage;          // AoS upload staging

  // multi-GPU
  vba_allreduce_fn allreduce = nullptr;
  void *allreduce_user = nullptr;
  int rank = 0, n_ranks = 1;
  bool force_collective = false;  // vba_options::force_collective (rehearsal: run the exchange step with one rank)
  int max_blocks_hess = 256;      // vba_options::hessian_workgroups
  int residual_vpl_from = 45000;  // vba_options::residual_vpl_from
  bool use_h3 = false;            // vba_options::hessian_compact_tiles != 0
  ncclComm_t comm = nullptr;      // RCCL communicator: the exchange step is issued by the library on the context's stream
  bool own_comm = false;
  bool collective_off = false;    // replica phases (bottom-layer HBA windows) run their LM loops without the exchange step
  bool collective() const { return !collective_off && (allreduce || comm) && (n_ranks > 1 || force_collective); }

  // timing
  bool timing = false;
  std::string timing_only;        // when non-empty only this kernel family is bracketed by events
  int timing_every = 1; unsigned timing_ctr = 0;   // bracket every n-th launch of the selected family
  int lm_spec = LM_SPEC;          // damping candidates per solve launch
  std::vector<std::array<double, 450>> covinv_cache; size_t covinv_next = 0;   // li_ba_device: (cov, cov^-1) of recently seen IMU factors
  std::map<std::string, std::vector<TimedSpan>> spans;

  // device-resident LM state (lm_begin / lm_iterate / lm_end)
  DevMem<LmDev> d_lm;
  PinMem<LmDev> h_lm;             // pinned mirror (download side)
  // vba_lm_begin copies nothing: it leaves the begin poses here and the first LM kernel of the call writes the image (LmInit), or
  // lm_init_flush does for callers whose first kernel is not a fused site
  struct { bool pending = false; int dbg = 0; double x[VBA_MAX_WIN_DEV * 12]; } lm_init;
  DevMem<double> d_raw;           // last valid all-reduced [H|g|r] (multi-rank only; single rank reads d_out in place)
  struct { bool active = false; int thd_num = 2; bool have_hess = false; bool pending_update = false; int k4_nb = 0; } lm;   // pending_update: the accept/reject step of the last iteration rides in the next Hessian pass
  DevMem<double> d_k4part;        // residual-pass partials of the LM loop (the Hessian pass reuses d_partial while they are still read)   // have_hess: [H|g|r] of the next solve is already reduced (multi-rank)
  std::vector<double> trace;

  // device-resident LI-BA (vba_kernels_li.hpp)
  DevMem<LiDev> d_li;
  DevMem<double> d_imu, d_himu, d_gimu;

  MapStore map;
  GbaStore gba;
  BigStore big;                   // arbitrary-window path (top-level global BA)
  DevMem<double> d_kdtree[2];     // pl_tree of the initialisation odometry (float-valued xyz), ping-pong for the re-sampling
  int kd_n = 0, kd_cur = 0;
  // vba_odom_lio_state_estimation_kdtree_resident: scratch sized by the scan (planes, partials, candidates), scratch
  // sized by map + scan (the re-sampler's count / first arrays and work area); the loop's state and pinned image are d_odom / h_odom
  // below.  kd_allocs / kd_bytes count these and the map's two halves, cumulatively (a freed block is not subtracted).
  DevMem<char> d_kdscan; size_t kdscan_pts = 0;
  DevMem<char> d_kdws; size_t kdws_pts = 0;
  int kd_allocs = 0; int64_t kd_bytes = 0;
  DevMem<double> d_refpts;        // submap cloud staging (HBA_add_edge)
  DevMem<double> d_lipack;        // li_ba_device: results gathered for one D2H copy
  DevMem<double> d_liscr;         // k_li_solve at W > 10: staged matrix / L outside the LDS
  DevMem<double> d_hba_all;       // vba_hba_global: keyframe clouds + submap clouds, kept across calls
  std::vector<vba_ctx *> hba_workers;                         // vba_hba_global: extra contexts (own stream, own octree) that optimise bottom-layer windows side by side
  DevMem<char> d_init;            // vba_motion_init: raw clouds (uploaded once per call), blurred rows, pose tables
  // loop retrieval (vba_btc_*): the query upload, the per-(query, cell) counts and the ICP state are shared by the context's databases
  DevMem<char> d_btcq; PinMem<char> h_btcq;
  DevMem<int> d_btccnt;
  DevMem<BtcIcpDev> d_icp; PinMem<BtcIcpDev> h_icp;
  DevMem<unsigned long long> d_icpkey;
  DevMem<double> d_icppart;
  // pose-graph optimisation (vba_pgo_optimize): graph structure and per-update work areas, and the dense skeleton system; grow-only
  DevMem<char> d_pgo;
  DevMem<double> d_pgoAb;
  // vba_kf_export_world: the per-keyframe table (pinned upload ring, so that a call need not drain the stream before
  // it writes the next image, and the device copy) and the staging of host output; grow-only
  static const int kExpRing = 4;
  PinMem<char> h_exp[kExpRing]; hipEvent_t exp_ev[kExpRing] = {nullptr}; int exp_next = 0;
  DevMem<char> d_exp;                                   // keyframes
  DevMem<float4> d_expout;                              // records
  std::vector<long long> exp_first; std::vector<int> exp_kbase;   // host scratch: exported points before every keyframe, keyframes before every store
  // vba_kf_voxel_export: the work arrays of a sequence of up to `pts` records: the table and the sums (slots_of(pts)
  // entries each), every record's slot, the workgroup counts with the total behind them, the pinned image of that total; a
  // deterministic context also holds the sort arrays skey | idx | sidx (sort_stride bytes each) | rocPRIM scratch (tmp_bytes) for
  // `sort_pts` records.  Grow-only; allocs / bytes count these and what a call or reserve adds to the export's table and staging.
  struct {
    size_t pts = 0, sort_pts = 0, sort_stride = 0, tmp_bytes = 0;
    DevMem<char> tab, sort; DevMem<double> sum; DevMem<unsigned int> slot; DevMem<int> blk; PinMem<int> h_n;
    int allocs = 0; int64_t bytes = 0;
  } vx;
  // vba_odom_lio_state_estimation_resident: the loop's device state, its pinned image (parameter block up, result
  // block down; also those of the kd-tree variant, §18) and the point loop's workgroup partials; grow-only
  DevMem<vbh::OdomEkf> d_odom; PinMem<vbh::OdomEkf> h_odom;
  DevMem<double> d_odom_part;

  void set_error(const std::string &s) { err = s; }
};
inline std::string &hipchk_err(std::string &err) { return err; }      // where VBA_HIPCHK / HIPCHK leave their message
inline std::string &hipchk_err(vba_ctx *c) { return c->err; }

// loop retrieval (vba_btc.hip); the keyframe store writes the generator's point buffer (db->gen->xyz)
struct vba_btc_db {
  vba_ctx *ctx = nullptr;
  vba_btc_config cfg{};
  int nstd = 0, cap = 0;                     // descriptors stored / capacity (rows)
  BtcStds d{};                               // the view the kernels take of the six arrays below (btc_reserve_rows)
  DevMem<double> tri, cen, loc; DevMem<unsigned long long> bits; DevMem<int> summ, frame;
  std::vector<int> tab;                      // host mirror of the cell table, 8 ints per slot (vba_kernels_btc.hpp)
  int tab_mask = 0, ncell = 0;
  DevMem<int> d_tab;
  int nchunk = 0, chunk_cap = 0;
  DevMem<int> d_ent, d_next;
  std::vector<int> off{0}, seq;              // plane clouds: point offsets, header.seq
  DevMem<float> d_pc; size_t pc_cap = 0;
  DevMem<int> d_off; int off_cap = 0;
  int mcap = 0; DevMem<int> d_m;             // match list and per-candidate pair lists: mq | md | mf | pq | pd, mcap each
  int vcap = 0; DevMem<int> d_votes;
  DevMem<int> d_cand, d_total; DevMem<double> d_cres, d_res; PinMem<double> h_res;
  bool have_search = false;                  // the last search ran the kernels (n > 0)
  // descriptor generation (vba_btc_generate_stds): its configuration, device buffers, the AddSTDescs count (current_frame_id_)
  // and the corners of the last call
  vba_btc_gen_config gcfg{};
  BtcGen *gen = nullptr;
  int n_add = 0;
  std::vector<double> last_loc; std::vector<uint64_t> last_bits;
  BtcCfgDev dev_cfg() const {
    BtcCfgDev f;
    f.skip_near = cfg.skip_near_num; f.cand_num = cfg.candidate_num; f.rough = cfg.rough_dis_threshold; f.sim = cfg.similarity_threshold;
    f.icp = cfg.icp_threshold; f.normal = cfg.normal_threshold; f.dis = cfg.dis_threshold;
    return f;
  }
  BtcIndex index() const { BtcIndex ix; ix.tab = d_tab; ix.mask = tab_mask; ix.ent = d_ent; ix.next = d_next; return ix; }
};

// keyframe store (vba_kf.hip); the loop map reads its clouds and poses
struct vba_kf_store {
  vba_ctx *ctx = nullptr;
  // the keyframes: points (their own frame, float values in doubles) and covariance diagonals, ragged by off
  DevMem<double> d_pnt; DevMem<float> d_var; size_t cap = 0;
  std::vector<int> off{0};
  struct Meta { double x0[12]; int id; double jour; int exist; };
  std::vector<Meta> kf;
  // scratch of one merge of up to mcap points: staged host input, merged cloud (also the world points of a load), gathered covariance
  // diagonals, per-voxel counts, the down-sampler's work area; pinned: gathered diagonals of a host covariance array
  size_t mcap = 0;
  DevMem<double> d_src, d_merge, d_mdiag; PinMem<double> h_diag;
  DevMem<int> d_cnt; DevMem<char> d_ws;
  // per-scan transforms [tcap][12] and offsets [tcap + 1]: pinned image and device copy; the voxel count of a build (pinned)
  int tcap = 0; PinMem<char> h_tab; DevMem<char> d_tab; PinMem<int> h_n;
  hipEvent_t ev = nullptr;
  int allocs = 0; int64_t bytes = 0;
  int hist = 0; std::vector<float> hist_pos;   // history_kfsize, pl_kdmap
  int last_m = 0;                              // voxels of the last build (their counts stay in d_cnt)
};

// scan log (vba_scanlog.hip); the keyframe store and the loop update read its arena in place
struct vba_scanlog {
  vba_ctx *ctx = nullptr;
  // one arena of ring.cap() points used as a ring of whole scans: body points and covariance rows as the map's ring held them
  DevMem<double> d_pnt, d_var;
  std::mutex mu;                   // the bookkeeping (ring, read_pending, counters); held across a wait only by a push or reserve that grows
  ScanRing ring;
  std::vector<ScanRing::Move> moves;          // host scratch of a growth
  DevMem<float> d_xyz;                        // the float form of one scan on its way out (vba_scanlog_read)
  // push_ev: behind the newest capture on the log's stream, for readers on other streams; read_ev: behind the newest reader that
  // returned with its work still queued on another stream, for the push that may write over what it reads
  hipEvent_t push_ev = nullptr, read_ev = nullptr;
  bool read_pending = false;
  int allocs = 0; int64_t bytes = 0;
};

// odometry state (vba_odom.hip); the scan frame reads its pose table in place
struct vba_odom_state {
  vba_ctx *ctx = nullptr;
  DevMem<double> d_blk;            // [state 25 | P 225 | 6 unused]
  // sized by cap IMU rows: the pose table [cap - 1][22] | end_pose 12 | extrinsic 12 (the parameter block of k_undistort), the upload
  // [parameters 16 | imu cap x 7] with its pinned image
  int cap = 0;
  DevMem<double> d_tab, d_up; PinMem<double> h_up;
  PinMem<double> h_blk;            // set / get / poses: one pinned block of max(256, table) doubles
  hipEvent_t up_ev = nullptr;      // behind the newest copy out of h_up or h_blk
  bool up_pending = false;
  hipEvent_t res_ev = nullptr;     // behind the result download of the scan-to-map update, ahead of the copy back into the block
  int n_poses = 0;                 // rows of the table that the last propagation wrote
  hipStream_t last = nullptr;      // the stream of the last call that queued work on the block
  int allocs = 0; int64_t bytes = 0;
};

namespace vba {

// ---------------------------------------------------------------- vba_odom.hip (vba_kernels_imu_ekf.hpp)
// Orders `stream` behind the work queued on the state's buffers by its last user.
int odom_state_order(vba_odom_state *st, hipStream_t stream, std::string &err);
// the map's pose image from the state block, launched by map_cut_voxel
__global__ __launch_bounds__(64) void k_odom_state_pose(const double *blk, double *poses);

// ---------------------------------------------------------------- vba_scanlog.hip
// Scans first .. first + k - 1 for a reader on `stream`, which is ordered behind their captures: starts[i] = the first arena row of
// scan i, rel[i] = the points before scan i among the k (rel[k] = their sum).  VBA_ERR_BAD_ARG when the range is not wholly live
// or its points exceed `max_points`; nothing is queued then.  stream == nullptr: the fields only, nothing is queued.
struct ScanLogView { const double *d_pnt, *d_var; std::vector<int> starts, rel; };
int scanlog_view(vba_scanlog *l, int64_t first, int k, long long max_points, hipStream_t stream, ScanLogView *out);
// a reader that returns with work on the arena still queued on `stream` leaves its mark for the next push
int scanlog_reader_queued(vba_scanlog *l, hipStream_t stream);

// ---------------------------------------------------------------- voxelba.hip
void span_begin(vba_ctx *c, const char *name, TimedSpan &s);
void span_end(vba_ctx *c, const char *name, TimedSpan &s);
int ensure_pin(vba_ctx *c, size_t n);
int ensure_stage(vba_ctx *c, size_t bytes);
int factor_reserve(vba_ctx *c, int need);
void factor_update_mask(vba_ctx *c, int base, int n);
int ctx_allgather(vba_ctx *c, double *buf, size_t chunk);
bool li_device_supported(int W);

// ---------------------------------------------------------------- vba_hba.hip (vba_kernels_big.hpp)
// the damped solve of the any-window path, also VBA_SOLVE_DENSE of vba_debug_solve in voxelba.hip
void big_pivot_order(const double *hd, double u, int n, int *ord);
double big_q1(const double *dxi, const double *hd, const double *g, double u, int n);
int big_solve(BigStore &s, hipStream_t st, const int *ord, double u, double *dxi, std::string &err);
// its dense LDL^T, also the skeleton solve of vba_pgo.hip
__global__ __launch_bounds__(256) void k_bigl_panel(double *__restrict__ Ab, double *__restrict__ Tb, int NP, int ld, int k0);
__global__ __launch_bounds__(256) void k_bigl_update(double *__restrict__ Ab, const double *__restrict__ Tb, int NP, int ld, int k0);
__global__ __launch_bounds__(64) void k_bigl_bs_tri(double *__restrict__ Ab, int NP, int ld, int n, int lo);
__global__ __launch_bounds__(256) void k_bigl_bs_gemv(double *__restrict__ Ab, int NP, int ld, int n, int lo);

// ---------------------------------------------------------------- vba_btc.hip
int btc_gen_ensure(vba_btc_db *db, int64_t points, int64_t cells, size_t corners);
int btc_generate_check(vba_btc_db *db, int n, int cap, double *rows, uint64_t *bits, int *n_stds);
int btc_generate_impl(vba_btc_db *db, int n, const float *xyz, int id, int cap, double *rows, uint64_t *bits, int *n_stds);

// ---------------------------------------------------------------- vba_kf.hip (vba_kernels_scan.hpp): the scan passes that the scan
// frame of vba_scan.hip chains on its own buffers
int ds_core(vba_ctx *c, hipStream_t stream, int mode, int n, const double *d_in, const double *d_var, int vrow, int vstep, double voxel_size,
            bool det, const DsWork &w);
size_t kf_ws_layout(vba_ctx *c, int n, bool det, char *base, DsWork *w, int *status);
__global__ void k_iota(int *__restrict__ a, int n);
__global__ __launch_bounds__(256) void k_ds_scan(int nb, int *__restrict__ blk, int *__restrict__ n_out);
__global__ __launch_bounds__(256) void k_ds_emit(int n, const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, const int *__restrict__ blk,
                                                 double *__restrict__ out, int *__restrict__ count, int *__restrict__ first, double *__restrict__ vout, int mode);
__global__ void k_undistort(int n, double *__restrict__ pnt, const double *__restrict__ curv, int m, const double *__restrict__ prm);
__global__ void k_var_init(int n, const double *__restrict__ pin, double *__restrict__ pout, double *__restrict__ var, const double *__restrict__ ext,
                           float range_inc, float degree_inc);

// ---------------------------------------------------------------- vba_scan.hip
// Stage 0 of a decoded frame (decoded, sorted, cut; vba_scan_prepare leaves it alone) for a reader on `stream`, which is ordered
// behind the decode.  false: the frame holds no decoded cloud.  stream == nullptr: the fields only, nothing is queued.
struct ScanStage0 { vba_ctx *ctx; int n; const double *pnt, *curv; };
bool scan_frame_stage0(vba_scan_frame *f, hipStream_t stream, ScanStage0 *out);

// ---------------------------------------------------------------- vba_map.hip
void map_init(MapStore &s, const vba_options &o);
std::vector<DevArr> node_arrays(MapView &v, int W);
std::vector<DevArr> scan_arrays(MapView &v, int W);
std::vector<DevArr> fix_arrays(MapView &v);
int map_read_counters(MapStore &s, hipStream_t st, std::string &err);
int map_hash_alloc(MapStore &s, unsigned int cap, hipStream_t st, std::string &err);
int map_base(MapStore &s, hipStream_t st, std::string &err);
void map_free(MapStore &s);
bool is_device_ptr(const void *p);
int map_cut_voxel(MapStore &s, hipStream_t st, int win_count, int n, const double *pnt_body, const double *var, const double *pose,
                  bool multi, std::string &err, const double *cov6 = nullptr, const double *d_state_blk = nullptr);
int map_cut_voxel_fix(MapStore &s, hipStream_t st, int n, const double *pnt_world, double jour, std::string &err);
int map_recut(MapStore &s, hipStream_t st, int win_count, const double *poses, bool multi, std::string &err, int *n_factors);
int map_extract_factors(MapStore &s, hipStream_t st, FactorView f, std::string &err, int *n_factors);
int map_margi(MapStore &s, hipStream_t st, int win_count, const double *poses, double jour, FactorView f, int nfac, std::string &err);
int map_slide(MapStore &s, int mgsize);
int map_reset(MapStore &s, hipStream_t st, std::string &err);
int map_num_roots(MapStore &s, hipStream_t st, bool slide);
int map_stats(MapStore &s, hipStream_t st, long long *out8, std::string &err);
int map_dump_leaves(MapStore &s, hipStream_t st, double *out, int max_leaves, std::string &err);
int map_dump_plane_var(MapStore &s, hipStream_t st, double *out, int max_leaves, std::string &err);
int map_prune(MapStore &s, hipStream_t st, double jour, int dist, std::string &err);
int map_odom_resident(MapStore &s, hipStream_t st, vbh::OdomEkf *d_S, vbh::OdomEkf *h_img, int n, const double *d_pts,
                      const double *d_var, double *d_partial, std::string &err);
// its four (point loop, update) pairs alone, on an image that is already in d_S
int map_odom_queue(MapStore &s, hipStream_t st, vbh::OdomEkf *d_S, int n, const double *d_pts, const double *d_var, double *d_partial,
                   std::string &err);
int map_odom_debug_sums(MapStore &s, hipStream_t st, vbh::OdomEkf *d_S, const vbh::OdomEkf *h_img, int n, const double *d_pts,
                        const double *d_var, double *d_partial, double *d_sums, int *nb_out, std::string &err);
int map_debug_plane_update(hipStream_t st, int n, const double *in, double *out, std::string &err);
// the update launch of the resident EKF loops (vba_kernels_odom.hpp), also the kd-tree variant's in vba_odom.hip, and the launch that
// stores its sums alone (vba_debug_odom_sums)
__global__ __launch_bounds__(256) void k_odom_update(vbh::OdomEkf *S, const double *__restrict__ partial, int nb, int iter, int kd);
__global__ __launch_bounds__(256) void k_odom_sums(const double *__restrict__ partial, int nb, double *__restrict__ sums);
int map_fix_source_ensure(MapStore &s, hipStream_t st, size_t nodes, size_t fix, size_t n, std::string &err);
int map_cut_voxel_fix_source(MapStore &s, hipStream_t st, int n, const FixSource &src, double jour, std::string &err);
// fills the map's root table with the empty key, also the hash tables of vba_kernels_big.hpp in vba_hba.hip
__global__ void k_fill_u64(unsigned long long *p, unsigned long long v, size_t n);
// the one-workgroup exclusive scan of the map's stable compactions, also the match-list offsets of vba_btc.hip
__global__ __launch_bounds__(1024) void k_det_scan(int *a, int n_max, int *cnt, int which_n, int cap_n, int which_out);

}  // namespace vba
