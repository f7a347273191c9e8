// Private header of libvoxelba.so's translation units ("source layout"): the BA core's context, the check macros, the pinned
// layout, and the declarations of what voxelba.hip, vba_map.hip and vba_hba.hip define and another unit calls.  The satellite units'
// context state is struct CtxSat (vba_sat.hpp), held here as a pointer; a handle struct has a header of its own.  It defines no kernel.
#pragma once
#include "../../include/voxelba.h"
#include "vba_types.hpp"
#include "vba_common.hpp"
#include "vba_mem.hpp"
#include "vba_stores.hpp"
#include "vba_launch.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // TYPES only: the entry points are resolved at run time (rccl_api in voxelba.hip), the library does not link librccl
#include <array>
#include <cstdlib>
#include <map>
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
struct CtxSat;                      // vba_sat.hpp

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
  bool lm_trial_fused = true;     // vba_options::lm_trial_launches != 2: solve + residual pass of the trial poses in one launch (k_lm_trial)
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
  DevMem<double> d_refpts;        // submap cloud staging (HBA_add_edge)
  DevMem<double> d_lipack;        // li_ba_device: results gathered for one D2H copy
  DevMem<double> d_liscr;         // k_li_solve at W > 10: staged matrix / L outside the LDS
  DevMem<double> d_hba_all;       // vba_hba_global: keyframe clouds + submap clouds, kept across calls
  std::vector<vba_ctx *> hba_workers;                         // vba_hba_global: extra contexts (own stream, own octree) that optimise bottom-layer windows side by side
  CtxSat *sat = nullptr;          // the satellite units' state: made by vba_create, released by vba_destroy, read by its owners alone

  void set_error(const std::string &s) { err = s; }
};
inline std::string &hipchk_err(std::string &err) { return err; }      // where VBA_HIPCHK / HIPCHK leave their message
inline std::string &hipchk_err(vba_ctx *c) { return c->err; }

namespace vba {

// ---------------------------------------------------------------- voxelba.hip
void span_begin(vba_ctx *c, const char *name, TimedSpan &s);
void span_end(vba_ctx *c, const char *name, TimedSpan &s);
int ensure_pin(vba_ctx *c, size_t n);
int ensure_stage(vba_ctx *c, size_t bytes);
int factor_reserve(vba_ctx *c, int need);
void factor_update_mask(vba_ctx *c, int base, int n);
int ctx_allgather(vba_ctx *c, double *buf, size_t chunk);
bool li_device_supported(int W);

// ---------------------------------------------------------------- vba_sat.hip
// Makes c->sat (VBA_ERR_CAPACITY: no host memory) / releases it with its buffers and events and leaves nullptr; the stream has drained.
int ctx_sat_create(vba_ctx *c);
void ctx_sat_release(vba_ctx *c);

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
// the map's one odometry export: ONE point loop (k_odom_match_dev) at the pose of the image d_S; returns the rows [34] of d_partial
// it wrote, 0 for n == 0 or a map never allocated.  The frame around it is vba_odom.hip's (odom_loop_queue).
int map_odom_point_loop(MapStore &s, hipStream_t st, const vbh::OdomEkf *d_S, int n, const double *d_pts, const double *d_var,
                        double *d_partial);
int map_debug_plane_update(hipStream_t st, int n, const double *in, double *out, std::string &err);
// the update launch of the resident EKF loops and the launch that stores its sums alone (vba_kernels_odom.hpp): compiled by the map
// unit, launched by the frame in vba_odom.hip and nowhere else
__global__ __launch_bounds__(256) void k_odom_update(vbh::OdomEkf *S, const double *__restrict__ partial, int nb, int iter, int kd);
__global__ __launch_bounds__(256) void k_odom_sums(const double *__restrict__ partial, int nb, double *__restrict__ sums);
int map_fix_source_ensure(MapStore &s, hipStream_t st, size_t nodes, size_t fix, size_t n, std::string &err);
int map_cut_voxel_fix_source(MapStore &s, hipStream_t st, int n, const FixSource &src, double jour, std::string &err);
// fills the map's root table with the empty key, also the hash tables of vba_kernels_big.hpp in vba_hba.hip
__global__ void k_fill_u64(unsigned long long *p, unsigned long long v, size_t n);
// the one-workgroup exclusive scan of the map's stable compactions, also the match-list offsets of vba_btc.hip
__global__ __launch_bounds__(1024) void k_det_scan(int *a, int n_max, int *cnt, int which_n, int cap_n, int which_out);

// ---------------------------------------------------------------- vba_surfreg.hip
// What the prior-map odometry update of vba_odom.hip (vba_odom_surfel_update*) needs of a surfel map, whose struct
// is private to its unit.  surfel_odom_args_ok: the map belongs to c and has cells, and the n points are host memory or memory of
// c's device.  surfel_odom_stage: *d_pnt = pnt when it is device memory, else the map's scan staging after one stream-ordered copy.
// surfel_odom_queue: ONE point loop (k_sodom_accum) of n > 0 points on st at the pose of the image d_S; returns nb, the rows [34]
// of d_partial it writes.  d_cost [nb], d_cell [n], d_gate [n]: taps, null in the loop.
bool surfel_odom_args_ok(const vba_surfel_map *m, const vba_ctx *c, int n, const double *pnt);
int surfel_odom_stage(vba_surfel_map *m, int n, const double *pnt, const double **d_pnt);
int surfel_odom_blocks(int n);
int surfel_odom_queue(vba_surfel_map *m, hipStream_t st, const vbh::OdomEkf *d_S, int n, const double *d_pnt, double gate, int neighbors,
                      double *d_partial, double *d_cost, int *d_cell, unsigned char *d_gate);

}  // namespace vba
