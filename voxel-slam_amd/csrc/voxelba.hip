// libvoxelba.so — implementation of include/voxelba.h for MI355X (gfx950).
// Host side: context / HBM store management, the three LM drivers (voxel_map.hpp:342-976) and the IMU factor;
// device side: the kernels in vba_kernels_factor.hpp / vba_kernels_map.hpp.  No CPU compute fallback exists.
#include "../../include/voxelba.h"

#define VBA_MAX_WIN_DEV VBA_MAX_WIN
#include "vba_kernels_factor.hpp"
#include "vba_kernels_h3.hpp"
#include "vba_kernels_map.hpp"
#include "vba_kernels_lm.hpp"
#include "vba_kernels_li.hpp"
#include "vba_kernels_scan.hpp"
#include "vba_kernels_gba.hpp"
#include "vba_kernels_big.hpp"
#include "vba_kernels_pgo.hpp"
#include "vba_kernels_kd.hpp"
#include "vba_kernels_init.hpp"
#include "vba_kernels_btc.hpp"
#include "vba_btcgen.hpp"
#include "vba_io.hpp"
#include <cstddef>
#include "vba_hostmath.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // TYPES only: the entry points are resolved at run time (rccl_api below), the library does not link librccl
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include <array>
#include <map>
#include <chrono>
#include <deque>
#include <functional>
#include <algorithm>

using namespace vba;

#define HIPCHK(ctx, expr)                                                                        \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      (ctx)->set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                       \
      return VBA_ERR_HIP;                                                                        \
    }                                                                                            \
  } while (0)

namespace {
struct TimedSpan { hipEvent_t a, b; };

// RCCL entry points, resolved on first use: the copy the process has ALREADY loaded wins (a host program that imported torch carries
// torch/lib/librccl.so; binding to a second build would split the communicator state), then the system librccl.so.1.  A process
// that never asks for the in-library exchange step (vba_rccl_init / vba_set_rccl_comm / vba_rccl_get_unique_id) needs no RCCL at all.
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
  std::string why;
};
const RcclApi &rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    void *h = nullptr;
    if (dlsym(RTLD_DEFAULT, "ncclAllReduce")) h = RTLD_DEFAULT;            // already in the process (e.g. torch's copy)
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) { const char *e = dlerror(); a.why = std::string("librccl.so.1 not found: ") + (e ? e : "?"); return a; }
    bool all = true;
    auto get = [&](const char *name) { void *s = dlsym(h, name); if (!s) { all = false; a.why = std::string("RCCL lacks ") + name; } return s; };
    a.GetUniqueId = (decltype(a.GetUniqueId))get("ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))get("ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))get("ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))get("ncclAllReduce");
    a.AllGather = (decltype(a.AllGather))get("ncclAllGather");
    a.GetErrorString = (decltype(a.GetErrorString))get("ncclGetErrorString");
    a.ok = all;
    return a;
  }();
  return api;
}

// Diagnostic switches (in-kernel stamps, host-side phase timers, ablation forms) exist only in a -DVBA_DIAG build (make diag ->
// libvoxelba_diag.so, tools/README.md); the shipped library reads no environment variable.
inline const char *diag_env(const char *name) {
#ifdef VBA_DIAG
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
}

struct vba_ctx {
  vba_options opt;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;

  // factor store (HBM, SoA)
  FactorView fv{};
  int nvox = 0;   // voxels stored
  int nvox_global = 0;   // the same summed over the ranks (set by vba_lm_begin when the factor store is sharded)
  int cap = 0;    // capacity = stride
  double *d_poses = nullptr;     // [W][12]
  double *d_partial = nullptr;   // workgroup partials
  size_t partial_doubles = 0;
  double *d_out = nullptr;       // reduced Hessian pass, tile layout (vba_kernels_factor.hpp)
  double *d_full = nullptr;      // the same in full layout [H | g | r] for host consumers
  double *d_scal = nullptr;      // reduced residual scalar
  double *h_pin = nullptr;       // pinned host staging
  size_t pin_doubles = 0;
  void *d_stage = nullptr;       // AoS upload staging
  size_t stage_bytes = 0;

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
  LmDev *d_lm = nullptr;
  LmDev *h_lm = nullptr;          // pinned mirror (download side)
  // vba_lm_begin copies nothing: it leaves the begin poses here and the first LM kernel of the call writes the image (LmInit), or
  // lm_init_flush does for callers whose first kernel is not a fused site
  struct { bool pending = false; int dbg = 0; double x[VBA_MAX_WIN_DEV * 12]; } lm_init;
  double *d_raw = nullptr;        // last valid all-reduced [H|g|r] (multi-rank only; single rank reads d_out in place)
  struct { bool active = false; int thd_num = 2; bool have_hess = false; bool pending_update = false; int k4_nb = 0; } lm;   // pending_update: the accept/reject step of the last iteration rides in the next Hessian pass
  int k4part_cap = 0;
  double *d_k4part = nullptr;     // residual-pass partials of the LM loop (the Hessian pass reuses d_partial while they are still read)   // have_hess: [H|g|r] of the next solve is already reduced (multi-rank)
  std::vector<double> trace;

  // device-resident LI-BA (vba_kernels_li.hpp)
  LiDev *d_li = nullptr;
  double *d_imu = nullptr, *d_himu = nullptr, *d_gimu = nullptr;

  MapStore map;
  GbaStore gba;
  BigStore big;                   // arbitrary-window path (top-level global BA)
  double *d_kdtree[2] = {nullptr, nullptr};   // pl_tree of the initialisation odometry (float-valued xyz), ping-pong for the re-sampling
  size_t kd_cap = 0; int kd_n = 0, kd_cur = 0;
  double *d_refpts = nullptr;     // submap cloud staging (HBA_add_edge)
  size_t refpts_doubles = 0;
  double *d_lipack = nullptr; size_t lipack_doubles = 0;       // li_ba_device: results gathered for one D2H copy
  double *d_liscr = nullptr; size_t liscr_doubles = 0;         // k_li_solve at W > 10: staged matrix / L outside the LDS
  double *d_hba_all = nullptr; size_t hba_all_doubles = 0;   // vba_hba_global: keyframe clouds + submap clouds, kept across calls
  std::vector<vba_ctx *> hba_workers;                         // vba_hba_global: extra contexts (own stream, own octree) that optimise bottom-layer windows side by side
  void *d_init = nullptr; size_t init_bytes = 0;            // vba_motion_init: raw clouds (uploaded once per call), blurred rows, pose tables
  // loop retrieval (vba_btc_*): the query upload, the per-(query, cell) counts and the ICP state are shared by the context's databases
  char *d_btcq = nullptr, *h_btcq = nullptr; size_t btcq_bytes = 0;
  int *d_btccnt = nullptr; size_t btccnt_cap = 0;
  BtcIcpDev *d_icp = nullptr, *h_icp = nullptr;
  unsigned long long *d_icpkey = nullptr; size_t icpkey_cap = 0;
  double *d_icppart = nullptr; size_t icppart_cap = 0;
  // pose-graph optimisation (vba_pgo_optimize): graph structure and per-update work areas, and the dense skeleton system; grow-only
  char *d_pgo = nullptr; size_t pgo_bytes = 0;
  double *d_pgoAb = nullptr; size_t pgoAb_bytes = 0;
  // vba_kf_export_world: the per-keyframe table (pinned upload ring, so that a call need not drain the stream before
  // it writes the next image, and the device copy) and the staging of host output; grow-only
  static const int kExpRing = 4;
  char *h_exp[kExpRing] = {nullptr}; hipEvent_t exp_ev[kExpRing] = {nullptr}; int exp_next = 0;
  char *d_exp = nullptr; size_t exp_cap = 0;            // keyframes
  char *d_expout = nullptr; size_t expout_cap = 0;      // records
  std::vector<long long> exp_first; std::vector<int> exp_kbase;   // host scratch: exported points before every keyframe, keyframes before every store

  void set_error(const std::string &s) { err = s; }
};

namespace {

// damping candidates per solve launch (vba_kernels_lm.hpp, "Speculative damping"); 1 = the plain sequential solve.  Read when a
// context is created (vba_options::lm_spec; tests compare the two forms bit for bit).
static const int kMaxDevices = 64;         // per-device "kernel attribute set" flags
static const int kMaxBlocksHess = 256;     // upper bound of vba_options::hessian_workgroups (sizes the partial slab): one workgroup per CU

int nout_of(int W) { return 36 * W * W + 6 * W + 1; }   // full layout [H | g | r]
int nout_tl(int W) {                                      // tile layout produced by k_hessian2 (HessCfg2<W>::NOUT2)
  const int nt16 = (6 * W + 15) / 16;
  return nt16 * (nt16 + 1) / 2 * 256 + 27 * W + 1;
}

static inline bool span_on(vba_ctx *c, const char *name) { return c->timing && (c->timing_only.empty() || c->timing_only == name); }
void span_begin(vba_ctx *c, const char *name, TimedSpan &s) {
  s.a = s.b = nullptr;
  if (!span_on(c, name)) return;
  if (c->timing_every > 1 && (c->timing_ctr++ % c->timing_every) != 0) return;   // sampled bracketing (vba_timing_sample_every)
  hipEventCreate(&s.a); hipEventCreate(&s.b);
  hipEventRecord(s.a, c->stream);
}
void span_end(vba_ctx *c, const char *name, TimedSpan &s) {
  if (!s.a) return;
  hipEventRecord(s.b, c->stream);
  c->spans[name].push_back(s);
}

int ensure_pin(vba_ctx *c, size_t n) {
  if (n <= c->pin_doubles) return VBA_OK;
  if (c->h_pin) hipHostFree(c->h_pin);
  c->h_pin = nullptr; c->pin_doubles = 0;
  HIPCHK(c, hipHostMalloc((void **)&c->h_pin, n * sizeof(double), hipHostMallocDefault));
  c->pin_doubles = n;
  return VBA_OK;
}
int ensure_stage(vba_ctx *c, size_t bytes) {
  if (bytes <= c->stage_bytes) return VBA_OK;
  if (c->d_stage) hipFree(c->d_stage);
  c->d_stage = nullptr; c->stage_bytes = 0;
  HIPCHK(c, hipMalloc(&c->d_stage, bytes));
  c->stage_bytes = bytes;
  return VBA_OK;
}

// (re)allocate the SoA factor store with stride newcap, preserving the first nvox voxels
int factor_reserve(vba_ctx *c, int need) {
  if (need <= c->cap) return VBA_OK;
  int newcap = c->cap ? c->cap : 4096;
  while (newcap < need) newcap *= 2;
  // the SoA rows are `stride` doubles apart and every pass streams ~100 of them at the same offset: a power-of-two stride would
  // put all those streams on the same HBM channels / cache sets, so the stride is skewed by an odd number of 512-byte blocks
  newcap = (newcap + 63) / 64 * 64 + 64 * 33;
  const int W = c->opt.win_size;
  FactorView n = c->fv;
  n.vs = newcap; n.W = W;
  const size_t rows[6] = {(size_t)10 * W, 10, 1, 3, 9, 10};
  double **np[6] = {&n.cl, &n.fix, &n.coe, &n.eigval, &n.eigvec, &n.pcr};
  double *op[6] = {c->fv.cl, c->fv.fix, c->fv.coe, c->fv.eigval, c->fv.eigvec, c->fv.pcr};
  for (int k = 0; k < 6; k++) {
    HIPCHK(c, hipMalloc((void **)np[k], rows[k] * newcap * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(*np[k], 0, rows[k] * newcap * sizeof(double), c->stream));
    if (c->nvox > 0 && op[k])
      HIPCHK(c, hipMemcpy2DAsync(*np[k], (size_t)newcap * sizeof(double), op[k], (size_t)c->cap * sizeof(double),
                                 (size_t)c->nvox * sizeof(double), rows[k], hipMemcpyDeviceToDevice, c->stream));
  }
  unsigned int *oocc = c->fv.occ;
  int *otiles = c->fv.tiles;
  HIPCHK(c, hipMalloc((void **)&n.tiles, ((size_t)4 * newcap + 16) * sizeof(int)));
  HIPCHK(c, hipMemsetAsync(n.tiles, 0, ((size_t)4 * newcap + 16) * sizeof(int), c->stream));
  HIPCHK(c, hipMalloc((void **)&n.occ, (size_t)newcap * sizeof(unsigned int)));
  HIPCHK(c, hipMemsetAsync(n.occ, 0, (size_t)newcap * sizeof(unsigned int), c->stream));
  if (c->nvox > 0 && oocc) HIPCHK(c, hipMemcpyAsync(n.occ, oocc, (size_t)c->nvox * sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 6; k++) if (op[k]) hipFree(op[k]);
  if (oocc) hipFree(oocc);
  if (otiles) hipFree(otiles);
  c->fv = n;
  if (c->nvox > 0 && c->use_h3) hipLaunchKernelGGL(k_factor_tiles, dim3(1), dim3(1024), 0, c->stream, c->fv, c->nvox);   // (the table lives in the new allocation)
  c->cap = newcap;
  return VBA_OK;
}

// the occupancy masks of voxels [base, base + n) follow every write of the cluster rows
void factor_update_mask(vba_ctx *c, int base, int n) {
  if (n > 0) hipLaunchKernelGGL(k_factor_mask, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->fv, base, n);
  // the Hessian pass' tile table of the whole store [0, base + n) (vba_kernels_h3.hpp)
  if (base + n > 0 && c->use_h3) hipLaunchKernelGGL(k_factor_tiles, dim3(1), dim3(1024), 0, c->stream, c->fv, base + n);
}

int upload_poses(vba_ctx *c, const double *poses) {
  const int W = c->opt.win_size;
  int st = ensure_pin(c, 65536);
  if (st) return st;
  std::memcpy(c->h_pin, poses, (size_t)W * 12 * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->d_poses, c->h_pin, (size_t)W * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return VBA_OK;
}

// The by-value init argument of the LM kernels.  take: consume the context's pending init (the launch that receives the argument
// writes the LmDev image); otherwise the argument is off.
template <int W>
LmInit<W> lm_init_arg(vba_ctx *c, bool take) {
  LmInit<W> a{};
  if (take && c->lm_init.pending) {
    std::memcpy(a.x, c->lm_init.x, sizeof(a.x));
    a.dst = c->d_lm; a.on = 1; a.dbg = c->lm_init.dbg;
    c->lm_init.pending = false;
  }
  return a;
}
// Everything that reads d_lm and is not a fused site calls this first: a pending init becomes a launch of its own.
int lm_init_flush(vba_ctx *c) {
  if (!c->lm_init.pending) return VBA_OK;
  switch (c->opt.win_size) {
#define VBA_LI_CASE(WW) case WW: hipLaunchKernelGGL(k_lm_init<WW>, dim3(1), dim3(256), 0, c->stream, lm_init_arg<WW>(c, true)); break;
    VBA_LI_CASE(2) VBA_LI_CASE(3) VBA_LI_CASE(4) VBA_LI_CASE(5) VBA_LI_CASE(6) VBA_LI_CASE(7) VBA_LI_CASE(8) VBA_LI_CASE(9) VBA_LI_CASE(10)
    VBA_LI_CASE(11) VBA_LI_CASE(12) VBA_LI_CASE(13) VBA_LI_CASE(14) VBA_LI_CASE(15) VBA_LI_CASE(16)
#undef VBA_LI_CASE
    default: return VBA_ERR_UNSUPPORTED_WINDOW;
  }
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}

template <int W>
int launch_hessian2_t(vba_ctx *c, const double *poses_dev, const int *gate, int head, int end, int *nblocks_out, LmDev *lm, const double *k4p, int k4nb,
                      const LiJob &li, size_t li_lds, bool init) {
  using C = HessCfg2<W>;
  const int ntiles = (end - head + C::TV - 1) / C::TV;
  const int maxb = li.dev ? c->max_blocks_hess - 1 : c->max_blocks_hess;      // (the IMU workgroup of LI-BA takes a CU of its own)
  int nb = ntiles < maxb ? ntiles : maxb;
  if (nb < 1) nb = 1;
  static bool attr_set[kMaxDevices] = {false};      // the attribute is per DEVICE (a process may hold contexts on several)
  if (!attr_set[c->device % kMaxDevices]) {
    // (the IMU workgroup of LI-BA needs up to 150 KB at W = 16; a lidar-only launch asks for C::LDS_BYTES)
    const size_t li_max = 150 * 1024;
    hipFuncSetAttribute((const void *)k_hessian2<W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(C::LDS_BYTES > li_max ? C::LDS_BYTES : li_max));
    attr_set[c->device % kMaxDevices] = true;
  }
  long long *stamps = nullptr;
  static const bool want_stamps = diag_env("VBA_K3_STAMPS") != nullptr;     // -DVBA_DIAG builds only
  if (want_stamps) {
    static long long *d_st = nullptr;
    if (!d_st) hipMalloc((void **)&d_st, (size_t)kMaxBlocksHess * 16 * 8);
    hipMemsetAsync(d_st, 0, (size_t)kMaxBlocksHess * 16 * 8, c->stream);
    stamps = d_st;
  }
  const size_t lds = (li.dev && li_lds > C::LDS_BYTES) ? li_lds : C::LDS_BYTES;
  hipLaunchKernelGGL(k_hessian2<W>, dim3(nb + (li.dev ? 1 : 0)), dim3(C::NT), lds, c->stream, c->fv, poses_dev, head, end, ntiles, c->d_partial, gate, stamps, lm, k4p, k4nb,
                     nb, li, lm_init_arg<W>(c, init));
  if (want_stamps) {
    std::vector<long long> h((size_t)nb * 16);
    hipStreamSynchronize(c->stream);
    hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost);
    long long t0 = h[0];
    for (int b = 0; b < nb; b++) if (h[(size_t)b * 16] && h[(size_t)b * 16] < t0) t0 = h[(size_t)b * 16];
    for (int b : {0, 1, nb / 2, nb - 1}) {
      fprintf(stderr, "[k3 stamps] wg %d:", b);
      for (int i = 0; i < 15; i++) fprintf(stderr, " %lld", h[(size_t)b * 16 + i] ? h[(size_t)b * 16 + i] - t0 : -1);
      fprintf(stderr, "\n");
    }
    long long tmax = 0;
    for (int b = 0; b < nb; b++) if (h[(size_t)b * 16 + 14] - t0 > tmax) tmax = h[(size_t)b * 16 + 14] - t0;
    fprintf(stderr, "[k3 stamps] last workgroup ends at %lld ticks (100 MHz wall clock: 1 tick = 10 ns)\n", tmax);
  }
  *nblocks_out = nb;
  return VBA_OK;
}

template <int W>
int launch_hessian3_t(vba_ctx *c, const double *poses_dev, const int *gate, int *nblocks_out, LmDev *lm, const double *k4p, int k4nb, const LiJob &li, size_t li_lds) {
  using C = HessCfg3<W>;
  const int nb = li.dev ? c->max_blocks_hess - 1 : c->max_blocks_hess;      // (the IMU workgroup of LI-BA takes a CU of its own)
  static bool attr_set[kMaxDevices] = {false};
  if (!attr_set[c->device % kMaxDevices]) {
    const size_t li_max = 150 * 1024;
    hipFuncSetAttribute((const void *)k_hessian3<W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(C::LDS_BYTES > li_max ? C::LDS_BYTES : li_max));
    attr_set[c->device % kMaxDevices] = true;
  }
  const size_t lds = (li.dev && li_lds > C::LDS_BYTES) ? li_lds : C::LDS_BYTES;
  long long *stamps = nullptr;
  static const bool want_stamps = diag_env("VBA_K3_STAMPS") != nullptr;     // -DVBA_DIAG builds only
  if (want_stamps) {
    static long long *d_st = nullptr;
    if (!d_st) hipMalloc((void **)&d_st, (size_t)kMaxBlocksHess * 16 * 8);
    hipMemsetAsync(d_st, 0, (size_t)kMaxBlocksHess * 16 * 8, c->stream);
    stamps = d_st;
  }
  hipLaunchKernelGGL(k_hessian3<W>, dim3(nb + (li.dev ? 1 : 0)), dim3(C::NT), lds, c->stream, c->fv, poses_dev, c->nvox, c->d_partial, gate, lm, k4p, k4nb, nb, li, stamps);
  if (want_stamps) {
    std::vector<long long> h((size_t)nb * 16);
    hipStreamSynchronize(c->stream);
    hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost);
    long long t0 = h[0];
    for (int b = 0; b < nb; b++) if (h[(size_t)b * 16] && h[(size_t)b * 16] < t0) t0 = h[(size_t)b * 16];
    for (int b : {0, 1, nb / 2, nb - 1}) {
      fprintf(stderr, "[k3 stamps] wg %d:", b);
      for (int i = 0; i < 16; i++) fprintf(stderr, " %lld", h[(size_t)b * 16 + i] ? h[(size_t)b * 16 + i] - t0 : -1);
      fprintf(stderr, "\n");
    }
    long long tmax = 0;
    for (int b = 0; b < nb; b++) if (h[(size_t)b * 16 + 15] - t0 > tmax) tmax = h[(size_t)b * 16 + 15] - t0;
    fprintf(stderr, "[k3 stamps] last workgroup ends at %lld ticks (100 MHz wall clock: 1 tick = 10 ns); per workgroup: start, prologue, then per tile [A, B, combine, E]\n", tmax);
  }
  *nblocks_out = nb;
  return VBA_OK;
}

// init: the launch may carry the call's pending LM init (k_hessian2 only: the opt-in occupancy-compact pass takes the stand-alone
// init kernel in front of it)
int launch_hessian(vba_ctx *c, const double *pd, const int *gate, int head, int end, int *nb, LmDev *lm = nullptr, const double *k4p = nullptr, int k4nb = 0,
                   const LiJob &li = LiJob{}, size_t li_lds = 0, bool init = false) {
  // whole store, W <= 10: the occupancy-compact pass (vba_kernels_h3.hpp); sub-ranges and wider windows: the dense-tile pass
  if (head == 0 && end == c->nvox && c->opt.win_size <= 10 && c->use_h3) {
    if (init) { const int st = lm_init_flush(c); if (st) return st; }
    switch (c->opt.win_size) {
#define VBA_H3_CASE(WW) case WW: return launch_hessian3_t<WW>(c, pd, gate, nb, lm, k4p, k4nb, li, li_lds);
      VBA_H3_CASE(2) VBA_H3_CASE(3) VBA_H3_CASE(4) VBA_H3_CASE(5) VBA_H3_CASE(6) VBA_H3_CASE(7) VBA_H3_CASE(8) VBA_H3_CASE(9) VBA_H3_CASE(10)
#undef VBA_H3_CASE
    }
  }
  switch (c->opt.win_size) {
#define VBA_H_CASE(WW) case WW: return launch_hessian2_t<WW>(c, pd, gate, head, end, nb, lm, k4p, k4nb, li, li_lds, init);
    VBA_H_CASE(2) VBA_H_CASE(3) VBA_H_CASE(4) VBA_H_CASE(5) VBA_H_CASE(6) VBA_H_CASE(7) VBA_H_CASE(8) VBA_H_CASE(9) VBA_H_CASE(10)
    VBA_H_CASE(11) VBA_H_CASE(12) VBA_H_CASE(13) VBA_H_CASE(14) VBA_H_CASE(15) VBA_H_CASE(16)
#undef VBA_H_CASE
    default: return VBA_ERR_UNSUPPORTED_WINDOW;
  }
}

#ifndef VBA_K4_TV
#define VBA_K4_TV 32        // voxels per workgroup of the residual pass (tools/ builds 16 / 64 for comparison)
#endif
// number of workgroups (= residual partials) of the residual pass over n voxels: small stores (latency-bound) take the
// slot-parallel kernel k_residual_s, large ones (throughput-bound) the voxel-per-lane kernel k_residual_v (vba_kernels_factor.hpp)
// (measured crossover on MI355X, hesai200k_w10 scene tiled: 36.8k voxels 6.4 vs 7.1 us, 55.1k voxels 8.7 vs 7.5 us)
// (the crossover is vba_options::residual_vpl_from, default 45000)
inline bool residual_vpl(const vba_ctx *c, int n) { return n > c->residual_vpl_from; }
inline int residual_nb(const vba_ctx *c, int n) { return residual_vpl(c, n) ? (n + 63) / 64 : (n + VBA_K4_TV - 1) / VBA_K4_TV; }

// diagnostic (VBA_K4_STAMPS=1): in-kernel clock stamps of a separate STAMPS instantiation; the production kernel holds none
void k4_stamps_dump(vba_ctx *c, int nb, long long *d_st) {
  const int n = nb < 2048 ? nb : 2048;
  std::vector<long long> h((size_t)n * 4);
  hipStreamSynchronize(c->stream);
  hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost);
  long long t0 = h[0];
  for (int b = 0; b < n; b++) if (h[b * 4] && h[b * 4] < t0) t0 = h[b * 4];
  double a = 0, e = 0, w = 0, last = 0;
  for (int b = 0; b < n; b++) { a += h[b * 4 + 1] - h[b * 4]; e += h[b * 4 + 2] - h[b * 4 + 1]; w += h[b * 4 + 3] - h[b * 4 + 2]; if (h[b * 4 + 3] - t0 > last) last = h[b * 4 + 3] - t0; }
  fprintf(stderr, "[k4 stamps] %d workgroups: loads+transforms %.0f, frame sum + eigen %.0f, stores+reduce %.0f cycles (mean per workgroup); last one ends at %.0f cycles\n", n, a / n, e / n, w / n, last);
}

// residual pass over voxels [head, end) (end > head); partials (one per workgroup) go to dst or d_partial; returns their number
// (negative: the stand-alone init of a diagnostic run failed, the context holds the error)
int launch_residual(vba_ctx *c, const double *pd, const int *gate, int head, int end, double *dst = nullptr, bool init = false) {
  double *part = dst ? dst : c->d_partial;
  const int nb = residual_nb(c, end - head);
  static const bool want_stamps = diag_env("VBA_K4_STAMPS") != nullptr;
  static long long *d_st = nullptr;
  if (want_stamps) {
    if (!d_st) hipMalloc((void **)&d_st, 2048 * 4 * 8);
    hipMemsetAsync(d_st, 0, 2048 * 4 * 8, c->stream);
  }
  if (want_stamps && init) {                // (the diagnostic STAMPS instances carry no init: it becomes a launch of its own)
    if (lm_init_flush(c)) return -1;
    init = false;
  }
  if (residual_vpl(c, end - head)) {
#define VBA_RESV_CASE(WW) case WW: \
    if (want_stamps) hipLaunchKernelGGL((k_residual_v<WW, true>), dim3(nb), dim3(64), 0, c->stream, c->fv, pd, head, end, part, gate, d_st, lm_init_arg<WW>(c, false)); \
    else if (init && c->lm_init.pending) hipLaunchKernelGGL((k_residual_v<WW, false, true>), dim3(nb), dim3(64), 0, c->stream, c->fv, pd, head, end, part, gate, (long long *)nullptr, lm_init_arg<WW>(c, true)); \
    else hipLaunchKernelGGL((k_residual_v<WW, false>), dim3(nb), dim3(64), 0, c->stream, c->fv, pd, head, end, part, gate, (long long *)nullptr, lm_init_arg<WW>(c, false)); break;
    switch (c->opt.win_size) {
      VBA_RESV_CASE(2) VBA_RESV_CASE(3) VBA_RESV_CASE(4) VBA_RESV_CASE(5) VBA_RESV_CASE(6) VBA_RESV_CASE(7) VBA_RESV_CASE(8) VBA_RESV_CASE(9) VBA_RESV_CASE(10)
      VBA_RESV_CASE(11) VBA_RESV_CASE(12) VBA_RESV_CASE(13) VBA_RESV_CASE(14) VBA_RESV_CASE(15) VBA_RESV_CASE(16)
    }
#undef VBA_RESV_CASE
  } else {
#define VBA_RES_CASE(WW) case WW: { using RC = ResCfg<WW, VBA_K4_TV>; \
    if (want_stamps) hipLaunchKernelGGL((k_residual_s<WW, VBA_K4_TV, true>), dim3(nb), dim3(RC::NT), 0, c->stream, c->fv, pd, head, end, part, gate, d_st, lm_init_arg<WW>(c, init)); \
    else hipLaunchKernelGGL((k_residual_s<WW, VBA_K4_TV, false>), dim3(nb), dim3(RC::NT), 0, c->stream, c->fv, pd, head, end, part, gate, (long long *)nullptr, lm_init_arg<WW>(c, init)); break; }
    switch (c->opt.win_size) {
      VBA_RES_CASE(2) VBA_RES_CASE(3) VBA_RES_CASE(4) VBA_RES_CASE(5) VBA_RES_CASE(6) VBA_RES_CASE(7) VBA_RES_CASE(8) VBA_RES_CASE(9) VBA_RES_CASE(10)
      VBA_RES_CASE(11) VBA_RES_CASE(12) VBA_RES_CASE(13) VBA_RES_CASE(14) VBA_RES_CASE(15) VBA_RES_CASE(16)
    }
#undef VBA_RES_CASE
  }
  if (want_stamps) k4_stamps_dump(c, nb, d_st);
  return nb;
}

// SUM all-reduce of n doubles in HBM across the ranks, ordered on the context's stream: RCCL when the context holds a
// communicator (vba_rccl_init / vba_set_rccl_comm), else the host program's hook (gloo rehearsals on the CPU side of tests).
int ctx_allreduce(vba_ctx *c, double *buf, size_t n) {
  if (c->comm) {
    const RcclApi &R = rccl_api();
    const ncclResult_t r = R.AllReduce(buf, buf, n, ncclDouble, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) { c->set_error(std::string("ncclAllReduce: ") + R.GetErrorString(r)); return VBA_ERR_HIP; }
    return VBA_OK;
  }
  if (!c->allreduce) { c->set_error("no collective configured"); return VBA_ERR_BAD_ARG; }
  if (c->allreduce(c->allreduce_user, buf, n, c->stream)) { c->set_error("allreduce hook failed"); return VBA_ERR_HIP; }
  return VBA_OK;
}
// All-gather in place: buf holds n_ranks chunks of `chunk` doubles, rank r has filled chunk r.  RCCL moves every chunk once;
// the hook (SUM only) emulates it by zeroing the foreign chunks first.
int ctx_allgather(vba_ctx *c, double *buf, size_t chunk) {
  if (chunk == 0) return VBA_OK;
  if (c->comm) {
    const RcclApi &R = rccl_api();
    const ncclResult_t r = R.AllGather(buf + (size_t)c->rank * chunk, buf, chunk, ncclDouble, c->comm, c->stream);
    if (r != ncclSuccess) { c->set_error(std::string("ncclAllGather: ") + R.GetErrorString(r)); return VBA_ERR_HIP; }
    return VBA_OK;
  }
  for (int r = 0; r < c->n_ranks; r++)
    if (r != c->rank) HIPCHK(c, hipMemsetAsync(buf + (size_t)r * chunk, 0, chunk * sizeof(double), c->stream));
  return ctx_allreduce(c, buf, chunk * (size_t)c->n_ranks);
}

// device passes on device-resident poses (gate == nullptr: unconditional)
int hessian_pass(vba_ctx *c, const double *poses_dev, const int *gate, int head, int end, LmDev *lm = nullptr, const double *k4p = nullptr, int k4nb = 0,
                 const LiJob &li = LiJob{}, size_t li_lds = 0, bool init = false) {
  const int W = c->opt.win_size, nout = nout_tl(W);
  if (end <= head) {
    if (init) { const int st = lm_init_flush(c); if (st) return st; }     // (no kernel to carry it)
    HIPCHK(c, hipMemsetAsync(c->d_out, 0, (size_t)nout * sizeof(double), c->stream));
  } else {
    int nb = 0;
    TimedSpan s1{}, s2{};
    span_begin(c, "hessian", s1);
    int st = launch_hessian(c, poses_dev, gate, head, end, &nb, lm, k4p, k4nb, li, li_lds, init);
    if (st) return st;
    span_end(c, "hessian", s1);
    span_begin(c, "reduce", s2);
    hipLaunchKernelGGL(k_reduce_partials, dim3((nout + 15) / 16), dim3(256), 0, c->stream, c->d_partial, nb, nout, c->d_out, gate);
    span_end(c, "reduce", s2);
    HIPCHK(c, hipGetLastError());
  }
  if (c->collective()) {
    int rc = ctx_allreduce(c, c->d_out, (size_t)nout);
    if (rc) return rc;
  }
  return VBA_OK;
}

int residual_pass(vba_ctx *c, const double *poses_dev, const int *gate, int head, int end, double *d_scalar_out) {
  if (end <= head) {
    HIPCHK(c, hipMemsetAsync(d_scalar_out, 0, sizeof(double), c->stream));
  } else {
    const int nb = residual_nb(c, end - head);
    if ((size_t)nb > c->partial_doubles) { c->set_error("partial buffer too small"); return VBA_ERR_CAPACITY; }
    TimedSpan s1{}, s2{};
    span_begin(c, "residual", s1);
    launch_residual(c, poses_dev, gate, head, end);
    span_end(c, "residual", s1);
    span_begin(c, "reduce", s2);
    hipLaunchKernelGGL(k_sum_scalar, dim3(1), dim3(256), 0, c->stream, c->d_partial, nb, d_scalar_out, gate);
    span_end(c, "reduce", s2);
    HIPCHK(c, hipGetLastError());
  }
  if (c->collective()) {
    int rc = ctx_allreduce(c, d_scalar_out, 1);
    if (rc) return rc;
  }
  return VBA_OK;
}

// tile layout -> full layout [H | g | r] in d_full (host consumers only; the device LM reads the tile layout directly)
int tiles_to_full(vba_ctx *c, const double *src) {
#define VBA_TF_CASE(WW) case WW: hipLaunchKernelGGL(k_tiles_to_full<WW>, dim3(16), dim3(256), 0, c->stream, src, c->d_full); break;
  switch (c->opt.win_size) {
    VBA_TF_CASE(2) VBA_TF_CASE(3) VBA_TF_CASE(4) VBA_TF_CASE(5) VBA_TF_CASE(6) VBA_TF_CASE(7) VBA_TF_CASE(8) VBA_TF_CASE(9) VBA_TF_CASE(10)
    VBA_TF_CASE(11) VBA_TF_CASE(12) VBA_TF_CASE(13) VBA_TF_CASE(14) VBA_TF_CASE(15) VBA_TF_CASE(16)
    default: return VBA_ERR_UNSUPPORTED_WINDOW;
  }
#undef VBA_TF_CASE
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}

// device: d_full = [H | g | r] over voxels [head,end) for host poses (+ all-reduce across ranks when configured)
int eval_hessian_dev(vba_ctx *c, const double *poses, int head, int end) {
  int st = upload_poses(c, poses);
  if (st) return st;
  st = hessian_pass(c, c->d_poses, nullptr, head, end);
  if (st) return st;
  return tiles_to_full(c, c->d_out);
}

int eval_residual_dev(vba_ctx *c, const double *poses, int head, int end, double *d_scalar_out) {
  int st = upload_poses(c, poses);
  if (st) return st;
  return residual_pass(c, c->d_poses, nullptr, head, end, d_scalar_out);
}

int ensure_partial(vba_ctx *c, size_t doubles) {
  if (doubles <= c->partial_doubles) return VBA_OK;
  if (c->d_partial) hipFree(c->d_partial);
  c->d_partial = nullptr; c->partial_doubles = 0;
  HIPCHK(c, hipMalloc((void **)&c->d_partial, doubles * sizeof(double)));
  c->partial_doubles = doubles;
  return VBA_OK;
}

// host copies of the reduced device results
int fetch(vba_ctx *c, const double *d_src, size_t n, double *dst) {
  int st = ensure_pin(c, n + 65536);
  if (st) return st;
  double *stage = c->h_pin + 32768;  // poses live in the first part
  HIPCHK(c, hipStreamSynchronize(c->stream));   // drain first: a D2H copy queued behind in-flight kernels completes much later (measured)
  HIPCHK(c, hipMemcpyAsync(stage, d_src, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(dst, stage, n * sizeof(double));
  return VBA_OK;
}

// states <-> poses
void states_to_poses(const double *states, int W, double *poses) {
  for (int i = 0; i < W; i++) { std::memcpy(poses + 12 * i, states + 25 * i + 1, 9 * sizeof(double)); std::memcpy(poses + 12 * i + 9, states + 25 * i + 10, 3 * sizeof(double)); }
}

}  // namespace

extern "C" {

void vba_default_options(vba_options *o) {
  std::memset(o, 0, sizeof(*o));
  o->win_size = 10; o->voxel_size = 1.0; o->max_layer = 2; o->max_points = 100; o->min_eigen_value = 0.0025;
  for (int i = 0; i < 4; i++) { o->plane_eigen_value_thre[i] = 0.25; o->min_point[i] = 5; }
  o->imu_coef = 1e-4; o->thread_num = 5; o->device = -1; o->stream = nullptr;
}

const char *vba_status_string(int s) {
  switch (s) {
    case VBA_OK: return "ok";
    case VBA_ERR_NO_DEVICE: return "no HIP device (libvoxelba has no CPU path)";
    case VBA_ERR_BAD_ARG: return "bad argument";
    case VBA_ERR_UNSUPPORTED_WINDOW: return "unsupported window size";
    case VBA_ERR_TOO_FEW_VOXELS: return "too few voxels (reference: 'Too Less Voxel' exit)";
    case VBA_ERR_OPT_STATE: return "opt_state out of range (reference: exit)";
    case VBA_ERR_HIP: return "HIP runtime error";
    case VBA_ERR_CAPACITY: return "capacity exceeded";
    case VBA_ERR_IO: return "file missing or malformed";
    case VBA_ERR_UNSUPPORTED: return "not available in this process (RCCL could not be resolved)";
    case VBA_ERR_SINGULAR: return "singular system (a component without a prior, or a non-positive pivot)";
    default: return "unknown";
  }
}

int vba_create(const vba_options *opt, vba_ctx **out) {
  if (!opt || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  if (opt->win_size < 2 || opt->win_size > VBA_MAX_WIN) return VBA_ERR_UNSUPPORTED_WINDOW;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VBA_ERR_NO_DEVICE;
  vba_ctx *c = new vba_ctx();
  c->opt = *opt;
  if (opt->device >= 0) {
    if (hipSetDevice(opt->device) != hipSuccess) { delete c; return VBA_ERR_NO_DEVICE; }
    c->device = opt->device;
  } else {
    hipGetDevice(&c->device);
  }
  c->lm_spec = opt->lm_spec > 0 ? std::min(opt->lm_spec, (int)LM_SPEC) : (int)LM_SPEC;
  c->force_collective = opt->force_collective != 0;
  c->max_blocks_hess = opt->hessian_workgroups > 0 ? std::min(opt->hessian_workgroups, kMaxBlocksHess) : kMaxBlocksHess;
  if (c->max_blocks_hess < 2) c->max_blocks_hess = 2;      // (LI-BA gives one workgroup's CU to the IMU factors)
  c->residual_vpl_from = opt->residual_vpl_from > 0 ? opt->residual_vpl_from : 45000;
  c->use_h3 = opt->hessian_compact_tiles != 0 && opt->deterministic == 0;   // (k_hessian3 adds into LDS with f64 atomics)
  if (opt->stream) { c->stream = (hipStream_t)opt->stream; c->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return VBA_ERR_HIP; }
    c->own_stream = true;
  }
  const int W = opt->win_size, nout = nout_of(W);
  c->fv.W = W;
  if (hipMalloc((void **)&c->d_poses, (size_t)VBA_MAX_WIN * 12 * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&c->d_out, ((size_t)nout_tl(W) + 64) * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&c->d_full, ((size_t)nout + 64) * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&c->d_scal, 64 * sizeof(double)) != hipSuccess) { vba_destroy(c); return VBA_ERR_HIP; }
  if (ensure_partial(c, (size_t)kMaxBlocksHess * (nout_tl(W) > nout ? nout_tl(W) : nout)) != VBA_OK || ensure_pin(c, 65536 + (size_t)nout + 1024) != VBA_OK) { vba_destroy(c); return VBA_ERR_HIP; }
  if (hipMalloc((void **)&c->d_lm, sizeof(LmDev)) != hipSuccess || hipMalloc((void **)&c->d_raw, ((size_t)nout_tl(W) + 64) * 8) != hipSuccess ||
      hipHostMalloc((void **)&c->h_lm, sizeof(LmDev), hipHostMallocDefault) != hipSuccess) { vba_destroy(c); return VBA_ERR_HIP; }
  if (opt->max_voxels && factor_reserve(c, (int)opt->max_voxels) != VBA_OK) { vba_destroy(c); return VBA_ERR_HIP; }
  map_init(c->map, c->opt);
  *out = c;
  return VBA_OK;
}

void vba_destroy(vba_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->comm && c->own_comm) rccl_api().CommDestroy(c->comm);      // (a communicator exists only if the API resolved)
  map_free(c->map);
  c->gba.free_all();
  c->big.release();
  for (vba_ctx *w : c->hba_workers) vba_destroy(w);
  c->hba_workers.clear();
  if (c->d_hba_all) hipFree(c->d_hba_all);
  if (c->d_init) hipFree(c->d_init);
  if (c->d_btcq) hipFree(c->d_btcq);
  if (c->h_btcq) hipHostFree(c->h_btcq);
  if (c->d_btccnt) hipFree(c->d_btccnt);
  if (c->d_icp) hipFree(c->d_icp);
  if (c->h_icp) hipHostFree(c->h_icp);
  if (c->d_icpkey) hipFree(c->d_icpkey);
  if (c->d_icppart) hipFree(c->d_icppart);
  if (c->d_pgo) hipFree(c->d_pgo);
  if (c->d_pgoAb) hipFree(c->d_pgoAb);
  for (int i = 0; i < vba_ctx::kExpRing; i++) { if (c->h_exp[i]) hipHostFree(c->h_exp[i]); if (c->exp_ev[i]) hipEventDestroy(c->exp_ev[i]); }
  if (c->d_exp) hipFree(c->d_exp);
  if (c->d_expout) hipFree(c->d_expout);
  if (c->d_lipack) hipFree(c->d_lipack);
  if (c->d_liscr) hipFree(c->d_liscr);
  for (int i = 0; i < 2; i++) if (c->d_kdtree[i]) hipFree(c->d_kdtree[i]);
  if (c->d_refpts) hipFree(c->d_refpts);
  if (c->d_li) hipFree(c->d_li);
  if (c->d_k4part) hipFree(c->d_k4part);
  if (c->d_imu) hipFree(c->d_imu);
  if (c->d_himu) hipFree(c->d_himu);
  if (c->d_gimu) hipFree(c->d_gimu);
  double *p[] = {c->fv.cl, c->fv.fix, c->fv.coe, c->fv.eigval, c->fv.eigvec, c->fv.pcr, c->d_poses, c->d_partial, c->d_out, c->d_full, c->d_scal};
  for (double *q : p) if (q) hipFree(q);
  if (c->fv.occ) hipFree(c->fv.occ);
  if (c->fv.tiles) hipFree(c->fv.tiles);
  if (c->d_stage) hipFree(c->d_stage);
  if (c->h_pin) hipHostFree(c->h_pin);
  if (c->d_lm) hipFree(c->d_lm);
  if (c->d_raw) hipFree(c->d_raw);
  if (c->h_lm) hipHostFree(c->h_lm);
  for (auto &kv : c->spans) for (auto &s : kv.second) { hipEventDestroy(s.a); hipEventDestroy(s.b); }
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete c;
}

const char *vba_last_error(vba_ctx *c) { return c ? c->err.c_str() : ""; }
int vba_synchronize(vba_ctx *c) { HIPCHK(c, hipStreamSynchronize(c->stream)); return VBA_OK; }

// ---------------------------------------------------------------- factor level
int vba_factor_clear(vba_ctx *c) { c->nvox = 0; return VBA_OK; }
int vba_factor_size(vba_ctx *c) { return c->nvox; }

int vba_factor_push_voxels(vba_ctx *c, int n, const double *clusters, const double *fix, const double *coe, const double *eig_val,
                           const double *eig_vec, const double *pcr_add) {
  if (n < 0) return VBA_ERR_BAD_ARG;
  if (n == 0) return VBA_OK;
  const int W = c->opt.win_size;
  int st = factor_reserve(c, c->nvox + n);
  if (st) return st;
  const size_t per = (size_t)10 * W + 33;
  st = ensure_stage(c, per * n * sizeof(double));
  if (st) return st;
  double *d = (double *)c->d_stage;
  double *d_cl = d, *d_fix = d_cl + (size_t)n * W * 10, *d_coe = d_fix + (size_t)n * 10, *d_ev = d_coe + n, *d_evec = d_ev + (size_t)n * 3,
         *d_pcr = d_evec + (size_t)n * 9;
  HIPCHK(c, hipMemcpyAsync(d_cl, clusters, (size_t)n * W * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_fix, fix, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_coe, coe, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ev, eig_val, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_evec, eig_vec, (size_t)n * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_pcr, pcr_add, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const long long tot = (long long)n * per;
  int nb = (int)((tot + 255) / 256);
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_aos_to_soa, dim3(nb), dim3(256), 0, c->stream, c->fv, c->nvox, n, d_cl, d_fix, d_coe, d_ev, d_evec, d_pcr);
  factor_update_mask(c, c->nvox, n);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));  // caller's arrays may go away
  c->nvox += n;
  return VBA_OK;
}

int vba_factor_acc_evaluate2(vba_ctx *c, const double *poses, int head, int end, double *Hess, double *JacT, double *residual) {
  if (head < 0 || end > c->nvox || head > end) return VBA_ERR_BAD_ARG;
  const int W = c->opt.win_size, n = 6 * W, nout = nout_of(W);
  int st = eval_hessian_dev(c, poses, head, end);
  if (st) return st;
  std::vector<double> buf(nout);
  st = fetch(c, c->d_full, nout, buf.data());
  if (st) return st;
  if (Hess) std::memcpy(Hess, buf.data(), (size_t)n * n * sizeof(double));
  if (JacT) std::memcpy(JacT, buf.data() + (size_t)n * n, (size_t)n * sizeof(double));
  if (residual) *residual = buf[(size_t)n * n + n];
  return VBA_OK;
}

int vba_factor_evaluate_only_residual(vba_ctx *c, const double *poses, int head, int end, double *residual) {
  if (head < 0 || end > c->nvox || head > end) return VBA_ERR_BAD_ARG;
  double *d_r = c->d_scal;
  int st = eval_residual_dev(c, poses, head, end, d_r);
  if (st) return st;
  double r = 0;
  st = fetch(c, d_r, 1, &r);
  if (st) return st;
  if (residual) *residual = r;
  return VBA_OK;
}

int vba_factor_read_back(vba_ctx *c, double *eig_val, double *eig_vec, double *pcr_add) {
  const int n = c->nvox;
  if (n == 0) return VBA_OK;
  int st = ensure_stage(c, (size_t)n * 22 * sizeof(double));
  if (st) return st;
  double *d = (double *)c->d_stage;
  double *d_ev = d, *d_evec = d + (size_t)n * 3, *d_pcr = d_evec + (size_t)n * 9;
  int nb = (int)(((long long)n * 22 + 255) / 256);
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_soa_to_aos_out, dim3(nb), dim3(256), 0, c->stream, c->fv, n, d_ev, d_evec, d_pcr);
  HIPCHK(c, hipGetLastError());
  if (eig_val) HIPCHK(c, hipMemcpyAsync(eig_val, d_ev, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (eig_vec) HIPCHK(c, hipMemcpyAsync(eig_vec, d_evec, (size_t)n * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (pcr_add) HIPCHK(c, hipMemcpyAsync(pcr_add, d_pcr, (size_t)n * 10 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_factor_occupancy_masks(vba_ctx *c, unsigned int *masks) {
  if (!masks && c->nvox > 0) return VBA_ERR_BAD_ARG;
  if (c->nvox == 0) return VBA_OK;
  HIPCHK(c, hipMemcpyAsync(masks, c->fv.occ, (size_t)c->nvox * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}
int vba_factor_occupied_slots(vba_ctx *c, long long *slots) {
  if (!slots) return VBA_ERR_BAD_ARG;
  *slots = 0;
  if (c->nvox == 0) return VBA_OK;
  int st = ensure_stage(c, 64);
  if (st) return st;
  HIPCHK(c, hipMemsetAsync(c->d_stage, 0, 8, c->stream));
  hipLaunchKernelGGL(k_count_slots, dim3(512), dim3(256), 0, c->stream, c->fv, c->nvox, (unsigned long long *)c->d_stage);
  unsigned long long h = 0;
  HIPCHK(c, hipMemcpyAsync(&h, c->d_stage, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *slots = (long long)h;
  return VBA_OK;
}

// ---------------------------------------------------------------- Lidar_BA_Optimizer (VM:342-498), device-resident loop
int vba_lm_begin(vba_ctx *c, const double *poses, int thd_num) {
  const int W = c->opt.win_size;
  // No copy, no host wait: the LmDev image (lm_init_store: x = xt = poses (VM:435), u = 0.01, v = 2 (VM:427), the flags) is written by the
  // first LM kernel of the call from a by-value argument; a second vba_lm_begin simply replaces a pending init.
  std::memcpy(c->lm_init.x, poses, (size_t)W * 12 * sizeof(double));
  { const char *e = diag_env("VBA_DEBUG_SOLVE"); c->lm_init.dbg = e ? atoi(e) : 0; }   // ablation / stamp mask of -DVBA_DIAG builds (0 otherwise)
  c->lm_init.pending = true;
  c->lm.active = true; c->lm.thd_num = thd_num; c->lm.have_hess = false; c->lm.pending_update = false;
  c->trace.clear();
  // "Too Less Voxel" (VM:399-403) is a statement about the whole window: a sharded rank decides it from the voxel count summed over
  // the ranks, so every rank takes the same branch and none is left waiting in the next collective
  c->nvox_global = c->nvox;
  if (c->collective()) {
    int st = ensure_pin(c, 65536);
    if (st) return st;
    c->h_pin[60000] = (double)c->nvox;
    HIPCHK(c, hipMemcpyAsync(c->d_scal + 8, c->h_pin + 60000, sizeof(double), hipMemcpyHostToDevice, c->stream));
    st = ctx_allreduce(c, c->d_scal + 8, 1);
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_pin + 60000, c->d_scal + 8, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->nvox_global = (int)(c->h_pin[60000] + 0.5);
  }
  return VBA_OK;
}

// Re-creates the per-voxel eigen state (eig_values / eig_vectors / pcr_adds) at the poses loaded by vba_lm_begin: one
// residual pass on the device, nothing is fetched.  In the reference this state comes from recut/tras_opt right before
// damping_iter (VM:1628); a caller that restarts the optimiser on an unchanged factor store uses this instead.
int vba_lm_refresh_eigen(vba_ctx *c) {
  if (!c->lm.active) return VBA_ERR_BAD_ARG;
  const double *x_dev = reinterpret_cast<const double *>(reinterpret_cast<char *>(c->d_lm) + offsetof(LmDev, x));
  if (c->nvox <= 0) return VBA_OK;
  // only the pass' side effect is wanted (eig_values / eig_vectors / pcr_adds at the begin poses): its partials are not summed
  if ((size_t)residual_nb(c, c->nvox) > c->partial_doubles) { c->set_error("partial buffer too small"); return VBA_ERR_CAPACITY; }
  TimedSpan s1{};
  span_begin(c, "residual", s1);
  // single-rank: the pass carries the call's init when it is the first LM kernel; the multi-rank flow takes the stand-alone init
  const bool fuse_init = !c->collective();
  if (!fuse_init) { const int st = lm_init_flush(c); if (st) return st; }
  if (launch_residual(c, x_dev, nullptr, 0, c->nvox, nullptr, fuse_init) < 0) return VBA_ERR_HIP;
  span_end(c, "residual", s1);
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}

int vba_timing_launch_hessian(vba_ctx *c) {
  if (!c->lm.active || c->nvox <= 0) return VBA_ERR_BAD_ARG;
  const double *x_dev = reinterpret_cast<const double *>(reinterpret_cast<char *>(c->d_lm) + offsetof(LmDev, x));
  int nb = 0;
  int st = lm_init_flush(c);
  if (st) return st;
  st = launch_hessian(c, x_dev, nullptr, 0, c->nvox, &nb);
  if (st) return st;
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}

// One trip through the loop body VM:441-494, enqueued without host synchronisation unless the caller asks for the flags.
int vba_lm_iterate(vba_ctx *c, int *accepted, int *stop) {
  if (!c->lm.active) return VBA_ERR_BAD_ARG;
  const int W = c->opt.win_size, nout = nout_of(W), V = c->nvox;
  if (c->nvox_global < c->lm.thd_num) { c->lm_init.pending = false; return VBA_ERR_TOO_FEW_VOXELS; }   // VM:399-403 (and g_size checks of VM:367); the same on every rank
  char *base = reinterpret_cast<char *>(c->d_lm);
  const double *x_dev = reinterpret_cast<const double *>(base + offsetof(LmDev, x));
  const double *xt_dev = reinterpret_cast<const double *>(base + offsetof(LmDev, xt));
  const int *run_hess = reinterpret_cast<const int *>(base + offsetof(LmDev, run_hess));
  const int *run_res = reinterpret_cast<const int *>(base + offsetof(LmDev, run_res));
  // Multi-rank: ONE collective per iteration.  After the residual pass at the trial poses the Hessian pass is run there
  // too (speculating that the step is accepted) and [H | g | r] is all-reduced once: its r (the sum of the eigenvalues the
  // residual pass just stored) is the trial residual the accept test needs, and on acceptance H is already the next
  // iteration's Hessian; on a reject the solve keeps using its saved copy (`raw`), exactly as VM:443 skips divide_thread.
  const int copy_raw = c->collective() ? 1 : 0;
  int st = VBA_OK;
  static const bool no_fuse = diag_env("VBA_NO_FUSED_UPDATE") != nullptr;   // diagnostic: accept/reject always as its own kernel
  if (copy_raw) { st = lm_init_flush(c); if (st) return st; }               // the multi-rank flow takes the stand-alone init
  if (!(copy_raw && c->lm.have_hess)) {
    if (c->lm.pending_update) {               // the previous iteration's accept/reject rides in this pass (runs on xt after an accepted step)
      st = hessian_pass(c, x_dev, run_hess, 0, V, c->d_lm, c->d_k4part, c->lm.k4_nb);
      c->lm.pending_update = false;
    } else {
      st = hessian_pass(c, x_dev, run_hess, 0, V, nullptr, nullptr, 0, LiJob{}, 0, true);   // divide_thread  VM:445 (skipped on device after a reject); the first pass of a call carries its init
    }
  }
  if (st) return st;
  TimedSpan sp{};
  span_begin(c, "solve", sp);
  switch (W) {
#define VBA_SM_CASE(WW) case WW: \
    if (copy_raw) hipLaunchKernelGGL((k_lm_solve_m<WW, true>), dim3(c->lm_spec), dim3(256), 0, c->stream, c->d_lm, c->d_out, c->d_raw, nullptr); \
    else hipLaunchKernelGGL((k_lm_solve_m<WW, false>), dim3(c->lm_spec), dim3(256), 0, c->stream, c->d_lm, c->d_out, c->d_raw, nullptr); \
    break;
    VBA_SM_CASE(2) VBA_SM_CASE(3) VBA_SM_CASE(4) VBA_SM_CASE(5) VBA_SM_CASE(6) VBA_SM_CASE(7) VBA_SM_CASE(8) VBA_SM_CASE(9) VBA_SM_CASE(10)
    VBA_SM_CASE(11) VBA_SM_CASE(12) VBA_SM_CASE(13) VBA_SM_CASE(14) VBA_SM_CASE(15) VBA_SM_CASE(16)
#undef VBA_SM_CASE
    default: return VBA_ERR_UNSUPPORTED_WINDOW;
  }
  span_end(c, "solve", sp);
  double *d_r = c->d_scal;
  if (copy_raw) {
    if (V > 0) launch_residual(c, xt_dev, run_res, 0, V);   // only_residual VM:467: refreshes the eigen state at the trial poses
    st = hessian_pass(c, xt_dev, run_res, 0, V);                      // speculative divide_thread there + the one all-reduce
    if (st) return st;
    c->lm.have_hess = true;
    hipLaunchKernelGGL(k_lm_update, dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_out + (nout_tl(W) - 1), 0, W);
  } else {
    const int nb = residual_nb(c, V);
    if (nb > c->k4part_cap) {
      if (c->d_k4part) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipFree(c->d_k4part); c->d_k4part = nullptr; }
      const int cap = nb > 65536 ? 2 * nb : 65536;
      HIPCHK(c, hipMalloc((void **)&c->d_k4part, (size_t)cap * sizeof(double)));
      c->k4part_cap = cap;
    }
    const bool fuse = !no_fuse && !(accepted || stop);
    TimedSpan s1{};
    span_begin(c, "residual", s1);
    launch_residual(c, xt_dev, run_res, 0, V, c->d_k4part);
    span_end(c, "residual", s1);
    if (fuse) { c->lm.pending_update = true; c->lm.k4_nb = nb; }
    else hipLaunchKernelGGL(k_lm_update, dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_k4part, nb, W);   // sums the partials itself
  }
  HIPCHK(c, hipGetLastError());
  if (accepted || stop) {
    HIPCHK(c, hipMemcpyAsync(c->h_lm, c->d_lm, sizeof(LmDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (accepted) *accepted = c->h_lm->last_accepted;
    if (stop) *stop = c->h_lm->stop;
  }
  return VBA_OK;
}

int vba_lm_end(vba_ctx *c, double *poses, double *hess, double *resis2) {
  if (!c->lm.active) return VBA_ERR_BAD_ARG;
  const int W = c->opt.win_size, n = 6 * W;
  const bool want = poses || hess || resis2;
  if (!want && !c->lm.pending_update) { c->lm_init.pending = false; c->lm.active = false; return VBA_OK; }   // (an init nothing consumed is dropped with the call)
  int st = lm_init_flush(c);                  // vba_lm_end right after vba_lm_begin
  if (st) return st;
  if (!want) {                                // nothing requested: no synchronisation; the last iteration's accept/reject has no Hessian pass to ride in
    hipLaunchKernelGGL(k_lm_update, dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_k4part, c->lm.k4_nb, W);
    c->lm.pending_update = false;
    c->lm.active = false;
    return VBA_OK;
  }
  // One host round trip and ONE launch (k_lm_finish): the pending accept/reject, then the LM state and *hess reach the pinned mirrors
  // through stores via the host mapping — a D2H copy queued behind in-flight kernels completes much later (see li_ba_device), and
  // draining the stream first is a second trip.
  double *h_hess = nullptr;
  if (hess) {
    st = ensure_pin(c, 65536 + (size_t)n * n + 1024);
    if (st) return st;
    h_hess = c->h_pin + 32768;
  }
  const double *src = c->collective() ? c->d_raw : c->d_out;      // *hess = Hess before gauge fixing (VM:446)
  const int upd = c->lm.pending_update ? 1 : 0;
  switch (W) {
#define VBA_FIN_CASE(WW) case WW: hipLaunchKernelGGL(k_lm_finish<WW>, dim3(hess ? 17 : 1), dim3(256), 0, c->stream, c->d_lm, c->d_k4part, upd ? c->lm.k4_nb : 0, upd, c->h_lm, src, h_hess); break;
    VBA_FIN_CASE(2) VBA_FIN_CASE(3) VBA_FIN_CASE(4) VBA_FIN_CASE(5) VBA_FIN_CASE(6) VBA_FIN_CASE(7) VBA_FIN_CASE(8) VBA_FIN_CASE(9) VBA_FIN_CASE(10)
    VBA_FIN_CASE(11) VBA_FIN_CASE(12) VBA_FIN_CASE(13) VBA_FIN_CASE(14) VBA_FIN_CASE(15) VBA_FIN_CASE(16)
#undef VBA_FIN_CASE
    default: return VBA_ERR_UNSUPPORTED_WINDOW;
  }
  c->lm.pending_update = false;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const LmDev *h = c->h_lm;
  if (poses) std::memcpy(poses, h->x, (size_t)W * 12 * sizeof(double));
  if (hess) std::memcpy(hess, c->h_pin + 32768, (size_t)n * n * sizeof(double));
  if (resis2) { resis2[0] = h->resis_first; resis2[1] = h->r2; }
  c->trace.assign(h->trace, h->trace + 5 * h->n_trace);
  if (h->pad & 16) {
    fprintf(stderr, "[k_lm_solve_m cycles] prologue %lld | tile load %lld | factorisation %lld | backsub %lld | epilogue %lld | panels:", h->stamps[1] - h->stamps[0],
            h->stamps[2] - h->stamps[1], h->stamps[3] - h->stamps[2], h->stamps[4] - h->stamps[3], h->stamps[5] - h->stamps[4]);
    const int npr = (int)h->stamps[6];             // panels run: the factorisation ends with the panel of the last live pivot
    for (int kb = 0; kb < npr && kb < 8; kb++) fprintf(stderr, " %lld+%lld", h->stamps[9 + 2 * kb] - h->stamps[8 + 2 * kb], kb < npr - 1 ? h->stamps[10 + 2 * kb] - h->stamps[9 + 2 * kb] : 0LL);
    fprintf(stderr, " | %d panels run\n", npr);
  }
  c->lm.active = false;
  return VBA_OK;
}

int vba_lidar_ba_damping_iter(vba_ctx *c, double *poses, double *hess, double *resis2, int max_iter, int thd_num, int *is_converge) {
  int st = vba_lm_begin(c, poses, thd_num);
  if (st) return st;
  for (int i = 0; i < max_iter; i++) {           // the 1e-6 break (VM:492) is a device flag: later launches return at once
    st = vba_lm_iterate(c, nullptr, nullptr);
    if (st) { c->lm.active = false; return st; }
  }
  st = vba_lm_end(c, poses, hess, resis2);
  if (is_converge) *is_converge = c->h_lm->all_accepted;
  return st;
}

int vba_last_lm_trace(vba_ctx *c, double *rows, int max_rows) {
  int n = (int)(c->trace.size() / 5);
  if (n > max_rows) n = max_rows;
  if (rows) std::memcpy(rows, c->trace.data(), (size_t)n * 5 * sizeof(double));
  return n;
}

// ---------------------------------------------------------------- LI_BA_Optimizer / LI_BA_OptimizerGravity on the device
extern "C++" {
template <int W>
struct LiSolveCfg {
  static constexpr int NMAX = 15 * W + 3, NP = ((NMAX + 1 + 15) / 16) * 16;
  static constexpr bool GL = W > 10;             // L of the 15 W + 3 system exceeds the LDS: it lives in c->d_liscr
  static constexpr size_t l_doubles = (size_t)LdltCfg<NP>::LTOT > (size_t)NMAX * (NMAX + 1) / 2 ? (size_t)LdltCfg<NP>::LTOT : (size_t)NMAX * (NMAX + 1) / 2;
  static constexpr size_t lds = ((GL ? (size_t)LdltCfg<NP>::DOUBLES - LdltCfg<NP>::LTOT : (size_t)LdltCfg<NP>::DOUBLES) + 4 * NMAX + NP + 32) * 8 + (size_t)NMAX * 4 + 64;
  static_assert(GL || l_doubles == (size_t)LdltCfg<NP>::LTOT, "the staged triangle must fit the region of L");
};
template <int W, int NT = (W > 10 ? 1024 : 512)>
static int launch_li_solve(vba_ctx *c, int copy_raw, int n, int gauge, int grav) {
  constexpr bool GL = LiSolveCfg<W>::GL;
  constexpr size_t l_doubles = LiSolveCfg<W>::l_doubles, lds = LiSolveCfg<W>::lds;
  static bool attr_set[kMaxDevices] = {false};
  if (!attr_set[c->device % kMaxDevices]) { hipFuncSetAttribute((const void *)k_li_solve<W, NT, GL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr_set[c->device % kMaxDevices] = true; }
  if (GL && c->liscr_doubles < l_doubles * LM_SPEC) {           // one region per damping candidate; W is fixed per context, so this runs once
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_liscr) hipFree(c->d_liscr);
    c->d_liscr = nullptr; c->liscr_doubles = 0;
    HIPCHK(c, hipMalloc((void **)&c->d_liscr, l_doubles * LM_SPEC * sizeof(double)));
    c->liscr_doubles = l_doubles * LM_SPEC;
  }
  hipLaunchKernelGGL((k_li_solve<W, NT, GL>), dim3(c->lm_spec), dim3(NT), lds, c->stream, c->d_lm, c->d_li, c->d_out, c->d_raw, copy_raw, c->d_himu, c->d_gimu, c->d_imu, n, gauge, grav,
                     c->opt.imu_coef, c->d_liscr, nullptr);
  return VBA_OK;
}
}  // extern "C++"

static bool li_device_supported(int W) { return W >= 2 && W <= LI_MAX_W; }

static int li_ba_device(vba_ctx *c, double *states, double *imus, int gravity, int max_iter, double *hess, double *resis2) {
  static const bool want_times = diag_env("VBA_LI_TIMES") != nullptr;   // diagnostic: host-side phases of one call
  const auto t_0 = std::chrono::steady_clock::now();
  auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count(); };
  const int W = c->opt.win_size, V = c->nvox, DIM = VBA_DIM, F = W - 1;
  const int n = W * DIM + (gravity ? 3 : 0), nb = gravity ? 33 : 30, n6 = 6 * W;
  if (!gravity) max_iter = 3;                                         // VM:643
  if (!c->d_li) {
    HIPCHK(c, hipMalloc((void **)&c->d_li, sizeof(LiDev)));
    HIPCHK(c, hipMalloc((void **)&c->d_imu, (size_t)LI_MAX_W * 304 * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&c->d_himu, (size_t)LI_MAX_N * LI_MAX_N * sizeof(double)));
    HIPCHK(c, hipMalloc((void **)&c->d_gimu, (size_t)LI_MAX_N * sizeof(double)));
  }
  // upload: LM state (poses view), the IMU extras, the factors with cov^-1 in place of cov
  std::vector<double> poses((size_t)W * 12);
  states_to_poses(states, W, poses.data());
  int st = vba_lm_begin(c, poses.data(), 0);
  if (st) return st;
  st = lm_init_flush(c);                      // the LI-BA kernels read the LM state from their first launch on
  if (st) return st;
  LiDev h{};
  h.W = W; h.n = n; h.nb = nb; h.gravity = gravity ? 1 : 0; h.gauge = gravity ? 6 : DIM; h.F = F; h.imu_coef = c->opt.imu_coef;   // VM:653-656 / 906-909
  for (int i = 0; i < W; i++) {
    const double *sx = states + 25 * i;
    h.tstamp[i] = sx[0];
    for (int k = 0; k < 12; k++) h.ex[12 * i + k] = h.ext[12 * i + k] = sx[13 + k];
  }
  std::vector<double> fimg((size_t)F * 304);
  std::memcpy(fimg.data(), imus, fimg.size() * sizeof(double));
  // cov^-1 (PI:166 / 244) is a property of the factor, and a sliding window hands the same factors in again scan after scan: a small
  // content-addressed cache (exact comparison of the 225 doubles) saves the host inversions (~4 us each)
  for (int f = 0; f < F; f++) {
    const double *cov = imus + 304 * (size_t)f + 79;
    double *dst = fimg.data() + 304 * (size_t)f + 79;
    bool hit = false;
    for (auto &e : c->covinv_cache)
      if (std::memcmp(e.data(), cov, 225 * sizeof(double)) == 0) { std::memcpy(dst, e.data() + 225, 225 * sizeof(double)); hit = true; break; }
    if (!hit) {
      vbh::inverse_pplu(cov, dst, 15);
      const bool grow = c->covinv_cache.size() < 32;
      if (grow) c->covinv_cache.emplace_back();
      auto &e = grow ? c->covinv_cache.back() : c->covinv_cache[c->covinv_next++ % 32];   // (round-robin replacement once full)
      std::memcpy(e.data(), cov, 225 * sizeof(double)); std::memcpy(e.data() + 225, dst, 225 * sizeof(double));
    }
  }
  {
    // (small pageable uploads are staged synchronously by the runtime, so the stack / vector sources may die after this)
    HIPCHK(c, hipMemcpyAsync(c->d_li, &h, sizeof(LiDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_imu, fimg.data(), fimg.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemsetAsync(c->d_himu, 0, (size_t)li_hb_size(W, 1) * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_gimu, 0, (size_t)n * sizeof(double), c->stream));
  char *base = reinterpret_cast<char *>(c->d_lm);
  const double *x_dev = reinterpret_cast<const double *>(base + offsetof(LmDev, x));
  const double *xt_dev = reinterpret_cast<const double *>(base + offsetof(LmDev, xt));
  const int *run_hess = reinterpret_cast<const int *>(base + offsetof(LmDev, run_hess));
  const int *run_res = reinterpret_cast<const int *>(base + offsetof(LmDev, run_res));
  const int copy_raw = c->collective() ? 1 : 0;
  const size_t lds_imu = ((size_t)2 * F * 15 * nb + 2 * F * 15 + F + 16) * sizeof(double);
  {
    static bool attr_set[kMaxDevices] = {false};      // W = 10 with gravity: 88 KB
    constexpr int FM = LI_MAX_W - 1;
    if (!attr_set[c->device % kMaxDevices]) { hipFuncSetAttribute((const void *)k_li_imu, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(((size_t)2 * FM * 15 * 33 + 2 * FM * 15 + FM + 16) * sizeof(double))); attr_set[c->device % kMaxDevices] = true; }
  }
  const double t_up = since(t_0);
  for (int it = 0; it < max_iter; it++) {
    // The IMU factors' workgroup rides in the lidar Hessian launch as block 0 on a CU of its own (k_hessian2).  As a kernel of its own
    // in front of the lidar pass it cost its 28 us + a kernel boundary; on a side stream (fork / join events around it) the two
    // cross-stream dependencies cost more than they hid (209 vs 196 us per iteration).
    const bool lidar_now = !(copy_raw && c->lm.have_hess) && V > 0 && lds_imu <= 150 * 1024;
    if (lidar_now) {          // the IMU workgroup rides in the lidar Hessian launch
      const LiJob job{c->d_lm, c->d_li, c->d_imu, c->d_himu, c->d_gimu};
      st = hessian_pass(c, x_dev, run_hess, 0, V, nullptr, nullptr, 0, job, lds_imu);   // lidar part of divide_thread (+ all-reduce)
    } else {
      hipLaunchKernelGGL(k_li_imu, dim3(1), dim3(LI_IMU_NT), lds_imu, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_himu, c->d_gimu);
      if (!(copy_raw && c->lm.have_hess)) st = hessian_pass(c, x_dev, run_hess, 0, V);
    }
    if (st) { c->lm.active = false; return st; }
    TimedSpan s1{};
    span_begin(c, "solve", s1);
    switch (W) {
      case 2: st = launch_li_solve<2>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 3: st = launch_li_solve<3>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 4: st = launch_li_solve<4>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 5: st = launch_li_solve<5>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 6: st = launch_li_solve<6>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 7: st = launch_li_solve<7>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 9: st = launch_li_solve<9>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 8: st = launch_li_solve<8>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 10: {
        static const int nt = diag_env("VBA_LI_NT") ? atoi(diag_env("VBA_LI_NT")) : 512;      // -DVBA_DIAG builds only
        if (nt == 256) st = launch_li_solve<10, 256>(c, copy_raw, n, h.gauge, h.gravity); else if (nt == 1024) st = launch_li_solve<10, 1024>(c, copy_raw, n, h.gauge, h.gravity); else st = launch_li_solve<10, 512>(c, copy_raw, n, h.gauge, h.gravity);
        break;
      }
      case 11: st = launch_li_solve<11>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 12: st = launch_li_solve<12>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 13: st = launch_li_solve<13>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 14: st = launch_li_solve<14>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 15: st = launch_li_solve<15>(c, copy_raw, n, h.gauge, h.gravity); break;
      case 16: st = launch_li_solve<16>(c, copy_raw, n, h.gauge, h.gravity); break;
      default: c->lm.active = false; return VBA_ERR_UNSUPPORTED_WINDOW;
    }
    span_end(c, "solve", s1);
    if (st) { c->lm.active = false; return st; }                     // (scratch allocation of the W > 10 solve failed: nothing was launched)
    if (copy_raw) {                                                   // one collective per iteration (see vba_lm_iterate)
      if (V > 0) launch_residual(c, xt_dev, run_res, 0, V);
      st = hessian_pass(c, xt_dev, run_res, 0, V);
      if (st) { c->lm.active = false; return st; }
      c->lm.have_hess = true;
      hipLaunchKernelGGL(k_li_update, dim3(1), dim3(LI_UPD_NT), 0, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_out + (nout_tl(W) - 1), 0);
    } else if (V == 0) {
      st = residual_pass(c, xt_dev, run_res, 0, V, c->d_scal);
      if (st) { c->lm.active = false; return st; }
      hipLaunchKernelGGL(k_li_update, dim3(1), dim3(LI_UPD_NT), 0, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_scal, 0);
    } else {
      const int nbk = residual_nb(c, V);
      TimedSpan s2{};
      span_begin(c, "residual", s2);
      launch_residual(c, xt_dev, run_res, 0, V);
      span_end(c, "residual", s2);
      hipLaunchKernelGGL(k_li_update, dim3(1), dim3(LI_UPD_NT), 0, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_partial, nbk);
    }
    HIPCHK(c, hipGetLastError());
  }
  const double t_enq = since(t_0);
  // (no drain before the download: with everything packed into ONE copy, queueing it behind the kernels is as fast as draining
  //  first — 497 vs 503 us per call; with five separate copies draining first had been 2-3x faster)
  const double t_gpu = since(t_0);
  // download: accepted state, the factors' bias increments, trace, and (on request) *hess = Hess before gauge fixing —
  // everything lands in ONE pinned block (pageable destinations make every copy a blocking staged transfer)
  // — gathered on the device into one block first: five separate D2H copies cost ~20 us each (110 us per call, measured)
  static_assert(sizeof(LiDev) % 8 == 0 && sizeof(LmDev) % 8 == 0, "packed as doubles");
  const size_t o_li = 0, o_img = o_li + sizeof(LiDev) / 8, o_hb = o_img + fimg.size(), o_lid = o_hb + (size_t)li_hb_size(W, 1),
               o_lm = o_lid + (size_t)n6 * n6, o_end = o_lm + sizeof(LmDev) / 8;
  st = ensure_pin(c, o_end + 64);
  if (st) return st;
  if (o_end + 64 > c->lipack_doubles) {
    if (c->d_lipack) hipFree(c->d_lipack);
    c->d_lipack = nullptr; c->lipack_doubles = 0;
    HIPCHK(c, hipMalloc((void **)&c->d_lipack, (o_end + 64) * sizeof(double)));
    c->lipack_doubles = o_end + 64;
  }
  PackSegs segs{};
  segs.n = 3;
  segs.src[0] = (const double *)c->d_li; segs.off[0] = o_li; segs.len[0] = sizeof(LiDev) / 8;
  segs.src[1] = c->d_imu; segs.off[1] = o_img; segs.len[1] = fimg.size();
  segs.src[2] = (const double *)c->d_lm; segs.off[2] = o_lm; segs.len[2] = sizeof(LmDev) / 8;
  if (hess) {
    st = tiles_to_full(c, copy_raw ? c->d_raw : c->d_out);
    if (st) return st;
    segs.n = 5;
    segs.src[3] = c->d_full; segs.off[3] = o_lid; segs.len[3] = (size_t)n6 * n6;
    segs.src[4] = c->d_himu; segs.off[4] = o_hb; segs.len[4] = (size_t)li_hb_size(W, gravity);
  }
  // (gathered on the device, then ONE copy: letting the gather kernel store the ~120 KB straight through the host mapping was
  //  measured slower — 187 against 174 us per iteration; for the few KB of the counters and of the lidar LM state it is faster)
  hipLaunchKernelGGL(k_pack_segments, dim3(64, segs.n), dim3(256), 0, c->stream, segs, c->d_lipack);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_pin, c->d_lipack, o_end * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(c->h_lm, c->h_pin + o_lm, sizeof(LmDev));
  std::memcpy(&h, c->h_pin + o_li, sizeof(LiDev));
  std::memcpy(fimg.data(), c->h_pin + o_img, fimg.size() * sizeof(double));
  const double *himu_h = c->h_pin + o_hb;
  c->lm.active = false;
  const LmDev *hl = c->h_lm;
  for (int i = 0; i < W; i++) {
    double *sx = states + 25 * i;
    for (int k = 0; k < 12; k++) sx[1 + k] = hl->x[12 * i + k];
    for (int k = 0; k < 12; k++) sx[13 + k] = h.ex[12 * i + k];
  }
  // (a rejected LAST step has installed the next damping candidate, which nothing evaluated: the caller sees what the sequential loop
  //  leaves behind, the restored increments of VM:701-705 = the buffers)
  if (hl->use_spec)
    for (int f = 0; f < F; f++) std::memcpy(fimg.data() + 304 * (size_t)f + 67, fimg.data() + 304 * (size_t)f + 73, 6 * sizeof(double));
  for (int f = 0; f < F; f++) std::memcpy(imus + 304 * (size_t)f + 67, fimg.data() + 304 * (size_t)f + 67, 12 * sizeof(double));   // dbg, dba, dbg_buf, dba_buf
  if (hess) {
    const double *lid = c->h_pin + o_lid;
    for (int r = 0; r < n; r++)
      for (int k = 0; k < n; k++) hess[(size_t)r * n + k] = c->opt.imu_coef * li_hb_get(himu_h, W, n, r, k);                     // VM:565
    for (int i = 0; i < W; i++)
      for (int j = 0; j < W; j++)
        for (int r = 0; r < 6; r++)
          for (int k = 0; k < 6; k++) hess[(size_t)(i * DIM + r) * n + j * DIM + k] += lid[(size_t)(i * 6 + r) * n6 + j * 6 + k];   // hess_plus VM:509-517
  }
  if (gravity && resis2) { resis2[0] = hl->resis_first; resis2[1] = hl->r2; }
  c->trace.assign(hl->trace, hl->trace + 5 * hl->n_trace);
  if (want_times && (hl->pad & 16)) {
    fprintf(stderr, "[k_li_solve prologue] stage imu %lld | stage lidar %lld | diag+g %lld | rank %lld\n", hl->stamps[50] - hl->stamps[0], hl->stamps[51] - hl->stamps[50], hl->stamps[52] - hl->stamps[51], hl->stamps[1] - hl->stamps[52]);
    fprintf(stderr, "[k_li_solve cycles] prologue %lld | tile load %lld | factorisation %lld | backsub %lld | epilogue %lld | panels:", hl->stamps[1] - hl->stamps[0],
            hl->stamps[2] - hl->stamps[1], hl->stamps[3] - hl->stamps[2], hl->stamps[4] - hl->stamps[3], hl->stamps[5] - hl->stamps[4]);
    const int npr = (int)hl->stamps[6];            // panels run: those from column n on are skipped
    for (int kb = 0; kb < npr && kb < 20; kb++) fprintf(stderr, " %lld+%lld", hl->stamps[9 + 2 * kb] - hl->stamps[8 + 2 * kb], kb < npr - 1 ? hl->stamps[10 + 2 * kb] - hl->stamps[9 + 2 * kb] : 0LL);
    fprintf(stderr, " | %d panels run\n", npr);
  }
  if (want_times && (hl->pad & 64)) fprintf(stderr, "[k_li_imu cycles] factor algebra (one lane per factor) %lld | cov^-1 joc %lld | contractions %lld\n", hl->stamps[41] - hl->stamps[40], hl->stamps[42] - hl->stamps[41], hl->stamps[43] - hl->stamps[42]);
  if (want_times && (hl->pad & 32)) { double v[6]; std::memcpy(v, &hl->stamps[58], sizeof(v)); fprintf(stderr, "[li r1 parts] rank %d: rimu %.10g lidar %.10g | %.10g %.10g | %.10g %.10g\n", c->rank, v[0], v[1], v[2], v[3], v[4], v[5]); }
  if (want_times) fprintf(stderr, "[li_ba_device] upload %.1f us | enqueue %.1f | gpu drained at %.1f | total %.1f\n", t_up, t_enq - t_up, t_gpu, since(t_0));
  return VBA_OK;
}

// ---------------------------------------------------------------- LI_BA_Optimizer / LI_BA_OptimizerGravity (VM:504-976)
int vba_li_ba_damping_iter(vba_ctx *c, double *states, double *imus, int gravity, int max_iter, double *hess, double *resis2) {
  // the whole optimiser runs on the device (k_li_imu / k_li_solve / k_li_update) for every window the context accepts (2..16)
  if (!li_device_supported(c->opt.win_size)) return VBA_ERR_UNSUPPORTED_WINDOW;
  return li_ba_device(c, states, imus, gravity, max_iter, hess, resis2);
}

// ---------------------------------------------------------------- initialisation odometry on a point-cloud map (vba_kernels_kd.hpp)
static int kd_reserve(vba_ctx *c, size_t pts) {
  if (pts <= c->kd_cap) return VBA_OK;
  size_t cap = c->kd_cap ? c->kd_cap : 65536;
  while (cap < pts) cap *= 2;
  for (int i = 0; i < 2; i++) {
    double *nw = nullptr;
    HIPCHK(c, hipMalloc((void **)&nw, cap * 3 * sizeof(double)));
    if (c->d_kdtree[i]) {
      if (i == c->kd_cur && c->kd_n > 0) HIPCHK(c, hipMemcpyAsync(nw, c->d_kdtree[i], (size_t)c->kd_n * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      hipFree(c->d_kdtree[i]);
    }
    c->d_kdtree[i] = nw;
  }
  c->kd_cap = cap;
  return VBA_OK;
}
int vba_odom_kdtree_reset(vba_ctx *c) { c->kd_n = 0; return VBA_OK; }
int vba_odom_kdtree_size(vba_ctx *c) { return c->kd_n; }
int vba_odom_kdtree_points(vba_ctx *c, double *out) {
  if (!out && c->kd_n > 0) return VBA_ERR_BAD_ARG;
  if (c->kd_n == 0) return VBA_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(out, c->d_kdtree[c->kd_cur], (size_t)c->kd_n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_odom_lio_state_estimation_kdtree(vba_ctx *c, int n, const double *pnt_body, double *state, double *cov, int *iterations) {
  if (n < 0 || (n > 0 && !pnt_body) || !state || !cov) return VBA_ERR_BAD_ARG;
  if (iterations) *iterations = 0;
  const int DIM = VBA_DIM, nb = (n + 255) / 256;
  const int kd_slices = nb >= 512 ? 1 : (nb >= 128 ? 4 : 8);               // enough workgroups to cover the chip
  int st = ensure_stage(c, ((size_t)n * 7 + (size_t)nb * 28 + (size_t)kd_slices * n * 5 + 64) * sizeof(double));
  if (st) return st;
  double *d_pts = (double *)c->d_stage, *d_pl = d_pts + (size_t)n * 3, *d_part = d_pl + (size_t)n * 4;
  unsigned long long *d_cand = (unsigned long long *)(d_part + (size_t)nb * 28);
  if (n > 0) HIPCHK(c, hipMemcpyAsync(d_pts, pnt_body, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  vbh::State x_curr, x_prop;
  std::memcpy(&x_curr, state, sizeof(x_curr));
  auto pose_of = [](const vbh::State &x) { KdPose X; std::memcpy(X.R, x.R, sizeof(X.R)); std::memcpy(X.t, x.p, sizeof(X.t)); return X; };
  st = kd_reserve(c, (size_t)c->kd_n + (size_t)n + 16);
  if (st) return st;
  if (c->kd_n < 100) {                                                       // VS:1105-1118: the map is only seeded
    if (n > 0) hipLaunchKernelGGL(k_kd_append, dim3(nb), dim3(256), 0, c->stream, n, d_pts, pose_of(x_curr), c->d_kdtree[c->kd_cur] + (size_t)c->kd_n * 3);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->kd_n += n;
    return VBA_OK;
  }
  x_prop = x_curr;
  std::vector<double> P(cov, cov + 225), cov_inv(225), part((size_t)nb * 28);
  vbh::inverse_pplu(P.data(), cov_inv.data(), DIM);                          // VS:1134
  const int num_max_iter = 4;
  int rematch_num = 0, iters = 0;
  bool refind = true, converged_once = false;
  double G[225];
  std::memset(G, 0, sizeof(G));
  for (int iter = 0; iter < num_max_iter; iter++) {
    iters++;
    const KdPose X = pose_of(x_curr);
    double s28[28];
    std::memset(s28, 0, sizeof(s28));
    if (n > 0) {
      if (refind) {
        hipLaunchKernelGGL(k_kd_match, dim3(nb, kd_slices), dim3(256), 0, c->stream, n, d_pts, X, c->kd_n, c->d_kdtree[c->kd_cur], d_cand);
        hipLaunchKernelGGL(k_kd_fit, dim3(nb), dim3(256), 0, c->stream, n, kd_slices, d_cand, c->d_kdtree[c->kd_cur], d_pl);
      }
      hipLaunchKernelGGL(k_kd_accum, dim3(nb), dim3(256), 0, c->stream, n, d_pts, X, d_pl, d_part);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (int b = 0; b < nb; b++) for (int k = 0; k < 28; k++) s28[k] += part[(size_t)b * 28 + k];
    }
    double HTH[36], HTz[6];
    { int idx = 0; for (int r = 0; r < 6; r++) for (int k = r; k < 6; k++) { HTH[r * 6 + k] = s28[idx]; HTH[k * 6 + r] = s28[idx]; idx++; } }
    for (int r = 0; r < 6; r++) HTz[r] = s28[21 + r];
    // K_1 = (H_T_H + cov_inv / 1000)^-1 ; G(:,0:6) = K_1(:,0:6) HTH ; solution = K_1(:,0:6) HTz + vec - G(:,0:6) vec(0:6)   VS:1213-1217
    std::vector<double> A(225), K1(225);
    for (int k = 0; k < 225; k++) A[k] = cov_inv[k] / 1000;
    for (int r = 0; r < 6; r++) for (int k = 0; k < 6; k++) A[r * DIM + k] += HTH[r * 6 + k];
    vbh::inverse_pplu(A.data(), K1.data(), DIM);
    for (int r = 0; r < DIM; r++)
      for (int k = 0; k < 6; k++) { double sacc = 0; for (int j = 0; j < 6; j++) sacc += K1[r * DIM + j] * HTH[j * 6 + k]; G[r * DIM + k] = sacc; }
    double vec[15], RtR[9], lg[3];
    vbh::m3_Tmul(x_curr.R, x_prop.R, RtR);
    vbh::so3_log(RtR, lg);
    for (int k = 0; k < 3; k++) { vec[k] = lg[k]; vec[3 + k] = x_prop.p[k] - x_curr.p[k]; vec[6 + k] = x_prop.v[k] - x_curr.v[k]; vec[9 + k] = x_prop.bg[k] - x_curr.bg[k]; vec[12 + k] = x_prop.ba[k] - x_curr.ba[k]; }
    double sol[15];
    for (int r = 0; r < DIM; r++) {
      double a = 0, b = 0;
      for (int j = 0; j < 6; j++) { a += K1[r * DIM + j] * HTz[j]; b += G[r * DIM + j] * vec[j]; }
      sol[r] = a + vec[r] - b;
    }
    double E[9], Rn[9];
    vbh::so3_exp(sol, E);
    vbh::m3_mul(x_curr.R, E, Rn);
    std::memcpy(x_curr.R, Rn, sizeof(Rn));
    for (int k = 0; k < 3; k++) { x_curr.p[k] += sol[3 + k]; x_curr.v[k] += sol[6 + k]; x_curr.bg[k] += sol[9 + k]; x_curr.ba[k] += sol[12 + k]; }
    const double rot_add = vbh::norm3(sol), tra_add = vbh::norm3(sol + 3);
    refind = false;                                                          // VS:1223-1234
    if ((rot_add * 57.3 < 0.01) && (tra_add * 100 < 0.015)) { refind = true; converged_once = true; rematch_num++; }
    if (iter == num_max_iter - 2 && !converged_once) refind = true;
    if (rematch_num >= 2 || (iter == num_max_iter - 1)) {
      std::vector<double> IG(225), Pn(225);
      for (int r = 0; r < DIM; r++) for (int k = 0; k < DIM; k++) IG[r * DIM + k] = (r == k ? 1.0 : 0.0) - G[r * DIM + k];
      vbh::mat_mul(IG.data(), P.data(), Pn.data(), DIM, DIM, DIM);
      P = Pn;
      break;
    }
  }
  // map update VS:1238-1250: append the scan in the refined pose, re-sample on a 0.5 m grid
  if (n > 0) hipLaunchKernelGGL(k_kd_append, dim3(nb), dim3(256), 0, c->stream, n, d_pts, pose_of(x_curr), c->d_kdtree[c->kd_cur] + (size_t)c->kd_n * 3);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int tot = c->kd_n + n;
  {
    std::vector<int> cnt(tot), first(tot);
    int m = 0;
    st = vba_scan_down_sampling_voxel(c, tot, c->d_kdtree[c->kd_cur], 0.5, c->d_kdtree[c->kd_cur ^ 1], cnt.data(), first.data(), &m);
    if (st) return st;
    c->kd_cur ^= 1; c->kd_n = m;
  }
  std::memcpy(state, &x_curr, sizeof(x_curr));
  std::memcpy(cov, P.data(), 225 * sizeof(double));
  if (iterations) *iterations = iters;
  return VBA_OK;
}

// ---------------------------------------------------------------- hierarchical global BA (vba_kernels_gba.hpp)
static GbaParams gba_params(vba_ctx *c, double voxel_size, double min_eig, const double *eig_array) {
  GbaParams P;
  P.voxel_size = voxel_size; P.min_eigen_value = min_eig; P.max_layer = c->opt.max_layer;
  for (int k = 0; k < 4; k++) P.eig_array[k] = eig_array[k];
  return P;
}
static int gba_build_into_store(vba_ctx *c, int wdsize, const int *offsets, const double *pl, const double *poses, const GbaParams &P) {
  int nf = 0;
  TimedSpan sp{};
  span_begin(c, "gba_build", sp);
  int st = gba_build(c->gba, c->stream, wdsize, offsets, pl, poses, P, &nf, c->err);
  if (st) return st;
  c->nvox = 0;
  st = factor_reserve(c, nf > 0 ? nf : 1);
  if (st) return st;
  if (nf > 0) {
    const int nn = c->gba.h_cnt[GCNT_NODES] < c->gba.v.cap ? c->gba.h_cnt[GCNT_NODES] : c->gba.v.cap;
    hipLaunchKernelGGL(k_gba_extract, dim3((nn + 255) / 256, 10 * wdsize + 33), dim3(256), 0, c->stream, c->gba.v, c->fv);
    factor_update_mask(c, 0, nf);
    HIPCHK(c, hipGetLastError());
  }
  span_end(c, "gba_build", sp);
  c->nvox = nf;
  return VBA_OK;
}
static int gba_check(vba_ctx *c, int wdsize, const int *offsets, const double *pl, const double *poses) {
  if (wdsize != c->opt.win_size) return VBA_ERR_UNSUPPORTED_WINDOW;
  if (!offsets || !poses || offsets[0] != 0) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < wdsize; i++) if (offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
  if (offsets[wdsize] > 0 && !pl) return VBA_ERR_BAD_ARG;
  return VBA_OK;
}
int vba_gba_build(vba_ctx *c, int wdsize, const int *offsets, const double *pnt_local, const double *poses, double gba_voxel_size,
                  double gba_min_eigen_value, const double *gba_eigen_value_array) {
  int st = gba_check(c, wdsize, offsets, pnt_local, poses);
  if (st) return st;
  if (!gba_eigen_value_array) return VBA_ERR_BAD_ARG;
  return gba_build_into_store(c, wdsize, offsets, pnt_local, poses, gba_params(c, gba_voxel_size, gba_min_eigen_value, gba_eigen_value_array));
}

// Lidar_BA_Optimizer::damping_iter (VM:422-497) for an arbitrary window: device Hessian / residual passes on the sparse
// store, gauge + (H + uD) LDL^T + retraction on the host.
// hdiag6_out: [W][W][6] = the six diagonal entries of every 6x6 block of *hess (all that HBA_add_edge reads of it, VS:2926-2951);
// the n x n Hessian itself stays in HBM.
static int big_damping_iter(vba_ctx *c, int W, double *poses, std::vector<double> &hdiag6_out, double *resis2, int max_iter, int thd_num, int *is_converge) {
  BigStore &S = c->big;
  const int n = 6 * W;
  if (S.b.V < thd_num) return VBA_ERR_TOO_FEW_VOXELS;                 // VM:399-403
  std::vector<double> x(poses, poses + (size_t)W * 12), xt(x), hd(n), JacT(n), dxi(n);
  double u = 0.01, v = 2, residual1 = 0, residual2 = 0;
  bool is_calc_hess = true, conv = true;
  c->trace.clear();
  for (int it = 0; it < max_iter; it++) {
    if (is_calc_hess) {
      int st = big_hessian(S, c->stream, x.data(), hd.data(), JacT.data(), &residual1, c->err);   // *hess = Hess (VM:446) stays on the device
      if (st) return st;
      for (int r = 0; r < 6; r++) { hd[r] = 1.0; JacT[r] = 0.0; }     // gauge VM:452-455 (k_bigl_setup applies it to the matrix)
    }
    if (it == 0) resis2[0] = residual1;
    {
      // pivot order of Eigen's LDLT (largest |stored diagonal| first, first index wins ties), then the device factorisation
      std::vector<int> ord(n);
      big_pivot_order(hd.data(), u, n, ord.data());
      int st2 = big_solve(S, c->stream, ord.data(), u, dxi.data(), c->err);
      if (st2) return st2;
    }
    for (int j = 0; j < W; j++) {
      double E[9];
      vbh::so3_exp(&dxi[6 * j], E);
      vbh::m3_mul(&x[12 * j], E, &xt[12 * j]);
      for (int k = 0; k < 3; k++) xt[12 * j + 9 + k] = x[12 * j + 9 + k] + dxi[6 * j + 3 + k];
    }
    const double q1 = big_q1(dxi.data(), hd.data(), JacT.data(), u, n);
    int st = big_residual(S, c->stream, xt.data(), &residual2, c->err);
    if (st) return st;
    double q = residual1 - residual2;
    const double tr[5] = {residual1, residual2, u, v, q1};
    c->trace.insert(c->trace.end(), tr, tr + 5);
    if (q > 0) {
      x = xt;
      q = q / q1;
      v = 2;
      q = 1 - std::pow(2 * q - 1, 3);
      u *= (q < 1.0 / 3 ? 1.0 / 3 : q);
      is_calc_hess = true;
    } else {
      u = u * v; v = 2 * v;
      is_calc_hess = false; conv = false;
    }
    if (std::fabs((residual1 - residual2) / residual1) < 1e-6) break;
  }
  resis2[1] = residual2;
  std::memcpy(poses, x.data(), x.size() * sizeof(double));
  if (is_converge) *is_converge = conv ? 1 : 0;
  hdiag6_out.resize((size_t)6 * W * W);
  return big_block_diagonals(S, c->stream, hdiag6_out.data(), c->err);   // b.H still holds the last evaluated Hessian (a rejected step does not recompute it)
}

int vba_hba_add_edge(vba_ctx *c, int wdsize, const int *offsets, const double *pnt_local, double *poses, double gba_voxel_size,
                     double gba_min_eigen_value, const double *gba_eigen_value_array, int max_iter, int thread_num, double *edges_out, int *n_edges,
                     double *cloud_out, int *cloud_count, int *n_cloud, double *resis_log, int *n_log) {
  const bool big = (wdsize != c->opt.win_size);      // any other window size (the top-level BA over all submaps): sparse path
  if (big && wdsize < 2) return VBA_ERR_BAD_ARG;
  int st = VBA_OK;
  if (!big) st = gba_check(c, wdsize, offsets, pnt_local, poses);
  else {
    if (!offsets || !poses || offsets[0] != 0) return VBA_ERR_BAD_ARG;
    for (int i = 0; i < wdsize; i++) if (offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
    if (offsets[wdsize] > 0 && !pnt_local) return VBA_ERR_BAD_ARG;
  }
  if (st) return st;
  if (!gba_eigen_value_array || !edges_out || !n_edges || (cloud_out && (!cloud_count || !n_cloud))) return VBA_ERR_BAD_ARG;
  const int W = wdsize, n6 = 6 * W, n = offsets[W];
  *n_edges = 0;
  if (n_log) *n_log = 0;
  static const bool want_times = diag_env("VBA_HBA_TIMES") != nullptr;      // diagnostic: wall-clock split of the call on stderr
  double t_ph[5] = {0, 0, 0, 0, 0};
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_mark = want_times ? now() : 0.0;
  auto lap = [&](int k) { if (want_times) { hipStreamSynchronize(c->stream); const double t = now(); t_ph[k] += t - t_mark; t_mark = t; } };
  // the keyframe clouds stay in HBM for the whole call (every outer iteration re-cuts them with the current poses)
  if ((size_t)n * 3 > c->refpts_doubles) {
    if (c->d_refpts) hipFree(c->d_refpts);
    c->refpts_doubles = (size_t)n * 3 + 3072;
    HIPCHK(c, hipMalloc((void **)&c->d_refpts, 2 * c->refpts_doubles * sizeof(double)));
  }
  double *d_pl = c->d_refpts, *d_ref = c->d_refpts + c->refpts_doubles;
  if (n > 0) HIPCHK(c, hipMemcpyAsync(d_pl, pnt_local, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  GbaParams P = gba_params(c, gba_voxel_size, gba_min_eigen_value, gba_eigen_value_array);
  std::vector<double> hess(big ? 0 : (size_t)n6 * n6, 0.0), hd6;      // the any-window path keeps *hess in HBM and returns its block diagonals
  lap(0);
  const int up = 4;                                                       // VS:2866
  int converge_flag = 0;
  double converge_thre = 0.05;
  for (int iterCnt = 0; iterCnt < max_iter; iterCnt++) {
    if (converge_flag == 1 || iterCnt == max_iter - 1)                    // VS:2871-2881: last pass with the local-map parameters
      P = gba_params(c, c->opt.voxel_size, c->opt.min_eigen_value, c->opt.plane_eigen_value_thre);
    double resis[2] = {0, 0};
    int is_converge = 0;
    if (!big) {
      st = gba_build_into_store(c, W, offsets, d_pl, poses, P);
      if (st) return st;
      lap(1);
      st = vba_lidar_ba_damping_iter(c, poses, hess.data(), resis, up, thread_num, &is_converge);
    } else {
      st = big_build(c->big, c->stream, W, offsets, d_pl, poses, P, c->err);
      if (st) return st;
      lap(1);
      st = big_damping_iter(c, W, poses, hd6, resis, up, thread_num, &is_converge);
    }
    if (st) return st;
    lap(2);
    if (resis_log && n_log) { resis_log[2 * *n_log] = resis[0]; resis_log[2 * *n_log + 1] = resis[1]; (*n_log)++; }
    if ((std::fabs(resis[0] - resis[1]) / resis[0] < converge_thre && is_converge) || (iterCnt == max_iter - 2 && converge_flag == 0)) {
      converge_thre = 0.01;                                               // VS:2903-2915
      if (converge_flag == 0) converge_flag = 1;
      else if (converge_flag == 1) break;
    }
  }
  int ne = 0;
  for (int i = 0; i < W - 1; i++)
    for (int j = i + 1; j < W; j++) {                                     // VS:2926-2951
      bool isAdd = true;
      double v6[6];
      for (int k = 0; k < 6; k++) {
        const double hc = std::fabs(big ? hd6[((size_t)i * W + j) * 6 + k] : hess[(size_t)(6 * i + k) * n6 + 6 * j + k]);
        if (hc < 1e-6) { isAdd = false; break; }
        v6[k] = 1.0 / hc;
      }
      if (!isAdd) continue;
      double *o = edges_out + 20 * (size_t)ne++;
      const double *Ri = poses + 12 * i, *Rj = poses + 12 * j;
      o[0] = i; o[1] = j;
      vbh::m3_Tmul(Ri, Rj, o + 2);
      const double d[3] = {Rj[9] - Ri[9], Rj[10] - Ri[10], Rj[11] - Ri[11]};
      vbh::m3_Tvec(Ri, d, o + 11);
      for (int k = 0; k < 6; k++) o[14 + k] = v6[k];
    }
  *n_edges = ne;
  lap(3);
  if (cloud_out) {                                                        // VS:2954-2989
    *n_cloud = 0;
    if (n > 0) {
      std::vector<double> rel((size_t)W * 12);
      for (int i = 0; i < W; i++) {
        const double *R0 = poses, *Ri = poses + 12 * i;
        vbh::m3_Tmul(R0, Ri, rel.data() + 12 * i);
        const double d[3] = {Ri[9] - R0[9], Ri[10] - R0[10], Ri[11] - R0[11]};
        vbh::m3_Tvec(R0, d, rel.data() + 12 * i + 9);
      }
      double *d_rel = big ? c->big.g.poses : c->gba.v.poses;
      const int *d_off = big ? c->big.g.offsets : c->gba.v.offsets;
      HIPCHK(c, hipMemcpyAsync(d_rel, rel.data(), rel.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(k_gba_to_ref, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, W, d_off, d_pl, d_rel, d_ref);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipStreamSynchronize(c->stream));      // rel is a host temporary
      std::vector<int> first(n);
      st = vba_scan_down_sampling_voxel(c, n, d_ref, c->opt.voxel_size / 8, cloud_out, cloud_count, first.data(), n_cloud);
      if (st) return st;
    }
  }
  lap(4);
  if (want_times)
    std::fprintf(stderr, "[hba_add_edge W=%d n=%d] upload %.0f  build %.0f  LM %.0f  edges %.0f  cloud %.0f us\n", W, n, t_ph[0], t_ph[1], t_ph[2], t_ph[3], t_ph[4]);
  return VBA_OK;
}

// thd_globalmapping (VS:3018-3141), the optimisation work of the hierarchical global BA over one map:
//   bottom layer  windows of `wdsize` keyframes, stride `mgsize` (VS:3033-3034, 3064-3066, 3136-3137): HBA_add_edge(xs = x0 of the
//                 window, max_iter 1, thread_num 2) -> edges1 + one submap (pose x0 of the window's first keyframe, cloud
//                 = the window's down-sampled points in that frame, VS:3084-3089);
//   top layer     HBA_add_edge over all submaps with their CURRENT poses (VS:3096-3110): edges2.
// Edge rows carry GLOBAL keyframe indices.  (Queue handling, map switching and the GTSAM pose graph stay with the caller.)
int vba_hba_global(vba_ctx *c, int n_kf, const int *offsets, const double *pnt_local, const double *poses_x0, const double *poses_now,
                   double gba_voxel_size, double gba_min_eigen_value, const double *gba_eigen_value_array, int total_max_iter, int wdsize, int mgsize,
                   double *edges1_out, int cap1, int *n_edges1, double *edges2_out, int cap2, int *n_edges2) {
  if (n_kf < 0 || wdsize < 2 || mgsize < 1 || !offsets || !poses_x0 || !poses_now || !gba_eigen_value_array || !n_edges1 || !n_edges2 ||
      (offsets[n_kf] > 0 && !pnt_local))
    return VBA_ERR_BAD_ARG;
  *n_edges1 = 0; *n_edges2 = 0;
  std::vector<int> sub_first, sub_n;                // global id of every submap's first keyframe, points of its cloud
  std::vector<double> edges((size_t)(wdsize * (wdsize - 1) / 2 + 1) * 20);
  // the keyframe clouds go to HBM once (the stride-5 windows overlap: every keyframe is used twice) and the submap clouds
  // never leave it: every window's down-sampled cloud is written behind the previous one and the top-level BA reads them there
  const size_t n_all = (size_t)offsets[n_kf];
  size_t n_sub_cap = 0, n_win_max = 0;
  for (int start = 0; start + wdsize <= n_kf; start += mgsize) {
    const size_t nw = (size_t)(offsets[start + wdsize] - offsets[start]);
    n_sub_cap += nw; if (nw > n_win_max) n_win_max = nw;
  }
  // More than one rank ("windows are independent problems => replicas across GPUs for the bottom layer"): window
  // wi is optimised by rank wi % n_ranks with the exchange step switched off; every rank packs its windows' clouds and its
  // [points, edges, status | edge rows] records into ITS chunk of two buffers, and one ALL-GATHER of each hands every rank all of
  // them (a rank receives each foreign byte once).  A window that fails on one rank travels as its status word: every rank
  // enters both collectives and all of them return the same error afterwards — no rank is left waiting in a collective.
  // The top-level window then runs replicated (identical inputs on every rank).
  const bool replicas = c->collective() && c->n_ranks > 1;
  int n_win = 0;
  for (int start = 0; start + wdsize <= n_kf; start += mgsize) n_win++;
  // ONE rank: the windows are independent problems too, and one window is a chain of small kernels and host round trips that leaves
  // most of the chip idle — KL worker contexts (own stream, own octree and LM state; host threads drive them) optimise windows
  // side by side, with the bookkeeping of the replicas: worker t takes windows t, t + KL, ... and writes their clouds into its chunk.
  const int kl_opt = c->opt.hba_workers > 0 ? (c->opt.hba_workers < 8 ? c->opt.hba_workers : 8) : 4;
  const int KL = (!replicas && n_win >= 2 * kl_opt) ? kl_opt : 1;
  const bool local_rep = KL > 1, chunked = replicas || local_rep;
  const int NR = replicas ? c->n_ranks : KL;
  const size_t meta_per = 3 + (size_t)(wdsize * (wdsize - 1) / 2) * 20;
  const size_t win_per_rank = chunked ? (size_t)(n_win + NR - 1) / NR : 0, meta_chunk = meta_per * win_per_rank;
  std::vector<size_t> rank_cap(NR, 0), win_roff(n_win > 0 ? n_win : 1, 0);      // points capacity per rank chunk, window offset inside it
  if (chunked) {
    int w = 0;
    for (int start = 0; start + wdsize <= n_kf; start += mgsize, w++) {
      win_roff[w] = rank_cap[w % NR];
      rank_cap[w % NR] += (size_t)(offsets[start + wdsize] - offsets[start]);
    }
  }
  size_t chunk_pts = 0;
  for (int r = 0; r < NR; r++) if (rank_cap[r] > chunk_pts) chunk_pts = rank_cap[r];
  if (!chunked) chunk_pts = 0;
  const size_t need = (n_all + n_sub_cap + (size_t)NR * chunk_pts) * 3 + (size_t)NR * meta_chunk + 64;
  if (need > c->hba_all_doubles) {
    if (c->d_hba_all) hipFree(c->d_hba_all);
    c->d_hba_all = nullptr; c->hba_all_doubles = 0;
    HIPCHK(c, hipMalloc((void **)&c->d_hba_all, need * sizeof(double)));
    c->hba_all_doubles = need;
  }
  double *d_all = c->d_hba_all, *d_sub = c->d_hba_all + n_all * 3;
  if (n_all > 0 && !local_rep) HIPCHK(c, hipMemcpyAsync(d_all, pnt_local, n_all * 3 * sizeof(double), hipMemcpyDefault, c->stream));   // (the worker path uploads in chunks, under the first windows)
  std::vector<int> ccnt(n_win_max > 0 ? n_win_max : 1);
  size_t sub_off = 0;
  double *d_rep = d_sub + n_sub_cap * 3, *d_meta = d_rep + (size_t)NR * chunk_pts * 3;      // replica mode only
  std::vector<double> meta((size_t)NR * meta_chunk, 0.0);
  struct Restore { vba_ctx *c; bool was; ~Restore() { c->collective_off = was; } } restore{c, c->collective_off};
  if (replicas) c->collective_off = true;                                       // the windows' own LM loops must not enter a collective
  int wi = -1;
  static const bool want_times = diag_env("VBA_HBA_TIMES") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_g0 = want_times ? (hipStreamSynchronize(c->stream), now()) : 0.0;
  double t_g1 = 0;
  if (local_rep) {
    while ((int)c->hba_workers.size() < KL - 1) {
      vba_options o = c->opt; o.stream = nullptr; o.device = c->device;
      vba_ctx *w = nullptr;
      const int stc = vba_create(&o, &w);
      if (stc) { c->set_error("vba_hba_global: could not create a worker context"); return stc; }
      c->hba_workers.push_back(w);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int w = 0; w < n_win; w++) meta[(size_t)(w % KL) * meta_chunk + meta_per * (size_t)(w / KL) + 2] = -1.0;   // "not run"
    std::vector<std::string> werr(KL);
    // the keyframe clouds travel to HBM in chunks on a stream of their own while the first windows are already being optimised
    // (2.4 GB at full length: as long as the windows themselves); a window starts when its keyframes have arrived
    std::atomic<int> kf_ready{0}, give_up{0};
    auto work = [&](int tw) {
      vba_ctx *cx = tw == 0 ? c : c->hba_workers[tw - 1];
      hipSetDevice(c->device);
      std::vector<double> ed(edges.size());
      std::vector<int> cc(ccnt.size()), off(wdsize + 1);
      for (int w = tw; w < n_win; w += KL) {
        const int start = w * mgsize;
        while (kf_ready.load(std::memory_order_acquire) < start + wdsize && !give_up.load()) std::this_thread::sleep_for(std::chrono::microseconds(20));
        if (give_up.load()) return;
        for (int i = 0; i <= wdsize; i++) off[i] = offsets[start + i] - offsets[start];
        std::vector<double> xs(poses_x0 + (size_t)start * 12, poses_x0 + (size_t)(start + wdsize) * 12);
        int ne = 0, nc = 0;
        double *mrec = &meta[(size_t)tw * meta_chunk + meta_per * (size_t)(w / KL)];
        const int st = vba_hba_add_edge(cx, wdsize, off.data(), d_all + (size_t)offsets[start] * 3, xs.data(), gba_voxel_size, gba_min_eigen_value,
                                        gba_eigen_value_array, 1, 2, ed.data(), &ne, d_rep + ((size_t)tw * chunk_pts + win_roff[w]) * 3,
                                        cc.data(), &nc, nullptr, nullptr);
        mrec[2] = st;
        if (st != VBA_OK) { werr[tw] = cx->err; return; }
        mrec[0] = nc; mrec[1] = ne;
        std::memcpy(mrec + 3, ed.data(), (size_t)ne * 20 * sizeof(double));
      }
    };
    int up_status = VBA_OK;
    {
      std::vector<std::thread> th;
      for (int tw = 0; tw < KL; tw++) th.emplace_back(work, tw);
      // (one uploader: three threads staging chunks in turn moved the pageable copy no faster — 4-5 GB/s either way; at full
      //  length the call is bound by this copy once the windows overlap it)
      hipStream_t up = nullptr;
      if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) { up_status = VBA_ERR_HIP; give_up.store(1); }
      const int CH = 16;                                                           // keyframes per chunk
      for (int k0 = 0; k0 < n_kf && up_status == VBA_OK; k0 += CH) {
        const int k1 = k0 + CH < n_kf ? k0 + CH : n_kf;
        const size_t o0 = (size_t)offsets[k0] * 3, nb = (size_t)(offsets[k1] - offsets[k0]) * 3 * sizeof(double);
        if (nb > 0 && (hipMemcpyAsync(d_all + o0, pnt_local + o0, nb, hipMemcpyDefault, up) != hipSuccess || hipStreamSynchronize(up) != hipSuccess)) {
          up_status = VBA_ERR_HIP; give_up.store(1); break;
        }
        kf_ready.store(k1, std::memory_order_release);
      }
      if (up) hipStreamDestroy(up);
      for (auto &x : th) x.join();
    }
    hipSetDevice(c->device);
    if (up_status != VBA_OK) { c->set_error("vba_hba_global: uploading the keyframe clouds failed"); return up_status; }
    for (int w = 0; w < n_win; w++) {                                            // the first failing window in window order decides
      const int stw = (int)meta[(size_t)(w % KL) * meta_chunk + meta_per * (size_t)(w / KL) + 2];
      if (stw > 0) { if (!werr[w % KL].empty()) c->set_error(werr[w % KL]); return stw; }
    }
    for (int w = 0; w < n_win; w++) {
      const double *mrec = &meta[(size_t)(w % KL) * meta_chunk + meta_per * (size_t)(w / KL)];
      if ((int)mrec[2] != VBA_OK) { c->set_error("vba_hba_global: a bottom-layer window was not run"); return VBA_ERR_HIP; }
      const int nc = (int)mrec[0], ne = (int)mrec[1], start = w * mgsize;
      for (int e = 0; e < ne; e++) {
        if (*n_edges1 >= cap1) return VBA_ERR_CAPACITY;
        double *o = edges1_out + (size_t)(*n_edges1) * 20;
        std::memcpy(o, mrec + 3 + (size_t)e * 20, 20 * sizeof(double));
        o[0] += start; o[1] += start;
        (*n_edges1)++;
      }
      if (nc > 0) HIPCHK(c, hipMemcpyAsync(d_sub + sub_off * 3, d_rep + ((size_t)(w % KL) * chunk_pts + win_roff[w]) * 3, (size_t)nc * 3 * sizeof(double),
                                           hipMemcpyDeviceToDevice, c->stream));
      sub_first.push_back(start);
      sub_n.push_back(nc);
      sub_off += (size_t)nc;
    }
  }
  for (int start = 0; !local_rep && start + wdsize <= n_kf; start += mgsize) {
    std::vector<int> off(wdsize + 1);
    for (int i = 0; i <= wdsize; i++) off[i] = offsets[start + i] - offsets[start];
    std::vector<double> xs(poses_x0 + (size_t)start * 12, poses_x0 + (size_t)(start + wdsize) * 12);
    int ne = 0, nc = 0;
    wi++;
    if (replicas) {
      sub_first.push_back(start);
      if (wi % NR != c->rank) continue;
      double *mrec = &meta[(size_t)c->rank * meta_chunk + meta_per * (size_t)(wi / NR)];
      const int st = vba_hba_add_edge(c, wdsize, off.data(), d_all + (size_t)offsets[start] * 3, xs.data(), gba_voxel_size, gba_min_eigen_value,
                                      gba_eigen_value_array, 1, 2, edges.data(), &ne, d_rep + ((size_t)c->rank * chunk_pts + win_roff[wi]) * 3,
                                      ccnt.data(), &nc, nullptr, nullptr);
      mrec[2] = st;                            // travels with the gather: every rank learns it
      if (st == VBA_OK) {
        mrec[0] = nc; mrec[1] = ne;
        std::memcpy(mrec + 3, edges.data(), (size_t)ne * 20 * sizeof(double));
      }
      continue;
    }
    int st = vba_hba_add_edge(c, wdsize, off.data(), d_all + (size_t)offsets[start] * 3, xs.data(), gba_voxel_size, gba_min_eigen_value,
                              gba_eigen_value_array, 1, 2, edges.data(), &ne, d_sub + sub_off * 3, ccnt.data(), &nc, nullptr, nullptr);
    if (st) return st;
    for (int e = 0; e < ne; e++) {
      if (*n_edges1 >= cap1) return VBA_ERR_CAPACITY;
      double *o = edges1_out + (size_t)(*n_edges1) * 20;
      std::memcpy(o, &edges[(size_t)e * 20], 20 * sizeof(double));
      o[0] += start; o[1] += start;
      (*n_edges1)++;
    }
    sub_first.push_back(start);
    sub_n.push_back(nc);
    sub_off += (size_t)nc;
  }
  if (replicas) {
    c->collective_off = restore.was;
    if (meta_chunk > 0)
      HIPCHK(c, hipMemcpyAsync(d_meta + (size_t)c->rank * meta_chunk, meta.data() + (size_t)c->rank * meta_chunk, meta_chunk * sizeof(double),
                               hipMemcpyHostToDevice, c->stream));
    int rc = ctx_allgather(c, d_rep, chunk_pts * 3);
    if (rc) return rc;
    rc = ctx_allgather(c, d_meta, meta_chunk);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyAsync(meta.data(), d_meta, meta.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int worst = VBA_OK;
    for (int w = 0; w < n_win; w++) {
      const int stw = (int)meta[(size_t)(w % NR) * meta_chunk + meta_per * (size_t)(w / NR) + 2];
      if (stw != VBA_OK && worst == VBA_OK) worst = stw;
    }
    if (worst != VBA_OK) { c->set_error("a bottom-layer window failed on one of the ranks"); return worst; }   // the same on every rank
    for (int w = 0; w < n_win; w++) {
      const double *mrec = &meta[(size_t)(w % NR) * meta_chunk + meta_per * (size_t)(w / NR)];
      const int nc = (int)mrec[0], ne = (int)mrec[1], start = sub_first[w];
      for (int e = 0; e < ne; e++) {
        if (*n_edges1 >= cap1) return VBA_ERR_CAPACITY;
        double *o = edges1_out + (size_t)(*n_edges1) * 20;
        std::memcpy(o, mrec + 3 + (size_t)e * 20, 20 * sizeof(double));
        o[0] += start; o[1] += start;
        (*n_edges1)++;
      }
      if (nc > 0) HIPCHK(c, hipMemcpyAsync(d_sub + sub_off * 3, d_rep + ((size_t)(w % NR) * chunk_pts + win_roff[w]) * 3, (size_t)nc * 3 * sizeof(double),
                                           hipMemcpyDeviceToDevice, c->stream));
      sub_n.push_back(nc);
      sub_off += (size_t)nc;
    }
  }
  const int ns = (int)sub_first.size();
  if (want_times) t_g1 = now();
  struct Report { bool on; double t0, *t1; decltype(now) *clk; ~Report() { if (on) std::fprintf(stderr, "[hba_global] windows %.0f us, top %.0f us (after the upload)\n", *t1 - t0, (*clk)() - *t1); } } report{want_times, t_g0, &t_g1, &now};
  if (ns >= 2) {
    std::vector<int> off(ns + 1, 0);
    for (int i = 0; i < ns; i++) off[i + 1] = off[i] + sub_n[i];
    std::vector<double> xs((size_t)ns * 12), e2((size_t)(ns * (ns - 1) / 2 + 1) * 20);
    for (int i = 0; i < ns; i++) std::memcpy(&xs[(size_t)i * 12], poses_now + (size_t)sub_first[i] * 12, 12 * sizeof(double));
    int ne = 0;
    int st = vba_hba_add_edge(c, ns, off.data(), d_sub, xs.data(), gba_voxel_size, gba_min_eigen_value, gba_eigen_value_array, total_max_iter, 5,
                              e2.data(), &ne, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (st) return st;
    for (int e = 0; e < ne; e++) {
      if (*n_edges2 >= cap2) return VBA_ERR_CAPACITY;
      double *o = edges2_out + (size_t)(*n_edges2) * 20;
      std::memcpy(o, &e2[(size_t)e * 20], 20 * sizeof(double));
      o[0] = sub_first[(int)e2[(size_t)e * 20]]; o[1] = sub_first[(int)e2[(size_t)e * 20 + 1]];
      (*n_edges2)++;
    }
  }
  return VBA_OK;
}

// ---------------------------------------------------------------- IMU factor (host)
int vba_imu_preintegrate(int n, const double *t, const double *gyr, const double *acc, const double *bg, const double *ba,
                         const double *nm6, const double *nw6, double scale_gravity, double *out) {
  if (n < 1 || !t || !gyr || !acc || !out) return VBA_ERR_BAD_ARG;
  vbh::ImuPre m;
  vbh::imu_init(m, bg, ba);
  vbh::imu_push(m, n, t, gyr, acc, nm6, nw6, scale_gravity);
  std::memcpy(out, &m, sizeof(m));
  return VBA_OK;
}
int vba_imu_give_evaluate(const double *imu_pre, const double *s1, const double *s2, int with_gravity, int jac_enable, double *jtj,
                          double *gg, double *resid) {
  if (!imu_pre || !s1 || !s2) return VBA_ERR_BAD_ARG;
  const double r = vbh::imu_evaluate(*reinterpret_cast<const vbh::ImuPre *>(imu_pre), *reinterpret_cast<const vbh::State *>(s1),
                                     *reinterpret_cast<const vbh::State *>(s2), with_gravity != 0, jac_enable != 0, jtj, gg);
  if (resid) *resid = r;
  return VBA_OK;
}

// ---------------------------------------------------------------- multi-GPU plumbing
int vba_set_allreduce(vba_ctx *c, vba_allreduce_fn fn, void *user) { c->allreduce = fn; c->allreduce_user = user; return VBA_OK; }

// RCCL inside the library (north_star: "RCCL all-reduce of the (6W)x(6W) Hessian over xGMI"): the communicator lives in the context
// and ncclAllReduce(ncclDouble, ncclSum) is issued on the context's stream, no host code in the LM loop.
int vba_rccl_get_unique_id(void *out128) {
  if (!out128) return VBA_ERR_BAD_ARG;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  const RcclApi &R = rccl_api();
  if (!R.ok) return VBA_ERR_UNSUPPORTED;
  ncclUniqueId id;
  if (R.GetUniqueId(&id) != ncclSuccess) return VBA_ERR_HIP;
  std::memcpy(out128, &id, sizeof(id));
  return VBA_OK;
}
int vba_rccl_init(vba_ctx *c, const void *unique_id128, int rank, int n_ranks) {
  if (!c || !unique_id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return VBA_ERR_BAD_ARG;
  const RcclApi &R = rccl_api();
  if (!R.ok) { c->set_error(R.why); return VBA_ERR_UNSUPPORTED; }
  if (c->comm && c->own_comm) { R.CommDestroy(c->comm); c->comm = nullptr; }
  ncclUniqueId id;
  std::memcpy(&id, unique_id128, sizeof(id));
  HIPCHK(c, hipSetDevice(c->device));
  const ncclResult_t r = R.CommInitRank(&c->comm, n_ranks, id, rank);
  if (r != ncclSuccess) { c->comm = nullptr; c->set_error(std::string("ncclCommInitRank: ") + R.GetErrorString(r)); return VBA_ERR_HIP; }
  c->own_comm = true;
  return vba_set_shard(c, rank, n_ranks);
}
int vba_set_rccl_comm(vba_ctx *c, void *nccl_comm) {
  if (!c) return VBA_ERR_BAD_ARG;
  const RcclApi &R = rccl_api();
  if (!R.ok) { c->set_error(R.why); return VBA_ERR_UNSUPPORTED; }
  if (c->comm && c->own_comm) R.CommDestroy(c->comm);
  c->comm = (ncclComm_t)nccl_comm; c->own_comm = false;
  return VBA_OK;
}
int vba_shard_owner(int64_t kx, int64_t ky, int64_t kz, int n_ranks) {
  if (n_ranks <= 1) return 0;
  return (int)(vba::shard_bucket(kx, ky, kz) * (uint64_t)n_ranks >> 16);   // contiguous bucket ranges per rank
}
int vba_set_shard(vba_ctx *c, int rank, int n_ranks) {
  if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return VBA_ERR_BAD_ARG;
  c->rank = rank; c->n_ranks = n_ranks;
  c->map.rank = rank; c->map.n_ranks = n_ranks;
  c->map.allreduce = [c](double *buf, size_t n) { return (c->allreduce || c->comm) ? ctx_allreduce(c, buf, n) : (int)VBA_ERR_BAD_ARG; };
  return VBA_OK;
}

// ---------------------------------------------------------------- timing
// Measurement aid: one launch that reads exactly n_bytes (rounded down to a multiple of 32 KiB) from a zero-filled scratch buffer
// in the access shape of the factor store (k_calib_read8).  Under `rocprofv3 --pmc FETCH_SIZE` its counter value calibrates the
// read-side correction factor tools/prof_summary.py applies to the residual pass.
int vba_timing_calibration_read(vba_ctx *c, size_t n_bytes) {
  const size_t nblk = n_bytes / (256 * 128);
  if (nblk == 0 || nblk > 0x7fffffffu) return VBA_ERR_BAD_ARG;
  double *buf = nullptr;
  HIPCHK(c, hipMalloc((void **)&buf, nblk * 256 * 128 + 64));
  HIPCHK(c, hipMemsetAsync(buf, 0, nblk * 256 * 128 + 64, c->stream));
  hipLaunchKernelGGL(k_calib_read8, dim3((unsigned)nblk), dim3(256), 0, c->stream, buf, buf + nblk * 256 * 16);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  hipFree(buf);
  return VBA_OK;
}
int vba_timing_enable(vba_ctx *c, int on) { c->timing = on != 0; return VBA_OK; }
int vba_timing_null_span(vba_ctx *c) {   // an event pair around nothing: the bracketing overhead itself (recorded as "null")
  TimedSpan s{};
  const bool was = c->timing;
  const std::string only = c->timing_only;
  c->timing = true; c->timing_only.clear();
  span_begin(c, "null", s);
  span_end(c, "null", s);
  c->timing = was; c->timing_only = only;
  return VBA_OK;
}
int vba_timing_select(vba_ctx *c, const char *name) { c->timing_only = name ? name : ""; return VBA_OK; }
int vba_timing_sample_every(vba_ctx *c, int n) { c->timing_every = n > 1 ? n : 1; c->timing_ctr = 0; return VBA_OK; }
int vba_timing_reset(vba_ctx *c) {
  hipStreamSynchronize(c->stream);
  for (auto &kv : c->spans) for (auto &s : kv.second) { hipEventDestroy(s.a); hipEventDestroy(s.b); }
  c->spans.clear();
  return VBA_OK;
}
int vba_timing_get(vba_ctx *c, const char *name, double *total_us, int *count) {
  hipStreamSynchronize(c->stream);
  double tot = 0; int n = 0;
  auto it = c->spans.find(name);
  if (it != c->spans.end())
    for (auto &s : it->second) { float ms = 0; if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { tot += (double)ms * 1000.0; n++; } }
  if (total_us) *total_us = tot;
  if (count) *count = n;
  return VBA_OK;
}

// ---------------------------------------------------------------- map level (vba_kernels_map.hpp)
int vba_map_cut_voxel(vba_ctx *c, int win_count, int n, const double *pnt_body, const double *var, const double *pose, int multi) {
  TimedSpan s{};
  span_begin(c, "insert", s);
  const int st = map_cut_voxel(c->map, c->stream, win_count, n, pnt_body, var, pose, multi != 0, c->err);
  span_end(c, "insert", s);
  return st;
}
int vba_map_pvec_update_cut_voxel(vba_ctx *c, int win_count, int n, const double *pnt_body, const double *var_body, const double *pose,
                                  const double *cov, int multi) {
  if (!cov || !var_body) return VBA_ERR_BAD_ARG;
  double cov6[18];
  for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) { cov6[3 * r + k] = cov[r * VBA_DIM + k]; cov6[9 + 3 * r + k] = cov[(3 + r) * VBA_DIM + 3 + k]; }
  TimedSpan s{};
  span_begin(c, "insert", s);
  const int st = map_cut_voxel(c->map, c->stream, win_count, n, pnt_body, var_body, pose, multi != 0, c->err, cov6);
  span_end(c, "insert", s);
  return st;
}
int vba_scan_var_init(vba_ctx *c, int n, const double *pnt_in, const double *ext_pose, double dept_err, double beam_err, double *pnt_out,
                      double *var_out) {
  if (n < 0 || (n > 0 && (!pnt_in || !pnt_out || !var_out)) || !ext_pose) return VBA_ERR_BAD_ARG;
  if (n == 0) return VBA_OK;
  int st = ensure_stage(c, ((size_t)n * 15 + 16) * sizeof(double));
  if (st) return st;
  double *d_in = (double *)c->d_stage, *d_out = d_in + (size_t)n * 3, *d_var = d_out + (size_t)n * 3, *d_ext = d_var + (size_t)n * 9;
  HIPCHK(c, hipMemcpyAsync(d_in, pnt_in, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ext, ext_pose, 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_var_init, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d_in, d_out, d_var, d_ext, (float)dept_err, (float)beam_err);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(pnt_out, d_out, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(var_out, d_var, (size_t)n * 9 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}
// The device half of the down-samplers: everything between the input and the emit, on buffers the caller owns.
//   tab [cap] slots (cap a power of two >= 2n), slot [n], blk [(n + 255) / 256], n_out [1]; dist [n] for mode 2;
//   deterministic mode: skey / idx / sidx [n] and rocPRIM scratch tmp (sort_pairs_u32 over n keys of key_bits bits).
// After it the table holds every voxel's sums, count and first point, blk the exclusive scan of the per-block voxel counts and
// *n_out the number of voxels: what k_ds_emit (and the keyframe store's k_kf_emit) compact in first-occurrence order.
struct DsWork {
  DsSlot *tab = nullptr; int cap = 0; unsigned int key_bits = 0;
  int *slot = nullptr, *blk = nullptr, *n_out = nullptr; double *dist = nullptr;
  unsigned int *skey = nullptr; int *idx = nullptr, *sidx = nullptr; void *tmp = nullptr; size_t tmp_bytes = 0;
};
static int ds_core(vba_ctx *c, hipStream_t stream, int mode, int n, const double *d_in, const double *d_var, int vrow, int vstep, double voxel_size,
                   bool det, const DsWork &w) {
  const int nb = (n + 255) / 256;
  hipLaunchKernelGGL(k_ds_clear, dim3((w.cap + 255) / 256), dim3(256), 0, stream, w.tab, w.cap);
  if (det) {
    hipLaunchKernelGGL(k_ds_insert<true>, dim3(nb), dim3(256), 0, stream, n, d_in, d_var, voxel_size, w.tab, w.cap - 1, w.slot, vrow, vstep);
    hipLaunchKernelGGL(k_iota, dim3(nb), dim3(256), 0, stream, w.idx, n);
    size_t tmp = w.tmp_bytes;
    HIPCHK(c, sort_pairs_u32(w.tmp, tmp, (const unsigned int *)w.slot, w.skey, w.idx, w.sidx, (size_t)n, w.key_bits, stream));
    hipLaunchKernelGGL(k_ds_segstart, dim3(nb), dim3(256), 0, stream, n, w.skey, w.tab);
    hipLaunchKernelGGL(k_ds_sum_det, dim3(nb), dim3(256), 0, stream, n, d_in, d_var, w.sidx, w.tab, w.slot, vrow, vstep);
  } else {
    hipLaunchKernelGGL(k_ds_insert<false>, dim3(nb), dim3(256), 0, stream, n, d_in, d_var, voxel_size, w.tab, w.cap - 1, w.slot, vrow, vstep);
  }
  if (mode == 2) {
    hipLaunchKernelGGL(k_ds_close_min, dim3(nb), dim3(256), 0, stream, n, d_in, w.tab, w.slot, w.dist);
    hipLaunchKernelGGL(k_ds_close_arg, dim3(nb), dim3(256), 0, stream, n, w.tab, w.slot, w.dist);
  }
  hipLaunchKernelGGL(k_ds_count, dim3(nb), dim3(256), 0, stream, n, w.tab, w.slot, w.blk);
  hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(256), 0, stream, nb, w.blk, w.n_out);
  return VBA_OK;
}
// mode 0 down_sampling_voxel, 1 down_sampling_pvec (var in, vout out), 2 down_sampling_close (first_out = chosen indices)
static int ds_common(vba_ctx *c, int mode, int n, const double *pnt, const double *var, double voxel_size, double *pnt_out, double *vout, int *count_out,
                     int *first_out, int *n_out) {
  if (n < 0 || !n_out || (n > 0 && (!pnt || !first_out)) || (mode != 2 && n > 0 && (!pnt_out || !count_out)) || (mode == 1 && n > 0 && (!var || !vout)))
    return VBA_ERR_BAD_ARG;
  *n_out = 0;
  if (n == 0) return VBA_OK;
  if (voxel_size < 0.001 && mode != 1) {                                // TL:203 / TL:242: the cloud is left untouched
    if (pnt_out) HIPCHK(c, hipMemcpyAsync(pnt_out, pnt, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    std::vector<int> z(n, 0), id(n);
    for (int i = 0; i < n; i++) id[i] = i;
    if (count_out) HIPCHK(c, hipMemcpyAsync(count_out, z.data(), (size_t)n * sizeof(int), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(first_out, id.data(), (size_t)n * sizeof(int), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = n;
    return VBA_OK;
  }
  int cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  const int nb = (n + 255) / 256;
  const bool det = c->opt.deterministic != 0;
  unsigned int key_bits = 1;
  while ((1u << key_bits) < (unsigned)cap) key_bits++;
  size_t b_sort = 0;   // deterministic mode: sorted slot keys, index values in / out, rocPRIM scratch
  if (det) {
    size_t tmp = 0;
    HIPCHK(c, sort_pairs_u32(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, (size_t)n, key_bits, c->stream));
    b_sort = 3 * ((((size_t)n * sizeof(int)) + 15) & ~(size_t)15) + ((tmp + 255) & ~(size_t)255);
  }
  const size_t b_tab = (size_t)cap * sizeof(DsSlot), b_pnt = (size_t)n * 3 * sizeof(double), b_i = (((size_t)n * sizeof(int)) + 15) & ~(size_t)15,
               b_blk = (((size_t)nb + 1) * sizeof(int) + 15) & ~(size_t)15, b_var = mode == 1 ? (size_t)n * 9 * sizeof(double) : 0,
               b_dist = mode == 2 ? (size_t)n * sizeof(double) : 0;
  int st = ensure_stage(c, b_tab + 3 * b_pnt + b_var + b_dist + 3 * b_i + b_blk + 64 + b_sort + 256);
  if (st) return st;
  char *base = (char *)c->d_stage;
  DsSlot *tab = (DsSlot *)base;
  double *d_in = (double *)(base + b_tab), *d_out = (double *)(base + b_tab + b_pnt), *d_vout = (double *)(base + b_tab + 2 * b_pnt),
         *d_var = (double *)(base + b_tab + 3 * b_pnt), *d_dist = (double *)(base + b_tab + 3 * b_pnt + b_var);
  int *d_slot = (int *)(base + b_tab + 3 * b_pnt + b_var + b_dist), *d_cnt = (int *)((char *)d_slot + b_i), *d_first = (int *)((char *)d_cnt + b_i),
      *d_blk = (int *)((char *)d_first + b_i), *d_n = d_blk + nb;
  HIPCHK(c, hipMemcpyAsync(d_in, pnt, b_pnt, hipMemcpyDefault, c->stream));
  if (mode == 1) HIPCHK(c, hipMemcpyAsync(d_var, var, b_var, hipMemcpyDefault, c->stream));
  TimedSpan sp{};
  span_begin(c, "downsample", sp);
  DsWork w{};
  w.tab = tab; w.cap = cap; w.key_bits = key_bits; w.slot = d_slot; w.blk = d_blk; w.n_out = d_n; w.dist = d_dist;
  if (det) {
    char *sb = (char *)(((uintptr_t)((char *)d_n + 64) + 255) & ~(uintptr_t)255);
    w.skey = (unsigned int *)sb; w.idx = (int *)(sb + b_i); w.sidx = (int *)(sb + 2 * b_i);
    w.tmp = sb + 3 * b_i; w.tmp_bytes = b_sort - 3 * b_i;
  }
  st = ds_core(c, c->stream, mode, n, d_in, mode == 1 ? d_var : nullptr, 9, 4, voxel_size, det, w);
  if (st) return st;
  hipLaunchKernelGGL(k_ds_emit, dim3(nb), dim3(256), 0, c->stream, n, tab, d_slot, d_blk, d_out, d_cnt, d_first, d_vout, mode);
  span_end(c, "downsample", sp);
  HIPCHK(c, hipGetLastError());
  int m = 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(&m, d_n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (m > 0) {
    if (pnt_out) HIPCHK(c, hipMemcpyAsync(pnt_out, d_out, (size_t)m * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    if (count_out) HIPCHK(c, hipMemcpyAsync(count_out, d_cnt, (size_t)m * sizeof(int), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(first_out, d_first, (size_t)m * sizeof(int), hipMemcpyDefault, c->stream));
    if (mode == 1) HIPCHK(c, hipMemcpyAsync(vout, d_vout, (size_t)m * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *n_out = m;
  return VBA_OK;
}
int vba_scan_down_sampling_voxel(vba_ctx *c, int n, const double *pnt, double voxel_size, double *pnt_out, int *count_out, int *first_out,
                                 int *n_out) {
  return ds_common(c, 0, n, pnt, nullptr, voxel_size, pnt_out, nullptr, count_out, first_out, n_out);
}
int vba_scan_down_sampling_pvec(vba_ctx *c, int n, const double *pnt, const double *var, double voxel_size, double *pnt_out, double *vardiag_out,
                                int *count_out, int *n_out) {
  std::vector<int> first(n > 0 ? n : 1);
  return ds_common(c, 1, n, pnt, var, voxel_size, pnt_out, vardiag_out, count_out, first.data(), n_out);
}
int vba_scan_down_sampling_close(vba_ctx *c, int n, const double *pnt, double voxel_size, int *index_out, int *n_out) {
  return ds_common(c, 2, n, pnt, nullptr, voxel_size, nullptr, nullptr, nullptr, index_out, n_out);
}
int vba_scan_undistort(vba_ctx *c, int n, double *pnt, const double *curv, int m, const double *imu_poses, const double *end_pose,
                       const double *ext_pose) {
  if (n < 0 || m < 0 || (n > 0 && (!pnt || !curv)) || (m > 0 && !imu_poses) || !end_pose || !ext_pose) return VBA_ERR_BAD_ARG;
  if (n == 0 || m == 0) return VBA_OK;
  const size_t nprm = (size_t)22 * m + 24;
  int st = ensure_stage(c, ((size_t)n * 4 + nprm) * sizeof(double));
  if (st) return st;
  double *d_p = (double *)c->d_stage, *d_c = d_p + (size_t)n * 3, *d_prm = d_c + n;
  std::vector<double> prm(nprm);
  std::memcpy(prm.data(), imu_poses, (size_t)22 * m * sizeof(double));
  std::memcpy(prm.data() + (size_t)22 * m, end_pose, 12 * sizeof(double));
  std::memcpy(prm.data() + (size_t)22 * m + 12, ext_pose, 12 * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(d_p, pnt, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_c, curv, (size_t)n * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_prm, prm.data(), nprm * sizeof(double), hipMemcpyHostToDevice, c->stream));
  TimedSpan sp{};
  span_begin(c, "undistort", sp);
  hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, d_p, d_c, m, d_prm);
  span_end(c, "undistort", sp);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(pnt, d_p, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // prm is a host temporary
  return VBA_OK;
}
int vba_map_cut_voxel_fix(vba_ctx *c, int n, const double *pnt_world, double jour) {
  return map_cut_voxel_fix(c->map, c->stream, n, pnt_world, jour, c->err);
}
int vba_map_recut(vba_ctx *c, int win_count, const double *poses, int multi) {
  int nf = 0;
  TimedSpan sp{};
  span_begin(c, "recut", sp);
  int st = map_recut(c->map, c->stream, win_count, poses, multi != 0, c->err, &nf);
  if (st) return st;
  // tras_opt: the map writes the planar leaves straight into the SoA factor store (no host round trip)
  c->nvox = 0;
  st = factor_reserve(c, nf > 0 ? nf : 1);
  if (st) return st;
  st = map_extract_factors(c->map, c->stream, c->fv, c->err, &nf);
  factor_update_mask(c, 0, nf);
  span_end(c, "recut", sp);
  if (st) return st;
  c->nvox = nf;
  return VBA_OK;
}
int vba_map_margi(vba_ctx *c, int win_count, const double *poses, double jour) {
  TimedSpan s{};
  span_begin(c, "margi", s);
  const int st = map_margi(c->map, c->stream, win_count, poses, jour, c->fv, c->nvox, c->err);
  span_end(c, "margi", s);
  return st;
}
int vba_map_slide(vba_ctx *c, int mgsize) { return map_slide(c->map, mgsize); }
int vba_map_prune(vba_ctx *c, double jour, int dist) { return map_prune(c->map, c->stream, jour, dist, c->err); }
int vba_map_reset(vba_ctx *c) { return map_reset(c->map, c->stream, c->err); }
int vba_map_num_roots(vba_ctx *c) { return map_num_roots(c->map, c->stream, false); }
int vba_map_num_slide_roots(vba_ctx *c) { return map_num_roots(c->map, c->stream, true); }
int vba_map_stats(vba_ctx *c, long long *out8) { return out8 ? map_stats(c->map, c->stream, out8, c->err) : VBA_ERR_BAD_ARG; }
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
  if (need > c->init_bytes) {
    if (c->d_init) hipFree(c->d_init);
    c->d_init = nullptr; c->init_bytes = 0;
    HIPCHK(c, hipMalloc(&c->d_init, need));
    c->init_bytes = need;
  }
  char *base = (char *)c->d_init;
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

// ---------------------------------------------------------------- odometry scan-to-map (VS:962-1098)
int vba_odom_lio_state_estimation(vba_ctx *c, int n, const double *pnt_body, const double *var_body, double *state, double *cov, int *ok) {
  if (n < 0 || (n > 0 && (!pnt_body || !var_body)) || !state || !cov) return VBA_ERR_BAD_ARG;
  const int DIM = VBA_DIM;
  // stage the scan once: [pts n*3 | var n*9 | partial nb*34 | out 34]
  const int nb = (n + 255) / 256;
  const size_t bytes = ((size_t)n * 12 + (size_t)nb * 34 + 64) * sizeof(double);
  int st = ensure_stage(c, bytes);
  if (st) return st;
  double *d_pts = (double *)c->d_stage, *d_var = d_pts + (size_t)n * 3, *d_part = d_var + (size_t)n * 9, *d_o34 = d_part + (size_t)nb * 34;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(d_pts, pnt_body, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_var, var_body, (size_t)n * 9 * sizeof(double), hipMemcpyDefault, c->stream));
  }
  vbh::State x_curr, x_prop;
  std::memcpy(&x_curr, state, sizeof(x_curr));
  x_prop = x_curr;                                                         // VS:965
  std::vector<double> P(cov, cov + 225), cov_inv(225);
  vbh::inverse_pplu(P.data(), cov_inv.data(), DIM);                        // VS:987
  const int num_max_iter = 4;
  int rematch_num = 0;
  double nnt[9] = {0};
  double G[225];
  for (int iter = 0; iter < num_max_iter; iter++) {
    OdomState X;
    std::memcpy(X.R, x_curr.R, sizeof(X.R)); std::memcpy(X.t, x_curr.p, sizeof(X.t));
    for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) { X.rot_var[3 * r + k] = P[r * DIM + k]; X.tsl_var[3 * r + k] = P[(3 + r) * DIM + 3 + k]; }   // VS:1000-1001
    double s34[34];
    if (n > 0) { st = map_odom_accumulate(c->map, c->stream, X, n, d_pts, d_var, d_part, d_o34, s34, c->err); if (st) return st; }
    else std::memset(s34, 0, sizeof(s34));
    double HTH[36], HTz[6];
    { int idx = 0; for (int r = 0; r < 6; r++) for (int k = r; k < 6; k++) { HTH[r * 6 + k] = s34[idx]; HTH[k * 6 + r] = s34[idx]; idx++; } }
    for (int r = 0; r < 6; r++) HTz[r] = s34[21 + r];
    nnt[0] = s34[27]; nnt[1] = nnt[3] = s34[28]; nnt[2] = nnt[6] = s34[29]; nnt[4] = s34[30]; nnt[5] = nnt[7] = s34[31]; nnt[8] = s34[32];
    // K_1 = (H_T_H + cov_inv)^-1 ; G(:,0:6) = K_1(:,0:6) HTH ; solution = K_1(:,0:6) HTz + vec - G(:,0:6) vec(0:6)      VS:1056-1060
    std::vector<double> A(cov_inv), K1(225);
    for (int r = 0; r < 6; r++) for (int k = 0; k < 6; k++) A[r * DIM + k] += HTH[r * 6 + k];
    vbh::inverse_pplu(A.data(), K1.data(), DIM);
    std::memset(G, 0, sizeof(G));
    for (int r = 0; r < DIM; r++)
      for (int k = 0; k < 6; k++) { double sacc = 0; for (int j = 0; j < 6; j++) sacc += K1[r * DIM + j] * HTH[j * 6 + k]; G[r * DIM + k] = sacc; }
    double vec[15], RtR[9], lg[3];
    vbh::m3_Tmul(x_curr.R, x_prop.R, RtR);                                 // x_prop - x_curr: Log(b.R^T this.R)  TL:164-173
    vbh::so3_log(RtR, lg);
    for (int k = 0; k < 3; k++) { vec[k] = lg[k]; vec[3 + k] = x_prop.p[k] - x_curr.p[k]; vec[6 + k] = x_prop.v[k] - x_curr.v[k]; vec[9 + k] = x_prop.bg[k] - x_curr.bg[k]; vec[12 + k] = x_prop.ba[k] - x_curr.ba[k]; }
    double sol[15];
    for (int r = 0; r < DIM; r++) {
      double a = 0, b = 0;
      for (int j = 0; j < 6; j++) { a += K1[r * DIM + j] * HTz[j]; b += G[r * DIM + j] * vec[j]; }
      sol[r] = a + vec[r] - b;
    }
    double E[9], Rn[9];                                                    // x_curr += solution  TL:154-162
    vbh::so3_exp(sol, E);
    vbh::m3_mul(x_curr.R, E, Rn);
    std::memcpy(x_curr.R, Rn, sizeof(Rn));
    for (int k = 0; k < 3; k++) { x_curr.p[k] += sol[3 + k]; x_curr.v[k] += sol[6 + k]; x_curr.bg[k] += sol[9 + k]; x_curr.ba[k] += sol[12 + k]; }
    const double rot_add = vbh::norm3(sol), tra_add = vbh::norm3(sol + 3);
    const bool converged = (rot_add * 57.3 < 0.01) && (tra_add * 100 < 0.015);     // VS:1072
    if (converged || ((rematch_num == 0) && (iter == num_max_iter - 2))) rematch_num++;   // VS:1076-1079
    if (rematch_num >= 2 || (iter == num_max_iter - 1)) {                  // x_curr.cov = (I - G) cov   VS:1082-1086
      std::vector<double> IG(225), Pn(225);
      for (int r = 0; r < DIM; r++) for (int k = 0; k < DIM; k++) IG[r * DIM + k] = (r == k ? 1.0 : 0.0) - G[r * DIM + k];
      vbh::mat_mul(IG.data(), P.data(), Pn.data(), DIM, DIM, DIM);
      P = Pn;
      break;
    }
  }
  std::memcpy(state, &x_curr, sizeof(x_curr));
  std::memcpy(cov, P.data(), 225 * sizeof(double));
  if (ok) {
    // SelfAdjointEigenSolver(nnt).eigenvalues()[0] < 14 -> false  (VS:1090-1097); closed form is not needed here: Jacobi on host
    double a[3][3] = {{nnt[0], nnt[1], nnt[2]}, {nnt[3], nnt[4], nnt[5]}, {nnt[6], nnt[7], nnt[8]}};
    for (int sweep = 0; sweep < 60; sweep++) {
      const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
      if (off == 0.0) break;
      for (int p = 0; p < 2; p++)
        for (int q = p + 1; q < 3; q++) {
          if (a[p][q] == 0.0) continue;
          const double theta = 0.5 * (a[q][q] - a[p][p]) / a[p][q];
          double t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
          if (theta < 0) t = -t;
          const double cth = 1.0 / std::sqrt(1 + t * t), sth = t * cth, apq = a[p][q];
          const int r = 3 - p - q;
          const double arp = a[r][p], arq = a[r][q];
          a[p][p] -= t * apq; a[q][q] += t * apq; a[p][q] = a[q][p] = 0.0;
          a[r][p] = a[p][r] = cth * arp - sth * arq; a[r][q] = a[q][r] = sth * arp + cth * arq;
          if (std::fabs(a[r][p]) < 1e-300) a[r][p] = a[p][r] = 0.0;
          if (std::fabs(a[r][q]) < 1e-300) a[r][q] = a[q][r] = 0.0;
        }
      if (off < 1e-14 * (std::fabs(a[0][0]) + std::fabs(a[1][1]) + std::fabs(a[2][2]))) break;
    }
    const double emin = std::min(a[0][0], std::min(a[1][1], a[2][2]));
    *ok = (emin < 14) ? 0 : 1;
  }
  return VBA_OK;
}

int vba_map_dump_leaves(vba_ctx *c, double *out, int max_leaves) { return map_dump_leaves(c->map, c->stream, out, max_leaves, c->err); }
int vba_map_dump_plane_var(vba_ctx *c, double *out, int max_leaves) { return map_dump_plane_var(c->map, c->stream, out, max_leaves, c->err); }

// ---------------------------------------------------------------- session-store formats (vba_io.hpp), host only
int vba_io_save_pcd(const char *path, int n, const double *xyz) {
  if (!path || n < 0 || (n > 0 && !xyz)) return VBA_ERR_BAD_ARG;
  FILE *f = std::fopen(path, "wb");
  if (!f) return VBA_ERR_IO;
  std::fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                  "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n", n, n);
  std::vector<float> rec((size_t)n * 4);
  for (int i = 0; i < n; i++) {                                // save_pcd sets x, y, z only: intensity keeps PointXYZI's default 0 (VS:170-176)
    rec[4 * (size_t)i] = (float)xyz[3 * (size_t)i]; rec[4 * (size_t)i + 1] = (float)xyz[3 * (size_t)i + 1];
    rec[4 * (size_t)i + 2] = (float)xyz[3 * (size_t)i + 2]; rec[4 * (size_t)i + 3] = 0.f;
  }
  const size_t w = n > 0 ? std::fwrite(rec.data(), 16, (size_t)n, f) : 0;
  const int bad = std::fclose(f);
  return (w == (size_t)n && !bad) ? VBA_OK : VBA_ERR_IO;
}

int vba_io_load_pcd(const char *path, int cap, double *xyz, double *intensity, int *n_out) {
  if (!path || !n_out || cap < 0 || (cap > 0 && !xyz)) return VBA_ERR_BAD_ARG;
  *n_out = 0;
  FILE *f = std::fopen(path, "rb");
  if (!f) return VBA_ERR_IO;
  struct Close { FILE *f; ~Close() { std::fclose(f); } } closer{f};
  vba_io::PcdHeader h;
  char line[1024];
  while (h.data.empty()) {
    if (!std::fgets(line, sizeof(line), f)) return VBA_ERR_IO;
    std::istringstream ss(line);
    std::string key, tok;
    if (!(ss >> key) || key[0] == '#') continue;
    if (key == "FIELDS" || key == "COLUMNS") while (ss >> tok) h.fields.push_back(tok);
    else if (key == "SIZE") while (ss >> tok) h.size.push_back(std::atoi(tok.c_str()));
    else if (key == "TYPE") while (ss >> tok) h.type.push_back(tok);
    else if (key == "COUNT") while (ss >> tok) h.count.push_back(std::atoi(tok.c_str()));
    else if (key == "WIDTH") ss >> h.width;
    else if (key == "HEIGHT") ss >> h.height;
    else if (key == "POINTS") ss >> h.points;
    else if (key == "DATA") ss >> h.data;
  }
  const size_t nf = h.fields.size();
  if (nf == 0 || h.size.size() != nf || h.type.size() != nf) return VBA_ERR_IO;
  if (h.count.empty()) h.count.assign(nf, 1);
  if (h.count.size() != nf) return VBA_ERR_IO;
  if (h.points < 0) h.points = h.width * h.height;
  if (h.points < 0) return VBA_ERR_IO;
  int fx = -1, fy = -1, fz = -1, fi = -1;
  std::vector<size_t> off(nf);
  size_t stride = 0;
  for (size_t k = 0; k < nf; k++) {
    off[k] = stride; stride += (size_t)h.size[k] * (size_t)h.count[k];
    if (h.fields[k] == "x") fx = (int)k; else if (h.fields[k] == "y") fy = (int)k; else if (h.fields[k] == "z") fz = (int)k;
    else if (h.fields[k] == "intensity") fi = (int)k;
  }
  if (fx < 0 || fy < 0 || fz < 0) return VBA_ERR_IO;
  *n_out = (int)h.points;
  if (h.points > cap) return VBA_ERR_CAPACITY;                 // *n_out tells the caller what to allocate
  auto scalar = [&](const unsigned char *p, size_t k) -> double {
    const char t = h.type[k][0]; const int sz = h.size[k];
    if (t == 'F') { if (sz == 4) { float v; std::memcpy(&v, p, 4); return v; } if (sz == 8) { double v; std::memcpy(&v, p, 8); return v; } }
    if (t == 'U') { uint64_t v = 0; std::memcpy(&v, p, (size_t)sz); return (double)v; }              // little endian
    if (t == 'I') { int64_t v = 0; std::memcpy(&v, p, (size_t)sz); const int sh = 64 - 8 * sz; return (double)((v << sh) >> sh); }
    return 0.0;
  };
  if (h.data == "binary") {
    std::vector<unsigned char> buf((size_t)h.points * stride);
    if (h.points > 0 && std::fread(buf.data(), stride, (size_t)h.points, f) != (size_t)h.points) return VBA_ERR_IO;
    for (long i = 0; i < h.points; i++) {
      const unsigned char *r = buf.data() + (size_t)i * stride;
      xyz[3 * i] = scalar(r + off[fx], fx); xyz[3 * i + 1] = scalar(r + off[fy], fy); xyz[3 * i + 2] = scalar(r + off[fz], fz);
      if (intensity) intensity[i] = fi >= 0 ? scalar(r + off[fi], fi) : 0.0;
    }
  } else if (h.data == "ascii") {
    for (long i = 0; i < h.points; i++) {
      if (!std::fgets(line, sizeof(line), f)) return VBA_ERR_IO;
      std::istringstream ss(line);
      if (intensity) intensity[i] = 0.0;
      for (size_t k = 0; k < nf; k++)
        for (int cidx = 0; cidx < h.count[k]; cidx++) {
          double v;
          if (!(ss >> v)) return VBA_ERR_IO;
          if (cidx) continue;
          if ((int)k == fx) xyz[3 * i] = v; else if ((int)k == fy) xyz[3 * i + 1] = v; else if ((int)k == fz) xyz[3 * i + 2] = v;
          else if ((int)k == fi && intensity) intensity[i] = v;
        }
    }
  } else {
    return VBA_ERR_IO;                                          // binary_compressed: never written by the reference (VS:178)
  }
  return VBA_OK;
}

int vba_io_save_pose(const char *path, int n, const double *states, const double *v6) {
  if (!path || n < 0 || (n > 0 && (!states || !v6))) return VBA_ERR_BAD_ARG;
  if (n < 100) return VBA_OK;                                   // VS:183-184: short sessions are not saved
  FILE *f = std::fopen(path, "w");
  if (!f) return VBA_ERR_IO;
  for (int i = 0; i < n; i++) {
    vbh::State x;
    std::memcpy(&x, states + (size_t)i * 25, sizeof(x));
    double q[4];
    vba_io::quat_from_rot(x.R, q);
    std::fprintf(f, "%.6f ", x.t);                              // fixed, precision 6; then precision 7 for the rest (VS:192-193)
    std::fprintf(f, "%.7f %.7f %.7f ", x.p[0], x.p[1], x.p[2]);
    std::fprintf(f, "%.7f %.7f %.7f %.7f", q[0], q[1], q[2], q[3]);
    const double *grp[4] = {x.v, x.bg, x.ba, x.g};
    for (int g = 0; g < 4; g++) std::fprintf(f, " %.7f %.7f %.7f", grp[g][0], grp[g][1], grp[g][2]);
    for (int j = 0; j < 6; j++) std::fprintf(f, " %.7f", v6[(size_t)i * 6 + j]);
    std::fprintf(f, "\n");
  }
  return std::fclose(f) ? VBA_ERR_IO : VBA_OK;
}

int vba_io_read_lidarstate(const char *path, int cap, double *states, double *v6, int *n_out) {
  if (!path || !n_out || cap < 0 || (cap > 0 && !states)) return VBA_ERR_BAD_ARG;
  *n_out = 0;
  FILE *f = std::fopen(path, "r");
  if (!f) return VBA_ERR_IO;                                    // the reference prints "not found" and exits (VH:271-275)
  struct Close { FILE *f; ~Close() { std::fclose(f); } } closer{f};
  std::vector<char> line(1 << 16);
  int n = 0;
  while (std::fgets(line.data(), (int)line.size(), f)) {
    std::vector<double> nums;
    char *p = line.data();
    for (;;) {
      char *e = nullptr;
      const double v = std::strtod(p, &e);
      if (e == p) break;
      nums.push_back(v); p = e;
    }
    if (nums.size() < 8) { if (nums.empty()) continue; return VBA_ERR_IO; }
    if (n < cap) {
      vbh::State x;
      std::memset(&x, 0, sizeof(x));
      x.g[2] = -9.8;                                            // lines without g: the reference leaves IMUST::g unset (TL:188-197); gravity here
      x.t = nums[0];
      for (int k = 0; k < 3; k++) x.p[k] = nums[1 + k];
      const double q[4] = {nums[4], nums[5], nums[6], nums[7]};
      vba_io::rot_from_quat(q, x.R);
      if (nums.size() >= 20)
        for (int k = 0; k < 3; k++) { x.v[k] = nums[8 + k]; x.bg[k] = nums[11 + k]; x.ba[k] = nums[14 + k]; x.g[k] = nums[17 + k]; }
      std::memcpy(states + (size_t)n * 25, &x, sizeof(x));
      if (v6) for (int k = 0; k < 6; k++) v6[(size_t)n * 6 + k] = nums.size() >= 26 ? nums[20 + k] : 0.0;
    }
    n++;
  }
  *n_out = n;
  return n > cap ? VBA_ERR_CAPACITY : VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ loop retrieval (vba_btc_*)
struct vba_btc_db {
  vba_ctx *ctx = nullptr;
  vba_btc_config cfg{};
  int nstd = 0, cap = 0;                     // descriptors stored / capacity (rows)
  BtcStds d{};
  std::vector<int> tab;                      // host mirror of the cell table, 8 ints per slot (vba_kernels_btc.hpp)
  int tab_mask = 0, ncell = 0;
  int *d_tab = nullptr;
  int nchunk = 0, chunk_cap = 0;
  int *d_ent = nullptr, *d_next = nullptr;
  std::vector<int> off{0}, seq;              // plane clouds: point offsets, header.seq
  float *d_pc = nullptr; size_t pc_cap = 0;
  int *d_off = nullptr; int off_cap = 0;
  int mcap = 0; int *d_m = nullptr;          // match list and per-candidate pair lists: mq | md | mf | pq | pd, mcap each
  int vcap = 0; int *d_votes = nullptr;
  int *d_cand = nullptr, *d_total = nullptr; double *d_cres = nullptr, *d_res = nullptr, *h_res = nullptr;
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

namespace {

// the "loop" timing span of one call, closed on every return path
struct BtcSpan {
  vba_ctx *c; TimedSpan s{}; bool open = true;
  explicit BtcSpan(vba_ctx *cc) : c(cc) { span_begin(c, "loop", s); }
  void end() { if (open) span_end(c, "loop", s); open = false; }
  ~BtcSpan() { end(); }
};

// grow a device array to new_n elements, keeping the first keep elements (stream-ordered copy; the old block is freed after it)
template <class T>
int btc_grow(vba_ctx *c, T **p, size_t keep, size_t new_n) {
  T *q = nullptr;
  HIPCHK(c, hipMalloc((void **)&q, new_n * sizeof(T)));
  if (*p && keep) HIPCHK(c, hipMemcpyAsync(q, *p, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
  if (*p) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipFree(*p); }
  *p = q;
  return VBA_OK;
}

int btc_reserve_rows(vba_btc_db *db, int need) {
  if (need <= db->cap) return VBA_OK;
  vba_ctx *c = db->ctx;
  int nc = db->cap ? db->cap : 1024;
  while (nc < need) nc *= 2;
  const size_t k = (size_t)db->nstd;
  int st;
  if ((st = btc_grow(c, &db->d.tri, 3 * k, 3 * (size_t)nc)) || (st = btc_grow(c, &db->d.cen, 3 * k, 3 * (size_t)nc)) ||
      (st = btc_grow(c, &db->d.loc, 9 * k, 9 * (size_t)nc)) || (st = btc_grow(c, &db->d.bits, 3 * k, 3 * (size_t)nc)) ||
      (st = btc_grow(c, &db->d.summ, 3 * k, 3 * (size_t)nc)) || (st = btc_grow(c, &db->d.frame, k, (size_t)nc)))
    return st;
  db->cap = nc;
  return VBA_OK;
}

// row checks shared by add_stds and the query: summaries are unsigned chars, masks fit occupy_len
int btc_check_rows(int n, const double *rows, const uint64_t *bits, int occupy_len) {
  const uint64_t mask = occupy_len >= 64 ? ~0ull : ((1ull << occupy_len) - 1ull);
  for (int i = 0; i < n; i++) {
    const double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    if (!(r[6] == std::floor(r[6]) && std::fabs(r[6]) < 2147483647.0)) return VBA_ERR_BAD_ARG;
    for (int k = 16; k < 19; k++) if (!(r[k] >= 0 && r[k] <= 255 && r[k] == std::floor(r[k]))) return VBA_ERR_BAD_ARG;
    for (int k = 0; k < 3; k++) if (bits[3 * (size_t)i + k] & ~mask) return VBA_ERR_BAD_ARG;
    for (int k = 0; k < 3; k++) if (!(std::fabs(r[k]) < 1e9)) return VBA_ERR_BAD_ARG;    // (int) of the cell key must be defined
  }
  return VBA_OK;
}

// rows -> SoA block [tri 3n | cen 3n | loc 9n | bits 3n | summ 3n | frame n] (host), and the views of the same block on the device
size_t btc_pack_bytes(int n) { return (size_t)n * (15 * sizeof(double) + 3 * sizeof(unsigned long long) + 4 * sizeof(int)); }
void btc_pack(int n, const double *rows, const uint64_t *bits, char *h) {
  double *tri = (double *)h, *cen = tri + 3 * (size_t)n, *loc = cen + 3 * (size_t)n;
  unsigned long long *bb = (unsigned long long *)(loc + 9 * (size_t)n);
  int *summ = (int *)(bb + 3 * (size_t)n), *frame = summ + 3 * (size_t)n;
  for (int i = 0; i < n; i++) {
    const double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    for (int k = 0; k < 3; k++) { tri[3 * i + k] = r[k]; cen[3 * i + k] = r[3 + k]; summ[3 * i + k] = (int)r[16 + k]; bb[3 * i + k] = bits[3 * (size_t)i + k]; }
    for (int k = 0; k < 9; k++) loc[9 * i + k] = r[7 + k];
    frame[i] = (int)r[6];
  }
}
BtcStds btc_view(int n, char *dev) {
  BtcStds v;
  v.tri = (double *)dev; v.cen = v.tri + 3 * (size_t)n; v.loc = v.cen + 3 * (size_t)n;
  v.bits = (unsigned long long *)(v.loc + 9 * (size_t)n);
  v.summ = (int *)(v.bits + 3 * (size_t)n); v.frame = v.summ + 3 * (size_t)n;
  return v;
}

int btc_table_upload(vba_btc_db *db) {
  vba_ctx *c = db->ctx;
  if (db->d_tab) hipFree(db->d_tab);
  db->d_tab = nullptr;
  HIPCHK(c, hipMalloc((void **)&db->d_tab, db->tab.size() * sizeof(int)));
  HIPCHK(c, hipMemcpyAsync(db->d_tab, db->tab.data(), db->tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return VBA_OK;
}
int btc_table_find(const std::vector<int> &tab, int mask, int x, int y, int z, bool &fresh) {
  unsigned s = btc_hash(x, y, z) & (unsigned)mask;
  for (;;) {
    const int *e = tab.data() + 8 * (size_t)s;
    if (e[3] < 0) { fresh = true; return (int)s; }
    if (e[0] == x && e[1] == y && e[2] == z) { fresh = false; return (int)s; }
    s = (s + 1) & (unsigned)mask;
  }
}
void btc_table_init(std::vector<int> &tab, int slots) {
  tab.assign((size_t)slots * 8, 0);
  for (int s = 0; s < slots; s++) { tab[8 * (size_t)s + 3] = -1; tab[8 * (size_t)s + 5] = -1; }
}

// the host table into `slots` slots (a power of two), entries re-probed in slot order; the caller uploads it
void btc_rehash(vba_btc_db *db, int slots) {
  std::vector<int> nt;
  btc_table_init(nt, slots);
  for (int u = 0; u <= db->tab_mask; u++) {
    const int *e = db->tab.data() + 8 * (size_t)u;
    if (e[3] < 0) continue;
    bool f2;
    const int t = btc_table_find(nt, slots - 1, e[0], e[1], e[2], f2);
    std::memcpy(nt.data() + 8 * (size_t)t, e, 8 * sizeof(int));
  }
  db->tab.swap(nt);
  db->tab_mask = slots - 1;
}

// one search of db, enqueued: counts, scan, ranked match list + votes, candidate list, verification, choice, result -> h_res
int btc_enqueue(vba_btc_db *db, const BtcStds &q, int n, const float *pl, int npl) {
  vba_ctx *c = db->ctx;
  const int nf = (int)db->off.size() - 1, G = 27 * n, nb = (G + 3) / 4;
  const BtcCfgDev cf = db->dev_cfg();
  const BtcIndex ix = db->index();
  int *mq = db->d_m, *md = mq + db->mcap, *mf = md + db->mcap, *pq = mf + db->mcap, *pd = pq + db->mcap;
  if (nf > 0) HIPCHK(c, hipMemsetAsync(db->d_votes, 0, (size_t)nf * sizeof(int), c->stream));
  k_btc_match<true><<<nb, 256, 0, c->stream>>>(n, q, db->d, ix, cf, c->d_btccnt, db->d_total, db->mcap, mq, md, mf, db->d_votes);
  k_det_scan<<<1, 1024, 0, c->stream>>>(c->d_btccnt, G, db->d_total, -1, 0, 0);
  k_btc_match<false><<<nb, 256, 0, c->stream>>>(n, q, db->d, ix, cf, c->d_btccnt, db->d_total, db->mcap, mq, md, mf, db->d_votes);
  k_btc_select<<<1, 256, 0, c->stream>>>(nf, db->cfg.candidate_num, db->mcap, db->d_total, db->d_votes, db->d_cand, db->d_res);
  k_btc_verify<<<db->cfg.candidate_num, 256, 0, c->stream>>>(q, db->d, cf, db->d_total, db->mcap, mq, md, mf, pq, pd, db->d_cand, db->d_res,
                                                             db->d_cres, pl, npl, db->d_pc, db->d_off);
  k_btc_final<<<1, 64, 0, c->stream>>>(cf, db->d_cand, db->d_cres, db->d_res);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(db->h_res, db->d_res, BTC_RES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return VBA_OK;
}

void btc_result(const vba_btc_db *db, vba_btc_result *r) {
  const double *h = db->h_res;
  r->loop_id = (int)h[0]; r->score = h[1];
  for (int k = 0; k < 3; k++) r->t[k] = h[2 + k];
  for (int k = 0; k < 9; k++) r->R[k] = h[5 + k];
}

int btc_search_run(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur, int cur_frame,
                   vba_btc_result *results);
int btc_search(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur, int cur_frame,
               vba_btc_result *results) {
  if (n_db < 0 || (n_db > 0 && (!dbs || !results)) || n < 0 || (n > 0 && (!rows || !bits)) || !cur) return VBA_ERR_BAD_ARG;
  if (n_db == 0) return VBA_OK;
  vba_ctx *c = dbs[0]->ctx;
  for (int k = 0; k < n_db; k++) if (!dbs[k] || dbs[k]->ctx != c) return VBA_ERR_BAD_ARG;
  if (cur->ctx != c || cur_frame < 0 || cur_frame >= (int)cur->off.size() - 1) return VBA_ERR_BAD_ARG;
  for (int k = 0; k < n_db; k++) { const int st = btc_check_rows(n, rows, bits, dbs[k]->cfg.occupy_len); if (st) return st; }
  if (n == 0) {                                                   // BTC.cpp:210-214
    for (int k = 0; k < n_db; k++) { results[k] = vba_btc_result{}; results[k].loop_id = -1; dbs[k]->have_search = false; }
    return VBA_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  BtcSpan sp(c);
  return btc_search_run(n_db, dbs, n, rows, bits, cur, cur_frame, results);
}

int btc_search_run(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur, int cur_frame,
                   vba_btc_result *results) {
  vba_ctx *c = dbs[0]->ctx;
  // query upload (once) and the shared count scratch
  const size_t qb = btc_pack_bytes(n);
  if (qb > c->btcq_bytes) {
    if (c->d_btcq) hipFree(c->d_btcq);
    if (c->h_btcq) hipHostFree(c->h_btcq);
    c->d_btcq = c->h_btcq = nullptr; c->btcq_bytes = 0;
    size_t nbytes = 1 << 16;
    while (nbytes < qb) nbytes *= 2;
    HIPCHK(c, hipMalloc((void **)&c->d_btcq, nbytes));
    HIPCHK(c, hipHostMalloc((void **)&c->h_btcq, nbytes, hipHostMallocDefault));
    c->btcq_bytes = nbytes;
  }
  if ((size_t)27 * n > c->btccnt_cap) {
    if (c->d_btccnt) hipFree(c->d_btccnt);
    c->d_btccnt = nullptr;
    size_t m = 8192;
    while (m < (size_t)27 * n) m *= 2;
    HIPCHK(c, hipMalloc((void **)&c->d_btccnt, m * sizeof(int)));
    c->btccnt_cap = m;
  }
  for (int k = 0; k < n_db; k++) {                                // votes sized by the frames pushed so far
    vba_btc_db *db = dbs[k];
    const int nf = (int)db->off.size() - 1;
    if (nf > db->vcap) {
      int m = db->vcap ? db->vcap : 1024;
      while (m < nf) m *= 2;
      const int st = btc_grow(c, &db->d_votes, 0, (size_t)m);
      if (st) return st;
      db->vcap = m;
    }
  }
  btc_pack(n, rows, bits, c->h_btcq);
  HIPCHK(c, hipMemcpyAsync(c->d_btcq, c->h_btcq, qb, hipMemcpyHostToDevice, c->stream));
  const BtcStds q = btc_view(n, c->d_btcq);
  const int plo = cur->off[cur_frame], npl = cur->off[cur_frame + 1] - plo;
  const float *pl = cur->d_pc ? cur->d_pc + 6 * (size_t)plo : nullptr;
  for (int k = 0; k < n_db; k++) { const int st = btc_enqueue(dbs[k], q, n, pl, npl); if (st) return st; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // a match list that did not fit: grow it and search that database again (amortised: the list only grows)
  for (int k = 0; k < n_db; k++) {
    vba_btc_db *db = dbs[k];
    const double total = db->h_res[15];
    if (total > db->mcap) {
      int m = db->mcap;
      while (m < total) m *= 2;
      int st = btc_grow(c, &db->d_m, 0, 5 * (size_t)m);
      if (st) return st;
      db->mcap = m;
      if ((st = btc_enqueue(db, q, n, pl, npl))) return st;
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    db->have_search = true;
    btc_result(db, &results[k]);
  }
  return VBA_OK;
}

}  // namespace

extern "C" {

int vba_btc_default_config(int is_high_fly, vba_btc_config *f) {   // BTC.cpp:3-68
  if (!f) return VBA_ERR_BAD_ARG;
  std::memset(f, 0, sizeof(*f));
  f->skip_near_num = 30;
  f->candidate_num = is_high_fly ? 100 : 20;
  f->rough_dis_threshold = 0.01f;
  f->similarity_threshold = is_high_fly ? 0.5f : 0.7f;
  f->icp_threshold = 0.15f;
  f->normal_threshold = 0.2f;
  f->dis_threshold = 0.5f;
  f->occupy_len = 50;   // (proj_dis_max_ - proj_dis_min_) / proj_image_high_inc_: 5 / 0.1 and 10 / 0.2
  return VBA_OK;
}

int vba_btc_create(vba_ctx *c, const vba_btc_config *cfg, vba_btc_db **out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VBA_ERR_NO_DEVICE;
  if (!c || !cfg || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->occupy_len < 0 || cfg->occupy_len > 64 || cfg->candidate_num < 1 || cfg->candidate_num > BTC_MAX_CAND) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  vba_btc_db *db = new vba_btc_db();
  db->ctx = c; db->cfg = *cfg;
  vba_btc_default_gen_config(0, &db->gcfg);
  btc_table_init(db->tab, 1024);
  db->tab_mask = 1023;
  int st = btc_table_upload(db);
  if (!st) st = btc_reserve_rows(db, 1024);
  if (!st) st = btc_grow(c, &db->d_off, 0, 1024);
  if (!st) st = btc_grow(c, &db->d_ent, 0, (size_t)256 * BTC_CHUNK);
  if (!st) st = btc_grow(c, &db->d_next, 0, 256);
  if (!st) st = btc_grow(c, &db->d_m, 0, 5 * (size_t)65536);
  if (!st) st = btc_grow(c, &db->d_votes, 0, 1024);
  if (!st) st = btc_grow(c, &db->d_cand, 0, 5 * (size_t)BTC_MAX_CAND);
  if (!st) st = btc_grow(c, &db->d_total, 0, 4);
  if (!st) st = btc_grow(c, &db->d_cres, 0, 13 * (size_t)BTC_MAX_CAND);
  if (!st) st = btc_grow(c, &db->d_res, 0, BTC_RES);
  if (!st && hipHostMalloc((void **)&db->h_res, BTC_RES * sizeof(double), hipHostMallocDefault) != hipSuccess) st = VBA_ERR_HIP;
  if (st) { vba_btc_destroy(db); return st; }
  db->off_cap = 1024; db->chunk_cap = 256; db->mcap = 65536; db->vcap = 1024;
  const int zero = 0;
  hipMemcpyAsync(db->d_off, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess) { vba_btc_destroy(db); return VBA_ERR_HIP; }
  *out = db;
  return VBA_OK;
}

void vba_btc_destroy(vba_btc_db *db) {
  if (!db) return;
  vba_ctx *c = db->ctx;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  void *p[] = {db->d.tri, db->d.cen, db->d.loc, db->d.bits, db->d.summ, db->d.frame, db->d_tab, db->d_ent, db->d_next, db->d_pc, db->d_off,
               db->d_m, db->d_votes, db->d_cand, db->d_total, db->d_cres, db->d_res};
  for (void *q : p) if (q) hipFree(q);
  if (db->h_res) hipHostFree(db->h_res);
  if (db->gen) { btcgen_free(*db->gen); delete db->gen; }
  delete db;
}

int vba_btc_reserve(vba_btc_db *db, int stds, int frames, int64_t cloud_points, int matches) {
  if (!db || stds < 0 || frames < 0 || cloud_points < 0 || matches < 0 || stds > (1 << 29) || frames > (1 << 29) || matches > (1 << 28))
    return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if ((st = btc_reserve_rows(db, stds))) return st;
  int slots = db->tab_mask + 1;                               // cells <= descriptors, load factor <= 1/2
  while (slots < 2 * stds) slots *= 2;
  if (slots > db->tab_mask + 1) { btc_rehash(db, slots); if ((st = btc_table_upload(db))) return st; }
  if (stds > db->chunk_cap) {                                 // chunks <= descriptors
    int m = db->chunk_cap;
    while (m < stds) m *= 2;
    if ((st = btc_grow(c, &db->d_ent, (size_t)db->nchunk * BTC_CHUNK, (size_t)m * BTC_CHUNK)) || (st = btc_grow(c, &db->d_next, (size_t)db->nchunk, (size_t)m)))
      return st;
    db->chunk_cap = m;
  }
  if (frames + 1 > db->off_cap) {
    int m = db->off_cap;
    while (m < frames + 1) m *= 2;
    if ((st = btc_grow(c, &db->d_off, db->off.size(), (size_t)m))) return st;
    db->off_cap = m;
  }
  if (frames > db->vcap) {
    int m = db->vcap;
    while (m < frames) m *= 2;
    if ((st = btc_grow(c, &db->d_votes, 0, (size_t)m))) return st;
    db->vcap = m;
  }
  if ((size_t)cloud_points > db->pc_cap) {
    size_t m = db->pc_cap ? db->pc_cap : 65536;
    while (m < (size_t)cloud_points) m *= 2;
    if ((st = btc_grow(c, &db->d_pc, 6 * (size_t)db->off.back(), 6 * m))) return st;
    db->pc_cap = m;
  }
  if (matches > db->mcap) {
    int m = db->mcap;
    while (m < matches) m *= 2;
    if ((st = btc_grow(c, &db->d_m, 0, 5 * (size_t)m))) return st;
    db->mcap = m;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_set_skip_near_num(vba_btc_db *db, int v) { if (!db) return VBA_ERR_BAD_ARG; db->cfg.skip_near_num = v; return VBA_OK; }
int vba_btc_num_frames(vba_btc_db *db) { return db ? (int)db->off.size() - 1 : -1; }
int vba_btc_frame_seq(vba_btc_db *db, int frame, int *seq) {
  if (!db || !seq || frame < 0 || frame >= (int)db->seq.size()) return VBA_ERR_BAD_ARG;
  *seq = db->seq[frame];
  return VBA_OK;
}

int vba_btc_push_plane_cloud(vba_btc_db *db, int n, const float *xyz_normal, int seq) {
  if (!db || n < 0 || (n > 0 && !xyz_normal)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t have = (size_t)db->off.back(), need = have + (size_t)n;
  if (need > db->pc_cap) {
    size_t m = db->pc_cap ? db->pc_cap : 65536;
    while (m < need) m *= 2;
    const int st = btc_grow(c, &db->d_pc, 6 * have, 6 * m);
    if (st) return st;
    db->pc_cap = m;
  }
  const int nf = (int)db->off.size();        // frames after this push + 1 offsets
  if (nf + 1 > db->off_cap) {
    int m = db->off_cap * 2;
    while (m < nf + 1) m *= 2;
    const int st = btc_grow(c, &db->d_off, (size_t)nf, (size_t)m);
    if (st) return st;
    db->off_cap = m;
  }
  if (need > (size_t)INT32_MAX) return VBA_ERR_CAPACITY;
  db->off.push_back((int)need);
  db->seq.push_back(seq);
  if (n) HIPCHK(c, hipMemcpyAsync(db->d_pc + 6 * have, xyz_normal, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d_off + nf, &db->off.back(), sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_add_stds(vba_btc_db *db, int n, const double *rows, const uint64_t *bits) {   // BTC.cpp:258-277
  if (!db || n < 0 || (n > 0 && (!rows || !bits))) return VBA_ERR_BAD_ARG;
  if (n == 0) { db->n_add++; return VBA_OK; }
  vba_ctx *c = db->ctx;
  int st = btc_check_rows(n, rows, bits, db->cfg.occupy_len);
  if (st) return st;
  const int nf = (int)db->off.size() - 1;
  for (int i = 0; i < n; i++) { const double f = rows[(size_t)i * VBA_BTC_ROW_LEN + 6]; if (f < 0 || f >= nf) return VBA_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = btc_reserve_rows(db, db->nstd + n))) return st;
  // rows -> SoA at [nstd, nstd + n)
  std::vector<char> h(btc_pack_bytes(n));
  btc_pack(n, rows, bits, h.data());
  const BtcStds v = btc_view(n, h.data());
  const size_t k = (size_t)db->nstd;
  HIPCHK(c, hipMemcpyAsync(db->d.tri + 3 * k, v.tri, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.cen + 3 * k, v.cen, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.loc + 9 * k, v.loc, 9 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.bits + 3 * k, v.bits, 3 * (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.summ + 3 * k, v.summ, 3 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.frame + k, v.frame, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  // cell index: STD_LOC = (int)(triangle_ + 0.5) (BTC.cpp:263-266); each cell's chunks list its descriptors in insertion order
  std::vector<int> ent, nxt, slots;          // (position, value) pairs and the touched table slots
  bool rehash = false;
  for (int i = 0; i < n; i++) {
    const double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    const int x = (int)(r[0] + 0.5), y = (int)(r[1] + 0.5), z = (int)(r[2] + 0.5);
    bool fresh;
    int s = btc_table_find(db->tab, db->tab_mask, x, y, z, fresh);
    if (fresh && 2 * (db->ncell + 1) > db->tab_mask + 1) {     // keep the load factor <= 1/2: rehash into twice the slots
      btc_rehash(db, 2 * (db->tab_mask + 1));
      rehash = true;
      slots.clear();
      s = btc_table_find(db->tab, db->tab_mask, x, y, z, fresh);
    }
    int *e = db->tab.data() + 8 * (size_t)s;
    if (fresh) { e[0] = x; e[1] = y; e[2] = z; e[3] = -1; e[4] = 0; e[5] = -1; db->ncell++; }
    if (e[4] % BTC_CHUNK == 0) {                                // a new chunk for this cell
      if (db->nchunk + 1 > db->chunk_cap) {
        const int m = db->chunk_cap * 2;
        if ((st = btc_grow(c, &db->d_ent, (size_t)db->nchunk * BTC_CHUNK, (size_t)m * BTC_CHUNK)) || (st = btc_grow(c, &db->d_next, (size_t)db->nchunk, (size_t)m)))
          return st;
        db->chunk_cap = m;
      }
      const int ch = db->nchunk++;
      if (e[5] >= 0) { nxt.push_back(e[5]); nxt.push_back(ch); }
      else e[3] = ch;
      nxt.push_back(ch); nxt.push_back(-1);
      e[5] = ch;
    }
    ent.push_back(e[5] * BTC_CHUNK + e[4] % BTC_CHUNK); ent.push_back(db->nstd + i);
    e[4]++;
    if (!rehash) slots.push_back(s);
  }
  db->nstd += n;
  // a chunk opened and then linked in the same batch appears twice in nxt ((ch, -1), later (ch, ch2)): keep the LAST value per
  // position, so every position is written once by the scatter (two writes to one address in one launch have no order)
  {
    std::map<int, int> last;
    for (size_t u = 0; u < nxt.size(); u += 2) last[nxt[u]] = nxt[u + 1];
    nxt.clear();
    for (const auto &kv : last) { nxt.push_back(kv.first); nxt.push_back(kv.second); }
  }
  // one upload of the (position, value) pairs, three scatters; the table goes whole after a rehash
  std::vector<int> tp;
  if (!rehash) {
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    for (int s : slots) for (int u = 0; u < 8; u++) { tp.push_back(8 * s + u); tp.push_back(db->tab[8 * (size_t)s + u]); }
  } else if ((st = btc_table_upload(db))) return st;
  std::vector<int> all;
  all.insert(all.end(), ent.begin(), ent.end());
  all.insert(all.end(), nxt.begin(), nxt.end());
  all.insert(all.end(), tp.begin(), tp.end());
  if ((st = ensure_stage(c, all.size() * sizeof(int)))) return st;
  int *ds = (int *)c->d_stage;
  HIPCHK(c, hipMemcpyAsync(ds, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  const int ne = (int)ent.size() / 2, nn = (int)nxt.size() / 2, nt = (int)tp.size() / 2;
  if (ne) k_btc_scatter<<<(ne + 255) / 256, 256, 0, c->stream>>>(ne, ds, db->d_ent);
  if (nn) k_btc_scatter<<<(nn + 255) / 256, 256, 0, c->stream>>>(nn, ds + 2 * ne, db->d_next);
  if (nt) k_btc_scatter<<<(nt + 255) / 256, 256, 0, c->stream>>>(nt, ds + 2 * (ne + nn), db->d_tab);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->n_add++;
  return VBA_OK;
}

int vba_btc_search_loop(vba_btc_db *db, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur_db, int cur_frame,
                        vba_btc_result *result) {
  if (!db || !result) return VBA_ERR_BAD_ARG;
  vba_btc_db *dbs[1] = {db};
  return btc_search(1, dbs, n, rows, bits, cur_db, cur_frame, result);
}

int vba_btc_search_loop_sessions(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits,
                                 const vba_btc_db *cur_db, int cur_frame, vba_btc_result *results) {
  return btc_search(n_db, dbs, n, rows, bits, cur_db, cur_frame, results);
}

int vba_btc_last_candidates(vba_btc_db *db, int cap, vba_btc_candidate *out, int *n) {
  if (!db || !n || cap < 0 || (cap > 0 && !out)) return VBA_ERR_BAD_ARG;
  *n = 0;
  if (!db->have_search) return VBA_OK;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const int nc = (int)db->h_res[14];
  *n = nc;
  const int m = nc < cap ? nc : cap;
  if (m == 0) return VBA_OK;
  std::vector<int> ci(5 * (size_t)m);
  std::vector<double> cr(13 * (size_t)m);
  HIPCHK(c, hipMemcpyAsync(ci.data(), db->d_cand, ci.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cr.data(), db->d_cres, cr.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < m; k++) {
    out[k].frame = ci[5 * k]; out[k].votes = ci[5 * k + 1]; out[k].match_len = ci[5 * k + 1];
    out[k].max_vote_index = ci[5 * k + 3]; out[k].max_vote = ci[5 * k + 4]; out[k].score = cr[13 * k];
  }
  return VBA_OK;
}

int vba_btc_icp_normal(vba_btc_db *src_db, int src_frame, vba_btc_db *tar_db, int tar_frame, double *t, double *R, double icp_eigval,
                       int *ok, double *eig, int *iters) {   // loop_refine.hpp:47-139
  if (!src_db || !tar_db || !t || !R || src_db->ctx != tar_db->ctx) return VBA_ERR_BAD_ARG;
  if (src_frame < 0 || src_frame >= (int)src_db->off.size() - 1 || tar_frame < 0 || tar_frame >= (int)tar_db->off.size() - 1) return VBA_ERR_BAD_ARG;
  vba_ctx *c = src_db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const int ns = src_db->off[src_frame + 1] - src_db->off[src_frame], nt = tar_db->off[tar_frame + 1] - tar_db->off[tar_frame];
  const float *src = src_db->d_pc ? src_db->d_pc + 6 * (size_t)src_db->off[src_frame] : nullptr;
  const float *tar = tar_db->d_pc ? tar_db->d_pc + 6 * (size_t)tar_db->off[tar_frame] : nullptr;
  const int nb = ns > 0 ? (ns + 255) / 256 : 1, ntile = (nt + 255) / 256;
  int slices = 1;
  while (slices < ntile && nb * slices * 2 <= 1024) slices *= 2;          // ~1024 workgroups on the 1-NN pass
  if (slices > ntile && ntile > 0) slices = ntile;
  if (!c->d_icp) {
    HIPCHK(c, hipMalloc((void **)&c->d_icp, sizeof(BtcIcpDev)));
    HIPCHK(c, hipHostMalloc((void **)&c->h_icp, sizeof(BtcIcpDev), hipHostMallocDefault));
  }
  if ((size_t)slices * ns > c->icpkey_cap) {
    size_t m = 65536;
    while (m < (size_t)slices * ns) m *= 2;
    const int st = btc_grow(c, &c->d_icpkey, 0, m);
    if (st) return st;
    c->icpkey_cap = m;
  }
  if ((size_t)nb * BTC_ICP_PART > c->icppart_cap) {
    size_t m = 4096;
    while (m < (size_t)nb * BTC_ICP_PART) m *= 2;
    const int st = btc_grow(c, &c->d_icppart, 0, m);
    if (st) return st;
    c->icppart_cap = m;
  }
  BtcSpan sp(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));       // (the pinned state block may still be in flight from an earlier call)
  BtcIcpDev *h = c->h_icp;
  std::memset(h, 0, sizeof(*h));
  for (int k = 0; k < 9; k++) h->R[k] = R[k];
  for (int k = 0; k < 3; k++) h->t[k] = t[k];
  h->paras[0] = 0.2; h->paras[1] = 0.2; h->paras[2] = 0.5; h->paras[3] = 3;
  HIPCHK(c, hipMemcpyAsync(c->d_icp, h, sizeof(*h), hipMemcpyHostToDevice, c->stream));
  for (int it = 0; it < 20; it++) {                  // launches after convergence return at once (BtcIcpDev::done)
    k_btc_icp_nn<<<dim3(nb, slices), 256, 0, c->stream>>>(ns, src, nt, tar, c->d_icp, c->d_icpkey);
    k_btc_icp_accum<<<nb, 256, 0, c->stream>>>(ns, src, tar, slices, c->d_icpkey, c->d_icp, c->d_icppart);
    k_btc_icp_step<<<1, 64, 0, c->stream>>>(nb, c->d_icppart, c->d_icp);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h, c->d_icp, sizeof(*h), hipMemcpyDeviceToHost, c->stream));
  sp.end();
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 9; k++) R[k] = h->R[k];
  for (int k = 0; k < 3; k++) t[k] = h->t[k];
  if (eig) for (int k = 0; k < 3; k++) eig[k] = h->eig[k];
  if (iters) *iters = h->iters;
  if (ok) *ok = (h->eig[0] > icp_eigval && h->is_conv == 1) ? 1 : 0;
  return VBA_OK;
}


// ------------------------------------------------------------------------------------------------ descriptor generation
int vba_btc_default_gen_config(int is_high_fly, vba_btc_gen_config *f) {   // BTC.cpp:3-68
  if (!f) return VBA_ERR_BAD_ARG;
  std::memset(f, 0, sizeof(*f));
  f->useful_corner_num = is_high_fly ? 200 : 100;
  f->plane_merge_normal_thre = is_high_fly ? 0.3f : 0.1f;
  f->plane_merge_dis_thre = is_high_fly ? 0.6f : 0.3f;
  f->plane_detection_thre = is_high_fly ? 0.05f : 0.01f;
  f->voxel_size = is_high_fly ? 2.0f : 1.0f;
  f->voxel_init_num = 10;
  f->proj_plane_num = is_high_fly ? 1 : 2;
  f->proj_image_resolution = 0.5f;
  f->proj_image_high_inc = is_high_fly ? 0.2f : 0.1f;
  f->proj_dis_min = 0.0f;
  f->proj_dis_max = is_high_fly ? 10.0f : 5.0f;
  f->summary_min_thre = is_high_fly ? 6.0f : 10.0f;
  f->line_filter_enable = is_high_fly ? 0 : 1;
  f->touch_filter_enable = 0;
  f->descriptor_near_num = 15.0f;
  f->descriptor_min_len = is_high_fly ? 3.0f : 2.0f;
  f->descriptor_max_len = 50.0f;
  f->non_max_suppression_radius = is_high_fly ? 3.0f : 2.0f;
  f->std_side_resolution = 0.2f;
  return VBA_OK;
}

namespace {
// cut_num of extract_binary: (int)((proj_dis_max_ - proj_dis_min_) / proj_image_high_inc_), the float fields promoted to double
int btc_cut_num(const vba_btc_gen_config &g) {
  return (int)(((double)g.proj_dis_max - (double)g.proj_dis_min) / (double)g.proj_image_high_inc);
}
size_t btc_max_stds(const vba_btc_gen_config &g) {      // useful_corner_num * C(K - 1, 2)
  const size_t K1 = (size_t)((int)g.descriptor_near_num - 1);
  return (size_t)g.useful_corner_num * (K1 * (K1 - 1) / 2);
}
BgCfg btc_bg_cfg(const vba_btc_gen_config &g) {
  BgCfg f;
  f.useful = g.useful_corner_num; f.vinit = g.voxel_init_num; f.proj_num = g.proj_plane_num; f.line_filter = g.line_filter_enable;
  f.touch_filter = g.touch_filter_enable; f.K = (int)g.descriptor_near_num; f.cut_num = btc_cut_num(g);
  f.merge_n = g.plane_merge_normal_thre; f.merge_d = g.plane_merge_dis_thre; f.detect = g.plane_detection_thre; f.vsize = g.voxel_size;
  f.res = g.proj_image_resolution; f.high_inc = g.proj_image_high_inc; f.dmin = g.proj_dis_min; f.dmax = g.proj_dis_max;
  f.summ_min = g.summary_min_thre; f.min_len = g.descriptor_min_len; f.max_len = g.descriptor_max_len;
  f.scale = 1.0 / (double)g.std_side_resolution;
  const double r = g.non_max_suppression_radius;
  f.nms_r2 = (float)(r * r);
  return f;
}
int btc_gen_check(const vba_btc_gen_config &g) {
  const int K = (int)g.descriptor_near_num;
  if (!(g.useful_corner_num >= 1 && g.voxel_size > 0 && g.voxel_init_num >= 0 && g.proj_plane_num >= 1 && g.proj_plane_num <= BG_MAX_PROJ &&
        g.proj_image_resolution > 0 && g.proj_image_high_inc > 0 && g.descriptor_near_num >= 3 && K <= BG_MAX_K &&
        g.descriptor_min_len >= 0 && g.descriptor_max_len <= 2000 && g.std_side_resolution > 0 && g.proj_dis_max >= g.proj_dis_min &&
        btc_cut_num(g) >= 0 && btc_cut_num(g) <= 64 && btc_max_stds(g) < (size_t)(1 << 26)))
    return VBA_ERR_BAD_ARG;
  return VBA_OK;
}
int btc_gen_ensure(vba_btc_db *db, int64_t points, int64_t cells, size_t corners) {
  vba_ctx *c = db->ctx;
  if (!db->gen) db->gen = new BtcGen();
  const BtcGen &g = *db->gen;
  const size_t stds = btc_max_stds(db->gcfg);
  if ((size_t)points <= g.pts_cap && (size_t)cells <= g.cell_cap && corners <= g.corn_cap && stds <= g.cand_cap &&
      g.pts_cap / (size_t)(db->gcfg.voxel_init_num + 1) + 1 <= g.plane_cap && g.cnt)
    return VBA_OK;
  HIPCHK(c, btcgen_reserve(*db->gen, (size_t)points, (size_t)cells, corners, stds, db->gcfg.voxel_init_num, c->stream));
  return VBA_OK;
}
}  // namespace

int vba_btc_set_gen_config(vba_btc_db *db, const vba_btc_gen_config *cfg) {
  if (!db || !cfg || btc_gen_check(*cfg)) return VBA_ERR_BAD_ARG;
  db->gcfg = *cfg;
  return VBA_OK;
}

int vba_btc_get_gen_config(const vba_btc_db *db, vba_btc_gen_config *cfg) {
  if (!db || !cfg) return VBA_ERR_BAD_ARG;
  *cfg = db->gcfg;
  return VBA_OK;
}

int vba_btc_gen_reserve(vba_btc_db *db, int64_t points, int64_t cells, int frames) {
  if (!db || points < 0 || cells < 0 || frames < 0 || points > (1 << 28) || cells > BG_MAX_CELLS || frames > (1 << 20)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if ((st = btc_gen_ensure(db, points, cells, 0))) return st;
  // plane-cloud room for `frames` more calls at the bound a call reserves (points / (voxel_init_num + 1) + 1 planes each)
  const int64_t planes = (int64_t)(points / (db->gcfg.voxel_init_num + 1) + 1) * frames;
  if ((st = vba_btc_reserve(db, 0, (int)db->off.size() - 1 + frames + 1, (int64_t)db->off.back() + planes, 0))) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_gen_allocations(vba_btc_db *db, int *count, int64_t *bytes) {
  if (!db || !count || !bytes) return VBA_ERR_BAD_ARG;
  *count = db->gen ? db->gen->allocs : 0;
  *bytes = db->gen ? (int64_t)db->gen->dev_bytes : 0;
  return VBA_OK;
}

// the argument checks of vba_btc_generate_stds that do not concern the cloud itself (no side effect)
static int btc_generate_check(vba_btc_db *db, int n, int cap, double *rows, uint64_t *bits, int *n_stds) {
  if (!db || n < 0 || n > (1 << 28) || !n_stds || cap < 0 || (cap > 0 && (!rows || !bits))) return VBA_ERR_BAD_ARG;
  const vba_btc_gen_config &g = db->gcfg;
  if ((size_t)cap < btc_max_stds(g) || btc_cut_num(g) > db->cfg.occupy_len) return VBA_ERR_BAD_ARG;
  return VBA_OK;
}
// GenerateSTDescs on a cloud from host memory (xyz) or from the device: with xyz == nullptr and n > 0 the caller has sized the
// generator for n points (btc_gen_ensure) and enqueued, ahead of the database's stream, the writes of float [n][3] into its point
// buffer db->gen->xyz; the generator only reads that buffer, so a second attempt after a buffer grew finds it intact
static int btc_generate_impl(vba_btc_db *db, int n, const float *xyz, int id, int cap, double *rows, uint64_t *bits, int *n_stds) {
  int chk = btc_generate_check(db, n, cap, rows, bits, n_stds);
  if (chk) return chk;
  const vba_btc_gen_config &g = db->gcfg;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  *n_stds = 0;
  if (n == 0) {                                 // empty cloud: an empty plane cloud, no corners, no descriptors
    db->last_loc.clear(); db->last_bits.clear();
    return vba_btc_push_plane_cloud(db, 0, nullptr, id);
  }
  BtcSpan sp(c);
  int st;
  const size_t planes = (size_t)n / (size_t)(g.voxel_init_num + 1) + 1;
  const size_t have = (size_t)db->off.back();
  if (have + planes > (size_t)INT32_MAX) return VBA_ERR_CAPACITY;
  if ((st = btc_gen_ensure(db, n, 0, 0))) return st;
  // room for this frame's plane cloud and offset (the same growth as vba_btc_push_plane_cloud), counted with the generator's own
  if (have + planes > db->pc_cap) {
    size_t m = db->pc_cap ? db->pc_cap : 65536;
    while (m < have + planes) m *= 2;
    if ((st = btc_grow(c, &db->d_pc, 6 * have, 6 * m))) return st;
    db->pc_cap = m;
    db->gen->allocs++;
  }
  const int nf = (int)db->off.size();
  if (nf + 1 > db->off_cap) {
    int m = db->off_cap * 2;
    while (m < nf + 1) m *= 2;
    if ((st = btc_grow(c, &db->d_off, (size_t)nf, (size_t)m))) return st;
    db->off_cap = m;
    db->gen->allocs++;
  }
  const BgCfg cf = btc_bg_cfg(g);
  // the image and the corner list grow on overflow and the call runs again (nothing is committed before it succeeds)
  for (int attempt = 0;; attempt++) {
    BtcGen &G = *db->gen;
    HIPCHK(c, btcgen_enqueue(G, cf, n, xyz, db->d_pc + 6 * have, db->d_off + nf, (int)have, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int *h = G.h_cnt;
    if (h[BGC_ERR] & 1) return VBA_ERR_BAD_ARG;
    if (h[BGC_ERR] & 4) return VBA_ERR_CAPACITY;           // a projection image above BG_MAX_CELLS: refused before allocating
    const bool cells_over = (h[BGC_ERR] & 2) != 0, corn_over = (size_t)h[BGC_NTEMP] > G.corn_cap;
    if (!cells_over && !corn_over) break;
    if (attempt >= 2) return VBA_ERR_CAPACITY;
    if ((st = btc_gen_ensure(db, n, cells_over ? (int64_t)h[BGC_CELLS] : 0, corn_over ? (size_t)h[BGC_NTEMP] : 0))) return st;
  }
  const BtcGen &G = *db->gen;
  const int np = G.h_cnt[BGC_NPL], ns = G.h_cnt[BGC_NSTD], nc = G.h_cnt[BGC_NCORN];
  db->off.push_back((int)(have + (size_t)np));
  db->seq.push_back(id);
  db->last_loc.resize(4 * (size_t)nc); db->last_bits.resize(nc);
  for (int i = 0; i < nc; i++) {
    const BgCorner &k = G.h_corn[i];
    for (int j = 0; j < 3; j++) db->last_loc[4 * (size_t)i + j] = k.loc[j];
    db->last_loc[4 * (size_t)i + 3] = (double)k.summ;
    db->last_bits[i] = k.bits;
  }
  // rows: [triangle center frame A.loc B.loc C.loc A.summ B.summ C.summ], masks of A, B, C
  for (int i = 0; i < ns; i++) {
    const BgStd &t = G.h_stds[i];
    double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    const int v[3] = {t.a, t.b, t.c};
    for (int j = 0; j < 3; j++) { r[j] = t.tri[j]; r[3 + j] = t.cen[j]; }
    r[6] = (double)db->n_add;
    for (int u = 0; u < 3; u++) {
      const BgCorner &k = G.h_corn[v[u]];
      for (int j = 0; j < 3; j++) r[7 + 3 * u + j] = k.loc[j];
      r[16 + u] = (double)k.summ;
      bits[3 * (size_t)i + u] = k.bits;
    }
  }
  *n_stds = ns;
  return VBA_OK;
}

int vba_btc_generate_stds(vba_btc_db *db, int n, const float *xyz, int id, int cap, double *rows, uint64_t *bits, int *n_stds) {
  if (n > 0 && !xyz) return VBA_ERR_BAD_ARG;
  return btc_generate_impl(db, n, xyz, id, cap, rows, bits, n_stds);
}

int vba_btc_plane_cloud(vba_btc_db *db, int frame, int cap, float *xyz_normal, int *n) {
  if (!db || !n || frame < 0 || frame >= (int)db->off.size() - 1 || cap < 0 || (cap > 0 && !xyz_normal)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const int b = db->off[frame], e = db->off[frame + 1];
  *n = e - b;
  const int w = (e - b) < cap ? (e - b) : cap;
  if (w > 0) HIPCHK(c, hipMemcpyAsync(xyz_normal, db->d_pc + 6 * (size_t)b, (size_t)w * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_last_corners(vba_btc_db *db, int cap, double *loc_summary, uint64_t *bits, int *n) {
  if (!db || !n || cap < 0 || (cap > 0 && (!loc_summary || !bits))) return VBA_ERR_BAD_ARG;
  const int k = (int)db->last_bits.size();
  *n = k;
  const int w = k < cap ? k : cap;
  for (int i = 0; i < w; i++) {
    for (int j = 0; j < 4; j++) loc_summary[4 * (size_t)i + j] = db->last_loc[4 * (size_t)i + j];
    bits[i] = db->last_bits[i];
  }
  return VBA_OK;
}

// ---------------------------------------------------------------- pose-graph optimisation (vba_kernels_pgo.hpp)
int vba_pgo_optimize(vba_ctx *c, int n, double *poses, int m, const double *edges, int n_prior, const double *priors, int n_updates,
                     double relin_threshold, double *stats) {
  if (!c || n < 1 || !poses || m < 0 || n_prior < 0 || (m > 0 && !edges) || (n_prior > 0 && !priors) || n_updates < 1 ||
      !(relin_threshold >= 0.0) || !std::isfinite(relin_threshold))
    return VBA_ERR_BAD_ARG;
  const int F = m + n_prior;
  // ---- validation and factor table (edges first, then priors)
  std::vector<int> fi(F), fj(F);
  std::vector<double> fz((size_t)F * 18);
  auto index_of = [n](double x, int &k) { if (!(x >= 0.0 && x < (double)n) || x != std::floor(x)) return false; k = (int)x; return true; };
  for (size_t q = 0; q < (size_t)n * 12; q++) if (!std::isfinite(poses[q])) return VBA_ERR_BAD_ARG;
  for (int f = 0; f < F; f++) {
    const bool pr = f >= m;
    const double *row = pr ? priors + (size_t)(f - m) * 19 : edges + (size_t)f * 20;
    const double *z = pr ? row + 1 : row + 2;
    int i, j = -1;
    if (!index_of(row[0], i) || (!pr && (!index_of(row[1], j) || i == j))) return VBA_ERR_BAD_ARG;
    for (int q = 0; q < 18; q++) {
      if (!std::isfinite(z[q]) || (q >= 12 && !(z[q] > 0.0))) return VBA_ERR_BAD_ARG;
      fz[(size_t)f * 18 + q] = q < 12 ? z[q] : 1.0 / z[q];
    }
    fi[f] = i; fj[f] = j;
  }
  // ---- distinct neighbour pairs, components, skeleton
  std::vector<long long> pk;
  pk.reserve(m);
  for (int f = 0; f < m; f++) pk.push_back((long long)std::min(fi[f], fj[f]) * n + std::max(fi[f], fj[f]));
  std::sort(pk.begin(), pk.end());
  pk.erase(std::unique(pk.begin(), pk.end()), pk.end());
  const int NPAIR = (int)pk.size(), NB = n + NPAIR;
  auto pair_block = [&](int a, int b) {   // block code of H(a, b): blk * 2 + transposed
    if (a == b) return 2 * a;
    const long long key = (long long)std::min(a, b) * n + std::max(a, b);
    const int p = (int)(std::lower_bound(pk.begin(), pk.end(), key) - pk.begin());
    return 2 * (n + p) + (a > b ? 1 : 0);
  };
  std::vector<int> nb_off(n + 1, 0), nb(2 * (size_t)NPAIR);
  for (long long key : pk) { nb_off[key / n + 1]++; nb_off[key % n + 1]++; }
  for (int k = 0; k < n; k++) nb_off[k + 1] += nb_off[k];
  {
    std::vector<int> fill(nb_off.begin(), nb_off.end() - 1);
    for (long long key : pk) { const int a = (int)(key / n), b = (int)(key % n); nb[fill[a]++] = b; nb[fill[b]++] = a; }
  }
  std::vector<int> uf(n);
  for (int k = 0; k < n; k++) uf[k] = k;
  std::function<int(int)> root = [&](int k) { while (uf[k] != k) { uf[k] = uf[uf[k]]; k = uf[k]; } return k; };
  for (long long key : pk) { const int a = root((int)(key / n)), b = root((int)(key % n)); if (a != b) uf[std::max(a, b)] = std::min(a, b); }
  std::vector<char> has_prior(n, 0), comp_prior(n, 0);
  for (int f = m; f < F; f++) has_prior[fi[f]] = 1;
  for (int k = 0; k < n; k++) if (has_prior[k]) comp_prior[root(k)] = 1;
  for (int k = 0; k < n; k++)
    if (!comp_prior[root(k)]) { c->set_error("vba_pgo_optimize: a connected component holds no prior"); return VBA_ERR_SINGULAR; }
  std::vector<int> node_skel(n, -1), skel_node;
  auto is_path = [&](int k) { return !has_prior[k] && nb_off[k + 1] - nb_off[k] <= 2; };
  for (int k = 0; k < n; k++) if (!is_path(k)) { node_skel[k] = (int)skel_node.size(); skel_node.push_back(k); }
  const int K = (int)skel_node.size();
  // ---- segments: maximal runs of path nodes, oriented so that a single attachment is B (eliminated towards it: no fill)
  std::vector<int> seg_off(1, 0), seg_nodes, seg_att, seg_ecode, seg_ccode;
  std::vector<char> seen(n, 0);
  for (int v0 = 0; v0 < n; v0++) {
    if (!is_path(v0) || seen[v0]) continue;
    int end = v0, prev = -1;                      // walk to one end of the run
    for (;;) {
      int nxt = -1;
      for (int e = nb_off[end]; e < nb_off[end + 1]; e++) if (nb[e] != prev && is_path(nb[e])) { nxt = nb[e]; break; }
      if (nxt < 0 || nxt == v0) break;            // (nxt == v0: a cycle of path nodes, impossible once every component has a prior)
      prev = end; end = nxt;
    }
    std::vector<int> run;
    prev = -1;
    for (int cur = end; cur >= 0;) {
      run.push_back(cur); seen[cur] = 1;
      int nxt = -1;
      for (int e = nb_off[cur]; e < nb_off[cur + 1]; e++) if (nb[e] != prev && is_path(nb[e]) && !seen[nb[e]]) { nxt = nb[e]; break; }
      prev = cur; cur = nxt;
    }
    const int L = (int)run.size();
    auto skel_nb = [&](int node, int other_path) {     // the skeleton neighbours of an end node (other than its run neighbour)
      std::vector<int> r;
      for (int e = nb_off[node]; e < nb_off[node + 1]; e++) if (nb[e] != other_path && !is_path(nb[e])) r.push_back(nb[e]);
      return r;
    };
    int A = -1, B = -1;
    if (L == 1) {
      std::vector<int> sn = skel_nb(run[0], -1);
      if (sn.size() == 2) { A = sn[0]; B = sn[1]; } else if (sn.size() == 1) B = sn[0];
    } else {
      std::vector<int> s0 = skel_nb(run[0], run[1]), s1 = skel_nb(run[L - 1], run[L - 2]);
      A = s0.empty() ? -1 : s0[0]; B = s1.empty() ? -1 : s1[0];
      if (B < 0) { std::reverse(run.begin(), run.end()); std::swap(A, B); }
    }
    if (B < 0) { c->set_error("vba_pgo_optimize: a chain without a skeleton node"); return VBA_ERR_SINGULAR; }
    for (int k = 0; k < L; k++) {
      seg_nodes.push_back(run[k]);
      seg_ccode.push_back(k + 1 < L ? pair_block(run[k], run[k + 1]) : pair_block(run[k], B));
    }
    seg_att.push_back(A >= 0 ? node_skel[A] : -1); seg_att.push_back(node_skel[B]);
    seg_ecode.push_back(A >= 0 ? pair_block(run[0], A) : -1);
    seg_off.push_back((int)seg_nodes.size());
  }
  const int S = (int)seg_off.size() - 1, LS = (int)seg_nodes.size();
  // ---- block CSR in factor order
  std::vector<int> blk_off(NB + 1, 0), blk_ent;
  auto pair_index = [&](int a, int b) { return pair_block(a, b) >> 1; };
  for (int f = 0; f < F; f++) { blk_off[fi[f] + 1]++; if (fj[f] >= 0) { blk_off[fj[f] + 1]++; blk_off[pair_index(fi[f], fj[f]) + 1]++; } }
  for (int b = 0; b < NB; b++) blk_off[b + 1] += blk_off[b];
  blk_ent.resize(blk_off[NB] > 0 ? blk_off[NB] : 1);
  {
    std::vector<int> fill(blk_off.begin(), blk_off.end() - 1);
    for (int f = 0; f < F; f++) {
      blk_ent[fill[fi[f]]++] = 4 * f + 0;
      if (fj[f] >= 0) {
        blk_ent[fill[fj[f]]++] = 4 * f + 1;
        blk_ent[fill[pair_index(fi[f], fj[f])]++] = 4 * f + (fi[f] < fj[f] ? 2 : 3);
      }
    }
  }
  // ---- skeleton blocks: diagonal, direct skeleton pairs, segment A-B pairs; CSR of segment contributions in segment order
  std::map<std::pair<int, int>, int> sbm;
  for (int p = 0; p < K; p++) sbm[{p, p}] = 0;
  for (long long key : pk) {
    const int a = node_skel[key / n], b = node_skel[key % n];
    if (a >= 0 && b >= 0) sbm[{std::max(a, b), std::min(a, b)}] = 0;
  }
  for (int s = 0; s < S; s++) { const int a = seg_att[2 * s], b = seg_att[2 * s + 1]; if (a >= 0 && a != b) sbm[{std::max(a, b), std::min(a, b)}] = 0; }
  const int NSB = (int)sbm.size();
  std::vector<int> sb_pq, sb_base;
  { int b = 0; for (auto &kv : sbm) { kv.second = b++; sb_pq.push_back(kv.first.first); sb_pq.push_back(kv.first.second);
      const int na = skel_node[kv.first.first], nbb = skel_node[kv.first.second];
      const long long key = (long long)std::min(na, nbb) * n + std::max(na, nbb);
      sb_base.push_back(na == nbb || std::binary_search(pk.begin(), pk.end(), key) ? pair_block(na, nbb) : -1); } }
  std::vector<std::vector<int>> sbl(NSB);
  for (int s = 0; s < S; s++) {
    const int a = seg_att[2 * s], b = seg_att[2 * s + 1];
    if (a >= 0) sbl[sbm[{a, a}]].push_back(4 * s + 0);
    sbl[sbm[{b, b}]].push_back(4 * s + 1);
    if (a >= 0) {
      if (a == b) { sbl[sbm[{a, a}]].push_back(4 * s + 2); sbl[sbm[{a, a}]].push_back(4 * s + 3); }
      else if (b > a) sbl[sbm[{b, a}]].push_back(4 * s + 2);    // rows B, columns A: S_BA
      else sbl[sbm[{a, b}]].push_back(4 * s + 3);               // rows A, columns B: S_BA^T
    }
  }
  std::vector<int> sb_off(1, 0), sb_ent;
  for (auto &l : sbl) { sb_ent.insert(sb_ent.end(), l.begin(), l.end()); sb_off.push_back((int)sb_ent.size()); }
  // ---- device memory: one grow-only arena for the structure and work areas, one for the dense skeleton system
  const int n6 = 6 * K, NP = (n6 + 7) / 8 * 8, ld = (NP + 63) / 64 * 64;
  size_t bytes = 0;
  auto take = [&](size_t b) { const size_t o = bytes; bytes += (b + 255) & ~(size_t)255; return o; };
  const int U = n_updates;
  const size_t o_theta = take((size_t)n * 96), o_fz = take((size_t)F * 144), o_fi = take((size_t)F * 4), o_fj = take((size_t)F * 4),
      o_slot = take((size_t)F * PGO_SLOT * 8), o_blk = take((size_t)NB * 288), o_g = take((size_t)n * 48),
      o_blkoff = take((size_t)(NB + 1) * 4), o_blkent = take(blk_ent.size() * 4), o_segoff = take(seg_off.size() * 4),
      o_segnodes = take((size_t)LS * 4), o_segatt = take((size_t)S * 8), o_sege = take((size_t)S * 4), o_segc = take((size_t)LS * 4),
      o_segY = take((size_t)LS * PGO_Y * 8), o_segout = take((size_t)S * PGO_SEGOUT * 8), o_skel = take((size_t)K * 4),
      o_sbpq = take((size_t)NSB * 8), o_sbbase = take((size_t)NSB * 4), o_sboff = take(sb_off.size() * 4), o_sbent = take(sb_ent.size() * 4),
      o_dx = take((size_t)n * 48), o_res = take((size_t)U * 24 + 8);   // cost[U] | mx[U] | cnt[U] | status
  HIPCHK(c, hipSetDevice(c->device));
  // grow-only buffers owned by the context; a size the device cannot hold is VBA_ERR_CAPACITY (the old buffer is released first)
  auto grow = [&](void **buf, size_t &have, size_t want, const char *what) -> int {
    if (want <= have) return VBA_OK;
    if (*buf) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(*buf)); *buf = nullptr; have = 0; }
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const hipError_t e = want > fr ? hipErrorOutOfMemory : hipMalloc(buf, want);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();                      // a refused allocation must not surface in a later call's error check
      *buf = nullptr;
      c->set_error(std::string("vba_pgo_optimize: the ") + what + " needs " + std::to_string(want) + " bytes, " + std::to_string(fr) + " free");
      return VBA_ERR_CAPACITY;
    }
    HIPCHK(c, e);
    have = want;
    return VBA_OK;
  };
  const size_t abytes = ((size_t)(NP + 1) * ld + (size_t)(NP + 1) * 8) * 8;
  if (int r = grow((void **)&c->d_pgo, c->pgo_bytes, bytes, "graph structure")) return r;
  if (int r = grow((void **)&c->d_pgoAb, c->pgoAb_bytes, abytes, "dense skeleton system (8 (6K)^2 bytes)")) return r;
  char *d = c->d_pgo;
  PgoView v{};
  v.n = n; v.F = F; v.NB = NB; v.S = S; v.K = K; v.NSB = NSB; v.U = U; v.NP = NP; v.ld = ld; v.thr = relin_threshold;
  v.theta = (double *)(d + o_theta); v.fz = (const double *)(d + o_fz); v.fi = (const int *)(d + o_fi); v.fj = (const int *)(d + o_fj);
  v.slot = (double *)(d + o_slot); v.blk = (double *)(d + o_blk); v.g = (double *)(d + o_g);
  v.blk_off = (const int *)(d + o_blkoff); v.blk_ent = (const int *)(d + o_blkent);
  v.seg_off = (const int *)(d + o_segoff); v.seg_nodes = (const int *)(d + o_segnodes); v.seg_att = (const int *)(d + o_segatt);
  v.seg_ecode = (const int *)(d + o_sege); v.seg_ccode = (const int *)(d + o_segc); v.segY = (double *)(d + o_segY);
  v.segout = (double *)(d + o_segout); v.skel_node = (const int *)(d + o_skel); v.sb_pq = (const int *)(d + o_sbpq);
  v.sb_base = (const int *)(d + o_sbbase); v.sb_off = (const int *)(d + o_sboff); v.sb_ent = (const int *)(d + o_sbent);
  v.Ab = c->d_pgoAb; v.Tb = c->d_pgoAb + (size_t)(NP + 1) * ld; v.dx = (double *)(d + o_dx);
  v.cost = (double *)(d + o_res); v.mx = (unsigned long long *)(d + o_res + (size_t)U * 8); v.cnt = (int *)(d + o_res + (size_t)U * 16);
  v.status = (int *)(d + o_res + (size_t)U * 20);
  hipStream_t st = c->stream;
  // the sources are pageable locals of this call: on a failed copy the stream is drained before they go out of scope
  hipError_t ue = hipSuccess;
  auto up = [&](size_t off, const void *src, size_t b) { if (ue == hipSuccess && b) ue = hipMemcpyAsync(d + off, src, b, hipMemcpyHostToDevice, st); };
  up(o_theta, poses, (size_t)n * 96);
  up(o_fz, fz.data(), fz.size() * 8); up(o_fi, fi.data(), (size_t)F * 4); up(o_fj, fj.data(), (size_t)F * 4);
  up(o_blkoff, blk_off.data(), blk_off.size() * 4); up(o_blkent, blk_ent.data(), blk_ent.size() * 4);
  up(o_segoff, seg_off.data(), seg_off.size() * 4); up(o_segnodes, seg_nodes.data(), (size_t)LS * 4);
  up(o_segatt, seg_att.data(), (size_t)S * 8); up(o_sege, seg_ecode.data(), (size_t)S * 4);
  up(o_segc, seg_ccode.data(), (size_t)LS * 4); up(o_skel, skel_node.data(), (size_t)K * 4);
  up(o_sbpq, sb_pq.data(), (size_t)NSB * 8); up(o_sbbase, sb_base.data(), (size_t)NSB * 4);
  up(o_sboff, sb_off.data(), sb_off.size() * 4); up(o_sbent, sb_ent.data(), sb_ent.size() * 4);
  if (ue != hipSuccess) { hipStreamSynchronize(st); HIPCHK(c, ue); }
  HIPCHK(c, hipMemsetAsync(d + o_res, 0, (size_t)U * 24 + 8, st));
  auto grid = [](long long cnt, int bs) { return dim3((unsigned)((cnt + bs - 1) / bs)); };
  TimedSpan sp;
  span_begin(c, "pgo", sp);
  for (int u = 0; u < U; u++) {
    if (F > 0) {
      hipLaunchKernelGGL(k_pgo_linearize, grid(F, 256), dim3(256), 0, st, v);
      hipLaunchKernelGGL(k_pgo_cost, dim3(1), dim3(256), 0, st, v, u);
    }
    hipLaunchKernelGGL(k_pgo_assemble, grid(NB, 256), dim3(256), 0, st, v);
    if (S > 0) hipLaunchKernelGGL(k_pgo_seg_elim, grid(S, 64), dim3(64), 0, st, v);
    hipLaunchKernelGGL(k_pgo_skel_fill, grid((long long)(NP + 1) * NP, 256), dim3(256), 0, st, v);
    hipLaunchKernelGGL(k_pgo_skel_scatter, grid(NSB, 256), dim3(256), 0, st, v);
    for (int k0 = 0; k0 < NP; k0 += 8) {
      hipLaunchKernelGGL(k_bigl_panel, dim3(1), dim3(256), 0, st, v.Ab, v.Tb, NP, ld, k0);
      const int kn = k0 + 8;
      const int nt = (NP + 1 - kn + 63) / 64;
      if (nt > 0) hipLaunchKernelGGL(k_bigl_update, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, v.Ab, v.Tb, NP, ld, k0);
    }
    hipLaunchKernelGGL(k_pgo_pivots, grid(n6, 256), dim3(256), 0, st, v);
    for (int lo = ((n6 - 1) / 64) * 64; lo >= 0; lo -= 64) {
      hipLaunchKernelGGL(k_bigl_bs_tri, dim3(1), dim3(64), 0, st, v.Ab, NP, ld, n6, lo);
      if (lo > 0) hipLaunchKernelGGL(k_bigl_bs_gemv, grid(lo, 256), dim3(256), 0, st, v.Ab, NP, ld, n6, lo);
    }
    hipLaunchKernelGGL(k_pgo_skel_dx, grid(K, 256), dim3(256), 0, st, v);
    if (S > 0) hipLaunchKernelGGL(k_pgo_seg_back, grid(S, 64), dim3(64), 0, st, v);
    hipLaunchKernelGGL(k_pgo_relin, grid(n, 256), dim3(256), 0, st, v, u);
  }
  span_end(c, "pgo", sp);
  HIPCHK(c, hipGetLastError());
  std::vector<double> out((size_t)n * 12);
  std::vector<char> res((size_t)U * 24 + 8);
  hipError_t de = hipMemcpyAsync(out.data(), v.theta, out.size() * 8, hipMemcpyDeviceToHost, st);
  if (de == hipSuccess) de = hipMemcpyAsync(res.data(), d + o_res, res.size(), hipMemcpyDeviceToHost, st);
  const hipError_t se = hipStreamSynchronize(st);   // always drained before out / res go out of scope
  HIPCHK(c, de);
  HIPCHK(c, se);
  int status;
  std::memcpy(&status, res.data() + (size_t)U * 20, 4);
  if (status == PGO_SINGULAR) { c->set_error("vba_pgo_optimize: non-positive or non-finite pivot"); return VBA_ERR_SINGULAR; }
  std::memcpy(poses, out.data(), out.size() * 8);
  if (stats)
    for (int u = 0; u < U; u++) {
      double cost, mx; int cnt;
      std::memcpy(&cost, res.data() + (size_t)u * 8, 8);
      std::memcpy(&mx, res.data() + (size_t)U * 8 + (size_t)u * 8, 8);
      std::memcpy(&cnt, res.data() + (size_t)U * 16 + (size_t)u * 4, 4);
      stats[3 * u] = cnt; stats[3 * u + 1] = cost; stats[3 * u + 2] = mx;
    }
  return VBA_OK;
}

// ---------------------------------------------------------------- diagnostic: one LM linear solve through the production kernels
// The caller's system is written into the buffers the solve kernel reads, in their production layout, and the kernel is launched
// as the LM loop launches it (lm_spec workgroups); every buffer belongs to this call, so the context's LM state is untouched.
extern "C++" {
namespace {
struct DbgBufs {                      // device buffers of one call; drained and freed on every exit path
  hipStream_t st;
  std::vector<void *> p;
  explicit DbgBufs(hipStream_t s) : st(s) {}
  ~DbgBufs() { if (!p.empty()) hipStreamSynchronize(st); for (void *q : p) hipFree(q); }
  template <typename T> hipError_t alloc(T **out, size_t count) {
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
    if (e == hipSuccess) { p.push_back(q); *out = (T *)q; }
    return e;
  }
};
// HessCfg2<W> tile image [tiles | E | g | r] of (H, g): E remainders zero, or (epack) each frame's 6 x 6 diagonal block held in E only
template <int W>
void dbg_lidar_image(const double *H, const double *g, bool epack, std::vector<double> &img) {
  using C2 = HessCfg2<W>;
  constexpr int n = 6 * W;
  img.assign(C2::NOUT2, 0.0);
  for (int row = 0; row < n; row++)
    for (int col = row; col < n; col++) {
      const double a = H[(size_t)row * n + col];
      const int e = tl_eidx<W>(row, col);
      if (epack && e >= 0) { img[e] = a; continue; }
      const int ta = row >> 4, tb = col >> 4, ut = ta * C2::NT16 - ta * (ta - 1) / 2 + (tb - ta);
      img[(size_t)ut * 256 + 16 * (row & 15) + (col & 15)] = a;
    }
  for (int k = 0; k < n; k++) img[C2::GB + k] = g[k];
}
template <int W>
int dbg_lidar(vba_ctx *c, DbgBufs &B, const double *H, const double *g, int flags, LmDev &h, double *d_dx) {
  using C2 = HessCfg2<W>;
  std::vector<double> img;
  dbg_lidar_image<W>(H, g, (flags & VBA_SOLVE_E_PACKED) != 0, img);
  const bool copy_raw = (flags & VBA_SOLVE_COPY_RAW) != 0, from_raw = copy_raw && (flags & VBA_SOLVE_FROM_RAW);
  double *red = nullptr, *raw = nullptr;
  LmDev *s = nullptr;
  HIPCHK(c, B.alloc(&red, C2::NOUT2)); HIPCHK(c, B.alloc(&raw, C2::NOUT2)); HIPCHK(c, B.alloc(&s, 1));
  h.is_calc_hess = from_raw ? 0 : 1;
  HIPCHK(c, hipMemsetAsync(red, 0, C2::NOUT2 * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(raw, 0, C2::NOUT2 * sizeof(double), c->stream));
  HIPCHK(c, hipMemcpyAsync(from_raw ? raw : red, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(s, &h, sizeof(LmDev), hipMemcpyHostToDevice, c->stream));
  if (copy_raw) hipLaunchKernelGGL((k_lm_solve_m<W, true>), dim3(c->lm_spec), dim3(256), 0, c->stream, s, red, raw, d_dx);
  else hipLaunchKernelGGL((k_lm_solve_m<W, false>), dim3(c->lm_spec), dim3(256), 0, c->stream, s, red, raw, d_dx);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&h, s, sizeof(LmDev), hipMemcpyDeviceToHost, c->stream));
  return VBA_OK;
}
// LI system: pose-pose entries to the lidar tiles, everything else to the compact IMU image (coef = 1); VBA_ERR_BAD_ARG for an
// entry outside the structure k_li_solve assumes (a coupling of frames more than one apart that is not pose-pose)
template <int W>
int dbg_li(vba_ctx *c, DbgBufs &B, const double *H, const double *g, int flags, LmDev &h, double *d_dx) {
  using C2 = HessCfg2<W>;
  using LC = LiSolveCfg<W>;
  constexpr int NT = W > 10 ? 1024 : 512, nw = 15 * W, nl = 6 * W;
  const int grav = (flags & VBA_SOLVE_GRAVITY) ? 1 : 0, n = nw + 3 * grav, gauge = grav ? 6 : 15, ne1 = li_hb_ne1(W);
  std::vector<double> hl((size_t)nl * nl, 0.0), hb(li_hb_size(W, 1), 0.0), gi(n, 0.0), gl(nl, 0.0);
  for (int R = 0; R < n; R++)
    for (int C = 0; C < n; C++) {
      const double a = H[(size_t)R * n + C];
      if (R < nw && C < nw) {
        const int fa = R / 15, fb = C / 15, ra = R - 15 * fa, cb = C - 15 * fb;
        if (ra < 6 && cb < 6) hl[(size_t)(6 * fa + ra) * nl + 6 * fb + cb] = a;
        else if (fa - fb > 1 || fb - fa > 1) { if (a != 0.0) return VBA_ERR_BAD_ARG; }
        else hb[li_hb_pair(fa, fb) + ra * 15 + cb] = a;
      } else if (R < nw) hb[ne1 + R * 3 + (C - nw)] = a;
      else if (C < nw) hb[ne1 + 45 * W + (R - nw) * nw + C] = a;
      else hb[ne1 + 90 * W + (R - nw) * 3 + (C - nw)] = a;
    }
  for (int R = 0; R < n; R++) {
    const int fa = R / 15, ra = R - 15 * fa;
    if (R < nw && ra < 6) gl[6 * fa + ra] = g[R]; else gi[R] = g[R];
  }
  std::vector<double> img;
  dbg_lidar_image<W>(hl.data(), gl.data(), false, img);
  const int copy_raw = (flags & VBA_SOLVE_COPY_RAW) ? 1 : 0, from_raw = copy_raw && (flags & VBA_SOLVE_FROM_RAW);
  LiDev li{};
  li.W = W; li.n = n; li.nb = n; li.gravity = grav; li.gauge = gauge; li.F = W - 1; li.imu_coef = 1.0;
  double *red = nullptr, *raw = nullptr, *himu = nullptr, *gimu = nullptr, *imu = nullptr, *scr = nullptr;
  LmDev *s = nullptr;
  LiDev *d_li = nullptr;
  HIPCHK(c, B.alloc(&red, C2::NOUT2)); HIPCHK(c, B.alloc(&raw, C2::NOUT2)); HIPCHK(c, B.alloc(&s, 1)); HIPCHK(c, B.alloc(&d_li, 1));
  HIPCHK(c, B.alloc(&himu, hb.size())); HIPCHK(c, B.alloc(&gimu, (size_t)n)); HIPCHK(c, B.alloc(&imu, (size_t)304 * W));
  if (LC::GL) HIPCHK(c, B.alloc(&scr, LC::l_doubles * LM_SPEC));
  h.is_calc_hess = from_raw ? 0 : 1;
  HIPCHK(c, hipMemsetAsync(red, 0, C2::NOUT2 * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(raw, 0, C2::NOUT2 * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(imu, 0, (size_t)304 * W * sizeof(double), c->stream));
  HIPCHK(c, hipMemcpyAsync(from_raw ? raw : red, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(himu, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(gimu, gi.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(s, &h, sizeof(LmDev), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_li, &li, sizeof(LiDev), hipMemcpyHostToDevice, c->stream));
  if (flags & VBA_SOLVE_DENSE_MASK) {
    HIPCHK(c, hipFuncSetAttribute((const void *)k_li_solve<W, NT, LC::GL, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LC::lds));
    hipLaunchKernelGGL((k_li_solve<W, NT, LC::GL, true>), dim3(c->lm_spec), dim3(NT), LC::lds, c->stream, s, d_li, red, raw, copy_raw, himu, gimu, imu, n, gauge, grav,
                       1.0, scr, d_dx);
  } else {
    HIPCHK(c, hipFuncSetAttribute((const void *)k_li_solve<W, NT, LC::GL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LC::lds));
    hipLaunchKernelGGL((k_li_solve<W, NT, LC::GL>), dim3(c->lm_spec), dim3(NT), LC::lds, c->stream, s, d_li, red, raw, copy_raw, himu, gimu, imu, n, gauge, grav,
                       1.0, scr, d_dx);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&h, s, sizeof(LmDev), hipMemcpyDeviceToHost, c->stream));
  return VBA_OK;
}
}  // namespace
}  // extern "C++"

int vba_debug_solve(vba_ctx *c, int kind, int W, int flags, const double *H, const double *g, double u, double v, double *dx, double *q1) {
  if (!c || !H || !g || !dx || !q1) return VBA_ERR_BAD_ARG;
  int n;
  if (kind == VBA_SOLVE_LIDAR) { if (W < 2 || W > 16) return VBA_ERR_BAD_ARG; n = 6 * W; }
  else if (kind == VBA_SOLVE_LI) { if (W < 2 || W > LI_MAX_W) return VBA_ERR_BAD_ARG; n = 15 * W + ((flags & VBA_SOLVE_GRAVITY) ? 3 : 0); }
  else if (kind == VBA_SOLVE_DENSE) { if (W < 2 || W > 1024) return VBA_ERR_BAD_ARG; n = 6 * W; }
  else return VBA_ERR_BAD_ARG;
  // finite, symmetric input; the damping of every candidate finite (no non-finite value reaches the device)
  for (int r = 0; r < n; r++) {
    if (!std::isfinite(g[r])) return VBA_ERR_BAD_ARG;
    for (int k = 0; k < n; k++) {
      const double a = H[(size_t)r * n + k];
      if (!std::isfinite(a) || a != H[(size_t)k * n + r]) return VBA_ERR_BAD_ARG;
    }
  }
  const int ncand = kind == VBA_SOLVE_DENSE ? 1 : c->lm_spec;
  {
    double ub = u, vb = v;
    if (!std::isfinite(u) || !std::isfinite(v)) return VBA_ERR_BAD_ARG;
    for (int k = 1; k < ncand; k++) { ub = ub * vb; vb = 2 * vb; if (!std::isfinite(ub) || !std::isfinite(vb)) return VBA_ERR_BAD_ARG; }
  }
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<LmDev> hv(1);                      // (declared before the buffers: their destructor drains the stream first)
  DbgBufs B(c->stream);
  if (kind == VBA_SOLVE_DENSE) {                 // big_damping_iter's solve: host pivot order, k_bigl_* on the device
    BigStore S;
    S.b.W = W; S.NP = (n + 7) / 8 * 8; S.ld = (S.NP + 63) / 64 * 64;
    HIPCHK(c, B.alloc(&S.b.H, (size_t)n * n)); HIPCHK(c, B.alloc(&S.b.g, (size_t)n));
    HIPCHK(c, B.alloc(&S.d_Ab, (size_t)(S.NP + 1) * S.ld)); HIPCHK(c, B.alloc(&S.d_Tb, (size_t)(S.NP + 1) * 8));
    HIPCHK(c, B.alloc(&S.d_ord, (size_t)n)); HIPCHK(c, B.alloc(&S.d_vec, (size_t)3 * n));
    HIPCHK(c, hipMemcpyAsync(S.b.H, H, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.b.g, g, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    std::vector<double> hd(n), jt(g, g + n);
    std::vector<int> ord(n);
    for (int r = 0; r < n; r++) hd[r] = H[(size_t)r * n + r];
    for (int r = 0; r < 6; r++) { hd[r] = 1.0; jt[r] = 0.0; }       // gauge VM:452-455
    big_pivot_order(hd.data(), u, n, ord.data());
    const int st = big_solve(S, c->stream, ord.data(), u, dx, c->err);
    if (st) return st;
    q1[0] = big_q1(dx, hd.data(), jt.data(), u, n);
    return VBA_OK;
  }
  LmDev *h = hv.data();
  std::memset(h, 0, sizeof(LmDev));
  for (int f = 0; f < W; f++) { h->x[12 * f] = h->x[12 * f + 4] = h->x[12 * f + 8] = 1.0; }
  h->u = u; h->v = v;
  if (flags & VBA_SOLVE_ALL_PANELS) h->pad = 128;   // bit of the diagnostic mask the solve kernels load: run every panel
  double *d_dx = nullptr;
  HIPCHK(c, B.alloc(&d_dx, (size_t)ncand * n));
  int st = VBA_ERR_BAD_ARG;
  switch (W) {
#define VBA_DS_CASE(WW) case WW: st = kind == VBA_SOLVE_LIDAR ? dbg_lidar<WW>(c, B, H, g, flags, *h, d_dx) : dbg_li<WW>(c, B, H, g, flags, *h, d_dx); break;
    VBA_DS_CASE(2) VBA_DS_CASE(3) VBA_DS_CASE(4) VBA_DS_CASE(5) VBA_DS_CASE(6) VBA_DS_CASE(7) VBA_DS_CASE(8) VBA_DS_CASE(9) VBA_DS_CASE(10)
    VBA_DS_CASE(11) VBA_DS_CASE(12) VBA_DS_CASE(13) VBA_DS_CASE(14) VBA_DS_CASE(15) VBA_DS_CASE(16)
#undef VBA_DS_CASE
  }
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(dx, d_dx, (size_t)ncand * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < ncand; b++) q1[b] = h->q1_spec[b];
  return VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ keyframe store (vba_kf_*)
#include "vba_kernels_kf.hpp"

struct vba_kf_store {
  vba_ctx *ctx = nullptr;
  // the keyframes: points (their own frame, float values in doubles) and covariance diagonals, ragged by off
  double *d_pnt = nullptr; float *d_var = nullptr; size_t cap = 0;
  std::vector<int> off{0};
  struct Meta { double x0[12]; int id; double jour; int exist; };
  std::vector<Meta> kf;
  // scratch of one merge of up to mcap points: staged host input, merged cloud (also the world points of a load), gathered covariance
  // diagonals, per-voxel counts, the down-sampler's work area; pinned: gathered diagonals of a host covariance array
  size_t mcap = 0;
  double *d_src = nullptr, *d_merge = nullptr, *d_mdiag = nullptr, *h_diag = nullptr;
  int *d_cnt = nullptr; char *d_ws = nullptr; size_t ws_bytes = 0;
  // per-scan transforms [tcap][12] and offsets [tcap + 1]: pinned image and device copy; the voxel count of a build (pinned)
  int tcap = 0; char *h_tab = nullptr, *d_tab = nullptr; int *h_n = nullptr;
  hipEvent_t ev = nullptr;
  int allocs = 0; int64_t bytes = 0;
  int hist = 0; std::vector<float> hist_pos;   // history_kfsize, pl_kdmap
  int last_m = 0;                              // voxels of the last build (their counts stay in d_cnt)
};

namespace {

size_t kf_tab_bytes(int t) { return (size_t)t * 12 * sizeof(double) + (((size_t)t + 1) * sizeof(int) + 15 & ~(size_t)15); }

template <class T>
int kf_alloc(vba_kf_store *s, T **p, size_t n) {
  vba_ctx *c = s->ctx;
  if (*p) hipFree(*p);
  *p = nullptr;
  HIPCHK(c, hipMalloc((void **)p, (n ? n : 1) * sizeof(T)));
  s->allocs++; s->bytes += (int64_t)(n * sizeof(T));
  return VBA_OK;
}

// layout of the down-sampler's work area for n points
size_t kf_ws_layout(vba_ctx *c, int n, bool det, char *base, DsWork *w, int *status) {
  int cap = 1024;
  while (cap < 2 * n) cap <<= 1;
  unsigned int key_bits = 1;
  while ((1u << key_bits) < (unsigned)cap) key_bits++;
  const int nb = (n + 255) / 256;
  const size_t b_i = (((size_t)n * sizeof(int)) + 255) & ~(size_t)255, b_tab = (size_t)cap * sizeof(DsSlot),
               b_blk = (((size_t)nb + 2) * sizeof(int) + 255) & ~(size_t)255;
  size_t tmp = 0;
  if (det && sort_pairs_u32(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, (size_t)n, key_bits, c->stream) != hipSuccess) { *status = VBA_ERR_HIP; return 0; }
  tmp = (tmp + 255) & ~(size_t)255;
  if (w) {
    w->tab = (DsSlot *)base; w->cap = cap; w->key_bits = key_bits;
    w->slot = (int *)(base + b_tab); w->blk = (int *)(base + b_tab + b_i); w->n_out = w->blk + nb;
    if (det) {
      char *sb = base + b_tab + b_i + b_blk;
      w->skey = (unsigned int *)sb; w->idx = (int *)(sb + b_i); w->sidx = (int *)(sb + 2 * b_i); w->tmp = sb + 3 * b_i; w->tmp_bytes = tmp;
    }
  }
  *status = VBA_OK;
  return b_tab + b_i + b_blk + (det ? 3 * b_i + tmp : 0);
}

// grow-only: the keyframe arrays move (device-to-device copy, the old blocks are freed after a synchronise)
int kf_ensure_rows(vba_kf_store *s, size_t need) {
  if (need <= s->cap) return VBA_OK;
  vba_ctx *c = s->ctx;
  size_t m = s->cap ? s->cap : 65536;
  while (m < need) m *= 2;
  double *np = nullptr; float *nv = nullptr;
  HIPCHK(c, hipMalloc((void **)&np, m * 3 * sizeof(double)));
  if (hipMalloc((void **)&nv, m * 3 * sizeof(float)) != hipSuccess) { hipFree(np); c->set_error("keyframe store: out of device memory"); return VBA_ERR_HIP; }
  const size_t have = (size_t)s->off.back();
  if (have) {
    HIPCHK(c, hipMemcpyAsync(np, s->d_pnt, have * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(nv, s->d_var, have * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (s->d_pnt) hipFree(s->d_pnt);
  if (s->d_var) hipFree(s->d_var);
  s->d_pnt = np; s->d_var = nv; s->cap = m;
  s->allocs += 2; s->bytes += (int64_t)(m * 3 * (sizeof(double) + sizeof(float)));
  return VBA_OK;
}

int kf_ensure_merge(vba_kf_store *s, size_t need) {
  if (need <= s->mcap) return VBA_OK;
  vba_ctx *c = s->ctx;
  size_t m = s->mcap ? s->mcap : 65536;
  while (m < need) m *= 2;
  if (m > ((size_t)1 << 28)) return VBA_ERR_CAPACITY;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int st = VBA_OK;
  const size_t ws = kf_ws_layout(c, (int)m, true, nullptr, nullptr, &st);
  if (st) return st;
  if ((st = kf_alloc(s, &s->d_src, 3 * m)) || (st = kf_alloc(s, &s->d_merge, 3 * m)) || (st = kf_alloc(s, &s->d_mdiag, 3 * m)) ||
      (st = kf_alloc(s, &s->d_cnt, m)) || (st = kf_alloc(s, &s->d_ws, ws)))
    return st;
  if (s->h_diag) hipHostFree(s->h_diag);
  s->h_diag = nullptr;
  HIPCHK(c, hipHostMalloc((void **)&s->h_diag, 3 * m * sizeof(double), hipHostMallocDefault));
  s->allocs++;
  s->ws_bytes = ws; s->mcap = m;
  return VBA_OK;
}

int kf_ensure_tab(vba_kf_store *s, int k) {
  if (k <= s->tcap) return VBA_OK;
  vba_ctx *c = s->ctx;
  int t = s->tcap ? s->tcap : 64;
  while (t < k) t *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (s->h_tab) hipHostFree(s->h_tab);
  s->h_tab = nullptr;
  HIPCHK(c, hipHostMalloc((void **)&s->h_tab, kf_tab_bytes(t), hipHostMallocDefault));
  s->allocs++;
  int st = kf_alloc(s, &s->d_tab, kf_tab_bytes(t));
  if (st) return st;
  s->tcap = t;
  return VBA_OK;
}

// Host half of the merge (include/voxelba.h, "order of operations"): T = [dR, dp] of a cloud at pose x into the frame of pose xc
void kf_delta(const double *xc, const double *x, double *T) {
  volatile double a, b, e;     // every product and sum rounded on its own, whatever the host compiler would contract
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) {
      a = xc[0 * 3 + r] * x[0 * 3 + cc]; b = xc[1 * 3 + r] * x[1 * 3 + cc]; a = a + b; e = xc[2 * 3 + r] * x[2 * 3 + cc];
      T[3 * r + cc] = a + e;
    }
  const double d0 = x[9] - xc[9], d1 = x[10] - xc[10], d2 = x[11] - xc[11];
  for (int r = 0; r < 3; r++) {
    a = xc[0 * 3 + r] * d0; b = xc[1 * 3 + r] * d1; a = a + b; e = xc[2 * 3 + r] * d2;
    T[9 + r] = a + e;
  }
}

// the transform table of k clouds with poses [k][12] (xc = the last) and row offsets rel [k + 1] -> pinned image -> device, on st
int kf_upload_tab(vba_kf_store *s, int k, const double *const *poses, const int *rel, hipStream_t st) {
  vba_ctx *c = s->ctx;
  double *T = (double *)s->h_tab;
  int *o = (int *)(s->h_tab + (size_t)s->tcap * 12 * sizeof(double));
  for (int i = 0; i < k; i++) kf_delta(poses[k - 1], poses[i], T + 12 * i);
  for (int i = 0; i <= k; i++) o[i] = rel[i];
  HIPCHK(c, hipMemcpyAsync(s->d_tab, s->h_tab, kf_tab_bytes(s->tcap), hipMemcpyHostToDevice, st));
  return VBA_OK;
}
const double *kf_dev_xf(const vba_kf_store *s) { return (const double *)s->d_tab; }
const int *kf_dev_off(const vba_kf_store *s) { return (const int *)(s->d_tab + (size_t)s->tcap * 12 * sizeof(double)); }

bool kf_pose_ok(const double *p) { for (int i = 0; i < 12; i++) if (!std::isfinite(p[i])) return false; return true; }

}  // namespace

extern "C" {

int vba_kf_create(vba_ctx *c, vba_kf_store **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  vba_kf_store *s = new vba_kf_store();
  s->ctx = c;
  int st = kf_ensure_tab(s, 64);
  if (!st && hipHostMalloc((void **)&s->h_n, 64, hipHostMallocDefault) != hipSuccess) st = VBA_ERR_HIP;
  if (!st && hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) != hipSuccess) st = VBA_ERR_HIP;
  if (st) { vba_kf_destroy(s); return st; }
  s->allocs++;
  *out = s;
  return VBA_OK;
}

void vba_kf_destroy(vba_kf_store *s) {
  if (!s) return;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  void *d[] = {s->d_pnt, s->d_var, s->d_src, s->d_merge, s->d_mdiag, s->d_cnt, s->d_ws, s->d_tab};
  for (void *p : d) if (p) hipFree(p);
  if (s->h_diag) hipHostFree(s->h_diag);
  if (s->h_tab) hipHostFree(s->h_tab);
  if (s->h_n) hipHostFree(s->h_n);
  if (s->ev) hipEventDestroy(s->ev);
  delete s;
}

int vba_kf_reserve(vba_kf_store *s, int64_t points, int keyframes, int64_t merge_points) {
  if (!s || points < 0 || keyframes < 0 || merge_points < 0 || points > ((int64_t)1 << 30) || merge_points > ((int64_t)1 << 28) || keyframes > (1 << 24))
    return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if (merge_points > 0 && (st = kf_ensure_merge(s, (size_t)merge_points))) return st;
  // a build writes its kept cloud straight behind the last keyframe, and that cloud is bounded only by the merged one
  if (points + merge_points > 0 && (st = kf_ensure_rows(s, (size_t)(points + merge_points)))) return st;
  s->off.reserve((size_t)keyframes + 1); s->kf.reserve((size_t)keyframes); s->hist_pos.reserve(3 * (size_t)keyframes);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_kf_allocations(vba_kf_store *s, int *count, int64_t *bytes) {
  if (!s || !count || !bytes) return VBA_ERR_BAD_ARG;
  *count = s->allocs; *bytes = s->bytes;
  return VBA_OK;
}

int vba_kf_size(vba_kf_store *s) { return s ? (int)s->kf.size() : 0; }

int vba_kf_build(vba_kf_store *s, int k, const int *offsets, const double *pnt, const double *var, const double *poses, double voxel_size, int id,
                 double jour, vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds, int *n_points) {
  if (!s || k < 1 || !offsets || !poses || !n_points || !(voxel_size > 0) || (!var && voxel_size < 0.001)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < k; i++) if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
  const int off0 = offsets[0], n = offsets[k] - off0;
  if (n > (1 << 28) || (n > 0 && !pnt)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < k; i++) if (!kf_pose_ok(poses + 12 * i)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  const size_t N = (size_t)s->off.back();
  if (N + (size_t)n > (size_t)INT32_MAX) return VBA_ERR_CAPACITY;
  int st;
  if (db) {
    if (db->ctx->device != c->device) return VBA_ERR_BAD_ARG;
    if ((st = btc_generate_check(db, n, cap, rows, bits, n_stds))) return st;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = kf_ensure_tab(s, k)) || (st = kf_ensure_merge(s, (size_t)n)) || (st = kf_ensure_rows(s, N + (size_t)n))) return st;
  if (db && n > 0 && (st = btc_gen_ensure(db, n, 0, 0))) return st;
  int m = 0;
  if (n > 0) {
    std::vector<const double *> pp(k);
    std::vector<int> rel(k + 1);
    for (int i = 0; i < k; i++) pp[i] = poses + 12 * i;
    for (int i = 0; i <= k; i++) rel[i] = offsets[i] - off0;
    if ((st = kf_upload_tab(s, k, pp.data(), rel.data(), c->stream))) return st;
    const double *src = pnt + 3 * (size_t)off0, *dvar = nullptr;
    if (!is_device_ptr(pnt)) {
      HIPCHK(c, hipMemcpyAsync(s->d_src, src, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
      src = s->d_src;
    }
    if (var) {
      if (is_device_ptr(var)) dvar = var + 9 * (size_t)off0;      // gathered by the merge kernel, 72 bytes apart
      else {                                                       // host array: only the three diagonal doubles per point cross
        const double *v = var + 9 * (size_t)off0;
        for (size_t i = 0; i < (size_t)n; i++) { s->h_diag[3 * i] = v[9 * i]; s->h_diag[3 * i + 1] = v[9 * i + 4]; s->h_diag[3 * i + 2] = v[9 * i + 8]; }
        HIPCHK(c, hipMemcpyAsync(s->d_mdiag, s->h_diag, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
      }
    }
    const int nb = (n + 255) / 256;
    hipLaunchKernelGGL(k_kf_merge, dim3(nb), dim3(256), 0, c->stream, n, k, kf_dev_off(s), kf_dev_xf(s), src, dvar, 9, 4, s->d_merge,
                       db ? db->gen->xyz : (float *)nullptr, dvar ? s->d_mdiag : (double *)nullptr);
    if (db && db->ctx->stream != c->stream) {                      // the generator runs on its database's stream, behind the merge
      HIPCHK(c, hipEventRecord(s->ev, c->stream));
      HIPCHK(c, hipStreamWaitEvent(db->ctx->stream, s->ev, 0));
    }
    const bool det = c->opt.deterministic != 0;
    DsWork w{};
    kf_ws_layout(c, n, det, s->d_ws, &w, &st);
    if (st) return st;
    TimedSpan sp{};
    span_begin(c, "downsample", sp);
    if ((st = ds_core(c, c->stream, var ? 1 : 0, n, s->d_merge, var ? s->d_mdiag : nullptr, 3, 1, voxel_size, det, w))) return st;
    hipLaunchKernelGGL(k_kf_emit, dim3(nb), dim3(256), 0, c->stream, n, w.tab, w.slot, w.blk, s->d_pnt + 3 * N, s->d_var + 3 * N, s->d_cnt, var ? 1 : 0);
    span_end(c, "downsample", sp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(s->h_n, w.n_out, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  if (db) {
    st = btc_generate_impl(db, n, nullptr, id, cap, rows, bits, n_stds);
    if (st) { hipStreamSynchronize(c->stream); return st; }
  }
  if (n > 0) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m = s->h_n[0];
  }
  // commit
  vba_kf_store::Meta me{};
  std::memcpy(me.x0, poses + 12 * (size_t)(k - 1), 12 * sizeof(double));
  me.id = id; me.jour = jour; me.exist = 0;
  s->kf.push_back(me);
  s->off.push_back((int)(N + (size_t)m));
  s->last_m = m;
  *n_points = m;
  return VBA_OK;
}

int vba_kf_last_counts(vba_kf_store *s, int cap, int *counts, int *n) {
  if (!s || !n || cap < 0 || (cap > 0 && !counts)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  *n = s->last_m;
  const int w = s->last_m < cap ? s->last_m : cap;
  if (w > 0) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(counts, s->d_cnt, (size_t)w * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VBA_OK;
}

int vba_kf_generate_stds(vba_kf_store *s, int first, int count, vba_btc_db *db, int cap, double *rows, uint64_t *bits, int *n_stds) {
  if (!s || !db || first < 0 || count < 1 || (size_t)first + (size_t)count > s->kf.size()) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  if (db->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  const int b = s->off[first], n = s->off[first + count] - b;
  int st;
  if ((st = btc_generate_check(db, n, cap, rows, bits, n_stds))) return st;
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = kf_ensure_tab(s, count))) return st;
  const int id = s->kf[first + count - 1].id;
  if (n > 0) {
    if ((st = btc_gen_ensure(db, n, 0, 0))) return st;
    std::vector<const double *> pp(count);
    std::vector<int> rel(count + 1);
    for (int i = 0; i < count; i++) pp[i] = s->kf[first + i].x0;
    for (int i = 0; i <= count; i++) rel[i] = s->off[first + i] - b;
    hipStream_t q = db->ctx->stream;                               // the store is quiescent between calls: everything on the database's stream
    if ((st = kf_upload_tab(s, count, pp.data(), rel.data(), q))) return st;
    hipLaunchKernelGGL(k_kf_merge, dim3((n + 255) / 256), dim3(256), 0, q, n, count, kf_dev_off(s), kf_dev_xf(s), s->d_pnt + 3 * (size_t)b,
                       (const double *)nullptr, 9, 4, (double *)nullptr, db->gen->xyz, (double *)nullptr);
    HIPCHK(c, hipGetLastError());
  }
  st = btc_generate_impl(db, n, nullptr, id, cap, rows, bits, n_stds);
  if (st) hipStreamSynchronize(db->ctx->stream);
  return st;
}

int vba_kf_set_poses(vba_kf_store *s, int first, int n, const double *poses) {
  if (!s || first < 0 || n < 0 || (size_t)first + (size_t)n > s->kf.size() || (n > 0 && !poses)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < n; i++) if (!kf_pose_ok(poses + 12 * i)) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < n; i++) std::memcpy(s->kf[first + i].x0, poses + 12 * (size_t)i, 12 * sizeof(double));
  return VBA_OK;
}

int vba_kf_get(vba_kf_store *s, int k, double *pose12, int *id, double *jour, int *exist, int *n_points) {
  if (!s || k < 0 || (size_t)k >= s->kf.size()) return VBA_ERR_BAD_ARG;
  const vba_kf_store::Meta &m = s->kf[k];
  if (pose12) std::memcpy(pose12, m.x0, 12 * sizeof(double));
  if (id) *id = m.id;
  if (jour) *jour = m.jour;
  if (exist) *exist = m.exist;
  if (n_points) *n_points = s->off[k + 1] - s->off[k];
  return VBA_OK;
}

int vba_kf_set_history(vba_kf_store *s, int n_hist) {
  if (!s || n_hist < 0 || (size_t)n_hist > s->kf.size()) return VBA_ERR_BAD_ARG;
  s->hist_pos.resize(3 * (size_t)n_hist);
  for (size_t i = 0; i < s->kf.size(); i++) {
    s->kf[i].exist = (int)i < n_hist ? 1 : 0;
    if ((int)i < n_hist) for (int j = 0; j < 3; j++) s->hist_pos[3 * i + j] = (float)s->kf[i].x0[9 + j];
  }
  s->hist = n_hist;
  return VBA_OK;
}

int vba_kf_history_size(vba_kf_store *s) { return s ? s->hist : 0; }

int vba_kf_load(vba_kf_store *s, int k, vba_ctx *mc, double jour) {
  if (!s || !mc || k < 0 || (size_t)k >= s->kf.size()) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  if (mc->device != c->device) return VBA_ERR_BAD_ARG;
  const int b = s->off[k], n = s->off[k + 1] - b;
  if (n > 0) {
    HIPCHK(c, hipSetDevice(c->device));
    int st;
    if ((st = kf_ensure_merge(s, (size_t)n))) return st;
    // the keyframe's x0 goes through the pinned table; the world points into the merge scratch, on the map context's stream
    std::memcpy(s->h_tab, s->kf[k].x0, 12 * sizeof(double));
    HIPCHK(mc, hipMemcpyAsync(s->d_tab, s->h_tab, 12 * sizeof(double), hipMemcpyHostToDevice, mc->stream));
    hipLaunchKernelGGL(k_kf_world, dim3((n + 255) / 256), dim3(256), 0, mc->stream, n, (const double *)s->d_tab, s->d_pnt + 3 * (size_t)b, s->d_merge);
    HIPCHK(mc, hipGetLastError());
    st = map_cut_voxel_fix(mc->map, mc->stream, n, s->d_merge, jour, mc->err);   // ends with the map's counter read-back: one synchronise
    if (st) { hipStreamSynchronize(mc->stream); return st; }
  }
  s->kf[k].exist = 0;
  return VBA_OK;
}

int vba_kf_load_nearby(vba_kf_store *s, vba_ctx *mc, const double *p3, double radius, double jour, int *loaded) {
  if (!s || !mc || !p3 || !loaded || !(radius >= 0)) return VBA_ERR_BAD_ARG;
  *loaded = -1;
  if (s->hist <= 0) return VBA_OK;                                   // VS:1382
  const float q[3] = {(float)p3[0], (float)p3[1], (float)p3[2]};
  const float r2 = (float)(radius * radius);
  std::vector<std::pair<float, int>> hit;
  const int nh = (int)(s->hist_pos.size() / 3);
  for (int i = 0; i < nh; i++) {
    volatile float d2 = 0.0f, t;                                     // x, then y, then z, each product and sum rounded to float
    for (int j = 0; j < 3; j++) { t = s->hist_pos[3 * (size_t)i + j] - q[j]; t = t * t; d2 = d2 + t; }
    if (d2 < r2) hit.emplace_back((float)d2, i);
  }
  std::sort(hit.begin(), hit.end());                                 // ascending distance, the lower index on a tie
  for (const auto &h : hit) {
    if (!s->kf[h.second].exist) continue;
    const int st = vba_kf_load(s, h.second, mc, jour);
    if (st) return st;
    s->hist--;
    *loaded = h.second;
    break;
  }
  return VBA_OK;
}

int vba_kf_read(vba_kf_store *s, int k, int cap, double *xyz, float *vardiag, int *n) {
  if (!s || !n || k < 0 || (size_t)k >= s->kf.size() || cap < 0) return VBA_ERR_BAD_ARG;
  vba_ctx *c = s->ctx;
  const int b = s->off[k], m = s->off[k + 1] - b;
  *n = m;
  const int w = m < cap ? m : cap;
  if (w > 0 && (xyz || vardiag)) {
    HIPCHK(c, hipSetDevice(c->device));
    if (xyz) HIPCHK(c, hipMemcpyAsync(xyz, s->d_pnt + 3 * (size_t)b, (size_t)w * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (vardiag) HIPCHK(c, hipMemcpyAsync(vardiag, s->d_var + 3 * (size_t)b, (size_t)w * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VBA_OK;
}

int vba_kf_clouds(vba_kf_store *s, const double **d_pnt, const int **offsets, int *n_kf) {
  if (!s || !d_pnt || !offsets || !n_kf) return VBA_ERR_BAD_ARG;
  *d_pnt = s->d_pnt; *offsets = s->off.data(); *n_kf = (int)s->kf.size();
  return VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ global map export (vba_kf_export_*)
namespace {

const long long kExpChunk = 1ll << 22;       // records per pass through the staging buffer of a host export (64 MiB)
const int kExpMaxBlocks = 2048;              // grid cap of the streaming kernel: 256 CUs x 8 workgroups, the rest is grid-strided

inline long long exp_count(long long size, long long jump) { return (size + jump - 1) / jump; }   // j = 0, jump, ... < size

// the table of `entries` keyframes: every image of the pinned ring and the device copy
int exp_ensure_tab(vba_ctx *c, size_t entries) {
  for (int i = 0; i < vba_ctx::kExpRing; i++)
    if (!c->exp_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->exp_ev[i], hipEventDisableTiming));
  if (entries <= c->exp_cap) return VBA_OK;
  size_t m = c->exp_cap ? c->exp_cap : 1024;
  while (m < entries) m *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < vba_ctx::kExpRing; i++) { if (c->h_exp[i]) hipHostFree(c->h_exp[i]); c->h_exp[i] = nullptr; }
  if (c->d_exp) hipFree(c->d_exp);
  c->d_exp = nullptr; c->exp_cap = 0;
  for (int i = 0; i < vba_ctx::kExpRing; i++) HIPCHK(c, hipHostMalloc((void **)&c->h_exp[i], m * sizeof(ExpKf), hipHostMallocDefault));
  HIPCHK(c, hipMalloc((void **)&c->d_exp, m * sizeof(ExpKf)));
  c->exp_cap = m;
  return VBA_OK;
}

int exp_ensure_out(vba_ctx *c, size_t recs) {
  if (recs <= c->expout_cap) return VBA_OK;
  size_t m = c->expout_cap ? c->expout_cap : 65536;
  while (m < recs) m *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->d_expout) hipFree(c->d_expout);
  c->d_expout = nullptr; c->expout_cap = 0;
  HIPCHK(c, hipMalloc((void **)&c->d_expout, m * sizeof(float4)));
  c->expout_cap = m;
  return VBA_OK;
}

}  // namespace

extern "C" {

int vba_kf_export_plan(int n_kf, const int *sizes, int64_t interval_size, int jump, int *jump_out, int64_t *kf_begin, int cap_msgs, int *msg_end_kf,
                       int *n_msgs) {
  if (n_kf < 0 || (n_kf > 0 && !sizes) || interval_size < 1 || jump < 0 || !jump_out || !kf_begin || !n_msgs || cap_msgs < 0 ||
      (cap_msgs > 0 && !msg_end_kf))
    return VBA_ERR_BAD_ARG;
  uint64_t psize = 0;                                          // VS:117-123 in 64 bits: the reference's `uint psize` wraps at 2^32
  for (int k = 0; k < n_kf; k++) {
    if (sizes[k] < 0) return VBA_ERR_BAD_ARG;
    psize += (uint64_t)sizes[k];
  }
  if (jump == 0) {
    if (psize >= ((uint64_t)1 << 32)) return VBA_ERR_BAD_ARG;
    const uint64_t ten = interval_size > INT64_MAX / 10 ? (uint64_t)INT64_MAX : 10 * (uint64_t)interval_size;
    jump = (int)(psize / ten) + 1;                             // VS:124
  }
  *jump_out = jump;
  int64_t total = 0, pl = 0;
  int nm = 0;
  for (int k = 0; k < n_kf; k++) {
    kf_begin[k] = total;
    const int64_t cnt = exp_count(sizes[k], jump);             // VS:133
    total += cnt; pl += cnt;
    if (pl > interval_size) {                                  // VS:145-150
      if (nm < cap_msgs) msg_end_kf[nm] = k + 1;
      nm++; pl = 0;
    }
  }
  kf_begin[n_kf] = total;
  if (nm < cap_msgs) msg_end_kf[nm] = n_kf;                    // VS:153: published whatever it holds
  nm++;
  *n_msgs = nm;
  return VBA_OK;
}

int vba_kf_export_world(vba_ctx *c, int n_stores, vba_kf_store *const *stores, const float *intensity, int jump, int64_t begin, int64_t count,
                        float *xyzi) {
  if (!c || n_stores < 1 || !stores || !intensity || jump < 1 || begin < 0 || count < 0 || (count > 0 && !xyzi)) return VBA_ERR_BAD_ARG;
  for (int s = 0; s < n_stores; s++) if (!stores[s] || stores[s]->ctx->device != c->device) return VBA_ERR_BAD_ARG;
  // exported points before every keyframe of the whole sequence (the plan's kf_begin), keyframes before every store
  std::vector<long long> &first = c->exp_first;
  std::vector<int> &kbase = c->exp_kbase;
  first.clear(); kbase.clear();
  long long total = 0;
  for (int s = 0; s < n_stores; s++) {
    const std::vector<int> &off = stores[s]->off;
    if (first.size() + stores[s]->kf.size() > (size_t)(1 << 30)) return VBA_ERR_CAPACITY;
    kbase.push_back((int)first.size());
    for (size_t k = 0; k + 1 < off.size(); k++) { first.push_back(total); total += exp_count((long long)off[k + 1] - off[k], jump); }
  }
  kbase.push_back((int)first.size());
  first.push_back(total);
  if (begin > total || count > total - begin) return VBA_ERR_BAD_ARG;
  if (count == 0) return VBA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dev_out = is_device_ptr(xyzi);
  if (dev_out && ((uintptr_t)xyzi & 15)) { c->set_error("vba_kf_export_world: a device xyzi must be 16-byte aligned"); return VBA_ERR_BAD_ARG; }
  const long long end = begin + count;
  // the keyframes of the first and of the last exported point: the last k with first[k] <= i (never an empty keyframe)
  auto kf_of = [&](long long i) { return (int)(std::upper_bound(first.begin(), first.end() - 1, i) - first.begin()) - 1; };
  const int ka = kf_of(begin), kb = kf_of(end - 1), nk = kb - ka + 1;
  int st;
  if ((st = exp_ensure_tab(c, (size_t)nk))) return st;
  if (!dev_out && (st = exp_ensure_out(c, (size_t)(count < kExpChunk ? count : kExpChunk)))) return st;
  const int slot = c->exp_next;
  c->exp_next = (slot + 1) % vba_ctx::kExpRing;
  HIPCHK(c, hipEventSynchronize(c->exp_ev[slot]));             // the upload that last read this image (kExpRing calls ago): long done
  ExpKf *h = (ExpKf *)c->h_exp[slot];
  for (int s = 0; s < n_stores; s++) {
    const vba_kf_store *S = stores[s];
    for (int g = std::max(ka, kbase[s]); g <= kb && g < kbase[s + 1]; g++) {
      const int k = g - kbase[s];
      ExpKf &e = h[g - ka];
      e.first = first[g]; e.row = S->off[k];
      std::memcpy(e.T, S->kf[k].x0, 12 * sizeof(double));
    }
  }
  HIPCHK(c, hipMemcpyAsync(c->d_exp, h, (size_t)nk * sizeof(ExpKf), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->exp_ev[slot], c->stream));
  const ExpKf *d_tab = (const ExpKf *)c->d_exp;
  for (long long cb = begin; cb < end; cb += dev_out ? count : kExpChunk) {
    const long long ce = dev_out ? end : std::min(end, cb + kExpChunk);
    float4 *out = dev_out ? (float4 *)xyzi : (float4 *)c->d_expout;                     // the record of cb
    for (int s = 0; s < n_stores; s++) {                       // one launch per store: its point array, its intensity, its rows of the table
      const long long a = std::max(cb, first[kbase[s]]), b = std::min(ce, first[kbase[s + 1]]);
      if (a >= b) continue;
      const int g0 = std::max(ka, kbase[s]), g1 = std::min(kb, kbase[s + 1] - 1);
      const long long nb = (b - a + 255) / 256;
      hipLaunchKernelGGL(k_kf_export, dim3((unsigned)std::min<long long>(nb, kExpMaxBlocks)), dim3(256), 0, c->stream, a, b - a, g1 - g0 + 1,
                         d_tab + (g0 - ka), (const double *)stores[s]->d_pnt, jump, intensity[s], out + (a - cb));
    }
    HIPCHK(c, hipGetLastError());
    if (!dev_out) HIPCHK(c, hipMemcpyAsync(xyzi + 4 * (size_t)(cb - begin), c->d_expout, (size_t)(ce - cb) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  }
  if (!dev_out) HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ loop-closure map (vba_loop_map_*, vba_loop_update)
#include "vba_kernels_loop.hpp"

struct vba_loop_map {
  vba_ctx *ctx = nullptr;
  MapStore map;                                  // map_loop; after vba_loop_update the map the context gave up (ping-pong)
  size_t res_fix = 0, res_nodes = 0;             // vba_loop_map_reserve: applied to whichever store the object owns
  // segment table int4 [tcap] + poses double [tcap][12]: pinned image and device copy
  int tcap = 0; char *h_tab = nullptr, *d_tab = nullptr;
  char *d_in = nullptr; size_t in_bytes = 0;     // host-memory scans of vba_loop_update on their way to the device
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
  b += (size_t)s.hcap * (s.det ? 16 : 12) + s.stage_bytes + s.sort_tmp_bytes + s.whist_cap * sizeof(int);
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
  if (lm->h_tab) hipHostFree(lm->h_tab);
  if (lm->d_tab) hipFree(lm->d_tab);
  lm->h_tab = nullptr; lm->d_tab = nullptr; lm->tcap = 0;
  HIPCHK(c, hipHostMalloc((void **)&lm->h_tab, lm_tab_bytes(m), hipHostMallocDefault));
  HIPCHK(c, hipMalloc((void **)&lm->d_tab, lm_tab_bytes(m)));
  lm->allocs += 2; lm->bytes += (int64_t)lm_tab_bytes(m);
  lm->tcap = m;
  return VBA_OK;
}
int lm_ensure_in(vba_loop_map *lm, size_t bytes) {
  if (bytes <= lm->in_bytes) return VBA_OK;
  vba_ctx *c = lm->ctx;
  HIPCHK(c, hipDeviceSynchronize());
  if (lm->d_in) hipFree(lm->d_in);
  lm->d_in = nullptr; lm->in_bytes = 0;
  HIPCHK(c, hipMalloc((void **)&lm->d_in, bytes));
  lm->allocs++; lm->bytes += (int64_t)bytes;
  lm->in_bytes = bytes;
  return VBA_OK;
}
int4 *lm_h_seg(vba_loop_map *lm) { return (int4 *)lm->h_tab; }
double *lm_h_pose(vba_loop_map *lm) { return (double *)(lm->h_tab + (size_t)lm->tcap * sizeof(int4)); }
const int4 *lm_d_seg(vba_loop_map *lm) { return (const int4 *)lm->d_tab; }
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
  if (lm->h_tab) hipHostFree(lm->h_tab);
  if (lm->d_tab) hipFree(lm->d_tab);
  if (lm->d_in) hipFree(lm->d_in);
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

int vba_loop_update(vba_ctx *c, vba_loop_map *lm, const double *dx12, int k, const int *offsets, const double *pnt, const double *var, const double *poses_bl,
                    int win_count, const double *win_pnt, const double *win_var, const int *win_offsets, const double *poses_win, int *n_factors) {
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
  const bool bl_host = n_bl > 0 && !is_device_ptr(pnt);
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
    for (int i = 0; i < k; i++) seg[i] = make_int4(offsets[i] - off0, offsets[i] - off0, i, 0);
    std::memcpy(lm_h_pose(lm), poses_bl, 12 * sizeof(double) * (size_t)k);
    if (hipMemcpyAsync(lm->d_tab, lm->h_tab, lm_tab_bytes(lm->tcap), hipMemcpyHostToDevice, st) != hipSuccess) { c->set_error("vba_loop_update: table upload failed"); return fail(VBA_ERR_HIP); }
    const double *d_p = pnt + 3 * (size_t)off0, *d_v = var ? var + 9 * (size_t)off0 : nullptr;
    if (bl_host) {
      hipError_t e = hipMemcpyAsync(lm->d_in, d_p, (size_t)n_bl * 24, hipMemcpyHostToDevice, st);
      if (e == hipSuccess && var) e = hipMemcpyAsync(lm->d_in + (size_t)n_bl * 24, d_v, (size_t)n_bl * 72, hipMemcpyHostToDevice, st);
      if (e != hipSuccess) { c->set_error("vba_loop_update: scan upload failed"); return fail(VBA_ERR_HIP); }
      d_p = (const double *)lm->d_in; d_v = var ? (const double *)(lm->d_in + (size_t)n_bl * 24) : nullptr;
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

}  // extern "C"
