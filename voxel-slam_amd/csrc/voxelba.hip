// libvoxelba.so — implementation of include/voxelba.h for MI355X (gfx950): the BA core.  The map, the odometry, hierarchical global BA,
// the initialisation, the scan pre-processing and keyframe store, the loop map, loop retrieval, pose-graph optimisation and the session
// formats are units of their own ("source layout").
// Host side: context / HBM store management, the three LM drivers (voxel_map.hpp:342-976) and the IMU factor;
// device side: the kernels in vba_kernels_factor.hpp and the headers included below.  No CPU compute fallback exists.
#include "vba_ctx.hpp"
#include "vba_kernels_factor.hpp"
#include "vba_kernels_h3.hpp"
#include "vba_kernels_lm.hpp"
#include "vba_kernels_li.hpp"
#include <cstddef>
#include "vba_hostmath.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // TYPES only: the entry points are resolved at run time (rccl_api below), the library does not link librccl
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <array>
#include <map>
#include <chrono>
#include <algorithm>

using namespace vba;

namespace {

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
}

namespace {

// damping candidates per solve launch (vba_kernels_lm.hpp, "Speculative damping"); 1 = the plain sequential solve.  Read when a
// context is created (vba_options::lm_spec; tests compare the two forms bit for bit).
static const int kMaxBlocksHess = 256;     // upper bound of vba_options::hessian_workgroups (sizes the partial slab): one workgroup per CU

int nout_of(int W) { return 36 * W * W + 6 * W + 1; }   // full layout [H | g | r]
int nout_tl(int W) {                                      // tile layout produced by k_hessian2 (HessCfg2<W>::NOUT2)
  const int nt16 = (6 * W + 15) / 16;
  return nt16 * (nt16 + 1) / 2 * 256 + 27 * W + 1;
}

static inline bool span_on(vba_ctx *c, const char *name) { return c->timing && (c->timing_only.empty() || c->timing_only == name); }
}  // namespace

namespace vba {
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
  HIPCHK(c, c->h_pin.ensure(n));
  return VBA_OK;
}
int ensure_stage(vba_ctx *c, size_t bytes) {
  HIPCHK(c, c->d_stage.ensure(bytes));
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
  // the new set is built in locals and swapped in after the synchronise: an early return frees it, the old set dies at scope exit
  DevMem<double> nr[6]; DevMem<unsigned int> nocc; DevMem<int> ntiles;
  for (int k = 0; k < 6; k++) {
    HIPCHK(c, nr[k].ensure(rows[k] * newcap));
    HIPCHK(c, hipMemsetAsync(nr[k], 0, rows[k] * newcap * sizeof(double), c->stream));
    if (c->nvox > 0 && c->fv_rows[k])
      HIPCHK(c, hipMemcpy2DAsync(nr[k], (size_t)newcap * sizeof(double), c->fv_rows[k], (size_t)c->cap * sizeof(double),
                                 (size_t)c->nvox * sizeof(double), rows[k], hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, ntiles.ensure((size_t)4 * newcap + 16));
  HIPCHK(c, hipMemsetAsync(ntiles, 0, ((size_t)4 * newcap + 16) * sizeof(int), c->stream));
  HIPCHK(c, nocc.ensure((size_t)newcap));
  HIPCHK(c, hipMemsetAsync(nocc, 0, (size_t)newcap * sizeof(unsigned int), c->stream));
  if (c->nvox > 0 && c->fv_occ) HIPCHK(c, hipMemcpyAsync(nocc, c->fv_occ, (size_t)c->nvox * sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 6; k++) std::swap(c->fv_rows[k], nr[k]);
  std::swap(c->fv_occ, nocc); std::swap(c->fv_tiles, ntiles);
  n.cl = c->fv_rows[0]; n.fix = c->fv_rows[1]; n.coe = c->fv_rows[2]; n.eigval = c->fv_rows[3]; n.eigvec = c->fv_rows[4]; n.pcr = c->fv_rows[5];
  n.occ = c->fv_occ; n.tiles = c->fv_tiles;
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
}  // namespace vba

namespace {

int upload_poses(vba_ctx *c, const double *poses) {
  const int W = c->opt.win_size;
  int st = ensure_pin(c, kPinFixed);
  if (st) return st;
  std::memcpy(c->h_pin, poses, (size_t)W * 12 * sizeof(double));      // the pose region, kPinPoses = 0
  HIPCHK(c, hipMemcpyAsync(c->d_poses, c->h_pin, (size_t)W * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return VBA_OK;
}

// device addresses of the LmDev fields the passes take as arguments: accepted and trial poses, the gates of the two passes
struct LmPtrs { const double *x, *xt; const int *run_hess, *run_res; };
LmPtrs lm_ptrs(vba_ctx *c) {
  const char *base = reinterpret_cast<const char *>(c->d_lm.p);
  return {reinterpret_cast<const double *>(base + offsetof(LmDev, x)), reinterpret_cast<const double *>(base + offsetof(LmDev, xt)),
          reinterpret_cast<const int *>(base + offsetof(LmDev, run_hess)), reinterpret_cast<const int *>(base + offsetof(LmDev, run_res))};
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
  return for_window<2, 16>(c->opt.win_size, [&](auto wc) {
    constexpr int W = decltype(wc)::value;
    hipLaunchKernelGGL(k_lm_init<W>, dim3(1), dim3(256), 0, c->stream, lm_init_arg<W>(c, true));
    HIPCHK(c, hipGetLastError());
    return VBA_OK;
  });
}

// the IMU workgroup of LI-BA rides a lidar Hessian launch when its LDS fits this ceiling (150 KB hold it up to W = 16)
constexpr size_t kLiRideLds = 150 * 1024;

// ---------------------------------------------------------------- diagnostics of the BA core (-DVBA_DIAG builds, tools/README.md)
// The call paths hold one call each; in the shipped build diag_env answers nullptr and LmDev::pad stays 0, so each returns at its first test.
// VBA_K3_STAMPS=1: 16 in-kernel clock stamps per workgroup of the Hessian pass.  k3_stamps_buffer: the cleared device
// buffer in front of the launch, nullptr unless asked for; k3_stamps_dump: the first nst of four workgroups, relative to the earliest.
long long *k3_stamps_buffer(vba_ctx *c) {
  static const bool want_stamps = diag_env("VBA_K3_STAMPS") != nullptr;     // -DVBA_DIAG builds only
  if (!want_stamps) return nullptr;
  static long long *d_st = nullptr;
  if (!d_st) hipMalloc((void **)&d_st, (size_t)kMaxBlocksHess * 16 * 8);
  hipMemsetAsync(d_st, 0, (size_t)kMaxBlocksHess * 16 * 8, c->stream);
  return d_st;
}
void k3_stamps_dump(vba_ctx *c, const long long *d_st, int nb, int nst, const char *legend) {
  if (!d_st) return;
  std::vector<long long> h((size_t)nb * 16);
  hipStreamSynchronize(c->stream);
  hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost);
  long long t0 = h[0];
  for (int b = 0; b < nb; b++) if (h[(size_t)b * 16] && h[(size_t)b * 16] < t0) t0 = h[(size_t)b * 16];
  for (int b : {0, 1, nb / 2, nb - 1}) {
    fprintf(stderr, "[k3 stamps] wg %d:", b);
    for (int i = 0; i < nst; i++) fprintf(stderr, " %lld", h[(size_t)b * 16 + i] ? h[(size_t)b * 16 + i] - t0 : -1);
    fprintf(stderr, "\n");
  }
  long long tmax = 0;
  for (int b = 0; b < nb; b++) if (h[(size_t)b * 16 + nst - 1] - t0 > tmax) tmax = h[(size_t)b * 16 + nst - 1] - t0;
  fprintf(stderr, "[k3 stamps] last workgroup ends at %lld ticks (100 MHz wall clock: 1 tick = 10 ns)%s\n", tmax, legend);
}

// VBA_K4_STAMPS=1: the same for the residual pass, whose stamps are in a separate STAMPS instantiation; the production kernel holds none
long long *k4_stamps_buffer(vba_ctx *c) {
  static const bool want_stamps = diag_env("VBA_K4_STAMPS") != nullptr;
  if (!want_stamps) return nullptr;
  static long long *d_st = nullptr;
  if (!d_st) hipMalloc((void **)&d_st, 2048 * 4 * 8);
  hipMemsetAsync(d_st, 0, 2048 * 4 * 8, c->stream);
  return d_st;
}
void k4_stamps_dump(vba_ctx *c, int nb, const long long *d_st) {
  if (!d_st) return;
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

// the cycle table a solve kernel left in LmDev::stamps (bit 16 of the VBA_DEBUG_SOLVE mask): phases, then load+factor per panel
void solve_cycles_dump(const char *kernel, const LmDev *h, int max_panels) {
  if (!(h->pad & 16)) return;
  fprintf(stderr, "[%s cycles] prologue %lld | tile load %lld | factorisation %lld | backsub %lld | epilogue %lld | panels:", kernel, h->stamps[1] - h->stamps[0],
          h->stamps[2] - h->stamps[1], h->stamps[3] - h->stamps[2], h->stamps[4] - h->stamps[3], h->stamps[5] - h->stamps[4]);
  const int npr = (int)h->stamps[6];             // panels run: k_lm_solve_m ends with the panel of the last live pivot, k_li_solve skips those from column n on
  for (int kb = 0; kb < npr && kb < max_panels; kb++) fprintf(stderr, " %lld+%lld", h->stamps[9 + 2 * kb] - h->stamps[8 + 2 * kb], kb < npr - 1 ? h->stamps[10 + 2 * kb] - h->stamps[9 + 2 * kb] : 0LL);
  fprintf(stderr, " | %d panels run\n", npr);
}

// VBA_LI_TIMES=1: host-side phases of one li_ba_device call, and the cycle tables of its kernels (VBA_DEBUG_SOLVE mask bits 16, 32, 64)
struct LiPhases {
  using Clock = std::chrono::steady_clock;
  bool on; Clock::time_point t0; double at[3] = {0, 0, 0};      // at: us since t0 when uploaded, enqueued, drained
  LiPhases() { static const bool want_times = diag_env("VBA_LI_TIMES") != nullptr; on = want_times; if (on) t0 = Clock::now(); }
  double since() const { return std::chrono::duration<double, std::micro>(Clock::now() - t0).count(); }
  void mark(int i) { if (on) at[i] = since(); }
  void report(const vba_ctx *c, const LmDev *hl) const {
    if (!on) return;
    if (hl->pad & 16) fprintf(stderr, "[k_li_solve prologue] stage imu %lld | stage lidar %lld | diag+g %lld | rank %lld\n", hl->stamps[50] - hl->stamps[0], hl->stamps[51] - hl->stamps[50], hl->stamps[52] - hl->stamps[51], hl->stamps[1] - hl->stamps[52]);
    solve_cycles_dump("k_li_solve", hl, 20);
    if (hl->pad & 64) fprintf(stderr, "[k_li_imu cycles] factor algebra (one lane per factor) %lld | cov^-1 joc %lld | contractions %lld\n", hl->stamps[41] - hl->stamps[40], hl->stamps[42] - hl->stamps[41], hl->stamps[43] - hl->stamps[42]);
    if (hl->pad & 32) { double v[6]; std::memcpy(v, &hl->stamps[58], sizeof(v)); fprintf(stderr, "[li r1 parts] rank %d: rimu %.10g lidar %.10g | %.10g %.10g | %.10g %.10g\n", c->rank, v[0], v[1], v[2], v[3], v[4], v[5]); }
    fprintf(stderr, "[li_ba_device] upload %.1f us | enqueue %.1f | gpu drained at %.1f | total %.1f\n", at[0], at[1] - at[0], at[2], since());
  }
};

// What a Hessian launch carries besides the lidar pass: up to three riders; an empty value carries nothing, the makers say which.
struct PassCargo {
  LmDev *lm = nullptr; const double *k4p = nullptr; int k4nb = 0;   // the previous iteration's accept/reject step and its K4 partials
  LiJob li{}; size_t li_lds = 0;                                     // the IMU workgroup of LI-BA and its dynamic LDS
  bool init = false;                                                 // the LM call's pending init (lm_init_arg)
};
PassCargo cargo_pending_update(vba_ctx *c) { PassCargo g; g.lm = c->d_lm; g.k4p = c->d_k4part; g.k4nb = c->lm.k4_nb; return g; }
PassCargo cargo_call_init() { PassCargo g; g.init = true; return g; }
PassCargo cargo_imu_job(vba_ctx *c, size_t lds_imu) { PassCargo g; g.li = LiJob{c->d_lm, c->d_li, c->d_imu, c->d_himu, c->d_gimu}; g.li_lds = lds_imu; return g; }

template <int W>
int launch_hessian2_t(vba_ctx *c, const double *poses_dev, const int *gate, int head, int end, int *nblocks_out, const PassCargo &g) {
  using C = HessCfg2<W>;
  const bool imu = g.li.dev != nullptr;
  const int ntiles = (end - head + C::TV - 1) / C::TV;
  const int maxb = imu ? c->max_blocks_hess - 1 : c->max_blocks_hess;      // (the IMU workgroup of LI-BA takes a CU of its own)
  int nb = ntiles < maxb ? ntiles : maxb;
  if (nb < 1) nb = 1;
  static LdsOptIn opt_in;      // (a lidar-only launch asks for C::LDS_BYTES, one that carries the IMU workgroup for up to kLiRideLds)
  HIPCHK(c, opt_in(c->device, (const void *)k_hessian2<W>, C::LDS_BYTES > kLiRideLds ? C::LDS_BYTES : kLiRideLds));
  long long *stamps = k3_stamps_buffer(c);
  const size_t lds = (imu && g.li_lds > C::LDS_BYTES) ? g.li_lds : C::LDS_BYTES;
  hipLaunchKernelGGL(k_hessian2<W>, dim3(nb + (imu ? 1 : 0)), dim3(C::NT), lds, c->stream, c->fv, poses_dev, head, end, ntiles, c->d_partial, gate, stamps, g.lm, g.k4p, g.k4nb,
                     nb, g.li, lm_init_arg<W>(c, g.init));
  k3_stamps_dump(c, stamps, nb, 15, "");
  *nblocks_out = nb;
  return VBA_OK;
}

template <int W>
int launch_hessian3_t(vba_ctx *c, const double *poses_dev, const int *gate, int *nblocks_out, const PassCargo &g) {
  using C = HessCfg3<W>;
  const bool imu = g.li.dev != nullptr;
  const int nb = imu ? c->max_blocks_hess - 1 : c->max_blocks_hess;      // (the IMU workgroup of LI-BA takes a CU of its own)
  static LdsOptIn opt_in;
  HIPCHK(c, opt_in(c->device, (const void *)k_hessian3<W>, C::LDS_BYTES > kLiRideLds ? C::LDS_BYTES : kLiRideLds));
  const size_t lds = (imu && g.li_lds > C::LDS_BYTES) ? g.li_lds : C::LDS_BYTES;
  long long *stamps = k3_stamps_buffer(c);
  hipLaunchKernelGGL(k_hessian3<W>, dim3(nb + (imu ? 1 : 0)), dim3(C::NT), lds, c->stream, c->fv, poses_dev, c->nvox, c->d_partial, gate, g.lm, g.k4p, g.k4nb, nb, g.li, stamps);
  k3_stamps_dump(c, stamps, nb, 16, "; per workgroup: start, prologue, then per tile [A, B, combine, E]");
  *nblocks_out = nb;
  return VBA_OK;
}

// The init rider travels in k_hessian2 only: the opt-in occupancy-compact pass takes the stand-alone init kernel in front of it.
int launch_hessian(vba_ctx *c, const double *pd, const int *gate, int head, int end, int *nb, const PassCargo &g) {
  // whole store, W <= 10: the occupancy-compact pass (vba_kernels_h3.hpp); sub-ranges and wider windows: the dense-tile pass
  if (head == 0 && end == c->nvox && c->opt.win_size <= 10 && c->use_h3) {
    if (g.init) { const int st = lm_init_flush(c); if (st) return st; }
    return for_window<2, 10>(c->opt.win_size, [&](auto wc) { return launch_hessian3_t<decltype(wc)::value>(c, pd, gate, nb, g); });
  }
  return for_window<2, 16>(c->opt.win_size, [&](auto wc) { return launch_hessian2_t<decltype(wc)::value>(c, pd, gate, head, end, nb, g); });
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

// what launch_residual has decided, and the one launch line of each kernel (VPL: k_residual_v; FUSED: its instance that writes the LM init)
struct ResidualLaunch {
  vba_ctx *c; const double *pd; const int *gate; int head, end; double *part; int nb; long long *stamps; bool init;
  template <int W, bool VPL, bool STAMPS, bool FUSED = false>
  void go() const {
    if constexpr (VPL) hipLaunchKernelGGL((k_residual_v<W, STAMPS, FUSED>), dim3(nb), dim3(64), 0, c->stream, c->fv, pd, head, end, part, gate, stamps, lm_init_arg<W>(c, FUSED));
    else hipLaunchKernelGGL((k_residual_s<W, VBA_K4_TV, STAMPS>), dim3(nb), dim3(ResCfg<W, VBA_K4_TV>::NT), 0, c->stream, c->fv, pd, head, end, part, gate, stamps, lm_init_arg<W>(c, init));
  }
};

// residual pass over voxels [head, end) (end > head); its residual_nb partials (one per workgroup) go to dst or d_partial
int launch_residual(vba_ctx *c, const double *pd, const int *gate, int head, int end, double *dst = nullptr, bool init = false) {
  long long *stamps = k4_stamps_buffer(c);
  if (stamps && init) {                     // (the diagnostic STAMPS instances carry no init: it becomes a launch of its own)
    const int st = lm_init_flush(c);
    if (st) return st;
    init = false;
  }
  const bool vpl = residual_vpl(c, end - head);
  const ResidualLaunch r{c, pd, gate, head, end, dst ? dst : c->d_partial, residual_nb(c, end - head), stamps, init};
  const int st = for_window<2, 16>(c->opt.win_size, [&](auto wc) {
    constexpr int W = decltype(wc)::value;
    if (!vpl) { if (stamps) r.go<W, false, true>(); else r.go<W, false, false>(); }    // the slot-parallel kernel takes the init by argument
    else if (stamps) r.go<W, true, true>();
    else if (init && c->lm_init.pending) r.go<W, true, false, true>();                 // the voxel-per-lane kernel has an instance for it
    else r.go<W, true, false>();
    return VBA_OK;
  });
  if (st == VBA_OK) k4_stamps_dump(c, r.nb, stamps);
  return st;
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
}  // namespace

namespace vba {
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
}  // namespace vba

namespace {

// device passes on device-resident poses (gate == nullptr: unconditional)
int hessian_pass(vba_ctx *c, const double *poses_dev, const int *gate, int head, int end, const PassCargo &g) {
  const int W = c->opt.win_size, nout = nout_tl(W);
  if (end <= head) {
    if (g.init) { const int st = lm_init_flush(c); if (st) return st; }     // (no kernel to carry it)
    HIPCHK(c, hipMemsetAsync(c->d_out, 0, (size_t)nout * sizeof(double), c->stream));
  } else {
    int nb = 0;
    TimedSpan s1{}, s2{};
    span_begin(c, "hessian", s1);
    int st = launch_hessian(c, poses_dev, gate, head, end, &nb, g);
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
    if ((size_t)nb > c->d_partial.n) { c->set_error("partial buffer too small"); return VBA_ERR_CAPACITY; }
    TimedSpan s1{}, s2{};
    span_begin(c, "residual", s1);
    const int st = launch_residual(c, poses_dev, gate, head, end);
    if (st) return st;
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

// Sharded (multi-rank) LM calls, the lidar one and the LI one: ONE collective per iteration.  After the residual pass at the trial
// poses the Hessian pass is run there too (speculating that the step is accepted) and [H | g | r] is all-reduced once: its r (the
// sum of the eigenvalues the residual pass just stored) is the trial residual the accept test needs, and on acceptance H is already
// the next iteration's Hessian; on a reject the solve keeps using its saved copy (`raw`), exactly as VM:443 skips divide_thread.
// So such a call needs a Hessian pass at the head of an iteration only until its first trial step has run:
bool needs_hessian_pass(const vba_ctx *c) { return !(c->collective() && c->lm.have_hess); }
// the trial step; launch_update(r) enqueues the caller's accept/reject kernel on the all-reduced trial residual r (device address)
template <class LaunchUpdate>
int sharded_trial_step(vba_ctx *c, const LmPtrs &p, int V, LaunchUpdate launch_update) {
  int st = VBA_OK;
  if (V > 0) st = launch_residual(c, p.xt, p.run_res, 0, V);   // only_residual VM:467: refreshes the eigen state at the trial poses
  if (!st) st = hessian_pass(c, p.xt, p.run_res, 0, V, PassCargo{});   // speculative divide_thread there + the one all-reduce
  if (st) return st;
  c->lm.have_hess = true;
  launch_update(c->d_out + (nout_tl(c->opt.win_size) - 1));
  return VBA_OK;
}

// tile layout -> full layout [H | g | r] in d_full (host consumers only; the device LM reads the tile layout directly)
int tiles_to_full(vba_ctx *c, const double *src) {
  return for_window<2, 16>(c->opt.win_size, [&](auto wc) {
    hipLaunchKernelGGL(k_tiles_to_full<decltype(wc)::value>, dim3(16), dim3(256), 0, c->stream, src, c->d_full);
    HIPCHK(c, hipGetLastError());
    return VBA_OK;
  });
}

// device: d_full = [H | g | r] over voxels [head,end) for host poses (+ all-reduce across ranks when configured)
int eval_hessian_dev(vba_ctx *c, const double *poses, int head, int end) {
  int st = upload_poses(c, poses);
  if (st) return st;
  st = hessian_pass(c, c->d_poses, nullptr, head, end, PassCargo{});
  if (st) return st;
  return tiles_to_full(c, c->d_out);
}

int eval_residual_dev(vba_ctx *c, const double *poses, int head, int end, double *d_scalar_out) {
  int st = upload_poses(c, poses);
  if (st) return st;
  return residual_pass(c, c->d_poses, nullptr, head, end, d_scalar_out);
}

int ensure_partial(vba_ctx *c, size_t doubles) {
  HIPCHK(c, c->d_partial.ensure(doubles));
  return VBA_OK;
}

// host copies of the reduced device results
int fetch(vba_ctx *c, const double *d_src, size_t n, double *dst) {
  int st = ensure_pin(c, n + kPinFixed);
  if (st) return st;
  double *stage = c->h_pin + kPinStage;  // poses live in the first part
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
  c->lm_trial_fused = opt->lm_trial_launches != 2;
  c->use_h3 = opt->hessian_compact_tiles != 0 && opt->deterministic == 0;   // (k_hessian3 adds into LDS with f64 atomics)
  if (opt->stream) { c->stream = (hipStream_t)opt->stream; c->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return VBA_ERR_HIP; }
    c->own_stream = true;
  }
  if (int r = ctx_sat_create(c)) { vba_destroy(c); return r; }
  const int W = opt->win_size, nout = nout_of(W);
  c->fv.W = W;
  if (c->d_poses.ensure((size_t)VBA_MAX_WIN * 12) != hipSuccess || c->d_out.ensure((size_t)nout_tl(W) + 64) != hipSuccess ||
      c->d_full.ensure((size_t)nout + 64) != hipSuccess || c->d_scal.ensure(64) != hipSuccess) { vba_destroy(c); return VBA_ERR_HIP; }
  if (ensure_partial(c, (size_t)kMaxBlocksHess * (nout_tl(W) > nout ? nout_tl(W) : nout)) != VBA_OK || ensure_pin(c, kPinCreate + (size_t)nout) != VBA_OK) { vba_destroy(c); return VBA_ERR_HIP; }
  if (c->d_lm.ensure(1) != hipSuccess || c->d_raw.ensure((size_t)nout_tl(W) + 64) != hipSuccess || c->h_lm.ensure(1) != hipSuccess) { vba_destroy(c); return VBA_ERR_HIP; }
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
  for (vba_ctx *w : c->hba_workers) vba_destroy(w);
  c->hba_workers.clear();
  ctx_sat_release(c);      // the satellites' buffers and events (vba_sat.hpp)
  for (auto &kv : c->spans) for (auto &s : kv.second) { hipEventDestroy(s.a); hipEventDestroy(s.b); }
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  delete c;      // the buffers free themselves here (vba_mem.hpp), after the stream has been drained
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
  double *d = (double *)c->d_stage.p;
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
  double *d = (double *)c->d_stage.p;
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
  hipLaunchKernelGGL(k_count_slots, dim3(512), dim3(256), 0, c->stream, c->fv, c->nvox, (unsigned long long *)c->d_stage.p);
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
    int st = ensure_pin(c, kPinFixed);
    if (st) return st;
    double *h_count = c->h_pin + kPinCount, *d_count = c->d_scal + kScalCount;
    *h_count = (double)c->nvox;
    HIPCHK(c, hipMemcpyAsync(d_count, h_count, sizeof(double), hipMemcpyHostToDevice, c->stream));
    st = ctx_allreduce(c, d_count, 1);
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyAsync(h_count, d_count, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->nvox_global = (int)(*h_count + 0.5);
  }
  return VBA_OK;
}

// Re-creates the per-voxel eigen state (eig_values / eig_vectors / pcr_adds) at the poses loaded by vba_lm_begin: one
// residual pass on the device, nothing is fetched.  In the reference this state comes from recut/tras_opt right before
// damping_iter (VM:1628); a caller that restarts the optimiser on an unchanged factor store uses this instead.
int vba_lm_refresh_eigen(vba_ctx *c) {
  if (!c->lm.active) return VBA_ERR_BAD_ARG;
  if (c->nvox <= 0) return VBA_OK;
  // only the pass' side effect is wanted (eig_values / eig_vectors / pcr_adds at the begin poses): its partials are not summed
  if ((size_t)residual_nb(c, c->nvox) > c->d_partial.n) { c->set_error("partial buffer too small"); return VBA_ERR_CAPACITY; }
  TimedSpan s1{};
  span_begin(c, "residual", s1);
  // single-rank: the pass carries the call's init when it is the first LM kernel; the multi-rank flow takes the stand-alone init
  const bool fuse_init = !c->collective();
  if (!fuse_init) { const int st = lm_init_flush(c); if (st) return st; }
  const int st = launch_residual(c, lm_ptrs(c).x, nullptr, 0, c->nvox, nullptr, fuse_init);
  if (st) return st;
  span_end(c, "residual", s1);
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}

int vba_timing_launch_hessian(vba_ctx *c) {
  if (!c->lm.active || c->nvox <= 0) return VBA_ERR_BAD_ARG;
  int nb = 0;
  int st = lm_init_flush(c);
  if (st) return st;
  st = launch_hessian(c, lm_ptrs(c).x, nullptr, 0, c->nvox, &nb, PassCargo{});
  if (st) return st;
  HIPCHK(c, hipGetLastError());
  return VBA_OK;
}

// k_lm_trial (vba_kernels_lm.hpp) takes the place of the solve + residual pair of a single-rank iteration where its workgroups can all be
// resident beside the solve.  Windows whose instance would not fit three workgroups of a CU's registers and LDS keep the two launches
// (LmTrialFits, from the kernel's resource usage: DESIGN.md 5), and so do the multi-rank flow, stores the voxel-per-lane residual kernel
// serves, an empty store, the diagnostic stamp instances and contexts created with vba_options::lm_trial_launches = 2.
extern "C++" {
template <int W>
struct LmTrialFits { static constexpr bool value = sizeof(typename LmTrialCfg<W, VBA_K4_TV>::Lds) + 16 <= 160 * 1024 / 3 && LmTrialCfg<W, VBA_K4_TV>::BS <= 320; };
static bool lm_trial_fused(vba_ctx *c, int V, int nb, int copy_raw) {
  if (!c->lm_trial_fused || copy_raw || V <= 0 || residual_vpl(c, V) || c->lm_init.dbg != 0 || k4_stamps_buffer(c)) return false;
  bool fits = false;
  for_window<2, 16>(c->opt.win_size, [&](auto wc) { fits = LmTrialFits<decltype(wc)::value>::value; return VBA_OK; });
  if (!fits) return false;
  // every workgroup resident at once: three per CU (registers and LDS, above) on the device's CUs
  static std::atomic<int> cus[kMaxDevices] = {};
  const bool known = c->device >= 0 && c->device < kMaxDevices;
  int n = known ? cus[c->device].load(std::memory_order_relaxed) : 0;
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || n <= 0) return false;
    if (known) cus[c->device].store(n, std::memory_order_relaxed);
  }
  return c->lm_spec + nb <= 3 * n;
}
// The fetched LmDev image says whether a rider of k_lm_trial gave up its bounded wait (it never should): the call that fetched it fails.
static bool lm_trial_fault_seen(vba_ctx *c) {
  if (c->h_lm->trial_fault == 0) return false;
  c->set_error("k_lm_trial: a residual workgroup gave up waiting for the solve's trial poses (the step was rejected)");
  return true;
}
}  // extern "C++"

// One trip through the loop body VM:441-494, enqueued without host synchronisation unless the caller asks for the flags.
int vba_lm_iterate(vba_ctx *c, int *accepted, int *stop) {
  if (!c->lm.active) return VBA_ERR_BAD_ARG;
  const int W = c->opt.win_size, nout = nout_of(W), V = c->nvox;
  if (c->nvox_global < c->lm.thd_num) { c->lm_init.pending = false; return VBA_ERR_TOO_FEW_VOXELS; }   // VM:399-403 (and g_size checks of VM:367); the same on every rank
  const LmPtrs p = lm_ptrs(c);
  const int copy_raw = c->collective() ? 1 : 0;      // multi-rank: one collective per iteration (sharded_trial_step)
  int st = VBA_OK;
  static const bool no_fuse = diag_env("VBA_NO_FUSED_UPDATE") != nullptr;   // diagnostic: accept/reject always as its own kernel
  if (copy_raw) { st = lm_init_flush(c); if (st) return st; }               // the multi-rank flow takes the stand-alone init
  if (needs_hessian_pass(c)) {
    // divide_thread  VM:445 (skipped on device after a reject); carries the previous iteration's accept/reject (and then runs on xt after an accepted step), else the call's init
    st = hessian_pass(c, p.x, p.run_hess, 0, V, c->lm.pending_update ? cargo_pending_update(c) : cargo_call_init());
    c->lm.pending_update = false;
  }
  if (st) return st;
  const int nb = residual_nb(c, V);
  if (!copy_raw && (size_t)nb > c->d_k4part.n) {
    if (c->d_k4part) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_k4part.ensure(nb > 65536 ? 2 * (size_t)nb : 65536));
  }
  const bool fused_trial = lm_trial_fused(c, V, nb, copy_raw);
  TimedSpan sp{};
  span_begin(c, "solve", sp);        // (the fused launch is bracketed as "solve": "residual" spans then cover stand-alone passes only)
  st = for_window<2, 16>(W, [&](auto wc) {
    constexpr int WW = decltype(wc)::value;
    if (fused_trial) {
      if constexpr (LmTrialFits<WW>::value)
        hipLaunchKernelGGL((k_lm_trial<WW, false, VBA_K4_TV>), dim3(c->lm_spec + nb), dim3(LmTrialCfg<WW, VBA_K4_TV>::BS), 0, c->stream, c->d_lm, c->d_out, c->d_raw, c->lm_spec,
                           c->fv, 0, V, c->d_k4part.p);
    }
    else if (copy_raw) hipLaunchKernelGGL((k_lm_solve_m<WW, true>), dim3(c->lm_spec), dim3(256), 0, c->stream, c->d_lm, c->d_out, c->d_raw, nullptr);
    else hipLaunchKernelGGL((k_lm_solve_m<WW, false>), dim3(c->lm_spec), dim3(256), 0, c->stream, c->d_lm, c->d_out, c->d_raw, nullptr);
    return VBA_OK;
  });
  if (st) return st;
  span_end(c, "solve", sp);
  if (copy_raw) {
    st = sharded_trial_step(c, p, V, [&](const double *r) { hipLaunchKernelGGL(k_lm_update, dim3(1), dim3(64), 0, c->stream, c->d_lm, r, 0, W); });
    if (st) return st;
  } else {
    const bool fuse = !no_fuse && !(accepted || stop);
    if (!fused_trial) {
      TimedSpan s1{};
      span_begin(c, "residual", s1);
      st = launch_residual(c, p.xt, p.run_res, 0, V, c->d_k4part);
      if (st) return st;
      span_end(c, "residual", s1);
    }
    if (fuse) { c->lm.pending_update = true; c->lm.k4_nb = nb; }
    else hipLaunchKernelGGL(k_lm_update, dim3(1), dim3(64), 0, c->stream, c->d_lm, c->d_k4part, nb, W);   // sums the partials itself
  }
  HIPCHK(c, hipGetLastError());
  if (accepted || stop) {
    HIPCHK(c, hipMemcpyAsync(c->h_lm, c->d_lm, sizeof(LmDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (accepted) *accepted = c->h_lm->last_accepted;
    if (stop) *stop = c->h_lm->stop;
    if (lm_trial_fault_seen(c)) return VBA_ERR_HIP;
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
    st = ensure_pin(c, kPinCreate + (size_t)n * n);
    if (st) return st;
    h_hess = c->h_pin + kPinStage;
  }
  const double *src = c->collective() ? c->d_raw : c->d_out;      // *hess = Hess before gauge fixing (VM:446)
  const int upd = c->lm.pending_update ? 1 : 0;
  st = for_window<2, 16>(W, [&](auto wc) {
    hipLaunchKernelGGL(k_lm_finish<decltype(wc)::value>, dim3(hess ? 17 : 1), dim3(256), 0, c->stream, c->d_lm, c->d_k4part, upd ? c->lm.k4_nb : 0, upd, c->h_lm, src, h_hess);
    return VBA_OK;
  });
  if (st) return st;
  c->lm.pending_update = false;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const LmDev *h = c->h_lm;
  if (poses) std::memcpy(poses, h->x, (size_t)W * 12 * sizeof(double));
  if (hess) std::memcpy(hess, h_hess, (size_t)n * n * sizeof(double));
  if (resis2) { resis2[0] = h->resis_first; resis2[1] = h->r2; }
  c->trace.assign(h->trace, h->trace + 5 * h->n_trace);
  solve_cycles_dump("k_lm_solve_m", h, 8);
  c->lm.active = false;
  if (lm_trial_fault_seen(c)) return VBA_ERR_HIP;
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
  static LdsOptIn opt_in;
  HIPCHK(c, opt_in(c->device, (const void *)k_li_solve<W, NT, GL>, lds));
  if (GL && c->d_liscr.n < l_doubles * LM_SPEC) {           // one region per damping candidate; W is fixed per context, so this runs once
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_liscr.ensure(l_doubles * LM_SPEC));
  }
  hipLaunchKernelGGL((k_li_solve<W, NT, GL>), dim3(c->lm_spec), dim3(NT), lds, c->stream, c->d_lm, c->d_li, c->d_out, c->d_raw, copy_raw, c->d_himu, c->d_gimu, c->d_imu, n, gauge, grav,
                     c->opt.imu_coef, c->d_liscr, nullptr);
  return VBA_OK;
}
namespace vba {
bool li_device_supported(int W) { return W >= 2 && W <= LI_MAX_W; }
}
}  // extern "C++"

// dynamic LDS of li_imu_body (joc, cov^-1 joc, rr, cov^-1 rr, the per-factor scalars)
static size_t li_imu_lds(int F, int nb) { return ((size_t)2 * F * 15 * nb + 2 * F * 15 + F + 16) * sizeof(double); }
// Set-up shared by li_ba_device and vba_debug_li_imu: device buffers, the LM state (poses view of `states`, flushed), LiDev `h`, the
// factor image `fimg` (= imus with cov^-1 in place of cov) uploaded, himu / gimu cleared, the LDS ceiling of k_li_imu.
static int li_setup(vba_ctx *c, const double *states, const double *imus, int gravity, LiDev &h, std::vector<double> &fimg) {
  const int W = c->opt.win_size, DIM = VBA_DIM, F = W - 1;
  const int n = W * DIM + (gravity ? 3 : 0), nb = gravity ? 33 : 30;
  if (!c->d_li) {
    HIPCHK(c, c->d_li.ensure(1));
    HIPCHK(c, c->d_imu.ensure((size_t)LI_MAX_W * 304));
    HIPCHK(c, c->d_himu.ensure((size_t)LI_MAX_N * LI_MAX_N));
    HIPCHK(c, c->d_gimu.ensure((size_t)LI_MAX_N));
  }
  // upload: LM state (poses view), the IMU extras, the factors with cov^-1 in place of cov
  std::vector<double> poses((size_t)W * 12);
  states_to_poses(states, W, poses.data());
  int st = vba_lm_begin(c, poses.data(), 0);
  if (st) return st;
  st = lm_init_flush(c);                      // the LI-BA kernels read the LM state from their first launch on
  if (st) return st;
  h = LiDev{};
  h.W = W; h.n = n; h.nb = nb; h.gravity = gravity ? 1 : 0; h.gauge = gravity ? 6 : DIM; h.F = F; h.imu_coef = c->opt.imu_coef;   // VM:653-656 / 906-909
  for (int i = 0; i < W; i++) {
    const double *sx = states + 25 * i;
    h.tstamp[i] = sx[0];
    for (int k = 0; k < 12; k++) h.ex[12 * i + k] = h.ext[12 * i + k] = sx[13 + k];
  }
  fimg.resize((size_t)F * 304);
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
  static LdsOptIn opt_in;      // W = 10 with gravity: 88 KB
  HIPCHK(c, opt_in(c->device, (const void *)k_li_imu, li_imu_lds(LI_MAX_W - 1, 33)));
  return VBA_OK;
}
// the IMU pass rides the lidar Hessian launch when there is one on this rank and its LDS fits beside it
static bool li_imu_rides(const vba_ctx *c, int V, size_t lds_imu) { return needs_hessian_pass(c) && V > 0 && lds_imu <= kLiRideLds; }

static int li_ba_device(vba_ctx *c, double *states, double *imus, int gravity, int max_iter, double *hess, double *resis2) {
  LiPhases phases;                                                     // diagnostic: host-side phases of one call
  const int W = c->opt.win_size, V = c->nvox, DIM = VBA_DIM, F = W - 1;
  const int n = W * DIM + (gravity ? 3 : 0), nb = gravity ? 33 : 30, n6 = 6 * W;
  if (!gravity) max_iter = 3;                                         // VM:643
  LiDev h{};
  std::vector<double> fimg;
  int st = li_setup(c, states, imus, gravity, h, fimg);
  if (st) return st;
  const LmPtrs p = lm_ptrs(c);
  const int copy_raw = c->collective() ? 1 : 0;
  const size_t lds_imu = li_imu_lds(F, nb);
  phases.mark(0);
  for (int it = 0; it < max_iter; it++) {
    // The IMU factors' workgroup rides in the lidar Hessian launch as block 0 on a CU of its own (k_hessian2).  As a kernel of its own
    // in front of the lidar pass it cost its 28 us + a kernel boundary; on a side stream (fork / join events around it) the two
    // cross-stream dependencies cost more than they hid (209 vs 196 us per iteration).
    if (li_imu_rides(c, V, lds_imu)) {
      st = hessian_pass(c, p.x, p.run_hess, 0, V, cargo_imu_job(c, lds_imu));   // lidar part of divide_thread (+ all-reduce)
    } else {
      hipLaunchKernelGGL(k_li_imu, dim3(1), dim3(LI_IMU_NT), lds_imu, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_himu, c->d_gimu);
      if (needs_hessian_pass(c)) st = hessian_pass(c, p.x, p.run_hess, 0, V, PassCargo{});
    }
    if (st) return st;
    TimedSpan s1{};
    span_begin(c, "solve", s1);
    st = for_window<2, 16>(W, [&](auto wc) {
      constexpr int WW = decltype(wc)::value;
      if constexpr (WW == 10) {
        static const int nt = diag_env("VBA_LI_NT") ? atoi(diag_env("VBA_LI_NT")) : 512;      // -DVBA_DIAG builds only
        if (nt == 256) return launch_li_solve<10, 256>(c, copy_raw, n, h.gauge, h.gravity);
        if (nt == 1024) return launch_li_solve<10, 1024>(c, copy_raw, n, h.gauge, h.gravity);
      }
      return launch_li_solve<WW>(c, copy_raw, n, h.gauge, h.gravity);
    });
    span_end(c, "solve", s1);
    if (st) return st;                                                // (the opt-in or the scratch allocation of the W > 10 solve failed: nothing was launched)
    if (copy_raw) {                                                   // one collective per iteration
      st = sharded_trial_step(c, p, V, [&](const double *r) { hipLaunchKernelGGL(k_li_update, dim3(1), dim3(LI_UPD_NT), 0, c->stream, c->d_lm, c->d_li, c->d_imu, r, 0); });
      if (st) return st;
    } else if (V == 0) {
      st = residual_pass(c, p.xt, p.run_res, 0, V, c->d_scal);
      if (st) return st;
      hipLaunchKernelGGL(k_li_update, dim3(1), dim3(LI_UPD_NT), 0, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_scal, 0);
    } else {
      const int nbk = residual_nb(c, V);
      TimedSpan s2{};
      span_begin(c, "residual", s2);
      st = launch_residual(c, p.xt, p.run_res, 0, V);
      if (st) return st;
      span_end(c, "residual", s2);
      hipLaunchKernelGGL(k_li_update, dim3(1), dim3(LI_UPD_NT), 0, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_partial, nbk);
    }
    HIPCHK(c, hipGetLastError());
  }
  phases.mark(1);
  // (no drain before the download: with everything packed into ONE copy, queueing it behind the kernels is as fast as draining
  //  first — 497 vs 503 us per call; with five separate copies draining first had been 2-3x faster)
  phases.mark(2);
  // download: accepted state, the factors' bias increments, trace, and (on request) *hess = Hess before gauge fixing —
  // everything lands in ONE pinned block (pageable destinations make every copy a blocking staged transfer)
  // — gathered on the device into one block first: five separate D2H copies cost ~20 us each (110 us per call, measured)
  static_assert(sizeof(LiDev) % 8 == 0 && sizeof(LmDev) % 8 == 0, "packed as doubles");
  // The block is packed from offset 0 of h_pin and overlays the fixed regions (vba_ctx.hpp): nothing of them is in flight after li_setup (the
  // count's round trip ends in a synchronise, every pose upload is followed by a fetch, which drains) and this call uses none of them.
  const size_t o_li = 0, o_img = o_li + sizeof(LiDev) / 8, o_hb = o_img + fimg.size(), o_lid = o_hb + (size_t)li_hb_size(W, 1),
               o_lm = o_lid + (size_t)n6 * n6, o_end = o_lm + sizeof(LmDev) / 8;
  st = ensure_pin(c, o_end + 64);
  if (st) return st;
  HIPCHK(c, c->d_lipack.ensure(o_end + 64));
  PackSegs segs{};
  segs.n = 3;
  segs.src[0] = (const double *)c->d_li.p; segs.off[0] = o_li; segs.len[0] = sizeof(LiDev) / 8;
  segs.src[1] = c->d_imu; segs.off[1] = o_img; segs.len[1] = fimg.size();
  segs.src[2] = (const double *)c->d_lm.p; segs.off[2] = o_lm; segs.len[2] = sizeof(LmDev) / 8;
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
  phases.report(c, hl);
  return VBA_OK;
}

// ---------------------------------------------------------------- LI_BA_Optimizer / LI_BA_OptimizerGravity (VM:504-976)
int vba_li_ba_damping_iter(vba_ctx *c, double *states, double *imus, int gravity, int max_iter, double *hess, double *resis2) {
  // the whole optimiser runs on the device (k_li_imu / k_li_solve / k_li_update) for every window the context accepts (2..16)
  if (!li_device_supported(c->opt.win_size)) return VBA_ERR_UNSUPPORTED_WINDOW;
  const int st = li_ba_device(c, states, imus, gravity, max_iter, hess, resis2);
  if (st) c->lm.active = false;                 // (li_setup began an LM call; a success has ended it)
  return st;
}

// ---------------------------------------------------------------- diagnostic: the IMU factor pass through the production kernels
static int debug_li_imu_run(vba_ctx *c, int gravity, int flags, const double *states, const double *imus, double *h_dense, double *g, double *rimu,
                            double *covinv_out) {
  const int W = c->opt.win_size, V = c->nvox, F = W - 1, n = 15 * W + (gravity ? 3 : 0), nb = gravity ? 33 : 30;
  LiDev h{};
  std::vector<double> fimg;
  int st = li_setup(c, states, imus, gravity, h, fimg);
  if (st) return st;
  const LmPtrs p = lm_ptrs(c);
  const size_t lds_imu = li_imu_lds(F, nb);
  if (flags & (VBA_IMU_RIDE_H2 | VBA_IMU_RIDE_H3)) {
    st = hessian_pass(c, p.x, p.run_hess, 0, V, cargo_imu_job(c, lds_imu));
    if (st) return st;
  } else {
    hipLaunchKernelGGL(k_li_imu, dim3(1), dim3(LI_IMU_NT), lds_imu, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_himu, c->d_gimu);
  }
  HIPCHK(c, hipGetLastError());
  if (flags & VBA_IMU_TRIAL) {      // xt = x and ext = ex hold the caller's states (li_setup); r2 = 0, r1 = q1 = 0: the bookkeeping has nothing to decide
    HIPCHK(c, hipMemsetAsync(c->d_scal, 0, sizeof(double), c->stream));
    hipLaunchKernelGGL(k_li_update, dim3(1), dim3(LI_UPD_NT), 0, c->stream, c->d_lm, c->d_li, c->d_imu, c->d_scal, 0);
    HIPCHK(c, hipGetLastError());
  }
  std::vector<double> hb((size_t)li_hb_size(W, gravity));
  hipError_t e = hipMemcpyAsync(hb.data(), c->d_himu, hb.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(g, c->d_gimu, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&h, c->d_li, sizeof(LiDev), hipMemcpyDeviceToHost, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);      // (always drained: the destinations are locals of this call)
  HIPCHK(c, e);
  HIPCHK(c, es);
  for (int r = 0; r < n; r++)
    for (int k = 0; k < n; k++) h_dense[(size_t)r * n + k] = li_hb_get(hb.data(), W, n, r, k);
  rimu[0] = h.rimu[0];
  rimu[1] = (flags & VBA_IMU_TRIAL) ? h.rimu[1] : 0.0;
  if (covinv_out)
    for (int f = 0; f < F; f++) std::memcpy(covinv_out + 225 * (size_t)f, fimg.data() + 304 * (size_t)f + 79, 225 * sizeof(double));
  return VBA_OK;
}
int vba_debug_li_imu(vba_ctx *c, int W, int gravity, int flags, const double *states, const double *imus, double *h_dense, double *g, double *rimu,
                     double *covinv_out) {
  if (!c || !states || !imus || !h_dense || !g || !rimu) return VBA_ERR_BAD_ARG;
  if (W != c->opt.win_size || !li_device_supported(W) || (gravity != 0 && gravity != 1)) return VBA_ERR_BAD_ARG;
  if (flags & ~(VBA_IMU_RIDE_H2 | VBA_IMU_RIDE_H3 | VBA_IMU_TRIAL)) return VBA_ERR_BAD_ARG;
  const bool h2 = (flags & VBA_IMU_RIDE_H2) != 0, h3 = (flags & VBA_IMU_RIDE_H3) != 0;
  if (h2 && h3) return VBA_ERR_BAD_ARG;
  if (c->collective()) return VBA_ERR_UNSUPPORTED;
  if (h2 || h3) {
    // the riding forms need a pushed store, and the lidar kernel is the one the context selects for it (launch_hessian)
    const bool ctx_h3 = c->use_h3 && W <= 10;
    if (c->nvox <= 0 || h3 != ctx_h3) return VBA_ERR_BAD_ARG;
    if (!li_imu_rides(c, c->nvox, li_imu_lds(W - 1, gravity ? 33 : 30))) return VBA_ERR_BAD_ARG;
  }
  for (size_t i = 0; i < (size_t)25 * W; i++) if (!std::isfinite(states[i])) return VBA_ERR_BAD_ARG;
  for (size_t i = 0; i < (size_t)304 * (W - 1); i++) if (!std::isfinite(imus[i])) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const int st = debug_li_imu_run(c, gravity, flags, states, imus, h_dense, g, rimu, covinv_out);
  if (st) hipStreamSynchronize(c->stream);       // (nothing of this call is left in flight behind a status)
  c->lm_init.pending = false;
  c->lm.active = false;
  return st;
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
  DevMem<char> mem;                             // freed at scope exit, after the synchronise
  HIPCHK(c, mem.ensure(nblk * 256 * 128 + 64));
  double *buf = (double *)mem.p;
  HIPCHK(c, hipMemsetAsync(buf, 0, nblk * 256 * 128 + 64, c->stream));
  hipLaunchKernelGGL(k_calib_read8, dim3((unsigned)nblk), dim3(256), 0, c->stream, buf, buf + nblk * 256 * 16);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
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
int vba_map_dump_leaves(vba_ctx *c, double *out, int max_leaves) { return map_dump_leaves(c->map, c->stream, out, max_leaves, c->err); }
int vba_map_dump_plane_var(vba_ctx *c, double *out, int max_leaves) { return map_dump_plane_var(c->map, c->stream, out, max_leaves, c->err); }
// diagnostic: plane_update_dev on caller-supplied leaves (include/voxelba.h); the context's map is not touched
int vba_debug_plane_update(vba_ctx *c, int n, const double *in, double *out) {
  if (!c || !in || !out || n < 1 || n > (1 << 20)) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return map_debug_plane_update(c->stream, n, in, out, c->err);
}

}  // extern "C"
extern "C" {

// ---------------------------------------------------------------- diagnostic: one LM linear solve through the production kernels
// The caller's system is written into the buffers the solve kernel reads, in their production layout, and the kernel is launched
// as the LM loop launches it (lm_spec workgroups); every buffer belongs to this call, so the context's LM state is untouched.
extern "C++" {
namespace {
struct DbgBufs {                      // device buffers of one call; drained and freed on every exit path
  hipStream_t st;
  std::vector<DevMem<char>> p;
  explicit DbgBufs(hipStream_t s) : st(s) {}
  ~DbgBufs() { if (!p.empty()) hipStreamSynchronize(st); }      // the blocks free themselves after the drain
  template <typename T> hipError_t alloc(T **out, size_t count) {
    DevMem<char> q;
    const hipError_t e = q.ensure((count ? count : 1) * sizeof(T));
    if (e == hipSuccess) { *out = (T *)q.p; p.push_back(std::move(q)); }
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
    static LdsOptIn opt_in;
    HIPCHK(c, opt_in(c->device, (const void *)k_li_solve<W, NT, LC::GL, true>, LC::lds));
    hipLaunchKernelGGL((k_li_solve<W, NT, LC::GL, true>), dim3(c->lm_spec), dim3(NT), LC::lds, c->stream, s, d_li, red, raw, copy_raw, himu, gimu, imu, n, gauge, grav,
                       1.0, scr, d_dx);
  } else {
    static LdsOptIn opt_in;
    HIPCHK(c, opt_in(c->device, (const void *)k_li_solve<W, NT, LC::GL>, LC::lds));
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
  const int st = for_window<2, 16>(W, [&](auto wc) {
    constexpr int WW = decltype(wc)::value;
    return kind == VBA_SOLVE_LIDAR ? dbg_lidar<WW>(c, B, H, g, flags, *h, d_dx) : dbg_li<WW>(c, B, H, g, flags, *h, d_dx);
  });
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(dx, d_dx, (size_t)ncand * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < ncand; b++) q1[b] = h->q1_spec[b];
  return VBA_OK;
}

}  // extern "C"
