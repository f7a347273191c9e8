// Pose-graph optimisation of libvoxelba.so (vba_pgo_optimize): host driver of the kernels in vba_kernels_pgo.hpp; the dense
// skeleton system is factorised by the k_bigl_* kernels that the BA core compiles (declared in vba_ctx.hpp).  The host plan is
// vba_pgo_plan.hpp; pgo_prepare uploads it, pgo_update launches one update.  vba_debug_pgo_step runs the same two with U = 1 and reads
// back what each pass left ("What pins the pose-graph passes").
#include "vba_ctx.hpp"
#include "vba_sat.hpp"
#include "vba_kernels_pgo.hpp"
#include "vba_pgo_plan.hpp"

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <map>
#include <functional>
#include <algorithm>

using namespace vba;

namespace {

bool pgo_args_ok(vba_ctx *c, int n, const double *poses, int m, const double *edges, int n_prior, const double *priors) {
  return c && n >= 1 && poses && m >= 0 && n_prior >= 0 && (m == 0 || edges) && (n_prior == 0 || priors);
}

// The plan of the caller's graph, the context's grow-only buffers sized for it, every table uploaded and the result words cleared.
// v is ready for pgo_update(c, v, 0 .. U - 1); o_res is the offset of cost[U] | mx[U] | cnt[U] | status in c->sat->pgo.d.
int pgo_prepare(vba_ctx *c, int n, const double *poses, int m, const double *edges, int n_prior, const double *priors, int U,
                double relin_threshold, PgoPlan &P, PgoView &v, size_t &o_res) {
  std::string perr;
  const int pr = pgo_plan(n, poses, m, edges, n_prior, priors, P, perr);
  if (pr == PGO_PLAN_BAD_ARG) return VBA_ERR_BAD_ARG;
  if (pr == PGO_PLAN_SINGULAR) { c->set_error(perr); return VBA_ERR_SINGULAR; }
  const int F = P.F, NB = P.NB, S = P.S, LS = P.LS, K = P.K, NSB = P.NSB, NP = P.NP, ld = P.ld;
  // ---- device memory: one grow-only arena for the structure and work areas, one for the dense skeleton system
  size_t bytes = 0;
  auto take = [&](size_t b) { const size_t o = bytes; bytes += (b + 255) & ~(size_t)255; return o; };
  const size_t o_theta = take((size_t)n * 96), o_fz = take((size_t)F * 144), o_fi = take((size_t)F * 4), o_fj = take((size_t)F * 4),
      o_slot = take((size_t)F * PGO_SLOT * 8), o_blk = take((size_t)NB * 288), o_g = take((size_t)n * 48),
      o_blkoff = take((size_t)(NB + 1) * 4), o_blkent = take(P.blk_ent.size() * 4), o_segoff = take(P.seg_off.size() * 4),
      o_segnodes = take((size_t)LS * 4), o_segatt = take((size_t)S * 8), o_sege = take((size_t)S * 4), o_segc = take((size_t)LS * 4),
      o_segY = take((size_t)LS * PGO_Y * 8), o_segout = take((size_t)S * PGO_SEGOUT * 8), o_skel = take((size_t)K * 4),
      o_sbpq = take((size_t)NSB * 8), o_sbbase = take((size_t)NSB * 4), o_sboff = take(P.sb_off.size() * 4), o_sbent = take(P.sb_ent.size() * 4),
      o_dx = take((size_t)n * 48);
  o_res = take((size_t)U * 24 + 8);   // cost[U] | mx[U] | cnt[U] | status
  HIPCHK(c, hipSetDevice(c->device));
  // grow-only buffers owned by the context; a size the device cannot hold is VBA_ERR_CAPACITY (the old buffer is released first)
  auto grow = [&](auto &buf, size_t want, const char *what) -> int {            // want: bytes
    if (want <= buf.n * sizeof(*buf.p)) return VBA_OK;
    if (buf) { HIPCHK(c, hipStreamSynchronize(c->stream)); buf.reset(); }
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const hipError_t e = want > fr ? hipErrorOutOfMemory : buf.ensure(want / sizeof(*buf.p));
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();                      // a refused allocation must not surface in a later call's error check
      c->set_error(std::string("vba_pgo_optimize: the ") + what + " needs " + std::to_string(want) + " bytes, " + std::to_string(fr) + " free");
      return VBA_ERR_CAPACITY;
    }
    HIPCHK(c, e);
    return VBA_OK;
  };
  const size_t abytes = ((size_t)(NP + 1) * ld + (size_t)(NP + 1) * 8) * 8;
  if (int r = grow(c->sat->pgo.d, bytes, "graph structure")) return r;
  if (int r = grow(c->sat->pgo.d_Ab, abytes, "dense skeleton system (8 (6K)^2 bytes)")) return r;
  char *d = c->sat->pgo.d;
  v = PgoView{};
  v.n = n; v.F = F; v.NB = NB; v.S = S; v.K = K; v.NSB = NSB; v.U = U; v.NP = NP; v.ld = ld; v.thr = relin_threshold;
  v.theta = (double *)(d + o_theta); v.fz = (const double *)(d + o_fz); v.fi = (const int *)(d + o_fi); v.fj = (const int *)(d + o_fj);
  v.slot = (double *)(d + o_slot); v.blk = (double *)(d + o_blk); v.g = (double *)(d + o_g);
  v.blk_off = (const int *)(d + o_blkoff); v.blk_ent = (const int *)(d + o_blkent);
  v.seg_off = (const int *)(d + o_segoff); v.seg_nodes = (const int *)(d + o_segnodes); v.seg_att = (const int *)(d + o_segatt);
  v.seg_ecode = (const int *)(d + o_sege); v.seg_ccode = (const int *)(d + o_segc); v.segY = (double *)(d + o_segY);
  v.segout = (double *)(d + o_segout); v.skel_node = (const int *)(d + o_skel); v.sb_pq = (const int *)(d + o_sbpq);
  v.sb_base = (const int *)(d + o_sbbase); v.sb_off = (const int *)(d + o_sboff); v.sb_ent = (const int *)(d + o_sbent);
  v.Ab = c->sat->pgo.d_Ab; v.Tb = c->sat->pgo.d_Ab + (size_t)(NP + 1) * ld; v.dx = (double *)(d + o_dx);
  v.cost = (double *)(d + o_res); v.mx = (unsigned long long *)(d + o_res + (size_t)U * 8); v.cnt = (int *)(d + o_res + (size_t)U * 16);
  v.status = (int *)(d + o_res + (size_t)U * 20);
  hipStream_t st = c->stream;
  // the sources are pageable memory of the caller and of the plan: on a failed copy the stream is drained before anything goes out of scope
  hipError_t ue = hipSuccess;
  auto up = [&](size_t off, const void *src, size_t b) { if (ue == hipSuccess && b) ue = hipMemcpyAsync(d + off, src, b, hipMemcpyHostToDevice, st); };
  up(o_theta, poses, (size_t)n * 96);
  up(o_fz, P.fz.data(), P.fz.size() * 8); up(o_fi, P.fi.data(), (size_t)F * 4); up(o_fj, P.fj.data(), (size_t)F * 4);
  up(o_blkoff, P.blk_off.data(), P.blk_off.size() * 4); up(o_blkent, P.blk_ent.data(), P.blk_ent.size() * 4);
  up(o_segoff, P.seg_off.data(), P.seg_off.size() * 4); up(o_segnodes, P.seg_nodes.data(), (size_t)LS * 4);
  up(o_segatt, P.seg_att.data(), (size_t)S * 8); up(o_sege, P.seg_ecode.data(), (size_t)S * 4);
  up(o_segc, P.seg_ccode.data(), (size_t)LS * 4); up(o_skel, P.skel_node.data(), (size_t)K * 4);
  up(o_sbpq, P.sb_pq.data(), (size_t)NSB * 8); up(o_sbbase, P.sb_base.data(), (size_t)NSB * 4);
  up(o_sboff, P.sb_off.data(), P.sb_off.size() * 4); up(o_sbent, P.sb_ent.data(), P.sb_ent.size() * 4);
  if (ue != hipSuccess) { hipStreamSynchronize(st); HIPCHK(c, ue); }
  HIPCHK(c, hipMemsetAsync(d + o_res, 0, (size_t)U * 24 + 8, st));
  return VBA_OK;
}

// The launches of update u
void pgo_update(vba_ctx *c, const PgoView &v, int u) {
  hipStream_t st = c->stream;
  const int F = v.F, NB = v.NB, S = v.S, K = v.K, NSB = v.NSB, NP = v.NP, ld = v.ld, n = v.n, n6 = 6 * v.K;
  auto grid = [](long long cnt, int bs) { return dim3((unsigned)((cnt + bs - 1) / bs)); };
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

}  // namespace

extern "C" {

// ---------------------------------------------------------------- pose-graph optimisation (vba_kernels_pgo.hpp)
int vba_pgo_optimize(vba_ctx *c, int n, double *poses, int m, const double *edges, int n_prior, const double *priors, int n_updates,
                     double relin_threshold, double *stats) {
  if (!pgo_args_ok(c, n, poses, m, edges, n_prior, priors) || n_updates < 1 || !(relin_threshold >= 0.0) || !std::isfinite(relin_threshold))
    return VBA_ERR_BAD_ARG;
  const int U = n_updates;
  PgoPlan P;
  PgoView v{};
  size_t o_res = 0;
  if (int r = pgo_prepare(c, n, poses, m, edges, n_prior, priors, U, relin_threshold, P, v, o_res)) return r;
  char *d = c->sat->pgo.d;
  hipStream_t st = c->stream;
  TimedSpan sp;
  span_begin(c, "pgo", sp);
  for (int u = 0; u < U; u++) pgo_update(c, v, u);
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

// ---------------------------------------------------------------- diagnostic: one update, every pass read back
int vba_debug_pgo_step(vba_ctx *c, int n, const double *poses, int m, const double *edges, int n_prior, const double *priors,
                       double *slot, int *n_pairs, int *pairs, double *blk, double *g, double *dx, double *cost, double *poses_out) {
  if (!pgo_args_ok(c, n, poses, m, edges, n_prior, priors)) return VBA_ERR_BAD_ARG;
  PgoPlan P;
  PgoView v{};
  size_t o_res = 0;
  if (int r = pgo_prepare(c, n, poses, m, edges, n_prior, priors, 1, 0.0, P, v, o_res)) return r;
  char *d = c->sat->pgo.d;
  hipStream_t st = c->stream;
  pgo_update(c, v, 0);
  HIPCHK(c, hipGetLastError());
  std::vector<double> h_slot((size_t)P.F * PGO_SLOT), h_blk((size_t)P.NB * 36), h_g((size_t)n * 6), h_dx((size_t)n * 6), h_th((size_t)n * 12);
  std::vector<char> res(32);
  hipError_t de = hipSuccess;
  auto down = [&](void *dst, const void *src, size_t b) { if (de == hipSuccess && b) de = hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, st); };
  down(h_slot.data(), v.slot, h_slot.size() * 8); down(h_blk.data(), v.blk, h_blk.size() * 8); down(h_g.data(), v.g, h_g.size() * 8);
  down(h_dx.data(), v.dx, h_dx.size() * 8); down(h_th.data(), v.theta, h_th.size() * 8); down(res.data(), d + o_res, 32);
  const hipError_t se = hipStreamSynchronize(st);   // always drained before the staging vectors go out of scope
  HIPCHK(c, de);
  HIPCHK(c, se);
  int status;
  std::memcpy(&status, res.data() + 20, 4);
  if (status == PGO_SINGULAR) { c->set_error("vba_debug_pgo_step: non-positive or non-finite pivot"); return VBA_ERR_SINGULAR; }
  if (slot) std::memcpy(slot, h_slot.data(), h_slot.size() * 8);
  if (n_pairs) *n_pairs = P.NPAIR;
  if (pairs) for (int p = 0; p < P.NPAIR; p++) { pairs[2 * p] = (int)(P.pk[p] / n); pairs[2 * p + 1] = (int)(P.pk[p] % n); }
  if (blk) std::memcpy(blk, h_blk.data(), h_blk.size() * 8);
  if (g) std::memcpy(g, h_g.data(), h_g.size() * 8);
  if (dx) std::memcpy(dx, h_dx.data(), h_dx.size() * 8);
  if (cost) std::memcpy(cost, res.data(), 8);
  if (poses_out) std::memcpy(poses_out, h_th.data(), h_th.size() * 8);
  return VBA_OK;
}

}  // extern "C"
