// Device-resident Levenberg-Marquardt loop of Lidar_BA_Optimizer::damping_iter (voxel_map.hpp:422-497): the state
// (poses, u, v, flags, H, g, trace) lives in HBM, so one LM iteration is a fixed chain of launches
//   k_hessian -> k_reduce_partials -> [all-reduce] -> k_lm_solve -> k_residual -> k_sum_scalar -> [all-reduce] -> k_lm_update
// with no host round trip; data-dependent control (is_calc_hess, the 1e-6 stop test) is carried by device flags that the
// kernels test on entry.
#pragma once
#include <hip/hip_runtime.h>
#include "vba_types.hpp"
#include "vba_ldlt.hpp"
#include "vba_kernels_factor.hpp"

namespace vba {


struct LmDev {
  double x[VBA_MAX_WIN_DEV * 12];    // x_stats       (accepted poses)
  double xt[VBA_MAX_WIN_DEV * 12];   // x_stats_temp  (trial poses)
  double u, v, r1, r2, q1, resis_first;
  int is_calc_hess, stop, iter, n_trace, all_accepted, last_accepted, max_trace, run_hess, run_res, pad;
  double trace[5 * 64];              // rows [r1, r2, u, v, q1]
  long long stamps[64];              // diagnostic (VBA_DEBUG_SOLVE bit 16)
  // speculative damping (see k_lm_solve_m): trial poses / q1 for the damping values the next LM_SPEC - 1 consecutive rejections would use
  int spec_n, spec_i, use_spec, xt_seq;      // xt_seq: the in-launch hand-off of xt (k_lm_trial): iter + 1 of the solve that stored it
  int trial_fault, pad3;                     // trial_fault: a rider of k_lm_trial gave up its wait for xt_seq (zero in every healthy call)
  double q1_spec[LM_SPEC];
  double xt_spec[LM_SPEC][VBA_MAX_WIN_DEV * 12];
};

// The image vba_lm_begin defines (x = xt = begin poses, u = 0.01, v = 2 (VM:427), is_calc_hess = all_accepted = run_hess = run_res = 1,
// max_trace = 64, pad = the diagnostic mask, every other byte zero), written by the nt threads of ONE workgroup of the first kernel
// of the call (LmInit, vba_kernels_factor.hpp) or by k_lm_init.  Every 8-byte word of the image is stored exactly once.
template <int W>
__device__ __forceinline__ void lm_init_store(const LmInit<W> &a, int tid, int nt) {
  constexpr int NW = sizeof(LmDev) / 8, XT = offsetof(LmDev, xt) / 8, U = offsetof(LmDev, u) / 8, V = offsetof(LmDev, v) / 8,
                I = offsetof(LmDev, is_calc_hess) / 8;
  static_assert(sizeof(LmDev) % 8 == 0 && offsetof(LmDev, x) == 0 && offsetof(LmDev, u) == 2 * offsetof(LmDev, xt) && 12 * W <= XT, "x and xt lead the image");
  static_assert(offsetof(LmDev, is_calc_hess) % 8 == 0 && offsetof(LmDev, pad) == offsetof(LmDev, is_calc_hess) + 36, "the ten flags are five words");
  auto two = [](int lo, int hi) { return (unsigned long long)(unsigned int)lo | ((unsigned long long)(unsigned int)hi << 32); };
  unsigned long long *o = reinterpret_cast<unsigned long long *>(a.dst);
  for (int w = tid; w < NW; w += nt) {
    unsigned long long val = 0ull;
    if (w < 2 * XT) { const int k = w < XT ? w : w - XT; if (k < 12 * W) val = (unsigned long long)__double_as_longlong(a.x[k]); }
    else if (w == U) val = (unsigned long long)__double_as_longlong(0.01);
    else if (w == V) val = (unsigned long long)__double_as_longlong(2.0);
    else if (w == I) val = two(1, 0);               // is_calc_hess, stop
    else if (w == I + 2) val = two(1, 0);           // all_accepted, last_accepted
    else if (w == I + 3) val = two(64, 1);          // max_trace, run_hess
    else if (w == I + 4) val = two(1, a.dbg);       // run_res, pad
    o[w] = val;
  }
}

// The same image from poses the workgroup already holds in LDS (sp, 12 W doubles, published by a barrier the caller has passed):
// the fused sites keep the begin poses there for their own work, so workgroup 0 needs no second read of the argument.  NT = the
// workgroup's thread count; the word loop is unrolled by the compile-time word count, the (at most ceil(2 XT / NT)) LDS reads come
// first, and what follows is stores only: nothing in it waits for memory, and every word is still stored exactly once.
template <int W, int NT>
__device__ __forceinline__ void lm_init_store_lds(const double *sp, LmDev *dst, int dbg, int tid) {
  constexpr int NW = sizeof(LmDev) / 8, XT = offsetof(LmDev, xt) / 8, U = offsetof(LmDev, u) / 8, V = offsetof(LmDev, v) / 8,
                I = offsetof(LmDev, is_calc_hess) / 8;
  constexpr int NI = (NW + NT - 1) / NT, NP = (2 * XT + NT - 1) / NT;     // rounds in all, rounds that reach a pose word
  static_assert(sizeof(LmDev) % 8 == 0 && offsetof(LmDev, x) == 0 && offsetof(LmDev, u) == 2 * offsetof(LmDev, xt) && 12 * W <= XT, "x and xt lead the image");
  static_assert(offsetof(LmDev, is_calc_hess) % 8 == 0 && offsetof(LmDev, pad) == offsetof(LmDev, is_calc_hess) + 36, "the ten flags are five words");
  auto two = [](int lo, int hi) { return (unsigned long long)(unsigned int)lo | ((unsigned long long)(unsigned int)hi << 32); };
  unsigned long long *o = reinterpret_cast<unsigned long long *>(dst);
  double pv[NP];
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const int w = tid + j * NT, k = w < XT ? w : w - XT;
    pv[j] = sp[(w < 2 * XT && k < 12 * W) ? k : 0];
  }
#pragma unroll
  for (int j = 0; j < NI; j++) {
    const int w = tid + j * NT;
    unsigned long long val = 0ull;
    if (j < NP && w < 2 * XT) { const int k = w < XT ? w : w - XT; if (k < 12 * W) val = (unsigned long long)__double_as_longlong(pv[j < NP ? j : 0]); }
    else if (w == U) val = (unsigned long long)__double_as_longlong(0.01);
    else if (w == V) val = (unsigned long long)__double_as_longlong(2.0);
    else if (w == I) val = two(1, 0);               // is_calc_hess, stop
    else if (w == I + 2) val = two(1, 0);           // all_accepted, last_accepted
    else if (w == I + 3) val = two(64, 1);          // max_trace, run_hess
    else if (w == I + 4) val = two(1, dbg);         // run_res, pad
    if (w < NW) o[w] = val;
  }
}

// Stand-alone form: callers whose first kernel is not one of the fused sites (multi-rank flow, the occupancy-compact Hessian pass,
// LI-BA, an empty store, vba_lm_end right after vba_lm_begin, vba_timing_launch_hessian).
template <int W>
__global__ __launch_bounds__(256) void k_lm_init(LmInit<W> a) { lm_init_store(a, threadIdx.x, 256); }

__device__ __forceinline__ void so3_exp_dev(const double *w, double *R) {   // tools.hpp:51-66
  const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (n >= 1e-11) {
    const double a0 = w[0] / n, a1 = w[1] / n, a2 = w[2] / n;
    const double s = sin(n), c1 = 1.0 - cos(n);
    // K = hat(a), K^2 = a a^T - I
    R[0] = 1.0 + c1 * (a0 * a0 - 1.0); R[1] = -s * a2 + c1 * a0 * a1;    R[2] = s * a1 + c1 * a0 * a2;
    R[3] = s * a2 + c1 * a1 * a0;      R[4] = 1.0 + c1 * (a1 * a1 - 1.0); R[5] = -s * a0 + c1 * a1 * a2;
    R[6] = -s * a1 + c1 * a2 * a0;     R[7] = s * a0 + c1 * a2 * a1;     R[8] = 1.0 + c1 * (a2 * a2 - 1.0);
  } else {
    R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
  }
}


// `red` = the reduced [H | g | r] of the last Hessian pass.  It is never modified here: the gauge (first 6 rows/cols ->
// identity, JacT.head(6) = 0, VM:452-455) and the damping u*diag are applied while the system is loaded, so a rejected
// step re-reads the same H with a new u (VM:443) and `red[0..n^2)` doubles as *hess (VM:446).  With more than one rank
// the exchange step all-reduces `red` in place on every iteration, so the valid copy is kept in `raw` (COPY_RAW).
// Elimination order = Eigen's LDLT pivoting: largest |diagonal| of the *stored* matrix first (ldlt_inplace::unblocked),
// realised as a rank computation (first index wins ties).
// (History, measured on MI355X at n = 60: unblocked LDS rows 58 us -> one wave blocked by pose 30.8 us -> this kernel 24 us,
//  profiles/r01_solve_ablation.txt; the two earlier kernels are no longer part of the library.)
//
// Blocked variant (vba_ldlt.hpp) for every supported window (n = 6W <= 96): trailing matrix in MFMA accumulators, panels
// of 8 columns, two barriers per panel.  Everything the kernel reads was written by other kernels (in general on another
// XCD, ~2 us per dependent trip), so the launch is one round trip deep before the factorisation:
//   * COPY_RAW (more than one rank, see above) is a template parameter, so that no control-flow join merges the two load orders
//     (the wait at such a join covers the longer queue of the two: vmcnt(0));
//   * the state flags are requested first (read before any store, they come in as scalar loads) and the reduced system right
//     behind them; the gate waits on lgkmcnt only, not on the system's vmcnt, so a gated launch costs one round trip;
//   * the system is read in its tile layout (coalesced, one load per upper-triangle tile per thread, plus the E-block remainder
//     at a clamped index: no load sits behind a branch, so none waits for another);
//   * every wave ranks the diagonal itself from registers (readlanes, no LDS, no barrier) while the system is in flight, and the
//     system is written straight into its PERMUTED position in a packed LDS image, so the tile build reads one LDS word per
//     element with no index indirection;
//   * the retraction runs on the last wave beside the q1 reduction of the first two.
//
// Speculative damping.  The solve is one workgroup on a 256-CU chip and the longest kernel of an iteration, and a REJECTED step
// repeats it on the same H and x with a damping that is known in advance (u <- u v, v <- 2 v, VM:485-486).  So the launch has
// LM_SPEC workgroups: workgroup b solves with the damping b consecutive rejections from now would use (the same f64 products the
// update would form, so every candidate is bit-identical to the sequential solve) and parks its trial poses and q1 in
// xt_spec[b] / q1_spec[b].  When the update rejects a step and a candidate is left it copies that candidate into xt / q1 and
// sets use_spec; the next launch of this kernel then returns at once.  An accepted step discards the candidates.  No field a
// workgroup reads on entry is written inside this kernel, so the workgroups need no ordering among themselves.

// A pose word of the trial state.  PUB: an agent-scope (write-through) store, for consumers inside the same launch (k_lm_trial).
template <bool PUB>
__device__ __forceinline__ void lm_xt_store(double *p, double v) {
  if constexpr (PUB) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// Index of the diagonal-block remainder E that tl_fetch adds to H(row, col), row <= col < 6W; -1 outside the frame's 6 x 6 block.
template <int W>
__host__ __device__ __forceinline__ int tl_eidx(int row, int col) {
  using C = HessCfg2<W>;
  const int fr = row / 6;
  if (col / 6 != fr) return -1;
  const int a = row - 6 * fr, b = col - 6 * fr;
  int idx;
  if (b < 3) idx = a * 3 - a * (a - 1) / 2 + (b - a);
  else if (a < 3) idx = 6 + 3 * a + (b - 3);
  else { const int a2 = a - 3, b2 = b - 3; idx = 15 + a2 * 3 - a2 * (a2 - 1) / 2 + (b2 - a2); }
  return C::EB + 21 * fr + idx;
}

// The solve's LDS, one object so that k_lm_trial can overlay it with the residual pass' (a workgroup there is one or the other).
template <int W>
struct LmSolveLds {
  static constexpr int n = 6 * W, NP = ((n + 1 + 15) / 16) * 16;
  alignas(16) double lds[LdltCfg<NP>::DOUBLES];
  alignas(16) double hd[n];                                   // (every array 16-byte aligned, as arrays of their own are: wide LDS reads)
  alignas(16) double gs[n];
  alignas(16) double xs[NP];
  alignas(16) double dxs[n];
  alignas(16) double red8[8];
  alignas(16) int ord[n];
};

// The body of k_lm_solve_m for damping candidate sb of nspec (the workgroup's first 256 threads).  dx_out (NULL in the LM loop): dx of
// candidate b to dx_out[b n ..] (vba_debug_solve).  PUBLISH (k_lm_trial): candidate 0 hands xt to the residual workgroups of the SAME
// launch: the pose words go out as agent-scope (write-through) stores, the storing wave drains them, then one lane stores
// xt_seq = iter + 1 with an agent-scope atomic store.  Arithmetic and order are the same in both forms.
template <int W, bool COPY_RAW, bool PUBLISH>
__device__ __forceinline__ void lm_solve_body(LmSolveLds<W> &L, const int sb, const int nspec, LmDev *s, const double *__restrict__ red, double *__restrict__ raw,
                                              double *__restrict__ dx_out) {
  using C2 = HessCfg2<W>;
  constexpr int n = 6 * W, NT = 256, NP = ((n + 1 + 15) / 16) * 16, NH = (n + 63) / 64, NU = C2::NU, T16 = C2::NT16;
  using LC = LdltCfg<NP>;
  // image of the whole NP x NP system ldlt_mfma factorises, packed lower triangle: P (Hess + u D) P^T, row n = -g, identity on the
  // padding (NP >= n + 2: row n + 1 is zero left of its diagonal, and (n + 1, 0) serves the upper triangle of the diagonal tiles)
  constexpr int IMG = NP * (NP + 1) / 2, ZERO = (n + 1) * (n + 2) / 2;
  static_assert(IMG <= LC::LTOT && NP >= n + 2, "the image must lie in the L region: ldlt_mfma writes P while the tiles are read");
  double *lds = L.lds, *hd = L.hd, *gs = L.gs, *xs = L.xs, *dxs = L.dxs, *red8 = L.red8;
  int *ord = L.ord;
  double *Lst = lds, *Tp = Lst + LC::LTOT, *P = Tp + NP * LC::LS, *img = lds;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // flags first: the gate below waits for these loads only
  const int use_spec = s->use_spec, stop = s->stop, calc = s->is_calc_hess;
  const double u0 = s->u, v0 = s->v;
  __builtin_amdgcn_sched_barrier(0);
  // lane k of every wave: H(k, k) (tile value, E remainder) and g[k], k = lane + 64 h
  double dgt[NH], dge[NH], gv[NH];
  auto load_diag = [&](const double *__restrict__ src) {
#pragma unroll
    for (int h = 0; h < NH; h++) {
      const int k = lane + 64 * h, kc = k < n ? k : n - 1, ta = kc >> 4, rt = kc & 15;
      dgt[h] = src[(ta * T16 - ta * (ta - 1) / 2) * 256 + (rt >> 2) * 64 + (rt & 3) * 16 + rt];
      dge[h] = src[tl_eidx<W>(kc, kc)];
      gv[h] = src[C2::GB + kc];
    }
  };
  // thread tid, upper-triangle tile u = (ta, tb): H(16 ta + ru, 16 tb + cu) = tile value (+ E remainder inside a frame's block)
  const int ru = (lane >> 4) + 4 * wv, cu = lane & 15;
  double tv[NU], ev[NU];
  bool eon[NU];
  auto load_bulk = [&](const double *__restrict__ src) {
    int u = 0;
#pragma unroll
    for (int ta = 0; ta < T16; ta++)
#pragma unroll
      for (int tb = ta; tb < T16; tb++, u++) {
        const int row = 16 * ta + ru, col = 16 * tb + cu;
        const int e = (row <= col && col < n) ? tl_eidx<W>(row, col) : -1;
        eon[u] = e >= 0;
        tv[u] = src[u * 256 + tid];
        ev[u] = src[e >= 0 ? e : C2::EB];
      }
  };
  if constexpr (!COPY_RAW) { load_diag(red); load_bulk(red); }
  const double r_v = COPY_RAW ? 0.0 : red[C2::RB];
  double xr[12];
  if (wv == 3 && lane < W)
#pragma unroll
    for (int k = 0; k < 12; k++) xr[k] = s->x[12 * lane + k];
  const long long t_begin = clock64();
  if (stop || use_spec) return;
  double u = u0;
  { double vb = v0; for (int k = 0; k < sb; k++) { u = u * vb; vb = 2 * vb; } }                         // VM:485-486, sb times
  if constexpr (COPY_RAW) {
    const double *__restrict__ src = calc ? red : raw;
    if (calc && sb == 0)
      for (int t = tid; t < C2::NOUT2; t += NT) raw[t] = src[t];
    load_diag(src); load_bulk(src);
  }
  // rank of row k = its position in the elimination order, computed by every wave for its own lanes
  double hk[NH], dk[NH];
  int rk[NH];
#pragma unroll
  for (int h = 0; h < NH; h++) {
    const int k = lane + 64 * h;
    hk[h] = k < 6 ? 1.0 : dgt[h] + dge[h];                                                              // gauge VM:452-455
    dk[h] = fabs(hk[h] + u * hk[h]);
    rk[h] = 0;
  }
#pragma unroll
  for (int j = 0; j < n; j++) {
    const double o = readlane_f64(dk[j >> 6], j & 63);
#pragma unroll
    for (int h = 0; h < NH; h++) rk[h] += (o > dk[h] || (o == dk[h] && j < lane + 64 * h)) ? 1 : 0;
  }
  // The last live pivot.  rmax = the largest rank of a row k >= 6: every rank above it belongs to a gauge row (an identity row with a
  // zero right-hand side, decoupled from every other row: its solution component is exactly 0), and behind those come only the
  // right-hand-side row and the padding.  The factorisation ends with the panel that holds rmax (ldlt_mfma's ncols), the back
  // substitution finds zeros in the rows beyond, the components beyond are written as 0.  A zero row is live (a frame without data at
  // u = 0 ranks behind the gauge rows), so nothing is skipped past it.  Every wave ranks all rows, so every wave holds the same rmax;
  // integer maximum over the wave by DPP moves (fixed tree, no LDS), read from lane 63.
  int rmax = 0;
#pragma unroll
  for (int h = 0; h < NH; h++) {
    const int k = lane + 64 * h;
    rmax = (k >= 6 && k < n && rk[h] > rmax) ? rk[h] : rmax;
  }
  rmax = wave_max_to_lane63(rmax);
  const int npan = __builtin_amdgcn_readlane(rmax, 63) / 8 + 1;
  // scatter the (gauged, damped) system to its permuted position
  int prow[T16], pcol[T16];
#pragma unroll
  for (int t = 0; t < T16; t++) {                   // 16 t < n, so a clamped row stays in the 64-row half of 16 t
    const int r = 16 * t + ru, c = 16 * t + cu;
    prow[t] = __shfl(rk[(16 * t) >> 6], (r < n ? r : n - 1) & 63);
    pcol[t] = __shfl(rk[(16 * t) >> 6], (c < n ? c : n - 1) & 63);
  }
  {
    int uu = 0;
#pragma unroll
    for (int ta = 0; ta < T16; ta++)
#pragma unroll
      for (int tb = ta; tb < T16; tb++, uu++) {
        const int row = 16 * ta + ru, col = 16 * tb + cu;
        if (row <= col && col < n) {
          double a = eon[uu] ? tv[uu] + ev[uu] : tv[uu];
          a = (row < 6) ? ((row == col) ? 1.0 : 0.0) : a;
          a = (row == col) ? a + u * a : a;
          const int pr = prow[ta], pc = pcol[tb], hi = pr > pc ? pr : pc, lo = pr > pc ? pc : pr;
          img[hi * (hi + 1) / 2 + lo] = a;
        }
      }
  }
  if (wv == 0)
#pragma unroll
    for (int h = 0; h < NH; h++) {
      const int k = lane + 64 * h;
      if (k < n) {
        const double g = k < 6 ? 0.0 : gv[h];
        hd[k] = hk[h]; gs[k] = g; ord[rk[h]] = k;
        img[n * (n + 1) / 2 + rk[h]] = -g;
      }
    }
#pragma unroll
  for (int i = n; i < NP; i++)                      // padding rows (NP <= 112 < NT: one element per thread and row)
    if (tid <= i && (i > n || tid >= n)) img[i * (i + 1) / 2 + tid] = (tid == i) ? 1.0 : 0.0;
  // (read after the gate and used only here, behind the system: in-order vmcnt)
  const int iter0 = s->iter, dbg = s->pad;
  if (tid == 0 && calc && sb == 0) { const double r = COPY_RAW ? red[C2::RB] : r_v; s->r1 = r; if (iter0 == 0) s->resis_first = r; }   // VM:445, 449-450
  long long *stamps = ((dbg & 16) && tid == 0 && sb == 0) ? s->stamps : nullptr;
  if (stamps) stamps[0] = t_begin;
  __syncthreads();
  auto elem = [&](int i, int j) -> double {        // one unconditional LDS read per element: no branch, no wait between elements
    return img[i >= j ? i * (i + 1) / 2 + j : ZERO];
  };
  if (stamps) stamps[1] = clock64();
  // (VBA_SOLVE_ALL_PANELS, bit 128 of the diagnostic mask: every panel, as before the limit existed; vba_debug_solve only)
  const int ncols = (dbg & 128) ? NP : 8 * npan, nsol = ncols < n ? ncols : n;
  ldlt_mfma<NP, NT>(Lst, Tp, P, n, elem, ((dbg & 16) && sb == 0) ? s->stamps : nullptr, LdltDense(), ncols);
  if (stamps) { stamps[3] = clock64(); stamps[6] = (ncols + 7) / 8 < LC::NBLK ? (ncols + 7) / 8 : LC::NBLK; }
  // The L blocks of the panels that were not run hold stale image words.  z is not loaded from them (0 beyond nsol), and the words
  // the back substitution reads there, L[j][i] for nsol <= i < j < n, are set to 0: the rows from nsol on then contribute 0 x 0, as
  // they do when their panels are run.  (At most six gauge rows lie beyond rmax, so this is one store on a few dozen threads; bounding
  // the substitution's loops by nsol instead, or masking its loads, cost 1.1-1.9k cycles at n = 60: with n a constant its loops are
  // unrolled and every load has an immediate offset.)
  if (tid < n) xs[tid] = tid < nsol ? Lst[LC::lat(n, tid)] : 0.0;
  for (int kb = (nsol + 7) >> 3; 8 * kb < n; kb++)
    for (int e = tid; e < (n - 8 * kb) * LC::LS; e += NT) Lst[LC::lst_off(kb) + e] = 0.0;
  __syncthreads();
  const double x = ldlt_backsub<NP>(Lst, xs, n);
  if (stamps) stamps[4] = clock64();
  if (tid < n) dxs[ord[tid]] = x;
  __syncthreads();
  if (wv == 3) {                                                                                        // VM:460-464
    if (lane < W) {
      double E[9];
      so3_exp_dev(dxs + 6 * lane, E);
      const double *R = xr;
      double *Rt = (sb == 0 ? s->xt : s->xt_spec[sb]) + 12 * lane;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) lm_xt_store<PUBLISH>(Rt + 3 * r + c, R[3 * r] * E[c] + R[3 * r + 1] * E[3 + c] + R[3 * r + 2] * E[6 + c]);
#pragma unroll
      for (int k = 0; k < 3; k++) lm_xt_store<PUBLISH>(Rt + 9 + k, R[9 + k] + dxs[6 * lane + 3 + k]);
    }
    if constexpr (PUBLISH) {
      if (sb == 0) {                               // this wave stored every word of xt: drain them, then the flag (one lane)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(&s->xt_seq, iter0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (lane == 63) red8[3] = 0.0;                 // (the wave sum of no rows)
  } else {
    double q = tid < n ? dxs[tid] * (u * hd[tid] * dxs[tid] - gs[tid]) : 0.0;                          // VM:465
    q = wave_sum_to_lane63(q);                                  // DPP adds (vba_common.hpp), no LDS round trips
    if (lane == 63) red8[wv] = q;
  }
  __syncthreads();
  if (dx_out && tid < n) dx_out[sb * n + tid] = dxs[tid];
  if (tid == 0) {
    const double q1 = 0.5 * (red8[0] + red8[1] + red8[2] + red8[3]);
    s->q1_spec[sb] = q1;
    if (sb == 0) { s->q1 = q1; s->spec_n = nspec; s->spec_i = 0; }
  }
  if (stamps) stamps[5] = clock64();
}

template <int W, bool COPY_RAW>
__global__ __launch_bounds__(256) void k_lm_solve_m(LmDev *s, const double *__restrict__ red, double *__restrict__ raw, double *__restrict__ dx_out) {
  __shared__ LmSolveLds<W> L;
  lm_solve_body<W, COPY_RAW, false>(L, blockIdx.x, gridDim.x, s, red, raw, dx_out);
}

// (Round 3 tried two single-wave forms of this solve for n <= 64 — lane i owns row i, no barriers, no tiles — and measured both slower on
//  MI355X at n = 60 than the blocked kernel's 24 us: rows in registers with the 1770 updates fully unrolled 31 us (a dependent f64
//  operation costs ~50 cycles with one wave per SIMD, so the 60 pivot steps are a ~350-cycle chain each: readlane, reciprocal + two
//  Newton steps, scale, first update), rows in LDS with rolled loops 62 us (every read-modify-write of a row element waits for its
//  own LDS round trip).  The blocked kernel's panel of 8 columns amortises that chain over 8 pivots.)

// ------------------------------------------------------------------------------------------------
// k_lm_trial: the solve and the residual pass of the trial poses in ONE launch (single rank, slot-parallel residual kernel).
// The seam between the two is 1 -> all: candidate 0's workgroup produces the 12 W words of xt, every residual workgroup consumes them,
// and everything else the residual pass reads (occupancy masks, fixed clusters, coe, the occupied slots' scalars) no kernel writes
// during an LM call.  So the residual workgroups ("riders", blocks nspec ..) are launched WITH the solve (blocks 0 .. nspec - 1,
// dispatched first), make both of their memory trips while it runs, and then wait for one word:
//   producer  lm_solve_body<PUBLISH>: xt as agent-scope stores, s_waitcnt vmcnt(0) on the storing wave, xt_seq = iter + 1 (agent-scope
//             atomic store, one lane).  iter grows with every step that is not stopped, and the call's init image zeroes xt_seq, so the
//             value a rider waits for is stored by this launch's solve and by nothing earlier.
//   consumer  one lane per workgroup polls xt_seq (relaxed agent-scope loads, s_sleep between them), the workgroup's barrier publishes
//             the outcome, then EVERY pose word is read with an agent-scope load (they bypass the CU's L1: no acquire fence needed).
// No wait where none is due: run_res == 0 (stopped) -> the rider returns after trip 1; use_spec != 0 (the previous Hessian pass
// installed a candidate, the solve of this launch returns at once) -> xt is valid as launched, and was requested with trip 1.
// run_res, stop, use_spec and iter were written before the launch and nothing inside it writes them.
// The wait is bounded: 20 ms of the 100 MHz wall clock (the longest solve this kernel is launched with, W = 10, lasts 20 us: three
// orders of magnitude; wider windows keep the two launches, voxelba.hip LmTrialFits).  A rider that gives up stores NaN as its
// partial (r1 - NaN > 0 is false: the step is rejected), sets LmDev::trial_fault, and the next call that fetches the state reports it.
// The bound only turns a surprise into an error: the riders cannot keep the solve from running, its workgroups are dispatched first.
constexpr long long kLmTrialWaitTicks = 2000000;            // 20 ms at 100 MHz

struct LmTrialRider {
  LmDev *s;
  int *ok_lds;                                              // one LDS word of the workgroup: the poll's outcome
  int run_res, stop, use_spec, iter;
  __device__ __forceinline__ double request(int npose, int tid) {
    run_res = s->run_res; stop = s->stop; use_spec = s->use_spec; iter = s->iter;
    return __hip_atomic_load(&s->xt[tid < npose ? tid : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ int run() const { return (run_res != 0 && stop == 0) ? 1 : 0; }
  __device__ __forceinline__ bool have_xt() const { return use_spec != 0; }
  __device__ __forceinline__ bool wait(int tid) const {
    if (tid == 0) {
      const int want = iter + 1;
      int ok = 1;
      const long long t0 = wall_clock64();
      while (__hip_atomic_load(&s->xt_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > kLmTrialWaitTicks) { ok = 0; break; }
      }
      *ok_lds = ok;
    }
    __syncthreads();
    return *ok_lds != 0;
  }
  __device__ __forceinline__ double xt(int npose, int tid) const {
    return __hip_atomic_load(&s->xt[tid < npose ? tid : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void fault() const { __hip_atomic_store(&s->trial_fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

template <int W, int TV>
struct LmTrialCfg {
  static constexpr int RNT = ResCfg<W, TV>::NT, BS = RNT > 256 ? RNT : 256;     // threads of a rider, of any workgroup
  union Lds { LmSolveLds<W> solve; ResLds<W, TV> res; };                        // a workgroup is one or the other
};

// One launch of nspec + residual workgroups; the partials are the residual pass', one per rider in the same order.
template <int W, bool COPY_RAW = false, int TV = 32>
__global__ __launch_bounds__((LmTrialCfg<W, TV>::BS)) void k_lm_trial(LmDev *s, const double *__restrict__ red, double *__restrict__ raw, int nspec, FactorView f,
                                                                    int head, int end, double *__restrict__ partial) {
  using TC = LmTrialCfg<W, TV>;
  __shared__ typename TC::Lds L;
  __shared__ int wait_ok;
  if ((int)blockIdx.x < nspec) {
    if (threadIdx.x >= 256) return;                         // (whole waves)
    lm_solve_body<W, COPY_RAW, true>(L.solve, blockIdx.x, nspec, s, red, raw, nullptr);
  } else {
    if (threadIdx.x >= TC::RNT) return;
    LmInit<W> none;
    none.on = 0;
    residual_s_body<W, TV, false, LmTrialRider>(L.res, (int)blockIdx.x - nspec, f, nullptr, head, end, partial, nullptr, nullptr, none, LmTrialRider{s, &wait_ok});
  }
}

// Accept / reject bookkeeping of VM:467-494 (one thread).  r2_dev = the reduced residual of the trial poses.
// nb > 0: r2 is first summed here from the residual pass' nb workgroup partials (single rank: saves one launch);
// nb == 0: r2_dev already holds the (all-reduced) scalar.  One wave; every lane takes the (uniform) decision so that the
// pose copy x <- x_temp is a parallel copy and no dependent chain of single-lane global accesses remains.
__device__ int lm_prev_stop(const LmDev *s) { return s->stop; }
__device__ double lm_r1(const LmDev *s) { return s->r1; }
__device__ const double *lm_xt(const LmDev *s) { return s->xt; }

// Everything a decision can need, requested in ONE batch: no address depends on a value of that batch.  The candidate a rejection
// installs is xt_spec[spec_i + 1], and spec_i is itself part of the state.  A caller that knows spec_i from an earlier trip (the Hessian
// passes read it with r1 and stop in front of their barrier) names the row; the stand-alone kernels request the lane's words of ALL
// LM_SPEC - 1 candidates (and their q1) and select when spec_i has arrived.  A lane owns the pose words lane, lane + 64, lane + 128
// of a 12 VBA_MAX_WIN_DEV-word row: all three lie inside the row for every W, so the loads carry no condition; the stores keep theirs.
struct LmCand { double q1, p0, p1, p2; };                    // a candidate's q1 and this lane's three pose words
struct LmUpdIn {                                            // (named scalars, no arrays: every field lives in a register from the start)
  int stop, ntr, mtr, it, spec_n, spec_i;
  double r1, q1, u0, v0, xt0, xt1, xt2;
  LmCand c;                                                 // the candidate behind spec_i (any row when there is none: unused then)
};
static_assert(VBA_MAX_WIN_DEV * 12 == 192 && LM_SPEC == 4, "three pose words per lane; candidates 1, 2, 3");
__device__ __forceinline__ LmCand lm_cand_load(const LmDev *s, int b, int lane) {
  return {s->q1_spec[b], s->xt_spec[b][lane], s->xt_spec[b][lane + 64], s->xt_spec[b][lane + 128]};
}
__device__ __forceinline__ void lm_update_load(const LmDev *s, int lane, LmUpdIn &in) {
  in.stop = s->stop; in.ntr = s->n_trace; in.mtr = s->max_trace; in.it = s->iter; in.spec_n = s->spec_n; in.spec_i = s->spec_i;
  in.r1 = s->r1; in.q1 = s->q1; in.u0 = s->u; in.v0 = s->v;
  in.xt0 = s->xt[lane]; in.xt1 = s->xt[lane + 64]; in.xt2 = s->xt[lane + 128];
}
// The pose words are used only inside the branches of the decision, and the compiler sinks their loads into those branches (measured:
// the rejected step's Hessian launch then lasted 0.4 us longer than the parent's).  Naming them as operands of an empty statement
// keeps the loads where they were issued; the caller puts this behind the last request of its first batch.
__device__ __forceinline__ void lm_pin(LmCand &c) { asm volatile("" : "+v"(c.p0), "+v"(c.p1), "+v"(c.p2)); }
__device__ __forceinline__ void lm_pin(LmUpdIn &in) { asm volatile("" : "+v"(in.xt0), "+v"(in.xt1), "+v"(in.xt2)); }
// Stand-alone kernels: the state and all candidates in one batch; `wait` runs between the requests and their use (the partial sum).
template <class F>
__device__ __forceinline__ void lm_update_load_all(const LmDev *s, int lane, LmUpdIn &in, F wait) {
  lm_update_load(s, lane, in);
  LmCand c1 = lm_cand_load(s, 1, lane), c2 = lm_cand_load(s, 2, lane), c3 = lm_cand_load(s, 3, lane);
  wait();
  lm_pin(in); lm_pin(c1); lm_pin(c2); lm_pin(c3);
  const int nx = in.spec_i + 1;                             // >= 1
  auto pick = [nx](double a1, double a2, double a3) { return nx == 2 ? a2 : nx == 3 ? a3 : a1; };
  in.c = {pick(c1.q1, c2.q1, c3.q1), pick(c1.p0, c2.p0, c3.p0), pick(c1.p1, c2.p1, c3.p1), pick(c1.p2, c2.p2, c3.p2)};
}

// One wave (all 64 lanes call it with the same r2 and their own `in`).  `in.stop` is the caller's to test.
__device__ __forceinline__ void lm_update_commit(LmDev *s, const LmUpdIn &in, double r2, int W) {
  const int ntr = in.ntr, mtr = in.mtr, it = in.it, spec_n = in.spec_n, spec_nx = in.spec_i + 1;
  const double r1 = in.r1, q1 = in.q1, u0 = in.u0, v0 = in.v0;
  const int lane = threadIdx.x & 63;
  const bool have_spec = spec_nx < spec_n;                  // a candidate for the damping a rejection leads to (k_lm_solve_m)
  const double sp0 = in.c.p0, sp1 = in.c.p1, sp2 = in.c.p2, q1_nx = in.c.q1;   // used only with have_spec
  const double xt0 = in.xt0, xt1 = in.xt1, xt2 = in.xt2;      // up to 192 pose scalars = 3 per lane
  double q = r1 - r2, u = u0, v = v0;
  const bool accept = q > 0;
  if (accept) {                                             // VM:473-483
    if (lane < 12 * W) s->x[lane] = xt0;
    if (lane + 64 < 12 * W) s->x[lane + 64] = xt1;
    if (lane + 128 < 12 * W) s->x[lane + 128] = xt2;
    const double one_three = 1.0 / 3;
    q = q / q1;
    v = 2;
    const double t = 2 * q - 1;
    q = 1 - t * t * t;                                      // pow(2q-1, 3)
    u *= (q < one_three ? one_three : q);
  } else {                                                  // VM:484-490
    u = u * v;
    v = 2 * v;
    if (have_spec) {                                        // the solve for this (u, H, x) has already been done
      if (lane < 12 * W) s->xt[lane] = sp0;
      if (lane + 64 < 12 * W) s->xt[lane + 64] = sp1;
      if (lane + 128 < 12 * W) s->xt[lane + 128] = sp2;
    }
  }
  if (lane != 0) return;
  if (!accept && have_spec) { s->q1 = q1_nx; s->spec_i = spec_nx; s->use_spec = 1; }
  else { s->use_spec = 0; s->spec_n = 0; }
  s->r2 = r2;
  if (ntr < mtr) {
    double *t = s->trace + 5 * ntr;
    t[0] = r1; t[1] = r2; t[2] = u0; t[3] = v0; t[4] = q1;
    s->n_trace = ntr + 1;
  }
  s->u = u; s->v = v;
  s->is_calc_hess = accept ? 1 : 0;
  s->last_accepted = accept ? 1 : 0;
  if (!accept) s->all_accepted = 0;                         // is_converge = false   VM:489
  s->iter = it + 1;
  const int nstop = (fabs((r1 - r2) / r1) < 1e-6) ? 1 : 0;  // VM:492-493
  s->stop = nstop;
  s->run_res = nstop ? 0 : 1;
  s->run_hess = (accept && !nstop) ? 1 : 0;
}

// The form the Hessian passes call behind their prologue's barrier (the caller has tested stop, and read spec_i / spec_n in front of
// the barrier: lm_spec_state): the state, the trial poses and the ONE candidate in one trip, then the stores.
__device__ void lm_spec_state(const LmDev *s, int &spec_i, int &spec_n) { spec_i = s->spec_i; spec_n = s->spec_n; }
__device__ void lm_update_apply(LmDev *s, double r2, int W, int spec_i, int spec_n) {
  const int lane = threadIdx.x & 63, nx = spec_i + 1;
  LmUpdIn in;
  lm_update_load(s, lane, in);
  in.c = lm_cand_load(s, (nx >= 1 && nx < spec_n && nx < LM_SPEC) ? nx : 1, lane);
  lm_pin(in); lm_pin(in.c);
  lm_update_commit(s, in, r2, W);
}

// Stand-alone form (multi-rank flow, the last iteration of a call, callers that want the flags after every iteration).
// The state batch, stop among it, is requested in front of the partials: one trip before the stores.
__global__ __launch_bounds__(64) void k_lm_update(LmDev *s, const double *__restrict__ r2_dev, int nb, int W) {
  LmUpdIn in;
  double r2;
  lm_update_load_all(s, threadIdx.x, in, [&] { r2 = (nb > 0) ? lm_sum_partials(r2_dev, nb, threadIdx.x) : r2_dev[0]; });
  if (in.stop) return;
  lm_update_commit(s, in, r2, W);
}

// The fetching vba_lm_end in ONE launch.  Workgroup 0: wave 0 applies the pending accept/reject (upd != 0: the same lm_sum_partials /
// lm_update_commit as k_lm_update, so the same sums), then the workgroup stores the LmDev image through the host mapping.  The image
// is RE-READ for that with device-scope loads behind a device-scope fence and the workgroup barrier: the copy then does not depend
// on this CU's L1 holding what wave 0 has just stored (lm_update_apply reads the lines it then writes).  Workgroups 1 .. : *hess,
// tile layout -> row-major (6W)^2 (tl_fetch, as k_tiles_to_full) straight into the pinned buffer (h_hess == nullptr: not launched).
template <int W>
__global__ __launch_bounds__(256) void k_lm_finish(LmDev *s, const double *__restrict__ r2_dev, int nb, int upd, LmDev *h_lm,
                                                   const double *__restrict__ red, double *__restrict__ h_hess) {
  if (blockIdx.x == 0) {
    if (upd && threadIdx.x < 64) {
      LmUpdIn in;
      double r2;
      lm_update_load_all(s, threadIdx.x, in, [&] { r2 = lm_sum_partials(r2_dev, nb, threadIdx.x); });
      if (!in.stop) lm_update_commit(s, in, r2, W);
      __threadfence();
    }
    __syncthreads();
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(s);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(h_lm);
    for (int w = threadIdx.x; w < (int)(sizeof(LmDev) / 8); w += 256) dst[w] = __hip_atomic_load(src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    constexpr int n = 6 * W;
    for (int t = (blockIdx.x - 1) * 256 + threadIdx.x; t < n * n; t += (gridDim.x - 1) * 256) h_hess[t] = tl_fetch<W>(red, t / n, t % n);
  }
}

}  // namespace vba
