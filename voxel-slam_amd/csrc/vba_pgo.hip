// Pose-graph optimisation of libvoxelba.so (vba_pgo_optimize): host driver of the kernels in vba_kernels_pgo.hpp; the dense
// skeleton system is factorised by the k_bigl_* kernels that the BA core compiles (declared in vba_ctx.hpp).
#include "vba_ctx.hpp"
#include "vba_kernels_pgo.hpp"

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

extern "C" {

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
  if (int r = grow(c->d_pgo, bytes, "graph structure")) return r;
  if (int r = grow(c->d_pgoAb, abytes, "dense skeleton system (8 (6K)^2 bytes)")) return r;
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

}  // extern "C"
