// The host plan of pose-graph optimisation (vba_pgo_optimize): validation of the caller's arrays, the factor table, the
// distinct node pairs, the skeleton / segment split and every CSR table a PgoView points at.  Host code over the standard library only,
// so that tests/host/pgo_host.cpp runs the same plan under the g++ build of vba_pgo_math.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace vba {

enum { PGO_PLAN_OK = 0, PGO_PLAN_BAD_ARG = 1, PGO_PLAN_SINGULAR = 2 };

struct PgoPlan {
  int n = 0, F = 0, NPAIR = 0, NB = 0, S = 0, LS = 0, K = 0, NSB = 0, n6 = 0, NP = 0, ld = 0;
  std::vector<int> fi, fj;
  std::vector<double> fz;                  // [F][18] Z(12) | 1 / var (6)
  std::vector<long long> pk;               // sorted keys lo * n + hi of the distinct node pairs
  std::vector<int> blk_off, blk_ent, seg_off, seg_nodes, seg_att, seg_ecode, seg_ccode, skel_node, sb_pq, sb_base, sb_off, sb_ent;
};

inline int pgo_plan(int n, const double *poses, int m, const double *edges, int n_prior, const double *priors, PgoPlan &P,
                    std::string &err) {
  const int F = m + n_prior;
  P.n = n; P.F = F;
  // ---- validation and factor table (edges first, then priors)
  std::vector<int> &fi = P.fi, &fj = P.fj;
  std::vector<double> &fz = P.fz;
  fi.assign(F, 0); fj.assign(F, 0); fz.assign((size_t)F * 18, 0.0);
  auto index_of = [n](double x, int &k) { if (!(x >= 0.0 && x < (double)n) || x != std::floor(x)) return false; k = (int)x; return true; };
  for (size_t q = 0; q < (size_t)n * 12; q++) if (!std::isfinite(poses[q])) return PGO_PLAN_BAD_ARG;
  for (int f = 0; f < F; f++) {
    const bool pr = f >= m;
    const double *row = pr ? priors + (size_t)(f - m) * 19 : edges + (size_t)f * 20;
    const double *z = pr ? row + 1 : row + 2;
    int i, j = -1;
    if (!index_of(row[0], i) || (!pr && (!index_of(row[1], j) || i == j))) return PGO_PLAN_BAD_ARG;
    for (int q = 0; q < 18; q++) {
      if (!std::isfinite(z[q]) || (q >= 12 && !(z[q] > 0.0))) return PGO_PLAN_BAD_ARG;
      fz[(size_t)f * 18 + q] = q < 12 ? z[q] : 1.0 / z[q];
    }
    fi[f] = i; fj[f] = j;
  }
  // ---- distinct neighbour pairs, components, skeleton
  std::vector<long long> &pk = P.pk;
  pk.clear();
  pk.reserve(m);
  for (int f = 0; f < m; f++) pk.push_back((long long)std::min(fi[f], fj[f]) * n + std::max(fi[f], fj[f]));
  std::sort(pk.begin(), pk.end());
  pk.erase(std::unique(pk.begin(), pk.end()), pk.end());
  const int NPAIR = (int)pk.size(), NB = n + NPAIR;
  P.NPAIR = NPAIR; P.NB = NB;
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
    if (!comp_prior[root(k)]) { err = "vba_pgo_optimize: a connected component holds no prior"; return PGO_PLAN_SINGULAR; }
  std::vector<int> node_skel(n, -1);
  std::vector<int> &skel_node = P.skel_node;
  skel_node.clear();
  auto is_path = [&](int k) { return !has_prior[k] && nb_off[k + 1] - nb_off[k] <= 2; };
  for (int k = 0; k < n; k++) if (!is_path(k)) { node_skel[k] = (int)skel_node.size(); skel_node.push_back(k); }
  const int K = (int)skel_node.size();
  P.K = K;
  // ---- segments: maximal runs of path nodes, oriented so that a single attachment is B (eliminated towards it: no fill)
  std::vector<int> &seg_off = P.seg_off, &seg_nodes = P.seg_nodes, &seg_att = P.seg_att, &seg_ecode = P.seg_ecode, &seg_ccode = P.seg_ccode;
  seg_off.assign(1, 0); seg_nodes.clear(); seg_att.clear(); seg_ecode.clear(); seg_ccode.clear();
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
    if (B < 0) { err = "vba_pgo_optimize: a chain without a skeleton node"; return PGO_PLAN_SINGULAR; }
    for (int k = 0; k < L; k++) {
      seg_nodes.push_back(run[k]);
      seg_ccode.push_back(k + 1 < L ? pair_block(run[k], run[k + 1]) : pair_block(run[k], B));
    }
    seg_att.push_back(A >= 0 ? node_skel[A] : -1); seg_att.push_back(node_skel[B]);
    seg_ecode.push_back(A >= 0 ? pair_block(run[0], A) : -1);
    seg_off.push_back((int)seg_nodes.size());
  }
  const int S = (int)seg_off.size() - 1;
  P.S = S; P.LS = (int)seg_nodes.size();
  // ---- block CSR in factor order
  std::vector<int> &blk_off = P.blk_off, &blk_ent = P.blk_ent;
  blk_off.assign(NB + 1, 0);
  auto pair_index = [&](int a, int b) { return pair_block(a, b) >> 1; };
  for (int f = 0; f < F; f++) { blk_off[fi[f] + 1]++; if (fj[f] >= 0) { blk_off[fj[f] + 1]++; blk_off[pair_index(fi[f], fj[f]) + 1]++; } }
  for (int b = 0; b < NB; b++) blk_off[b + 1] += blk_off[b];
  blk_ent.assign(blk_off[NB] > 0 ? blk_off[NB] : 1, 0);
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
  P.NSB = NSB;
  std::vector<int> &sb_pq = P.sb_pq, &sb_base = P.sb_base;
  sb_pq.clear(); sb_base.clear();
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
  std::vector<int> &sb_off = P.sb_off, &sb_ent = P.sb_ent;
  sb_off.assign(1, 0); sb_ent.clear();
  for (auto &l : sbl) { sb_ent.insert(sb_ent.end(), l.begin(), l.end()); sb_off.push_back((int)sb_ent.size()); }
  P.n6 = 6 * K; P.NP = (P.n6 + 7) / 8 * 8; P.ld = (P.NP + 63) / 64 * 64;
  return PGO_PLAN_OK;
}

}  // namespace vba
