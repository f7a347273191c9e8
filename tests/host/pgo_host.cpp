// Host build of the pose-graph arithmetic the device runs (csrc/vba_pgo_math.hpp: chart, factor linearisation, block assembly, segment
// elimination and back-substitution, skeleton scatter, retraction) under the production plan (csrc/vba_pgo_plan.hpp), for the CPU checks
// of tests/test_pgo_ref_cpu.py against tests/pgo_ref.py.  pgo_host_step has the outputs of vba_debug_pgo_step; the dense skeleton system,
// which the device hands to the k_bigl_* kernels, is solved here by a plain unpivoted LDL^T.  Test harness only.
#include "../../voxel-slam_amd/csrc/vba_pgo_math.hpp"
#include "../../voxel-slam_amd/csrc/vba_pgo_plan.hpp"
#include <cstring>

using namespace vba;

static PgoPlan g_plan;   // the plan of the last pgo_host_step (read by pgo_host_plan_vec)

extern "C" void pgo_host_coeffs(double phi, double *out) {
  const PgoCoef k = pgo_coeffs(phi);
  out[0] = k.A; out[1] = k.B; out[2] = k.C; out[3] = k.D; out[4] = k.E; out[5] = k.F;
}
extern "C" void pgo_host_exp(const double *xi, double *X) { pgo_exp(xi, X); }
extern "C" void pgo_host_log(const double *X, double *xi) { pgo_log(X, xi); }
extern "C" void pgo_host_jrinv(const double *xi, double *J) { pgo_jrinv(xi, J); }
extern "C" void pgo_host_retract(const double *d, double *th) { pgo_retract(d, th); }

// k_pgo_cost's order: 256 strided sums, then the 128 .. 1 tree
static double cost_tree(const double *slot, int F) {
  double red[256];
  for (int t = 0; t < 256; t++) { double acc = 0.0; for (int f = t; f < F; f += 256) acc += slot[(size_t)f * PGO_SLOT + 120]; red[t] = acc; }
  for (int w = 128; w > 0; w >>= 1) for (int t = 0; t < w; t++) red[t] += red[t + w];
  return red[0];
}

// One update with U = 1.  Returns 0, 1 (bad argument), 2 (no prior in a component / a chain without a skeleton node) or 3 (pivot).
// Every output may be NULL.  segY_out [LS][78] and segout_out [S][120]: what the elimination left (for the numpy model of the teeth).
extern "C" int pgo_host_step(int n, const double *poses, int m, const double *edges, int n_prior, const double *priors, double *slot,
                             int *n_pairs, int *pairs, double *blk, double *g, double *dx, double *cost, double *poses_out,
                             double *segY_out, double *segout_out, double *Ab_out) {
  PgoPlan &P = g_plan;
  std::string err;
  if (int r = pgo_plan(n, poses, m, edges, n_prior, priors, P, err)) return r;
  std::vector<double> theta(poses, poses + (size_t)n * 12), h_slot((size_t)P.F * PGO_SLOT + 1), h_blk((size_t)P.NB * 36), h_g((size_t)n * 6),
      segY((size_t)P.LS * PGO_Y + 1), segout((size_t)P.S * PGO_SEGOUT + 1), Ab((size_t)(P.NP + 1) * P.ld, 0.0), h_dx((size_t)n * 6, 0.0);
  double h_cost = 0.0;
  int status = 0;
  PgoView v{};
  v.n = n; v.F = P.F; v.NB = P.NB; v.S = P.S; v.K = P.K; v.NSB = P.NSB; v.U = 1; v.NP = P.NP; v.ld = P.ld; v.thr = 0.0;
  v.theta = theta.data(); v.fz = P.fz.data(); v.fi = P.fi.data(); v.fj = P.fj.data(); v.slot = h_slot.data(); v.blk = h_blk.data();
  v.g = h_g.data(); v.blk_off = P.blk_off.data(); v.blk_ent = P.blk_ent.data(); v.seg_off = P.seg_off.data();
  v.seg_nodes = P.seg_nodes.data(); v.seg_att = P.seg_att.data(); v.seg_ecode = P.seg_ecode.data(); v.seg_ccode = P.seg_ccode.data();
  v.segY = segY.data(); v.segout = segout.data(); v.skel_node = P.skel_node.data(); v.sb_pq = P.sb_pq.data(); v.sb_base = P.sb_base.data();
  v.sb_off = P.sb_off.data(); v.sb_ent = P.sb_ent.data(); v.Ab = Ab.data(); v.Tb = nullptr; v.dx = h_dx.data(); v.cost = &h_cost;
  v.status = &status;
  for (int f = 0; f < P.F; f++) pgo_linearize_factor(v, f);
  h_cost = cost_tree(h_slot.data(), P.F);
  for (int b = 0; b < P.NB; b++) pgo_assemble_block(v, b);
  for (int s = 0; s < P.S; s++) if (!pgo_seg_elim(v, s)) status = PGO_SINGULAR;
  const int NP = P.NP, ld = P.ld, n6 = P.n6;
  for (int i = 0; i < NP; i++) Ab[(size_t)i * ld + i] = i >= n6 ? 1.0 : 0.0;
  for (int b = 0; b < P.NSB; b++) pgo_skel_scatter_block(v, b);
  if (Ab_out) std::memcpy(Ab_out, Ab.data(), Ab.size() * 8);
  // plain LDL^T of the lower triangle (row i, column j <= i at Ab[i * ld + j]); the right-hand side is row NP
  double *z = Ab.data() + (size_t)NP * ld;
  for (int k = 0; k < n6; k++) {
    double d = Ab[(size_t)k * ld + k];
    for (int j = 0; j < k; j++) d -= Ab[(size_t)k * ld + j] * Ab[(size_t)k * ld + j] * Ab[(size_t)j * ld + j];
    if (!(d > 0.0) || !std::isfinite(d)) status = PGO_SINGULAR;
    Ab[(size_t)k * ld + k] = d;
    for (int i = k + 1; i < n6; i++) {
      double s = Ab[(size_t)i * ld + k];
      for (int j = 0; j < k; j++) s -= Ab[(size_t)i * ld + j] * Ab[(size_t)k * ld + j] * Ab[(size_t)j * ld + j];
      Ab[(size_t)i * ld + k] = s / d;
    }
  }
  for (int i = 0; i < n6; i++) for (int j = 0; j < i; j++) z[i] -= Ab[(size_t)i * ld + j] * z[j];
  for (int i = 0; i < n6; i++) z[i] /= Ab[(size_t)i * ld + i];
  for (int i = n6 - 1; i >= 0; i--) for (int j = i + 1; j < n6; j++) z[i] -= Ab[(size_t)j * ld + i] * z[j];
  for (int p = 0; p < P.K; p++) for (int k = 0; k < 6; k++) h_dx[(size_t)P.skel_node[p] * 6 + k] = z[6 * p + k];
  for (int s = 0; s < P.S; s++) pgo_seg_back(v, s);
  for (int k = 0; k < n; k++) pgo_retract(h_dx.data() + (size_t)k * 6, theta.data() + (size_t)k * 12);
  if (status == PGO_SINGULAR) return 3;
  if (slot) std::memcpy(slot, h_slot.data(), (size_t)P.F * PGO_SLOT * 8);
  if (n_pairs) *n_pairs = P.NPAIR;
  if (pairs) for (int p = 0; p < P.NPAIR; p++) { pairs[2 * p] = (int)(P.pk[p] / n); pairs[2 * p + 1] = (int)(P.pk[p] % n); }
  if (blk) std::memcpy(blk, h_blk.data(), h_blk.size() * 8);
  if (g) std::memcpy(g, h_g.data(), h_g.size() * 8);
  if (dx) std::memcpy(dx, h_dx.data(), h_dx.size() * 8);
  if (cost) *cost = h_cost;
  if (poses_out) std::memcpy(poses_out, theta.data(), theta.size() * 8);
  if (segY_out) std::memcpy(segY_out, segY.data(), (size_t)P.LS * PGO_Y * 8);
  if (segout_out) std::memcpy(segout_out, segout.data(), (size_t)P.S * PGO_SEGOUT * 8);
  return 0;
}

// The tables of the last plan: 0 seg_off, 1 seg_nodes, 2 seg_att, 3 seg_ecode, 4 seg_ccode, 5 skel_node, 6 sb_pq, 7 sb_base, 8 sb_off,
// 9 sb_ent, 10 blk_off, 11 blk_ent, 12 {K, NP, ld, S, LS, NSB, NB}.  Returns the length; copies when out is not NULL.
extern "C" int pgo_host_plan_vec(int which, int *out) {
  const PgoPlan &P = g_plan;
  const std::vector<int> dims{P.K, P.NP, P.ld, P.S, P.LS, P.NSB, P.NB};
  const std::vector<int> *t[] = {&P.seg_off, &P.seg_nodes, &P.seg_att, &P.seg_ecode, &P.seg_ccode, &P.skel_node, &P.sb_pq, &P.sb_base,
                                 &P.sb_off, &P.sb_ent, &P.blk_off, &P.blk_ent, &dims};
  if (which < 0 || which > 12) return -1;
  if (out) std::memcpy(out, t[which]->data(), t[which]->size() * sizeof(int));
  return (int)t[which]->size();
}
