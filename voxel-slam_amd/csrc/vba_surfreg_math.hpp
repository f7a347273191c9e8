// The arithmetic of the surfel map and of one registration iteration against it (vba_surfel_map_*, vba_surfel_register, DESIGN.md
// §26), written once for the device (vba_kernels_surfreg.hpp) and for the g++ build of tests/host/surfreg_host.cpp: the cell weight
// W = (C + sigma^2 I)^-1, the table lookup, the query point, the choice among the candidate cells, the gate and the 29 terms of a
// point, and the step (solve, pose update, stop rules, report).  Nothing is contracted and every operation order below is the
// definition.  No kernel, no launch, no reduction: the order of the sums is the kernels'.
#pragma once
#include "vba_btc_svd.hpp"     // BTC_HD, BTC_NOCONTRACT
#include "vba_hostmath.hpp"
#include "vba_ldlt6.hpp"
#include "vba_voxel_key.hpp"

namespace vba {

constexpr int SREG_PART = 29;       // upper triangle of J^T W J (21, row-major) | J^T W d (6) | m / 2 | 1
constexpr int SREG_MAX_ITER = 32;

// A slot of the open-addressing table (ds_hash, linear probing, a power of two >= 2 cells slots) and the cell behind its row: one
// 16-byte probe, then one 64-byte line per hit.  row = the index of the cell's record in the arrays the map was built from.
struct alignas(16) SregSlot { unsigned long long key; int row, pad; };               // key DS_EMPTY when free
struct alignas(64) SregCell { float c[3]; float cnt; double W[6]; };                 // W: xx xy xz yy yz zz
static_assert(sizeof(SregSlot) == 16 && sizeof(SregCell) == 64, "slot and cell sizes are part of the counted bytes");

struct SregTable { const SregSlot *tab; const SregCell *cell; unsigned int mask; double voxel; };

// vba_surfel_reg_report (include/voxelba.h) field for field
struct SregReport {
  int iters, converged, lost, singular;
  int matches[SREG_MAX_ITER];
  double cost[SREG_MAX_ITER], step_rot[SREG_MAX_ITER], step_tra[SREG_MAX_ITER];
  double H[21], g[6], eig_tt[3];
};
// the state block of one call: pose, parameters, the report; `done` gates every later launch
struct SregState {
  double R[9], t[3];
  double gate2, eps_rot, eps_tra;
  int neighbors, max_iter, min_matches, done;
  SregReport rep;
};

// W = (C + sigma^2 I)^-1 by cofactors: A = C with s2 = sigma * sigma added to the diagonal; the six cofactors; the determinant
// along the first row; one reciprocal; six products.
BTC_HD void sreg_weight(const double *C, double sigma, double *W) {
  BTC_NOCONTRACT
  const double s2 = sigma * sigma;
  const double a = C[0] + s2, b = C[1], c = C[2], d = C[3] + s2, e = C[4], f = C[5] + s2;
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
  const double det = (a * c00 + b * c01) + c * c02;
  const double inv = 1.0 / det;
  W[0] = c00 * inv; W[1] = c01 * inv; W[2] = c02 * inv; W[3] = c11 * inv; W[4] = c12 * inv; W[5] = c22 * inv;
}

// the cell of a record: the float mean as it stands, the count, the weight of its covariance
BTC_HD void sreg_make_cell(const float *rec, const double *C, double sigma, SregCell *o) {
  o->c[0] = rec[0]; o->c[1] = rec[1]; o->c[2] = rec[2]; o->cnt = rec[11];
  sreg_weight(C, sigma, o->W);
}

// the key of a record's mean, and of the cell (ix, iy, iz)
BTC_HD unsigned long long sreg_key(const float *c, double voxel) {
  return ds_pack(ds_axis_key((double)c[0], voxel), ds_axis_key((double)c[1], voxel), ds_axis_key((double)c[2], voxel));
}

// row of `key`, -1 when the probe ends at an empty slot (the table has >= 2 cells slots; the bound only guards a full table)
BTC_HD int sreg_lookup(const SregTable &T, unsigned long long key) {
  unsigned int h = ds_hash(key) & T.mask;
  for (unsigned int probe = 0; probe <= T.mask; probe++) {
    const unsigned long long k = T.tab[h].key;
    if (k == key) return T.tab[h].row;
    if (k == DS_EMPTY) return -1;
    h = (h + 1) & T.mask;
  }
  return -1;
}

// q = R p + t
BTC_HD void sreg_query(const double *R, const double *t, const double *p, double *q) {
  BTC_NOCONTRACT
  for (int r = 0; r < 3; r++) q[r] = ((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) + t[r];
}

// m = d^T W d with Wd kept
BTC_HD double sreg_maha(const double *W, const double *d, double *Wd) {
  BTC_NOCONTRACT
  Wd[0] = (W[0] * d[0] + W[1] * d[1]) + W[2] * d[2];
  Wd[1] = (W[1] * d[0] + W[3] * d[1]) + W[4] * d[2];
  Wd[2] = (W[2] * d[0] + W[4] * d[1]) + W[5] * d[2];
  return (d[0] * Wd[0] + d[1] * Wd[1]) + d[2] * Wd[2];
}

// The cell of the query q among its own voxel and, for neighbors == 7, the six face neighbours in the order own, -x, +x, -y, +y,
// -z, +z (+-1 on the integer axis index before packing): the smallest m, ties to the earlier candidate.  Returns the row or -1;
// d = q - c, Wd and m are those of the chosen cell.
BTC_HD int sreg_choose(const SregTable &T, int neighbors, const double *q, double *d, double *Wd, double *m) {
  BTC_NOCONTRACT
  const long long ix = ds_axis_key((double)(float)q[0], T.voxel), iy = ds_axis_key((double)(float)q[1], T.voxel),
                  iz = ds_axis_key((double)(float)q[2], T.voxel);
  int best = -1;
  for (int k = 0; k < neighbors; k++) {
    const long long s = (k & 1) ? -1 : 1;                  // k = 1, 3, 5: -1;  k = 2, 4, 6: +1
    const long long dx = (k == 1 || k == 2) ? s : 0, dy = (k == 3 || k == 4) ? s : 0, dz = (k == 5 || k == 6) ? s : 0;
    const int row = sreg_lookup(T, ds_pack(ix + dx, iy + dy, iz + dz));
    if (row < 0) continue;
    const SregCell &c = T.cell[row];
    const double dd[3] = {q[0] - (double)c.c[0], q[1] - (double)c.c[1], q[2] - (double)c.c[2]};
    double wd[3];
    const double mm = sreg_maha(c.W, dd, wd);
    if (best < 0 || mm < *m) {
      best = row; *m = mm;
      for (int r = 0; r < 3; r++) { d[r] = dd[r]; Wd[r] = wd[r]; }
    }
  }
  return best;
}

// The 29 terms of a gated point p (body frame) under R against the cell weight W: J = [-R hat(p) | I] for the update
// R <- R Exp(dphi), t <- t + dt.  s += terms (the caller's accumulators, a chain per lane).
BTC_HD void sreg_terms(const double *R, const double *p, const double *W, const double *Wd, double m, double *s) {
  BTC_NOCONTRACT
  const double x = p[0], y = p[1], z = p[2];
  double A[9], WA[9];                                      // A = -R hat(p);  WA = W A
  for (int r = 0; r < 3; r++) {
    A[3 * r] = R[3 * r + 2] * y - R[3 * r + 1] * z;
    A[3 * r + 1] = R[3 * r] * z - R[3 * r + 2] * x;
    A[3 * r + 2] = R[3 * r + 1] * x - R[3 * r] * y;
  }
  const double Wm[9] = {W[0], W[1], W[2], W[1], W[3], W[4], W[2], W[4], W[5]};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) WA[3 * r + c] = (Wm[3 * r] * A[c] + Wm[3 * r + 1] * A[3 + c]) + Wm[3 * r + 2] * A[6 + c];
  // rows 0..2 of the upper triangle: A^T W A (c >= r), then A^T W = (W A)^T
  s[0] += (A[0] * WA[0] + A[3] * WA[3]) + A[6] * WA[6];
  s[1] += (A[0] * WA[1] + A[3] * WA[4]) + A[6] * WA[7];
  s[2] += (A[0] * WA[2] + A[3] * WA[5]) + A[6] * WA[8];
  s[3] += WA[0]; s[4] += WA[3]; s[5] += WA[6];
  s[6] += (A[1] * WA[1] + A[4] * WA[4]) + A[7] * WA[7];
  s[7] += (A[1] * WA[2] + A[4] * WA[5]) + A[7] * WA[8];
  s[8] += WA[1]; s[9] += WA[4]; s[10] += WA[7];
  s[11] += (A[2] * WA[2] + A[5] * WA[5]) + A[8] * WA[8];
  s[12] += WA[2]; s[13] += WA[5]; s[14] += WA[8];
  // rows 3..5: W
  s[15] += W[0]; s[16] += W[1]; s[17] += W[2]; s[18] += W[3]; s[19] += W[4]; s[20] += W[5];
  // J^T W d
  s[21] += (A[0] * Wd[0] + A[3] * Wd[1]) + A[6] * Wd[2];
  s[22] += (A[1] * Wd[0] + A[4] * Wd[1]) + A[7] * Wd[2];
  s[23] += (A[2] * Wd[0] + A[5] * Wd[1]) + A[8] * Wd[2];
  s[24] += Wd[0]; s[25] += Wd[1]; s[26] += Wd[2];
  s[27] += 0.5 * m;
  s[28] += 1.0;
}

// One point of one iteration: query, choice, gate, terms.  Returns the chosen row (-1: no candidate cell exists); *pass says
// whether the point entered the sums.
BTC_HD int sreg_point(const SregTable &T, const SregState &st, const double *p, double *s, bool *pass) {
  double q[3], d[3], Wd[3], m = 0.0;
  sreg_query(st.R, st.t, p, q);
  const int row = sreg_choose(T, st.neighbors, q, d, Wd, &m);
  *pass = row >= 0 && m < st.gate2;
  if (*pass) sreg_terms(st.R, p, T.cell[row].W, Wd, m, s);
  return row;
}

BTC_HD double sreg_norm3(double x, double y, double z) {
  BTC_NOCONTRACT
  return sqrt((x * x + y * y) + z * z);
}

// The step on the 29 reduced sums: the report slots of this iteration, then lost (fewer than min_matches: the pose stays),
// H dx = -g by ldlt_solve_fixed<6>, singular (a non-finite step: the pose stays), else R <- R Exp(dx[0..2]), t <- t + dx[3..5],
// converged when both step norms are below their eps, and the iteration limit.  dx is zero where no step was taken.  H is the
// caller's work array of 36 doubles (LDS on the device, so that the factorisation's indexing costs no scratch).
BTC_HD void sreg_step(const double *acc, SregState *st, double *dx, double *H) {
  BTC_NOCONTRACT
  SregReport &rp = st->rep;
  const int it = rp.iters;
  for (int k = 0; k < 21; k++) rp.H[k] = acc[k];
  for (int k = 0; k < 6; k++) { rp.g[k] = acc[21 + k]; dx[k] = 0.0; }
  rp.matches[it] = (int)acc[28];
  rp.cost[it] = acc[27];
  rp.iters = it + 1;
  if (rp.matches[it] < st->min_matches) { rp.lost = 1; st->done = 1; return; }
  double g[6], x[6];
  int idx = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) { H[6 * r + c] = acc[idx]; H[6 * c + r] = acc[idx]; idx++; }
  for (int r = 0; r < 6; r++) g[r] = -acc[21 + r];
  vbh::ldlt_solve_fixed<6>(H, g, x);
  bool finite = true;
  for (int k = 0; k < 6; k++) finite = finite && (fabs(x[k]) <= DBL_MAX);
  if (!finite) { rp.singular = 1; st->done = 1; return; }
  double E[9], Rn[9];
  vbh::so3_exp(x, E);
  vbh::m3_mul(st->R, E, Rn);
  for (int k = 0; k < 9; k++) st->R[k] = Rn[k];
  for (int k = 0; k < 3; k++) st->t[k] = st->t[k] + x[3 + k];
  for (int k = 0; k < 6; k++) dx[k] = x[k];
  rp.step_rot[it] = sreg_norm3(x[0], x[1], x[2]);
  rp.step_tra[it] = sreg_norm3(x[3], x[4], x[5]);
  if (rp.step_rot[it] < st->eps_rot && rp.step_tra[it] < st->eps_tra) { rp.converged = 1; st->done = 1; }
  if (rp.iters >= st->max_iter) st->done = 1;
}

}  // namespace vba
