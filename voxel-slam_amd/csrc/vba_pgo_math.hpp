// The arithmetic of pose-graph optimisation (vba_pgo_optimize) as host-and-device functions: the SE(3) chart, one
// factor's linearisation, one Hessian block's assembly, the 6x6 LDL^T, one segment's elimination and back-substitution, one skeleton
// block's scatter and one node's retraction.  The kernels of vba_kernels_pgo.hpp call these, one thread per item;
// tests/host/pgo_host.cpp compiles the same text with g++ (tests/test_pgo_ref_cpu.py), so the reference of tests/pgo_ref.py is held
// against this text on the CPU before it is held against the device ("What pins the pose-graph passes").
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBE_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define VBE_HD inline
#endif

namespace vba {

constexpr int PGO_SLOT = 121;          // factor slot: Hii 36 | Hjj 36 | Hij 36 | gi 6 | gj 6 | cost 1
constexpr int PGO_SEGOUT = 120;        // segment Schur slot: S_AA 36 | S_BB 36 | S_BA 36 | b_A 6 | b_B 6
constexpr int PGO_Y = 78;              // per segment step: D^-1 [C | E | b] (6 x 13, column-major)
constexpr int PGO_SINGULAR = 1;

struct PgoView {
  int n, F, NB, S, K, NSB, U, NP, ld;
  double thr;
  double *theta;           // [n][12] linearisation points
  const double *fz;        // [F][18] Z(12) | lambda(6)
  const int *fi, *fj;      // [F] (fj = -1: prior)
  double *slot;            // [F][PGO_SLOT]
  double *blk;             // [NB][36] (0..n-1 diagonal, then the distinct node pairs, rows = lower node id)
  double *g;               // [n][6]
  const int *blk_off, *blk_ent;      // CSR per block, entry = f * 4 + part (0 Hii, 1 Hjj, 2 Hij, 3 Hij^T)
  const int *seg_off, *seg_nodes;    // CSR per segment
  const int *seg_att;      // [S][2] skeleton index of A / B (-1 none)
  const int *seg_ecode;    // [S] block code (blk * 2 + transposed) of H(s_1, A), -1 none
  const int *seg_ccode;    // [Ls] block code of H(s_k, s_k+1), or of H(s_L, B) at the last step, -1 none
  double *segY;            // [Ls][PGO_Y]
  double *segout;          // [S][PGO_SEGOUT]
  const int *skel_node;    // [K]
  const int *sb_pq;        // [NSB][2] skeleton indices p >= q
  const int *sb_base;      // [NSB] block code of H(node p, node q), -1 none
  const int *sb_off, *sb_ent;        // CSR per skeleton block, entry = s * 4 + part (0 S_AA, 1 S_BB, 2 S_BA, 3 S_BA^T)
  double *Ab, *Tb;         // dense skeleton system (k_bigl_* layout)
  double *dx;              // [n][6]
  double *cost;            // [U]
  int *cnt;                // [U]
  unsigned long long *mx;  // [U] bits of max |delta|_inf (non-negative doubles order as integers)
  int *status;
};

// ---------------------------------------------------------------- SE(3) in [omega; v] order, right retraction
// The coefficients of tests/pgo_oracle.py::_coeffs: Taylor series below 0.2 rad, closed forms above.
struct PgoCoef { double A, B, C, D, E, F; };
VBE_HD PgoCoef pgo_coeffs(double phi) {
  const double t = phi * phi;
  PgoCoef k;
  if (phi < 0.2) {
    k.A = 1 - t / 6 * (1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110))));
    k.B = 0.5 * (1 - t / 12 * (1 - t / 30 * (1 - t / 56 * (1 - t / 90 * (1 - t / 132)))));
    k.C = (1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110 * (1 - t / 156))))) / 6;
    k.D = 1.0 / 12 + t * (1.0 / 720 + t * (1.0 / 30240 + t * (1.0 / 1209600 + t * (1.0 / 47900160))));
    k.E = -(1 - t / 30 * (1 - t / 56 * (1 - t / 90 * (1 - t / 132 * (1 - t / 182))))) / 24;
    k.F = -(1 - t / 42 * (1 - t / 72 * (1 - t / 110 * (1 - t / 156 * (1 - t / 210))))) / 120;
  } else {
    const double s = sin(phi), c = cos(phi);
    k.A = s / phi; k.B = (1 - c) / t; k.C = (phi - s) / (t * phi);
    k.D = 1 / t - (1 + c) / (2 * phi * s);
    k.E = (1 - t / 2 - c) / (t * t);
    k.F = (phi - s - t * phi / 6) / (t * t * phi);
  }
  return k;
}
VBE_HD void pgo_hat(const double *w, double *W) {
  W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0;
}
VBE_HD void pgo_mm3(const double *a, const double *b, double *c) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
VBE_HD void pgo_compose(const double *X, const double *Y, double *Z) {   // Z = X Y
  pgo_mm3(X, Y, Z);
  for (int i = 0; i < 3; i++) Z[9 + i] = X[3 * i] * Y[9] + X[3 * i + 1] * Y[10] + X[3 * i + 2] * Y[11] + X[9 + i];
}
VBE_HD void pgo_inverse(const double *X, double *Y) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Y[3 * i + j] = X[3 * j + i];
  for (int i = 0; i < 3; i++) Y[9 + i] = -(Y[3 * i] * X[9] + Y[3 * i + 1] * X[10] + Y[3 * i + 2] * X[11]);
}
VBE_HD void pgo_exp(const double *xi, double *X) {
  double W[9], WW[9];
  pgo_hat(xi, W);
  pgo_mm3(W, W, WW);
  const PgoCoef k = pgo_coeffs(sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]));
  double V[9];
  for (int q = 0; q < 9; q++) {
    const double I = (q % 4 == 0) ? 1.0 : 0.0;
    X[q] = I + k.A * W[q] + k.B * WW[q];
    V[q] = I + k.B * W[q] + k.C * WW[q];
  }
  for (int i = 0; i < 3; i++) X[9 + i] = V[3 * i] * xi[3] + V[3 * i + 1] * xi[4] + V[3 * i + 2] * xi[5];
}
VBE_HD void pgo_log(const double *X, double *xi) {
  const double a0 = X[7] - X[5], a1 = X[2] - X[6], a2 = X[3] - X[1];
  const double s2 = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
  const double phi = atan2(0.5 * s2, 0.5 * (X[0] + X[4] + X[8] - 1.0));
  const double t = phi * phi;
  const double f = phi < 1e-4 ? 1 + t / 6 * (1 + 7 * t / 60) : phi / sin(phi);
  xi[0] = 0.5 * f * a0; xi[1] = 0.5 * f * a1; xi[2] = 0.5 * f * a2;
  double W[9], WW[9];
  pgo_hat(xi, W);
  pgo_mm3(W, W, WW);
  const double D = pgo_coeffs(sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2])).D;
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int j = 0; j < 3; j++) s += ((i == j ? 1.0 : 0.0) - 0.5 * W[3 * i + j] + D * WW[3 * i + j]) * X[9 + j];
    xi[3 + i] = s;
  }
}
// Jr^-1(xi) = [[Ji, 0], [-Ji Q Ji, Ji]] (row-major 6x6), as tests/pgo_oracle.py::jr_inv
VBE_HD void pgo_jrinv(const double *xi, double *J) {
  double W[9], V[9], WW[9], WV[9], VW[9], WVW[9], T1[9], T2[9], Q[9], Ji[9];
  pgo_hat(xi, W); pgo_hat(xi + 3, V);
  const PgoCoef k = pgo_coeffs(sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]));
  pgo_mm3(W, W, WW); pgo_mm3(W, V, WV); pgo_mm3(V, W, VW); pgo_mm3(WV, W, WVW);
  double WWV[9], VWW[9], WVWW[9], WWVW[9];
  pgo_mm3(W, WV, WWV); pgo_mm3(VW, W, VWW); pgo_mm3(WVW, W, WVWW); pgo_mm3(W, WVW, WWVW);
  for (int q = 0; q < 9; q++) {
    Q[q] = -0.5 * V[q] + k.C * (WV[q] + VW[q] - WVW[q]) + k.E * (WWV[q] + VWW[q] - 3 * WVW[q]) - 0.5 * (k.E - 3 * k.F) * (WVWW[q] + WWVW[q]);
    Ji[q] = ((q % 4 == 0) ? 1.0 : 0.0) + 0.5 * W[q] + k.D * WW[q];
  }
  pgo_mm3(Ji, Q, T1); pgo_mm3(T1, Ji, T2);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      J[6 * i + j] = Ji[3 * i + j]; J[6 * i + 3 + j] = 0.0;
      J[6 * (3 + i) + j] = -T2[3 * i + j]; J[6 * (3 + i) + 3 + j] = Ji[3 * i + j];
    }
}

// ---------------------------------------------------------------- per-factor linearisation
// Factor f (between: j >= 0, prior: j < 0) at the linearisation points theta: the factor's slot.
VBE_HD void pgo_linearize_factor(const PgoView &v, int f) {
  const int i = v.fi[f], j = v.fj[f];
  const double *z = v.fz + (size_t)f * 18, *lam = z + 12;
  double Zi[12], A[12], B[12], e[6], Jj[36], Ji[36];
  pgo_inverse(z, Zi);
  const double *Xi = v.theta + (size_t)i * 12;
  if (j >= 0) {                                 // between: e = Log(Z^-1 Xi^-1 Xj)
    const double *Xj = v.theta + (size_t)j * 12;
    double Xii[12], Xji[12];
    pgo_inverse(Xi, Xii);
    pgo_compose(Xii, Xj, A);
    pgo_compose(Zi, A, B);
    pgo_log(B, e);
    pgo_jrinv(e, Jj);
    pgo_inverse(Xj, Xji);
    pgo_compose(Xji, Xi, A);                    // Xj^-1 Xi; Ad = [[R, 0], [p^ R, R]]
    double P[9], PR[9], Ad[36];
    pgo_hat(A + 9, P);
    pgo_mm3(P, A, PR);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        Ad[6 * r + c] = A[3 * r + c]; Ad[6 * r + 3 + c] = 0.0;
        Ad[6 * (3 + r) + c] = PR[3 * r + c]; Ad[6 * (3 + r) + 3 + c] = A[3 * r + c];
      }
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) {
        double s = 0;
        for (int q = 0; q < 6; q++) s += Jj[6 * r + q] * Ad[6 * q + c];
        Ji[6 * r + c] = -s;
      }
  } else {                                      // prior: e = Log(P^-1 Xk), J = Jr^-1(e) in the i slot; no j side
    pgo_compose(Zi, Xi, B);
    pgo_log(B, e);
    pgo_jrinv(e, Ji);
    for (int q = 0; q < 36; q++) Jj[q] = 0.0;
  }
  double *s = v.slot + (size_t)f * PGO_SLOT;
  double c = 0.0;
  for (int q = 0; q < 6; q++) c += e[q] * e[q] * lam[q];
  s[120] = 0.5 * c;
  for (int a = 0; a < 6; a++) {
    double gi = 0, gj = 0;
    for (int q = 0; q < 6; q++) { gi += Ji[6 * q + a] * lam[q] * e[q]; gj += Jj[6 * q + a] * lam[q] * e[q]; }
    s[108 + a] = gi;
    s[114 + a] = gj;
    for (int b = 0; b < 6; b++) {
      double hii = 0, hjj = 0, hij = 0;
      for (int q = 0; q < 6; q++) {
        const double li = lam[q] * Ji[6 * q + a];
        hii += li * Ji[6 * q + b];
        if (j >= 0) { hij += li * Jj[6 * q + b]; hjj += lam[q] * Jj[6 * q + a] * Jj[6 * q + b]; }
      }
      s[6 * a + b] = hii; s[36 + 6 * a + b] = hjj; s[72 + 6 * a + b] = hij;
    }
  }
}

// ---------------------------------------------------------------- assembly of one Hessian block (and, for b < n, of g[b])
VBE_HD void pgo_assemble_block(const PgoView &v, int b) {
  double h[36], g[6];
  for (int q = 0; q < 36; q++) h[q] = 0.0;
  for (int q = 0; q < 6; q++) g[q] = 0.0;
  for (int e = v.blk_off[b]; e < v.blk_off[b + 1]; e++) {
    const int code = v.blk_ent[e], part = code & 3;
    const double *s = v.slot + (size_t)(code >> 2) * PGO_SLOT;
    if (part == 3) {
      for (int r = 0; r < 6; r++)
        for (int c = 0; c < 6; c++) h[6 * r + c] += s[72 + 6 * c + r];
    } else {
      const double *src = s + 36 * (part == 0 ? 0 : part == 1 ? 1 : 2);
      for (int q = 0; q < 36; q++) h[q] += src[q];
      if (part < 2) for (int q = 0; q < 6; q++) g[q] += s[108 + 6 * part + q];
    }
  }
  for (int q = 0; q < 36; q++) v.blk[(size_t)b * 36 + q] = h[q];
  if (b < v.n) for (int q = 0; q < 6; q++) v.g[(size_t)b * 6 + q] = g[q];
}

VBE_HD void pgo_load_block(const PgoView &v, int code, double *M) {
  if (code < 0) { for (int q = 0; q < 36; q++) M[q] = 0.0; return; }
  const double *s = v.blk + (size_t)(code >> 1) * 36;
  if (code & 1) { for (int r = 0; r < 6; r++) for (int c = 0; c < 6; c++) M[6 * r + c] = s[6 * c + r]; }
  else for (int q = 0; q < 36; q++) M[q] = s[q];
}

// LDL^T of a symmetric 6x6 in place (lower: L, diagonal: d), no pivoting: the blocks are SPD in a well-posed graph.  Returns
// false on a pivot <= 0 or not finite.
VBE_HD bool pgo_ldl6(double *A) {
  bool ok = true;
  for (int k = 0; k < 6; k++) {
    double d = A[7 * k];
    for (int j = 0; j < k; j++) d -= A[6 * k + j] * A[6 * k + j] * A[7 * j];
    ok = ok && (d > 0.0) && isfinite(d);
    A[7 * k] = d;
    for (int i = k + 1; i < 6; i++) {
      double s = A[6 * i + k];
      for (int j = 0; j < k; j++) s -= A[6 * i + j] * A[6 * k + j] * A[7 * j];
      A[6 * i + k] = s / d;
    }
  }
  return ok;
}
VBE_HD void pgo_ldl6_solve(const double *A, double *x) {
  for (int i = 0; i < 6; i++) for (int j = 0; j < i; j++) x[i] -= A[6 * i + j] * x[j];
  for (int i = 0; i < 6; i++) x[i] /= A[7 * i];
  for (int i = 5; i >= 0; i--) for (int j = i + 1; j < 6; j++) x[i] -= A[6 * j + i] * x[j];
}

// One segment s_1 .. s_L (attached to skeleton A before s_1 and B after s_L, either may be absent), eliminated front to back.
// Per step: Y = D^-1 [C | E | b] with D the Schur-updated diagonal block, C = H(s_k, next), E = the coupling to A, b the
// updated right-hand side; the next step receives D -= C^T Y_C, E = -C^T Y_E, b -= C^T Y_b; A collects E^T Y_E and E^T Y_b.
// Returns false on a pivot <= 0 or not finite.
VBE_HD bool pgo_seg_elim(const PgoView &v, int s) {
  const int o0 = v.seg_off[s], o1 = v.seg_off[s + 1];
  const bool hasA = v.seg_att[2 * s] >= 0;
  double Dup[36], E[36], bup[6], SAA[36], bA[6];
  for (int q = 0; q < 36; q++) { Dup[q] = 0.0; SAA[q] = 0.0; }
  for (int q = 0; q < 6; q++) { bup[q] = 0.0; bA[q] = 0.0; }
  pgo_load_block(v, v.seg_ecode[s], E);
  double *out = v.segout + (size_t)s * PGO_SEGOUT;
  bool ok = true;
  for (int o = o0; o < o1; o++) {
    const int node = v.seg_nodes[o];
    double D[36], C[36];
    const double *hd = v.blk + (size_t)node * 36;
    for (int q = 0; q < 36; q++) D[q] = hd[q] - Dup[q];
    ok = pgo_ldl6(D) && ok;
    pgo_load_block(v, v.seg_ccode[o], C);
    double *Y = v.segY + (size_t)o * PGO_Y;
    for (int c = 0; c < 13; c++) {
      double x[6];
      for (int r = 0; r < 6; r++) x[r] = c < 6 ? C[6 * r + c] : c < 12 ? E[6 * r + c - 6] : (-v.g[(size_t)node * 6 + r] - bup[r]);
      pgo_ldl6_solve(D, x);
      for (int r = 0; r < 6; r++) Y[6 * c + r] = x[r];
    }
    if (hasA)
      for (int a = 0; a < 6; a++) {
        for (int b = 0; b < 6; b++) {
          double t = 0;
          for (int r = 0; r < 6; r++) t += E[6 * r + a] * Y[6 * (6 + b) + r];
          SAA[6 * a + b] += t;
        }
        double t = 0;
        for (int r = 0; r < 6; r++) t += E[6 * r + a] * Y[72 + r];
        bA[a] += t;
      }
    // what the next node (or B at the last step) receives: C^T Y_C, C^T Y_E, C^T Y_b
    double nE[36];
    for (int a = 0; a < 6; a++) {
      for (int b = 0; b < 6; b++) {
        double tc = 0, te = 0;
        for (int r = 0; r < 6; r++) { tc += C[6 * r + a] * Y[6 * b + r]; te += C[6 * r + a] * Y[6 * (6 + b) + r]; }
        Dup[6 * a + b] = tc; nE[6 * a + b] = te;
      }
      double t = 0;
      for (int r = 0; r < 6; r++) t += C[6 * r + a] * Y[72 + r];
      bup[a] = t;
    }
    for (int q = 0; q < 36; q++) E[q] = (o + 1 < o1) ? -nE[q] : nE[q];   // the last step keeps C^T Y_E = S_BA
  }
  for (int q = 0; q < 36; q++) { out[q] = SAA[q]; out[36 + q] = Dup[q]; out[72 + q] = E[q]; }
  for (int q = 0; q < 6; q++) { out[108 + q] = bA[q]; out[114 + q] = bup[q]; }
  return ok;
}

// Skeleton block b = (p, q), p >= q, of the dense system: H(node p, node q) minus the block's segment slots in CSR order; the
// diagonal blocks also write their rows of the right-hand side (row NP of Ab).
VBE_HD void pgo_skel_scatter_block(const PgoView &v, int b) {
  const int p = v.sb_pq[2 * b], q = v.sb_pq[2 * b + 1];
  double h[36], r[6];
  pgo_load_block(v, v.sb_base[b], h);
  const int node = v.skel_node[p];
  if (p == q) for (int k = 0; k < 6; k++) r[k] = -v.g[(size_t)node * 6 + k];
  for (int e = v.sb_off[b]; e < v.sb_off[b + 1]; e++) {
    const int code = v.sb_ent[e], part = code & 3;
    const double *so = v.segout + (size_t)(code >> 2) * PGO_SEGOUT;
    if (part == 3) {
      for (int a = 0; a < 6; a++) for (int c = 0; c < 6; c++) h[6 * a + c] -= so[72 + 6 * c + a];
    } else {
      for (int k = 0; k < 36; k++) h[k] -= so[36 * part + k];
      if (part < 2 && p == q) for (int k = 0; k < 6; k++) r[k] -= so[108 + 6 * part + k];
    }
  }
  for (int a = 0; a < 6; a++)
    for (int c = 0; c < 6; c++) v.Ab[(size_t)(6 * p + a) * v.ld + 6 * q + c] = h[6 * a + c];
  if (p == q) for (int k = 0; k < 6; k++) v.Ab[(size_t)v.NP * v.ld + 6 * p + k] = r[k];
}

// The nodes of segment s, last to first, from the skeleton solution z (row NP of Ab) and the Y of the elimination.
VBE_HD void pgo_seg_back(const PgoView &v, int s) {
  const int o0 = v.seg_off[s], o1 = v.seg_off[s + 1];
  const int A = v.seg_att[2 * s], B = v.seg_att[2 * s + 1];
  const double *z = v.Ab + (size_t)v.NP * v.ld;
  double xa[6], xn[6];
  for (int k = 0; k < 6; k++) { xa[k] = A >= 0 ? z[6 * A + k] : 0.0; xn[k] = B >= 0 ? z[6 * B + k] : 0.0; }
  for (int o = o1 - 1; o >= o0; o--) {
    const double *Y = v.segY + (size_t)o * PGO_Y;
    double x[6];
    for (int r = 0; r < 6; r++) {
      double t = Y[72 + r];
      for (int c = 0; c < 6; c++) t -= Y[6 * c + r] * xn[c] + Y[6 * (6 + c) + r] * xa[c];
      x[r] = t;
    }
    for (int r = 0; r < 6; r++) { xn[r] = x[r]; v.dx[(size_t)v.seg_nodes[o] * 6 + r] = x[r]; }
  }
}

// theta_k (+) Exp(delta_k), in place
VBE_HD void pgo_retract(const double *d, double *th) {
  double E[12], X[12];
  pgo_exp(d, E);
  for (int q = 0; q < 12; q++) X[q] = th[q];
  pgo_compose(X, E, th);
}

}  // namespace vba
