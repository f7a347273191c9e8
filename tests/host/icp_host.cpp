// Host build of the icp_normal arithmetic the device runs (csrc/vba_icp_math.hpp: the 1-NN query, the per-point gate and 35 terms, the
// 6x6 solve with the pose update, the state table) with the order of k_btc_icp_nn / k_btc_icp_accum / k_btc_icp_step restated around
// it (slices of tiles of 256, the xor butterfly of a wave, (w0 + w1) + (w2 + w3), the partials in workgroup order), for the CPU checks
// of tests/test_icp_ref_cpu.py against tests/icp_ref.py.  icp_host_pass has the outputs of vba_debug_btc_icp_pass.  Built by the tests
// with g++ -ffp-contract=off.  Test harness only.
#include "../../voxel-slam_amd/csrc/vba_icp_math.hpp"
#include "../../voxel-slam_amd/csrc/vba_eig3.hpp"
#include <cstdint>
#include <cstring>
#include <vector>

using namespace vba;

struct IcpState {            // vba_btc_icp_state
  double R[9], t[3], paras[4];
  int is_conv, done, iters, pad;
  double mat[6], eig[3];
};

extern "C" void icp_host_query(const double *R, const double *t, const float *sp, float *q) { btc_icp_query(R, t, sp, q); }
extern "C" int icp_host_point(const double *R, const double *t, const double *pa, const float *sp, const float *tp, double *s) {
  return btc_icp_point(R, t, pa, sp, tp, s) ? 1 : 0;
}
extern "C" void icp_host_transition(const double *dx, double *paras, int *is_conv, int *done, int *iters) {
  btc_icp_transition(dx, paras, is_conv, done, iters);
}
extern "C" void icp_host_solve_update(const double *acc, double *R, double *t, double *mat, double *dx) { btc_icp_solve_update(acc, R, t, mat, dx); }
extern "C" void icp_host_ldlt_inplace(double *A, const double *b, double *x) {   // the std::vector twin that ldlt_solve_fixed<6> copies
  std::vector<double> a(A, A + 36), r(b, b + 6), y(6);
  vbh::ldlt_solve_inplace(a.data(), r.data(), y.data(), 6);
  std::memcpy(x, y.data(), 48);
}

// slices >= 1.  Returns 0; 1 when the state says done (nothing is touched); 2 when the direct eigen-solver declined (eig is left).
extern "C" int icp_host_pass(int ns, const float *src, int nt, const float *tar, IcpState *st, int slices, uint64_t *key, unsigned char *gate,
                             double *partial, double *sums, double *dx_out) {
  if (st->done) return 1;
  const int nb = ns > 0 ? (ns + 255) / 256 : 1, ntile = (nt + 255) / 256, per = (ntile + slices - 1) / slices;
  std::vector<double> part((size_t)nb * BTC_ICP_PART, 0.0);
  for (int b = 0; b < nb; b++) {
    double lane[256][BTC_ICP_PART];
    std::memset(lane, 0, sizeof(lane));
    for (int l = 0; l < 256; l++) {
      const int i = b * 256 + l;
      if (i >= ns) continue;
      float q[3];
      btc_icp_query(st->R, st->t, src + 6 * (size_t)i, q);
      uint64_t best = ~0ull;
      for (int sl = 0; sl < slices; sl++) {
        const int lo = sl * per * 256, hi = (lo + per * 256 < nt) ? lo + per * 256 : nt;
        uint64_t sb = ~0ull;
        for (int base = lo < nt ? lo : nt; base < hi; base += 256) {
          const int cnt = hi - base < 256 ? hi - base : 256;
          float bd = 3.4e38f; int bi = -1;
          for (int k = 0; k < cnt; k++) {
            const float *p = tar + 6 * (size_t)(base + k);
            const float ddx = q[0] - p[0], ddy = q[1] - p[1], ddz = q[2] - p[2];
            float dd = ddx * ddx; dd += ddy * ddy; dd += ddz * ddz;
            if (dd < bd) { bd = dd; bi = base + k - lo; }
          }
          if (bi >= 0) {
            uint32_t bits; std::memcpy(&bits, &bd, 4);
            const uint64_t kk = ((uint64_t)bits << 32) | (uint32_t)bi;
            sb = kk < sb ? kk : sb;
          }
        }
        if (sb != ~0ull) sb += (uint32_t)lo;
        best = sb < best ? sb : best;
      }
      bool pass = false;
      if (best != ~0ull) pass = btc_icp_point(st->R, st->t, st->paras, src + 6 * (size_t)i, tar + 6 * (size_t)(uint32_t)(best & 0xFFFFFFFFull), lane[l]);
      if (key) key[i] = best;
      if (gate) gate[i] = pass ? 1 : 0;
    }
    double red[4][BTC_ICP_PART];
    for (int w = 0; w < 4; w++)
      for (int k = 0; k < BTC_ICP_PART; k++) {
        double x[64], y[64];
        for (int l = 0; l < 64; l++) x[l] = lane[64 * w + l][k];
        for (int m = 32; m >= 1; m >>= 1) { for (int l = 0; l < 64; l++) y[l] = x[l] + x[l ^ m]; std::memcpy(x, y, sizeof(x)); }
        red[w][k] = x[0];
      }
    for (int k = 0; k < BTC_ICP_PART; k++) part[(size_t)b * BTC_ICP_PART + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
  double acc[BTC_ICP_PART];
  for (int k = 0; k < BTC_ICP_PART; k++) { double a = 0; for (int b = 0; b < nb; b++) a += part[(size_t)b * BTC_ICP_PART + k]; acc[k] = a; }
  if (partial) std::memcpy(partial, part.data(), part.size() * 8);
  if (sums) std::memcpy(sums, acc, sizeof(acc));
  double dx[6];
  btc_icp_solve_update(acc, st->R, st->t, st->mat, dx);
  if (dx_out) std::memcpy(dx_out, dx, 48);
  btc_icp_transition(dx, st->paras, &st->is_conv, &st->done, &st->iters);
  if (st->done) {
    const double *m = st->mat;
    Eig3 e;
    if (!eig3_direct(m[0], m[1], m[2], m[3], m[4], m[5], e)) return 2;
    st->eig[0] = e.w0; st->eig[1] = e.w1; st->eig[2] = e.w2;
  }
  return 0;
}
