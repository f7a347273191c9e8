// Host build of the prior-map odometry update the device runs (vba_odom_surfel_update): the point of
// csrc/vba_surfreg_math.hpp and the EKF iteration of csrc/vba_odom_ekf.hpp, with the order of k_sodom_accum and of odom_sum_partials
// restated around them (nb = min(ceil(n / 256), 1024) workgroups, lane chains over the tiles b, b + nb, ..., the xor butterfly of a
// wave, (w0 + w1) + (w2 + w3), the 34 columns of a row, the seven-group reduction over the rows) and the loop of odom_ekf_loop_host
// (tests/host/odom_ekf_host.cpp), for tests/test_surfodom_cpu.py and tests/test_gpu_surfodom.py against tests/surfodom_ref.py.
// A stand-alone program: surfodom_host IN OUT.  Built by the tests with g++ -ffp-contract=off.  Test harness only.
//
// IN : int64 n_rec, n_pnt; double voxel, sigma, gate, min_eig; int32 min_count, neighbors, min_matches, kd;
//      double state[25], cov[225]; float rec[n_rec][12]; double cov6[n_rec][6]; double pnt[n_pnt][3]
// OUT: int64 n_cells, nb; taps of iteration 0: int32 cell[n_pnt]; uint8 gate[n_pnt]; double partial[nb][34], cost[nb], sums[34];
//      the loop's result: double state[25], cov[225], nnt[9], rot_add[4], tra_add[4]; int32 match_num[4], iterations, ok,
//      rematch_num, 0; double eig_min
#include "../../voxel-slam_amd/csrc/vba_surfreg_math.hpp"
#include "../../voxel-slam_amd/csrc/vba_odom_ekf.hpp"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace vba;

namespace {

constexpr int kMaxBlocks = 1024;     // SREG_MAX_BLOCKS of csrc/vba_kernels_surfreg.hpp
constexpr int kRow = 34;             // SODOM_ROW
constexpr int kRedLanes = 7 * 34;    // ODOM_RED_LANES of csrc/vba_kernels_odom.hpp

struct NoSync { void operator()() const {} };

template <class T>
bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <class T>
bool wr(FILE *f, const T *p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

struct Head {
  int64_t n_rec, n_pnt;
  double voxel, sigma, gate, min_eig;
  int32_t min_count, neighbors, min_matches, kd;
  double state[25], cov[225];
};

// k_sodom_accum over np points at the pose of S: rows [nb][34], cost [nb]; taps when asked for
void point_loop(const SregTable &T, const vbh::OdomEkf &S, const Head &h, const std::vector<double> &pnt, int nb, std::vector<double> &part,
                std::vector<double> &cost, int32_t *tcell, uint8_t *tgate) {
  const size_t np = pnt.size() / 3;
  SregState X;
  std::memset(&X, 0, sizeof(X));
  std::memcpy(X.R, S.R, sizeof(X.R)); std::memcpy(X.t, S.t, sizeof(X.t));
  X.gate2 = h.gate * h.gate; X.neighbors = h.neighbors;
  std::vector<double> lane(256 * SREG_PART);
  for (int b = 0; b < nb; b++) {
    std::fill(lane.begin(), lane.end(), 0.0);
    for (int l = 0; l < 256; l++)
      for (size_t i = (size_t)b * 256 + l; i < np; i += (size_t)nb * 256) {
        bool pass;
        const int row = sreg_point(T, X, pnt.data() + 3 * i, lane.data() + (size_t)l * SREG_PART, &pass);
        if (tcell) { tcell[i] = row; tgate[i] = pass ? 1 : 0; }
      }
    double red[4][SREG_PART];
    for (int w = 0; w < 4; w++)
      for (int k = 0; k < SREG_PART; k++) {
        double x[64], y[64];
        for (int l = 0; l < 64; l++) x[l] = lane[(size_t)(64 * w + l) * SREG_PART + k];
        for (int m = 32; m >= 1; m >>= 1) { for (int l = 0; l < 64; l++) y[l] = x[l] + x[l ^ m]; std::memcpy(x, y, sizeof(x)); }
        red[w][k] = x[0];
      }
    for (int c = 0; c < kRow; c++) {
      const int k = c < 27 ? c : (c < 33 ? c - 12 : 28);
      const double v = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
      part[(size_t)b * kRow + c] = (c >= 21 && c < 27) ? -v : v;
    }
    cost[b] = (red[0][27] + red[1][27]) + (red[2][27] + red[3][27]);
  }
}

// odom_sum_partials
void sum_partials(const std::vector<double> &part, int nb, double *out) {
  double rdl[kRedLanes];
  const size_t tot = (size_t)nb * kRow;
  for (int t = 0; t < kRedLanes; t++) {
    double s = 0.0;
    for (size_t i = t; i < tot; i += kRedLanes) s += part[i];
    rdl[t] = s;
  }
  for (int t = 0; t < kRow; t++) {
    double s = rdl[t];
    for (int g = 1; g < 7; g++) s += rdl[t + kRow * g];
    out[t] = s;
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: surfodom_host IN OUT\n"); return 2; }
  FILE *fi = std::fopen(argv[1], "rb");
  if (!fi) { std::perror(argv[1]); return 2; }
  Head h;
  if (!rd(fi, &h, 1) || h.n_rec < 0 || h.n_pnt < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
  const size_t nr = (size_t)h.n_rec, np = (size_t)h.n_pnt;
  std::vector<float> rec(12 * nr);
  std::vector<double> cov(6 * nr), pnt(3 * np);
  if (!rd(fi, rec.data(), rec.size()) || !rd(fi, cov.data(), cov.size()) || !rd(fi, pnt.data(), pnt.size())) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(fi);

  // ---- the map: records in order, linear probing (tests/host/surfreg_host.cpp)
  size_t slots = 2;
  while (slots < 2 * nr) slots *= 2;
  std::vector<SregSlot> tab(slots);
  for (auto &s : tab) { s.key = DS_EMPTY; s.row = -1; s.pad = 0; }
  std::vector<SregCell> cell(nr ? nr : 1);
  int64_t n_cells = 0;
  const unsigned int mask = (unsigned int)(slots - 1);
  for (size_t i = 0; i < nr; i++) {
    const float *r = rec.data() + 12 * i;
    if (!(r[11] >= (float)h.min_count)) continue;
    const unsigned long long key = sreg_key(r, h.voxel);
    unsigned int s = ds_hash(key) & mask;
    bool mine = false;
    for (unsigned int probe = 0; probe <= mask; probe++) {
      if (tab[s].key == DS_EMPTY) { tab[s].key = key; mine = true; break; }
      if (tab[s].key == key) break;
      s = (s + 1) & mask;
    }
    if (!mine) { std::fprintf(stderr, "two records share a key\n"); return 2; }
    tab[s].row = (int)i;
    sreg_make_cell(r, cov.data() + 6 * i, h.sigma, &cell[i]);
    n_cells++;
  }
  SregTable T; T.tab = tab.data(); T.cell = cell.data(); T.mask = mask; T.voxel = h.voxel;

  // ---- the loop (odom_ekf_loop_host): every launch of the four checks `done` first
  const int nb = (int)(((np + 255) / 256) < (size_t)kMaxBlocks ? (np + 255) / 256 : (size_t)kMaxBlocks);
  std::vector<double> part((size_t)nb * kRow), cost((size_t)nb), tpart((size_t)nb * kRow), tcost((size_t)nb);
  std::vector<int32_t> tcell(np, -1);
  std::vector<uint8_t> tgate(np, 0);
  double tsums[kRow] = {0};
  double cov_inv[225];
  vbh::inverse_pplu(h.cov, cov_inv, 15);
  vbh::OdomEkf S;
  vbh::odom_ekf_begin(S, h.state, h.cov, cov_inv);
  for (int iter = 0; iter < vbh::ODOM_EKF_MAX_ITER; iter++) {
    if (S.done) continue;
    double w[vbh::OE_WORK] = {0};
    if (np > 0) point_loop(T, S, h, pnt, nb, part, cost, iter == 0 ? tcell.data() : nullptr, tgate.data());
    sum_partials(part, np > 0 ? nb : 0, w + vbh::OE_S34);
    if (iter == 0) { tpart = part; tcost = cost; std::memcpy(tsums, w + vbh::OE_S34, sizeof(tsums)); }
    vbh::odom_ekf_iterate((double *)w, &S, iter, 0, 1, NoSync(), h.kd);
  }
  const double eig_min = vbh::odom_nnt_eig_min(S.nnt);
  const int last = S.iterations > 0 ? S.match_num[S.iterations - 1] : 0;
  const int32_t ints[4] = {S.iterations, (last >= h.min_matches && eig_min >= h.min_eig) ? 1 : 0, S.rematch_num, 0};

  FILE *fo = std::fopen(argv[2], "wb");
  if (!fo) { std::perror(argv[2]); return 2; }
  const int64_t head[2] = {n_cells, (int64_t)nb};
  const bool ok = wr(fo, head, 2) && wr(fo, tcell.data(), np) && wr(fo, tgate.data(), np) && wr(fo, tpart.data(), tpart.size()) &&
                  wr(fo, tcost.data(), tcost.size()) && wr(fo, tsums, kRow) && wr(fo, &S.x_curr.t, 25) && wr(fo, S.P_out, 225) && wr(fo, S.nnt, 9) &&
                  wr(fo, S.rot_add, 4) && wr(fo, S.tra_add, 4) && wr(fo, S.match_num, 4) && wr(fo, ints, 4) && wr(fo, &eig_min, 1);
  if (std::fclose(fo) != 0 || !ok) { std::fprintf(stderr, "write failed\n"); return 2; }
  return 0;
}
