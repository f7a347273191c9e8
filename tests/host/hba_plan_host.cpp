// Host build of the bottom-layer plan of vba_hba_global (voxel-slam_amd/csrc/vba_hba_plan.hpp) for tests/test_hba_plan_cpu.py: a
// stand-alone program over the standard library.  `hba_plan_host plan n_kf wdsize mgsize n_ranks hba_workers off_0 .. off_n_kf`
// prints every field of the plan, one `name value` line each, then one line per window with the offset of its record; the test
// compares them with its own restatement.  Every other case checks itself and exits 0 when it holds.  Test harness only.
#include "../../voxel-slam_amd/csrc/vba_hba_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

using namespace vba;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static int case_plan(int argc, char **argv) {
  if (argc < 7) return 2;
  const int n_kf = std::atoi(argv[2]), wdsize = std::atoi(argv[3]), mgsize = std::atoi(argv[4]), n_ranks = std::atoi(argv[5]), opt = std::atoi(argv[6]);
  if (n_kf < 0 || argc != 7 + n_kf + 1) return 2;
  std::vector<int> off(n_kf + 1);
  for (int i = 0; i <= n_kf; i++) off[i] = std::atoi(argv[7 + i]);
  const HbaPlan P = hba_plan(n_kf, off.data(), wdsize, mgsize, n_ranks, opt);
  std::printf("mode %d\nn_win %d\nKL %d\nNR %d\n", (int)P.mode, P.n_win, P.KL, P.NR);
  std::printf("n_all %zu\nn_sub_cap %zu\nn_win_max %zu\nchunk_pts %zu\nmeta_per %zu\nwin_per_lane %zu\nmeta_chunk %zu\n", P.n_all, P.n_sub_cap, P.n_win_max,
              P.chunk_pts, P.meta_per, P.win_per_lane, P.meta_chunk);
  std::printf("meta_len %zu\nneed %zu\noff_sub %zu\noff_rep %zu\noff_meta %zu\n", P.meta_len, P.need, P.off_sub, P.off_rep, P.off_meta);
  std::vector<double> meta(P.meta_len + 1);
  for (int w = 0; w < P.n_win; w++) {
    const HbaWindow &x = P.win[w];
    const long rec = P.mode == HBA_SEQUENTIAL ? -1 : (long)(P.rec(meta.data(), w) - meta.data());      // one after the other keeps no records
    std::printf("win %d %d %d %zu %zu %ld\n", x.start, x.lane, x.slot, x.pts, x.roff, rec);
  }
  for (int r = 0; r < P.NR; r++) std::printf("lane_recs %ld\n", (long)(P.lane_recs(meta.data(), r) - meta.data()));
  return 0;
}

// ---------------------------------------------------------------- hba_append_edges
static std::vector<double> rows_of(int ne) {      // row e: indices (e, e + 1), then 100 e + column
  std::vector<double> r((size_t)(ne > 0 ? ne : 1) * 20);
  for (int e = 0; e < ne; e++)
    for (int k = 0; k < 20; k++) r[(size_t)e * 20 + k] = k == 0 ? e : k == 1 ? e + 1 : 100.0 * e + k;
  return r;
}
static bool row_is(const double *o, double i, double j, int e) {
  if (o[0] != i || o[1] != j) return false;
  for (int k = 2; k < 20; k++) if (o[k] != 100.0 * e + k) return false;
  return true;
}
static int case_append_shift() {
  const std::vector<double> r = rows_of(3);
  std::vector<double> dst(6 * 20, -1.0);
  int n = 2;                                       // two rows are there already
  REQUIRE(hba_append_edges(dst.data(), 6, &n, r.data(), 3, [](double i) { return i + 15; }) == HBA_PLAN_OK && n == 5);
  for (int e = 0; e < 3; e++) REQUIRE(row_is(&dst[(size_t)(2 + e) * 20], 15 + e, 16 + e, e));
  for (int k = 0; k < 40; k++) REQUIRE(dst[k] == -1.0 && dst[100 + k % 20] == -1.0);      // rows 0, 1 and 5 untouched
  return 0;
}
static int case_append_lookup() {
  const std::vector<double> r = rows_of(3);
  const std::vector<int> first = {0, 5, 10, 15};
  std::vector<double> dst(3 * 20, -1.0);
  int n = 0;
  REQUIRE(hba_append_edges(dst.data(), 3, &n, r.data(), 3, [&](double i) { return (double)first[(int)i]; }) == HBA_PLAN_OK && n == 3);
  for (int e = 0; e < 3; e++) REQUIRE(row_is(&dst[(size_t)e * 20], first[e], first[e + 1], e));
  return 0;
}
static int case_append_cap_exact() {
  const std::vector<double> r = rows_of(4);
  std::vector<double> dst(5 * 20, -1.0);
  int n = 1;
  REQUIRE(hba_append_edges(dst.data(), 5, &n, r.data(), 4, [](double i) { return i + 7; }) == HBA_PLAN_OK && n == 5);
  REQUIRE(row_is(&dst[4 * 20], 10, 11, 3));
  return 0;
}
static int case_append_cap_over() {
  const std::vector<double> r = rows_of(5);
  std::vector<double> dst(5 * 20, -1.0);           // (exactly cap rows: a write past the cap is the address sanitizer's to find)
  int n = 1;
  REQUIRE(hba_append_edges(dst.data(), 5, &n, r.data(), 5, [](double i) { return i + 7; }) == HBA_PLAN_ERR_CAPACITY && n == 5);
  for (int e = 0; e < 4; e++) REQUIRE(row_is(&dst[(size_t)(1 + e) * 20], 7 + e, 8 + e, e));
  int z = 0;                                       // no room at all: nothing is touched, not even a null destination
  REQUIRE(hba_append_edges(nullptr, 0, &z, r.data(), 1, [](double i) { return i; }) == HBA_PLAN_ERR_CAPACITY && z == 0);
  return 0;
}
static int case_append_empty() {
  std::vector<double> dst(20, -1.0);
  int n = 0, calls = 0;
  REQUIRE(hba_append_edges(dst.data(), 1, &n, nullptr, 0, [&](double i) { calls++; return i; }) == HBA_PLAN_OK && n == 0 && calls == 0);
  REQUIRE(hba_append_edges(dst.data(), 0, &n, nullptr, 0, [&](double i) { calls++; return i; }) == HBA_PLAN_OK && n == 0);
  REQUIRE(dst[0] == -1.0);
  return 0;
}

// ---------------------------------------------------------------- hba_run_lanes, hba_gate, hba_stop_at
// The lanes of the worker driver over 12 windows on 3 lanes: lane t takes windows t, t + 3, ...; a window first takes a ticket, then
// passes its gate; window `fail_at` lowers stop_after and takes a ticket after that.  `thrower` (lane, what): that lane throws at its
// second window.  The uploader opens the gate keyframe by keyframe, or throws at once.
struct Lanes {
  static const int KL = 3, NW = 12;
  std::atomic<int> kf_ready{0}, stop_after{NW}, ticket{0}, exited{0};
  std::atomic<int> ran[NW], seq[NW];
  int fail_at = -1, fail_seq = -1, throw_lane = -1, throw_what = 0, main_throws = 0, uploaded = 0;
  HbaPlan plan;                                    // 13 keyframes, windows of 2 at stride 1: window w needs keyframes w and w + 1
  Lanes() {
    for (int w = 0; w < NW; w++) { ran[w] = 0; seq[w] = -1; }
    std::vector<int> off(NW + 2);
    for (int i = 0; i < NW + 2; i++) off[i] = 10 * i;
    plan = hba_plan(NW + 1, off.data(), 2, 1, 1, KL);
  }
  int run() {
    auto work = [this](int lane) {
      struct Exit { std::atomic<int> &n; ~Exit() { n++; } } on_exit{exited};
      for (int w = lane; w < NW; w += KL) {
        seq[w] = ticket++;
        if (!hba_gate(kf_ready, plan.win[w].start + plan.wdsize, stop_after, w)) return;
        if (lane == throw_lane && w >= KL) { if (throw_what == 0) throw std::bad_alloc(); throw std::runtime_error("lane"); }
        ran[w] = 1;
        if (w == fail_at) { hba_stop_at(stop_after, w); fail_seq = ticket++; return; }
      }
    };
    auto upload = [this]() -> int {
      if (main_throws) throw std::runtime_error("uploader");
      for (int k0 = 0; k0 < NW + 1; k0++) {          // one keyframe per chunk, the loop of the worker driver's uploader
        // (the keyframes behind the failing window wait for its failure, so that what runs does not depend on the scheduler)
        while (fail_at >= 0 && k0 == fail_at + 2 && stop_after.load() == NW) std::this_thread::sleep_for(std::chrono::microseconds(20));
        if (!hba_upload_wanted(plan, stop_after.load(), k0)) break;
        kf_ready.store(k0 + 1, std::memory_order_release);
        uploaded = k0 + 1;
      }
      return HBA_PLAN_OK;
    };
    return hba_run_lanes(KL, stop_after, work, upload);
  }
};
static int case_upload_wanted() {
  std::vector<int> off(62);
  for (int i = 0; i < 62; i++) off[i] = 7 * i;
  const HbaPlan P = hba_plan(61, off.data(), 10, 5, 1, 2);      // 11 windows; window 3 is keyframes 15..24
  REQUIRE(P.n_win == 11 && P.win[3].start == 15);
  for (int k0 = 0; k0 < 61; k0++) {
    REQUIRE(hba_upload_wanted(P, 11, k0));                      // nobody failed: every keyframe goes up
    REQUIRE(!hba_upload_wanted(P, -1, k0));                     // everybody stops
    REQUIRE(hba_upload_wanted(P, 3, k0) == (k0 < 25));          // up to the last keyframe of the lowest failing window
    REQUIRE(hba_upload_wanted(P, 0, k0) == (k0 < 10) && hba_upload_wanted(P, 10, k0) == (k0 < 60));
  }
  return 0;
}
static int case_lanes_ok() {
  Lanes L;
  REQUIRE(L.plan.mode == HBA_WORKERS && L.plan.KL == Lanes::KL && L.plan.n_win == Lanes::NW);
  REQUIRE(L.run() == HBA_PLAN_OK && L.exited == Lanes::KL && L.stop_after == Lanes::NW && L.uploaded == Lanes::NW + 1);
  for (int w = 0; w < Lanes::NW; w++) REQUIRE(L.ran[w] == 1);
  return 0;
}
static int case_lanes_stop() {
  Lanes L;
  L.fail_at = 5;
  REQUIRE(L.run() == HBA_PLAN_OK && L.exited == Lanes::KL && L.stop_after == 5);      // a failing window is the records' to report, not the runner's
  for (int w = 0; w <= 5; w++) REQUIRE(L.ran[w] == 1);
  for (int w = 6; w < Lanes::NW; w++) REQUIRE(L.ran[w] == 0 || (L.seq[w] >= 0 && L.seq[w] < L.fail_seq));   // only what had started before
  REQUIRE(L.ran[Lanes::NW - 1] == 0 && L.uploaded == 5 + 2);                          // the uploader stopped behind window 5's keyframes
  int lo = 20;                                                                        // hba_stop_at only ever lowers
  std::atomic<int> s{lo};
  hba_stop_at(s, 7); hba_stop_at(s, 9); REQUIRE(s == 7);
  hba_stop_at(s, 7); hba_stop_at(s, 3); REQUIRE(s == 3);
  return 0;
}
static int lanes_throw(int what, int expect) {
  Lanes L;
  L.throw_lane = 1; L.throw_what = what;
  REQUIRE(L.run() == expect && L.exited == Lanes::KL && L.stop_after == -1);
  REQUIRE(L.ran[1] == 1 && L.ran[4] == 0);          // the lane's first window ran, the one it threw in did not
  return 0;
}
static int case_lanes_bad_alloc() { return lanes_throw(0, HBA_PLAN_ERR_CAPACITY); }
static int case_lanes_runtime_error() { return lanes_throw(1, HBA_PLAN_ERR_RUNTIME); }
static int case_main_throws() {
  Lanes L;
  L.main_throws = 1;                               // the gate never opens: the lanes end through stop_after = -1
  REQUIRE(L.run() == HBA_PLAN_ERR_RUNTIME && L.exited == Lanes::KL && L.stop_after == -1 && L.kf_ready == 0);
  for (int w = 0; w < Lanes::NW; w++) REQUIRE(L.ran[w] == 0);
  return 0;
}
static int case_main_status() {
  std::atomic<int> stop{4}, gate{0}, ended{0};     // a status of the uploader stops the lanes too, and comes back
  const int st = hba_run_lanes(2, stop, [&](int lane) { hba_gate(gate, 1, stop, lane); ended++; }, [] { return (int)HBA_PLAN_ERR_RUNTIME; });
  REQUIRE(st == HBA_PLAN_ERR_RUNTIME && ended == 2 && stop == -1);
  return 0;
}

int main(int argc, char **argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  if (which == "plan") return case_plan(argc, argv);
  if (which == "append_shift") return case_append_shift();
  if (which == "append_lookup") return case_append_lookup();
  if (which == "append_cap_exact") return case_append_cap_exact();
  if (which == "append_cap_over") return case_append_cap_over();
  if (which == "append_empty") return case_append_empty();
  if (which == "upload_wanted") return case_upload_wanted();
  if (which == "lanes_ok") return case_lanes_ok();
  if (which == "lanes_stop") return case_lanes_stop();
  if (which == "lanes_bad_alloc") return case_lanes_bad_alloc();
  if (which == "lanes_runtime_error") return case_lanes_runtime_error();
  if (which == "main_throws") return case_main_throws();
  if (which == "main_status") return case_main_status();
  std::fprintf(stderr, "unknown case '%s'\n", which.c_str());
  return 2;
}
