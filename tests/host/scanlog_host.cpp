// The ring bookkeeping of the scan log (csrc/vba_scanlog_ring.hpp) on the CPU, stand-alone: the header needs the standard library
// only.  Built with the address and undefined-behaviour sanitizers by tests/test_scanlog_cpu.py and run one case per process.  A
// model arena (one int per point holding the number of the scan that owns it, -1 = free) is kept beside the ring: every push must
// land on free points inside the arena, every release frees exactly the scan's points.
#include "../../voxel-slam_amd/csrc/vba_scanlog_ring.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using vba::ScanRing;

static int g_fail = 0;
#define EXPECT(cond)                                                                   \
  do {                                                                                 \
    if (!(cond)) { std::fprintf(stderr, "%s:%d: EXPECT(%s)\n", __FILE__, __LINE__, #cond); g_fail++; } \
  } while (0)

struct Model {
  ScanRing r;
  std::vector<long long> owner;        // per arena point
  void init(int64_t cap, size_t scans) { r.set_cap(cap); r.reserve_scans(scans); owner.assign((size_t)cap, -1); }
  // the store's push: grow when the bookkeeping says so, as log_place does
  int64_t push(int64_t n, bool *grew = nullptr) {
    if (grew) *grew = false;
    if (r.table_full()) r.reserve_scans(r.scan_cap() ? 2 * r.scan_cap() : 4);
    if (r.place(n) < 0) {
      const int64_t nc = r.grown_cap(n, 8);
      std::vector<ScanRing::Move> mv;
      std::vector<long long> nw((size_t)nc, -1);
      r.rebase(nc, &mv);
      int64_t expect_to = 0;
      for (const auto &m : mv) {
        EXPECT(m.to == expect_to);                                     // packed from 0, in order
        for (int64_t j = 0; j < m.n; j++) { EXPECT(owner[(size_t)(m.from + j)] >= 0); nw[(size_t)(m.to + j)] = owner[(size_t)(m.from + j)]; }
        expect_to += m.n;
      }
      owner.swap(nw);
      if (grew) *grew = true;
    }
    const int64_t at = r.place(n);
    EXPECT(at >= 0 && at + n <= r.cap());
    for (int64_t j = 0; j < n; j++) { EXPECT(owner[(size_t)(at + j)] == -1); }
    const int64_t seq = r.push(n);
    EXPECT(r.start(seq) == at && r.size(seq) == n);
    for (int64_t j = 0; j < n; j++) owner[(size_t)(at + j)] = seq;
    check();
    return seq;
  }
  void release(int64_t upto) {
    const int64_t f = r.first(), e = r.end();
    r.release(upto);
    for (auto &o : owner) if (o >= f && o < upto && o < e) o = -1;
    check();
  }
  // every live scan owns exactly its rows; nothing else is owned
  void check() {
    long long owned = 0;
    for (auto o : owner) if (o >= 0) { owned++; EXPECT(r.live(o)); }
    EXPECT(owned == r.live_points());
    for (int64_t s = r.first(); s < r.end(); s++)
      for (int64_t j = 0; j < r.size(s); j++) EXPECT(owner[(size_t)(r.start(s) + j)] == s);
  }
};

static void case_sizes() {          // scans of 0, 1 and cap points
  Model m; m.init(16, 8);
  EXPECT(m.r.first() == 0 && m.r.end() == 0 && m.r.fits(16) && !m.r.fits(17));
  EXPECT(m.push(0) == 0);
  EXPECT(m.push(1) == 1 && m.r.start(1) == 0);
  m.release(2);
  EXPECT(m.r.scans() == 0 && m.r.first() == 2);
  EXPECT(m.push(16) == 2 && m.r.start(2) == 0);                      // nothing live: the ring is rewound, a whole-arena scan fits
  EXPECT(!m.r.fits(1) && m.r.fits(0));
  EXPECT(m.push(0) == 3 && m.r.start(3) == 16 && m.r.size(3) == 0);   // an empty scan takes no room, even in a full arena
  EXPECT(m.r.cap() == 16);
}

static void case_exact_tail() {     // a push that exactly fills the tail
  Model m; m.init(16, 8);
  m.push(6); m.push(6);
  EXPECT(m.r.place(4) == 12);
  m.push(4);
  EXPECT(m.r.head() == 16 && !m.r.wrapped() && !m.r.fits(1));
  m.release(1);
  EXPECT(m.r.place(6) == 0 && m.r.place(7) < 0);                     // [0, 6) is free again
  m.push(6);
  EXPECT(m.r.wrapped() && m.r.start(3) == 0 && !m.r.fits(1));
}

static void case_skip_tail() {      // a push that skips the tail
  Model m; m.init(16, 8);
  m.push(5); m.push(5); m.push(3);                                    // head 13, tail gap 3
  EXPECT(m.r.place(4) < 0);                                           // tail too short, nothing released yet
  m.release(1);
  EXPECT(m.r.place(4) == 0 && m.r.place(5) == 0 && m.r.place(6) < 0 && m.r.place(3) == 13);
  const int64_t s = m.push(4);
  EXPECT(m.r.start(s) == 0 && m.r.wrapped());
  EXPECT(m.r.start(1) == 5 && m.r.start(2) == 10);                    // consecutive scans are not contiguous: 10..13 then 0..4
  EXPECT(m.r.place(1) == 4 && m.r.place(2) < 0);                      // wrapped: free = [4, 5); the skipped [13, 16) stays unusable
  m.push(0);                                                          // an empty scan while wrapped and nearly full
  EXPECT(m.r.wrapped() && m.r.place(2) < 0);
  m.release(3);                                                       // the oldest scan is now past the wrap
  EXPECT(!m.r.wrapped() && m.r.tail() == 0 && m.r.head() == 4 && m.r.place(12) == 4 && m.r.place(13) < 0);
}

static void case_release() {        // release of part and of all of the log
  Model m; m.init(32, 8);
  for (int i = 0; i < 5; i++) m.push(4);
  m.release(0);
  EXPECT(m.r.first() == 0 && m.r.scans() == 5);
  m.release(2);
  EXPECT(m.r.first() == 2 && m.r.end() == 5 && m.r.live_points() == 12 && !m.r.live(1) && m.r.live(2) && !m.r.live(5));
  EXPECT(m.r.live_range(2, 3) && !m.r.live_range(1, 2) && !m.r.live_range(3, 3) && m.r.live_range(5, 0) && !m.r.live_range(2, -1));
  m.release(100);                                                     // past the end: everything goes, the numbers go on
  EXPECT(m.r.scans() == 0 && m.r.first() == 5 && m.r.end() == 5 && m.r.live_points() == 0);
  EXPECT(m.push(32) == 5 && m.r.start(5) == 0);
  // the scan table is a ring of its own: many pushes and releases through 8 records
  m.release(6);
  for (int i = 0; i < 50; i++) { const int64_t s = m.push(3); EXPECT(s == 6 + i); m.release(s); }
  EXPECT(m.r.scan_cap() == 8 && m.r.cap() == 32);
}

static void case_growth() {         // a full arena forces growth; numbers and starts before and after
  Model m; m.init(16, 4);
  m.push(5); m.push(5); m.push(3);
  m.release(1);
  m.push(4);                                                          // wrapped: scans 1 (5..10), 2 (10..13), 3 (0..4)
  EXPECT(m.r.first() == 1 && m.r.end() == 4 && m.r.start(1) == 5 && m.r.start(2) == 10 && m.r.start(3) == 0);
  bool grew = false;
  const int64_t s = m.push(6, &grew);                                 // does not fit in [4, 5)
  EXPECT(grew && s == 4 && m.r.cap() == 32 && !m.r.wrapped());
  EXPECT(m.r.first() == 1 && m.r.end() == 5);                         // numbers kept
  EXPECT(m.r.start(1) == 0 && m.r.start(2) == 5 && m.r.start(3) == 8 && m.r.start(4) == 12);   // re-based in order, packed
  EXPECT(m.r.size(1) == 5 && m.r.size(2) == 3 && m.r.size(3) == 4 && m.r.size(4) == 6);
  // a scan larger than twice the arena: doubled until it fits
  const int64_t t = m.push(100, &grew);
  EXPECT(grew && m.r.cap() == 128 && m.r.start(t) == 18);
  // the scan table grows too (4 -> 8) and keeps its records
  EXPECT(m.r.scans() == 5);
  m.push(1); m.push(1); m.push(1);
  EXPECT(m.r.scan_cap() >= 8 && m.r.start(1) == 0 && m.r.first() == 1 && m.r.end() == 9);
  // an empty log grows from the floor
  Model e; e.r.reserve_scans(2);
  e.owner.clear();
  EXPECT(e.r.cap() == 0 && e.r.place(3) < 0 && e.r.place(0) == 0);
  EXPECT(e.push(3, &grew) == 0 && grew && e.r.cap() == 8);
}

static void case_reserve_condition() {   // the condition of vba_scanlog_reserve: s live scans of at most m points fit (s + 1) m for ever
  const int64_t mpts = 7; const int live = 4;
  Model m; m.init((live + 1) * mpts, live);
  unsigned x = 12345;
  for (int i = 0; i < 2000; i++) {
    x = x * 1664525u + 1013904223u;
    const int64_t n = (x >> 16) % (mpts + 1);
    if ((int)m.r.scans() == live) m.release(m.r.first() + 1 + (x >> 28) % live);
    bool grew = false;
    m.push(n, &grew);
    EXPECT(!grew);
  }
  EXPECT(m.r.cap() == (live + 1) * mpts && m.r.scan_cap() == (size_t)live && m.r.end() == 2000);
}

int main(int argc, char **argv) {
  const std::string c = argc > 1 ? argv[1] : "";
  if (c == "sizes") case_sizes();
  else if (c == "exact_tail") case_exact_tail();
  else if (c == "skip_tail") case_skip_tail();
  else if (c == "release") case_release();
  else if (c == "growth") case_growth();
  else if (c == "reserve_condition") case_reserve_condition();
  else { std::fprintf(stderr, "unknown case '%s'\n", c.c_str()); return 2; }
  return g_fail ? 1 : 0;
}
