// Host build of the product's owning buffer types (voxel-slam_amd/csrc/vba_mem.hpp) for tests/test_mem_cpu.py: a stand-alone
// program over host stubs of the eight runtime calls the header makes.  The stubs allocate with malloc, count the live blocks, log
// the order of allocations and frees, and fail the k-th allocation or the next copy on request.  `mem_host <case>` exits 0 when the
// case holds; every case also requires that no block is live when it ends.  Test harness only.
#include "../../voxel-slam_amd/csrc/vba_mem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

static std::set<void *> g_live;
static std::string g_log;              // 'A' per allocation, 'F' per free, 'C' per copy, 'Z' per fill, 'S' per synchronise
static int g_allocs = 0, g_fail_alloc = 0;   // the g_fail_alloc-th allocation from now fails (0: none)
static bool g_fail_copy = false;

static hipError_t stub_alloc(void **p, size_t bytes) {
  if (g_fail_alloc && --g_fail_alloc == 0) { *p = (void *)0x1; return hipErrorOutOfMemory; }   // (a failed call may leave garbage)
  *p = std::malloc(bytes ? bytes : 1);
  g_live.insert(*p); g_log += 'A'; g_allocs++;
  return hipSuccess;
}
static hipError_t stub_free(void *p) {
  if (!g_live.erase(p)) { std::fprintf(stderr, "free of a block that is not live\n"); std::abort(); }
  std::free(p); g_log += 'F';
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return stub_alloc(p, bytes); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return stub_alloc(p, bytes); }
hipError_t hipFree(void *p) { return stub_free(p); }
hipError_t hipHostFree(void *p) { return stub_free(p); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
  if (g_fail_copy) { g_fail_copy = false; return hipErrorInvalidValue; }
  std::memcpy(dst, src, bytes); g_log += 'C';
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t) {
  if (g_fail_copy) { g_fail_copy = false; return hipErrorInvalidValue; }
  for (size_t r = 0; r < height; r++) std::memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
  g_log += 'C';
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) { std::memset(dst, value, bytes); g_log += 'Z'; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { g_log += 'S'; return hipSuccess; }
}

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

using vba::DevMem;
using vba::PinMem;

template <class M>
static int case_ensure() {
  M m;
  g_allocs = 0;
  REQUIRE(m.p == nullptr && m.n == 0 && !m);
  REQUIRE(m.ensure(0) == hipSuccess && g_allocs == 0);                  // nothing asked for
  REQUIRE(m.ensure(100) == hipSuccess && m.p && m.n == 100 && g_allocs == 1);
  for (size_t i = 0; i < 100; i++) m.p[i] = (int)i;                       // exactly 100 elements are writable (the sanitizer checks)
  int *was = m.p;
  REQUIRE(m.ensure(40) == hipSuccess && m.ensure(100) == hipSuccess && m.p == was && m.n == 100 && g_allocs == 1);   // below, at capacity
  g_log.clear();
  REQUIRE(m.ensure(101) == hipSuccess && m.n == 101 && g_log == "FA" && g_live.size() == 1);   // growth frees before it allocates
  int *q = m;                                                              // the conversion existing uses rely on
  REQUIRE(q == m.p && m + 1 == m.p + 1);
  return 0;
}

template <class M>
static int case_failed_ensure() {
  M m;
  REQUIRE(m.ensure(8) == hipSuccess);
  g_fail_alloc = 1;
  REQUIRE(m.ensure(16) == hipErrorOutOfMemory && m.p == nullptr && m.n == 0 && g_live.empty());
  REQUIRE(m.ensure(16) == hipSuccess && m.p && m.n == 16 && g_live.size() == 1);
  g_fail_alloc = 1;
  M e;
  REQUIRE(e.ensure(4) == hipErrorOutOfMemory && e.p == nullptr && e.n == 0);
  return 0;
}

static int case_move() {
  DevMem<int> a;
  REQUIRE(a.ensure(10) == hipSuccess);
  int *pa = a.p;
  DevMem<int> b(std::move(a));                                             // construction
  REQUIRE(a.p == nullptr && a.n == 0 && b.p == pa && b.n == 10 && g_live.size() == 1);
  DevMem<int> c;
  REQUIRE(c.ensure(3) == hipSuccess && g_live.size() == 2);
  c = std::move(b);                                                        // assignment frees what the target held
  REQUIRE(b.p == nullptr && b.n == 0 && c.p == pa && c.n == 10 && g_live.size() == 1);
  DevMem<int> &self = c;
  c = std::move(self);                                                     // to itself: unchanged
  REQUIRE(c.p == pa && c.n == 10 && g_live.size() == 1);
  PinMem<double> h, k;
  REQUIRE(h.ensure(5) == hipSuccess);
  std::swap(h, k);
  REQUIRE(h.p == nullptr && k.n == 5 && g_live.size() == 2);
  return 0;
}

static int case_reset() {
  DevMem<int> a;
  a.reset();                                                               // empty: nothing to free
  REQUIRE(g_log.empty());
  REQUIRE(a.ensure(7) == hipSuccess);
  a.reset();
  REQUIRE(a.p == nullptr && a.n == 0 && g_live.empty() && g_log == "AF");
  a.reset();
  REQUIRE(g_log == "AF");
  REQUIRE(a.ensure(2) == hipSuccess && a.n == 2);                          // usable again
  return 0;
}

static int case_grow_keep() {
  DevMem<int> a;
  REQUIRE(a.grow_keep(8, 0, nullptr) == hipSuccess && a.n == 8 && g_log == "A");   // no old block: no copy, no synchronise
  for (int i = 0; i < 8; i++) a.p[i] = 100 + i;
  g_log.clear();
  REQUIRE(a.grow_keep(32, 5, nullptr) == hipSuccess && a.n == 32 && g_log == "ACSF" && g_live.size() == 1);
  for (int i = 0; i < 5; i++) REQUIRE(a.p[i] == 100 + i);
  a.p[31] = 1;
  g_log.clear();
  REQUIRE(a.grow_keep(64, 0, nullptr) == hipSuccess && g_log == "ASF");            // nothing kept: still drained before the free
  return 0;
}

static int case_grow_keep_alloc_fails() {
  DevMem<int> a;
  REQUIRE(a.ensure(8) == hipSuccess);
  for (int i = 0; i < 8; i++) a.p[i] = i;
  int *was = a.p;
  g_fail_alloc = 1;
  REQUIRE(a.grow_keep(16, 8, nullptr) == hipErrorOutOfMemory && a.p == was && a.n == 8 && g_live.size() == 1);
  for (int i = 0; i < 8; i++) REQUIRE(a.p[i] == i);
  return 0;
}

static int case_grow_keep_copy_fails() {
  DevMem<int> a;
  REQUIRE(a.ensure(8) == hipSuccess);
  for (int i = 0; i < 8; i++) a.p[i] = i;
  int *was = a.p;
  g_fail_copy = true;
  REQUIRE(a.grow_keep(16, 8, nullptr) == hipErrorInvalidValue && a.p == was && a.n == 8 && g_live.size() == 1);   // the new block is gone
  for (int i = 0; i < 8; i++) REQUIRE(a.p[i] == i);
  return 0;
}

// ---------------------------------------------------------------- grow_family: [rows][cap] arrays that share one capacity
struct Arr { size_t elem, rows; };
static const std::vector<Arr> kFam = {{8, 1}, {4, 3}, {24, 2}};      // different element sizes and row counts
static unsigned char fam_byte(size_t a, size_t row, size_t col, size_t b) { return (unsigned char)(1 + 61 * a + 17 * row + 5 * col + b); }

// a family at capacity `cap` whose every byte tells its array, row, column and byte
static int fam_make(std::vector<DevMem<char>> &own, size_t cap) {
  REQUIRE(vba::grow_family(own, kFam, 0, cap, 0, nullptr) == hipSuccess && own.size() == kFam.size());
  for (size_t a = 0; a < kFam.size(); a++) {
    REQUIRE(own[a].n == kFam[a].elem * kFam[a].rows * cap);
    for (size_t r = 0; r < kFam[a].rows; r++)
      for (size_t c = 0; c < cap; c++)
        for (size_t b = 0; b < kFam[a].elem; b++) own[a].p[(r * cap + c) * kFam[a].elem + b] = (char)fam_byte(a, r, c, b);
  }
  return 0;
}
// [rows][used] of every array as fam_make wrote it at stride `cap`, everything else `rest` (-1: not looked at)
static int fam_check(const std::vector<DevMem<char>> &own, size_t cap, size_t used, int rest) {
  for (size_t a = 0; a < kFam.size(); a++)
    for (size_t r = 0; r < kFam[a].rows; r++)
      for (size_t c = 0; c < cap; c++)
        for (size_t b = 0; b < kFam[a].elem; b++) {
          const unsigned char got = (unsigned char)own[a].p[(r * cap + c) * kFam[a].elem + b];
          if (c < used) REQUIRE(got == fam_byte(a, r, c, b));
          else if (rest >= 0) REQUIRE(got == (unsigned char)rest);
        }
  return 0;
}

static int case_family_grow() {
  std::vector<DevMem<char>> own;
  g_log.clear();
  REQUIRE(fam_make(own, 5) == 0 && g_log == "AZAZAZS");                    // first allocation: nothing to copy, one synchronise
  g_log.clear();
  REQUIRE(vba::grow_family(own, kFam, 5, 16, 3, nullptr) == hipSuccess);
  REQUIRE(g_log == "AZCAZCAZCSFFF" && g_live.size() == 3);                 // one synchronise for the family, the frees after it
  for (size_t a = 0; a < kFam.size(); a++) REQUIRE(own[a].n == kFam[a].elem * kFam[a].rows * 16);
  REQUIRE(fam_check(own, 16, 3, 0) == 0);                                  // [rows][3] at the new stride, the rest zero
  g_log.clear();
  REQUIRE(vba::grow_family(own, kFam, 16, 32, 0, nullptr) == hipSuccess && g_log == "AZAZAZSFFF");   // nothing kept: still drained first
  return 0;
}

// the failing step leaves every old block, pointer and size as it was and no block live beyond them
template <class Arm>
static int family_failure(Arm arm, hipError_t want) {
  std::vector<DevMem<char>> own;
  REQUIRE(fam_make(own, 5) == 0);
  char *was[3] = {own[0].p, own[1].p, own[2].p};
  arm();
  g_log.clear();
  REQUIRE(vba::grow_family(own, kFam, 5, 16, 5, nullptr) == want);
  g_fail_alloc = 0; g_fail_copy = false;
  REQUIRE(own.size() == 3 && g_live.size() == 3 && g_log.find('S') == std::string::npos);
  for (size_t a = 0; a < 3; a++) REQUIRE(own[a].p == was[a] && own[a].n == kFam[a].elem * kFam[a].rows * 5 && g_live.count(was[a]));
  REQUIRE(fam_check(own, 5, 5, -1) == 0);
  REQUIRE(vba::grow_family(own, kFam, 5, 16, 5, nullptr) == hipSuccess && fam_check(own, 16, 5, 0) == 0);   // and grows when asked again
  return 0;
}
static int case_family_alloc_fails() {
  for (int k = 1; k <= 3; k++)
    if (family_failure([k] { g_fail_alloc = k; }, hipErrorOutOfMemory)) return 1;
  return 0;
}
static int case_family_copy_fails() { return family_failure([] { g_fail_copy = true; }, hipErrorInvalidValue); }

int main(int argc, char **argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  int r = 2;
  if (which == "ensure") r = case_ensure<DevMem<int>>() || case_ensure<PinMem<int>>();
  else if (which == "failed_ensure") r = case_failed_ensure<DevMem<int>>() || case_failed_ensure<PinMem<int>>();
  else if (which == "move") r = case_move();
  else if (which == "reset") r = case_reset();
  else if (which == "grow_keep") r = case_grow_keep();
  else if (which == "grow_keep_alloc_fails") r = case_grow_keep_alloc_fails();
  else if (which == "grow_keep_copy_fails") r = case_grow_keep_copy_fails();
  else if (which == "family_grow") r = case_family_grow();
  else if (which == "family_alloc_fails") r = case_family_alloc_fails();
  else if (which == "family_copy_fails") r = case_family_copy_fails();
  else std::fprintf(stderr, "unknown case '%s'\n", which.c_str());
  if (r == 0 && !g_live.empty()) { std::fprintf(stderr, "%zu blocks live at exit\n", g_live.size()); r = 3; }
  return r;
}
