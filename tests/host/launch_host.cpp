// Host build of the product's launch plumbing (voxel-slam_amd/csrc/vba_launch.hpp) for tests/test_launch_cpu.py: a stand-alone
// program over a host stub of hipFuncSetAttribute, the one runtime call the header makes.  The stub counts its calls per "device"
// (the test sets the current device before each call, as the library's callers have) and fails on request.  `launch_host <case>`
// exits 0 when the case holds.  Test harness only.
#include "../../include/voxelba.h"
#include "../../voxel-slam_amd/csrc/vba_launch.hpp"

#include <atomic>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

static thread_local int t_device = 0;                     // what hipGetDevice would say on the calling thread
static std::atomic<int> g_calls[vba::kMaxDevices + 2];    // stub calls per device index, shifted by one (slot 0: device -1)
static std::atomic<int> g_bad_args{0};
static std::atomic<bool> g_fail{false};
static const int kKernelA = 0, kKernelB = 0;              // stand-ins for two kernels' addresses

extern "C" hipError_t hipFuncSetAttribute(const void *func, hipFuncAttribute attr, int value) {
  if ((func != &kKernelA && func != &kKernelB) || attr != hipFuncAttributeMaxDynamicSharedMemorySize || value != 98304) g_bad_args++;
  g_calls[t_device + 1]++;
  return g_fail ? hipErrorInvalidValue : hipSuccess;
}
static int calls(int device) { return g_calls[device + 1]; }
static hipError_t ask(vba::LdsOptIn &o, int device, const void *k = &kKernelA) { t_device = device; return o(device, k, 98304); }

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// every w of [LO, HI] reaches the functor once, with its own constant, and the functor's status comes back (non-zero included);
// the listed outsiders give VBA_ERR_UNSUPPORTED_WINDOW and never enter it
template <int LO, int HI>
static int dispatch(std::vector<int> outside) {
  int entered = 0, seen = -1;
  auto f = [&](auto wc) { entered++; seen = decltype(wc)::value; return 1000 + 7 * decltype(wc)::value; };
  for (int w = LO; w <= HI; w++) {
    entered = 0; seen = -1;
    REQUIRE((vba::for_window<LO, HI>(w, f)) == 1000 + 7 * w && entered == 1 && seen == w);
    REQUIRE((vba::for_window<LO, HI>(w, [&](auto) { entered++; return 0; })) == 0 && entered == 2);
  }
  entered = 0;
  for (int w : outside) REQUIRE((vba::for_window<LO, HI>(w, f)) == VBA_ERR_UNSUPPORTED_WINDOW && entered == 0);
  return 0;
}
static int case_window_2_16() { return dispatch<2, 16>({1, 0, -1, 17}); }
static int case_window_2_10() { return dispatch<2, 10>({11, 1, 17}); }

static int case_opt_in() {
  vba::LdsOptIn a;
  REQUIRE(ask(a, 0) == hipSuccess && calls(0) == 1);                          // the first call asks the runtime
  REQUIRE(ask(a, 0) == hipSuccess && ask(a, 0) == hipSuccess && calls(0) == 1);   // later ones on that device do not
  REQUIRE(ask(a, 3) == hipSuccess && calls(3) == 1 && ask(a, 3) == hipSuccess && calls(3) == 1 && calls(0) == 1);   // another device does, once
  REQUIRE(g_bad_args == 0);                                                   // kernel, attribute and byte count as given
  return 0;
}

static int case_opt_in_failure() {
  vba::LdsOptIn a;
  g_fail = true;
  REQUIRE(ask(a, 5) == hipErrorInvalidValue && calls(5) == 1);
  REQUIRE(ask(a, 5) == hipErrorInvalidValue && calls(5) == 2);                // not remembered: asked again, refused again
  g_fail = false;
  REQUIRE(ask(a, 5) == hipSuccess && calls(5) == 3);                          // the retry succeeds ...
  REQUIRE(ask(a, 5) == hipSuccess && calls(5) == 3);                          // ... and is remembered
  return 0;
}

static int case_opt_in_out_of_range() {
  vba::LdsOptIn a;
  for (int k = 1; k <= 3; k++) {
    REQUIRE(ask(a, -1) == hipSuccess && calls(-1) == k);                      // never cached, never aliased onto a flag in range
    REQUIRE(ask(a, vba::kMaxDevices) == hipSuccess && calls(vba::kMaxDevices) == k);
  }
  REQUIRE(ask(a, 0) == hipSuccess && calls(0) == 1 && ask(a, vba::kMaxDevices - 1) == hipSuccess && calls(vba::kMaxDevices - 1) == 1);
  REQUIRE(ask(a, 0) == hipSuccess && calls(0) == 1 && ask(a, vba::kMaxDevices - 1) == hipSuccess && calls(vba::kMaxDevices - 1) == 1);
  return 0;
}

static int case_opt_in_instances() {
  vba::LdsOptIn a, b;                                                         // two kernels with one signature: one instance each
  REQUIRE(ask(a, 2, &kKernelA) == hipSuccess && calls(2) == 1);
  REQUIRE(ask(b, 2, &kKernelB) == hipSuccess && calls(2) == 2);               // a's flag says nothing about b
  REQUIRE(ask(a, 2, &kKernelA) == hipSuccess && ask(b, 2, &kKernelB) == hipSuccess && calls(2) == 2);
  REQUIRE(g_bad_args == 0);
  return 0;
}

// 8 threads, 1000 calls each on ONE instance over two devices, as the first launches of side-by-side contexts make them
static int case_opt_in_threads() {
  static vba::LdsOptIn a;                                                     // (as at the call sites: a function-local static)
  std::atomic<int> failures{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; t++)
    ts.emplace_back([&, t] { for (int i = 0; i < 1000; i++) if (ask(a, (t + i) & 1) != hipSuccess) failures++; });
  for (auto &t : ts) t.join();
  REQUIRE(failures == 0);
  for (int d = 0; d < 2; d++) REQUIRE(calls(d) >= 1 && calls(d) <= 8);        // both may find the flag clear; nobody asks twice
  return 0;
}

int main(int argc, char **argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  if (which == "window_2_16") return case_window_2_16();
  if (which == "window_2_10") return case_window_2_10();
  if (which == "opt_in") return case_opt_in();
  if (which == "opt_in_failure") return case_opt_in_failure();
  if (which == "opt_in_out_of_range") return case_opt_in_out_of_range();
  if (which == "opt_in_instances") return case_opt_in_instances();
  if (which == "opt_in_threads") return case_opt_in_threads();
  std::fprintf(stderr, "unknown case '%s'\n", which.c_str());
  return 2;
}
