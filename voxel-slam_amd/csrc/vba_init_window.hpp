// Host side of the initialisation window (vba_init_window_*) that needs no device: the ragged offsets of pl_origs, the
// growth rule of its buffers and the checks of pushed arrays.  Plain C++ (tests/host/init_window_host.cpp builds it with g++ under
// the sanitizers); vba_init.hip owns the buffers and the launches.  It defines no kernel.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vba {

// rows before every scan, and their total: pl_origs.size() = scans(), never empty
struct InitWindowIndex {
  std::vector<int64_t> off{0};

  int scans() const { return (int)off.size() - 1; }
  int64_t rows() const { return off.back(); }
  void clear() { off.assign(1, 0); }                                   // pl_origs.clear() (VS:795)
  void append(int64_t n) { off.push_back(off.back() + (n > 0 ? n : 0)); }
  // rows [*first, *first + *n) of one scan; false: no such scan
  bool range(int scan, int64_t *first, int64_t *n) const {
    if (scan < 0 || scan >= scans()) return false;
    *first = off[(size_t)scan]; *n = off[(size_t)scan + 1] - off[(size_t)scan];
    return true;
  }
  // [scans() + 1] offsets; out may be NULL
  void copy_to(int64_t *out) const { if (out) std::memcpy(out, off.data(), off.size() * sizeof(int64_t)); }
  // the int offsets vba_motion_init's body takes: false when the window does not hold exactly W scans or its rows exceed an int
  bool as_int(int W, std::vector<int> *pto) const {
    if (W < 0 || scans() != W || rows() > (int64_t)INT_MAX) return false;
    pto->resize((size_t)W + 1);
    for (int i = 0; i <= W; i++) (*pto)[(size_t)i] = (int)off[(size_t)i];
    return true;
  }
};

// capacity after growing to at least `need`: doubling from the current one (from `first` when there is none); 0 when it would pass
// `limit`
inline size_t init_window_grow(size_t have, size_t first, size_t need, size_t limit) {
  size_t m = have ? have : first;
  while (m < need) {
    if (m > limit / 2) return 0;
    m *= 2;
  }
  return m <= limit ? m : 0;
}

// curvature ascends (the walk of vba_motion_init_resident searches it); a NaN fails
inline bool init_window_ascends(int n, const double *curv) {
  for (int k = 1; k < n; k++)
    if (!(curv[k - 1] <= curv[k])) return false;
  return n <= 0 || curv[0] == curv[0];
}

// arguments of vba_init_window_push_points / _reserve that can be judged without a device
inline bool init_window_points_args_ok(int n, const double *pnt, const double *curv) { return n >= 0 && (n == 0 || (pnt && curv)); }
inline bool init_window_reserve_args_ok(int max_scans, int max_points_per_scan) {
  return max_scans >= 0 && max_points_per_scan >= 0 && max_points_per_scan <= (1 << 28);
}

}  // namespace vba
