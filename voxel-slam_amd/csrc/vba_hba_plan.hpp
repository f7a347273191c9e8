// The host plan of the hierarchical global BA's bottom layer (vba_hba_global, DESIGN.md "The drivers of vba_hba_global"): which
// windows there are, which lane (worker context or rank) owns each, where a window's cloud lies inside its lane's chunk, how large the
// call's device buffer is and where its parts start; the one append loop of edge rows; the runner of the worker lanes.  Host code over
// the standard library only: no runtime call, no context, no pointer into device memory is followed.  Tested stand-alone under the
// sanitizers (tests/host/hba_plan_host.cpp).
#pragma once
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

namespace vba {

// the statuses this header returns: the values of VBA_OK, VBA_ERR_HIP and VBA_ERR_CAPACITY (include/voxelba.h; the unit asserts it)
enum { HBA_PLAN_OK = 0, HBA_PLAN_ERR_RUNTIME = 6, HBA_PLAN_ERR_CAPACITY = 7 };

enum HbaMode { HBA_SEQUENTIAL, HBA_WORKERS, HBA_REPLICAS };

struct HbaWindow {
  int start, lane, slot;      // first keyframe; the owner w % NR; the owner's slot w / NR
  size_t pts, roff;           // points of the window's keyframes; offset of its cloud inside the lane's chunk, in points (0: sequential)
};

struct HbaPlan {
  HbaMode mode = HBA_SEQUENTIAL;
  int wdsize = 0, mgsize = 0, n_win = 0, KL = 1, NR = 1;      // KL worker lanes (1: none), NR lanes in all (ranks or workers)
  size_t n_all = 0, n_sub_cap = 0, n_win_max = 0;             // points of all keyframes, of all windows, of the largest window
  size_t chunk_pts = 0, meta_per = 0, win_per_lane = 0, meta_chunk = 0, meta_len = 0;   // a lane's cloud chunk in points; doubles per record, records and doubles per lane, doubles of all lanes
  size_t need = 0, off_sub = 0, off_rep = 0, off_meta = 0;    // doubles of d_hba_all: [keyframe clouds | submap clouds | NR cloud chunks | NR record chunks | 64]
  std::vector<HbaWindow> win;
  // the record chunk of a lane in the NR chunks at `meta`, and in it the [n_cloud, n_edges, status | edge rows] record of window w
  // (the two chunked modes only: HBA_SEQUENTIAL has meta_len == 0 and keeps no records)
  template <class T> T *lane_recs(T *meta, int lane) const { return meta + (size_t)lane * meta_chunk; }
  template <class T> T *rec(T *meta, int w) const { return lane_recs(meta, win[w].lane) + meta_per * (size_t)win[w].slot; }
};

// n_ranks: 1 when the context has no collective.  hba_workers: vba_options::hba_workers (0: the default of 4; at most 8).
inline HbaPlan hba_plan(int n_kf, const int *offsets, int wdsize, int mgsize, int n_ranks, int hba_workers) {
  HbaPlan P;
  P.wdsize = wdsize; P.mgsize = mgsize;
  P.n_all = (size_t)offsets[n_kf];
  for (int start = 0; start + wdsize <= n_kf; start += mgsize) {
    HbaWindow w{start, 0, 0, (size_t)(offsets[start + wdsize] - offsets[start]), 0};
    P.n_sub_cap += w.pts;
    if (w.pts > P.n_win_max) P.n_win_max = w.pts;
    P.win.push_back(w);
  }
  P.n_win = (int)P.win.size();
  // replicas across ranks; else worker contexts side by side once every one of them has two windows; else one window after the other
  const int kl_opt = hba_workers > 0 ? (hba_workers < 8 ? hba_workers : 8) : 4;
  P.KL = (n_ranks <= 1 && P.n_win >= 2 * kl_opt) ? kl_opt : 1;
  P.mode = n_ranks > 1 ? HBA_REPLICAS : P.KL > 1 ? HBA_WORKERS : HBA_SEQUENTIAL;
  P.NR = n_ranks > 1 ? n_ranks : P.KL;
  P.meta_per = 3 + (size_t)(wdsize * (wdsize - 1) / 2) * 20;
  std::vector<size_t> lane_pts(P.NR, 0);
  for (int w = 0; w < P.n_win; w++) {
    HbaWindow &x = P.win[w];
    x.lane = w % P.NR; x.slot = w / P.NR;
    if (P.mode == HBA_SEQUENTIAL) continue;         // no chunks and no records: the clouds go straight to the submap area
    x.roff = lane_pts[x.lane];
    lane_pts[x.lane] += x.pts;
  }
  if (P.mode != HBA_SEQUENTIAL) {
    for (size_t n : lane_pts) if (n > P.chunk_pts) P.chunk_pts = n;
    P.win_per_lane = (size_t)(P.n_win + P.NR - 1) / P.NR;
  }
  P.meta_chunk = P.meta_per * P.win_per_lane;
  P.off_sub = P.n_all * 3;
  P.off_rep = P.off_sub + P.n_sub_cap * 3;
  P.off_meta = P.off_rep + (size_t)P.NR * P.chunk_pts * 3;
  P.meta_len = (size_t)P.NR * P.meta_chunk;
  P.need = P.off_meta + P.meta_len + 64;
  return P;
}

// Appends `ne` edge rows of 20 doubles to dst (room for `cap` rows, *n written so far); the two index columns go through `remap`.
// At the cap the rows that fitted stay written, *n == cap and the status is HBA_PLAN_ERR_CAPACITY.
template <class Remap>
inline int hba_append_edges(double *dst, int cap, int *n, const double *rows, int ne, Remap remap) {
  for (int e = 0; e < ne; e++) {
    if (*n >= cap) return HBA_PLAN_ERR_CAPACITY;
    double *o = dst + (size_t)(*n) * 20;
    std::memcpy(o, rows + (size_t)e * 20, 20 * sizeof(double));
    o[0] = remap(o[0]); o[1] = remap(o[1]);
    (*n)++;
  }
  return HBA_PLAN_OK;
}

// ---------------------------------------------------------------- the worker lanes
// stop_after: the lowest window that failed so far (n_win: none; -1: everybody stops).  Windows above it are skipped, windows up to
// it all run, so the lowest failing window in window order is found as without the early stop.
inline void hba_stop_at(std::atomic<int> &stop_after, int w) {
  int cur = stop_after.load();
  while (w < cur && !stop_after.compare_exchange_weak(cur, w)) {}
}
// A lane's gate in front of window w: true once `need` keyframes are up, false when the window is not to run any more.
inline bool hba_gate(const std::atomic<int> &kf_ready, int need, const std::atomic<int> &stop_after, int w) {
  while (w <= stop_after.load() && kf_ready.load(std::memory_order_acquire) < need) std::this_thread::sleep_for(std::chrono::microseconds(20));
  return w <= stop_after.load();
}

// The uploader goes on to keyframe k0 while no window has failed, or while the lowest failing window still lacks keyframes.
inline bool hba_upload_wanted(const HbaPlan &P, int stop_after, int k0) {
  return stop_after >= P.n_win || (stop_after >= 0 && k0 < P.win[stop_after].start + P.wdsize);
}

// Runs work(lane) on KL threads and main_job() (-> status) on the calling thread, joins every thread it started and returns the
// first failure: main_job's status, HBA_PLAN_ERR_CAPACITY for a std::bad_alloc and HBA_PLAN_ERR_RUNTIME for any other exception
// that left work or main_job or that starting a thread threw.  Every failure sets stop_after to -1; main_job does not run when a
// thread could not be started.  No exception leaves the runner.
template <class Work, class MainJob>
inline int hba_run_lanes(int KL, std::atomic<int> &stop_after, Work work, MainJob main_job) {
  std::atomic<int> status{HBA_PLAN_OK};
  auto fail = [&](int st) { int ok = HBA_PLAN_OK; status.compare_exchange_strong(ok, st); stop_after.store(-1); };
  auto guarded = [&](auto &&job) {
    try { const int st = job(); if (st != HBA_PLAN_OK) fail(st); }
    catch (const std::bad_alloc &) { fail(HBA_PLAN_ERR_CAPACITY); }
    catch (...) { fail(HBA_PLAN_ERR_RUNTIME); }
  };
  std::vector<std::thread> th;
  guarded([&] {
    th.reserve(KL);
    for (int lane = 0; lane < KL; lane++) th.emplace_back([&, lane] { guarded([&] { work(lane); return (int)HBA_PLAN_OK; }); });
    return (int)HBA_PLAN_OK;
  });
  if ((int)th.size() == KL) guarded(main_job);
  for (std::thread &t : th) t.join();
  return status.load();
}

}  // namespace vba
