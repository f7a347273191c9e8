// Private header of the units that read a scan log ("Source layout": where state lives): the handle struct of
// vba_scanlog.hip and the view through which the keyframe and loop units take a range of scans.  It defines no kernel.
#pragma once
#include "vba_ctx.hpp"
#include "vba_scanlog_ring.hpp"

#include <mutex>

// scan log (vba_scanlog.hip); the keyframe store and the loop update read its arena in place
struct vba_scanlog {
  vba_ctx *ctx = nullptr;
  // one arena of ring.cap() points used as a ring of whole scans: body points and covariance rows as the map's ring held them
  DevMem<double> d_pnt, d_var;
  std::mutex mu;                   // the bookkeeping (ring, read_pending, counters); held across a wait only by a push or reserve that grows
  ScanRing ring;
  std::vector<ScanRing::Move> moves;          // host scratch of a growth
  DevMem<float> d_xyz;                        // the float form of one scan on its way out (vba_scanlog_read)
  // push_ev: behind the newest capture on the log's stream, for readers on other streams; read_ev: behind the newest reader that
  // returned with its work still queued on another stream, for the push that may write over what it reads
  hipEvent_t push_ev = nullptr, read_ev = nullptr;
  bool read_pending = false;
  int allocs = 0; int64_t bytes = 0;
};

namespace vba {
// Scans first .. first + k - 1 for a reader on `stream`, which is ordered behind their captures: starts[i] = the first arena row of
// scan i, rel[i] = the points before scan i among the k (rel[k] = their sum).  VBA_ERR_BAD_ARG when the range is not wholly live
// or its points exceed `max_points`; nothing is queued then.  stream == nullptr: the fields only, nothing is queued.
struct ScanLogView { const double *d_pnt, *d_var; std::vector<int> starts, rel; };
int scanlog_view(vba_scanlog *l, int64_t first, int k, long long max_points, hipStream_t stream, ScanLogView *out);
// a reader that returns with work on the arena still queued on `stream` leaves its mark for the next push
int scanlog_reader_queued(vba_scanlog *l, hipStream_t stream);
}  // namespace vba
