// Scan log of libvoxelba.so (vba_scanlog_*): the marginalised scans of a session between the map's ring and the
// keyframes, resident in HBM.  Host drivers of the kernels in vba_kernels_scanlog.hpp over the bookkeeping of vba_scanlog_ring.hpp.
// Its readers in other units: vba_kf_build_from_log and vba_scanlog_export_world (vba_kf.hip), vba_scanlog_loop_update (vba_loop.hip).
#include "vba_ctx.hpp"
#include "vba_scanlog.hpp"
#include "vba_kernels_scanlog.hpp"

#include <hip/hip_runtime.h>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include <algorithm>

using namespace vba;

namespace {

const int64_t kLogMaxPoints = (int64_t)1 << 30;   // arena rows are addressed with 32-bit starts by the readers' tables
const int64_t kLogFirstCap = 65536;
const int kLogMaxBlocks = 2048;                   // grid cap of the streaming kernels: 256 CUs x 8 workgroups

unsigned log_grid(long long elems) { return (unsigned)std::max<long long>(1, std::min<long long>((elems + 255) / 256, kLogMaxBlocks)); }

// The arena becomes `newcap` points: new blocks, the live scans copied device to device in order and packed from 0, the old blocks
// freed after a synchronise.  Called with the log's mutex held; the caller excludes every reader (include/voxelba.h).
int log_grow(vba_scanlog *l, int64_t newcap) {
  vba_ctx *c = l->ctx;
  if (newcap > kLogMaxPoints) { c->set_error("vba_scanlog: the arena would exceed 2^30 points"); return VBA_ERR_CAPACITY; }
  DevMem<double> np, nv;
  HIPCHK(c, np.ensure((size_t)newcap * 3));
  HIPCHK(c, nv.ensure((size_t)newcap * 9));
  if (l->read_pending) { HIPCHK(c, hipStreamWaitEvent(c->stream, l->read_ev, 0)); l->read_pending = false; }
  l->moves.clear();
  l->ring.rebase(newcap, &l->moves);
  for (const ScanRing::Move &m : l->moves) {
    HIPCHK(c, hipMemcpyAsync(np + 3 * m.to, l->d_pnt + 3 * m.from, (size_t)m.n * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(nv + 9 * m.to, l->d_var + 9 * m.from, (size_t)m.n * 9 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  l->d_pnt = std::move(np); l->d_var = std::move(nv);
  l->allocs++; l->bytes += newcap * 12 * (int64_t)sizeof(double);
  return VBA_OK;
}

// Room for a scan of n points: *start = its first arena row.  Grows the scan table and the arena when the bookkeeping says the
// push does not fit; orders the log's stream behind a reader that left work queued elsewhere.  Mutex held.
int log_place(vba_scanlog *l, int64_t n, int64_t *start) {
  vba_ctx *c = l->ctx;
  ScanRing &r = l->ring;
  if (r.table_full()) r.reserve_scans(r.scan_cap() ? 2 * r.scan_cap() : 64);
  if (r.place(n) < 0) {
    const int st = log_grow(l, r.grown_cap(n, kLogFirstCap));
    if (st) return st;
  }
  if (l->read_pending) { HIPCHK(c, hipStreamWaitEvent(c->stream, l->read_ev, 0)); l->read_pending = false; }
  *start = r.place(n);
  return VBA_OK;
}

}  // namespace

namespace vba {

int scanlog_view(vba_scanlog *l, int64_t first, int k, long long max_points, hipStream_t stream, ScanLogView *out) {
  vba_ctx *c = l->ctx;
  std::lock_guard<std::mutex> lk(l->mu);
  if (k < 0 || !l->ring.live_range(first, k)) return VBA_ERR_BAD_ARG;
  out->starts.resize((size_t)k); out->rel.resize((size_t)k + 1);
  long long total = 0;
  for (int i = 0; i < k; i++) {
    out->starts[i] = (int)l->ring.start(first + i);
    out->rel[i] = (int)total;
    total += l->ring.size(first + i);
    if (total > max_points) return VBA_ERR_BAD_ARG;
  }
  out->rel[k] = (int)total;
  out->d_pnt = l->d_pnt; out->d_var = l->d_var;
  if (stream && stream != c->stream && total > 0) HIPCHK(c, hipStreamWaitEvent(stream, l->push_ev, 0));
  return VBA_OK;
}

int scanlog_reader_queued(vba_scanlog *l, hipStream_t stream) {
  vba_ctx *c = l->ctx;
  if (stream == c->stream) return VBA_OK;          // the next push is behind it on the same stream
  std::lock_guard<std::mutex> lk(l->mu);
  HIPCHK(c, hipEventRecord(l->read_ev, stream));
  l->read_pending = true;
  return VBA_OK;
}

}  // namespace vba

extern "C" {

int vba_scanlog_create(vba_ctx *c, vba_scanlog **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  vba_scanlog *l = new vba_scanlog();
  l->ctx = c;
  if (hipEventCreateWithFlags(&l->push_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&l->read_ev, hipEventDisableTiming) != hipSuccess) {
    vba_scanlog_destroy(l);
    return VBA_ERR_HIP;
  }
  *out = l;
  return VBA_OK;
}

void vba_scanlog_destroy(vba_scanlog *l) {
  if (!l) return;
  hipSetDevice(l->ctx->device);
  hipStreamSynchronize(l->ctx->stream);
  if (l->read_pending) hipEventSynchronize(l->read_ev);
  if (l->push_ev) hipEventDestroy(l->push_ev);
  if (l->read_ev) hipEventDestroy(l->read_ev);
  delete l;
}

int vba_scanlog_reserve(vba_scanlog *l, int64_t points, int scans) {
  if (!l || points < 0 || scans < 0 || points > kLogMaxPoints || scans > (1 << 24)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(l->mu);
  l->ring.reserve_scans((size_t)scans);
  if (points > l->ring.cap()) {
    const int st = log_grow(l, points);
    if (st) return st;
  }
  if ((size_t)points * 3 > l->d_xyz.n) {            // the float form of the largest scan the arena can hold
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, l->d_xyz.ensure((size_t)points * 3));
    l->allocs++; l->bytes += points * 3 * (int64_t)sizeof(float);
  }
  return VBA_OK;
}

int vba_scanlog_allocations(vba_scanlog *l, int *count, int64_t *bytes) {
  if (!l || !count || !bytes) return VBA_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(l->mu);
  *count = l->allocs; *bytes = l->bytes;
  return VBA_OK;
}

int vba_scanlog_push_window(vba_scanlog *l, int frame, int64_t *seq) {
  if (!l || !seq) return VBA_ERR_BAD_ARG;
  vba_ctx *c = l->ctx;
  if (c->n_ranks > 1 || c->map.n_ranks > 1 || c->rank != 0) {
    c->set_error("vba_scanlog_push_window: a sharded map's ring holds only the rank's share of a scan");
    return VBA_ERR_UNSUPPORTED;
  }
  if (frame < 0 || frame >= c->opt.win_size) { c->set_error("vba_scanlog_push_window: frame outside 0..win_size-1"); return VBA_ERR_BAD_ARG; }
  MapStore &m = c->map;
  const int slot = m.mp[frame];
  const int64_t n = m.allocated ? m.npts[slot] : 0;                  // known on the host: nothing is read back
  HIPCHK(c, hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(l->mu);
  int64_t start = 0;
  const int st = log_place(l, n, &start);
  if (st) return st;
  if (n > 0) {
    const double *sp = m.v.px + (size_t)slot * m.v.max_pts * 3;
    const double *sv = m.have_var ? m.v.pvar + (size_t)slot * m.v.max_pts * 9 : nullptr;
    hipLaunchKernelGGL(k_scanlog_copy, dim3(log_grid(12 * n)), dim3(256), 0, c->stream, (long long)n, sp, sv, l->d_pnt + 3 * start, l->d_var + 9 * start);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(l->push_ev, c->stream));
  }
  *seq = l->ring.push(n);
  return VBA_OK;
}

int vba_scanlog_push_points(vba_scanlog *l, int n, const double *pnt, const double *var, int64_t *seq) {
  if (!l || !seq || n < 0 || (n > 0 && !pnt)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = l->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(l->mu);
  int64_t start = 0;
  const int st = log_place(l, n, &start);
  if (st) return st;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(l->d_pnt + 3 * start, pnt, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
    if (var) HIPCHK(c, hipMemcpyAsync(l->d_var + 9 * start, var, (size_t)n * 9 * sizeof(double), hipMemcpyDefault, c->stream));
    else HIPCHK(c, hipMemsetAsync(l->d_var + 9 * start, 0, (size_t)n * 9 * sizeof(double), c->stream));
    HIPCHK(c, hipEventRecord(l->push_ev, c->stream));
    if (!is_device_ptr(pnt) || (var && !is_device_ptr(var))) HIPCHK(c, hipStreamSynchronize(c->stream));   // the host arrays are the caller's again
  }
  *seq = l->ring.push(n);
  return VBA_OK;
}

int vba_scanlog_range(vba_scanlog *l, int64_t *first, int64_t *end, int cap, int *sizes) {
  if (!l || !first || !end || cap < 0 || (cap > 0 && !sizes)) return VBA_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(l->mu);
  *first = l->ring.first(); *end = l->ring.end();
  for (int64_t s = *first; s < *end && s - *first < cap; s++) sizes[s - *first] = (int)l->ring.size(s);
  return VBA_OK;
}

int vba_scanlog_release(vba_scanlog *l, int64_t upto) {
  if (!l) return VBA_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(l->mu);
  l->ring.release(upto);
  return VBA_OK;
}

int vba_scanlog_read(vba_scanlog *l, int64_t seq, int cap, double *pnt, double *var, float *xyz, int *n) {
  if (!l || !n || cap < 0) return VBA_ERR_BAD_ARG;
  vba_ctx *c = l->ctx;
  int64_t start, size;
  {
    std::lock_guard<std::mutex> lk(l->mu);
    if (!l->ring.live(seq)) return VBA_ERR_BAD_ARG;
    start = l->ring.start(seq); size = l->ring.size(seq);
  }
  *n = (int)size;
  const size_t w = (size_t)std::min<int64_t>(size, cap);
  if (w == 0 || (!pnt && !var && !xyz)) return VBA_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (xyz && 3 * w > l->d_xyz.n) {
    size_t m = l->d_xyz.n ? l->d_xyz.n : 3 * (size_t)kLogFirstCap;
    while (m < 3 * w) m *= 2;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, l->d_xyz.ensure(m));
    std::lock_guard<std::mutex> lk(l->mu);
    l->allocs++; l->bytes += (int64_t)(m * sizeof(float));
  }
  if (pnt) HIPCHK(c, hipMemcpyAsync(pnt, l->d_pnt + 3 * start, w * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (var) HIPCHK(c, hipMemcpyAsync(var, l->d_var + 9 * start, w * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (xyz) {
    hipLaunchKernelGGL(k_scanlog_narrow, dim3(log_grid(3 * (long long)w)), dim3(256), 0, c->stream, 3 * (long long)w, l->d_pnt + 3 * start, l->d_xyz.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(xyz, l->d_xyz, w * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

}  // extern "C"
