// Scan front end of libvoxelba.so (vba_scan_decode, vba_scan_prepare, vba_scan_frame_*, vba_scan_layout_*): a frame that
// owns the device buffers of one scan from the raw message bytes to the body-frame points and covariances that the odometry and the
// map consume in place.  The decode kernels are in vba_kernels_decode.hpp; undistortion, down-sampling and var_init are the kernels of
// vba_kernels_scan.hpp (compiled in vba_kf.hip), run unchanged on the frame's buffers.
#include "vba_ctx.hpp"
#include "vba_odom_state.hpp"
#include "vba_kf_store_decl.hpp"
#include "vba_scan_frame.hpp"
#include "vba_kernels_decode.hpp"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>

using namespace vba;

struct vba_scan_frame {
  vba_ctx *ctx = nullptr;
  // raw message bytes (16-byte aligned, padded to a multiple of 16)
  DevMem<unsigned char> d_raw;
  // everything sized by the number of raw points: one block, carved by frame_carve
  DevMem<char> d_pts; int pcap = 0;
  float *d_rec = nullptr; unsigned int *d_key = nullptr, *d_kin = nullptr, *d_kout = nullptr; int *d_vin = nullptr, *d_vout = nullptr, *d_blk = nullptr, *d_res = nullptr;
  double *d_pnt0 = nullptr, *d_curv = nullptr; float *d_int = nullptr;                     // stage 0: decoded, sorted, cut
  double *d_pnt1 = nullptr;                                                               // stage 1: undistorted
  double *d_dsp = nullptr; int *d_dscnt = nullptr, *d_dsfirst = nullptr;                  // stage 2: down-sampled
  double *d_pb = nullptr, *d_vb = nullptr;                                                // stage 3: var_init
  DevMem<char> d_sort;                                                                    // rocPRIM scratch of the time sort
  DevMem<char> d_ws;                                                                      // the down-sampler's work area
  DevMem<double> d_prm; PinMem<double> h_prm; int prm_cap = 0;                            // undistortion parameters: pinned image, device copy
  PinMem<int> h_res;                                                                      // pinned: {n, bits of the last curvature, kept, -, voxels}
  int allocs = 0; int64_t bytes = 0;
  bool decoded = false, prepared = false;
  int n = 0, n_ds = 0;
  int scratch_for = 0;                                                                    // the point capacity that d_sort and d_ws were sized for
  hipStream_t last = nullptr;                                                             // the stream of the last call that queued work on the buffers
  hipEvent_t ev0 = nullptr;                                                               // recorded behind the decode: readers of stage 0 on other streams wait for it
};

namespace {

const size_t kAlign = 256;
size_t up(size_t b) { return (b + kAlign - 1) & ~(kAlign - 1); }

// carves the point block for p raw points (base == nullptr: only its size)
size_t frame_carve(vba_scan_frame *f, char *base, int p) {
  const size_t pp = (size_t)p + 2, nb = ((size_t)p + 255) / 256 + 2;      // + 2: the two points of an empty message
  size_t o = 0;
  auto take = [&](size_t b) { char *q = base ? base + o : nullptr; o += up(b); return q; };
  char *rec = take(pp * 5 * sizeof(float)), *key = take(pp * 4), *kin = take(pp * 4), *kout = take(pp * 4), *vin = take(pp * 4), *vout = take(pp * 4),
       *blk = take(nb * 4), *res = take(64), *p0 = take(pp * 24), *cv = take(pp * 8), *in = take(pp * 4), *p1 = take(pp * 24), *dsp = take(pp * 24),
       *dc = take(pp * 4), *df = take(pp * 4), *pb = take(pp * 24), *vb = take(pp * 72);
  if (base) {
    f->d_rec = (float *)rec; f->d_key = (unsigned int *)key; f->d_kin = (unsigned int *)kin; f->d_kout = (unsigned int *)kout; f->d_vin = (int *)vin;
    f->d_vout = (int *)vout; f->d_blk = (int *)blk; f->d_res = (int *)res; f->d_pnt0 = (double *)p0; f->d_curv = (double *)cv; f->d_int = (float *)in;
    f->d_pnt1 = (double *)p1; f->d_dsp = (double *)dsp; f->d_dscnt = (int *)dc; f->d_dsfirst = (int *)df; f->d_pb = (double *)pb; f->d_vb = (double *)vb;
  }
  return o;
}

int frame_drain(vba_scan_frame *f) {
  vba_ctx *c = f->ctx;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (f->last && f->last != c->stream) HIPCHK(c, hipDeviceSynchronize());   // the stream of another context, which may be gone by now
  return VBA_OK;
}

// grow-only, by doubling from `first` bytes (first == 0: exactly `need`, the caller doubles), after a synchronise; the contents do not
// survive (a decode rewrites all of them)
template <class Byte>
int frame_grow(vba_scan_frame *f, DevMem<Byte> &p, size_t need, size_t first) {
  if (need <= p.n) return VBA_OK;
  vba_ctx *c = f->ctx;
  size_t m = first ? (p.n ? p.n : first) : need;
  while (m < need) m *= 2;
  int st = frame_drain(f);
  if (st) return st;
  HIPCHK(c, p.ensure(m));
  f->allocs++; f->bytes += (int64_t)m;
  f->decoded = f->prepared = false;
  return VBA_OK;
}

int frame_ensure_points(vba_scan_frame *f, int need) {
  vba_ctx *c = f->ctx;
  if (need > f->pcap) {
    int m = f->pcap ? f->pcap : 65536;
    while (m < need) m *= 2;
    int st = frame_grow(f, f->d_pts, frame_carve(f, nullptr, m), 0);
    if (st) { f->pcap = 0; return st; }
    frame_carve(f, f->d_pts, m);
    f->pcap = m;
  }
  if (f->scratch_for == f->pcap) return VBA_OK;
  // scratch of the sort over pcap pairs and of the down-sampler over pcap + 2 points (deterministic mode is the larger layout)
  size_t tmp = 0;
  HIPCHK(c, sort_pairs_u32(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, (size_t)f->pcap, 32u, c->stream));
  int st = frame_grow(f, f->d_sort, up(tmp), 1 << 16);
  if (st) return st;
  const size_t ws = kf_ws_layout(c, f->pcap + 2, true, nullptr, nullptr, &st);
  if (st) return st;
  if ((st = frame_grow(f, f->d_ws, ws, 1 << 16))) return st;
  f->scratch_for = f->pcap;
  return VBA_OK;
}

int frame_ensure_prm(vba_scan_frame *f, int m) {
  if (m <= f->prm_cap) return VBA_OK;
  vba_ctx *c = f->ctx;
  int k = f->prm_cap ? f->prm_cap : 64;
  while (k < m) k *= 2;
  int st = frame_drain(f);
  if (st) return st;
  f->prm_cap = 0;
  const size_t b = ((size_t)22 * k + 24) * sizeof(double);
  HIPCHK(c, f->d_prm.ensure((size_t)22 * k + 24));
  HIPCHK(c, f->h_prm.ensure((size_t)22 * k + 24));
  f->prm_cap = k; f->allocs += 2; f->bytes += (int64_t)b;
  return VBA_OK;
}

bool field_ok(int off, int size, int step) { return off >= 0 && off <= step - size; }

}  // namespace

namespace vba {
// the initialisation window (vba_init.hip) reads stage 0 in place on its own context's stream
bool scan_frame_stage0(vba_scan_frame *f, hipStream_t stream, ScanStage0 *out) {
  if (!f || !f->decoded) return false;
  out->ctx = f->ctx; out->n = f->n; out->pnt = f->d_pnt0; out->curv = f->d_curv;
  if (stream && stream != f->ctx->stream && hipStreamWaitEvent(stream, f->ev0, 0) != hipSuccess) return false;
  return true;
}
}  // namespace vba

extern "C" {

int vba_scan_layout_livox(vba_scan_layout *l) {
  if (!l) return VBA_ERR_BAD_ARG;
  l->point_step = 20; l->off_time = 0; l->time_type = VBA_SCAN_TIME_U32_DIV1E9; l->off_x = 4; l->off_y = 8; l->off_z = 12;
  l->off_intensity = 16; l->intensity_type = VBA_SCAN_INTENSITY_U8; l->filter = 1;
  return VBA_OK;
}

int vba_scan_layout_check(const vba_scan_layout *l) {
  if (!l || l->point_step < 1) return VBA_ERR_BAD_ARG;
  const int s = l->point_step;
  if (!field_ok(l->off_x, 4, s) || !field_ok(l->off_y, 4, s) || !field_ok(l->off_z, 4, s)) return VBA_ERR_BAD_ARG;
  switch (l->intensity_type) {
    case VBA_SCAN_INTENSITY_NONE: break;
    case VBA_SCAN_INTENSITY_F32: if (!field_ok(l->off_intensity, 4, s)) return VBA_ERR_BAD_ARG; break;
    case VBA_SCAN_INTENSITY_U8: if (!field_ok(l->off_intensity, 1, s)) return VBA_ERR_BAD_ARG; break;
    default: return VBA_ERR_BAD_ARG;
  }
  switch (l->time_type) {
    case VBA_SCAN_TIME_NONE: break;
    case VBA_SCAN_TIME_F32: case VBA_SCAN_TIME_U32_DIV1E9: if (!field_ok(l->off_time, 4, s)) return VBA_ERR_BAD_ARG; break;
    case VBA_SCAN_TIME_F64_REL_FIRST: if (!field_ok(l->off_time, 8, s)) return VBA_ERR_BAD_ARG; break;
    default: return VBA_ERR_BAD_ARG;
  }
  if (l->filter != 0 && l->filter != 1) return VBA_ERR_BAD_ARG;
  return VBA_OK;
}

int vba_scan_frame_create(vba_ctx *c, vba_scan_frame **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  vba_scan_frame *f = new vba_scan_frame();
  f->ctx = c;
  int st = frame_ensure_prm(f, 64);
  if (!st && f->h_res.ensure(16) != hipSuccess) st = VBA_ERR_HIP;
  if (!st && hipEventCreateWithFlags(&f->ev0, hipEventDisableTiming) != hipSuccess) st = VBA_ERR_HIP;
  if (st) { vba_scan_frame_destroy(f); return st; }
  f->allocs++;
  *out = f;
  return VBA_OK;
}

void vba_scan_frame_destroy(vba_scan_frame *f) {
  if (!f) return;
  hipSetDevice(f->ctx->device);
  hipStreamSynchronize(f->ctx->stream);
  if (f->last && f->last != f->ctx->stream) hipDeviceSynchronize();
  if (f->ev0) hipEventDestroy(f->ev0);
  delete f;
}

int vba_scan_frame_reserve(vba_scan_frame *f, int max_raw_points, int max_point_step) {
  if (!f || max_raw_points < 0 || max_point_step < 1 || max_raw_points > (1 << 28) || max_point_step > (1 << 16)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = f->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st = frame_grow(f, f->d_raw, ((size_t)max_raw_points * (size_t)max_point_step + 15) & ~(size_t)15, 1 << 20);
  if (st) return st;
  return frame_ensure_points(f, max_raw_points > 0 ? max_raw_points : 1);
}

int vba_scan_frame_allocations(vba_scan_frame *f, int *n_allocs, int64_t *bytes) {
  if (!f || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = f->allocs; *bytes = f->bytes;
  return VBA_OK;
}

int vba_scan_decode(vba_scan_frame *f, const vba_scan_layout *l, const void *raw, int n_raw, int point_filter_num, double blind2, int *n_out,
                    double *last_curvature) {
  if (!f || !l || !n_out || !last_curvature || n_raw < 0 || n_raw > (1 << 28) || (n_raw > 0 && !raw) || point_filter_num < 1) return VBA_ERR_BAD_ARG;
  if (vba_scan_layout_check(l) != VBA_OK) return VBA_ERR_BAD_ARG;
  *n_out = 0; *last_curvature = 0.0;
  if (l->time_type == VBA_SCAN_TIME_F32 && n_raw > 0) {           // FP:176: anything else selects the yaw-angle branch, which is not built
    float t;
    std::memcpy(&t, (const unsigned char *)raw + (size_t)(n_raw - 1) * (size_t)l->point_step + (size_t)l->off_time, 4);
    if (!((double)t > 0.01 && (double)t < 0.12)) return VBA_ERR_UNSUPPORTED;
  }
  vba_ctx *c = f->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  f->decoded = f->prepared = false;
  const size_t nbytes = (size_t)n_raw * (size_t)l->point_step, padded = (nbytes + 15) & ~(size_t)15;
  int st = frame_grow(f, f->d_raw, padded, 1 << 20);
  if (st || (st = frame_ensure_points(f, n_raw > 0 ? n_raw : 1))) return st;
  hipStream_t s = c->stream;
  f->last = s;
  ScanLayoutDev L{l->point_step, l->off_x, l->off_y, l->off_z, l->off_intensity, l->intensity_type, l->off_time, l->time_type, l->filter};
  const int nb = (n_raw + 255) / 256;
  const int n_sort = l->filter ? (n_raw + point_filter_num - 1) / point_filter_num : n_raw;
  int *d_total = f->d_res + 2;
  if (n_raw > 0) {
    HIPCHK(c, hipMemcpyAsync(f->d_raw, raw, nbytes, hipMemcpyHostToDevice, s));
    if (l->point_step <= SCAN_LDS_STEP)
      hipLaunchKernelGGL(k_scan_decode<true>, dim3(nb), dim3(256), 0, s, f->d_raw, padded, n_raw, L, point_filter_num, blind2, f->d_rec, f->d_key, f->d_blk);
    else
      hipLaunchKernelGGL(k_scan_decode<false>, dim3(nb), dim3(256), 0, s, f->d_raw, padded, n_raw, L, point_filter_num, blind2, f->d_rec, f->d_key, f->d_blk);
  }
  hipLaunchKernelGGL(k_ds_scan, dim3(1), dim3(256), 0, s, nb, f->d_blk, d_total);
  if (n_raw > 0) {
    hipLaunchKernelGGL(k_scan_pairs, dim3(nb), dim3(256), 0, s, n_raw, l->filter, point_filter_num, n_sort, f->d_key, f->d_blk, d_total, f->d_kin, f->d_vin);
    size_t tmp = f->d_sort.n;
    HIPCHK(c, sort_pairs_u32(f->d_sort, tmp, f->d_kin, f->d_kout, f->d_vin, f->d_vout, (size_t)n_sort, 32u, s));
  }
  float fcut = (float)0.11;                                        // the largest float that is <= 0.11 as a double
  if ((double)fcut > 0.11) fcut = std::nextafterf(fcut, 0.f);
  const int nf = n_sort > 2 ? n_sort : 2;
  hipLaunchKernelGGL(k_scan_finish, dim3((nf + 255) / 256), dim3(256), 0, s, f->d_kout, f->d_vout, f->d_rec, d_total, scan_time_key(fcut), f->d_pnt0, f->d_curv,
                     f->d_int, f->d_res);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(f->h_res, f->d_res, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipEventRecord(f->ev0, s));
  HIPCHK(c, hipStreamSynchronize(s));
  f->n = f->h_res[0];
  float lc;
  std::memcpy(&lc, &f->h_res[1], 4);
  *n_out = f->n; *last_curvature = f->n > 0 ? (double)lc : 0.0;
  f->decoded = true;
  return VBA_OK;
}

// vba_scan_prepare, and with `os` vba_scan_prepare_on_state: the table and end_pose are then the ones a propagation left in the state's
// parameter block, read in place; only the extrinsic goes up, behind them
static int scan_prepare_core(vba_ctx *c, vba_scan_frame *f, int m, const double *imu_poses, const double *end_pose, const double *ext_pose, int point_notime,
                             double down_size, int min_points, double dept_err, double beam_err, int *n_out, const double **d_pnt_body,
                             const double **d_var_body, vba_odom_state *os) {
  if (!c || !f || !n_out || !d_pnt_body || !d_var_body || m < 0 || !ext_pose || !(down_size == down_size)) return VBA_ERR_BAD_ARG;
  if (!os && !point_notime && (!end_pose || (m > 0 && !imu_poses))) return VBA_ERR_BAD_ARG;
  if (!f->decoded || c->device != f->ctx->device) return VBA_ERR_BAD_ARG;
  *n_out = 0; *d_pnt_body = f->d_pb; *d_var_body = f->d_vb;
  f->prepared = false; f->n_ds = 0;
  HIPCHK(c, hipSetDevice(c->device));
  const int n = f->n;
  if (n == 0) { f->prepared = true; return VBA_OK; }
  const int mu = point_notime ? 0 : m;
  int st = frame_ensure_prm(f, os ? 0 : mu);
  if (st) return st;
  hipStream_t s = c->stream;
  f->last = s;
  // the parameter block of k_undistort; its last 12 doubles, the extrinsic, are also var_init's
  double *prm = f->h_prm, *d_prm = f->d_prm;
  const size_t ext_at = (size_t)22 * (os ? os->n_poses : mu) + 12;         // (the state's table keeps its rows when the scan has no time stamps)
  if (os) {
    if ((st = odom_state_order(os, s, c->err))) return st;
    d_prm = os->d_tab;
    std::memcpy(prm, ext_pose, 12 * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(d_prm + ext_at, prm, 12 * sizeof(double), hipMemcpyHostToDevice, s));
  } else {
    if (mu > 0) std::memcpy(prm, imu_poses, (size_t)22 * mu * sizeof(double));
    if (end_pose) std::memcpy(prm + (size_t)22 * mu, end_pose, 12 * sizeof(double)); else std::memset(prm + (size_t)22 * mu, 0, 12 * sizeof(double));
    std::memcpy(prm + (size_t)22 * mu + 12, ext_pose, 12 * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(d_prm, prm, ((size_t)22 * mu + 24) * sizeof(double), hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, hipMemcpyAsync(f->d_pnt1, f->d_pnt0, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  const int nb = (n + 255) / 256;
  if (mu > 0) hipLaunchKernelGGL(k_undistort, dim3(nb), dim3(256), 0, s, n, f->d_pnt1, f->d_curv, mu, (const double *)d_prm);
  int nd = n;
  const bool det = c->opt.deterministic != 0;
  DsWork w{};
  if (kf_ws_layout(c, n, det, f->d_ws, &w, &st) > f->d_ws.n || st) return st ? st : VBA_ERR_CAPACITY;
  auto down_sample = [&](double vs) -> int {
    if (vs < 0.001) {                                              // TL:203: the cloud as it is, counts 0
      HIPCHK(c, hipMemcpyAsync(f->d_dsp, f->d_pnt1, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
      HIPCHK(c, hipMemsetAsync(f->d_dscnt, 0, (size_t)n * sizeof(int), s));
      hipLaunchKernelGGL(k_iota, dim3(nb), dim3(256), 0, s, f->d_dsfirst, n);
      HIPCHK(c, hipStreamSynchronize(s));                          // the pinned parameter image is free again
      nd = n;
      return VBA_OK;
    }
    int e = ds_core(c, s, 0, n, f->d_pnt1, nullptr, 9, 4, vs, det, w);
    if (e) return e;
    hipLaunchKernelGGL(k_ds_emit, dim3(nb), dim3(256), 0, s, n, w.tab, w.slot, w.blk, f->d_dsp, f->d_dscnt, f->d_dsfirst, (double *)nullptr, 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(f->h_res + 4, w.n_out, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    nd = f->h_res[4];
    return VBA_OK;
  };
  if ((st = down_sample(down_size))) return st;
  if (min_points > 0 && nd < min_points && (st = down_sample(down_size / 2))) return st;   // VS:1880-1884: from the undistorted cloud, kept whatever its count
  if (nd < 1 || nd > n) { c->set_error("scan prepare: voxel count out of range"); return VBA_ERR_HIP; }
  hipLaunchKernelGGL(k_var_init, dim3((nd + 255) / 256), dim3(256), 0, s, nd, f->d_dsp, f->d_pb, f->d_vb, (const double *)d_prm + ext_at,
                     (float)dept_err, (float)beam_err);
  HIPCHK(c, hipGetLastError());
  f->n_ds = nd; f->prepared = true;
  *n_out = nd;
  return VBA_OK;
}

int vba_scan_prepare(vba_ctx *c, vba_scan_frame *f, int m, const double *imu_poses, const double *end_pose, const double *ext_pose, int point_notime,
                     double down_size, int min_points, double dept_err, double beam_err, int *n_out, const double **d_pnt_body, const double **d_var_body) {
  return scan_prepare_core(c, f, m, imu_poses, end_pose, ext_pose, point_notime, down_size, min_points, dept_err, beam_err, n_out, d_pnt_body, d_var_body,
                           nullptr);
}

int vba_scan_prepare_on_state(vba_ctx *c, vba_scan_frame *f, vba_odom_state *os, const double *ext_pose, int point_notime, double down_size,
                              int min_points, double dept_err, double beam_err, int *n_out, const double **d_pnt_body, const double **d_var_body) {
  if (!c || !os || c->device != os->ctx->device || os->n_poses < 1) return VBA_ERR_BAD_ARG;
  return scan_prepare_core(c, f, os->n_poses, nullptr, nullptr, ext_pose, point_notime, down_size, min_points, dept_err, beam_err, n_out, d_pnt_body,
                           d_var_body, os);
}

int vba_scan_frame_read(vba_scan_frame *f, int stage, double *pnt, float *intensity, double *curvature, int *count, int *first, double *var) {
  if (!f || stage < 0 || stage > 3 || !f->decoded || (stage > 0 && !f->prepared)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = f->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = f->last ? f->last : c->stream;
  const size_t n = (size_t)(stage < 2 ? f->n : f->n_ds);
  if (n > 0) {
    const double *src = stage == 0 ? f->d_pnt0 : stage == 1 ? f->d_pnt1 : stage == 2 ? f->d_dsp : f->d_pb;
    if (pnt) HIPCHK(c, hipMemcpyAsync(pnt, src, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (stage < 2 && intensity) HIPCHK(c, hipMemcpyAsync(intensity, f->d_int, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (stage < 2 && curvature) HIPCHK(c, hipMemcpyAsync(curvature, f->d_curv, n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (stage == 2 && count) HIPCHK(c, hipMemcpyAsync(count, f->d_dscnt, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (stage == 2 && first) HIPCHK(c, hipMemcpyAsync(first, f->d_dsfirst, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (stage == 3 && var) HIPCHK(c, hipMemcpyAsync(var, f->d_vb, n * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  return VBA_OK;
}

}  // extern "C"
