// libvoxelba.so, the surfel-map unit: vba_surfel_map_* and vba_surfel_register, kernels in vba_kernels_surfreg.hpp;
// also the point loop of the odometry update against a surfel map (§27), queued from vba_odom.hip through surfel_odom_queue.
// Compiled with -ffp-contract=off (csrc/Makefile): the order and rounding of every operation of the build and of an iteration is
// part of the interface, and a host build of vba_surfreg_math.hpp gives the device's bits for a cell and for a point.
#include "vba_ctx.hpp"
#include "vba_kernels_surfreg.hpp"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>

using namespace vba;

static_assert(sizeof(vba_surfel_reg_report) == sizeof(SregReport), "vba_surfel_reg_report mirrors SregReport");
static_assert(VBA_SURFEL_REG_MAX_ITER == SREG_MAX_ITER, "the report's slots");

struct vba_surfel_map {
  vba_ctx *ctx = nullptr;
  // the table and the cells; rec / cov: the records of a host build on their way in, and the export's output of build_from_kf
  DevMem<SregSlot> tab; DevMem<SregCell> cell; DevMem<float> rec; DevMem<double> cov;
  size_t cap_rec = 0, cap_stage = 0;             // records that cell (tab: a power of two >= 2 cap_rec slots) / rec and cov hold
  DevMem<double> pnt, part; size_t cap_pnt = 0;  // a host scan on its way in, the partials of its workgroups
  DevMem<SregState> d_state; PinMem<SregState> h_state;
  DevMem<SregBuildStatus> d_status; PinMem<SregBuildStatus> h_status;
  // the map as built
  int64_t n_rec = 0, n_cells = 0; unsigned int mask = 0; double voxel = 0, sigma = 0;
  int allocs = 0; int64_t bytes = 0;
};

namespace {

size_t sreg_slots(size_t n) { size_t s = 2; while (s < 2 * n) s *= 2; return s; }
int sreg_blocks(int64_t n) { const int64_t nb = (n + 255) / 256; return (int)(nb < SREG_MAX_BLOCKS ? nb : SREG_MAX_BLOCKS); }

// -1: not device memory; otherwise the device that holds it
int sreg_device_of(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

template <class M>
int sreg_grow(vba_surfel_map *m, M &buf, size_t want) {
  if (want <= buf.n) return VBA_OK;
  vba_ctx *c = m->ctx;
  HIPCHK(c, buf.ensure(want));
  m->allocs++; m->bytes += (int64_t)(want * sizeof(*buf.p));
  return VBA_OK;
}

// room for n records: as it is when it suffices, else exactly n (a reservation) or doubled until it does, after a synchronise
// `stage`: with the record and covariance arrays (a host build, build_from_kf, a reservation), which a build from device arrays
// does not need
int sreg_ensure_rec(vba_surfel_map *m, size_t n, bool exact, bool stage) {
  vba_ctx *c = m->ctx;
  int st;
  if ((st = sreg_grow(m, m->d_status, 1)) || (st = sreg_grow(m, m->h_status, 1))) return st;
  if (n > m->cap_rec) {
    size_t want = (exact || !m->cap_rec) ? n : m->cap_rec;
    while (want < n) want *= 2;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m->cap_rec = 0; m->n_cells = 0; m->n_rec = 0;            // (the map as built goes with its blocks)
    if ((st = sreg_grow(m, m->tab, sreg_slots(want))) || (st = sreg_grow(m, m->cell, want))) return st;
    m->cap_rec = want;
  }
  if (stage && n > m->cap_stage) {
    size_t want = (exact || !m->cap_stage) ? n : m->cap_stage;
    while (want < n) want *= 2;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m->cap_stage = 0;
    if ((st = sreg_grow(m, m->rec, 12 * want)) || (st = sreg_grow(m, m->cov, 6 * want))) return st;
    m->cap_stage = want;
  }
  return VBA_OK;
}

int sreg_ensure_pnt(vba_surfel_map *m, size_t n, bool exact) {
  vba_ctx *c = m->ctx;
  int st;
  if ((st = sreg_grow(m, m->d_state, 1)) || (st = sreg_grow(m, m->h_state, 1)) || (st = sreg_grow(m, m->part, (size_t)SREG_MAX_BLOCKS * SREG_PART)))
    return st;
  if (n <= m->cap_pnt) return VBA_OK;
  size_t want = (exact || !m->cap_pnt) ? n : m->cap_pnt;
  while (want < n) want *= 2;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  m->cap_pnt = 0;
  if ((st = sreg_grow(m, m->pnt, 3 * want))) return st;
  m->cap_pnt = want;
  return VBA_OK;
}

// the table over n device records (the map's own arrays or the caller's): clear, insert, one wait for the status words
int sreg_build_device(vba_surfel_map *m, int64_t n, const float *rec, const double *cov, double voxel, double sigma, int min_count, int64_t *n_cells) {
  vba_ctx *c = m->ctx;
  m->n_cells = 0; m->n_rec = 0;
  if (n > 0) {
    const unsigned int slots = (unsigned int)sreg_slots((size_t)n);
    // the kernels below write slots table entries and n cells: never beyond what the map holds, whichever path sized it
    if ((size_t)n > m->cap_rec || (size_t)n > m->cell.n || slots > m->tab.n) { c->set_error("vba_surfel_map_build: table and cells hold fewer records than the build"); return VBA_ERR_CAPACITY; }
    hipLaunchKernelGGL(k_sreg_clear, dim3((slots + 255) / 256), dim3(256), 0, c->stream, m->tab.p, slots, m->d_status.p);
    hipLaunchKernelGGL(k_sreg_insert, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, c->stream, (int)n, rec, cov, voxel, sigma, min_count, m->tab.p,
                       slots - 1, m->cell.p, m->d_status.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(m->h_status.p, m->d_status.p, sizeof(SregBuildStatus), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m->h_status->dup) {
      c->set_error("vba_surfel_map_build: two records share a voxel key: they were not made at this voxel_size");
      return VBA_ERR_BAD_ARG;
    }
    m->n_cells = m->h_status->n_cells; m->n_rec = n; m->mask = slots - 1;
  }
  m->voxel = voxel; m->sigma = sigma;
  *n_cells = m->n_cells;
  return VBA_OK;
}

bool sreg_build_args_ok(vba_surfel_map *m, double voxel_size, double sigma, int min_count, const int64_t *n_cells) {
  return m && n_cells && voxel_size >= 0.001 && sigma >= 1e-4 && std::isfinite(voxel_size) && std::isfinite(sigma) && min_count >= 1;
}

int sreg_unsharded(vba_ctx *c, const char *who) {
  if (c->n_ranks > 1 || c->rank != 0) { c->set_error(std::string(who) + ": sharded contexts are not supported"); return VBA_ERR_UNSUPPORTED; }
  return VBA_OK;
}

struct SregTaps { int *cell = nullptr; unsigned char *gate = nullptr; double *sums = nullptr, *dx = nullptr; };   // device, null in the loop

// one iteration: the two launches, for the loop of vba_surfel_register and for vba_debug_surfel_reg_pass alike
void sreg_pass(vba_surfel_map *m, int64_t n, const double *d_pnt, const SregTaps &tp) {
  const int nb = sreg_blocks(n);
  SregTable T; T.tab = m->tab.p; T.cell = m->cell.p; T.mask = m->mask; T.voxel = m->voxel;
  k_sreg_accum<<<nb, 256, 0, m->ctx->stream>>>((int)n, d_pnt, T, m->d_state.p, m->part.p, tp.cell, tp.gate);
  k_sreg_step<<<1, 64, 0, m->ctx->stream>>>(nb, m->part.p, m->d_state.p, tp.sums, tp.dx);
}

bool sreg_reg_args_ok(vba_surfel_map *m, int64_t n, const double *pnt, const vba_surfel_reg_params *p, const double *R, const double *t) {
  if (!m || !pnt || !p || !R || !t || n < 1 || n > ((int64_t)1 << 30)) return false;
  if ((p->neighbors != 1 && p->neighbors != 7) || p->max_iter < 1 || p->max_iter > SREG_MAX_ITER || !(p->gate > 0.0) || !std::isfinite(p->gate)) return false;
  if (m->n_cells < 1) return false;
  const int dev = sreg_device_of(pnt);
  return dev < 0 || dev == m->ctx->device;
}

// the scan where the kernels read it: in place, or staged once
int sreg_stage_pnt(vba_surfel_map *m, int64_t n, const double *pnt, const double **d_pnt) {
  vba_ctx *c = m->ctx;
  int st;
  const bool host = sreg_device_of(pnt) < 0;
  if ((st = sreg_ensure_pnt(m, host ? (size_t)n : 0, false))) return st;
  *d_pnt = pnt;
  if (host) {
    HIPCHK(c, hipMemcpyAsync(m->pnt.p, pnt, (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
    *d_pnt = m->pnt.p;
  }
  return VBA_OK;
}

void sreg_fill_state(SregState *h, const vba_surfel_reg_params *p, const double *R, const double *t, int max_iter) {
  std::memset(h, 0, sizeof(*h));
  for (int k = 0; k < 9; k++) h->R[k] = R[k];
  for (int k = 0; k < 3; k++) h->t[k] = t[k];
  h->gate2 = p->gate * p->gate; h->eps_rot = p->eps_rot; h->eps_tra = p->eps_tra;
  h->neighbors = p->neighbors; h->max_iter = max_iter; h->min_matches = p->min_matches;
}

}  // namespace

// ---------------------------------------------------------------- for vba_odom.hip (declared in vba_ctx.hpp)
namespace vba {
bool surfel_odom_args_ok(const vba_surfel_map *m, const vba_ctx *c, int n, const double *pnt) {
  if (!m || m->ctx != c || m->n_cells < 1) return false;
  if (n == 0) return true;
  const int dev = sreg_device_of(pnt);
  return dev < 0 || dev == c->device;
}
int surfel_odom_stage(vba_surfel_map *m, int n, const double *pnt, const double **d_pnt) {
  *d_pnt = pnt;
  if (n == 0 || sreg_device_of(pnt) >= 0) return VBA_OK;
  return sreg_stage_pnt(m, n, pnt, d_pnt);
}
int surfel_odom_blocks(int n) { return sreg_blocks(n); }
int surfel_odom_queue(vba_surfel_map *m, hipStream_t st, const vbh::OdomEkf *d_S, int n, const double *d_pnt, double gate, int neighbors,
                      double *d_partial, double *d_cost, int *d_cell, unsigned char *d_gate) {
  const int nb = sreg_blocks(n);
  SregTable T; T.tab = m->tab.p; T.cell = m->cell.p; T.mask = m->mask; T.voxel = m->voxel;
  k_sodom_accum<<<nb, 256, 0, st>>>(n, d_pnt, T, d_S, gate * gate, neighbors, d_partial, d_cost, d_cell, d_gate);
  return nb;
}
}  // namespace vba

extern "C" {

int vba_surfel_map_create(vba_ctx *c, vba_surfel_map **out) {
  if (!c || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  int st;
  if ((st = sreg_unsharded(c, "vba_surfel_map_create"))) return st;
  HIPCHK(c, hipSetDevice(c->device));
  vba_surfel_map *m = new vba_surfel_map();
  m->ctx = c;
  *out = m;
  return VBA_OK;
}

int vba_surfel_map_destroy(vba_surfel_map *m) {
  if (!m) return VBA_ERR_BAD_ARG;
  hipSetDevice(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  delete m;
  return VBA_OK;
}

int vba_surfel_map_reserve(vba_surfel_map *m, int64_t max_cells, int64_t max_points) {
  if (!m || max_cells < 0 || max_points < 0) return VBA_ERR_BAD_ARG;
  if (max_cells > ((int64_t)1 << 30) || max_points > ((int64_t)1 << 30)) return VBA_ERR_CAPACITY;
  vba_ctx *c = m->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if ((st = sreg_ensure_rec(m, (size_t)max_cells, true, true))) return st;
  return sreg_ensure_pnt(m, (size_t)max_points, true);
}

int vba_surfel_map_allocations(vba_surfel_map *m, int *n_allocs, int64_t *bytes) {
  if (!m || !n_allocs || !bytes) return VBA_ERR_BAD_ARG;
  *n_allocs = m->allocs; *bytes = m->bytes;
  return VBA_OK;
}

int vba_surfel_map_build(vba_surfel_map *m, int64_t n, const float *surfels, const double *cov, double voxel_size, double sigma, int min_count,
                         int64_t *n_cells) {
  if (!sreg_build_args_ok(m, voxel_size, sigma, min_count, n_cells) || n < 0 || n > ((int64_t)1 << 30) || (n > 0 && (!surfels || !cov))) return VBA_ERR_BAD_ARG;
  vba_ctx *c = m->ctx;
  int st;
  if ((st = sreg_unsharded(c, "vba_surfel_map_build"))) return st;
  const int ds = n > 0 ? sreg_device_of(surfels) : -1, dc = n > 0 ? sreg_device_of(cov) : -1;
  if ((ds < 0) != (dc < 0)) { c->set_error("vba_surfel_map_build: surfels and cov must both be host or both be device memory"); return VBA_ERR_BAD_ARG; }
  if (ds >= 0 && (ds != c->device || dc != c->device)) { c->set_error("vba_surfel_map_build: the records are on another device"); return VBA_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = sreg_ensure_rec(m, (size_t)n, false, ds < 0))) return st;
  const float *d_rec = surfels; const double *d_cov = cov;
  if (n > 0 && ds < 0) {
    HIPCHK(c, hipMemcpyAsync(m->rec.p, surfels, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(m->cov.p, cov, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
    d_rec = m->rec.p; d_cov = m->cov.p;
  }
  return sreg_build_device(m, n, d_rec, d_cov, voxel_size, sigma, min_count, n_cells);
}

int vba_surfel_map_build_from_kf(vba_surfel_map *m, int n_stores, vba_kf_store *const *stores, int jump, double voxel_size, double sigma, int min_count,
                                 int64_t *n_cells) {
  if (!sreg_build_args_ok(m, voxel_size, sigma, min_count, n_cells) || n_stores < 1 || !stores || jump < 1) return VBA_ERR_BAD_ARG;
  vba_ctx *c = m->ctx;
  int st;
  if ((st = sreg_unsharded(c, "vba_surfel_map_build_from_kf"))) return st;
  HIPCHK(c, hipSetDevice(c->device));
  const std::vector<float> inten((size_t)n_stores, 0.0f);      // the records' intensity is not read
  int64_t need = 0;
  if (!m->cap_stage) {                                         // nothing reserved: ask for the size first
    if ((st = vba_kf_surfel_export(c, n_stores, stores, inten.data(), jump, voxel_size, min_count, 0, nullptr, nullptr, nullptr, &need))) return st;
    if ((st = sreg_ensure_rec(m, (size_t)(need > 0 ? need : 1), false, true))) return st;
  }
  st = vba_kf_surfel_export(c, n_stores, stores, inten.data(), jump, voxel_size, min_count, (int64_t)m->cap_stage, m->rec.p, m->cov.p, nullptr, &need);
  if (st == VBA_ERR_CAPACITY && need > (int64_t)m->cap_stage && need <= ((int64_t)1 << 30)) {
    if ((st = sreg_ensure_rec(m, (size_t)need, false, true))) return st;
    st = vba_kf_surfel_export(c, n_stores, stores, inten.data(), jump, voxel_size, min_count, (int64_t)m->cap_stage, m->rec.p, m->cov.p, nullptr, &need);
  }
  if (st) return st;
  // table and cells grow on their own (a build from device arrays needs no staging): the staging may hold more records than they do
  if ((st = sreg_ensure_rec(m, (size_t)need, false, false))) return st;
  return sreg_build_device(m, need, m->rec.p, m->cov.p, voxel_size, sigma, min_count, n_cells);
}

int vba_surfel_map_size(vba_surfel_map *m, int64_t *n_cells, double *voxel_size, double *sigma) {
  if (!m || !n_cells) return VBA_ERR_BAD_ARG;
  *n_cells = m->n_cells;
  if (voxel_size) *voxel_size = m->voxel;
  if (sigma) *sigma = m->sigma;
  return VBA_OK;
}

int vba_debug_surfel_map_read(vba_surfel_map *m, int64_t cap, int64_t *slot, unsigned long long *key, int *row, float *c4, double *W, int64_t *n_out,
                              int64_t *n_slots) {
  if (!m || !n_out || cap < 0) return VBA_ERR_BAD_ARG;
  vba_ctx *c = m->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_out = m->n_cells;
  if (n_slots) *n_slots = m->n_cells > 0 ? (int64_t)m->mask + 1 : 0;
  if (cap == 0 || m->n_cells == 0) return VBA_OK;
  if (cap < m->n_cells) return VBA_ERR_CAPACITY;
  std::vector<SregSlot> tab((size_t)m->mask + 1);
  std::vector<SregCell> cell((size_t)m->n_rec);
  HIPCHK(c, hipMemcpy(tab.data(), m->tab.p, tab.size() * sizeof(SregSlot), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(cell.data(), m->cell.p, cell.size() * sizeof(SregCell), hipMemcpyDeviceToHost));
  int64_t k = 0;
  for (size_t s = 0; s < tab.size() && k < cap; s++) {
    if (tab[s].key == DS_EMPTY) continue;
    const SregCell &e = cell[(size_t)tab[s].row];
    if (slot) slot[k] = (int64_t)s;
    if (key) key[k] = tab[s].key;
    if (row) row[k] = tab[s].row;
    if (c4) { c4[4 * k] = e.c[0]; c4[4 * k + 1] = e.c[1]; c4[4 * k + 2] = e.c[2]; c4[4 * k + 3] = e.cnt; }
    if (W) std::memcpy(W + 6 * k, e.W, 48);
    k++;
  }
  return VBA_OK;
}

void vba_surfel_reg_default_params(vba_surfel_reg_params *p) {
  if (!p) return;
  p->gate = 3.0; p->neighbors = 7; p->max_iter = 30; p->min_matches = 50; p->eps_rot = 1e-5; p->eps_tra = 1e-5;
}

int vba_surfel_register(vba_surfel_map *m, int64_t n, const double *pnt, const vba_surfel_reg_params *p, double *R, double *t,
                        vba_surfel_reg_report *rep) {
  if (!sreg_reg_args_ok(m, n, pnt, p, R, t)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = m->ctx;
  int st;
  if ((st = sreg_unsharded(c, "vba_surfel_register"))) return st;
  HIPCHK(c, hipSetDevice(c->device));
  const double *d_pnt;
  if ((st = sreg_stage_pnt(m, n, pnt, &d_pnt))) return st;
  SregState *h = m->h_state.p;
  sreg_fill_state(h, p, R, t, p->max_iter);
  HIPCHK(c, hipMemcpyAsync(m->d_state.p, h, sizeof(*h), hipMemcpyHostToDevice, c->stream));
  for (int it = 0; it < p->max_iter; it++) sreg_pass(m, n, d_pnt, SregTaps{});   // launches after the end return at once (SregState::done)
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h, m->d_state.p, sizeof(*h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 9; k++) R[k] = h->R[k];
  for (int k = 0; k < 3; k++) t[k] = h->t[k];
  if (rep) std::memcpy(rep, &h->rep, sizeof(*rep));
  return VBA_OK;
}

int vba_debug_surfel_reg_pass(vba_surfel_map *m, int64_t n, const double *pnt, const vba_surfel_reg_params *p, double *R, double *t, int *cell,
                              unsigned char *gate, double *sums, double *dx) {
  if (!sreg_reg_args_ok(m, n, pnt, p, R, t)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = m->ctx;
  int st;
  if ((st = sreg_unsharded(c, "vba_debug_surfel_reg_pass"))) return st;
  HIPCHK(c, hipSetDevice(c->device));
  const double *d_pnt;
  if ((st = sreg_stage_pnt(m, n, pnt, &d_pnt))) return st;
  // the taps in buffers of this call: [sums 29 | dx 6] doubles, [cell n] ints, [gate n] bytes
  DevMem<double> d_out; DevMem<int> d_cell; DevMem<unsigned char> d_gate;
  HIPCHK(c, d_out.ensure(SREG_PART + 6));
  HIPCHK(c, d_cell.ensure((size_t)n));
  HIPCHK(c, d_gate.ensure((size_t)n));
  hipStream_t s = c->stream;
  SregState *h = m->h_state.p;
  sreg_fill_state(h, p, R, t, 1);
  HIPCHK(c, hipMemcpyAsync(m->d_state.p, h, sizeof(*h), hipMemcpyHostToDevice, s));
  SregTaps taps;
  taps.cell = d_cell.p; taps.gate = d_gate.p; taps.sums = d_out.p; taps.dx = d_out.p + SREG_PART;
  sreg_pass(m, n, d_pnt, taps);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h, m->d_state.p, sizeof(*h), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  hipError_t e = hipSuccess;
  if (sums) e = hipMemcpy(sums, d_out.p, SREG_PART * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && dx) e = hipMemcpy(dx, d_out.p + SREG_PART, 6 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && cell) e = hipMemcpy(cell, d_cell.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess && gate) e = hipMemcpy(gate, d_gate.p, (size_t)n, hipMemcpyDeviceToHost);
  HIPCHK(c, e);
  for (int k = 0; k < 9; k++) R[k] = h->R[k];
  for (int k = 0; k < 3; k++) t[k] = h->t[k];
  return VBA_OK;
}

}  // extern "C"
