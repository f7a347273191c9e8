// Loop retrieval of libvoxelba.so (vba_btc_*): the descriptor database, search and ICP over the kernels of
// vba_kernels_btc.hpp, and the glue around descriptor generation (vba_btcgen.hip, a unit of its own without floating-point contraction).
#include "vba_ctx.hpp"
#include "vba_sat.hpp"
#include "vba_btc_db.hpp"
#include "vba_kernels_btc.hpp"

#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <map>
#include <functional>
#include <algorithm>

using namespace vba;

namespace {

// the "loop" timing span of one call, closed on every return path
struct BtcSpan {
  vba_ctx *c; TimedSpan s{}; bool open = true;
  explicit BtcSpan(vba_ctx *cc) : c(cc) { span_begin(c, "loop", s); }
  void end() { if (open) span_end(c, "loop", s); open = false; }
  ~BtcSpan() { end(); }
};

int btc_reserve_rows(vba_btc_db *db, int need) {
  if (need <= db->cap) return VBA_OK;
  vba_ctx *c = db->ctx;
  int nc = db->cap ? db->cap : 1024;
  while (nc < need) nc *= 2;
  const size_t k = (size_t)db->nstd;
  hipStream_t s = c->stream;
  hipError_t e;
  (e = db->tri.grow_keep(3 * (size_t)nc, 3 * k, s)) || (e = db->cen.grow_keep(3 * (size_t)nc, 3 * k, s)) ||
      (e = db->loc.grow_keep(9 * (size_t)nc, 9 * k, s)) || (e = db->bits.grow_keep(3 * (size_t)nc, 3 * k, s)) ||
      (e = db->summ.grow_keep(3 * (size_t)nc, 3 * k, s)) || (e = db->frame.grow_keep((size_t)nc, k, s));
  db->d = BtcStds{db->tri, db->cen, db->loc, db->bits, db->summ, db->frame};      // the view follows whatever did grow
  HIPCHK(c, e);
  db->cap = nc;
  return VBA_OK;
}

// row checks shared by add_stds and the query: summaries are unsigned chars, masks fit occupy_len
int btc_check_rows(int n, const double *rows, const uint64_t *bits, int occupy_len) {
  const uint64_t mask = occupy_len >= 64 ? ~0ull : ((1ull << occupy_len) - 1ull);
  for (int i = 0; i < n; i++) {
    const double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    if (!(r[6] == std::floor(r[6]) && std::fabs(r[6]) < 2147483647.0)) return VBA_ERR_BAD_ARG;
    for (int k = 16; k < 19; k++) if (!(r[k] >= 0 && r[k] <= 255 && r[k] == std::floor(r[k]))) return VBA_ERR_BAD_ARG;
    for (int k = 0; k < 3; k++) if (bits[3 * (size_t)i + k] & ~mask) return VBA_ERR_BAD_ARG;
    for (int k = 0; k < 3; k++) if (!(std::fabs(r[k]) < 1e9)) return VBA_ERR_BAD_ARG;    // (int) of the cell key must be defined
  }
  return VBA_OK;
}

// rows -> SoA block [tri 3n | cen 3n | loc 9n | bits 3n | summ 3n | frame n] (host), and the views of the same block on the device
size_t btc_pack_bytes(int n) { return (size_t)n * (15 * sizeof(double) + 3 * sizeof(unsigned long long) + 4 * sizeof(int)); }
void btc_pack(int n, const double *rows, const uint64_t *bits, char *h) {
  double *tri = (double *)h, *cen = tri + 3 * (size_t)n, *loc = cen + 3 * (size_t)n;
  unsigned long long *bb = (unsigned long long *)(loc + 9 * (size_t)n);
  int *summ = (int *)(bb + 3 * (size_t)n), *frame = summ + 3 * (size_t)n;
  for (int i = 0; i < n; i++) {
    const double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    for (int k = 0; k < 3; k++) { tri[3 * i + k] = r[k]; cen[3 * i + k] = r[3 + k]; summ[3 * i + k] = (int)r[16 + k]; bb[3 * i + k] = bits[3 * (size_t)i + k]; }
    for (int k = 0; k < 9; k++) loc[9 * i + k] = r[7 + k];
    frame[i] = (int)r[6];
  }
}
BtcStds btc_view(int n, char *dev) {
  BtcStds v;
  v.tri = (double *)dev; v.cen = v.tri + 3 * (size_t)n; v.loc = v.cen + 3 * (size_t)n;
  v.bits = (unsigned long long *)(v.loc + 9 * (size_t)n);
  v.summ = (int *)(v.bits + 3 * (size_t)n); v.frame = v.summ + 3 * (size_t)n;
  return v;
}

int btc_table_upload(vba_btc_db *db) {
  vba_ctx *c = db->ctx;
  db->d_tab.reset();
  HIPCHK(c, db->d_tab.ensure(db->tab.size()));
  HIPCHK(c, hipMemcpyAsync(db->d_tab, db->tab.data(), db->tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return VBA_OK;
}
int btc_table_find(const std::vector<int> &tab, int mask, int x, int y, int z, bool &fresh) {
  unsigned s = btc_hash(x, y, z) & (unsigned)mask;
  for (;;) {
    const int *e = tab.data() + 8 * (size_t)s;
    if (e[3] < 0) { fresh = true; return (int)s; }
    if (e[0] == x && e[1] == y && e[2] == z) { fresh = false; return (int)s; }
    s = (s + 1) & (unsigned)mask;
  }
}
void btc_table_init(std::vector<int> &tab, int slots) {
  tab.assign((size_t)slots * 8, 0);
  for (int s = 0; s < slots; s++) { tab[8 * (size_t)s + 3] = -1; tab[8 * (size_t)s + 5] = -1; }
}

// the host table into `slots` slots (a power of two), entries re-probed in slot order; the caller uploads it
void btc_rehash(vba_btc_db *db, int slots) {
  std::vector<int> nt;
  btc_table_init(nt, slots);
  for (int u = 0; u <= db->tab_mask; u++) {
    const int *e = db->tab.data() + 8 * (size_t)u;
    if (e[3] < 0) continue;
    bool f2;
    const int t = btc_table_find(nt, slots - 1, e[0], e[1], e[2], f2);
    std::memcpy(nt.data() + 8 * (size_t)t, e, 8 * sizeof(int));
  }
  db->tab.swap(nt);
  db->tab_mask = slots - 1;
}

// one search of db, enqueued: counts, scan, ranked match list + votes, candidate list, verification, choice, result -> h_res
int btc_enqueue(vba_btc_db *db, const BtcStds &q, int n, const float *pl, int npl) {
  vba_ctx *c = db->ctx;
  const int nf = (int)db->off.size() - 1, G = 27 * n, nb = (G + 3) / 4;
  const BtcCfgDev cf = db->dev_cfg();
  const BtcIndex ix = db->index();
  int *mq = db->d_m, *md = mq + db->mcap, *mf = md + db->mcap, *pq = mf + db->mcap, *pd = pq + db->mcap;
  if (nf > 0) HIPCHK(c, hipMemsetAsync(db->d_votes, 0, (size_t)nf * sizeof(int), c->stream));
  k_btc_match<true><<<nb, 256, 0, c->stream>>>(n, q, db->d, ix, cf, c->sat->btc.d_cnt, db->d_total, db->mcap, mq, md, mf, db->d_votes);
  k_det_scan<<<1, 1024, 0, c->stream>>>(c->sat->btc.d_cnt, G, db->d_total, -1, 0, 0);
  k_btc_match<false><<<nb, 256, 0, c->stream>>>(n, q, db->d, ix, cf, c->sat->btc.d_cnt, db->d_total, db->mcap, mq, md, mf, db->d_votes);
  k_btc_select<<<1, 256, 0, c->stream>>>(nf, db->cfg.candidate_num, db->mcap, db->d_total, db->d_votes, db->d_cand, db->d_res);
  k_btc_verify<<<db->cfg.candidate_num, 256, 0, c->stream>>>(q, db->d, cf, db->d_total, db->mcap, mq, md, mf, pq, pd, db->d_cand, db->d_res,
                                                             db->d_cres, pl, npl, db->d_pc, db->d_off);
  k_btc_final<<<1, 64, 0, c->stream>>>(cf, db->d_cand, db->d_cres, db->d_res);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(db->h_res, db->d_res, BTC_RES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return VBA_OK;
}

void btc_result(const vba_btc_db *db, vba_btc_result *r) {
  const double *h = db->h_res;
  r->loop_id = (int)h[0]; r->score = h[1];
  for (int k = 0; k < 3; k++) r->t[k] = h[2 + k];
  for (int k = 0; k < 9; k++) r->R[k] = h[5 + k];
}

int btc_search_run(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur, int cur_frame,
                   vba_btc_result *results);
int btc_search(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur, int cur_frame,
               vba_btc_result *results) {
  if (n_db < 0 || (n_db > 0 && (!dbs || !results)) || n < 0 || (n > 0 && (!rows || !bits)) || !cur) return VBA_ERR_BAD_ARG;
  if (n_db == 0) return VBA_OK;
  vba_ctx *c = dbs[0]->ctx;
  for (int k = 0; k < n_db; k++) if (!dbs[k] || dbs[k]->ctx != c) return VBA_ERR_BAD_ARG;
  if (cur->ctx != c || cur_frame < 0 || cur_frame >= (int)cur->off.size() - 1) return VBA_ERR_BAD_ARG;
  for (int k = 0; k < n_db; k++) { const int st = btc_check_rows(n, rows, bits, dbs[k]->cfg.occupy_len); if (st) return st; }
  if (n == 0) {                                                   // BTC.cpp:210-214
    for (int k = 0; k < n_db; k++) { results[k] = vba_btc_result{}; results[k].loop_id = -1; dbs[k]->have_search = false; }
    return VBA_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  BtcSpan sp(c);
  return btc_search_run(n_db, dbs, n, rows, bits, cur, cur_frame, results);
}

int btc_search_run(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur, int cur_frame,
                   vba_btc_result *results) {
  vba_ctx *c = dbs[0]->ctx;
  // query upload (once) and the shared count scratch
  const size_t qb = btc_pack_bytes(n);
  if (qb > c->sat->btc.h_q.n) {                                          // (the pinned half is made last)
    c->sat->btc.d_q.reset(); c->sat->btc.h_q.reset();
    size_t nbytes = 1 << 16;
    while (nbytes < qb) nbytes *= 2;
    HIPCHK(c, c->sat->btc.d_q.ensure(nbytes));
    HIPCHK(c, c->sat->btc.h_q.ensure(nbytes));
  }
  if ((size_t)27 * n > c->sat->btc.d_cnt.n) {
    size_t m = 8192;
    while (m < (size_t)27 * n) m *= 2;
    HIPCHK(c, c->sat->btc.d_cnt.ensure(m));
  }
  for (int k = 0; k < n_db; k++) {                                // votes sized by the frames pushed so far
    vba_btc_db *db = dbs[k];
    const int nf = (int)db->off.size() - 1;
    if (nf > db->vcap) {
      int m = db->vcap ? db->vcap : 1024;
      while (m < nf) m *= 2;
      HIPCHK(c, db->d_votes.grow_keep((size_t)m, 0, c->stream));
      db->vcap = m;
    }
  }
  btc_pack(n, rows, bits, c->sat->btc.h_q);
  HIPCHK(c, hipMemcpyAsync(c->sat->btc.d_q, c->sat->btc.h_q, qb, hipMemcpyHostToDevice, c->stream));
  const BtcStds q = btc_view(n, c->sat->btc.d_q);
  const int plo = cur->off[cur_frame], npl = cur->off[cur_frame + 1] - plo;
  const float *pl = cur->d_pc ? cur->d_pc + 6 * (size_t)plo : nullptr;
  for (int k = 0; k < n_db; k++) { const int st = btc_enqueue(dbs[k], q, n, pl, npl); if (st) return st; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // a match list that did not fit: grow it and search that database again (amortised: the list only grows)
  for (int k = 0; k < n_db; k++) {
    vba_btc_db *db = dbs[k];
    const double total = db->h_res[15];
    if (total > db->mcap) {
      int m = db->mcap;
      while (m < total) m *= 2;
      HIPCHK(c, db->d_m.grow_keep(5 * (size_t)m, 0, c->stream));
      db->mcap = m;
      int st;
      if ((st = btc_enqueue(db, q, n, pl, npl))) return st;
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    db->have_search = true;
    btc_result(db, &results[k]);
  }
  return VBA_OK;
}

}  // namespace

extern "C" {

int vba_btc_default_config(int is_high_fly, vba_btc_config *f) {   // BTC.cpp:3-68
  if (!f) return VBA_ERR_BAD_ARG;
  std::memset(f, 0, sizeof(*f));
  f->skip_near_num = 30;
  f->candidate_num = is_high_fly ? 100 : 20;
  f->rough_dis_threshold = 0.01f;
  f->similarity_threshold = is_high_fly ? 0.5f : 0.7f;
  f->icp_threshold = 0.15f;
  f->normal_threshold = 0.2f;
  f->dis_threshold = 0.5f;
  f->occupy_len = 50;   // (proj_dis_max_ - proj_dis_min_) / proj_image_high_inc_: 5 / 0.1 and 10 / 0.2
  return VBA_OK;
}

int vba_btc_create(vba_ctx *c, const vba_btc_config *cfg, vba_btc_db **out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VBA_ERR_NO_DEVICE;
  if (!c || !cfg || !out) return VBA_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->occupy_len < 0 || cfg->occupy_len > 64 || cfg->candidate_num < 1 || cfg->candidate_num > BTC_MAX_CAND) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  vba_btc_db *db = new vba_btc_db();
  db->ctx = c; db->cfg = *cfg;
  vba_btc_default_gen_config(0, &db->gcfg);
  btc_table_init(db->tab, 1024);
  db->tab_mask = 1023;
  auto make = [c](auto &m, size_t n) -> int { HIPCHK(c, m.ensure(n)); return VBA_OK; };
  int st = btc_table_upload(db);
  if (!st) st = btc_reserve_rows(db, 1024);
  if (!st) st = make(db->d_off, 1024);
  if (!st) st = make(db->d_ent, (size_t)256 * BTC_CHUNK);
  if (!st) st = make(db->d_next, 256);
  if (!st) st = make(db->d_m, 5 * (size_t)65536);
  if (!st) st = make(db->d_votes, 1024);
  if (!st) st = make(db->d_cand, 5 * (size_t)BTC_MAX_CAND);
  if (!st) st = make(db->d_total, 4);
  if (!st) st = make(db->d_cres, 13 * (size_t)BTC_MAX_CAND);
  if (!st) st = make(db->d_res, BTC_RES);
  if (!st && db->h_res.ensure(BTC_RES) != hipSuccess) st = VBA_ERR_HIP;
  if (st) { vba_btc_destroy(db); return st; }
  db->off_cap = 1024; db->chunk_cap = 256; db->mcap = 65536; db->vcap = 1024;
  const int zero = 0;
  hipMemcpyAsync(db->d_off, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess) { vba_btc_destroy(db); return VBA_ERR_HIP; }
  *out = db;
  return VBA_OK;
}

void vba_btc_destroy(vba_btc_db *db) {
  if (!db) return;
  vba_ctx *c = db->ctx;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  delete db->gen;      // its buffers free themselves (vba_mem.hpp)
  delete db;
}

int vba_btc_reserve(vba_btc_db *db, int stds, int frames, int64_t cloud_points, int matches) {
  if (!db || stds < 0 || frames < 0 || cloud_points < 0 || matches < 0 || stds > (1 << 29) || frames > (1 << 29) || matches > (1 << 28))
    return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if ((st = btc_reserve_rows(db, stds))) return st;
  int slots = db->tab_mask + 1;                               // cells <= descriptors, load factor <= 1/2
  while (slots < 2 * stds) slots *= 2;
  if (slots > db->tab_mask + 1) { btc_rehash(db, slots); if ((st = btc_table_upload(db))) return st; }
  if (stds > db->chunk_cap) {                                 // chunks <= descriptors
    int m = db->chunk_cap;
    while (m < stds) m *= 2;
    HIPCHK(c, db->d_ent.grow_keep((size_t)m * BTC_CHUNK, (size_t)db->nchunk * BTC_CHUNK, c->stream));
    HIPCHK(c, db->d_next.grow_keep((size_t)m, (size_t)db->nchunk, c->stream));
    db->chunk_cap = m;
  }
  if (frames + 1 > db->off_cap) {
    int m = db->off_cap;
    while (m < frames + 1) m *= 2;
    HIPCHK(c, db->d_off.grow_keep((size_t)m, db->off.size(), c->stream));
    db->off_cap = m;
  }
  if (frames > db->vcap) {
    int m = db->vcap;
    while (m < frames) m *= 2;
    HIPCHK(c, db->d_votes.grow_keep((size_t)m, 0, c->stream));
    db->vcap = m;
  }
  if ((size_t)cloud_points > db->pc_cap) {
    size_t m = db->pc_cap ? db->pc_cap : 65536;
    while (m < (size_t)cloud_points) m *= 2;
    HIPCHK(c, db->d_pc.grow_keep(6 * m, 6 * (size_t)db->off.back(), c->stream));
    db->pc_cap = m;
  }
  if (matches > db->mcap) {
    int m = db->mcap;
    while (m < matches) m *= 2;
    HIPCHK(c, db->d_m.grow_keep(5 * (size_t)m, 0, c->stream));
    db->mcap = m;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_set_skip_near_num(vba_btc_db *db, int v) { if (!db) return VBA_ERR_BAD_ARG; db->cfg.skip_near_num = v; return VBA_OK; }
int vba_btc_num_frames(vba_btc_db *db) { return db ? (int)db->off.size() - 1 : -1; }
int vba_btc_frame_seq(vba_btc_db *db, int frame, int *seq) {
  if (!db || !seq || frame < 0 || frame >= (int)db->seq.size()) return VBA_ERR_BAD_ARG;
  *seq = db->seq[frame];
  return VBA_OK;
}

int vba_btc_push_plane_cloud(vba_btc_db *db, int n, const float *xyz_normal, int seq) {
  if (!db || n < 0 || (n > 0 && !xyz_normal)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t have = (size_t)db->off.back(), need = have + (size_t)n;
  if (need > db->pc_cap) {
    size_t m = db->pc_cap ? db->pc_cap : 65536;
    while (m < need) m *= 2;
    HIPCHK(c, db->d_pc.grow_keep(6 * m, 6 * have, c->stream));
    db->pc_cap = m;
  }
  const int nf = (int)db->off.size();        // frames after this push + 1 offsets
  if (nf + 1 > db->off_cap) {
    int m = db->off_cap * 2;
    while (m < nf + 1) m *= 2;
    HIPCHK(c, db->d_off.grow_keep((size_t)m, (size_t)nf, c->stream));
    db->off_cap = m;
  }
  if (need > (size_t)INT32_MAX) return VBA_ERR_CAPACITY;
  db->off.push_back((int)need);
  db->seq.push_back(seq);
  if (n) HIPCHK(c, hipMemcpyAsync(db->d_pc + 6 * have, xyz_normal, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d_off + nf, &db->off.back(), sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_add_stds(vba_btc_db *db, int n, const double *rows, const uint64_t *bits) {   // BTC.cpp:258-277
  if (!db || n < 0 || (n > 0 && (!rows || !bits))) return VBA_ERR_BAD_ARG;
  if (n == 0) { db->n_add++; return VBA_OK; }
  vba_ctx *c = db->ctx;
  int st = btc_check_rows(n, rows, bits, db->cfg.occupy_len);
  if (st) return st;
  const int nf = (int)db->off.size() - 1;
  for (int i = 0; i < n; i++) { const double f = rows[(size_t)i * VBA_BTC_ROW_LEN + 6]; if (f < 0 || f >= nf) return VBA_ERR_BAD_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if ((st = btc_reserve_rows(db, db->nstd + n))) return st;
  // rows -> SoA at [nstd, nstd + n)
  std::vector<char> h(btc_pack_bytes(n));
  btc_pack(n, rows, bits, h.data());
  const BtcStds v = btc_view(n, h.data());
  const size_t k = (size_t)db->nstd;
  HIPCHK(c, hipMemcpyAsync(db->d.tri + 3 * k, v.tri, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.cen + 3 * k, v.cen, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.loc + 9 * k, v.loc, 9 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.bits + 3 * k, v.bits, 3 * (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.summ + 3 * k, v.summ, 3 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(db->d.frame + k, v.frame, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  // cell index: STD_LOC = (int)(triangle_ + 0.5) (BTC.cpp:263-266); each cell's chunks list its descriptors in insertion order
  std::vector<int> ent, nxt, slots;          // (position, value) pairs and the touched table slots
  bool rehash = false;
  for (int i = 0; i < n; i++) {
    const double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    const int x = (int)(r[0] + 0.5), y = (int)(r[1] + 0.5), z = (int)(r[2] + 0.5);
    bool fresh;
    int s = btc_table_find(db->tab, db->tab_mask, x, y, z, fresh);
    if (fresh && 2 * (db->ncell + 1) > db->tab_mask + 1) {     // keep the load factor <= 1/2: rehash into twice the slots
      btc_rehash(db, 2 * (db->tab_mask + 1));
      rehash = true;
      slots.clear();
      s = btc_table_find(db->tab, db->tab_mask, x, y, z, fresh);
    }
    int *e = db->tab.data() + 8 * (size_t)s;
    if (fresh) { e[0] = x; e[1] = y; e[2] = z; e[3] = -1; e[4] = 0; e[5] = -1; db->ncell++; }
    if (e[4] % BTC_CHUNK == 0) {                                // a new chunk for this cell
      if (db->nchunk + 1 > db->chunk_cap) {
        const int m = db->chunk_cap * 2;
        HIPCHK(c, db->d_ent.grow_keep((size_t)m * BTC_CHUNK, (size_t)db->nchunk * BTC_CHUNK, c->stream));
        HIPCHK(c, db->d_next.grow_keep((size_t)m, (size_t)db->nchunk, c->stream));
        db->chunk_cap = m;
      }
      const int ch = db->nchunk++;
      if (e[5] >= 0) { nxt.push_back(e[5]); nxt.push_back(ch); }
      else e[3] = ch;
      nxt.push_back(ch); nxt.push_back(-1);
      e[5] = ch;
    }
    ent.push_back(e[5] * BTC_CHUNK + e[4] % BTC_CHUNK); ent.push_back(db->nstd + i);
    e[4]++;
    if (!rehash) slots.push_back(s);
  }
  db->nstd += n;
  // a chunk opened and then linked in the same batch appears twice in nxt ((ch, -1), later (ch, ch2)): keep the LAST value per
  // position, so every position is written once by the scatter (two writes to one address in one launch have no order)
  {
    std::map<int, int> last;
    for (size_t u = 0; u < nxt.size(); u += 2) last[nxt[u]] = nxt[u + 1];
    nxt.clear();
    for (const auto &kv : last) { nxt.push_back(kv.first); nxt.push_back(kv.second); }
  }
  // one upload of the (position, value) pairs, three scatters; the table goes whole after a rehash
  std::vector<int> tp;
  if (!rehash) {
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    for (int s : slots) for (int u = 0; u < 8; u++) { tp.push_back(8 * s + u); tp.push_back(db->tab[8 * (size_t)s + u]); }
  } else if ((st = btc_table_upload(db))) return st;
  std::vector<int> all;
  all.insert(all.end(), ent.begin(), ent.end());
  all.insert(all.end(), nxt.begin(), nxt.end());
  all.insert(all.end(), tp.begin(), tp.end());
  if ((st = ensure_stage(c, all.size() * sizeof(int)))) return st;
  int *ds = (int *)c->d_stage.p;
  HIPCHK(c, hipMemcpyAsync(ds, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  const int ne = (int)ent.size() / 2, nn = (int)nxt.size() / 2, nt = (int)tp.size() / 2;
  if (ne) k_btc_scatter<<<(ne + 255) / 256, 256, 0, c->stream>>>(ne, ds, db->d_ent);
  if (nn) k_btc_scatter<<<(nn + 255) / 256, 256, 0, c->stream>>>(nn, ds + 2 * ne, db->d_next);
  if (nt) k_btc_scatter<<<(nt + 255) / 256, 256, 0, c->stream>>>(nt, ds + 2 * (ne + nn), db->d_tab);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->n_add++;
  return VBA_OK;
}

int vba_btc_search_loop(vba_btc_db *db, int n, const double *rows, const uint64_t *bits, const vba_btc_db *cur_db, int cur_frame,
                        vba_btc_result *result) {
  if (!db || !result) return VBA_ERR_BAD_ARG;
  vba_btc_db *dbs[1] = {db};
  return btc_search(1, dbs, n, rows, bits, cur_db, cur_frame, result);
}

int vba_btc_search_loop_sessions(int n_db, vba_btc_db *const *dbs, int n, const double *rows, const uint64_t *bits,
                                 const vba_btc_db *cur_db, int cur_frame, vba_btc_result *results) {
  return btc_search(n_db, dbs, n, rows, bits, cur_db, cur_frame, results);
}

int vba_btc_last_candidates(vba_btc_db *db, int cap, vba_btc_candidate *out, int *n) {
  if (!db || !n || cap < 0 || (cap > 0 && !out)) return VBA_ERR_BAD_ARG;
  *n = 0;
  if (!db->have_search) return VBA_OK;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const int nc = (int)db->h_res[14];
  *n = nc;
  const int m = nc < cap ? nc : cap;
  if (m == 0) return VBA_OK;
  std::vector<int> ci(5 * (size_t)m);
  std::vector<double> cr(13 * (size_t)m);
  HIPCHK(c, hipMemcpyAsync(ci.data(), db->d_cand, ci.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cr.data(), db->d_cres, cr.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < m; k++) {
    out[k].frame = ci[5 * k]; out[k].votes = ci[5 * k + 1]; out[k].match_len = ci[5 * k + 1];
    out[k].max_vote_index = ci[5 * k + 3]; out[k].max_vote = ci[5 * k + 4]; out[k].score = cr[13 * k];
  }
  return VBA_OK;
}

// ---- icp_normal: one iteration is btc_icp_pass, for the loop of vba_btc_icp_normal and for vba_debug_btc_icp_pass alike
struct BtcIcpClouds { int ns, nt; const float *src, *tar; };
struct BtcIcpTaps { unsigned long long *key = nullptr; unsigned char *gate = nullptr; double *sums = nullptr, *dx = nullptr; };   // device, null in the loop

static bool btc_icp_frames_ok(const vba_btc_db *src_db, int src_frame, const vba_btc_db *tar_db, int tar_frame) {
  return src_frame >= 0 && src_frame < (int)src_db->off.size() - 1 && tar_frame >= 0 && tar_frame < (int)tar_db->off.size() - 1;
}
static BtcIcpClouds btc_icp_clouds(const vba_btc_db *src_db, int src_frame, const vba_btc_db *tar_db, int tar_frame) {
  BtcIcpClouds cl;
  cl.ns = src_db->off[src_frame + 1] - src_db->off[src_frame]; cl.nt = tar_db->off[tar_frame + 1] - tar_db->off[tar_frame];
  cl.src = src_db->d_pc ? src_db->d_pc + 6 * (size_t)src_db->off[src_frame] : nullptr;
  cl.tar = tar_db->d_pc ? tar_db->d_pc + 6 * (size_t)tar_db->off[tar_frame] : nullptr;
  return cl;
}
// The plan of a pass: nb workgroups of 256 source points, the target cut into `slices` runs of ceil(ntile / slices) tiles of 256 for
// the 1-NN launch (about 1024 workgroups).  want = 0: the pass's own choice; k >= 1: k, refused beyond max(ntile, 1) (k_btc_icp_nn
// would divide the tiles by more slices than there are) and beyond 1024 workgroups.  Touches nothing.
struct BtcIcpPlan { int nb, slices; };
static bool btc_icp_plan(const BtcIcpClouds &cl, int want, BtcIcpPlan *p) {
  const int nb = cl.ns > 0 ? (cl.ns + 255) / 256 : 1, ntile = (cl.nt + 255) / 256;
  int slices = 1;
  if (want > 0) {
    if (want > (ntile > 1 ? ntile : 1) || (long long)nb * want > 1024) return false;
    slices = want;
  } else {
    while (slices < ntile && nb * slices * 2 <= 1024) slices *= 2;          // ~1024 workgroups on the 1-NN pass
    if (slices > ntile && ntile > 0) slices = ntile;
  }
  p->nb = nb; p->slices = slices;
  return true;
}
// the key [slices][ns] and partial [nb][35] buffers of a plan (grow-only; nothing to do once they fit)
static int btc_icp_ensure(vba_ctx *c, const BtcIcpClouds &cl, const BtcIcpPlan &p) {
  if ((size_t)p.slices * cl.ns > c->sat->btc.d_icpkey.n) {
    size_t m = 65536;
    while (m < (size_t)p.slices * cl.ns) m *= 2;
    HIPCHK(c, c->sat->btc.d_icpkey.grow_keep(m, 0, c->stream));
  }
  if ((size_t)p.nb * BTC_ICP_PART > c->sat->btc.d_icppart.n) {
    size_t m = 4096;
    while (m < (size_t)p.nb * BTC_ICP_PART) m *= 2;
    HIPCHK(c, c->sat->btc.d_icppart.grow_keep(m, 0, c->stream));
  }
  return VBA_OK;
}
static int btc_icp_pass(vba_ctx *c, const BtcIcpClouds &cl, int want, const BtcIcpTaps &tp, int *slices_used) {
  BtcIcpPlan p;
  if (!btc_icp_plan(cl, want, &p)) return VBA_ERR_BAD_ARG;
  const int st = btc_icp_ensure(c, cl, p);
  if (st) return st;
  const int nb = p.nb, slices = p.slices;
  auto &B = c->sat->btc;
  k_btc_icp_nn<<<dim3(nb, slices), 256, 0, c->stream>>>(cl.ns, cl.src, cl.nt, cl.tar, B.d_icp, B.d_icpkey);
  k_btc_icp_accum<<<nb, 256, 0, c->stream>>>(cl.ns, cl.src, cl.tar, slices, B.d_icpkey, B.d_icp, B.d_icppart, tp.key, tp.gate);
  k_btc_icp_step<<<1, 64, 0, c->stream>>>(nb, B.d_icppart, B.d_icp, tp.sums, tp.dx);
  if (slices_used) *slices_used = slices;
  return VBA_OK;
}

int vba_btc_icp_normal(vba_btc_db *src_db, int src_frame, vba_btc_db *tar_db, int tar_frame, double *t, double *R, double icp_eigval,
                       int *ok, double *eig, int *iters) {   // loop_refine.hpp:47-139
  if (!src_db || !tar_db || !t || !R || src_db->ctx != tar_db->ctx) return VBA_ERR_BAD_ARG;
  if (!btc_icp_frames_ok(src_db, src_frame, tar_db, tar_frame)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = src_db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const BtcIcpClouds cl = btc_icp_clouds(src_db, src_frame, tar_db, tar_frame);
  HIPCHK(c, c->sat->btc.d_icp.ensure(1));
  HIPCHK(c, c->sat->btc.h_icp.ensure(1));
  BtcSpan sp(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));       // (the pinned state block may still be in flight from an earlier call)
  BtcIcpDev *h = c->sat->btc.h_icp;
  std::memset(h, 0, sizeof(*h));
  for (int k = 0; k < 9; k++) h->R[k] = R[k];
  for (int k = 0; k < 3; k++) h->t[k] = t[k];
  h->paras[0] = 0.2; h->paras[1] = 0.2; h->paras[2] = 0.5; h->paras[3] = 3;
  HIPCHK(c, hipMemcpyAsync(c->sat->btc.d_icp, h, sizeof(*h), hipMemcpyHostToDevice, c->stream));
  for (int it = 0; it < BTC_ICP_ITERS; it++) {       // launches after convergence return at once (BtcIcpDev::done)
    const int st = btc_icp_pass(c, cl, 0, BtcIcpTaps{}, nullptr);
    if (st) return st;
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h, c->sat->btc.d_icp, sizeof(*h), hipMemcpyDeviceToHost, c->stream));
  sp.end();
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 9; k++) R[k] = h->R[k];
  for (int k = 0; k < 3; k++) t[k] = h->t[k];
  if (eig) for (int k = 0; k < 3; k++) eig[k] = h->eig[k];
  if (iters) *iters = h->iters;
  if (ok) *ok = (h->eig[0] > icp_eigval && h->is_conv == 1) ? 1 : 0;
  return VBA_OK;
}

static_assert(sizeof(vba_btc_icp_state) == sizeof(BtcIcpDev), "vba_btc_icp_state mirrors BtcIcpDev");

int vba_debug_btc_icp_pass(vba_btc_db *src_db, int src_frame, vba_btc_db *tar_db, int tar_frame, vba_btc_icp_state *state, int slices,
                           unsigned long long *key, unsigned char *gate, double *partial, double *sums, double *dx, int *slices_used) {
  if (!src_db || !tar_db || !state || src_db->ctx != tar_db->ctx || slices < 0) return VBA_ERR_BAD_ARG;
  if (!btc_icp_frames_ok(src_db, src_frame, tar_db, tar_frame)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = src_db->ctx;
  if (c->n_ranks > 1) { c->set_error("vba_debug_btc_icp_pass runs the ICP of one device: unsharded contexts only"); return VBA_ERR_UNSUPPORTED; }
  HIPCHK(c, hipSetDevice(c->device));
  const BtcIcpClouds cl = btc_icp_clouds(src_db, src_frame, tar_db, tar_frame);
  BtcIcpPlan plan;
  if (!btc_icp_plan(cl, slices, &plan)) return VBA_ERR_BAD_ARG;      // a slice count outside the plan: nothing is touched
  const int nb = plan.nb;
  int st = btc_icp_ensure(c, cl, plan);                 // (the caller's partial is copied into the production buffer below)
  if (st) return st;
  HIPCHK(c, c->sat->btc.d_icp.ensure(1));
  HIPCHK(c, c->sat->btc.h_icp.ensure(1));
  // the taps in buffers of this call: [sums 35 | dx 6] doubles, [merged key ns] words, [gate ns] bytes.  Each starts as the caller's
  // array, so a launch that returns at once leaves the caller's values.
  const size_t ns = (size_t)cl.ns;
  DevMem<double> d_out;
  DevMem<unsigned long long> d_key;
  DevMem<unsigned char> d_gate;
  HIPCHK(c, d_out.ensure(BTC_ICP_PART + 6));
  HIPCHK(c, d_key.ensure(ns ? ns : 1));
  HIPCHK(c, d_gate.ensure(ns ? ns : 1));
  hipStream_t s = c->stream;
  HIPCHK(c, hipStreamSynchronize(s));
  BtcIcpDev *h = c->sat->btc.h_icp;
  std::memcpy(h, state, sizeof(*h));
  HIPCHK(c, hipMemcpyAsync(c->sat->btc.d_icp, h, sizeof(*h), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(d_out.p, 0, (BTC_ICP_PART + 6) * sizeof(double), s));
  if (sums) HIPCHK(c, hipMemcpyAsync(d_out.p, sums, BTC_ICP_PART * sizeof(double), hipMemcpyHostToDevice, s));
  if (dx) HIPCHK(c, hipMemcpyAsync(d_out.p + BTC_ICP_PART, dx, 6 * sizeof(double), hipMemcpyHostToDevice, s));
  if (partial) HIPCHK(c, hipMemcpyAsync(c->sat->btc.d_icppart, partial, (size_t)nb * BTC_ICP_PART * sizeof(double), hipMemcpyHostToDevice, s));
  if (key && ns) HIPCHK(c, hipMemcpyAsync(d_key.p, key, ns * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
  if (gate && ns) HIPCHK(c, hipMemcpyAsync(d_gate.p, gate, ns, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));                   // (the caller's arrays are pageable: nothing of them stays in flight)
  BtcIcpTaps taps;
  taps.key = d_key.p; taps.gate = d_gate.p; taps.sums = d_out.p; taps.dx = d_out.p + BTC_ICP_PART;
  st = btc_icp_pass(c, cl, slices, taps, slices_used);
  if (st) { hipStreamSynchronize(s); return st; }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h, c->sat->btc.d_icp, sizeof(*h), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  hipError_t e = hipSuccess;
  if (sums) e = hipMemcpy(sums, d_out.p, BTC_ICP_PART * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && dx) e = hipMemcpy(dx, d_out.p + BTC_ICP_PART, 6 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && partial) e = hipMemcpy(partial, c->sat->btc.d_icppart, (size_t)nb * BTC_ICP_PART * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && key && ns) e = hipMemcpy(key, d_key.p, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (e == hipSuccess && gate && ns) e = hipMemcpy(gate, d_gate.p, ns, hipMemcpyDeviceToHost);
  HIPCHK(c, e);
  std::memcpy(state, h, sizeof(*h));
  return VBA_OK;
}


// ------------------------------------------------------------------------------------------------ descriptor generation
int vba_btc_default_gen_config(int is_high_fly, vba_btc_gen_config *f) {   // BTC.cpp:3-68
  if (!f) return VBA_ERR_BAD_ARG;
  std::memset(f, 0, sizeof(*f));
  f->useful_corner_num = is_high_fly ? 200 : 100;
  f->plane_merge_normal_thre = is_high_fly ? 0.3f : 0.1f;
  f->plane_merge_dis_thre = is_high_fly ? 0.6f : 0.3f;
  f->plane_detection_thre = is_high_fly ? 0.05f : 0.01f;
  f->voxel_size = is_high_fly ? 2.0f : 1.0f;
  f->voxel_init_num = 10;
  f->proj_plane_num = is_high_fly ? 1 : 2;
  f->proj_image_resolution = 0.5f;
  f->proj_image_high_inc = is_high_fly ? 0.2f : 0.1f;
  f->proj_dis_min = 0.0f;
  f->proj_dis_max = is_high_fly ? 10.0f : 5.0f;
  f->summary_min_thre = is_high_fly ? 6.0f : 10.0f;
  f->line_filter_enable = is_high_fly ? 0 : 1;
  f->touch_filter_enable = 0;
  f->descriptor_near_num = 15.0f;
  f->descriptor_min_len = is_high_fly ? 3.0f : 2.0f;
  f->descriptor_max_len = 50.0f;
  f->non_max_suppression_radius = is_high_fly ? 3.0f : 2.0f;
  f->std_side_resolution = 0.2f;
  return VBA_OK;
}

namespace {
// cut_num of extract_binary: (int)((proj_dis_max_ - proj_dis_min_) / proj_image_high_inc_), the float fields promoted to double
int btc_cut_num(const vba_btc_gen_config &g) {
  return (int)(((double)g.proj_dis_max - (double)g.proj_dis_min) / (double)g.proj_image_high_inc);
}
size_t btc_max_stds(const vba_btc_gen_config &g) {      // useful_corner_num * C(K - 1, 2)
  const size_t K1 = (size_t)((int)g.descriptor_near_num - 1);
  return (size_t)g.useful_corner_num * (K1 * (K1 - 1) / 2);
}
BgCfg btc_bg_cfg(const vba_btc_gen_config &g) {
  BgCfg f;
  f.useful = g.useful_corner_num; f.vinit = g.voxel_init_num; f.proj_num = g.proj_plane_num; f.line_filter = g.line_filter_enable;
  f.touch_filter = g.touch_filter_enable; f.K = (int)g.descriptor_near_num; f.cut_num = btc_cut_num(g);
  f.merge_n = g.plane_merge_normal_thre; f.merge_d = g.plane_merge_dis_thre; f.detect = g.plane_detection_thre; f.vsize = g.voxel_size;
  f.res = g.proj_image_resolution; f.high_inc = g.proj_image_high_inc; f.dmin = g.proj_dis_min; f.dmax = g.proj_dis_max;
  f.summ_min = g.summary_min_thre; f.min_len = g.descriptor_min_len; f.max_len = g.descriptor_max_len;
  f.scale = 1.0 / (double)g.std_side_resolution;
  const double r = g.non_max_suppression_radius;
  f.nms_r2 = (float)(r * r);
  return f;
}
int btc_gen_check(const vba_btc_gen_config &g) {
  const int K = (int)g.descriptor_near_num;
  if (!(g.useful_corner_num >= 1 && g.voxel_size > 0 && g.voxel_init_num >= 0 && g.proj_plane_num >= 1 && g.proj_plane_num <= BG_MAX_PROJ &&
        g.proj_image_resolution > 0 && g.proj_image_high_inc > 0 && g.descriptor_near_num >= 3 && K <= BG_MAX_K &&
        g.descriptor_min_len >= 0 && g.descriptor_max_len <= 2000 && g.std_side_resolution > 0 && g.proj_dis_max >= g.proj_dis_min &&
        btc_cut_num(g) >= 0 && btc_cut_num(g) <= 64 && btc_max_stds(g) < (size_t)(1 << 26)))
    return VBA_ERR_BAD_ARG;
  return VBA_OK;
}
}  // namespace
extern "C++" {
namespace vba {
int btc_gen_ensure(vba_btc_db *db, int64_t points, int64_t cells, size_t corners) {
  vba_ctx *c = db->ctx;
  if (!db->gen) db->gen = new BtcGen();
  const BtcGen &g = *db->gen;
  const size_t stds = btc_max_stds(db->gcfg);
  if ((size_t)points <= g.pts_cap && (size_t)cells <= g.cell_cap && corners <= g.corn_cap && stds <= g.cand_cap &&
      g.pts_cap / (size_t)(db->gcfg.voxel_init_num + 1) + 1 <= g.plane_cap && g.h_cnt)
    return VBA_OK;
  HIPCHK(c, btcgen_reserve(*db->gen, (size_t)points, (size_t)cells, corners, stds, db->gcfg.voxel_init_num, c->stream));
  return VBA_OK;
}
}  // namespace vba
}  // extern "C++"

int vba_btc_set_gen_config(vba_btc_db *db, const vba_btc_gen_config *cfg) {
  if (!db || !cfg || btc_gen_check(*cfg)) return VBA_ERR_BAD_ARG;
  db->gcfg = *cfg;
  return VBA_OK;
}

int vba_btc_get_gen_config(const vba_btc_db *db, vba_btc_gen_config *cfg) {
  if (!db || !cfg) return VBA_ERR_BAD_ARG;
  *cfg = db->gcfg;
  return VBA_OK;
}

int vba_btc_gen_reserve(vba_btc_db *db, int64_t points, int64_t cells, int frames) {
  if (!db || points < 0 || cells < 0 || frames < 0 || points > (1 << 28) || cells > BG_MAX_CELLS || frames > (1 << 20)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  int st;
  if ((st = btc_gen_ensure(db, points, cells, 0))) return st;
  // plane-cloud room for `frames` more calls at the bound a call reserves (points / (voxel_init_num + 1) + 1 planes each)
  const int64_t planes = (int64_t)(points / (db->gcfg.voxel_init_num + 1) + 1) * frames;
  if ((st = vba_btc_reserve(db, 0, (int)db->off.size() - 1 + frames + 1, (int64_t)db->off.back() + planes, 0))) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_gen_allocations(vba_btc_db *db, int *count, int64_t *bytes) {
  if (!db || !count || !bytes) return VBA_ERR_BAD_ARG;
  *count = db->gen ? db->gen->allocs : 0;
  *bytes = db->gen ? (int64_t)db->gen->dev_bytes : 0;
  return VBA_OK;
}

extern "C++" {
namespace vba {
// the argument checks of vba_btc_generate_stds that do not concern the cloud itself (no side effect)
int btc_generate_check(vba_btc_db *db, int n, int cap, double *rows, uint64_t *bits, int *n_stds) {
  if (!db || n < 0 || n > (1 << 28) || !n_stds || cap < 0 || (cap > 0 && (!rows || !bits))) return VBA_ERR_BAD_ARG;
  const vba_btc_gen_config &g = db->gcfg;
  if ((size_t)cap < btc_max_stds(g) || btc_cut_num(g) > db->cfg.occupy_len) return VBA_ERR_BAD_ARG;
  return VBA_OK;
}
// GenerateSTDescs on a cloud from host memory (xyz) or from the device: with xyz == nullptr and n > 0 the caller has sized the
// generator for n points (btc_gen_ensure) and enqueued, ahead of the database's stream, the writes of float [n][3] into its point
// buffer db->gen->pts.xyz; the generator only reads that buffer, so a second attempt after a buffer grew finds it intact
int btc_generate_impl(vba_btc_db *db, int n, const float *xyz, int id, int cap, double *rows, uint64_t *bits, int *n_stds) {
  int chk = btc_generate_check(db, n, cap, rows, bits, n_stds);
  if (chk) return chk;
  const vba_btc_gen_config &g = db->gcfg;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  *n_stds = 0;
  if (n == 0) {                                 // empty cloud: an empty plane cloud, no corners, no descriptors
    db->last_loc.clear(); db->last_bits.clear();
    return vba_btc_push_plane_cloud(db, 0, nullptr, id);
  }
  BtcSpan sp(c);
  int st;
  const size_t planes = (size_t)n / (size_t)(g.voxel_init_num + 1) + 1;
  const size_t have = (size_t)db->off.back();
  if (have + planes > (size_t)INT32_MAX) return VBA_ERR_CAPACITY;
  if ((st = btc_gen_ensure(db, n, 0, 0))) return st;
  // room for this frame's plane cloud and offset (the same growth as vba_btc_push_plane_cloud), counted with the generator's own
  if (have + planes > db->pc_cap) {
    size_t m = db->pc_cap ? db->pc_cap : 65536;
    while (m < have + planes) m *= 2;
    HIPCHK(c, db->d_pc.grow_keep(6 * m, 6 * have, c->stream));
    db->pc_cap = m;
    db->gen->allocs++;
  }
  const int nf = (int)db->off.size();
  if (nf + 1 > db->off_cap) {
    int m = db->off_cap * 2;
    while (m < nf + 1) m *= 2;
    HIPCHK(c, db->d_off.grow_keep((size_t)m, (size_t)nf, c->stream));
    db->off_cap = m;
    db->gen->allocs++;
  }
  const BgCfg cf = btc_bg_cfg(g);
  // the image and the corner list grow on overflow and the call runs again (nothing is committed before it succeeds)
  for (int attempt = 0;; attempt++) {
    BtcGen &G = *db->gen;
    HIPCHK(c, btcgen_enqueue(G, cf, n, xyz, db->d_pc + 6 * have, db->d_off + nf, (int)have, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int *h = G.h_cnt;
    if (h[BGC_ERR] & 1) return VBA_ERR_BAD_ARG;
    if (h[BGC_ERR] & 4) return VBA_ERR_CAPACITY;           // a projection image above BG_MAX_CELLS: refused before allocating
    const bool cells_over = (h[BGC_ERR] & 2) != 0, corn_over = (size_t)h[BGC_NTEMP] > G.corn_cap;
    if (!cells_over && !corn_over) break;
    if (attempt >= 2) return VBA_ERR_CAPACITY;
    if ((st = btc_gen_ensure(db, n, cells_over ? (int64_t)h[BGC_CELLS] : 0, corn_over ? (size_t)h[BGC_NTEMP] : 0))) return st;
  }
  const BtcGen &G = *db->gen;
  const int np = G.h_cnt[BGC_NPL], ns = G.h_cnt[BGC_NSTD], nc = G.h_cnt[BGC_NCORN];
  db->off.push_back((int)(have + (size_t)np));
  db->seq.push_back(id);
  db->last_loc.resize(4 * (size_t)nc); db->last_bits.resize(nc);
  for (int i = 0; i < nc; i++) {
    const BgCorner &k = G.cor.h_corn[i];
    for (int j = 0; j < 3; j++) db->last_loc[4 * (size_t)i + j] = k.loc[j];
    db->last_loc[4 * (size_t)i + 3] = (double)k.summ;
    db->last_bits[i] = k.bits;
  }
  // rows: [triangle center frame A.loc B.loc C.loc A.summ B.summ C.summ], masks of A, B, C
  for (int i = 0; i < ns; i++) {
    const BgStd &t = G.tri.h_stds[i];
    double *r = rows + (size_t)i * VBA_BTC_ROW_LEN;
    const int v[3] = {t.a, t.b, t.c};
    for (int j = 0; j < 3; j++) { r[j] = t.tri[j]; r[3 + j] = t.cen[j]; }
    r[6] = (double)db->n_add;
    for (int u = 0; u < 3; u++) {
      const BgCorner &k = G.cor.h_corn[v[u]];
      for (int j = 0; j < 3; j++) r[7 + 3 * u + j] = k.loc[j];
      r[16 + u] = (double)k.summ;
      bits[3 * (size_t)i + u] = k.bits;
    }
  }
  *n_stds = ns;
  return VBA_OK;
}
}  // namespace vba
}  // extern "C++"

int vba_btc_generate_stds(vba_btc_db *db, int n, const float *xyz, int id, int cap, double *rows, uint64_t *bits, int *n_stds) {
  if (n > 0 && !xyz) return VBA_ERR_BAD_ARG;
  return btc_generate_impl(db, n, xyz, id, cap, rows, bits, n_stds);
}

int vba_btc_plane_cloud(vba_btc_db *db, int frame, int cap, float *xyz_normal, int *n) {
  if (!db || !n || frame < 0 || frame >= (int)db->off.size() - 1 || cap < 0 || (cap > 0 && !xyz_normal)) return VBA_ERR_BAD_ARG;
  vba_ctx *c = db->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const int b = db->off[frame], e = db->off[frame + 1];
  *n = e - b;
  const int w = (e - b) < cap ? (e - b) : cap;
  if (w > 0) HIPCHK(c, hipMemcpyAsync(xyz_normal, db->d_pc + 6 * (size_t)b, (size_t)w * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_btc_last_corners(vba_btc_db *db, int cap, double *loc_summary, uint64_t *bits, int *n) {
  if (!db || !n || cap < 0 || (cap > 0 && (!loc_summary || !bits))) return VBA_ERR_BAD_ARG;
  const int k = (int)db->last_bits.size();
  *n = k;
  const int w = k < cap ? k : cap;
  for (int i = 0; i < w; i++) {
    for (int j = 0; j < 4; j++) loc_summary[4 * (size_t)i + j] = db->last_loc[4 * (size_t)i + j];
    bits[i] = db->last_bits[i];
  }
  return VBA_OK;
}

}  // extern "C"
