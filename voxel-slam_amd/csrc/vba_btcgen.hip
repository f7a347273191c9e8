// BTC descriptor generation on the device: GenerateSTDescs (BTC.cpp:156-203) with init_voxel_map, get_plane, get_project_plane,
// merge_plane, binary_extractor / extract_binary, non_maxi_suppression and generate_std (BTC.cpp:279-1126).  Compiled with
// -ffp-contract=off: every floating-point expression is evaluated as written, in the order the reference writes it, so that the
// numpy restatement (tests/btc_gen_oracle.py) reproduces each result bit for bit.
//
// Order contract (include/voxelba.h):
//  - voxels are ordered by the index of their first point; a stable radix sort of (key, point index) keeps each voxel's points in
//    input order, and a voxel's moments are folded sequentially in that order;
//  - plane cloud and origin_list in voxel order; the greedy id assignment of get_project_plane / merge_plane replays the
//    reference's loop order (rows descending, columns ascending: each row's column tests run across a workgroup); groups fold
//    their members in ascending index from the first; the two sorts by points_size_ are stable;
//  - extract_binary: per-cell sums in the order of the kept points (stable radix sort by cell), first strict maximum in x-then-y
//    order, corners in (x segment, y segment) order;
//  - neighbours exact in float (squared L2, x then y then z, ties to the earlier index), radius test d^2 < (float)(r r);
//  - triangle dedupe: the first in (i, m, n) order wins (atomicMin of the emission index per key), output in emission order.
#include "vba_btcgen.hpp"
#include "vba_common.hpp"
#include "vba_mem.hpp"
#include "vba_btcgen_fit.hpp"

#include <climits>

namespace vba {

// (sort_pairs_u32: vba_common.hpp)
hipError_t sort_pairs_u64(void *tmp, size_t &tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out, const int *vals_in,
                          int *vals_out, size_t n, unsigned int end_bit, hipStream_t stream);

namespace {

struct BgPlane { double c[3], n[3], cov[6]; int N; float d; };
struct BgSel { double c[3], n[3], xa[3], ya[3], A, B, C, D, dx, dy; };

constexpr int BG_KEY_BITS = 21;                         // per voxel-key component: |key| < 2^20
constexpr long long BG_KEY_OFF = 1ll << 20;
constexpr unsigned long long BG_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long bg_enc(double d) {   // monotone map of a double to an unsigned key
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double bg_dec(unsigned long long u) {
  const unsigned long long b = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
  return __longlong_as_double((long long)b);
}

// exclusive scan of a[0, n) in place by one workgroup of 1024 (wg_scan_chunked of vba_common.hpp); the total goes to *total
__global__ __launch_bounds__(1024) void k_bg_scan(int *a, const int *n_in, int n_max, int *total) {
  __shared__ int buf[WG_SCAN_CHUNK];
  __shared__ int wsum[16];
  int n = n_in ? *n_in : n_max;
  if (n > n_max) n = n_max;
  const int tot = wg_scan_chunked(a, n, buf, wsum);
  if (threadIdx.x == 0) *total = tot;
}

// ---------------------------------------------------------------- voxel pass (init_voxel_map, BTC.cpp:279-320)
// key = (int64_t)(p / voxel_size - (p / voxel_size < 0 ? 1 : 0)) in double; packed into 63 bits (out of range / non-finite: error)
__global__ void k_bg_key(int n, const float *xyz, double vsize, unsigned long long *key, int *idx, int *cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long k = 0;
  bool bad = false;
  for (int j = 0; j < 3; j++) {
    double l = (double)xyz[3 * i + j] / vsize;
    if (l < 0) l -= 1.0;
    if (!(fabs(l) < (double)(BG_KEY_OFF - 1))) { bad = true; l = 0; }
    const long long q = (long long)l;
    k = (k << BG_KEY_BITS) | (unsigned long long)(q + BG_KEY_OFF);
  }
  if (bad) atomicOr(cnt + BGC_ERR, 1);
  key[i] = k; idx[i] = i;
}

// gather the points in key order; flag the first point of each voxel (its smallest index: the sort is stable)
__global__ void k_bg_gather(int n, const float *xyz, const unsigned long long *skey, const int *sidx, float *sxyz, int *flag) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int i = sidx[j];
  sxyz[3 * j] = xyz[3 * i]; sxyz[3 * j + 1] = xyz[3 * i + 1]; sxyz[3 * j + 2] = xyz[3 * i + 2];
  if (j == 0 || skey[j] != skey[j - 1]) flag[i] = 1;
}

// per voxel run (its head thread): ordinal = rank of the first point; start, length, and whether it has > voxel_init_num points
__global__ void k_bg_runs(int n, const unsigned long long *skey, const int *sidx, const int *flag, int vinit, int *vstart, int *vlen, int *isc) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (!(j == 0 || skey[j] != skey[j - 1])) return;
  int e = j + 1;
  while (e < n && skey[e] == skey[j]) e++;
  const int o = flag[sidx[j]];
  vstart[o] = j; vlen[o] = e - j; isc[o] = (e - j) > vinit ? 1 : 0;
}

// init_plane (BTC.cpp:96-138) of each candidate voxel: sequential sums in input order, covariance, eigen-solve, sign rule
__global__ void k_bg_fit(const int *cnt, const float *sxyz, const int *vstart, const int *vlen, const int *isc, const int *cidx,
                         double detect, BgPlane *cpl, int *isp) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= cnt[BGC_NVOX] || !isc[o]) return;
  const int ci = cidx[o];
  const int s = vstart[o], N = vlen[o];
  double s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0, c0 = 0, c1 = 0, c2 = 0;
  for (int k = s; k < s + N; k++) {
    const double x = sxyz[3 * k], y = sxyz[3 * k + 1], z = sxyz[3 * k + 2];
    s00 += x * x; s01 += x * y; s02 += x * z; s11 += y * y; s12 += y * z; s22 += z * z;
    c0 += x; c1 += y; c2 += z;
  }
  const double dn = (double)N;
  c0 = c0 / dn; c1 = c1 / dn; c2 = c2 / dn;
  BgPlane p;
  p.cov[0] = s00 / dn - c0 * c0; p.cov[1] = s01 / dn - c1 * c0; p.cov[2] = s02 / dn - c2 * c0;
  p.cov[3] = s11 / dn - c1 * c1; p.cov[4] = s12 / dn - c2 * c1; p.cov[5] = s22 / dn - c2 * c2;
  p.c[0] = c0; p.c[1] = c1; p.c[2] = c2; p.N = N;
  double wmin;
  btcg_plane_eig(p.cov[0], p.cov[1], p.cov[2], p.cov[3], p.cov[4], p.cov[5], wmin, p.n);
  p.d = (float)(-(p.n[0] * c0 + p.n[1] * c1 + p.n[2] * c2));
  const int ok = wmin < detect ? 1 : 0;
  isp[ci] = ok;
  cpl[ci] = p;
}

// get_plane (BTC.cpp:322-337): planes in voxel order, and the plane cloud straight into the database
__global__ void k_bg_planes(const int *cnt, const BgPlane *cpl, const int *isp_flag, const int *pidx, BgPlane *pl, float *pc, int *off_slot,
                            int have) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) *off_slot = have + cnt[BGC_NPL];
  if (c >= cnt[BGC_NCAND] || !isp_flag[c]) return;
  const int q = pidx[c];
  const BgPlane p = cpl[c];
  pl[q] = p;
  float *o = pc + 6 * (size_t)q;
  o[0] = (float)p.c[0]; o[1] = (float)p.c[1]; o[2] = (float)p.c[2];
  o[3] = (float)p.n[0]; o[4] = (float)p.n[1]; o[5] = (float)p.n[2];
}

// ---------------------------------------------------------------- projection-plane selection (one workgroup of 1024)
__device__ __forceinline__ double bg_norm(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// the pair test of get_project_plane / merge_plane (BTC.cpp:339-357): row r (iter) against column j (iter2)
__device__ __forceinline__ bool bg_pass(const BgPlane &r, const BgPlane &j, double thn, double thd) {
  const double nd = bg_norm(r.n[0] - j.n[0], r.n[1] - j.n[1], r.n[2] - j.n[2]);
  const double na = bg_norm(r.n[0] + j.n[0], r.n[1] + j.n[1], r.n[2] + j.n[2]);
  const double d1 = fabs(r.n[0] * j.c[0] + r.n[1] * j.c[1] + r.n[2] * j.c[2] + (double)r.d);
  const double d2 = fabs(j.n[0] * r.c[0] + j.n[1] * r.c[1] + j.n[2] * r.c[2] + (double)j.d);
  return (nd < thn || na < thn) && (d1 < thd && d2 < thd);
}

// exclusive rank of a flag across the workgroup (1024 threads, 16 waves); *total = flags set
__device__ int bg_block_rank(bool f, int *sh, int &total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long b = __ballot(f);
  const int r = __popcll(b & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
  if (lane == 0) sh[wave] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < 16; w++) { const int c = sh[w]; base += w < wave ? c : 0; tot += c; }
  __syncthreads();
  total = tot;
  return base + r;
}

// the greedy id assignment: rows descending; a row with id 0 takes its first passing column's id (or a new one for both); then
// every passing column still at 0 takes the row's id.  Returns the next unused id.
__device__ int bg_greedy(const BgPlane *L, int m, int *ids, int *cnt, double thn, double thd) {
  const int tid = threadIdx.x;
  for (int i = tid; i < m; i += blockDim.x) ids[i] = 0;
  if (tid == 0) cnt[BGC_CUR] = 1;
  __syncthreads();
  for (int r = m - 1; r >= 1; r--) {
    const BgPlane R = L[r];
    if (tid == 0) cnt[BGC_JMIN] = INT_MAX;
    __syncthreads();
    const int rid0 = ids[r];
    if (rid0 == 0) {
      int jm = INT_MAX;
      for (int j = tid; j < r; j += blockDim.x) if (bg_pass(R, L[j], thn, thd)) { jm = j; break; }
      if (jm != INT_MAX) atomicMin(cnt + BGC_JMIN, jm);
      __syncthreads();
      if (tid == 0) {
        const int jm2 = cnt[BGC_JMIN];
        if (jm2 != INT_MAX) {
          if (ids[jm2] == 0) { const int nid = cnt[BGC_CUR]; ids[r] = nid; ids[jm2] = nid; cnt[BGC_CUR] = nid + 1; }
          else ids[r] = ids[jm2];
        }
      }
      __syncthreads();
    }
    const int rid = ids[r];
    if (rid != 0)
      for (int j = tid; j < r; j += blockDim.x) if (ids[j] == 0 && bg_pass(R, L[j], thn, thd)) ids[j] = rid;
    __syncthreads();
  }
  return cnt[BGC_CUR];
}

// fold of a group (BTC.cpp:382-402): members in ascending index from the first, then the eigen-solve of the merged covariance
__device__ BgPlane bg_fold(const BgPlane *L, int m, const int *ids, int i) {
  BgPlane a = L[i];
  const int id = ids[i];
  for (int j = i + 1; j < m; j++) {
    if (ids[j] != id) continue;
    const BgPlane &b = L[j];
    const double n1 = (double)a.N, n2 = (double)b.N, nt = (double)(a.N + b.N);
    double mc[3], P1[6], P2[6];
    const int rr[6] = {0, 1, 2, 1, 2, 2}, cc[6] = {0, 0, 0, 1, 1, 2};
    for (int k = 0; k < 6; k++) {
      P1[k] = (a.cov[k] + a.c[rr[k]] * a.c[cc[k]]) * n1;
      P2[k] = (b.cov[k] + b.c[rr[k]] * b.c[cc[k]]) * n2;
    }
    for (int k = 0; k < 3; k++) mc[k] = (a.c[k] * n1 + b.c[k] * n2) / nt;
    for (int k = 0; k < 6; k++) a.cov[k] = (P1[k] + P2[k]) / nt - mc[rr[k]] * mc[cc[k]];
    for (int k = 0; k < 3; k++) a.c[k] = mc[k];
    a.N = a.N + b.N;
  }
  double wmin;
  btcg_plane_eig(a.cov[0], a.cov[1], a.cov[2], a.cov[3], a.cov[4], a.cov[5], wmin, a.n);
  a.d = (float)(-(a.n[0] * a.c[0] + a.n[1] * a.c[1] + a.n[2] * a.c[2]));
  return a;
}

// the lists of get_project_plane (keep_singles = 0) and merge_plane (1): in ascending position, a plane with id 0 (kept as is) or
// the fold of the group it is the first member of
__device__ int bg_groups(const BgPlane *L, int m, int *ids, int *first, int ncur, bool keep_singles, BgPlane *out, int *sh) {
  const int tid = threadIdx.x;
  for (int k = tid; k < ncur; k += blockDim.x) first[k] = INT_MAX;
  __syncthreads();
  for (int j = tid; j < m; j += blockDim.x) if (ids[j]) atomicMin(first + ids[j], j);
  __syncthreads();
  int base = 0;
  for (int c0 = 0; c0 < m; c0 += blockDim.x) {
    const int i = c0 + tid;
    bool e = false;
    if (i < m) e = ids[i] == 0 ? keep_singles : first[ids[i]] == i;
    int tot;
    const int r = bg_block_rank(e, sh, tot);
    if (e) out[base + r] = ids[i] == 0 ? L[i] : bg_fold(L, m, ids, i);
    base += tot;
  }
  __syncthreads();
  return base;
}

// std::sort(plane_greater_sort) made stable: points_size_ descending, ties in list order
__device__ void bg_sort_planes(const BgPlane *L, int m, BgPlane *out) {
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    const int Ni = L[i].N;
    int r = 0;
    for (int j = 0; j < m; j++) { const int Nj = L[j].N; r += (Nj > Ni || (Nj == Ni && j < i)) ? 1 : 0; }
    out[r] = L[i];
  }
  __syncthreads();
}

__device__ void bg_make_sel(const double *c, const double *n, BgSel &s) {   // extract_binary's axes (BTC.cpp:513-548)
  for (int k = 0; k < 3; k++) { s.c[k] = c[k]; s.n[k] = n[k]; }
  const double A = n[0], B = n[1], C = n[2];
  s.A = A; s.B = B; s.C = C;
  s.D = -(A * c[0] + B * c[1] + C * c[2]);
  double x[3] = {1, 1, 0};
  if (C != 0) x[2] = -(A + B) / C;
  else if (B != 0) x[1] = -A / B;
  else { x[0] = 0; x[1] = 1; }
  double z = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  if (z > 0) { const double q = sqrt(z); x[0] = x[0] / q; x[1] = x[1] / q; x[2] = x[2] / q; }
  double y[3] = {n[1] * x[2] - n[2] * x[1], n[2] * x[0] - n[0] * x[2], n[0] * x[1] - n[1] * x[0]};
  z = y[0] * y[0] + y[1] * y[1] + y[2] * y[2];
  if (z > 0) { const double q = sqrt(z); y[0] = y[0] / q; y[1] = y[1] / q; y[2] = y[2] / q; }
  for (int k = 0; k < 3; k++) { s.xa[k] = x[k]; s.ya[k] = y[k]; }
  s.dx = -(x[0] * c[0] + x[1] * c[1] + x[2] * c[2]);
  s.dy = -(y[0] * c[0] + y[1] * c[1] + y[2] * c[2]);
}

// get_project_plane, the sort, merge_plane, the sort, and binary_extractor's choice of projection planes (BTC.cpp:156-186, :453-483)
__global__ __launch_bounds__(1024) void k_bg_select(BgCfg cf, const float *xyz, int *cnt, BgPlane *pl, BgPlane *grp, BgPlane *srt,
                                                    BgPlane *mrg, BgPlane *fin, int *ids, int *first, BgSel *sel, unsigned long long *mm) {
  __shared__ int sh[16];
  const int tid = threadIdx.x;
  const int P = cnt[BGC_NPL];
  int ncur = bg_greedy(pl, P, ids, cnt, cf.merge_n, cf.merge_d);
  const int G = bg_groups(pl, P, ids, first, ncur, false, grp, sh);
  int M = 0;
  const BgPlane *E = nullptr;
  if (G > 0) {
    bg_sort_planes(grp, G, srt);
    if (G == 1) { M = 1; E = srt; }
    else {
      ncur = bg_greedy(srt, G, ids, cnt, cf.merge_n, cf.merge_d);
      const int M0 = bg_groups(srt, G, ids, first, ncur, true, mrg, sh);
      bg_sort_planes(mrg, M0, fin);
      M = M0; E = fin;
    }
  }
  if (tid == 0) {
    cnt[BGC_NG] = G; cnt[BGC_NM] = M;
    int ns = 0;
    if (G == 0) {                                         // single_plane: normal (0, 0, 1) through the first point
      const double c[3] = {(double)xyz[0], (double)xyz[1], (double)xyz[2]}, n[3] = {0, 0, 1};
      bg_make_sel(c, n, sel[0]);
      ns = cf.proj_num >= 1 ? 1 : 0;
    } else {
      double ln[3] = {0, 0, 0};
      for (int i = 0; i < M && ns < cf.proj_num; i++) {
        const double *n = E[i].n;
        if (bg_norm(n[0] - ln[0], n[1] - ln[1], n[2] - ln[2]) < 0.3 || bg_norm(n[0] + ln[0], n[1] + ln[1], n[2] + ln[2]) > 0.3) {
          ln[0] = n[0]; ln[1] = n[1]; ln[2] = n[2];
          bg_make_sel(E[i].c, n, sel[ns]);
          ns++;
        }
      }
    }
    cnt[BGC_NSEL] = ns;
    for (int s = 0; s < BG_MAX_PROJ; s++) {
      cnt[BGC_KEPT0 + s] = 0;
      mm[4 * s] = bg_enc(10.0); mm[4 * s + 1] = bg_enc(-10.0); mm[4 * s + 2] = bg_enc(10.0); mm[4 * s + 3] = bg_enc(-10.0);
    }
  }
}

// ---------------------------------------------------------------- extract_binary (BTC.cpp:488-797), projection plane s
__global__ void k_bg_proj(int n, const float *xyz, const BgCfg cf, const BgSel *sel, int s, int *cnt, unsigned long long *mm, double *px,
                          double *py, double *pd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cnt[BGC_NSEL] || i >= n) return;
  const BgSel &S = sel[s];
  const double A = S.A, B = S.B, C = S.C, D = S.D;
  const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  const double dis = fabs(x * A + y * B + z * C + D);
  const bool keep = !(dis < cf.dmin || dis > cf.dmax);
  double X = 0, Y = 0;
  if (keep) {
    const double den = A * A + B * B + C * C;
    const double p0 = (-A * (B * y + C * z + D) + x * (B * B + C * C)) / den;
    const double p1 = (-B * (A * x + C * z + D) + y * (A * A + C * C)) / den;
    const double p2 = (-C * (A * x + B * y + D) + z * (A * A + B * B)) / den;
    X = p0 * S.ya[0] + p1 * S.ya[1] + p2 * S.ya[2] + S.dy;
    Y = p0 * S.xa[0] + p1 * S.xa[1] + p2 * S.xa[2] + S.dx;
    atomicAdd(cnt + BGC_KEPT0 + s, 1);
    atomicMin(mm + 4 * s, bg_enc(X)); atomicMax(mm + 4 * s + 1, bg_enc(X));
    atomicMin(mm + 4 * s + 2, bg_enc(Y)); atomicMax(mm + 4 * s + 3, bg_enc(Y));
  }
  px[i] = X; py[i] = Y; pd[i] = keep ? dis : -1.0;
}

struct BgImg { double minx, miny; int xlen, ylen, xseg, yseg; long long cells; bool live; };
__device__ __forceinline__ BgImg bg_img(const BgCfg &cf, const int *cnt, const unsigned long long *mm, int s) {
  BgImg g;
  g.live = s < cnt[BGC_NSEL] && cnt[BGC_KEPT0 + s] > 5;
  g.minx = bg_dec(mm[4 * s]); g.miny = bg_dec(mm[4 * s + 2]);
  const double W = bg_dec(mm[4 * s + 1]) - g.minx, H = bg_dec(mm[4 * s + 3]) - g.miny;
  const double seg = 5 * cf.res;
  if (!(W / cf.res < 1e8 && H / cf.res < 1e8)) { g.cells = LLONG_MAX; g.xlen = g.ylen = g.xseg = g.yseg = 0; return g; }
  g.xseg = (int)(W / seg + 1); g.yseg = (int)(H / seg + 1);
  g.xlen = (int)(W / cf.res + 5); g.ylen = (int)(H / cf.res + 5);
  g.cells = (long long)g.xlen * g.ylen;
  return g;
}

__global__ void k_bg_cellkey(int n, const BgCfg cf, int s, int *cnt, const unsigned long long *mm, const double *px, const double *py,
                             const double *pd, long long cap, unsigned *key, int *idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const BgImg g = bg_img(cf, cnt, mm, s);
  if (i == 0 && s < cnt[BGC_NSEL] && cnt[BGC_KEPT0 + s] > 5) {
    if (g.cells > cap) {                                 // 2: grow the image and run again; 4: beyond BG_MAX_CELLS, refused
      atomicOr(cnt + BGC_ERR, g.cells > (long long)BG_MAX_CELLS ? 4 : 2);
      atomicMax(cnt + BGC_CELLS, g.cells > INT_MAX ? INT_MAX : (int)g.cells);
    }
  }
  if (!g.live || g.cells > cap || i >= n) return;
  unsigned k = 0xffffffffu;
  if (pd[i] >= 0) {
    const int xi = (int)((px[i] - g.minx) / cf.res), yi = (int)((py[i] - g.miny) / cf.res);
    k = (unsigned)xi * (unsigned)g.ylen + (unsigned)yi;
  }
  key[i] = k; idx[i] = i;
}

__global__ void k_bg_cellzero(const BgCfg cf, int s, const int *cnt, const unsigned long long *mm, long long cap, int *ccnt, int *cdis) {
  const BgImg g = bg_img(cf, cnt, mm, s);
  if (!g.live || g.cells > cap) return;
  for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < g.cells; c += (long long)gridDim.x * blockDim.x) { ccnt[c] = 0; cdis[c] = 0; }
}

// per occupied cell (its head in cell order): count, sums of the kept points in input order, occupancy bits, summary
__global__ void k_bg_cells(int n, const BgCfg cf, int s, const int *cnt, const unsigned long long *mm, long long cap, const unsigned *skey,
                           const int *sidx, const double *px, const double *py, const double *pd, int *ccnt, int *cdis, double *csx,
                           double *csy, unsigned long long *cbits) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const BgImg g = bg_img(cf, cnt, mm, s);
  if (!g.live || g.cells > cap || j >= n) return;
  const unsigned k = skey[j];
  if (k == 0xffffffffu || !(j == 0 || skey[j - 1] != k)) return;
  double sx = 0, sy = 0;
  int c = 0;
  unsigned long long bits = 0;
  for (int e = j; e < n && skey[e] == k; e++) {
    const int i = sidx[e];
    sx += px[i]; sy += py[i]; c++;
    const int ci = (int)((pd[i] - cf.dmin) / cf.high_inc);
    if (ci < cf.cut_num) bits |= 1ull << ci;             // ci == cut_num near proj_dis_max: counted, but no occupancy bit
  }
  ccnt[k] = c; csx[k] = sx; csy[k] = sy; cbits[k] = bits; cdis[k] = __popcll(bits);
}

// segment maxima, touch and line filters; corners appended in (x segment, y segment) order
__global__ __launch_bounds__(1024) void k_bg_segments(const BgCfg cf, int s, int *cnt, const unsigned long long *mm, long long cap,
                                                      const BgSel *sel, const int *ccnt, const int *cdis, const double *csx,
                                                      const double *csy, const unsigned long long *cbits, BgCorner *corn, int corn_cap) {
  __shared__ int sh[16];
  const BgImg g = bg_img(cf, cnt, mm, s);
  if (!g.live || g.cells > cap) return;
  const BgSel &S = sel[s];
  const int tid = threadIdx.x;
  const int base0 = cnt[BGC_NTEMP];
  __syncthreads();
  const long long nseg = (long long)g.xseg * g.yseg;
  int base = base0;
  auto dis = [&](int x, int y) -> double { return (x < g.xlen && y < g.ylen) ? (double)cdis[(long long)x * g.ylen + y] : 0.0; };
  for (long long c0 = 0; c0 < nseg; c0 += blockDim.x) {
    const long long q = c0 + tid;
    bool add = false;
    int bx = 0, by = 0;
    if (q < nseg) {
      const int xs = (int)(q / g.yseg), ys = (int)(q % g.yseg);
      double md = 0;
      bx = -10; by = -10;
      for (int x = xs * 5; x < (xs + 1) * 5; x++)
        for (int y = ys * 5; y < (ys + 1) * 5; y++) { const double v = dis(x, y); if (v > md) { md = v; bx = x; by = y; } }
      if (md >= cf.summ_min) {
        add = !(bx <= 0 || bx >= g.xlen - 1 || by <= 0 || by >= g.ylen - 1);   // (checked first: bx = -10 when nothing beat 0)
        if (add && cf.touch_filter) add = (cbits[(long long)bx * g.ylen + by] & 0xfull) != 0;
        if (add && cf.line_filter) {
          const int dr[4][2] = {{0, 1}, {1, 0}, {1, 1}, {1, -1}};
          const double v = dis(bx, by);
          for (int d = 0; d < 4; d++) {
            const double v1 = dis(bx + dr[d][0], by + dr[d][1]), v2 = dis(bx - dr[d][0], by - dr[d][1]);
            const double thr = v - 3;
            if (v1 >= thr && v2 >= 0.5 * v) add = false;
            if (v2 >= thr && v1 >= 0.5 * v) add = false;
            if (v1 >= thr && v2 >= thr) add = false;
            if (v2 >= thr && v1 >= thr) add = false;
          }
        }
      }
    }
    int tot;
    const int r = bg_block_rank(add, sh, tot);
    if (add && base + r < corn_cap) {
      const long long c = (long long)bx * g.ylen + by;
      const double cn = (double)ccnt[c];
      const double pxv = csx[c] / cn, pyv = csy[c] / cn;
      BgCorner o;
      for (int k = 0; k < 3; k++) o.loc[k] = pyv * S.xa[k] + pxv * S.ya[k] + S.c[k];
      o.bits = cbits[c]; o.summ = cdis[c]; o.pad = 0;
      corn[base + r] = o;
    }
    base += tot;
  }
  if (tid == 0) cnt[BGC_NTEMP] = base;
}

// ---------------------------------------------------------------- non_maxi_suppression + top-N (BTC.cpp:472-483, :799-846)
__global__ __launch_bounds__(1024) void k_bg_corners(const BgCfg cf, int *cnt, const BgCorner *tmp, int corn_cap, BgCorner *pass,
                                                     BgCorner *out) {
  __shared__ int sh[16];
  const int tid = threadIdx.x;
  const int C = cnt[BGC_NTEMP];
  if (C > corn_cap) return;                               // overflow: the host grows the list and runs the call again
  int base = 0;
  for (int c0 = 0; c0 < C; c0 += blockDim.x) {
    const int i = c0 + tid;
    bool keep = false;
    if (i < C) {
      keep = true;
      const float xi = (float)tmp[i].loc[0], yi = (float)tmp[i].loc[1], zi = (float)tmp[i].loc[2];
      const int si = tmp[i].summ;
      for (int j = 0; j < C; j++) {
        if (j == i) continue;
        const float dx = xi - (float)tmp[j].loc[0], dy = yi - (float)tmp[j].loc[1], dz = zi - (float)tmp[j].loc[2];
        const float d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < cf.nms_r2 && si <= tmp[j].summ) { keep = false; break; }
      }
    }
    int tot;
    const int r = bg_block_rank(keep, sh, tot);
    if (keep) pass[base + r] = tmp[i];
    base += tot;
  }
  __syncthreads();
  const int Np = base;
  if (cf.useful > Np) {
    for (int i = tid; i < Np; i += blockDim.x) out[i] = pass[i];
    if (tid == 0) cnt[BGC_NCORN] = Np;
  } else {                                                // stable std::sort(binary_greater_sort), first useful_corner_num
    for (int i = tid; i < Np; i += blockDim.x) {
      const int si = pass[i].summ;
      int r = 0;
      for (int j = 0; j < Np; j++) { const int sj = pass[j].summ; r += (sj > si || (sj == si && j < i)) ? 1 : 0; }
      if (r < cf.useful) out[r] = pass[i];
    }
    if (tid == 0) cnt[BGC_NCORN] = cf.useful;
  }
}

// ---------------------------------------------------------------- generate_std (BTC.cpp:848-985)
__device__ __forceinline__ unsigned bg_hash64(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return (unsigned)k;
}

__global__ __launch_bounds__(1024) void k_bg_std(const BgCfg cf, int *cnt, const BgCorner *cr, BgStd *cand, unsigned long long *ckeys,
                                                 int *cslot, unsigned long long *htab, int *hmin, int hsize, BgStd *out) {
  __shared__ int sh[16];
  const int tid = threadIdx.x;
  const int N = cnt[BGC_NCORN];
  const int Kf = cf.K < N ? cf.K : N;
  const int T = Kf >= 3 ? (Kf - 1) * (Kf - 2) / 2 : 0;
  const int E = N * T;
  for (int h = tid; h < hsize; h += blockDim.x) { htab[h] = BG_EMPTY; hmin[h] = INT_MAX; }
  __syncthreads();
  for (int i = tid; i < N; i += blockDim.x) {
    const float qx = (float)cr[i].loc[0], qy = (float)cr[i].loc[1], qz = (float)cr[i].loc[2];
    int nb[BG_MAX_K]; float nd[BG_MAX_K];
    int have = 0;
    for (int j = 0; j < N; j++) {                         // exact kNN: (d^2, index) ascending
      const float dx = qx - (float)cr[j].loc[0], dy = qy - (float)cr[j].loc[1], dz = qz - (float)cr[j].loc[2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (have == Kf && !(d2 < nd[Kf - 1])) continue;
      int p = have < Kf ? have : Kf - 1;
      while (p > 0 && d2 < nd[p - 1]) { if (p < Kf) { nd[p] = nd[p - 1]; nb[p] = nb[p - 1]; } p--; }
      nd[p] = d2; nb[p] = j;
      if (have < Kf) have++;
    }
    int t = 0;
    for (int m = 1; m < Kf - 1; m++)
      for (int nn = m + 1; nn < Kf; nn++, t++) {
        const int e = i * T + t;
        ckeys[e] = BG_EMPTY;
        const int ci[3] = {i, nb[m], nb[nn]};
        float P[3][3];
        for (int v = 0; v < 3; v++) for (int k = 0; k < 3; k++) P[v][k] = (float)cr[ci[v]].loc[k];
        const float a0 = P[0][0] - P[1][0], a1 = P[0][1] - P[1][1], a2 = P[0][2] - P[1][2];
        const float b0 = P[0][0] - P[2][0], b1 = P[0][1] - P[2][1], b2 = P[0][2] - P[2][2];
        const float c0 = P[2][0] - P[1][0], c1 = P[2][1] - P[1][1], c2 = P[2][2] - P[1][2];
        double a = sqrt((double)a0 * (double)a0 + (double)a1 * (double)a1 + (double)a2 * (double)a2);
        double b = sqrt((double)b0 * (double)b0 + (double)b1 * (double)b1 + (double)b2 * (double)b2);
        double c = sqrt((double)c0 * (double)c0 + (double)c1 * (double)c1 + (double)c2 * (double)c2);
        if (a > cf.max_len || b > cf.max_len || c > cf.max_len || a < cf.min_len || b < cf.min_len || c < cf.min_len) continue;
        int l1[3] = {1, 2, 0}, l2[3] = {1, 0, 3}, l3[3] = {0, 2, 3}, lt[3];
        double tmp;
        if (a > b) { tmp = a; a = b; b = tmp; for (int k = 0; k < 3; k++) { lt[k] = l1[k]; l1[k] = l2[k]; l2[k] = lt[k]; } }
        if (b > c) { tmp = b; b = c; c = tmp; for (int k = 0; k < 3; k++) { lt[k] = l2[k]; l2[k] = l3[k]; l3[k] = lt[k]; } }
        if (a > b) { tmp = a; a = b; b = tmp; for (int k = 0; k < 3; k++) { lt[k] = l1[k]; l1[k] = l2[k]; l2[k] = lt[k]; } }
        if (fabs(c - (a + b)) < 0.2) continue;
        const long long kx = (long long)(float)(a * 1000), ky = (long long)(float)(b * 1000), kz = (long long)(float)(c * 1000);
        const int va = (l1[0] == l2[0]) ? 0 : ((l1[1] == l2[1]) ? 1 : 2);
        const int vb = (l1[0] == l3[0]) ? 0 : ((l1[1] == l3[1]) ? 1 : 2);
        const int vc = (l2[0] == l3[0]) ? 0 : ((l2[1] == l3[1]) ? 1 : 2);
        BgStd o;
        for (int k = 0; k < 3; k++) o.cen[k] = ((double)P[va][k] + (double)P[vb][k] + (double)P[vc][k]) / 3;
        o.tri[0] = cf.scale * a; o.tri[1] = cf.scale * b; o.tri[2] = cf.scale * c;
        o.a = ci[va]; o.b = ci[vb]; o.c = ci[vc]; o.pad = 0;
        cand[e] = o;
        ckeys[e] = ((unsigned long long)kx << 42) | ((unsigned long long)ky << 21) | (unsigned long long)kz;
      }
  }
  __syncthreads();
  for (int e = tid; e < E; e += blockDim.x) {             // first in emission order wins: atomicMin of e per key
    const unsigned long long k = ckeys[e];
    if (k == BG_EMPTY) continue;
    unsigned h = bg_hash64(k) & (unsigned)(hsize - 1);
    for (;;) {
      const unsigned long long prev = atomicCAS(htab + h, BG_EMPTY, k);
      if (prev == BG_EMPTY || prev == k) { atomicMin(hmin + h, e); cslot[e] = (int)h; break; }
      h = (h + 1) & (unsigned)(hsize - 1);
    }
  }
  __syncthreads();
  int base = 0;
  for (int c0 = 0; c0 < E; c0 += blockDim.x) {
    const int e = c0 + tid;
    const bool keep = e < E && ckeys[e] != BG_EMPTY && hmin[cslot[e]] == e;
    int tot;
    const int r = bg_block_rank(keep, sh, tot);
    if (keep) out[base + r] = cand[e];
    base += tot;
  }
  if (tid == 0) cnt[BGC_NSTD] = base;
}

// one array of a group: counted whether or not the allocation succeeds
template <class T>
hipError_t bg_grow(BtcGen &g, DevMem<T> &m, size_t n) {
  g.allocs++;
  g.dev_bytes += n * sizeof(T);
  return m.ensure(n);
}

#define BGCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return _e; } while (0)

// a capacity group goes from its old size to m: `cap` reads 0 while `grow` runs, and a failure empties the group (complete or empty)
template <class G, class F>
hipError_t bg_regroup(G &grp, size_t &cap, size_t m, F grow) {
  cap = 0;
  const hipError_t e = grow();
  if (e != hipSuccess) grp = G();
  else cap = m;
  return e;
}

}  // namespace

hipError_t btcgen_reserve(BtcGen &g, size_t n, size_t cells, size_t corners, size_t stds, int vinit, hipStream_t st) {
  if (n > g.pts_cap) {
    BGCHK(hipStreamSynchronize(st));
    size_t m = g.pts_cap ? g.pts_cap : 65536;
    while (m < n) m *= 2;
    BtcGen::Pts &p = g.pts;
    BGCHK(bg_regroup(p, g.pts_cap, m, [&]() -> hipError_t {
      BGCHK(bg_grow(g, p.xyz, 3 * m)); BGCHK(bg_grow(g, p.sxyz, 3 * m));
      BGCHK(bg_grow(g, p.key, m)); BGCHK(bg_grow(g, p.skey, m));
      BGCHK(bg_grow(g, p.idx, m)); BGCHK(bg_grow(g, p.sidx, m)); BGCHK(bg_grow(g, p.flag, m));
      BGCHK(bg_grow(g, p.ckey, m)); BGCHK(bg_grow(g, p.sckey, m));
      BGCHK(bg_grow(g, p.px, m)); BGCHK(bg_grow(g, p.py, m)); BGCHK(bg_grow(g, p.pd, m));
      BGCHK(bg_grow(g, p.vstart, m)); BGCHK(bg_grow(g, p.vlen, m)); BGCHK(bg_grow(g, p.isc, m + 1));
      size_t b1 = 0, b2 = 0;
      BGCHK(sort_pairs_u64(nullptr, b1, nullptr, nullptr, nullptr, nullptr, m, 3 * BG_KEY_BITS, st));
      BGCHK(sort_pairs_u32(nullptr, b2, nullptr, nullptr, nullptr, nullptr, m, 32u, st));
      g.sort_bytes = b1 > b2 ? b1 : b2;
      return bg_grow(g, p.sort_tmp, g.sort_bytes);
    }));
  }
  const size_t pc = g.pts_cap / (size_t)(vinit + 1) + 1;
  if (pc > g.plane_cap) {
    BGCHK(hipStreamSynchronize(st));
    BtcGen::Planes &p = g.pln;
    BGCHK(bg_regroup(p, g.plane_cap, pc, [&]() -> hipError_t {
      BGCHK(bg_grow(g, p.planes, 5 * pc * sizeof(BgPlane)));
      BGCHK(bg_grow(g, p.isp, pc + 1)); BGCHK(bg_grow(g, p.ids, pc)); BGCHK(bg_grow(g, p.ids2, pc + 1));
      return bg_grow(g, p.first, pc + 1);
    }));
  }
  if (!g.h_cnt) {
    BGCHK(bg_grow(g, g.cnt, BGC_N));
    BGCHK(bg_grow(g, g.mm, 4 * BG_MAX_PROJ));
    BGCHK(bg_grow(g, g.sel, BG_MAX_PROJ * sizeof(BgSel)));
    g.allocs++;
    BGCHK(g.h_cnt.ensure(BGC_N));
  }
  if (cells < 65536) cells = 65536;
  if (cells > g.cell_cap) {
    BGCHK(hipStreamSynchronize(st));
    size_t m = g.cell_cap ? g.cell_cap : 65536;
    while (m < cells) m *= 2;
    BtcGen::Cells &p = g.cel;
    BGCHK(bg_regroup(p, g.cell_cap, m, [&]() -> hipError_t {
      BGCHK(bg_grow(g, p.ccnt, m)); BGCHK(bg_grow(g, p.cdis, m)); BGCHK(bg_grow(g, p.csx, m)); BGCHK(bg_grow(g, p.csy, m));
      return bg_grow(g, p.cbits, m);
    }));
  }
  if (corners < 1024) corners = 1024;
  if (corners > g.corn_cap) {
    BGCHK(hipStreamSynchronize(st));
    size_t m = g.corn_cap ? g.corn_cap : 1024;
    while (m < corners) m *= 2;
    BtcGen::Corners &p = g.cor;
    BGCHK(bg_regroup(p, g.corn_cap, m, [&]() -> hipError_t {
      BGCHK(bg_grow(g, p.corn, m)); BGCHK(bg_grow(g, p.corn2, m)); BGCHK(bg_grow(g, p.corn3, m));
      g.allocs++;
      return p.h_corn.ensure(m);
    }));
  }
  if (stds < 1024) stds = 1024;
  if (stds > g.cand_cap) {
    BGCHK(hipStreamSynchronize(st));
    size_t m = g.cand_cap ? g.cand_cap : 1024;
    while (m < stds) m *= 2;
    BtcGen::Cands &p = g.tri;
    BGCHK(bg_regroup(p, g.cand_cap, m, [&]() -> hipError_t {
      BGCHK(bg_grow(g, p.cand, m)); BGCHK(bg_grow(g, p.stds, m)); BGCHK(bg_grow(g, p.ckeys, m)); BGCHK(bg_grow(g, p.cslot, m));
      BGCHK(bg_grow(g, p.htab, 2 * m)); BGCHK(bg_grow(g, p.hmin, 2 * m));
      g.allocs++;
      return p.h_stds.ensure(m);
    }));
  }
  return hipSuccess;
}

hipError_t btcgen_enqueue(BtcGen &g, const BgCfg &cf, int n, const float *h_xyz, float *pc_dst, int *off_slot, int have, hipStream_t st) {
  const int nb = (n + 255) / 256;
  const size_t pc = g.plane_cap;
  BgPlane *cpl = (BgPlane *)g.pln.planes.p, *pl = cpl + pc, *grp = pl + pc, *srt = grp + pc, *mrg = srt + pc;
  BgPlane *fin = cpl;                                     // the candidates are dead once the planes are compacted
  BGCHK(hipMemsetAsync(g.cnt, 0, BGC_N * sizeof(int), st));
  if (h_xyz) BGCHK(hipMemcpyAsync(g.pts.xyz, h_xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, st));   // nullptr: g.pts.xyz was filled on the device
  // voxels
  k_bg_key<<<nb, 256, 0, st>>>(n, g.pts.xyz, cf.vsize, g.pts.key, g.pts.idx, g.cnt);
  size_t tb = g.sort_bytes;
  BGCHK(sort_pairs_u64(g.pts.sort_tmp, tb, g.pts.key, g.pts.skey, g.pts.idx, g.pts.sidx, (size_t)n, 3 * BG_KEY_BITS, st));
  BGCHK(hipMemsetAsync(g.pts.flag, 0, (size_t)n * sizeof(int), st));
  k_bg_gather<<<nb, 256, 0, st>>>(n, g.pts.xyz, g.pts.skey, g.pts.sidx, g.pts.sxyz, g.pts.flag);
  k_bg_scan<<<1, 1024, 0, st>>>(g.pts.flag, nullptr, n, g.cnt + BGC_NVOX);
  k_bg_runs<<<nb, 256, 0, st>>>(n, g.pts.skey, g.pts.sidx, g.pts.flag, cf.vinit, g.pts.vstart, g.pts.vlen, g.pts.isc);
  // candidate voxels (> voxel_init_num points) -> candidate index in voxel order; fits; planes -> plane index
  BGCHK(hipMemcpyAsync(g.pts.flag, g.pts.isc, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
  k_bg_scan<<<1, 1024, 0, st>>>(g.pts.flag, g.cnt + BGC_NVOX, n, g.cnt + BGC_NCAND);
  k_bg_fit<<<nb, 256, 0, st>>>(g.cnt, g.pts.sxyz, g.pts.vstart, g.pts.vlen, g.pts.isc, g.pts.flag, cf.detect, cpl, g.pln.isp);
  const int npc = (int)pc;
  BGCHK(hipMemcpyAsync(g.pln.ids2, g.pln.isp, pc * sizeof(int), hipMemcpyDeviceToDevice, st));
  k_bg_scan<<<1, 1024, 0, st>>>(g.pln.ids2, g.cnt + BGC_NCAND, npc, g.cnt + BGC_NPL);
  k_bg_planes<<<(npc + 255) / 256, 256, 0, st>>>(g.cnt, cpl, g.pln.isp, g.pln.ids2, pl, pc_dst, off_slot, have);
  // projection planes
  BgSel *sel = (BgSel *)g.sel.p;
  k_bg_select<<<1, 1024, 0, st>>>(cf, g.pts.xyz, g.cnt, pl, grp, srt, mrg, fin, g.pln.ids, g.pln.first, sel, g.mm);
  // extract_binary for each selected plane (launches of planes beyond the selection return at once)
  const long long ccap = (long long)g.cell_cap;
  for (int s = 0; s < cf.proj_num; s++) {
    k_bg_proj<<<nb, 256, 0, st>>>(n, g.pts.xyz, cf, sel, s, g.cnt, g.mm, g.pts.px, g.pts.py, g.pts.pd);
    k_bg_cellkey<<<nb, 256, 0, st>>>(n, cf, s, g.cnt, g.mm, g.pts.px, g.pts.py, g.pts.pd, ccap, g.pts.ckey, g.pts.idx);
    tb = g.sort_bytes;
    BGCHK(sort_pairs_u32(g.pts.sort_tmp, tb, g.pts.ckey, g.pts.sckey, g.pts.idx, g.pts.sidx, (size_t)n, 32u, st));
    k_bg_cellzero<<<1024, 256, 0, st>>>(cf, s, g.cnt, g.mm, ccap, g.cel.ccnt, g.cel.cdis);
    k_bg_cells<<<nb, 256, 0, st>>>(n, cf, s, g.cnt, g.mm, ccap, g.pts.sckey, g.pts.sidx, g.pts.px, g.pts.py, g.pts.pd, g.cel.ccnt, g.cel.cdis, g.cel.csx, g.cel.csy, g.cel.cbits);
    k_bg_segments<<<1, 1024, 0, st>>>(cf, s, g.cnt, g.mm, ccap, sel, g.cel.ccnt, g.cel.cdis, g.cel.csx, g.cel.csy, g.cel.cbits, g.cor.corn, (int)g.corn_cap);
  }
  k_bg_corners<<<1, 1024, 0, st>>>(cf, g.cnt, g.cor.corn, (int)g.corn_cap, g.cor.corn2, g.cor.corn3);
  const int hs = (int)(2 * g.cand_cap);
  k_bg_std<<<1, 1024, 0, st>>>(cf, g.cnt, g.cor.corn3, g.tri.cand, g.tri.ckeys, g.tri.cslot, g.tri.htab, g.tri.hmin, hs, g.tri.stds);
  BGCHK(hipGetLastError());
  // read-back: counters, every triangle slot the configuration allows, the final corners
  const size_t K1 = (size_t)(cf.K - 1);
  size_t maxstd = (size_t)cf.useful * (K1 * (K1 - 1) / 2);
  if (maxstd > g.cand_cap) maxstd = g.cand_cap;
  size_t maxc = (size_t)cf.useful < g.corn_cap ? (size_t)cf.useful : g.corn_cap;
  BGCHK(hipMemcpyAsync(g.h_cnt, g.cnt, BGC_N * sizeof(int), hipMemcpyDeviceToHost, st));
  if (maxstd) BGCHK(hipMemcpyAsync(g.tri.h_stds, g.tri.stds, maxstd * sizeof(BgStd), hipMemcpyDeviceToHost, st));
  if (maxc) BGCHK(hipMemcpyAsync(g.cor.h_corn, g.cor.corn3, maxc * sizeof(BgCorner), hipMemcpyDeviceToHost, st));
  return hipSuccess;
}

}  // namespace vba
