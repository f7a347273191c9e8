// Loop retrieval and verification of the loop-closure thread (BTC.cpp, loop_refine.hpp): STDescManager::SearchLoop
// (BTC.cpp:205-256) with candidate_selector (1128-1279), candidate_verify (1281-1396), triangle_solver (1398-1420) and
// plane_geometric_verify (1422-1479), and icp_normal (loop_refine.hpp:47-139).  Layout, order contract and measured figures:
// DESIGN.md §11.
//
// Database (one per STDescManager, append-only, HBM): descriptor rows SoA; a cell index keyed by STD_LOC (open addressing,
// 8 ints per slot: x, y, z, first chunk, count, last chunk) whose cells list their descriptors in insertion order in chunks of 64
// (one wave reads one chunk); plane clouds as float[6] per point with an offset table.  The host keeps the mirror of the cell
// table and tells the device which chunk slots, chunk links and table slots a batch of new descriptors writes, so add_stds costs
// O(new descriptors).
//
// Order contract: the match list is written by a stable compaction (count / k_det_scan / ballot rank) in the reference's order
// (query i, then the 27 cell offsets in voxel_round order, then the position inside the cell); votes are integer counts;
// candidates are taken by (votes desc, frame asc).  Nothing here adds floating point with atomics: every result is the same bits
// in every run.
#pragma once
#include <hip/hip_runtime.h>
#include "vba_hostmath.hpp"
#include "vba_ldlt6.hpp"
#include "vba_types.hpp"
#include "vba_common.hpp"
#include "vba_btc_svd.hpp"
#include "vba_icp_math.hpp"

namespace vba {

constexpr int BTC_CHUNK = 64;        // cell entries per chunk
constexpr int BTC_MAX_CAND = 256;    // upper bound of candidate_num_
constexpr int BTC_SAMPLES = 50;      // use_size <= 50 (skip_len = size / 50 + 1)
constexpr int BTC_RES = 16;          // per-search result doubles: id, score, t[3], R[9], ncand, total matches

__host__ __device__ inline unsigned btc_hash(int x, int y, int z) {
  return ((unsigned)x * 73856093u) ^ ((unsigned)y * 19349663u) ^ ((unsigned)z * 83492791u);
}

__device__ __forceinline__ int btc_lookup(const BtcIndex &ix, int x, int y, int z) {
  unsigned s = btc_hash(x, y, z) & (unsigned)ix.mask;
  for (;;) {                                             // load factor <= 1/2: an empty slot ends every probe
    const int *e = ix.tab + 8 * (size_t)s;
    if (e[3] < 0) return -1;
    if (e[0] == x && e[1] == y && e[2] == z) return (int)s;
    s = (s + 1) & (unsigned)ix.mask;
  }
}

// binary_similarity (BTC.cpp:70-80): 2 popcount(a & b) / (sa + sb); 0/0 is NaN and never similar
__device__ __forceinline__ double btc_bsim(unsigned long long a, unsigned long long b, int sa, int sb) {
  BTC_NOCONTRACT
  return 2.0 * (double)__popcll(a & b) / (double)(sa + sb);
}

// candidate_selector, the search over the 27 cells around each query descriptor (BTC.cpp:1160-1224).  One wave per (query i,
// offset r); the wave walks the cell's chunks in order and ranks its matches by ballot.  COUNT: cnt[g] = matches of (i, r).
// !COUNT: cnt[] holds exclusive offsets (k_det_scan); the matches go to the list in order and vote for their frame.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_btc_match(int n, BtcStds q, BtcStds d, BtcIndex ix, BtcCfgDev cf, int *cnt, const int *total,
                                                   int mcap, int *mq, int *md, int *mf, int *votes) {
  BTC_NOCONTRACT
  const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= 27 * n) return;                               // (whole waves; no barrier below)
  if (!COUNT && *total > mcap) return;                   // list overflow: the host grows the list and searches again
  const int i = g / 27, r = g % 27;
  const double tx = q.tri[3 * i], ty = q.tri[3 * i + 1], tz = q.tri[3 * i + 2];
  const int px = (int)(tx + (double)(r / 9 - 1)), py = (int)(ty + (double)((r / 3) % 3 - 1)), pz = (int)(tz + (double)(r % 3 - 1));
  int found = 0;
  if (btc_norm3(tx - ((double)px + 0.5), ty - ((double)py + 0.5), tz - ((double)pz + 0.5)) < 1.5) {
    const int s = btc_lookup(ix, px, py, pz);
    if (s >= 0) {
      const double thr = btc_norm3(tx, ty, tz) * cf.rough;
      const int qf = q.frame[i];
      const unsigned long long qa = q.bits[3 * i], qb = q.bits[3 * i + 1], qc = q.bits[3 * i + 2];
      const int sa = q.summ[3 * i], sb = q.summ[3 * i + 1], sc = q.summ[3 * i + 2];
      const int count = ix.tab[8 * (size_t)s + 4];
      int base = COUNT ? 0 : cnt[g];
      for (int ch = ix.tab[8 * (size_t)s + 3], seen = 0; ch >= 0 && seen < count; ch = ix.next[ch], seen += BTC_CHUNK) {
        const int j = (seen + lane < count) ? ix.ent[(size_t)ch * BTC_CHUNK + lane] : -1;
        bool ok = false;
        int fj = 0;
        if (j >= 0) {
          fj = d.frame[j];
          if (qf - fj > cf.skip_near) {
            const double dis = btc_norm3(tx - d.tri[3 * (size_t)j], ty - d.tri[3 * (size_t)j + 1], tz - d.tri[3 * (size_t)j + 2]);
            if (dis < thr) {
              const double sim = (btc_bsim(qa, d.bits[3 * (size_t)j], sa, d.summ[3 * (size_t)j]) +
                                  btc_bsim(qb, d.bits[3 * (size_t)j + 1], sb, d.summ[3 * (size_t)j + 1]) +
                                  btc_bsim(qc, d.bits[3 * (size_t)j + 2], sc, d.summ[3 * (size_t)j + 2])) / 3;
              ok = sim > cf.sim;
            }
          }
        }
        const unsigned long long m = __ballot(ok);
        if (!COUNT && ok) {
          const int pos = base + found + __popcll(m & ((1ull << lane) - 1ull));
          mq[pos] = i; md[pos] = j; mf[pos] = fj;
          atomicAdd(&votes[fj], 1);                      // integer counts: the order of the adds does not matter
        }
        found += __popcll(m);
      }
    }
  }
  if (COUNT && lane == 0) cnt[g] = found;
}

// candidate list (BTC.cpp:1239-1277): up to candidate_num_ frames by (votes desc, frame asc) while votes >= 5 — what the repeated
// max_element + zeroing computes.  cand[c] = {frame, votes, offset of its pairs, -, -} (offsets: running sum of the votes, which
// equal the lengths of the match lists).  One workgroup of 256.
__global__ __launch_bounds__(256) void k_btc_select(int nframes, int cand_num, int mcap, const int *total, int *votes, int *cand, double *res) {
  __shared__ unsigned long long wbest[4];
  __shared__ int s_stop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nc = 0, off = 0;
  const bool overflow = *total > mcap;
  for (int c = 0; c < cand_num && !overflow && nframes > 0; c++) {
    unsigned long long best = 0;
    for (int f = tid; f < nframes; f += 256) {
      const unsigned long long key = ((unsigned long long)(unsigned)votes[f] << 32) | (0xFFFFFFFFu - (unsigned)f);
      best = key > best ? key : best;
    }
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(best, m, 64); best = o > best ? o : best; }
    if (lane == 0) wbest[wave] = best;
    __syncthreads();
    if (tid == 0) {
      unsigned long long b = wbest[0];
      for (int w = 1; w < 4; w++) b = wbest[w] > b ? wbest[w] : b;
      const int v = (int)(b >> 32), f = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull));
      s_stop = v < 5;
      if (v >= 5) {
        cand[5 * c] = f; cand[5 * c + 1] = v; cand[5 * c + 2] = off; cand[5 * c + 3] = 0; cand[5 * c + 4] = 0;
        votes[f] = 0;
      }
      off += v;
    }
    __syncthreads();
    if (s_stop) break;
    nc++;
  }
  if (tid == 0) {
    res[14] = (double)nc;
    res[15] = (double)*total;
  }
}

// triangle_solver (BTC.cpp:1398-1420): rot = V U^T of the SVD of src ref^T (det < 0: V diag(1,1,-1) U^T), t = -rot c1 + c2.  The SVD
// restates Eigen's JacobiSVD for a square 3x3 (no QR preconditioner): two-sided Jacobi sweeps of real_2x2_jacobi_svd, signs fixed
// on U, singular values sorted descending with the columns of U and V.  src ref^T has rank <= 2 (a triangle minus its centroid),
// and V U^T with the determinant fixed is the same rotation whatever sign the third singular vectors take.
// pair (query row a of q, database row b of d) -> (R row-major, t)
__device__ inline void btc_triangle_solver(const BtcStds &q, int a, const BtcStds &d, int b, double *R, double *t) {
  BTC_NOCONTRACT
  double src[9], ref[9];   // columns = A, B, C minus the centre
  for (int v = 0; v < 3; v++)
    for (int k = 0; k < 3; k++) {
      src[3 * k + v] = q.loc[9 * (size_t)a + 3 * v + k] - q.cen[3 * (size_t)a + k];
      ref[3 * k + v] = d.loc[9 * (size_t)b + 3 * v + k] - d.cen[3 * (size_t)b + k];
    }
  double cov[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) cov[3 * r + c] = (src[3 * r] * ref[3 * c] + src[3 * r + 1] * ref[3 * c + 1]) + src[3 * r + 2] * ref[3 * c + 2];
  double U[9], S[3], V[9];
  btc_svd3(cov, U, S, V);
  btc_kabsch(U, V, R);
  const double *c1 = q.cen + 3 * (size_t)a, *c2 = d.cen + 3 * (size_t)b;
  for (int r = 0; r < 3; r++) t[r] = -((R[3 * r] * c1[0] + R[3 * r + 1] * c1[1]) + R[3 * r + 2] * c1[2]) + c2[r];
}

// exact 1-NN of one query point over a cloud streamed through LDS (kd_match_body's conventions: squared L2 in float, x then y then
// z; the key (distance bits << 32 | index) orders by distance, then index).  Every thread of the workgroup must call it.
__device__ __forceinline__ unsigned long long btc_nn_tile(float qx, float qy, float qz, const float *cl, int lo, int hi, float *tx, float *ty, float *tz) {
  BTC_NOCONTRACT
  unsigned long long best = ~0ull;
  for (int base = lo; base < hi; base += 256) {
    const int j = base + (int)threadIdx.x;
    __syncthreads();
    if (j < hi) { tx[threadIdx.x] = cl[6 * (size_t)j]; ty[threadIdx.x] = cl[6 * (size_t)j + 1]; tz[threadIdx.x] = cl[6 * (size_t)j + 2]; }
    __syncthreads();
    const int cnt = (hi - base < 256) ? hi - base : 256;
    float bd = 3.4e38f; int bi = -1;
    for (int k = 0; k < cnt; k++) {
      const float dx = qx - tx[k], dy = qy - ty[k], dz = qz - tz[k];
      float dd = dx * dx; dd += dy * dy; dd += dz * dz;
      if (dd < bd) { bd = dd; bi = base + k - lo; }
    }
    if (bi >= 0) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(bd) << 32) | (unsigned)bi;
      best = key < best ? key : best;
    }
  }
  return best;
}

// candidate_verify + plane_geometric_verify (BTC.cpp:1281-1396, 1422-1479), one workgroup per candidate: gather the candidate's
// pairs in match-list order, solve the sampled pairs, vote over all pairs (first strict maximum), max_vote >= 4, then the 1-NN
// plane check of pl_cur (query cloud) against the candidate's cloud.  cres[c] = {score, t[3], R[9]}.
__global__ __launch_bounds__(256) void k_btc_verify(BtcStds q, BtcStds d, BtcCfgDev cf, const int *total_p, int mcap, const int *mq, const int *md,
                                                    const int *mf, int *pq, int *pd, int *cand, const double *res, double *cres,
                                                    const float *pl_cur, int n_cur, const float *pc, const int *pc_off) {
  BTC_NOCONTRACT
  __shared__ int wsum[4];
  __shared__ double sR[BTC_SAMPLES][12];
  __shared__ int svote[BTC_SAMPLES];
  __shared__ float tx[256], ty[256], tz[256];
  __shared__ int s_best;
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (c >= (int)res[14]) return;
  const int total = *total_p, frame = cand[5 * c], size = cand[5 * c + 1], off = cand[5 * c + 2];
  // 1. this candidate's pairs, in list order (stable compaction)
  int run = 0;
  for (int b = 0; b < total; b += 256) {
    const int k = b + tid;
    const bool f = k < total && mf[k] == frame;
    int tot;
    const int rk = wg_rank(f, wsum, tot);
    if (f) { pq[off + run + rk] = mq[k]; pd[off + run + rk] = md[k]; }
    run += tot;
    __syncthreads();
  }
  __syncthreads();
  const int *P = pq + off, *D = pd + off;
  // 2. sampled transforms
  const int skip = size / 50 + 1, use = size / skip;
  if (tid < use) btc_triangle_solver(q, P[tid * skip], d, D[tid * skip], sR[tid], sR[tid] + 9);
  __syncthreads();
  // 3. votes over all pairs: wave w takes samples w, w + 4, ...
  for (int s = wave; s < use; s += 4) {
    const double *R = sR[s], *t = sR[s] + 9;
    int v = 0;
    for (int j0 = 0; j0 < size; j0 += 64) {
      const int j = j0 + lane;
      bool ok = false;
      if (j < size) {
        ok = true;
        for (int e = 0; e < 3 && ok; e++) {
          const double *a = q.loc + 9 * (size_t)P[j] + 3 * e, *bb = d.loc + 9 * (size_t)D[j] + 3 * e;
          const double x = ((R[0] * a[0] + R[1] * a[1]) + R[2] * a[2]) + t[0];
          const double y = ((R[3] * a[0] + R[4] * a[1]) + R[5] * a[2]) + t[1];
          const double z = ((R[6] * a[0] + R[7] * a[1]) + R[8] * a[2]) + t[2];
          ok = btc_norm3(x - bb[0], y - bb[1], z - bb[2]) < 3.0;
        }
      }
      v += __popcll(__ballot(ok));
    }
    if (lane == 0) svote[s] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int mv = 0, mi = 0;
    for (int s = 0; s < use; s++) if (mv < svote[s]) { mv = svote[s]; mi = s; }
    cand[5 * c + 3] = mi; cand[5 * c + 4] = mv;
    s_best = mv >= 4 ? mi : -1;
  }
  __syncthreads();
  double *o = cres + 13 * (size_t)c;
  const int bs = s_best;
  if (bs < 0) {
    if (tid == 0) { o[0] = -1.0; for (int k = 0; k < 12; k++) o[1 + k] = 0.0; }
    return;
  }
  // 4. plane_geometric_verify(pl_cur, plane_cloud_vec_[frame], (t, R))
  const double *R = sR[bs], *t = sR[bs] + 9;
  const int lo = pc_off[frame], hi = pc_off[frame + 1];
  int useful = 0;
  for (int sb = 0; sb < n_cur; sb += 256) {
    const int i = sb + tid;
    double pi[3] = {0, 0, 0}, ni[3] = {0, 0, 0};
    float qx = 0, qy = 0, qz = 0;
    if (i < n_cur) {
      const float *p = pl_cur + 6 * (size_t)i;
      const double px = p[0], py = p[1], pz = p[2], nx = p[3], ny = p[4], nz = p[5];
      for (int r = 0; r < 3; r++) {
        pi[r] = ((R[3 * r] * px + R[3 * r + 1] * py) + R[3 * r + 2] * pz) + t[r];
        ni[r] = (R[3 * r] * nx + R[3 * r + 1] * ny) + R[3 * r + 2] * nz;
      }
      qx = (float)pi[0]; qy = (float)pi[1]; qz = (float)pi[2];
    }
    const unsigned long long key = btc_nn_tile(qx, qy, qz, pc, lo, hi, tx, ty, tz);
    if (i < n_cur && key != ~0ull) {
      const float *tp = pc + 6 * ((size_t)lo + (unsigned)(key & 0xFFFFFFFFull));
      const double tpx = tp[0], tpy = tp[1], tpz = tp[2], tnx = tp[3], tny = tp[4], tnz = tp[5];
      const double ninc = btc_norm3(ni[0] - tnx, ni[1] - tny, ni[2] - tnz), nadd = btc_norm3(ni[0] + tnx, ni[1] + tny, ni[2] + tnz);
      const double p2p = fabs((tnx * (pi[0] - tpx) + tny * (pi[1] - tpy)) + tnz * (pi[2] - tpz));
      if ((ninc < cf.normal || nadd < cf.normal) && p2p < cf.dis) useful++;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) useful += __shfl_xor(useful, m, 64);
  __syncthreads();
  if (lane == 0) wsum[wave] = useful;
  __syncthreads();
  if (tid == 0) {
    const int cnt = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    o[0] = (double)cnt / (double)n_cur;                  // an empty pl_cur gives NaN, which never wins
    for (int k = 0; k < 9; k++) o[4 + k] = R[k];
    for (int k = 0; k < 3; k++) o[1 + k] = t[k];
  }
}

// SearchLoop's choice (BTC.cpp:222-255): the first strict maximum of the scores above 0; a loop when it exceeds icp_threshold_
__global__ void k_btc_final(BtcCfgDev cf, const int *cand, const double *cres, double *res) {
  BTC_NOCONTRACT
  if (threadIdx.x != 0) return;
  const int nc = (int)res[14];
  double best = 0; int bc = -1;
  for (int c = 0; c < nc; c++) if (cres[13 * c] > best) { best = cres[13 * c]; bc = c; }
  const bool loop = bc >= 0 && best > cf.icp;
  res[0] = loop ? (double)cand[5 * bc] : -1.0;
  res[1] = loop ? best : 0.0;
  for (int k = 0; k < 12; k++) res[2 + k] = loop ? cres[13 * bc + 1 + k] : 0.0;
}

// appends to an int array: dst[pairs[2k]] = pairs[2k + 1]
__global__ void k_btc_scatter(int n, const int *pairs, int *dst) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) dst[pairs[2 * k]] = pairs[2 * k + 1];
}

// ------------------------------------------------------------------------------------------------ icp_normal (loop_refine.hpp:47-139)
// The per-point and per-step arithmetic is vba_icp_math.hpp (shared with the g++ build of the tests); the kernels below own the 1-NN
// search, the slice plan and the order of the sums.  The outputs marked "tap" are null in vba_btc_icp_normal and are what
// vba_debug_btc_icp_pass reads back.

// 1-NN of every transformed source point within one slice of the target (gridDim.y slices); key per (slice, point)
__global__ __launch_bounds__(256) void k_btc_icp_nn(int ns, const float *src, int nt, const float *tar, const BtcIcpDev *st, unsigned long long *key) {
  BTC_NOCONTRACT
  __shared__ float tx[256], ty[256], tz[256];
  if (st->done) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  float q[3] = {0, 0, 0};
  if (i < ns) btc_icp_query(st->R, st->t, src + 6 * (size_t)i, q);
  const int ntile = (nt + 255) / 256, per = (ntile + (int)gridDim.y - 1) / (int)gridDim.y;
  const int lo = (int)blockIdx.y * per * 256, hi = (lo + per * 256 < nt) ? lo + per * 256 : nt;
  unsigned long long b = btc_nn_tile(q[0], q[1], q[2], tar, lo < nt ? lo : nt, hi, tx, ty, tz);
  if (b != ~0ull) b += (unsigned)lo;                     // slice-local index -> cloud index (same distance bits)
  if (i < ns) key[(size_t)blockIdx.y * ns + i] = b;
}

// merge the slices, gate, accumulate the point-to-plane normal equations: per-workgroup partials [nb][35] (fixed tree).
// Taps: mkey[ns] the merged key, gate[ns] 1 where the point entered the sums.
__global__ __launch_bounds__(256) void k_btc_icp_accum(int ns, const float *src, const float *tar, int slices, const unsigned long long *key,
                                                      const BtcIcpDev *st, double *part, unsigned long long *mkey, unsigned char *gate) {
  BTC_NOCONTRACT
  __shared__ double red[4][BTC_ICP_PART];
  if (st->done) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s[BTC_ICP_PART];
#pragma unroll
  for (int k = 0; k < BTC_ICP_PART; k++) s[k] = 0.0;
  if (i < ns) {
    unsigned long long b = ~0ull;
    for (int sl = 0; sl < slices; sl++) { const unsigned long long k = key[(size_t)sl * ns + i]; b = k < b ? k : b; }
    bool pass = false;
    if (b != ~0ull) pass = btc_icp_point(st->R, st->t, st->paras, src + 6 * (size_t)i, tar + 6 * (size_t)(unsigned)(b & 0xFFFFFFFFull), s);
    if (mkey) mkey[i] = b;
    if (gate) gate[i] = pass ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < BTC_ICP_PART; k++) s[k] = wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < BTC_ICP_PART; k++) red[threadIdx.x >> 6][k] = s[k];
  __syncthreads();
  if (threadIdx.x < BTC_ICP_PART) part[(size_t)blockIdx.x * BTC_ICP_PART + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// reduce the partials (in workgroup order), solve Hess dxi = -JacT, update the pose, the convergence / parameter switch
// (loop_refine.hpp:115-134); after the last iteration the eigenvalues of mat_norm (loop_refine.hpp:135-137).
// Taps: sums[35] the reduced partials, dxo[6] the solved step.
__global__ __launch_bounds__(64) void k_btc_icp_step(int nb, const double *part, BtcIcpDev *st, double *sums, double *dxo) {
  BTC_NOCONTRACT
  __shared__ double acc[BTC_ICP_PART];
  if (st->done) return;
  const int tid = threadIdx.x;
  if (tid < BTC_ICP_PART) {
    double a = 0;
    for (int b = 0; b < nb; b++) a += part[(size_t)b * BTC_ICP_PART + tid];
    acc[tid] = a;
    if (sums) sums[tid] = a;
  }
  __syncthreads();
  if (tid != 0) return;
  double dx[6];
  btc_icp_solve_update(acc, st->R, st->t, st->mat, dx);
  if (dxo) for (int k = 0; k < 6; k++) dxo[k] = dx[k];
  btc_icp_transition(dx, st->paras, &st->is_conv, &st->done, &st->iters);
  if (st->done) {
    const double *m = st->mat;
    Eig3 e;
    if (!eig3_direct(m[0], m[1], m[2], m[3], m[4], m[5], e)) e = eig3_jacobi_dev(m[0], m[1], m[2], m[3], m[4], m[5]);
    st->eig[0] = e.w0; st->eig[1] = e.w1; st->eig[2] = e.w2;
  }
}

}  // namespace vba
