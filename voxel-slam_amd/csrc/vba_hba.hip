// libvoxelba.so: hierarchical global BA (vba_gba_build, vba_hba_add_edge, vba_hba_global).  The octree build and extraction of
// vba_kernels_gba.hpp, the any-window sparse path of vba_kernels_big.hpp (compiled here and nowhere else) and their host drivers; the
// fixed-window LM loop, the factor store and the exchange step are the BA core's (voxelba.hip), reached through the C ABI and vba_ctx.hpp.
#include "vba_ctx.hpp"
#include "vba_kernels_gba.hpp"
#include "vba_kernels_big.hpp"
#include "vba_hostmath.hpp"
#include "vba_hba_plan.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace vba {

// ---------------------------------------------------------------- host side of vba_kernels_gba.hpp: the octree of one window

// the view's pointers from the owners (null where a group is empty)
inline void gba_refresh(GbaStore &s) {
  GbaView &v = s.v;
  v.nadd = s.nodes.nadd; v.nlc = s.nodes.nlc; v.ncenter = s.nodes.ncenter; v.nql = s.nodes.nql; v.nchild = s.nodes.nchild; v.nfac = s.nodes.nfac;
  v.nlayer = s.nodes.nlayer; v.neval = s.nodes.neval; v.nevec = s.nodes.nevec;
  v.hkeys = s.hash.keys; v.hvals = s.hash.vals;
  v.pw = s.pts.pw; v.pl = s.pts.pl; v.pframe = s.pts.pframe; v.pnode = s.pts.pnode;
  v.cnt = s.cnt; v.poses = s.poses; v.offsets = s.offsets;
}

// The groups of GbaStore are re-allocated as a whole: the old group is freed first (its contents are not kept), and a group that
// could not be allocated completely is left empty with its capacity at 0, so that the next call allocates it again.
inline int gba_alloc_nodes(GbaStore &s, int cap, int W, std::string &err) {
  GbaStore::Nodes &m = s.nodes;
  m = GbaStore::Nodes(); s.v.cap = 0;
  const size_t cp = (size_t)cap;
  hipError_t alloc;
  if ((alloc = m.nadd.ensure(10 * cp)) || (alloc = m.nlc.ensure(10 * cp * W)) || (alloc = m.ncenter.ensure(3 * cp)) || (alloc = m.nql.ensure(cp)) || (alloc = m.nchild.ensure(cp)) ||
      (alloc = m.nfac.ensure(cp)) || (alloc = m.nlayer.ensure(cp)) || (alloc = m.neval.ensure(3 * cp)) || (alloc = m.nevec.ensure(9 * cp)))
    m = GbaStore::Nodes();
  gba_refresh(s);
  VBA_HIPCHK(err, alloc);
  s.v.cap = cap; s.v.W = W;
  return VBA_OK;
}

// Builds the octree of one keyframe window and leaves the planar voxels in device node storage; *n_factors = their count.
// pl may be a host or device pointer ([n][3] local points, keyframe i = rows offsets[i]..offsets[i+1]).
inline int gba_build(GbaStore &s, hipStream_t st, int W, const int *offsets, const double *pl, const double *poses, const GbaParams &P, int *n_factors,
                     std::string &err) {
  const int n = offsets[W];
  *n_factors = 0;
  hipError_t alloc;
  VBA_HIPCHK(err, s.h_cnt.ensure(GCNT_N));
  VBA_HIPCHK(err, s.cnt.ensure(GCNT_N));
  VBA_HIPCHK(err, s.poses.ensure(VBA_MAX_WIN * 12));
  VBA_HIPCHK(err, s.offsets.ensure(VBA_MAX_WIN + 1));
  if (n > s.cap_pts) {
    GbaStore::Pts &m = s.pts;
    m = GbaStore::Pts(); s.cap_pts = 0;
    const size_t c = (size_t)n + n / 4 + 1024;
    if ((alloc = m.pw.ensure(3 * c)) || (alloc = m.pframe.ensure(c)) || (alloc = m.pnode.ensure(c)) || (alloc = m.pl.ensure(3 * c))) { m = GbaStore::Pts(); gba_refresh(s); }
    VBA_HIPCHK(err, alloc);
    s.cap_pts = (int)c;
  }
  int hcap = 1 << 16;
  while (hcap < 2 * n && hcap < (1 << 28)) hcap <<= 1;
  if (hcap > s.cap_hash) {
    GbaStore::Hash &m = s.hash;
    m = GbaStore::Hash(); s.cap_hash = 0;
    if ((alloc = m.keys.ensure(hcap)) || (alloc = m.vals.ensure(hcap))) { m = GbaStore::Hash(); gba_refresh(s); }
    VBA_HIPCHK(err, alloc);
    s.cap_hash = hcap;
  }
  gba_refresh(s);
  s.v.hmask = (unsigned int)(s.cap_hash - 1);
  s.v.npts = n;
  VBA_HIPCHK(err, hipMemcpyAsync(s.pts.pl, pl, (size_t)n * 3 * 8, hipMemcpyDefault, st));
  VBA_HIPCHK(err, hipMemcpyAsync(s.v.poses, poses, (size_t)W * 12 * 8, hipMemcpyHostToDevice, st));
  VBA_HIPCHK(err, hipMemcpyAsync(s.v.offsets, offsets, (size_t)(W + 1) * 4, hipMemcpyHostToDevice, st));
  if (s.v.cap == 0 || s.v.W != W) { int r = gba_alloc_nodes(s, 1 << 17, W, err); if (r) return r; }
  const dim3 b(256), gp((n + 255) / 256);
  for (int attempt = 0; attempt < 8; attempt++) {
    const size_t cp = (size_t)s.v.cap;
    VBA_HIPCHK(err, hipMemsetAsync(s.v.cnt, 0, GCNT_N * sizeof(int), st));
    VBA_HIPCHK(err, hipMemsetAsync(s.v.hkeys, 0xFF, (size_t)s.cap_hash * 8, st));
    VBA_HIPCHK(err, hipMemsetAsync(s.v.nadd, 0, 10 * cp * 8, st));
    VBA_HIPCHK(err, hipMemsetAsync(s.v.nlc, 0, 10 * cp * W * 8, st));
    if (n > 0) {
      hipLaunchKernelGGL(k_gba_keys, gp, b, 0, st, s.v, P);
      hipLaunchKernelGGL(k_gba_roots, dim3((s.cap_hash + 4095) / 4096), b, 0, st, s.v, P);
      hipLaunchKernelGGL(k_gba_rootid, gp, b, 0, st, s.v);
      for (int L = 0; L <= P.max_layer; L++) {
        hipLaunchKernelGGL(k_gba_accum, gp, b, 0, st, s.v);
        hipLaunchKernelGGL(k_gba_decide, dim3((s.v.cap + 255) / 256), b, 0, st, s.v, P, L);
        if (L < P.max_layer) hipLaunchKernelGGL(k_gba_descend, gp, b, 0, st, s.v);
      }
    }
    VBA_HIPCHK(err, hipGetLastError());
    VBA_HIPCHK(err, hipStreamSynchronize(st));   // drain first (see map_read_counters)
    VBA_HIPCHK(err, hipMemcpyAsync(s.h_cnt, s.v.cnt, GCNT_N * sizeof(int), hipMemcpyDeviceToHost, st));
    VBA_HIPCHK(err, hipStreamSynchronize(st));
    if (s.h_cnt[GCNT_OVERFLOW] == 2) { err = "keyframe point outside the 21-bit voxel index range"; return VBA_ERR_CAPACITY; }
    if (!s.h_cnt[GCNT_OVERFLOW]) { *n_factors = s.h_cnt[GCNT_FACTORS]; return VBA_OK; }
    int want = s.v.cap * 2;
    while (want < s.h_cnt[GCNT_NODES] + 64) want *= 2;
    int r = gba_alloc_nodes(s, want, W, err);
    if (r) return r;
  }
  err = "octree node capacity";
  return VBA_ERR_CAPACITY;
}

// ---------------------------------------------------------------- host side of vba_kernels_big.hpp: the any-window sparse path

// The sparse factor store of W frames in the arena, in three steps with the producer's launches between them (big_build: the octree
// kernels; vba_debug_big_load: the caller's arrays).  1: the per-voxel arrays, H / g / r, the dense solver's buffers and NP / ld; vptr and
// d_fill are cleared.  2: the per-entry arrays, once E is known.  3: the (voxel, frame) -> entry map from evox / efr (k_big_eidx).
inline int big_store_voxels(BigStore &s, hipStream_t st, int W, int V, std::string &err) {
  auto al = [&](void **p, size_t bytes) { return s.arena(p, bytes); };
  BigView &b = s.b;
  b.W = W; b.V = V; b.capV = V > 0 ? V : 1;
  VBA_HIPCHK(err, al((void **)&b.vptr, (size_t)(V + 1) * 4)); VBA_HIPCHK(err, al((void **)&s.d_vcnt, (size_t)b.capV * 4)); VBA_HIPCHK(err, al((void **)&s.d_fill, (size_t)b.capV * 4));
  VBA_HIPCHK(err, al((void **)&b.eval, (size_t)b.capV * 3 * 8)); VBA_HIPCHK(err, al((void **)&b.evec, (size_t)b.capV * 9 * 8)); VBA_HIPCHK(err, al((void **)&b.pcr, (size_t)b.capV * 10 * 8));
  VBA_HIPCHK(err, al((void **)&b.poses, (size_t)W * 12 * 8));
  const size_t n6 = (size_t)6 * W;
  VBA_HIPCHK(err, al((void **)&b.H, n6 * n6 * 8)); VBA_HIPCHK(err, al((void **)&b.g, n6 * 8)); VBA_HIPCHK(err, al((void **)&b.r, 8));

  s.NP = (int)((n6 + 7) / 8 * 8); s.ld = (int)((s.NP + 63) / 64 * 64);
  VBA_HIPCHK(err, al((void **)&s.d_Ab, (size_t)(s.NP + 1) * s.ld * 8)); VBA_HIPCHK(err, al((void **)&s.d_Tb, (size_t)(s.NP + 1) * 8 * 8)); VBA_HIPCHK(err, al((void **)&s.d_ord, n6 * 4)); VBA_HIPCHK(err, al((void **)&s.d_vec, ((size_t)3 * n6 + (size_t)6 * W * W) * 8));
  VBA_HIPCHK(err, hipMemsetAsync(s.d_fill, 0, (size_t)b.capV * 4, st));
  VBA_HIPCHK(err, hipMemsetAsync(b.vptr, 0, (size_t)(V + 1) * 4, st));
  return VBA_OK;
}
inline int big_store_entries(BigStore &s, int E, std::string &err) {
  auto al = [&](void **p, size_t bytes) { return s.arena(p, bytes); };
  BigView &b = s.b;
  b.E = E; b.capE = E > 0 ? E : 1;
  VBA_HIPCHK(err, al((void **)&b.efr, (size_t)b.capE * 4)); VBA_HIPCHK(err, al((void **)&b.evox, (size_t)b.capE * 4));
  VBA_HIPCHK(err, al((void **)&b.ecl, (size_t)b.capE * 10 * 8)); VBA_HIPCHK(err, al((void **)&b.gv, (size_t)b.capE * 18 * 8)); VBA_HIPCHK(err, al((void **)&b.es, (size_t)b.capE * 27 * 8));
  return VBA_OK;
}
inline int big_store_eidx(BigStore &s, hipStream_t st, std::string &err) {
  BigView &b = s.b;
  VBA_HIPCHK(err, s.arena((void **)&b.eidx, (size_t)b.capV * b.W * 4));
  VBA_HIPCHK(err, hipMemsetAsync(b.eidx, 0xFF, (size_t)b.capV * b.W * 4, st));
  if (b.V > 0 && b.E > 0) {
    hipLaunchKernelGGL(k_big_eidx, dim3((b.E + 255) / 256), dim3(256), 0, st, b);
    VBA_HIPCHK(err, hipGetLastError());
  }
  return VBA_OK;
}

// Builds the octree of `W` keyframes and the sparse factor store (everything is re-allocated per call: the top-level BA
// runs once per loop closure).  pl: device pointer to the local points [n][3].
inline int big_build(BigStore &s, hipStream_t st, int W, const int *offsets, const double *d_pl, const double *poses, const GbaParams &P, std::string &err) {
  s.reset();
  const int n = offsets[W];
  auto al = [&](void **p, size_t bytes) { return s.arena(p, bytes); };
  VBA_HIPCHK(err, s.h_cnt.ensure(GCNT_N));
  GbaBigView &g = s.g;
  g.W = W; g.npts = n; g.pl = d_pl;
  unsigned int hcap = 1u << 16; while (hcap < 2u * (unsigned)n && hcap < (1u << 28)) hcap <<= 1;
  unsigned int ecap = 1u << 16;                         // (node, frame) pairs of ALL levels share the table: <= points per level
  while ((unsigned long long)ecap < 2ull * (unsigned long long)n * (unsigned)(P.max_layer + 1) && ecap < (1u << 30)) ecap <<= 1;
  g.hmask = hcap - 1; g.emask = ecap - 1;
  VBA_HIPCHK(err, al((void **)&g.hkeys, (size_t)hcap * 8)); VBA_HIPCHK(err, al((void **)&g.hvals, (size_t)hcap * 4));
  VBA_HIPCHK(err, al((void **)&g.ekeys, (size_t)ecap * 8)); VBA_HIPCHK(err, al((void **)&g.ecl, (size_t)ecap * 10 * 8));
  VBA_HIPCHK(err, al((void **)&g.pw, (size_t)n * 3 * 8)); VBA_HIPCHK(err, al((void **)&g.pframe, (size_t)n * 4)); VBA_HIPCHK(err, al((void **)&g.pnode, (size_t)n * 4));
  unsigned int *skey_b = nullptr; void *sort_tmp = nullptr; size_t sort_bytes = 0;
  VBA_HIPCHK(err, al((void **)&g.skey, (size_t)n * 4)); VBA_HIPCHK(err, al((void **)&skey_b, (size_t)n * 4)); VBA_HIPCHK(err, al((void **)&g.sval, (size_t)n * 4)); VBA_HIPCHK(err, al((void **)&g.perm, (size_t)n * 4));
  if (n > 0) {
    VBA_HIPCHK(err, sort_pairs_u32(nullptr, sort_bytes, g.skey, skey_b, g.sval, g.perm, (size_t)n, 32u, st));
    VBA_HIPCHK(err, al(&sort_tmp, sort_bytes + 256));
  }
  VBA_HIPCHK(err, al((void **)&g.cnt, GCNT_N * sizeof(int))); VBA_HIPCHK(err, al((void **)&g.poses, (size_t)W * 12 * 8)); VBA_HIPCHK(err, al((void **)&g.offsets, (size_t)(W + 1) * 4));
  VBA_HIPCHK(err, hipMemcpyAsync(g.poses, poses, (size_t)W * 12 * 8, hipMemcpyHostToDevice, st));
  VBA_HIPCHK(err, hipMemcpyAsync(g.offsets, offsets, (size_t)(W + 1) * 4, hipMemcpyHostToDevice, st));
  int cap = s.last_cap;                          // (the node capacity the previous build ended with: no doubling attempts, each of which re-clears the tables)
  const dim3 bk(256), gp((n + 255) / 256);
  for (int attempt = 0; attempt < 10; attempt++) {
    const size_t cp = (size_t)cap;
    g.cap = cap;
    void *tmp[9];
    size_t sz[9] = {10 * cp * 8, 3 * cp * 8, 3 * cp * 8, 9 * cp * 8, cp * 4, cp * 4, cp * 4, cp * 4, cp};
    for (int k = 0; k < 9; k++) { if (s.arena(&tmp[k], sz[k]) != hipSuccess) { err = "octree node storage"; return VBA_ERR_HIP; } }
    g.nadd = (double *)tmp[0]; g.ncenter = (double *)tmp[1]; g.neval = (double *)tmp[2]; g.nevec = (double *)tmp[3]; g.nql = (float *)tmp[4];
    g.nchild = (int *)tmp[5]; g.nfac = (int *)tmp[6]; g.nexi = (int *)tmp[7]; g.nlayer = (signed char *)tmp[8];
    VBA_HIPCHK(err, hipMemsetAsync(g.cnt, 0, GCNT_N * sizeof(int), st));
    VBA_HIPCHK(err, hipMemsetAsync(g.hkeys, 0xFF, (size_t)hcap * 8, st));
    VBA_HIPCHK(err, hipMemsetAsync(g.nadd, 0, 10 * cp * 8, st));
    VBA_HIPCHK(err, hipMemsetAsync(g.nexi, 0, cp * 4, st));
    if (n > 0) {
      hipLaunchKernelGGL(k_gbab_keys, gp, bk, 0, st, g, P);
      hipLaunchKernelGGL(k_gbab_roots, dim3((hcap + 4095) / 4096), bk, 0, st, g, P);
      hipLaunchKernelGGL(k_gbab_rootid, gp, bk, 0, st, g);
      {
        unsigned int bits = 1; while (bits < 32 && (1ull << bits) <= (unsigned long long)cap) bits++;     // keys are <= cap
        size_t tb = sort_bytes + 256;
        VBA_HIPCHK(err, sort_pairs_u32(sort_tmp, tb, g.skey, skey_b, g.sval, g.perm, (size_t)n, bits, st));
      }
      for (int L = 0; L <= P.max_layer; L++) {
        // entries of the previous level are dead: a planar node keeps its own entries (it stopped descending), so the
        // table is only cleared of nothing here — finished nodes never receive points again and their keys stay valid
        if (L == 0) {   // (a fill kernel: the runtime's memset moved the 5.4 GB of an 8 M-point window at 750 GB/s, 7.2 ms a time)
          hipLaunchKernelGGL(k_fill_u64, dim3(4096), dim3(256), 0, st, g.ekeys, ~0ull, (size_t)ecap);
          hipLaunchKernelGGL(k_fill_u64, dim3(4096), dim3(256), 0, st, (unsigned long long *)g.ecl, 0ull, (size_t)ecap * 10);
        }
        hipLaunchKernelGGL(k_gbab_accum, gp, bk, 0, st, g);
        hipLaunchKernelGGL(k_gbab_decide, dim3((cap + 255) / 256), bk, 0, st, g, P, L);
        if (L < P.max_layer) hipLaunchKernelGGL(k_gbab_descend, gp, bk, 0, st, g);
      }
    }
    VBA_HIPCHK(err, hipGetLastError());
    VBA_HIPCHK(err, hipStreamSynchronize(st));
    VBA_HIPCHK(err, hipMemcpyAsync(s.h_cnt, g.cnt, GCNT_N * sizeof(int), hipMemcpyDeviceToHost, st));
    VBA_HIPCHK(err, hipStreamSynchronize(st));
    if (s.h_cnt[GCNT_OVERFLOW] == 2) { err = "keyframe point outside the 21-bit voxel index range"; return VBA_ERR_CAPACITY; }
    if (!s.h_cnt[GCNT_OVERFLOW]) { s.last_cap = cap; break; }
    // (the undersized node arrays stay in the arena until the next build rewinds it)
    cap *= 2;
    if (attempt == 9) { err = "octree node capacity"; return VBA_ERR_CAPACITY; }
  }
  // sparse factor store
  BigView &b = s.b;
  const int V = s.h_cnt[GCNT_FACTORS];
  { int r = big_store_voxels(s, st, W, V, err); if (r) return r; }
  int E = 0;
  if (V > 0) {
    const int nn = s.h_cnt[GCNT_NODES] < g.cap ? s.h_cnt[GCNT_NODES] : g.cap;
    hipLaunchKernelGGL(k_gbab_vcount, dim3((nn + 255) / 256), bk, 0, st, g, s.d_vcnt);
    hipLaunchKernelGGL(k_big_scan, dim3(1), bk, 0, st, V, s.d_vcnt, b.vptr);
    VBA_HIPCHK(err, hipStreamSynchronize(st));
    VBA_HIPCHK(err, hipMemcpyAsync(&E, b.vptr + V, 4, hipMemcpyDeviceToHost, st));
    VBA_HIPCHK(err, hipStreamSynchronize(st));
  }
  { int r = big_store_entries(s, E, err); if (r) return r; }
  if (V > 0) {
    const int nn = s.h_cnt[GCNT_NODES] < g.cap ? s.h_cnt[GCNT_NODES] : g.cap;
    BigView bt = b;                                  // table order into scratch (es: 27 rows of capE doubles), frame order into the store
    bt.ecl = b.es; bt.efr = (int *)(b.es + (size_t)10 * b.capE);
    hipLaunchKernelGGL(k_gbab_fill, dim3((ecap + 255) / 256), bk, 0, st, g, bt, s.d_fill);
    if (E > 0) hipLaunchKernelGGL(k_gbab_order, dim3((E + 255) / 256), bk, 0, st, b, (const int *)bt.efr, (const double *)bt.ecl);
    hipLaunchKernelGGL(k_gbab_voxels, dim3((nn + 255) / 256), bk, 0, st, g, b);
    VBA_HIPCHK(err, hipGetLastError());
  }
  return big_store_eidx(s, st, err);
}

// divide_thread (VM:347-389): H, g, r at `poses` on the host side buffers (full layout)
// Hessian pass on the sparse store: H (n x n) and g stay in HBM (the solver reads them there); the host gets diag(H), g and r.
// slices: voxel slices of the SYRK, 0 = chosen here (about 2048 workgroups), k >= 1 = k; either way at most one per chunk.
inline int big_hessian(BigStore &s, hipStream_t st, const double *poses, double *hdiag, double *gvec, double *r, std::string &err, int slices) {
  BigView &b = s.b;
  const size_t n6 = (size_t)6 * b.W;
  VBA_HIPCHK(err, hipMemcpyAsync(b.poses, poses, (size_t)b.W * 12 * 8, hipMemcpyHostToDevice, st));
  VBA_HIPCHK(err, hipMemsetAsync(b.H, 0, n6 * n6 * 8, st)); VBA_HIPCHK(err, hipMemsetAsync(b.g, 0, n6 * 8, st)); VBA_HIPCHK(err, hipMemsetAsync(b.r, 0, 8, st));
  if (b.E > 0) {
    hipLaunchKernelGGL(k_big_slot, dim3((b.E + 127) / 128), dim3(128), 0, st, b);
    const int nt = (b.W + BIG_TF - 1) / BIG_TF, npair = nt * (nt + 1) / 2, nchunk = (b.V + BIG_VC - 1) / BIG_VC;
    int nslice = slices >= 1 ? slices : (2048 + npair - 1) / npair;
    if (nslice > nchunk) nslice = nchunk;
    if (nslice < 1) nslice = 1;
    hipLaunchKernelGGL(k_big_syrk, dim3(npair, nslice), dim3(256), 0, st, b, nt, nslice);
    hipLaunchKernelGGL(k_big_diag, dim3(b.W), dim3(256), 0, st, b);   // after the SYRK atomics on H (stream order)
  }
  hipLaunchKernelGGL(k_big_getdiag, dim3((unsigned)((n6 + 255) / 256)), dim3(256), 0, st, b.H, (int)n6, s.d_vec);
  VBA_HIPCHK(err, hipGetLastError());
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  VBA_HIPCHK(err, hipMemcpyAsync(hdiag, s.d_vec, n6 * 8, hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipMemcpyAsync(gvec, b.g, n6 * 8, hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipMemcpyAsync(r, b.r, 8, hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  return VBA_OK;
}
// the six diagonal entries of every 6x6 cross block of the Hessian of the last big_hessian (before the gauge): [W][W][6]
inline int big_block_diagonals(BigStore &s, hipStream_t st, double *out, std::string &err) {
  const int W = s.b.W;
  const size_t n6 = (size_t)6 * W, cnt = (size_t)6 * W * W;
  hipLaunchKernelGGL(k_big_blockdiag, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, s.b.H, W, s.d_vec + 3 * n6);
  VBA_HIPCHK(err, hipGetLastError());
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  VBA_HIPCHK(err, hipMemcpyAsync(out, s.d_vec + 3 * n6, cnt * 8, hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  return VBA_OK;
}
// only_residual (VM:391-420): also refreshes the per-voxel eigen state
inline int big_residual(BigStore &s, hipStream_t st, const double *poses, double *r, std::string &err) {
  BigView &b = s.b;
  VBA_HIPCHK(err, hipMemcpyAsync(b.poses, poses, (size_t)b.W * 12 * 8, hipMemcpyHostToDevice, st));
  VBA_HIPCHK(err, hipMemsetAsync(b.r, 0, 8, st));
  if (b.V > 0) hipLaunchKernelGGL(k_big_residual, dim3((b.V + 255) / 256), dim3(256), 0, st, b);
  VBA_HIPCHK(err, hipGetLastError());
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  VBA_HIPCHK(err, hipMemcpyAsync(r, b.r, 8, hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  return VBA_OK;
}

// Eigen's LDLT pivot order for (H + u D): largest |stored diagonal| first, first index wins ties.  hd = diag(H) after the gauge.
void big_pivot_order(const double *hd, double u, int n, int *ord) {
  std::vector<double> dabs(n);
  for (int r = 0; r < n; r++) { ord[r] = r; dabs[r] = std::fabs(hd[r] + u * hd[r]); }
  std::stable_sort(ord, ord + n, [&](int a, int b) { return dabs[a] > dabs[b]; });
}
// the model decrease q1 = 0.5 dx^T (u D dx - g) of VM:465 (hd, g after the gauge), summed in row order
double big_q1(const double *dxi, const double *hd, const double *g, double u, int n) {
  double q1 = 0;
  for (int r = 0; r < n; r++) q1 += dxi[r] * (u * hd[r] * dxi[r] - g[r]);
  return 0.5 * q1;
}

// (H + u D) dxi = -g with the gauge of VM:452-455, H / g = the device buffers of the last big_hessian (before the gauge).
// ord = Eigen's pivot order (host).  Factorisation and back substitution run on the device; the host gets dxi (n doubles).
int big_solve(BigStore &s, hipStream_t st, const int *ord, double u, double *dxi, std::string &err) {
  const int n = 6 * s.b.W, NP = s.NP, ld = s.ld;
  VBA_HIPCHK(err, hipMemcpyAsync(s.d_ord, ord, (size_t)n * 4, hipMemcpyHostToDevice, st));
  const long long tot = (long long)(NP + 1) * NP;
  hipLaunchKernelGGL(k_bigl_setup, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, s.b.H, s.b.g, s.d_ord, n, NP, ld, u, s.d_Ab);
  for (int k0 = 0; k0 < NP; k0 += 8) {
    hipLaunchKernelGGL(k_bigl_panel, dim3(1), dim3(256), 0, st, s.d_Ab, s.d_Tb, NP, ld, k0);
    const int kn = k0 + 8;
    if (kn <= NP) {
      const int nt = (NP + 1 - kn + 63) / 64;
      if (nt > 0) hipLaunchKernelGGL(k_bigl_update, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, s.d_Ab, s.d_Tb, NP, ld, k0);
    }
  }
  // back substitution on the device, 64 unknowns per step from the bottom
  for (int lo = ((n - 1) / 64) * 64; lo >= 0; lo -= 64) {
    hipLaunchKernelGGL(k_bigl_bs_tri, dim3(1), dim3(64), 0, st, s.d_Ab, NP, ld, n, lo);
    if (lo > 0) hipLaunchKernelGGL(k_bigl_bs_gemv, dim3((lo + 255) / 256), dim3(256), 0, st, s.d_Ab, NP, ld, n, lo);
  }
  double *d_dxi = s.d_vec + 2 * (size_t)n;
  hipLaunchKernelGGL(k_bigl_bs_out, dim3((n + 255) / 256), dim3(256), 0, st, s.d_Ab, NP, ld, n, s.d_ord, d_dxi);
  VBA_HIPCHK(err, hipGetLastError());
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  VBA_HIPCHK(err, hipMemcpyAsync(dxi, d_dxi, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  VBA_HIPCHK(err, hipStreamSynchronize(st));
  return VBA_OK;
}

}  // namespace vba

extern "C" {

// ---------------------------------------------------------------- the entry points
static GbaParams gba_params(vba_ctx *c, double voxel_size, double min_eig, const double *eig_array) {
  GbaParams P;
  P.voxel_size = voxel_size; P.min_eigen_value = min_eig; P.max_layer = c->opt.max_layer;
  for (int k = 0; k < 4; k++) P.eig_array[k] = eig_array[k];
  return P;
}
static int gba_build_into_store(vba_ctx *c, int wdsize, const int *offsets, const double *pl, const double *poses, const GbaParams &P) {
  int nf = 0;
  TimedSpan sp{};
  span_begin(c, "gba_build", sp);
  int st = gba_build(c->gba, c->stream, wdsize, offsets, pl, poses, P, &nf, c->err);
  if (st) return st;
  c->nvox = 0;
  st = factor_reserve(c, nf > 0 ? nf : 1);
  if (st) return st;
  if (nf > 0) {
    const int nn = c->gba.h_cnt[GCNT_NODES] < c->gba.v.cap ? c->gba.h_cnt[GCNT_NODES] : c->gba.v.cap;
    hipLaunchKernelGGL(k_gba_extract, dim3((nn + 255) / 256, 10 * wdsize + 33), dim3(256), 0, c->stream, c->gba.v, c->fv);
    factor_update_mask(c, 0, nf);
    HIPCHK(c, hipGetLastError());
  }
  span_end(c, "gba_build", sp);
  c->nvox = nf;
  return VBA_OK;
}
static int gba_check(vba_ctx *c, int wdsize, const int *offsets, const double *pl, const double *poses) {
  if (wdsize != c->opt.win_size) return VBA_ERR_UNSUPPORTED_WINDOW;
  if (!offsets || !poses || offsets[0] != 0) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < wdsize; i++) if (offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
  if (offsets[wdsize] > 0 && !pl) return VBA_ERR_BAD_ARG;
  return VBA_OK;
}
int vba_gba_build(vba_ctx *c, int wdsize, const int *offsets, const double *pnt_local, const double *poses, double gba_voxel_size,
                  double gba_min_eigen_value, const double *gba_eigen_value_array) {
  int st = gba_check(c, wdsize, offsets, pnt_local, poses);
  if (st) return st;
  if (!gba_eigen_value_array) return VBA_ERR_BAD_ARG;
  return gba_build_into_store(c, wdsize, offsets, pnt_local, poses, gba_params(c, gba_voxel_size, gba_min_eigen_value, gba_eigen_value_array));
}

// Lidar_BA_Optimizer::damping_iter (VM:422-497) for an arbitrary window: device Hessian / residual passes on the sparse
// store, gauge + (H + uD) LDL^T + retraction on the host.
// hdiag6_out: [W][W][6] = the six diagonal entries of every 6x6 block of *hess (all that HBA_add_edge reads of it, VS:2926-2951);
// the n x n Hessian itself stays in HBM.
static int big_damping_iter(vba_ctx *c, int W, double *poses, std::vector<double> &hdiag6_out, double *resis2, int max_iter, int thd_num, int *is_converge) {
  BigStore &S = c->big;
  const int n = 6 * W;
  if (S.b.V < thd_num) return VBA_ERR_TOO_FEW_VOXELS;                 // VM:399-403
  std::vector<double> x(poses, poses + (size_t)W * 12), xt(x), hd(n), JacT(n), dxi(n);
  double u = 0.01, v = 2, residual1 = 0, residual2 = 0;
  bool is_calc_hess = true, conv = true;
  c->trace.clear();
  for (int it = 0; it < max_iter; it++) {
    if (is_calc_hess) {
      int st = big_hessian(S, c->stream, x.data(), hd.data(), JacT.data(), &residual1, c->err, 0);   // *hess = Hess (VM:446) stays on the device
      if (st) return st;
      for (int r = 0; r < 6; r++) { hd[r] = 1.0; JacT[r] = 0.0; }     // gauge VM:452-455 (k_bigl_setup applies it to the matrix)
    }
    if (it == 0) resis2[0] = residual1;
    {
      // pivot order of Eigen's LDLT (largest |stored diagonal| first, first index wins ties), then the device factorisation
      std::vector<int> ord(n);
      big_pivot_order(hd.data(), u, n, ord.data());
      int st2 = big_solve(S, c->stream, ord.data(), u, dxi.data(), c->err);
      if (st2) return st2;
    }
    for (int j = 0; j < W; j++) {
      double E[9];
      vbh::so3_exp(&dxi[6 * j], E);
      vbh::m3_mul(&x[12 * j], E, &xt[12 * j]);
      for (int k = 0; k < 3; k++) xt[12 * j + 9 + k] = x[12 * j + 9 + k] + dxi[6 * j + 3 + k];
    }
    const double q1 = big_q1(dxi.data(), hd.data(), JacT.data(), u, n);
    int st = big_residual(S, c->stream, xt.data(), &residual2, c->err);
    if (st) return st;
    double q = residual1 - residual2;
    const double tr[5] = {residual1, residual2, u, v, q1};
    c->trace.insert(c->trace.end(), tr, tr + 5);
    if (q > 0) {
      x = xt;
      q = q / q1;
      v = 2;
      q = 1 - std::pow(2 * q - 1, 3);
      u *= (q < 1.0 / 3 ? 1.0 / 3 : q);
      is_calc_hess = true;
    } else {
      u = u * v; v = 2 * v;
      is_calc_hess = false; conv = false;
    }
    if (std::fabs((residual1 - residual2) / residual1) < 1e-6) break;
  }
  resis2[1] = residual2;
  std::memcpy(poses, x.data(), x.size() * sizeof(double));
  if (is_converge) *is_converge = conv ? 1 : 0;
  hdiag6_out.resize((size_t)6 * W * W);
  return big_block_diagonals(S, c->stream, hdiag6_out.data(), c->err);   // b.H still holds the last evaluated Hessian (a rejected step does not recompute it)
}

// the keyframe clouds of an HBA_add_edge call in HBM: the two halves of d_refpts, the cloud (*d_pl) and its reference (*d_ref)
static int hba_stage_points(vba_ctx *c, int n, const double *pnt_local, double **d_pl, double **d_ref) {
  if ((size_t)n * 3 > c->d_refpts.n / 2) HIPCHK(c, c->d_refpts.ensure(2 * ((size_t)n * 3 + 3072)));
  *d_pl = c->d_refpts; *d_ref = c->d_refpts + c->d_refpts.n / 2;
  if (n > 0) HIPCHK(c, hipMemcpyAsync(*d_pl, pnt_local, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  return VBA_OK;
}

int vba_hba_add_edge(vba_ctx *c, int wdsize, const int *offsets, const double *pnt_local, double *poses, double gba_voxel_size,
                     double gba_min_eigen_value, const double *gba_eigen_value_array, int max_iter, int thread_num, double *edges_out, int *n_edges,
                     double *cloud_out, int *cloud_count, int *n_cloud, double *resis_log, int *n_log) {
  const bool big = (wdsize != c->opt.win_size);      // any other window size (the top-level BA over all submaps): sparse path
  if (big && wdsize < 2) return VBA_ERR_BAD_ARG;
  int st = VBA_OK;
  if (!big) st = gba_check(c, wdsize, offsets, pnt_local, poses);
  else {
    if (!offsets || !poses || offsets[0] != 0) return VBA_ERR_BAD_ARG;
    for (int i = 0; i < wdsize; i++) if (offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
    if (offsets[wdsize] > 0 && !pnt_local) return VBA_ERR_BAD_ARG;
  }
  if (st) return st;
  if (!gba_eigen_value_array || !edges_out || !n_edges || (cloud_out && (!cloud_count || !n_cloud))) return VBA_ERR_BAD_ARG;
  const int W = wdsize, n6 = 6 * W, n = offsets[W];
  *n_edges = 0;
  if (n_log) *n_log = 0;
  static const bool want_times = diag_env("VBA_HBA_TIMES") != nullptr;      // diagnostic: wall-clock split of the call on stderr
  double t_ph[5] = {0, 0, 0, 0, 0};
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_mark = want_times ? now() : 0.0;
  auto lap = [&](int k) { if (want_times) { hipStreamSynchronize(c->stream); const double t = now(); t_ph[k] += t - t_mark; t_mark = t; } };
  // the keyframe clouds stay in HBM for the whole call (every outer iteration re-cuts them with the current poses)
  double *d_pl = nullptr, *d_ref = nullptr;
  st = hba_stage_points(c, n, pnt_local, &d_pl, &d_ref);
  if (st) return st;
  GbaParams P = gba_params(c, gba_voxel_size, gba_min_eigen_value, gba_eigen_value_array);
  std::vector<double> hess(big ? 0 : (size_t)n6 * n6, 0.0), hd6;      // the any-window path keeps *hess in HBM and returns its block diagonals
  lap(0);
  const int up = 4;                                                       // VS:2866
  int converge_flag = 0;
  double converge_thre = 0.05;
  for (int iterCnt = 0; iterCnt < max_iter; iterCnt++) {
    if (converge_flag == 1 || iterCnt == max_iter - 1)                    // VS:2871-2881: last pass with the local-map parameters
      P = gba_params(c, c->opt.voxel_size, c->opt.min_eigen_value, c->opt.plane_eigen_value_thre);
    double resis[2] = {0, 0};
    int is_converge = 0;
    if (!big) {
      st = gba_build_into_store(c, W, offsets, d_pl, poses, P);
      if (st) return st;
      lap(1);
      st = vba_lidar_ba_damping_iter(c, poses, hess.data(), resis, up, thread_num, &is_converge);
    } else {
      st = big_build(c->big, c->stream, W, offsets, d_pl, poses, P, c->err);
      if (st) return st;
      lap(1);
      st = big_damping_iter(c, W, poses, hd6, resis, up, thread_num, &is_converge);
    }
    if (st) return st;
    lap(2);
    if (resis_log && n_log) { resis_log[2 * *n_log] = resis[0]; resis_log[2 * *n_log + 1] = resis[1]; (*n_log)++; }
    if ((std::fabs(resis[0] - resis[1]) / resis[0] < converge_thre && is_converge) || (iterCnt == max_iter - 2 && converge_flag == 0)) {
      converge_thre = 0.01;                                               // VS:2903-2915
      if (converge_flag == 0) converge_flag = 1;
      else if (converge_flag == 1) break;
    }
  }
  int ne = 0;
  for (int i = 0; i < W - 1; i++)
    for (int j = i + 1; j < W; j++) {                                     // VS:2926-2951
      bool isAdd = true;
      double v6[6];
      for (int k = 0; k < 6; k++) {
        const double hc = std::fabs(big ? hd6[((size_t)i * W + j) * 6 + k] : hess[(size_t)(6 * i + k) * n6 + 6 * j + k]);
        if (hc < 1e-6) { isAdd = false; break; }
        v6[k] = 1.0 / hc;
      }
      if (!isAdd) continue;
      double *o = edges_out + 20 * (size_t)ne++;
      const double *Ri = poses + 12 * i, *Rj = poses + 12 * j;
      o[0] = i; o[1] = j;
      vbh::m3_Tmul(Ri, Rj, o + 2);
      const double d[3] = {Rj[9] - Ri[9], Rj[10] - Ri[10], Rj[11] - Ri[11]};
      vbh::m3_Tvec(Ri, d, o + 11);
      for (int k = 0; k < 6; k++) o[14 + k] = v6[k];
    }
  *n_edges = ne;
  lap(3);
  if (cloud_out) {                                                        // VS:2954-2989
    *n_cloud = 0;
    if (n > 0) {
      std::vector<double> rel((size_t)W * 12);
      for (int i = 0; i < W; i++) {
        const double *R0 = poses, *Ri = poses + 12 * i;
        vbh::m3_Tmul(R0, Ri, rel.data() + 12 * i);
        const double d[3] = {Ri[9] - R0[9], Ri[10] - R0[10], Ri[11] - R0[11]};
        vbh::m3_Tvec(R0, d, rel.data() + 12 * i + 9);
      }
      double *d_rel = big ? c->big.g.poses : c->gba.v.poses;
      const int *d_off = big ? c->big.g.offsets : c->gba.v.offsets;
      HIPCHK(c, hipMemcpyAsync(d_rel, rel.data(), rel.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(k_gba_to_ref, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, W, d_off, d_pl, d_rel, d_ref);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipStreamSynchronize(c->stream));      // rel is a host temporary
      std::vector<int> first(n);
      st = vba_scan_down_sampling_voxel(c, n, d_ref, c->opt.voxel_size / 8, cloud_out, cloud_count, first.data(), n_cloud);
      if (st) return st;
    }
  }
  lap(4);
  if (want_times)
    std::fprintf(stderr, "[hba_add_edge W=%d n=%d] upload %.0f  build %.0f  LM %.0f  edges %.0f  cloud %.0f us\n", W, n, t_ph[0], t_ph[1], t_ph[2], t_ph[3], t_ph[4]);
  return VBA_OK;
}

// ---------------------------------------------------------------- diagnostic entries of the any-window path (tests/test_gpu_big.py)
static bool big_finite(const double *a, size_t n) {
  for (size_t i = 0; i < n; i++) if (!std::isfinite(a[i])) return false;
  return true;
}
static int big_dbg_ctx(vba_ctx *c, const char *who) {
  if (!c) return VBA_ERR_BAD_ARG;
  if (c->n_ranks > 1) { c->set_error(std::string(who) + " runs the any-window path of one device: unsharded contexts only"); return VBA_ERR_UNSUPPORTED; }
  return VBA_OK;
}
static bool big_has_store(const vba_ctx *c) { return c->big.b.W >= 2 && c->big.b.H != nullptr && c->big.b.eidx != nullptr; }

int vba_debug_big_load(vba_ctx *c, int W, int V, const int *vptr, const int *efr, const double *ecl, const double *eig_val, const double *eig_vec,
                       const double *pcr_add) {
  int st = big_dbg_ctx(c, "vba_debug_big_load");
  if (st) return st;
  if (W < 2 || W > 1024 || V < 0 || !vptr || vptr[0] != 0) return VBA_ERR_BAD_ARG;
  for (int v = 0; v < V; v++) if (vptr[v + 1] <= vptr[v]) return VBA_ERR_BAD_ARG;        // non-decreasing, and no voxel without an entry (N = 0)
  const int E = vptr[V];
  if (V > 0 && (!efr || !ecl || !eig_val || !eig_vec || !pcr_add)) return VBA_ERR_BAD_ARG;
  for (int v = 0; v < V; v++)
    for (int e = vptr[v]; e < vptr[v + 1]; e++)
      if (efr[e] < 0 || efr[e] >= W || (e > vptr[v] && efr[e] <= efr[e - 1])) return VBA_ERR_BAD_ARG;
  if (V > 0 && (!big_finite(ecl, (size_t)E * 10) || !big_finite(eig_val, (size_t)V * 3) || !big_finite(eig_vec, (size_t)V * 9) || !big_finite(pcr_add, (size_t)V * 10)))
    return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  BigStore &s = c->big;
  HIPCHK(c, hipStreamSynchronize(c->stream));        // nothing of the previous store is in flight when the arena is rewound
  s.reset();
  st = big_store_voxels(s, c->stream, W, V, c->err);
  if (st) return st;
  st = big_store_entries(s, E, c->err);
  if (st) return st;
  BigView &b = s.b;
  if (V > 0) {
    // the arrays of the view are SoA with strides capV / capE; evox is the CSR row of every entry
    const size_t cv = (size_t)b.capV, ce = (size_t)b.capE;
    std::vector<double> hv(22 * cv), he(10 * ce);
    std::vector<int> hx(ce);
    for (int v = 0; v < V; v++) {
      for (int k = 0; k < 3; k++) hv[(size_t)k * cv + v] = eig_val[3 * (size_t)v + k];
      for (int k = 0; k < 9; k++) hv[(size_t)(3 + k) * cv + v] = eig_vec[9 * (size_t)v + k];
      for (int k = 0; k < 10; k++) hv[(size_t)(12 + k) * cv + v] = pcr_add[10 * (size_t)v + k];
      for (int e = vptr[v]; e < vptr[v + 1]; e++) hx[e] = v;
    }
    for (int e = 0; e < E; e++)
      for (int k = 0; k < 10; k++) he[(size_t)k * ce + e] = ecl[10 * (size_t)e + k];
    HIPCHK(c, hipMemcpyAsync(b.vptr, vptr, (size_t)(V + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.eval, hv.data(), 3 * cv * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.evec, hv.data() + 3 * cv, 9 * cv * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.pcr, hv.data() + 12 * cv, 10 * cv * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.efr, efr, (size_t)E * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.evox, hx.data(), (size_t)E * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.ecl, he.data(), 10 * ce * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the staging vectors are host temporaries
  }
  st = big_store_eidx(s, c->stream, c->err);
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return VBA_OK;
}

int vba_debug_big_build(vba_ctx *c, int W, const int *offsets, const double *pnt_local, const double *poses, double gba_voxel_size,
                        double gba_min_eigen_value, const double *gba_eigen_value_array, int *V, int *E) {
  int st = big_dbg_ctx(c, "vba_debug_big_build");
  if (st) return st;
  if (W < 2 || W > 1024 || !offsets || !poses || !gba_eigen_value_array || !V || !E || offsets[0] != 0) return VBA_ERR_BAD_ARG;
  for (int i = 0; i < W; i++) if (offsets[i + 1] < offsets[i]) return VBA_ERR_BAD_ARG;
  const int n = offsets[W];
  if (n > 0 && !pnt_local) return VBA_ERR_BAD_ARG;
  if (!big_finite(poses, (size_t)W * 12) || !big_finite(gba_eigen_value_array, 4) || !std::isfinite(gba_voxel_size) || !(gba_voxel_size > 0.0) ||
      !std::isfinite(gba_min_eigen_value))
    return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  double *d_pl = nullptr, *d_ref = nullptr;
  st = hba_stage_points(c, n, pnt_local, &d_pl, &d_ref);
  if (st) return st;
  st = big_build(c->big, c->stream, W, offsets, d_pl, poses, gba_params(c, gba_voxel_size, gba_min_eigen_value, gba_eigen_value_array), c->err);
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *V = c->big.b.V; *E = c->big.b.E;
  return VBA_OK;
}

int vba_debug_big_size(vba_ctx *c, int *W, int *V, int *E) {
  int st = big_dbg_ctx(c, "vba_debug_big_size");
  if (st) return st;
  if (!W || !V || !E) return VBA_ERR_BAD_ARG;
  const bool has = big_has_store(c);
  *W = has ? c->big.b.W : 0; *V = has ? c->big.b.V : 0; *E = has ? c->big.b.E : 0;
  return VBA_OK;
}

int vba_debug_big_read(vba_ctx *c, int *vptr, int *efr, int *evox, int *eidx, double *ecl, double *eig_val, double *eig_vec, double *pcr_add) {
  int st = big_dbg_ctx(c, "vba_debug_big_read");
  if (st) return st;
  if (!big_has_store(c)) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const BigView &b = c->big.b;
  const int V = b.V, E = b.E, W = b.W;
  const size_t cv = (size_t)b.capV, ce = (size_t)b.capE;
  std::vector<double> hv(22 * cv), he(10 * ce);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (vptr) HIPCHK(c, hipMemcpy(vptr, b.vptr, (size_t)(V + 1) * 4, hipMemcpyDeviceToHost));
  if (efr && E > 0) HIPCHK(c, hipMemcpy(efr, b.efr, (size_t)E * 4, hipMemcpyDeviceToHost));
  if (evox && E > 0) HIPCHK(c, hipMemcpy(evox, b.evox, (size_t)E * 4, hipMemcpyDeviceToHost));
  if (eidx && V > 0) HIPCHK(c, hipMemcpy(eidx, b.eidx, (size_t)V * W * 4, hipMemcpyDeviceToHost));
  if (ecl && E > 0) {
    HIPCHK(c, hipMemcpy(he.data(), b.ecl, 10 * ce * 8, hipMemcpyDeviceToHost));
    for (int e = 0; e < E; e++)
      for (int k = 0; k < 10; k++) ecl[10 * (size_t)e + k] = he[(size_t)k * ce + e];
  }
  if (V > 0 && (eig_val || eig_vec || pcr_add)) {
    HIPCHK(c, hipMemcpy(hv.data(), b.eval, 3 * cv * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hv.data() + 3 * cv, b.evec, 9 * cv * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hv.data() + 12 * cv, b.pcr, 10 * cv * 8, hipMemcpyDeviceToHost));
    for (int v = 0; v < V; v++) {
      if (eig_val) for (int k = 0; k < 3; k++) eig_val[3 * (size_t)v + k] = hv[(size_t)k * cv + v];
      if (eig_vec) for (int k = 0; k < 9; k++) eig_vec[9 * (size_t)v + k] = hv[(size_t)(3 + k) * cv + v];
      if (pcr_add) for (int k = 0; k < 10; k++) pcr_add[10 * (size_t)v + k] = hv[(size_t)(12 + k) * cv + v];
    }
  }
  return VBA_OK;
}

int vba_debug_big_hessian(vba_ctx *c, const double *poses, int slices, double *H, double *g, double *r, double *blockdiag) {
  int st = big_dbg_ctx(c, "vba_debug_big_hessian");
  if (st) return st;
  if (!poses || !H || !g || !r || !blockdiag || slices < 0 || !big_has_store(c)) return VBA_ERR_BAD_ARG;
  BigStore &S = c->big;
  const size_t n6 = (size_t)6 * S.b.W;
  if (!big_finite(poses, (size_t)S.b.W * 12)) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<double> hd(n6);
  st = big_hessian(S, c->stream, poses, hd.data(), g, r, c->err, slices);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(H, S.b.H, n6 * n6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return big_block_diagonals(S, c->stream, blockdiag, c->err);
}

int vba_debug_big_residual(vba_ctx *c, const double *poses, double *r) {
  int st = big_dbg_ctx(c, "vba_debug_big_residual");
  if (st) return st;
  if (!poses || !r || !big_has_store(c)) return VBA_ERR_BAD_ARG;
  if (!big_finite(poses, (size_t)c->big.b.W * 12)) return VBA_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return big_residual(c->big, c->stream, poses, r, c->err);
}

// thd_globalmapping (VS:3018-3141), the optimisation work of the hierarchical global BA over one map:
//   bottom layer  windows of `wdsize` keyframes, stride `mgsize` (VS:3033-3034, 3064-3066, 3136-3137): HBA_add_edge(xs = x0 of the
//                 window, max_iter 1, thread_num 2) -> edges1 + one submap (pose x0 of the window's first keyframe, cloud
//                 = the window's down-sampled points in that frame, VS:3084-3089);
//   top layer     HBA_add_edge over all submaps with their CURRENT poses (VS:3096-3110): edges2.
// Edge rows carry GLOBAL keyframe indices.  (Queue handling, map switching and the GTSAM pose graph stay with the caller.)
//
// The bottom layer has three drivers over one plan (vba_hba_plan.hpp: windows, lanes, the layout of d_hba_all) and shared pieces
// ("The drivers of vba_hba_global"): hba_window optimises one window into a [n_cloud, n_edges, status | edge rows] record,
// hba_collect walks the records of the two chunked modes in window order, hba_top is the top-level window.
static_assert(HBA_PLAN_OK == VBA_OK && HBA_PLAN_ERR_RUNTIME == VBA_ERR_HIP && HBA_PLAN_ERR_CAPACITY == VBA_ERR_CAPACITY, "vba_hba_plan.hpp returns the ABI's statuses");

struct HbaCall {                                    // the caller's arrays and parameters, as vba_hba_global received them
  int n_kf; const int *offsets; const double *pnt_local, *poses_x0, *poses_now;
  double voxel_size, min_eig; const double *eig; int total_max_iter;
  double *edges1; int cap1, *n1; double *edges2; int cap2, *n2;
};
struct HbaSubmaps {                                 // global id of every submap's first keyframe, points of its cloud, points of all clouds
  std::vector<int> first, n; size_t pts = 0;
  void push(int start, int nc) { first.push_back(start); n.push_back(nc); pts += (size_t)nc; }
};
// VBA_HBA_TIMES (diagnostic build): the wall-clock split of the call on stderr, once the bottom layer has succeeded
struct HbaTimes {
  bool on; double t0 = 0, t1 = 0;
  static double now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  explicit HbaTimes(vba_ctx *c) { static const bool want = diag_env("VBA_HBA_TIMES") != nullptr; on = want; if (on) { hipStreamSynchronize(c->stream); t0 = now(); } }
  void windows_done() { if (on) t1 = now(); }
  ~HbaTimes() { if (on && t1 > 0) std::fprintf(stderr, "[hba_global] windows %.0f us, top %.0f us (after the upload)\n", t1 - t0, now() - t1); }
};

// One bottom-layer window on context cx: HBA_add_edge(xs = x0 of the window, max_iter 1, thread_num 2) on the keyframe clouds at d_all,
// the down-sampled cloud to d_cloud, status, counts and edge rows (window-local indices) into the record.  No exception leaves it.
static int hba_window(vba_ctx *cx, const HbaPlan &P, int w, const HbaCall &A, const double *d_all, double *d_cloud, double *rec, std::vector<int> &ccnt) try {
  const int start = P.win[w].start;
  std::vector<int> off(P.wdsize + 1);
  for (int i = 0; i <= P.wdsize; i++) off[i] = A.offsets[start + i] - A.offsets[start];
  std::vector<double> xs(A.poses_x0 + (size_t)start * 12, A.poses_x0 + (size_t)(start + P.wdsize) * 12);
  int ne = 0, nc = 0;
  const int st = vba_hba_add_edge(cx, P.wdsize, off.data(), d_all + (size_t)A.offsets[start] * 3, xs.data(), A.voxel_size, A.min_eig, A.eig, 1, 2, rec + 3, &ne,
                                  d_cloud, ccnt.data(), &nc, nullptr, nullptr);
  rec[2] = st;
  if (st == VBA_OK) { rec[0] = nc; rec[1] = ne; }
  return st;
} catch (const std::bad_alloc &) {                  // a host allocation of the window is the window's failure: it travels like any other status
  cx->set_error("vba_hba_global: out of host memory in a bottom-layer window");
  return (int)(rec[2] = VBA_ERR_CAPACITY);
} catch (...) {
  cx->set_error("vba_hba_global: unexpected exception in a bottom-layer window");
  return (int)(rec[2] = VBA_ERR_HIP);
}
static double *hba_chunk_cloud(const HbaPlan &P, double *d_rep, int w) { return d_rep + ((size_t)P.win[w].lane * P.chunk_pts + P.win[w].roff) * 3; }

// The records of the two chunked modes in window order: the first failing window decides (lane_err: the worker lanes' error texts;
// null: replicas, where the text is the same on every rank); otherwise edges1 with global indices, and every window's cloud from its
// lane's chunk to the compact submap area that the top level reads.
static int hba_collect(vba_ctx *c, const HbaPlan &P, const HbaCall &A, const std::vector<double> &meta, double *d_sub, double *d_rep, HbaSubmaps &S,
                       const std::vector<std::string> *lane_err) {
  for (int w = 0; w < P.n_win; w++) {
    const int st = (int)P.rec(meta.data(), w)[2];
    if (st == VBA_OK) continue;
    if (st < 0) { c->set_error("vba_hba_global: a bottom-layer window was not run"); return VBA_ERR_HIP; }
    if (!lane_err) c->set_error("a bottom-layer window failed on one of the ranks");
    else if (!(*lane_err)[P.win[w].lane].empty()) c->set_error((*lane_err)[P.win[w].lane]);
    return st;
  }
  for (int w = 0; w < P.n_win; w++) {
    const double *rec = P.rec(meta.data(), w);
    const int nc = (int)rec[0], start = P.win[w].start;
    if (hba_append_edges(A.edges1, A.cap1, A.n1, rec + 3, (int)rec[1], [start](double i) { return i + start; })) return VBA_ERR_CAPACITY;
    if (nc > 0) HIPCHK(c, hipMemcpyAsync(d_sub + S.pts * 3, hba_chunk_cloud(P, d_rep, w), (size_t)nc * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    S.push(start, nc);
  }
  return VBA_OK;
}

// the keyframe clouds go to HBM once (the stride-5 windows overlap: every keyframe is used twice); the worker driver uploads them itself
static int hba_upload_all(vba_ctx *c, const HbaPlan &P, const HbaCall &A, double *d_all) {
  if (P.n_all > 0) HIPCHK(c, hipMemcpyAsync(d_all, A.pnt_local, P.n_all * 3 * sizeof(double), hipMemcpyDefault, c->stream));
  return VBA_OK;
}

// One window after the other: the submap clouds never leave HBM, every window's down-sampled cloud is written behind the previous one.
static int hba_bottom_sequential(vba_ctx *c, const HbaPlan &P, const HbaCall &A, double *d_all, double *d_sub, std::vector<int> &ccnt, HbaSubmaps &S) {
  std::vector<double> rec(P.meta_per);
  for (int w = 0; w < P.n_win; w++) {
    const int start = P.win[w].start;
    const int st = hba_window(c, P, w, A, d_all, d_sub + S.pts * 3, rec.data(), ccnt);
    if (st) return st;
    if (hba_append_edges(A.edges1, A.cap1, A.n1, rec.data() + 3, (int)rec[1], [start](double i) { return i + start; })) return VBA_ERR_CAPACITY;
    S.push(start, (int)rec[0]);
  }
  return VBA_OK;
}

// ONE rank: one window is a chain of small kernels and host round trips that leaves most of the chip idle — KL worker contexts (own
// stream, own octree and LM state; host threads drive them) optimise windows side by side: lane t takes windows t, t + KL, ... and
// writes their clouds into its chunk.  The keyframe clouds travel to HBM in chunks on a stream of their own while the first windows
// are already being optimised (2.4 GB at full length: as long as the windows themselves); a window starts when its keyframes have
// arrived.  A failing window lowers stop_after: lanes skip the windows above it and the uploader stops behind its keyframes.
static int hba_bottom_workers(vba_ctx *c, const HbaPlan &P, const HbaCall &A, double *d_all, double *d_sub, double *d_rep, std::vector<double> &meta, HbaSubmaps &S) {
  while ((int)c->hba_workers.size() < P.KL - 1) {
    vba_options o = c->opt; o.stream = nullptr; o.device = c->device;
    vba_ctx *w = nullptr;
    const int stc = vba_create(&o, &w);
    if (stc) { c->set_error("vba_hba_global: could not create a worker context"); return stc; }
    c->hba_workers.push_back(w);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int w = 0; w < P.n_win; w++) P.rec(meta.data(), w)[2] = -1.0;             // "not run"
  std::vector<std::string> werr(P.KL);
  std::atomic<int> kf_ready{0}, stop_after{P.n_win};
  auto work = [&](int lane) {
    vba_ctx *cx = lane == 0 ? c : c->hba_workers[lane - 1];
    hipSetDevice(c->device);
    std::vector<int> ccnt(P.n_win_max > 0 ? P.n_win_max : 1);                    // (every lane its own, lane 0 too: see vba_hba_global)
    for (int w = lane; w < P.n_win; w += P.KL) {
      if (!hba_gate(kf_ready, P.win[w].start + P.wdsize, stop_after, w)) return;
      if (hba_window(cx, P, w, A, d_all, hba_chunk_cloud(P, d_rep, w), P.rec(meta.data(), w), ccnt) != VBA_OK) { werr[lane] = cx->err; hba_stop_at(stop_after, w); return; }
    }
  };
  // (one uploader: three threads staging chunks in turn moved the pageable copy no faster — 4-5 GB/s either way; at full length
  //  the call is bound by this copy once the windows overlap it)
  auto upload = [&]() -> int {
    hipStream_t up = nullptr;
    if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) return VBA_ERR_HIP;
    const int CH = 16;                                                           // keyframes per chunk
    int st = VBA_OK;
    for (int k0 = 0; k0 < A.n_kf && st == VBA_OK; k0 += CH) {
      if (!hba_upload_wanted(P, stop_after.load(), k0)) break;                   // the keyframes of the lowest failing window are up
      const int k1 = k0 + CH < A.n_kf ? k0 + CH : A.n_kf;
      const size_t o0 = (size_t)A.offsets[k0] * 3, nb = (size_t)(A.offsets[k1] - A.offsets[k0]) * 3 * sizeof(double);
      if (nb > 0 && (hipMemcpyAsync(d_all + o0, A.pnt_local + o0, nb, hipMemcpyDefault, up) != hipSuccess || hipStreamSynchronize(up) != hipSuccess)) st = VBA_ERR_HIP;
      else kf_ready.store(k1, std::memory_order_release);
    }
    hipStreamDestroy(up);
    return st;
  };
  const int st = hba_run_lanes(P.KL, stop_after, work, upload);
  hipSetDevice(c->device);
  if (st) { c->set_error(st == VBA_ERR_CAPACITY ? "vba_hba_global: out of host memory in a worker lane" : "vba_hba_global: uploading the keyframe clouds or starting the worker lanes failed"); return st; }
  return hba_collect(c, P, A, meta, d_sub, d_rep, S, &werr);
}

// More than one rank ("windows are independent problems => replicas across GPUs for the bottom layer"): window w is
// optimised by rank w % n_ranks with the exchange step switched off; every rank packs its windows' clouds and records into ITS chunk
// of two buffers, and one ALL-GATHER of each hands every rank all of them (a rank receives each foreign byte once).  A window that
// fails on one rank travels as its status word: every rank goes on, enters both collectives and all of them return the same error
// afterwards — no rank is left waiting in a collective.  The top-level window then runs replicated (identical inputs on every rank).
static int hba_bottom_replicas(vba_ctx *c, const HbaPlan &P, const HbaCall &A, double *d_all, double *d_sub, double *d_rep, double *d_meta, std::vector<int> &ccnt,
                               std::vector<double> &meta, HbaSubmaps &S) {
  {
    struct Restore { vba_ctx *c; bool was; ~Restore() { c->collective_off = was; } } restore{c, c->collective_off};
    c->collective_off = true;                                                    // the windows' own LM loops must not enter a collective
    for (int w = 0; w < P.n_win; w++)
      if (P.win[w].lane == c->rank) hba_window(c, P, w, A, d_all, hba_chunk_cloud(P, d_rep, w), P.rec(meta.data(), w), ccnt);   // its status travels with the gather
  }
  if (P.meta_chunk > 0)
    HIPCHK(c, hipMemcpyAsync(P.lane_recs(d_meta, c->rank), P.lane_recs(meta.data(), c->rank), P.meta_chunk * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int rc = ctx_allgather(c, d_rep, P.chunk_pts * 3);
  if (rc) return rc;
  rc = ctx_allgather(c, d_meta, P.meta_chunk);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(meta.data(), d_meta, meta.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return hba_collect(c, P, A, meta, d_sub, d_rep, S, nullptr);
}

// The top-level window over all submaps with their CURRENT poses: edges2, indices looked up in the submaps' first keyframes.
static int hba_top(vba_ctx *c, const HbaCall &A, const double *d_sub, const HbaSubmaps &S) {
  const int ns = (int)S.first.size();
  if (ns < 2) return VBA_OK;
  std::vector<int> off(ns + 1, 0);
  for (int i = 0; i < ns; i++) off[i + 1] = off[i] + S.n[i];
  std::vector<double> xs((size_t)ns * 12), e2((size_t)(ns * (ns - 1) / 2 + 1) * 20);
  for (int i = 0; i < ns; i++) std::memcpy(&xs[(size_t)i * 12], A.poses_now + (size_t)S.first[i] * 12, 12 * sizeof(double));
  int ne = 0;
  const int st = vba_hba_add_edge(c, ns, off.data(), d_sub, xs.data(), A.voxel_size, A.min_eig, A.eig, A.total_max_iter, 5, e2.data(), &ne, nullptr, nullptr, nullptr,
                                  nullptr, nullptr);
  if (st) return st;
  return hba_append_edges(A.edges2, A.cap2, A.n2, e2.data(), ne, [&S](double i) { return (double)S.first[(int)i]; });
}

int vba_hba_global(vba_ctx *c, int n_kf, const int *offsets, const double *pnt_local, const double *poses_x0, const double *poses_now,
                   double gba_voxel_size, double gba_min_eigen_value, const double *gba_eigen_value_array, int total_max_iter, int wdsize, int mgsize,
                   double *edges1_out, int cap1, int *n_edges1, double *edges2_out, int cap2, int *n_edges2) try {
  if (n_kf < 0 || wdsize < 2 || mgsize < 1 || !offsets || !poses_x0 || !poses_now || !gba_eigen_value_array || !n_edges1 || !n_edges2 ||
      (offsets[n_kf] > 0 && !pnt_local))
    return VBA_ERR_BAD_ARG;
  *n_edges1 = 0; *n_edges2 = 0;
  const HbaPlan P = hba_plan(n_kf, offsets, wdsize, mgsize, c->collective() && c->n_ranks > 1 ? c->n_ranks : 1, c->opt.hba_workers);
  HIPCHK(c, c->d_hba_all.ensure(P.need));
  double *d_all = c->d_hba_all, *d_sub = d_all + P.off_sub, *d_rep = d_all + P.off_rep, *d_meta = d_all + P.off_meta;
  const HbaCall A{n_kf, offsets, pnt_local, poses_x0, poses_now, gba_voxel_size, gba_min_eigen_value, gba_eigen_value_array, total_max_iter,
                  edges1_out, cap1, n_edges1, edges2_out, cap2, n_edges2};
  int st = P.mode == HBA_WORKERS ? VBA_OK : hba_upload_all(c, P, A, d_all);       // (in one copy; the worker driver uploads in chunks, under its first windows)
  if (st) return st;
  HbaTimes times(c);
  HbaSubmaps S;
  // The cloud-count scratch of the sequential and the replica driver, then the records of the chunked modes (none one after the other).
  // Both are allocated here in every mode and live to the end of the call, as they always have.  The worker driver does not use the
  // scratch (every lane has its own), but its 2 MB decide where glibc trims the heap between the call's 12.7 MB buffers: without
  // them every second full-length call took 25 ms longer (profiles/README.md).
  std::vector<int> ccnt(P.n_win_max > 0 ? P.n_win_max : 1);
  std::vector<double> meta(P.meta_len, 0.0);
  st = P.mode == HBA_WORKERS ? hba_bottom_workers(c, P, A, d_all, d_sub, d_rep, meta, S)
     : P.mode == HBA_REPLICAS ? hba_bottom_replicas(c, P, A, d_all, d_sub, d_rep, d_meta, ccnt, meta, S) : hba_bottom_sequential(c, P, A, d_all, d_sub, ccnt, S);
  if (st) return st;
  times.windows_done();
  return hba_top(c, A, d_sub, S);
} catch (const std::bad_alloc &) {                  // a std::vector of the plan, the records or a driver: nothing crosses the ABI
  c->set_error("vba_hba_global: out of host memory");
  return VBA_ERR_CAPACITY;
} catch (...) {
  c->set_error("vba_hba_global: unexpected exception");
  return VBA_ERR_HIP;
}

}  // extern "C"
