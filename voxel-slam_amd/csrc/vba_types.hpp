// Plain structs that a host-side struct holds by value or that cross a translation-unit boundary: views of device arrays passed to
// kernels by value and the small records kernels and host code share (the stores that own the arrays are host code: vba_stores.hpp).
// No kernel and no device function is defined here, so every unit may include it ("source layout").
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/voxelba.h"

#define VBA_MAX_WIN_DEV VBA_MAX_WIN

namespace vba {

// ---------------------------------------------------------------- factor store (vba_kernels_factor.hpp)
struct FactorView {
  double *cl;      // [10][W][vs]   body-frame clusters per (frame, voxel): Pxx,Pxy,Pxz,Pyy,Pyz,Pzz,vx,vy,vz,N
  double *fix;     // [10][vs]      sig_vecs (fixed world cluster)
  double *coe;     // [vs]
  double *eigval;  // [3][vs]
  double *eigvec;  // [9][vs]       row-major r*3+c, column c = eigenvector c
  double *pcr;     // [10][vs]      pcr_adds
  unsigned int *occ;   // [vs]      bit i set <=> slot (voxel, frame i) holds points (cl N != 0): what the residual pass tests instead of
                       //           reading the N of all W slots (4 B per voxel instead of 8 W); kept current by k_factor_mask
  int *tiles;      // Hessian-pass tile table (k_factor_tiles): [0] = number of tiles, then (first voxel, voxels, union mask, 0) from [4]
  int vs;          // voxel stride (capacity)
  int W;
};

// ---------------------------------------------------------------- LM loop (vba_kernels_lm.hpp, vba_kernels_li.hpp)
constexpr int LM_SPEC = 4;           // damping candidates solved per launch of the solve kernel (one workgroup each)
struct LmDev;
struct LiDev;

// ---------------------------------------------------------------- voxel map (vba_kernels_map.hpp, vba_kernels_loop.hpp)
struct MapParams {
  int W, max_layer, max_points, thread_num;
  double voxel_size, min_eigen_value;
  double plane_thre[4], min_point[4];
  int mp[VBA_MAX_WIN];
  int rank, n_ranks;
};

struct MapView {
  // hash table of roots
  unsigned long long *hkeys; int *hvals; unsigned int hmask;
  // nodes
  int cap;
  unsigned long long *nkey; int *nroot; int *nparent; int *nchild; int *npath; int *nopt; int *nflist /* factor index -> leaf (tras_opt order) */; int *nfl2 /* the same before the occupancy sort */; unsigned int *nfkey; int *fhist /* [EXTRACT_NB_MAX] */; int *nlast; int *nstamp; int *nsplit; int *ntake; int *nclear; int *ndead;
  int *nfree_root, *nfree_blk;   // stacks of recycled node ids: single root nodes / bases of 8-node child blocks (map_prune)
  int *ndet, *dblk;              // deterministic mode: [cap] split flags of a recut level / [cap] per-workgroup counts of a compaction
  unsigned int *hfirst;          // deterministic mode: [hash cap] smallest index of an input point of a root created by the current insert
  int *nseg_a, *nseg_b;          // [W][cap]: the points a scan slot gave to a leaf AT INSERTION = perm[slot][nseg_a .. nseg_b) (scan order)
  int *ncnt;                     // [cap] points of the scan being inserted per leaf, then the scatter cursor; zero between inserts
  int *nsl;                      // [cap] leaves split by the current recut level (margi: leaves whose oldest frame joins the fixed points)
  int *nfb_head, *nfb_tail;      // [cap] a leaf's fixed points (point_fix) arrive in BLOCKS of consecutive pool entries; the blocks are chained in arrival order
  signed char *nlayer; signed char *nstate;
  unsigned char *f_exist, *f_sw, *f_plane, *f_touched; int *f_slide;
  float *nql; double *ncenter; double *njour;
  double *nadd, *nfix, *ncov, *neval, *nevec, *nplane, *nlc;
  // scan ring
  int max_pts;
  double *px;   // [W][max_pts][3]  (AoS: the per-leaf kernels gather whole points by index)
  double *pvar; // [W][max_pts][9]
  int *pnode;   // [W][max_pts]
  int *phash;   // [max_pts] temp
  int *newslots;  // [max_pts] temp
  int *perm;    // [W][max_pts] point indices of a slot grouped by insertion leaf, scan order inside a group
  // the slot's points IN THAT ORDER (what sw->points[mord] of the leaves hold in the reference): the passes that walk a leaf's points again
  // (subdivide, the move of the oldest frame to point_fix) stream them instead of chasing perm -> point
  double *sx;   // [3][W][max_pts]
  double *svar; // [9][W][max_pts]
  int *pleaf;   // [W][max_pts] the leaf that holds the point NOW (-1: none / released)
  unsigned int *skey_a, *skey_b;   // [max_pts] sort keys (leaf id) in / out
  int *sval_a;  // [max_pts] sort values in (the point index)
  int *wl;      // [max_pts] leaves that received points of the scan being inserted
  int *wlb;     // [max_pts] those with more than 64 points
  int4 *wl4;    // [max_pts] work list entries (leaf, segment start, points, -) for the per-leaf kernels: one 16-byte load
  // fixed-point pool
  int cap_fix;
  double *fx;   // [cap_fix][3]  (AoS, as the window points: a leaf's block is one contiguous run)
  double *fvar; // [cap_fix][9]
  int *fnode;
  int *fb_base, *fb_len, *fb_next;   // [cap_fix] block table of the pool (a block has >= 1 point)
  int *sval_b;  // [max_pts] sort values out where the destination is not a slot's perm (fixed-point insertion)
  int *cnt;     // counters [CNT_N]
  double *poses;  // [W][12]
};

enum { FIXCOV_KEEP = 0, FIXCOV_DIAG_F32 = 1, FIXCOV_FULL_F64 = 2, FIXCOV_ZERO = 3 };

struct OdomState { double R[9], t[3], rot_var[9], tsl_var[9]; };

// ---------------------------------------------------------------- global BA (vba_kernels_gba.hpp, vba_kernels_big.hpp)
struct GbaView {
  unsigned long long *hkeys; int *hvals; unsigned int hmask;
  int cap, W, npts;
  double *nadd;     // [10][cap]     world cluster (pcr_add)
  double *nlc;      // [10][W][cap]  body clusters per keyframe
  double *ncenter;  // [3][cap]
  float *nql;       // [cap]
  int *nchild, *nfac;
  signed char *nlayer;
  double *neval, *nevec;   // [3][cap], [9][cap]
  double *pw;       // [3][npts] world points
  const double *pl; // [npts][3] local points (caller's layout)
  int *pframe, *pnode;
  int *cnt;
  double *poses;    // [W][12]
  int *offsets;     // [W+1]
};

struct GbaParams { double voxel_size, min_eigen_value, eig_array[4]; int max_layer; };

struct BigView {
  int W, V, E, capV, capE;
  int *vptr;        // [V + 1]
  int *efr, *evox;  // [E] frame / voxel of an entry
  double *ecl;      // [10][capE] body clusters
  double *gv;       // [18][capE] g1, g2, h of an entry (Hessian pass scratch)
  double *eval, *evec, *pcr;   // [3][capV], [9][capV], [10][capV]
  double *poses;    // [W][12]
  double *H, *g, *r;   // dense (6W)^2, 6W, 1
  int *eidx;           // [V][W] entry of (voxel, frame) or -1 (k_big_syrk operand staging)
  double *es;          // [27][capE] diagonal-block remainder E (21 upper) + gradient (6) of an entry, summed per frame by k_big_diag
};

struct GbaBigView {
  // roots
  unsigned long long *hkeys; int *hvals; unsigned int hmask;
  // nodes
  int cap, W, npts;
  double *nadd, *ncenter, *neval, *nevec;
  float *nql;
  int *nchild, *nfac, *nexi;
  signed char *nlayer;
  // (node, frame) entries
  unsigned long long *ekeys; unsigned int emask; double *ecl;   // [10][emask + 1]
  // points
  double *pw; const double *pl; int *pframe, *pnode;
  int *perm;                   // points ordered by root voxel (the accumulation pass walks them in this order: see k_gbab_accum)
  unsigned int *skey; int *sval;   // sort input: root id (all ones = no root) / point index
  int *cnt; double *poses; int *offsets;
};

// ---------------------------------------------------------------- scan pre-processing (vba_kernels_scan.hpp)
struct DsSlot {
  unsigned long long key;      // packed voxel index, DS_EMPTY when free
  double sx, sy, sz;
  double vx, vy, vz;           // down_sampling_pvec: sums of the covariance diagonals
  unsigned long long mind;     // down_sampling_close: smallest squared distance to the centroid (bits of a non-negative double)
  int cnt, first, best, pad;
};

// The device half of the down-samplers: everything between the input and the emit, on buffers the caller owns.
//   tab [cap] slots (cap a power of two >= 2n), slot [n], blk [(n + 255) / 256], n_out [1]; dist [n] for mode 2;
//   deterministic mode: skey / idx / sidx [n] and rocPRIM scratch tmp (sort_pairs_u32 over n keys of key_bits bits).
// After it the table holds every voxel's sums, count and first point, blk the exclusive scan of the per-block voxel counts and
// *n_out the number of voxels: what k_ds_emit (and the keyframe store's k_kf_emit) compact in first-occurrence order.
struct DsWork {
  DsSlot *tab = nullptr; int cap = 0; unsigned int key_bits = 0;
  int *slot = nullptr, *blk = nullptr, *n_out = nullptr; double *dist = nullptr;
  unsigned int *skey = nullptr; int *idx = nullptr, *sidx = nullptr; void *tmp = nullptr; size_t tmp_bytes = 0;
};

// ---------------------------------------------------------------- loop retrieval (vba_kernels_btc.hpp)
struct BtcStds {                     // descriptor rows, SoA (a database, or the uploaded query)
  double *tri, *cen, *loc;           // [cap][3], [cap][3], [cap][9] (locations of A, B, C)
  unsigned long long *bits;          // [cap][3]  occupy_array_ of A, B, C as bit masks
  int *summ;                         // [cap][3]  summary_ of A, B, C
  int *frame;                        // [cap]     frame_number_
};

struct BtcIndex {                    // the cell index of a database
  const int *tab; int mask;          // [mask + 1][8]
  const int *ent;                    // [chunks][64] descriptor indices
  const int *next;                   // [chunks]     next chunk of the same cell, -1 = last
};

struct BtcCfgDev { int skip_near, cand_num; double rough, sim, icp, normal, dis; };

struct BtcIcpDev {
  double R[9], t[3], paras[4];
  int is_conv, done, iters, pad;
  double mat[6];            // mat_norm of the last iteration (xx xy xz yy yz zz)
  double eig[3];
};

}  // namespace vba
