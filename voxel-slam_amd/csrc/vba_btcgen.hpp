// Host interface of BTC descriptor generation on the device (GenerateSTDescs, BTC.cpp:156-203; kernels in vba_btcgen.hip, a
// translation unit of its own compiled with -ffp-contract=off).  One call is one stream-ordered sequence: voxel pass, plane fit and
// plane-cloud compaction into the database's cloud storage, projection-plane selection, extract_binary per selected plane,
// non-maximum suppression and top-N, triangles with their dedupe.  The order contract is DESIGN.md §11 and include/voxelba.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "vba_mem.hpp"

namespace vba {

constexpr int BG_MAX_PROJ = 8;       // proj_plane_num_ upper bound
constexpr int BG_MAX_K = 32;         // descriptor_near_num_ upper bound
constexpr int BG_MAX_CELLS = 1 << 24;   // projection image cells (x_axis_len * y_axis_len); larger images are refused

struct BgCfg {                       // ConfigSetting fields read by GenerateSTDescs, float ones promoted to double
  int useful, vinit, proj_num, line_filter, touch_filter, K, cut_num;
  double merge_n, merge_d, detect, vsize, res, high_inc, dmin, dmax, summ_min, min_len, max_len, scale;
  float nms_r2;                      // (float)(r * r): FLANN's radius test
};

// device counters (ints) of one call
enum { BGC_NVOX = 0, BGC_NCAND, BGC_NPL, BGC_NG, BGC_NM, BGC_NSEL, BGC_NTEMP, BGC_NCORN, BGC_NSTD, BGC_ERR, BGC_CELLS, BGC_CUR,
       BGC_JMIN, BGC_KEPT0, BGC_N = BGC_KEPT0 + BG_MAX_PROJ };

struct BgStd { double tri[3], cen[3]; int a, b, c, pad; };      // corner indices of A, B, C into the final corner list
struct BgCorner { double loc[3]; unsigned long long bits; int summ, pad; };

// Five capacity groups and a fixed one, each array an owning member (vba_mem.hpp).  A group grows as a whole, contents not kept, and
// is complete or empty: a failed growth leaves it empty with its capacity at 0, so the next reserve allocates it again.
struct BtcGen {
  size_t pts_cap = 0, plane_cap = 0, cell_cap = 0, corn_cap = 0, cand_cap = 0, sort_bytes = 0;
  int allocs = 0;                    // device and pinned-host allocations made so far (plane-cloud growth of the database included)
  size_t dev_bytes = 0;
  struct Pts {                       // [pts_cap]: point-indexed, the voxel scratch bounded by the point count, the sort scratch
    DevMem<float> xyz, sxyz;
    DevMem<unsigned long long> key, skey;
    DevMem<int> idx, sidx, flag;
    DevMem<unsigned> ckey, sckey;
    DevMem<double> px, py, pd;
    DevMem<int> vstart, vlen, isc;
    DevMem<char> sort_tmp;
  } pts;
  struct Planes {                    // [plane_cap = pts_cap / (voxel_init_num + 1) + 1]
    DevMem<char> planes;             // BgPlane [5][plane_cap]: candidates, planes, groups, sorted, merged
    DevMem<int> isp, ids, ids2, first;
  } pln;
  struct Cells { DevMem<int> ccnt, cdis; DevMem<double> csx, csy; DevMem<unsigned long long> cbits; } cel;   // [cell_cap] projection images
  struct Corners { DevMem<BgCorner> corn, corn2, corn3; PinMem<BgCorner> h_corn; } cor;                        // [corn_cap]
  struct Cands {                     // [cand_cap] triangles
    DevMem<BgStd> cand, stds; DevMem<unsigned long long> ckeys; DevMem<int> cslot;
    DevMem<unsigned long long> htab; DevMem<int> hmin;   // [2 cand_cap]
    PinMem<BgStd> h_stds;
  } tri;
  // fixed size: counters, per-projection min/max and selection, the counters' pinned read-back (allocated last: it marks the four as there)
  DevMem<int> cnt; DevMem<unsigned long long> mm; DevMem<char> sel;
  PinMem<int> h_cnt;
};

// grow the buffers for n points, `cells` image cells, `corners` temporary corners and `stds` triangle candidates (0 keeps a size)
hipError_t btcgen_reserve(BtcGen &g, size_t n, size_t cells, size_t corners, size_t stds, int vinit, hipStream_t st);
// enqueue one GenerateSTDescs over n >= 1 host points (h_xyz == nullptr: the caller has already enqueued the writes of the
// points into g.pts.xyz on st); the plane cloud goes to pc_dst (room for n / (vinit + 1) + 1 points) and
// its end offset (have + planes) to *off_slot; the counters, triangles and corners land in g.h_cnt / tri.h_stds / cor.h_corn after the
// caller synchronises the stream
hipError_t btcgen_enqueue(BtcGen &g, const BgCfg &cfg, int n, const float *h_xyz, float *pc_dst, int *off_slot, int have, hipStream_t st);

}  // namespace vba
