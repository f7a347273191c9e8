// Host interface of BTC descriptor generation on the device (GenerateSTDescs, BTC.cpp:156-203; kernels in vba_btcgen.hip, a
// translation unit of its own compiled with -ffp-contract=off).  One call is one stream-ordered sequence: voxel pass, plane fit and
// plane-cloud compaction into the database's cloud storage, projection-plane selection, extract_binary per selected plane,
// non-maximum suppression and top-N, triangles with their dedupe.  The order contract is DESIGN.md §11 and include/voxelba.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

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

struct BtcGen {
  size_t pts_cap = 0, cell_cap = 0, corn_cap = 0, cand_cap = 0, sort_bytes = 0;
  int allocs = 0;                    // device and pinned-host allocations made so far (plane-cloud growth of the database included)
  size_t dev_bytes = 0;
  // point-indexed
  float *xyz = nullptr, *sxyz = nullptr;
  unsigned long long *key = nullptr, *skey = nullptr;
  int *idx = nullptr, *sidx = nullptr, *flag = nullptr;
  unsigned *ckey = nullptr, *sckey = nullptr;
  double *px = nullptr, *py = nullptr, *pd = nullptr;
  void *sort_tmp = nullptr;
  // voxel / plane scratch (bounded by the point count)
  int *vstart = nullptr, *vlen = nullptr, *isc = nullptr, *isp = nullptr, *ids = nullptr, *ids2 = nullptr, *first = nullptr;
  char *planes = nullptr;            // BgPlane [5][pts_cap / (voxel_init_num + 1) + 1]: candidates, planes, groups, sorted, merged
  size_t plane_cap = 0;
  // projection images
  int *ccnt = nullptr, *cdis = nullptr; double *csx = nullptr, *csy = nullptr; unsigned long long *cbits = nullptr;
  char *sel = nullptr; unsigned long long *mm = nullptr;
  BgCorner *corn = nullptr, *corn2 = nullptr, *corn3 = nullptr;
  // triangles
  BgStd *cand = nullptr, *stds = nullptr; unsigned long long *ckeys = nullptr, *htab = nullptr; int *hmin = nullptr, *cslot = nullptr;
  int *cnt = nullptr;
  // pinned read-back
  int *h_cnt = nullptr; BgStd *h_stds = nullptr; BgCorner *h_corn = nullptr; size_t h_std_cap = 0, h_corn_cap = 0;
};

// grow the buffers for n points, `cells` image cells, `corners` temporary corners and `stds` triangle candidates (0 keeps a size)
hipError_t btcgen_reserve(BtcGen &g, size_t n, size_t cells, size_t corners, size_t stds, int vinit, hipStream_t st);
// enqueue one GenerateSTDescs over n >= 1 host points (h_xyz == nullptr: the caller has already enqueued the writes of the
// points into g.xyz on st); the plane cloud goes to pc_dst (room for n / (vinit + 1) + 1 points) and
// its end offset (have + planes) to *off_slot; the counters, triangles and corners land in g.h_cnt / h_stds / h_corn after the
// caller synchronises the stream
hipError_t btcgen_enqueue(BtcGen &g, const BgCfg &cfg, int n, const float *h_xyz, float *pc_dst, int *off_slot, int have, hipStream_t st);
void btcgen_free(BtcGen &g);

}  // namespace vba
