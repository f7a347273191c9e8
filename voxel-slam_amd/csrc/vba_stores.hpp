// The host-side stores behind the views of vba_types.hpp: each holds the view its kernels take by value and, beside it, the owning
// members (vba_mem.hpp) of every block the view points into; the view is refreshed from the owners after a growth.  Host code only:
// the units reach it through vba_ctx.hpp, no kernel header includes it ("source layout").
#pragma once
#include "vba_types.hpp"
#include "vba_mem.hpp"
#include <functional>
#include <utility>
#include <vector>

namespace vba {

// ---------------------------------------------------------------- voxel map
struct DevArr {  // a [rows][cap] device array that can grow its cap keeping [rows][used]
  void **slot; size_t elem, rows;
};

// the map's memory, apart from the rest of MapStore so that map_free can empty it as a whole
struct MapMem {
  // the three array families, index-aligned with node_arrays / scan_arrays / fix_arrays (vba_map.hip); a family grows as a whole
  std::vector<DevMem<char>> node_mem, scan_mem, fix_mem;
  DevMem<unsigned long long> hkeys; DevMem<int> hvals; DevMem<unsigned int> hfirst;   // root table [hcap]; hfirst: deterministic mode
  DevMem<int> cnt, fhist; DevMem<double> poses;
  PinMem<int> h_cnt;
  PinMem<double> h_pose_ring;
  DevMem<char> d_stage;
  DevMem<char> d_sort_tmp;       // rocPRIM scratch, sized for max_pts pairs
  DevMem<double> d_gc;           // the 2-double scratch of the sharded map's all-reduce
  DevMem<int> d_whist;           // deterministic mode: the per-workgroup bucket histograms of the stable sort
  // the display export (vba_map_display.hip): plane index per node, the workgroup counts (nodes, then points), scan index -> position in
  // the slot per window point, the counts and poses on the device, their pinned partners, the device staging of a host result
  DevMem<int> disp_nidx, disp_blk, disp_inv, disp_cnt; DevMem<double> disp_poses; PinMem<char> disp_pin; DevMem<char> disp_stage;
};

struct MapStore : MapMem {
  vba_options opt;
  int rank = 0, n_ranks = 1;
  MapView v{};
  bool allocated = false;
  bool have_var = false;
  int mp[VBA_MAX_WIN];
  int npts[VBA_MAX_WIN];
  int epoch = 1, stamp = 1;
  unsigned int hcap = 0;
  // Inserts are enqueued without reading the counters back: the host keeps pessimistic upper bounds (every point may
  // create a root) and re-reads the true counters only when a bound would exceed a capacity.
  long long ub_nodes = 0, ub_roots = 0, ub_used = 0;   // ub_used: hash slots that are not EMPTY (live roots + tombstones)
  bool cnt_stale = false;
  hipEvent_t pose_ev[8] = {nullptr}; int pose_next = 0;
  int sort_tmp_for = 0;
  // sharded map: SUM all-reduce of n doubles in HBM over the ranks, stream-ordered (set by the context)
  std::function<int(double *, size_t)> allreduce;
  // per-call plane thresholds (vba_motion_init's relaxed values, VS:624-630): when set they replace opt's in every MapParams
  bool thr_override = false;
  double ovr_min_eigen_value = 0.0, ovr_plane_thre[4] = {0.0, 0.0, 0.0, 0.0};
  bool det = false;              // deterministic mode (vba_options::deterministic)
  int disp_allocs = 0; int64_t disp_bytes = 0;   // vba_map_display_allocations: cumulative, they outlive a map_free
};

// a fixed insertion whose points and covariances are in HBM already
struct FixSource {
  int nseg = 0;
  const int4 *d_seg = nullptr;        // [nseg] device
  const double *d_poses = nullptr;    // [.][12] device
  const double *d_pnt = nullptr;      // source rows [.][3]
  int cov_kind = FIXCOV_ZERO;          // FIXCOV_* of vba_kernels_map.hpp (not FIXCOV_KEEP: the pool tail is not zeroed here)
  const void *d_cov = nullptr;        // float [.][3] diagonals (VS:2614-2621) or double [.][9] rows, taken over unrotated (VS:1341-1344)
};

// ---------------------------------------------------------------- global BA
// Three groups that are re-allocated as a whole, each complete or empty (an empty group has its capacity at 0, so the next
// gba_build allocates it again): the node arrays [v.cap], the root table [cap_hash] and the point arrays [cap_pts].
struct GbaStore {
  GbaView v{};
  int cap_pts = 0, cap_hash = 0;
  struct Nodes { DevMem<double> nadd, nlc, ncenter, neval, nevec; DevMem<float> nql; DevMem<int> nchild, nfac; DevMem<signed char> nlayer; } nodes;
  struct Hash { DevMem<unsigned long long> keys; DevMem<int> vals; } hash;
  struct Pts { DevMem<double> pw, pl /* device copy of the local points [n][3] */; DevMem<int> pframe, pnode; } pts;
  DevMem<int> cnt, offsets; DevMem<double> poses;
  PinMem<int> h_cnt;
};

struct BigStore {
  int last_cap = 1 << 17;
  BigView b{};
  GbaBigView g{};
  // Device memory comes from an arena of large chunks that survives across builds (reset() rewinds it): an allocation and a free
  // of ~40 buffers per build, some of them 10^8 bytes, cost more than the kernels of a top-level window.  What arena() hands out
  // are views into the chunks.
  struct Chunk { DevMem<char> mem; size_t used = 0; };
  std::vector<Chunk> chunks;
  hipError_t arena(void **p, size_t bytes) {
    bytes = (bytes ? bytes : 8) + 255 & ~(size_t)255;
    for (Chunk &ck : chunks)
      if (ck.mem.n - ck.used >= bytes) { *p = ck.mem.p + ck.used; ck.used += bytes; return hipSuccess; }
    Chunk ck;
    hipError_t e = ck.mem.ensure(bytes > ((size_t)256 << 20) ? bytes : ((size_t)256 << 20));
    if (e != hipSuccess) return e;
    ck.used = bytes; *p = ck.mem.p;
    chunks.push_back(std::move(ck));
    return hipSuccess;
  }
  void reset() { for (Chunk &ck : chunks) ck.used = 0; b = BigView(); g = GbaBigView(); }
  PinMem<int> h_cnt;
  int *d_vcnt = nullptr, *d_fill = nullptr;
  double *d_Ab = nullptr, *d_Tb = nullptr; int *d_ord = nullptr;   // dense solver (allocated by big_build)
  double *d_vec = nullptr;                                          // [3 n + 6 W W]: diag(H) | g copy | dxi | cross-block diagonals
  int NP = 0, ld = 0;
};

}  // namespace vba
