// The context state of the satellite units ("Source layout": where state lives): one member per owner.  The BA core, the map
// and global BA see a CtxSat only as the pointer vba_ctx::sat; vba_sat.hip makes and releases it.  It defines no kernel.
#pragma once
#include "vba_ctx.hpp"

struct CtxSat {
  // vba_odom.hip: the initialisation odometry's map and the scratch of vba_odom_lio_state_estimation_kdtree_resident
  struct Kd {
    DevMem<double> d_tree[2];     // pl_tree of the initialisation odometry (float-valued xyz), ping-pong for the re-sampling
    int n = 0, cur = 0;
    // scratch sized by the scan (planes, partials, candidates), scratch sized by map + scan (the re-sampler's count / first arrays and
    // work area); the loop's state and pinned image are odom.d / odom.h below.  allocs / bytes count these and the map's two halves,
    // cumulatively (a freed block is not subtracted).
    DevMem<char> d_scan; size_t scan_pts = 0;
    DevMem<char> d_ws; size_t ws_pts = 0;
    int allocs = 0; int64_t bytes = 0;
  } kd;
  // vba_odom.hip, vba_odom_lio_state_estimation_resident: the loop's device state, its pinned image (parameter block
  // up, result block down; also those of the kd-tree variant, §18) and the point loop's workgroup partials; grow-only
  struct Odom {
    DevMem<vbh::OdomEkf> d; PinMem<vbh::OdomEkf> h;
    DevMem<double> d_part;
  } odom;
  // vba_btc.hip, loop retrieval (vba_btc_*): the query upload, the per-(query, cell) counts and the ICP state are shared by the
  // context's databases
  struct Btc {
    DevMem<char> d_q; PinMem<char> h_q;
    DevMem<int> d_cnt;
    DevMem<BtcIcpDev> d_icp; PinMem<BtcIcpDev> h_icp;
    DevMem<unsigned long long> d_icpkey;
    DevMem<double> d_icppart;
  } btc;
  // vba_pgo.hip, pose-graph optimisation (vba_pgo_optimize): graph structure and per-update work areas, and the dense skeleton system;
  // grow-only
  struct Pgo {
    DevMem<char> d;
    DevMem<double> d_Ab;
  } pgo;
  // vba_kf.hip, vba_kf_export_world: the per-keyframe table (pinned upload ring, so that a call need not drain the
  // stream before it writes the next image, and the device copy) and the staging of host output; grow-only.  The events go with the
  // struct, which vba_destroy releases after the stream has drained.
  struct Exp {
    static const int kRing = 4;
    PinMem<char> h[kRing]; hipEvent_t ev[kRing] = {nullptr}; int next = 0;
    DevMem<char> d;                                       // keyframes
    DevMem<float4> d_out;                                 // records
    std::vector<long long> first; std::vector<int> kbase;   // host scratch: exported points before every keyframe, keyframes before every store
    ~Exp() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }      // (no copy of an Exp exists: its buffers forbid one)
  } exp;
  // vba_kf.hip, vba_kf_voxel_export: the work arrays of a sequence of up to `pts` records: the table and the sums
  // (slots_of(pts) entries each), every record's slot, the workgroup counts with the total behind them, the pinned image of that
  // total; a deterministic context also holds the sort arrays skey | idx | sidx (sort_stride bytes each) | rocPRIM scratch
  // (tmp_bytes) for `sort_pts` records.  Grow-only; allocs / bytes count these and what a call or reserve adds to the export's table
  // and staging.  vba_kf_surfel_export runs on the same arrays and adds, for `sf_vox` KEPT voxels, a row of six
  // moment sums and the slot of every output row; sf_allocs / sf_bytes count those two.
  struct {
    size_t pts = 0, sort_pts = 0, sort_stride = 0, tmp_bytes = 0;
    DevMem<char> tab, sort; DevMem<double> sum; DevMem<unsigned int> slot; DevMem<int> blk; PinMem<int> h_n;
    int allocs = 0; int64_t bytes = 0;
    size_t sf_vox = 0;
    DevMem<double> sf_mom; DevMem<int> sf_row;
    int sf_allocs = 0; int64_t sf_bytes = 0;
  } vx;
  // vba_init.hip, vba_motion_init: raw clouds (uploaded once per call), blurred rows, pose tables
  struct Init {
    DevMem<char> d;
  } init;
};
