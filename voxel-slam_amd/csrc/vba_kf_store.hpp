// Private header of the units that read a keyframe store ("Source layout": where state lives): the handle struct of
// vba_kf.hip.  It defines no kernel.
#pragma once
#include "vba_ctx.hpp"
#include "vba_kf_store_decl.hpp"

// keyframe store (vba_kf.hip); the loop map reads its clouds and poses
struct vba_kf_store {
  vba_ctx *ctx = nullptr;
  // the keyframes: points (their own frame, float values in doubles) and covariance diagonals, ragged by off
  DevMem<double> d_pnt; DevMem<float> d_var; size_t cap = 0;
  std::vector<int> off{0};
  struct Meta { double x0[12]; int id; double jour; int exist; };
  std::vector<Meta> kf;
  // scratch of one merge of up to mcap points: staged host input, merged cloud (also the world points of a load), gathered covariance
  // diagonals, per-voxel counts, the down-sampler's work area; pinned: gathered diagonals of a host covariance array
  size_t mcap = 0;
  DevMem<double> d_src, d_merge, d_mdiag; PinMem<double> h_diag;
  DevMem<int> d_cnt; DevMem<char> d_ws;
  // per-scan transforms [tcap][12] and offsets [tcap + 1]: pinned image and device copy; the voxel count of a build (pinned)
  int tcap = 0; PinMem<char> h_tab; DevMem<char> d_tab; PinMem<int> h_n;
  hipEvent_t ev = nullptr;
  int allocs = 0; int64_t bytes = 0;
  int hist = 0; std::vector<float> hist_pos;   // history_kfsize, pl_kdmap
  int last_m = 0;                              // voxels of the last build (their counts stay in d_cnt)
};
