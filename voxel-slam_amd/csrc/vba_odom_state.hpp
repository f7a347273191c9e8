// Private header of the units that read an odometry state ("Source layout": where state lives): the handle struct of
// vba_odom.hip.  It defines no kernel.
#pragma once
#include "vba_ctx.hpp"
#include "vba_odom_state_decl.hpp"

// odometry state (vba_odom.hip); the scan frame reads its pose table in place
struct vba_odom_state {
  vba_ctx *ctx = nullptr;
  DevMem<double> d_blk;            // [state 25 | P 225 | 6 unused]
  // sized by cap IMU rows: the pose table [cap - 1][22] | end_pose 12 | extrinsic 12 (the parameter block of k_undistort), the upload
  // [parameters 16 | imu cap x 7] with its pinned image
  int cap = 0;
  DevMem<double> d_tab, d_up; PinMem<double> h_up;
  PinMem<double> h_blk;            // set / get / poses: one pinned block of max(256, table) doubles
  hipEvent_t up_ev = nullptr;      // behind the newest copy out of h_up or h_blk
  bool up_pending = false;
  hipEvent_t res_ev = nullptr;     // behind the result download of the scan-to-map update, ahead of the copy back into the block
  int n_poses = 0;                 // rows of the table that the last propagation wrote
  hipStream_t last = nullptr;      // the stream of the last call that queued work on the block
  int allocs = 0; int64_t bytes = 0;
};
