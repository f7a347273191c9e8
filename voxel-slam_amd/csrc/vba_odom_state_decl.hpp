// What vba_odom.hip defines around the odometry state (vba_kernels_imu_ekf.hpp) and units that never read the state's fields call:
// the map launches k_odom_state_pose on the state block it is handed.  Declarations only: the state itself is vba_odom_state.hpp.
#pragma once
#include "../../include/voxelba.h"

#include <hip/hip_runtime.h>
#include <string>

namespace vba {
// Orders `stream` behind the work queued on the state's buffers by its last user.
int odom_state_order(vba_odom_state *st, hipStream_t stream, std::string &err);
// the map's pose image from the state block, launched by map_cut_voxel
__global__ __launch_bounds__(64) void k_odom_state_pose(const double *blk, double *poses);
}  // namespace vba
