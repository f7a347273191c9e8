// The voxel map of libvoxelba.so: the kernels and the map_* host functions of vba_kernels_map.hpp, vba_kernels_loop.hpp and
// vba_kernels_odom.hpp (the resident EKF loop runs the map's point loop), compiled here and nowhere else; the other units reach the map
// through the declarations in vba_ctx.hpp.
#include "vba_ctx.hpp"
#include "vba_kernels_map.hpp"
#include "vba_kernels_loop.hpp"
#include "vba_kernels_odom.hpp"
