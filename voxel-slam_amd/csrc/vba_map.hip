// The voxel map of libvoxelba.so: the kernels and the map_* host functions of vba_kernels_map.hpp and vba_kernels_loop.hpp, compiled here
// and nowhere else; the other units reach the map through the declarations in vba_ctx.hpp.
#include "vba_ctx.hpp"
#include "vba_kernels_map.hpp"
#include "vba_kernels_loop.hpp"
