// The voxel key of the down-samplers (tools.hpp:201-238, voxel_map.cpp:39-83) and the hash of their open-addressing tables, written
// once for the device (the k_ds_* and k_vx_* kernels, the surfel map of vba_kernels_surfreg.hpp) and for the g++ build of
// tests/host/surfreg_host.cpp.  No kernel.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VBK_HD __host__ __device__ __forceinline__
#else
#define VBK_HD inline
#endif

namespace vba {

static constexpr unsigned long long DS_EMPTY = ~0ull;

// TL:210-217 on PCL float coordinates; dbl != 0: the pointVar form of VM:45-51 (double coordinates)
VBK_HD long long ds_axis_key(double v, double voxel_size, int dbl = 0) {
  float loc = (float)((dbl ? v : (double)(float)v) / voxel_size);
  if (loc < 0) loc = (float)((double)loc - 1.0);
  return (long long)loc;
}
VBK_HD unsigned long long ds_pack(long long x, long long y, long long z) {
  return ((unsigned long long)(x & 0x1FFFFF) << 42) | ((unsigned long long)(y & 0x1FFFFF) << 21) | (unsigned long long)(z & 0x1FFFFF);
}
VBK_HD unsigned int ds_hash(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return (unsigned int)k;
}

}  // namespace vba
