// Scan log (vba_scanlog_*): the capture of one scan of the map's ring into the log's arena, and the float form of a
// stored scan (pl_save of save_pcd, VS:172-174).  Both are streaming copies: lanes on consecutive doubles, a capped grid that
// strides over the rest, every index formed in 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vba {

// One launch over both arrays of a scan of n points: doubles [0, 3n) are the points, [3n, 12n) the covariance rows.  src_var ==
// nullptr (the map holds no covariances) writes zeros.  Source and destination are the first double of the scan in each array.
__global__ __launch_bounds__(256) void k_scanlog_copy(long long n, const double *__restrict__ src_pnt, const double *__restrict__ src_var,
                                                      double *__restrict__ dst_pnt, double *__restrict__ dst_var) {
  const long long np = 3 * n, total = 12 * n, step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    if (i < np) dst_pnt[i] = src_pnt[i];
    else dst_var[i - np] = src_var ? src_var[i - np] : 0.0;
  }
}

// xyz[i] = (float)pnt[i] for the 3n coordinates of a scan: each narrowed once
__global__ __launch_bounds__(256) void k_scanlog_narrow(long long n3, const double *__restrict__ pnt, float *__restrict__ xyz) {
  const long long step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n3; i += step) xyz[i] = (float)pnt[i];
}

}  // namespace vba
