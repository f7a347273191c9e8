// libvoxelba.so, the surfel unit: the moment and fit passes of vba_kf_surfel_export, kernels in
// vba_kernels_surfel.hpp.  Compiled with -ffp-contract=off (csrc/Makefile): the order and rounding of every operation of these
// passes is part of the interface, and the fit matches a host build of vba_surfel_fit.hpp bit for bit.  The entry point, its
// argument checks and the work arrays are vba_kf.hip's, which runs the voxel export's front half first.
#include "vba_surfel_decl.hpp"
#include "vba_kernels_surfel.hpp"

#include <hip/hip_runtime.h>
#include <algorithm>

namespace vba {

int sf_run(const SfPass &p, int max_blocks, float4 *out, double *cov, int *counts, hipStream_t stream) {
  const long long nb = (p.n + 255) / 256;
  hipLaunchKernelGGL(k_sf_rank, dim3(p.nblk), dim3(256), 0, stream, p.n, p.per, p.tab, p.slot_of, p.min_count, p.blk, p.slot_of_row);
  if (p.skey) {
    hipLaunchKernelGGL(k_sf_mom_det, dim3((unsigned)nb), dim3(256), 0, stream, p.n, p.skey, p.sidx, (const VxSlot *)p.tab, p.nkf, p.kft, p.jump, p.sum,
                       p.min_count, p.mom);
  } else {
    const hipError_t e = hipMemsetAsync(p.mom, 0, (size_t)p.m * 6 * sizeof(double), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_sf_mom, dim3((unsigned)std::min<long long>(nb, max_blocks)), dim3(256), 0, stream, p.n, p.nkf, p.kft, p.jump,
                       (const VxSlot *)p.tab, p.slot_of, p.sum, p.min_count, p.mom);
  }
  hipLaunchKernelGGL(k_sf_fit, dim3((unsigned)((p.m + 255) / 256)), dim3(256), 0, stream, p.m, (const int *)p.slot_of_row, (const VxSlot *)p.tab, p.sum,
                     (const double *)p.mom, p.nkf, p.kft, out, cov, counts);
  return (int)hipGetLastError();
}

}  // namespace vba
