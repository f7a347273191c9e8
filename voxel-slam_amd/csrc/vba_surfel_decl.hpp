// The surfel passes of vba_surfel.hip (vba_kernels_surfel.hpp) that vba_kf.hip chains behind the front half of its voxel export.
// Declarations only.
#pragma once
#include <hip/hip_runtime.h>
#include "vba_vx.hpp"

namespace vba {
// What the front half left on the device for a sequence of n records, and the kept voxels' work rows.
struct SfPass {
  long long n, per;                       // records of S; records per count / emit workgroup
  int nblk, nkf, jump, min_count, m;      // those workgroups, table rows, stride, filter, kept voxels
  const VxKf *kft; VxSlot *tab; const unsigned int *slot_of; const double *sum; const int *blk;
  const unsigned int *skey; const int *sidx;   // the sorted runs of a deterministic context, else nullptr
  int *slot_of_row; double *mom;          // [m], [m][6]
};
// rank, centred moments (deterministic when p.skey), fit and emit of p.m > 0 kept voxels on `stream`; out [m][3] float4, cov [m][6]
// or nullptr (may be p.mom), counts [m] or nullptr, all device memory.  Returns a hipError_t as int.
int sf_run(const SfPass &p, int max_blocks, float4 *out, double *cov, int *counts, hipStream_t stream);
}  // namespace vba
