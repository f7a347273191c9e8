// The scan passes of vba_kf.hip (vba_kernels_scan.hpp) that other units chain on buffers of their own: the scan frame of vba_scan.hip,
// the kd-tree re-sampler of vba_odom.hip, the initialisation window of vba_init.hip.  Declarations only: the keyframe store itself is
// vba_kf_store.hpp.
#pragma once
#include "vba_ctx.hpp"

namespace vba {
int ds_core(vba_ctx *c, hipStream_t stream, int mode, int n, const double *d_in, const double *d_var, int vrow, int vstep, double voxel_size,
            bool det, const DsWork &w);
size_t kf_ws_layout(vba_ctx *c, int n, bool det, char *base, DsWork *w, int *status);
__global__ void k_iota(int *__restrict__ a, int n);
__global__ __launch_bounds__(256) void k_ds_scan(int nb, int *__restrict__ blk, int *__restrict__ n_out);
__global__ __launch_bounds__(256) void k_ds_emit(int n, const DsSlot *__restrict__ tab, const int *__restrict__ slot_of, const int *__restrict__ blk,
                                                 double *__restrict__ out, int *__restrict__ count, int *__restrict__ first, double *__restrict__ vout, int mode);
__global__ void k_undistort(int n, double *__restrict__ pnt, const double *__restrict__ curv, int m, const double *__restrict__ prm);
__global__ void k_var_init(int n, const double *__restrict__ pin, double *__restrict__ pout, double *__restrict__ var, const double *__restrict__ ext,
                           float range_inc, float degree_inc);
}  // namespace vba
