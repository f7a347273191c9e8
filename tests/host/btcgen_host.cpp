// Host build of the plane fit of descriptor generation (voxel-slam_amd/csrc/vba_btcgen_fit.hpp: the project's 3x3 solver in its
// IEEE variant plus the Jacobi fallback and the normal's sign rule) for tests/btc_gen_oracle.py.  Compiled with -ffp-contract=off,
// as the device build is, so that both give the same bits.  Test harness only.
#include "../../voxel-slam_amd/csrc/vba_btcgen_fit.hpp"
extern "C" void btcg_plane_eig_host(int n, const double *cov6, double *wmin, double *normal, int *direct) {
  for (int i = 0; i < n; i++) {
    const double *a = cov6 + 6 * (size_t)i;
    direct[i] = vba::btcg_plane_eig(a[0], a[1], a[2], a[3], a[4], a[5], wmin[i], normal + 3 * (size_t)i);
  }
}
