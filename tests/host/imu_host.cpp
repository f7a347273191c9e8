// Host build of the IMU factor evaluation the LI-BA pass runs on the device (vbh::imu_residual_jacobian, vbh::imu_evaluate,
// vbh::inverse_pplu of csrc/vba_hostmath.hpp) and of the compact-image reader li_hb_get (csrc/vba_li_order.hpp) for the CPU checks of
// tests/test_imu_cpu.py against tests/imu_ref.py.  Test harness only.
#include "../../voxel-slam_amd/csrc/vba_hostmath.hpp"
#include "../../voxel-slam_amd/csrc/vba_li_order.hpp"
extern "C" void imu_host_covinv(const double *imu, double *cinv) { vbh::inverse_pplu(imu + 79, cinv, 15); }
// rr[15], joc[15 * nb] (zeroed here)
extern "C" void imu_host_rj(const double *imu, const double *s1, const double *s2, int with_g, double *rr, double *joc) {
  const int nb = with_g ? 33 : 30;
  for (int i = 0; i < 15 * nb; i++) joc[i] = 0.0;
  vbh::imu_residual_jacobian(*reinterpret_cast<const vbh::ImuPre *>(imu), *reinterpret_cast<const vbh::State *>(s1),
                             *reinterpret_cast<const vbh::State *>(s2), with_g != 0, rr, joc, nb);
}
// jtj[nb * nb], gg[nb]; returns r^T cov^-1 r (cinv given, as inside damping_iter)
extern "C" double imu_host_eval(const double *imu, const double *s1, const double *s2, int with_g, const double *cinv, double *jtj, double *gg) {
  return vbh::imu_evaluate(*reinterpret_cast<const vbh::ImuPre *>(imu), *reinterpret_cast<const vbh::State *>(s1),
                           *reinterpret_cast<const vbh::State *>(s2), with_g != 0, true, jtj, gg, cinv);
}
extern "C" int li_hb_size_host(int W, int grav) { return vba::li_hb_size(W, grav); }
extern "C" int li_hb_pair_host(int a, int b) { return vba::li_hb_pair(a, b); }
extern "C" int li_hb_ne1_host(int W) { return vba::li_hb_ne1(W); }
extern "C" double li_hb_get_host(const double *hb, int W, int n, int R, int C) { return vba::li_hb_get(hb, W, n, R, C); }
extern "C" void li_hb_dense_host(const double *hb, int W, int n, double *out) {
  for (int r = 0; r < n; r++) for (int c = 0; c < n; c++) out[(size_t)r * n + c] = vba::li_hb_get(hb, W, n, r, c);
}
