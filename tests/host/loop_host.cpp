// Host side of the loop-closure tests (tests/test_loop_cpu.py, tests/test_gpu_loop.py), built by the tests with g++ -ffp-contract=off.
// 1. The oracle's C API has no fixed insertion WITH covariances; VoxelMapOracle::cut_voxel_fix stores whatever pv.var it is given,
//    so the missing entry is added here on a handle made by liboracle's vso_map_create (the oracle is header-only C++).
// 2. The adapter's host algebra (loop_dx, ScanPose::update, the window states and g_update of loop_update) for the comparison
//    with the numpy restatement tests/loop_oracle.py.
#include "../../oracle/map_oracle.hpp"
#include "../../include/voxelba_adapter.hpp"

using namespace vso;

extern "C" {

// pnt_world [n][3], var [n][9] row-major (null: zeros), one cut_voxel(map, pvec, win_size, jour) call (VM:2108-2152)
void lh_map_cut_voxel_fix_var(void *m, int n, const double *pnt_world, const double *var, double jour) {
  VoxelMapOracle *vm = (VoxelMapOracle *)m;
  PVec pv(n);
  for (int i = 0; i < n; i++) {
    pv[i].pnt = v3(pnt_world[3 * i], pnt_world[3 * i + 1], pnt_world[3 * i + 2]);
    if (var) for (int k = 0; k < 9; k++) pv[i].var[k] = var[9 * i + k];
  }
  vm->cut_voxel_fix(pv, jour);
}

// states are [t, R(9), p(3), v(3), bg(3), ba(3), g(3)] (25)
static vba::IMUST st_in(const double *s) { vba::IMUST x; std::memcpy(&x.t, s, 25 * sizeof(double)); return x; }
static void st_out(const vba::IMUST &x, double *s) { std::memcpy(s, &x.t, 25 * sizeof(double)); }

void lh_loop_dx(const double *x1, const double *x3, double *dx12) {
  const vba::IMUST dx = vba::loop_dx(st_in(x1), st_in(x3));
  std::memcpy(dx12, dx.R, 72); std::memcpy(dx12 + 9, dx.p, 24);
}

// the host half of VoxelMap::loop_update: bl [k][25], x_buf [n_buf][25], x_curr [25] in place; returns g_update after the call
int lh_loop_update_states(const double *dx12, int k, double *bl, int n_buf, double *x_buf, int win_count, double *x_curr, int g_update) {
  vba::IMUST dx;
  std::memcpy(dx.R, dx12, 72); std::memcpy(dx.p, dx12 + 9, 24);
  std::vector<vba::ScanPose> store;
  store.reserve(k);
  for (int i = 0; i < k; i++) store.emplace_back(st_in(bl + 25 * i), std::make_shared<vba::PVec>());
  std::vector<vba::ScanPose *> buf;
  for (int i = 0; i < k; i++) buf.push_back(&store[i]);
  std::vector<vba::IMUST> xs(n_buf);
  for (int i = 0; i < n_buf; i++) xs[i] = st_in(x_buf + 25 * i);
  vba::IMUST xc = st_in(x_curr);
  vba::loop_update_states(dx, buf, xs, win_count, xc, g_update);
  vba::loop_update_finish(g_update);
  for (int i = 0; i < k; i++) st_out(store[i].x, bl + 25 * i);
  for (int i = 0; i < n_buf; i++) st_out(xs[i], x_buf + 25 * i);
  st_out(xc, x_curr);
  return g_update;
}

}  // extern "C"
