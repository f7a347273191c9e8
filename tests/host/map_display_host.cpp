// The adapter path of the local-map display export (include/voxelba_adapter.hpp: vba::VoxelMap::display / tras_display and
// vba::pub_voxelmap) on the GPU, driven by tests/test_gpu_map_display.py: the steady-state loop of local mapping without its LM step
// (insert, recut; with a full window evaluate, marginalise, slide), every scan at the one pose the input gives it, then the display of
// the final window.  The test runs the same session through the ctypes binding and compares the bytes.
//
//   input  (doubles): [magic 20261020, win_size, n_scans, voxel_size, max_layer, max_points, min_eigen_value, plane_thre[4], min_point[4],
//                      thread_num, deterministic]  per scan: [n, R(9), p(3)] points[n][3]
//   output (bytes):   int64 [n, m, win_count, n_all], then
//                     display(flags 0): xyzi f32 [n][4], plane_of_point i32 [n], frame_begin i64 [win_count + 1], planes f32 [m][16], plane_key i64 [m][5]
//                     tras_display: pl_wind f32 [n][4];  pub_voxelmap: points f32 [n][4], planes f32 [m][16], keys i64 [m][5]
//                     display(flags 1): xyzi f32 [n_all][4], plane_of_point i32 [n_all]
#include "voxelba_adapter.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace vba;

template <class T>
static void put(std::vector<char> &out, const T *p, size_t n) {
  const char *b = (const char *)p;
  out.insert(out.end(), b, b + n * sizeof(T));
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <input.bin> <output.bin>\n", argv[0]); return 2; }
  std::vector<double> in;
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    in.resize((size_t)bytes / 8);
    if (std::fread(in.data(), 8, in.size(), f) != in.size()) return 2;
    std::fclose(f);
  }
  size_t q = 0;
  auto next = [&]() { return in.at(q++); };
  if (next() != 20261020.0) { std::fprintf(stderr, "map_display_host: bad magic\n"); return 2; }
  vba_options opt;
  vba_default_options(&opt);
  opt.win_size = (int)next();
  const int n_scans = (int)next();
  opt.voxel_size = next(); opt.max_layer = (int)next(); opt.max_points = (int)next(); opt.min_eigen_value = next();
  for (int i = 0; i < 4; i++) opt.plane_eigen_value_thre[i] = next();
  for (int i = 0; i < 4; i++) opt.min_point[i] = next();
  opt.thread_num = (int)next(); opt.deterministic = (int)next();
  std::vector<char> out;
  try {
    Context ctx(opt);
    VoxelMap surf_map(ctx);
    LidarFactor voxhess(ctx, opt.win_size);
    std::vector<IMUST> x_buf;
    int win_count = 0;
    for (int k = 0; k < n_scans; k++) {
      const size_t n = (size_t)next();
      IMUST x;
      for (int i = 0; i < 9; i++) x.R[i] = next();
      for (int i = 0; i < 3; i++) x.p[i] = next();
      PVec pvec(n);
      for (size_t i = 0; i < n; i++) for (int c = 0; c < 3; c++) pvec[i].pnt[c] = next();
      x_buf.push_back(x);
      win_count++;
      surf_map.cut_voxel_multi(pvec, win_count - 1, x, false);
      surf_map.multi_recut(win_count, x_buf);
      if (win_count >= opt.win_size) {
        double residual = 0;
        voxhess.evaluate_only_residual(x_buf, 0, (int)voxhess.size(), residual);
        surf_map.multi_margi((double)k, win_count, x_buf);
        surf_map.slide(1);
        x_buf.erase(x_buf.begin());
        win_count--;
      }
    }
    const VoxelMap::Display d = surf_map.display(win_count, x_buf, 0), all = surf_map.display(win_count, x_buf, 1);
    const int64_t hdr[4] = {d.n_points(), d.n_planes(), win_count, all.n_points()};
    put(out, hdr, 4);
    put(out, d.xyzi.data(), d.xyzi.size()); put(out, d.plane_of_point.data(), d.plane_of_point.size());
    put(out, d.frame_begin.data(), d.frame_begin.size()); put(out, d.planes.data(), d.planes.size()); put(out, d.plane_key.data(), d.plane_key.size());
    std::vector<float> pl_wind;
    surf_map.tras_display(win_count, pl_wind, x_buf);
    put(out, pl_wind.data(), pl_wind.size());
    int64_t published = -1, np = -1, nm = -1;
    published = pub_voxelmap(surf_map, win_count, x_buf,
                             [&](const float *xyzi, int64_t n) { np = n; put(out, xyzi, (size_t)n * 4); },
                             [&](const float *planes, const long long *keys, int64_t m) { nm = m; put(out, planes, (size_t)m * 16); put(out, keys, (size_t)m * 5); });
    if (published != d.n_points() || np != d.n_points() || nm != d.n_planes() || (int64_t)pl_wind.size() != 4 * d.n_points()) {
      std::fprintf(stderr, "map_display_host: the three adapter paths disagree on the sizes\n");
      return 1;
    }
    put(out, all.xyzi.data(), all.xyzi.size()); put(out, all.plane_of_point.data(), all.plane_of_point.size());
  } catch (const std::exception &e) {
    std::fprintf(stderr, "map_display_host: %s\n", e.what());
    return 1;
  }
  FILE *f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(out.data(), 1, out.size(), f);
  std::fclose(f);
  return 0;
}
