// The adapter's prior-map localisation (vba::SurfelMap, vba::relocalize of include/voxelba_adapter.hpp) for
// tests/test_gpu_surfreg.py.  Plain C++17, linked against libvoxelba.so.
//   surfreg_adapter_host IN OUT VOXEL SIGMA MINCOUNT BUILDVOXEL
//        IN:  int32 n_stores (2), then per store int32 n_kf, then per keyframe int32 n, double pose[12], double xyz[n][3]; then the
//             first guess double R[9], p[3].  Every keyframe is built from one scan at BUILDVOXEL with zero covariances on a
//             deterministic context.  Store 0 is the mapped session; keyframes 0 and 1 of store 1 are relocalised in its map.
//        OUT: int64 cells; per relocalised keyframe int32 ok, int32 iters, double R[9], p[3]
#include "voxelba_adapter.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

static bool get(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static int run(char **a) {
  const double voxel = std::atof(a[2]), sigma = std::atof(a[3]);
  const int min_count = std::atoi(a[4]);
  const double build_voxel = std::atof(a[5]);
  std::FILE *in = std::fopen(a[0], "rb");
  if (!in) { std::fprintf(stderr, "cannot read %s\n", a[0]); return 3; }
  vba_options o;
  vba_default_options(&o);
  o.device = 0; o.deterministic = 1;
  vba::Context ctx(o);
  std::vector<std::unique_ptr<vba::KeyframeStore>> own;
  int n_stores = 0;
  if (!get(in, &n_stores, 4) || n_stores != 2) return 3;
  for (int s = 0; s < n_stores; s++) {
    own.emplace_back(new vba::KeyframeStore(ctx));
    int n_kf = 0;
    if (!get(in, &n_kf, 4)) return 3;
    for (int k = 0; k < n_kf; k++) {
      int n = 0;
      double pose[12];
      if (!get(in, &n, 4) || !get(in, pose, sizeof(pose))) return 3;
      std::vector<double> xyz((size_t)n * 3);
      if (!get(in, xyz.data(), xyz.size() * sizeof(double))) return 3;
      vba::IMUST x;
      std::memcpy(x.R, pose, 72); std::memcpy(x.p, pose + 9, 24);
      vba::PVec pvec((size_t)n);
      for (int i = 0; i < n; i++) { std::memcpy(pvec[(size_t)i].pnt, &xyz[3 * (size_t)i], 24); std::memset(pvec[(size_t)i].var, 0, 72); }
      own.back()->build({vba::ScanPoseRef{&x, &pvec}}, build_voxel, k, (double)k);
    }
  }
  double guess[12];
  if (!get(in, guess, sizeof(guess))) return 3;
  std::fclose(in);
  std::FILE *out = std::fopen(a[1], "wb");
  if (!out) return 3;
  {
    vba::SurfelMap map(ctx);
    const std::vector<vba::KeyframeStore *> relc_submaps = {own[0].get(), own[1].get()};
    const int64_t cells = map.build(relc_submaps, {0}, voxel, sigma, min_count);
    if (cells != map.size()) return 4;
    std::fwrite(&cells, sizeof(cells), 1, out);
    for (int kf = 0; kf < 2; kf++) {
      vba::IMUST x;
      std::memcpy(x.R, guess, 72); std::memcpy(x.p, guess + 9, 24);
      vba_surfel_reg_report rep;
      const int ok = vba::relocalize(map, *own[1], kf, x, &rep) ? 1 : 0;
      std::fwrite(&ok, 4, 1, out); std::fwrite(&rep.iters, 4, 1, out);
      std::fwrite(x.R, 8, 9, out); std::fwrite(x.p, 8, 3, out);
    }
  }
  std::fclose(out);
  own.clear();
  return 0;
}

int main(int argc, char **argv) {
  try {
    if (argc == 7) return run(argv + 1);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: surfreg_adapter_host IN OUT VOXEL SIGMA MINCOUNT BUILDVOXEL\n");
  return 2;
}
