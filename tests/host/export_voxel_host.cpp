// Runs the adapter's vba::pub_globalmap_voxel, vba::voxel_message_ends and vba::pub_global_path (include/voxelba_adapter.hpp) for
// tests/test_export_voxel_cpu.py and tests/test_gpu_export_voxel.py.  Plain C++17, linked against libvoxelba.so.
//   cuts N INTERVAL            prints the message ends of a result of N records, one line            (host only)
//   path                       prints the records of pub_global_path for the sessions built below    (host only)
//   gpu IN OUT VOXEL MINCOUNT INTERVAL JUMP DET
//        IN:  int32 n_stores, then per store int32 n_kf, then per keyframe int32 n, double pose[12], double xyz[n][3]
//        every keyframe is built from one scan at voxel_size_10 = 0.05 with zero covariances; the stores are sessions 0, 1, ...
//        OUT: per message int64 n, float xyzi[n][4]
#include "voxelba_adapter.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static int run_cuts(long long n, long long interval) {
  for (int64_t e : vba::voxel_message_ends(n, interval)) std::printf("%lld ", (long long)e);
  std::printf("\n");
  return 0;
}

static int run_path() {
  // sessions 0, 1 (empty), 2; published in the order 2, 0
  std::vector<std::unique_ptr<vba::ScanPose>> own;
  std::vector<std::vector<vba::ScanPose *>> sessions(3);
  const int sizes[3] = {3, 0, 2};
  for (int s = 0; s < 3; s++)
    for (int i = 0; i < sizes[s]; i++) {
      vba::IMUST x;
      x.p[0] = 100.0 * s + i + 0.1; x.p[1] = -(double)i - 1.0 / 3.0; x.p[2] = 16777217.0 + s;   // none of them a float
      own.emplace_back(new vba::ScanPose(x, nullptr));
      sessions[(size_t)s].push_back(own.back().get());
    }
  std::vector<std::vector<vba::ScanPose *> *> relc_bl_buf{&sessions[0], &sessions[1], &sessions[2]};
  std::vector<int> ids{2, 0};
  int msgs = 0;
  const int64_t n = vba::pub_global_path(relc_bl_buf, ids, [&](const float *xyzi, int64_t m) {
    msgs++;
    for (int64_t i = 0; i < m; i++) std::printf("%.9g %.9g %.9g %.9g\n", xyzi[4 * i], xyzi[4 * i + 1], xyzi[4 * i + 2], xyzi[4 * i + 3]);
  });
  std::printf("records %lld messages %d\n", (long long)n, msgs);
  ids.clear();
  msgs = 0;
  const int64_t none = vba::pub_global_path(relc_bl_buf, ids, [&](const float *, int64_t m) { msgs += (m == 0); });
  std::printf("records %lld messages %d\n", (long long)none, msgs);
  return 0;
}

static bool get(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static int run_gpu(char **a) {
  const double voxel = std::atof(a[2]);
  const int min_count = std::atoi(a[3]);
  const long long interval = std::atoll(a[4]);
  const int jump = std::atoi(a[5]), det = std::atoi(a[6]);
  std::FILE *in = std::fopen(a[0], "rb");
  if (!in) { std::fprintf(stderr, "cannot read %s\n", a[0]); return 3; }
  vba_options o;
  vba_default_options(&o);
  o.device = 0; o.deterministic = det;
  vba::Context ctx(o);
  std::vector<std::unique_ptr<vba::KeyframeStore>> own;
  std::vector<vba::KeyframeStore *> relc_submaps;
  std::vector<int> ids;
  int n_stores = 0;
  if (!get(in, &n_stores, 4)) return 3;
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
      if (own.back()->build({vba::ScanPoseRef{&x, &pvec}}, 0.05, k, (double)k) != n) { std::fprintf(stderr, "keyframe %d: points merged\n", k); return 4; }
    }
    relc_submaps.push_back(own.back().get());
    ids.push_back(s);
  }
  std::fclose(in);
  std::FILE *out = std::fopen(a[1], "wb");
  if (!out) return 3;
  int msgs = 0;
  const int64_t total = vba::pub_globalmap_voxel(ctx, relc_submaps, ids, voxel, [&](const float *xyzi, int64_t n) {
    std::fwrite(&n, sizeof(n), 1, out);
    if (n > 0) std::fwrite(xyzi, 16, (size_t)n, out);
    msgs++;
  }, min_count, interval, jump);
  std::fclose(out);
  std::printf("records %lld messages %d\n", (long long)total, msgs);
  own.clear();
  return 0;
}

int main(int argc, char **argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cuts" && argc == 4) return run_cuts(std::atoll(argv[2]), std::atoll(argv[3]));
    if (mode == "path" && argc == 2) return run_path();
    if (mode == "gpu" && argc == 9) return run_gpu(argv + 2);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: cuts N INTERVAL | path | gpu IN OUT VOXEL MINCOUNT INTERVAL JUMP DET\n");
  return 2;
}
