// The host halves of vba_kf_surfel_export for tests/test_export_surfel_cpu.py and tests/test_gpu_export_surfel.py: the fit header
// csrc/vba_surfel_fit.hpp built by g++ (compile with -ffp-contract=off), and the adapter's vba::pub_globalmap_surfel
// (include/voxelba_adapter.hpp).  Plain C++17, linked against libvoxelba.so.
//   fit IN OUT                  IN:  int64 m, then per voxel 14 doubles: c[3], C[6] (xx xy xz yy yz zz), sensor[3], cnt, intensity
//                               OUT: float rec[m][12], then double eig[m][12]: w0 w1 w2 and V row-major (vectors in the columns),
//                                    the decomposition the record was made from                                       (host only)
//   cuts N INTERVAL             prints the message ends of a result of N records, one line                            (host only)
//   gpu IN OUT VOXEL MINCOUNT INTERVAL JUMP DET BUILDVOXEL
//        IN:  int32 n_stores, then per store int32 n_kf, then per keyframe int32 n, double pose[12], double xyz[n][3]
//        every keyframe is built from one scan at BUILDVOXEL with zero covariances; the stores are sessions 0, 1, ...
//        OUT: per message int64 n, float rec[n][12], double cov[n][6]
#include "voxelba_adapter.hpp"
#include "../../voxel-slam_amd/csrc/vba_surfel_fit.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static bool get(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static int run_fit(char **a) {
  std::FILE *in = std::fopen(a[0], "rb");
  if (!in) { std::fprintf(stderr, "cannot read %s\n", a[0]); return 3; }
  int64_t m = 0;
  if (!get(in, &m, 8) || m < 0) return 3;
  std::vector<double> rows((size_t)m * 14);
  if (!get(in, rows.data(), rows.size() * sizeof(double))) return 3;
  std::fclose(in);
  std::vector<float> rec((size_t)m * 12);
  std::vector<double> eig((size_t)m * 12);
  for (int64_t i = 0; i < m; i++) {
    const double *r = &rows[(size_t)i * 14];
    vba::sf_fit(r, r + 3, (int)r[12], r + 9, (float)r[13], &rec[(size_t)i * 12]);
    vba::Eig3 o;                                                 // the decomposition sf_fit starts from
    if (!vba::eig3_direct<true>(r[3], r[4], r[5], r[6], r[7], r[8], o)) o = vba::btcg_jacobi(r[3], r[4], r[5], r[6], r[7], r[8]);
    const double e[12] = {o.w0, o.w1, o.w2, o.v00, o.v01, o.v02, o.v10, o.v11, o.v12, o.v20, o.v21, o.v22};
    std::memcpy(&eig[(size_t)i * 12], e, sizeof(e));
  }
  std::FILE *out = std::fopen(a[1], "wb");
  if (!out) return 3;
  std::fwrite(rec.data(), sizeof(float), rec.size(), out);
  std::fwrite(eig.data(), sizeof(double), eig.size(), out);
  std::fclose(out);
  return 0;
}

static int run_cuts(long long n, long long interval) {
  for (int64_t e : vba::voxel_message_ends(n, interval)) std::printf("%lld ", (long long)e);
  std::printf("\n");
  return 0;
}

static int run_gpu(char **a) {
  const double voxel = std::atof(a[2]);
  const int min_count = std::atoi(a[3]);
  const long long interval = std::atoll(a[4]);
  const int jump = std::atoi(a[5]), det = std::atoi(a[6]);
  const double build_voxel = std::atof(a[7]);
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
      if (own.back()->build({vba::ScanPoseRef{&x, &pvec}}, build_voxel, k, (double)k) != n) { std::fprintf(stderr, "keyframe %d: points merged\n", k); return 4; }
    }
    relc_submaps.push_back(own.back().get());
    ids.push_back(s);
  }
  std::fclose(in);
  std::FILE *out = std::fopen(a[1], "wb");
  if (!out) return 3;
  int msgs = 0;
  const int64_t total = vba::pub_globalmap_surfel(ctx, relc_submaps, ids, voxel, [&](const float *rec, const double *cov, int64_t n) {
    std::fwrite(&n, sizeof(n), 1, out);
    if (n > 0) { std::fwrite(rec, 48, (size_t)n, out); std::fwrite(cov, 48, (size_t)n, out); }
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
    if (mode == "fit" && argc == 4) return run_fit(argv + 2);
    if (mode == "cuts" && argc == 4) return run_cuts(std::atoll(argv[2]), std::atoll(argv[3]));
    if (mode == "gpu" && argc == 10) return run_gpu(argv + 2);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: fit IN OUT | cuts N INTERVAL | gpu IN OUT VOXEL MINCOUNT INTERVAL JUMP DET BUILDVOXEL\n");
  return 2;
}
