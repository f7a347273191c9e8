// The adapter's localisation mode (vba::lio_state_estimation_prior and vba::OdomState::lio_state_estimation_prior of
// include/voxelba_adapter.hpp) for tests/test_gpu_surfodom.py.  Plain C++17, linked against libvoxelba.so.
//   surfodom_adapter_host IN OUT VOXEL SIGMA MINCOUNT
//        IN:  int64 n_rec, n_pnt; float rec[n_rec][12]; double cov6[n_rec][6]; double pnt[n_pnt][3] (body frame); double state[25],
//             cov[225].  The map is built from the records on a deterministic context; the scan is handed over as it lies, in
//             host memory (the library stages it).
//        OUT: int64 cells; the free function: int32 ok, iterations, double state[25], cov[225]; the state object: int32 ok,
//             iterations, double x_out[25], then what get() returns, double state[25], cov[225]
#include "voxelba_adapter.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool get(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static int run(char **a) {
  const double voxel = std::atof(a[2]), sigma = std::atof(a[3]);
  const int min_count = std::atoi(a[4]);
  std::FILE *in = std::fopen(a[0], "rb");
  if (!in) { std::fprintf(stderr, "cannot read %s\n", a[0]); return 3; }
  int64_t n_rec = 0, n_pnt = 0;
  if (!get(in, &n_rec, 8) || !get(in, &n_pnt, 8) || n_rec < 1 || n_pnt < 0) return 3;
  std::vector<float> rec((size_t)n_rec * 12);
  std::vector<double> cov6((size_t)n_rec * 6), pnt((size_t)n_pnt * 3);
  vba::IMUST x0;
  if (!get(in, rec.data(), rec.size() * 4) || !get(in, cov6.data(), cov6.size() * 8) || !get(in, pnt.data(), pnt.size() * 8) || !get(in, &x0.t, 25 * 8) ||
      !get(in, x0.cov, 225 * 8))
    return 3;
  std::fclose(in);
  vba_options o;
  vba_default_options(&o);
  o.device = 0; o.deterministic = 1;
  vba::Context ctx(o);
  std::FILE *out = std::fopen(a[1], "wb");
  if (!out) return 3;
  {
    vba::SurfelMap map(ctx);
    const int64_t cells = map.build(n_rec, rec.data(), cov6.data(), voxel, sigma, min_count);
    if (cells != map.size()) return 4;
    std::fwrite(&cells, sizeof(cells), 1, out);
    vba::ScanView scan;
    scan.n = (int)n_pnt; scan.pnt = pnt.data();
    vba_odom_report rep;
    {
      vba::IMUST x = x0;
      const int ok = vba::lio_state_estimation_prior(ctx, map, scan, x, vba::surfel_odom_defaults(), &rep) ? 1 : 0;
      std::fwrite(&ok, 4, 1, out); std::fwrite(&rep.iterations, 4, 1, out);
      std::fwrite(&x.t, 8, 25, out); std::fwrite(x.cov, 8, 225, out);
    }
    {
      vba::OdomState st(ctx);
      st.set(x0);
      vba::IMUST xo, xg;
      const int ok = st.lio_state_estimation_prior(ctx, map, scan, vba::surfel_odom_defaults(), &rep, &xo) ? 1 : 0;
      st.get(xg);
      std::fwrite(&ok, 4, 1, out); std::fwrite(&rep.iterations, 4, 1, out);
      std::fwrite(&xo.t, 8, 25, out); std::fwrite(&xg.t, 8, 25, out); std::fwrite(xg.cov, 8, 225, out);
    }
  }
  std::fclose(out);
  return 0;
}

int main(int argc, char **argv) {
  try {
    if (argc == 6) return run(argv + 1);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: surfodom_adapter_host IN OUT VOXEL SIGMA MINCOUNT\n");
  return 2;
}
