// Host build of the shape header of the dense-tile Hessian pass (voxel-slam_amd/csrc/vba_hess_units.hpp) for
// tests/test_hess_units_cpu.py: a stand-alone program, plain g++, nothing of the runtime.
//   hess_units_host table        one line per window W = 2..16 with the tile shape and LDS budget, then one line per (wave, t) unit
//   hess_units_host tree N       reads 8 N doubles (binary, stdin), writes the N sums group8_tree gives of each run of 8 (binary, stdout)
// Test harness only.
#include "../../voxel-slam_amd/csrc/vba_hess_units.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <int W>
static void table_of() {
  using C = vba::HessCfg2<W>;
  // (the table is a constant expression: this is what the kernel's unrolled selects are folded from)
  constexpr vba::HessUnit first = C::unit(0, 0);
  static_assert(first.u == 0 && first.ta == 0 && first.tb == 0 && first.ks == 0, "unit 0 is tile (0, 0) of k-split 0");
  std::printf("W %d TV %d NT16 %d NU %d KS %d UPW %d NWV %d KSTEPS %d NK %d PRESCALE %d LDS_MAIN %zu LDS_EPI %zu LDS_BYTES %zu\n", W, C::TV, C::NT16, C::NU, C::KS,
              C::UPW, C::NWV, C::KSTEPS, C::NK, (int)C::PRESCALE, C::LDS_MAIN * sizeof(double), C::LDS_EPI * sizeof(double), C::LDS_BYTES);
  for (int w = 0; w < C::NWV; w++)
    for (int t = 0; t < C::UPW; t++) {
      const vba::HessUnit un = C::unit(w, t);
      std::printf("unit %d %d %d %d %d %d %d\n", W, w, t, un.u, un.ta, un.tb, un.ks);
    }
}
template <int LO, int HI>
static void tables() {
  table_of<LO>();
  if constexpr (LO < HI) tables<LO + 1, HI>();
}

static int tree(size_t n) {
  std::vector<double> x(8 * n), y(n);
  if (std::fread(x.data(), sizeof(double), x.size(), stdin) != x.size()) return 1;
  for (size_t i = 0; i < n; i++) y[i] = vba::group8_tree(&x[8 * i]);
  return std::fwrite(y.data(), sizeof(double), n, stdout) == n ? 0 : 1;
}

int main(int argc, char **argv) {
  const std::string which = argc > 1 ? argv[1] : "";
  if (which == "table") { tables<2, 16>(); return 0; }
  if (which == "tree" && argc > 2) return tree((size_t)std::atol(argv[2]));
  std::fprintf(stderr, "unknown case '%s'\n", which.c_str());
  return 2;
}
