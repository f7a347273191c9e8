// Host build of the product's symmetric solver (vbh::ldlt_solve_inplace, csrc/vba_hostmath.hpp) and of the LI elimination order
// and structure mask (csrc/vba_li_order.hpp) for the CPU checks of tests/test_solve_cpu.py.  Test harness only.
#include "../../voxel-slam_amd/csrc/vba_hostmath.hpp"
#include "../../voxel-slam_amd/csrc/vba_li_order.hpp"
extern "C" void ldlt_solve_host(double *A, const double *b, double *x, int n) { vbh::ldlt_solve_inplace(A, b, x, n); }
extern "C" int li_ord_host(int k, int W) { return vba::li_ord(k, W); }
extern "C" unsigned li_live_host(int kb, int W, int n, int NP) { return vba::li_live(kb, W, n, NP); }
