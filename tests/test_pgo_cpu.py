"""CPU checks of the pose-graph optimisation: the oracle's SE(3) chart against scipy's matrix exponential /
logarithm, its factor Jacobians against central differences, its ISAM2 schedule on a noise-free graph, and the C ABI / adapter
surface of vba_pgo_optimize (declared, exported, callable from C++ through vba::PoseGraph)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg

import pgo_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twist(xi):
    T = np.zeros((4, 4))
    T[:3, :3] = po.hat(xi[:3])
    T[:3, 3] = xi[3:]
    return T


def _mat(X):
    T = np.eye(4)
    T[:3, :3] = X[:9].reshape(3, 3)
    T[:3, 3] = X[9:]
    return T


@pytest.mark.parametrize("scale", [1e-9, 1e-5, 1e-3, 0.05, 0.19, 0.21, 1.0, 2.5])
def test_exp_log_round_trip_and_scipy(scale):
    rng = np.random.default_rng(int(scale * 1e9) % 1000)
    for _ in range(20):
        w = rng.normal(size=3)
        w *= scale / np.linalg.norm(w)
        xi = np.concatenate([w, rng.normal(size=3)])
        X = po.exp6(xi)
        np.testing.assert_allclose(_mat(X), scipy.linalg.expm(_twist(xi)), rtol=0, atol=1e-12)
        np.testing.assert_allclose(po.log6(X), xi, rtol=0, atol=1e-12)
        L = scipy.linalg.logm(_mat(X)).real
        np.testing.assert_allclose(po.log6(X), np.concatenate([[L[2, 1], L[0, 2], L[1, 0]], L[:3, 3]]), rtol=0, atol=1e-12)
        R = X[:9].reshape(3, 3)
        np.testing.assert_allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-14)


def _numeric(f, X, h=1e-6):
    J = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        J[:, k] = (f(po.retract(X, d)) - f(po.retract(X, -d))) / (2 * h)
    return J


@pytest.mark.parametrize("err", [1e-7, 1e-3, 0.1, 0.8])
def test_between_and_prior_jacobians_central_differences(err):
    rng = np.random.default_rng(7)
    for _ in range(10):
        Xi = po.exp6(rng.normal(size=6) * 2)
        Xj = po.exp6(rng.normal(size=6) * 2)
        Z = po.retract(po.compose(po.inverse(Xi), Xj), rng.normal(size=6) * err)
        e, Ji, Jj = po.between_jacobians(Xi, Xj, Z)
        np.testing.assert_allclose(Ji, _numeric(lambda X: po.between_error(X, Xj, Z), Xi), rtol=0, atol=1e-7)
        np.testing.assert_allclose(Jj, _numeric(lambda X: po.between_error(Xi, X, Z), Xj), rtol=0, atol=1e-7)
        P = po.retract(Xi, rng.normal(size=6) * err)
        e, J = po.prior_jacobian(Xi, P)
        np.testing.assert_allclose(J, _numeric(lambda X: po.prior_error(X, P), Xi), rtol=0, atol=1e-7)


def test_noise_free_graph_recovers_truth():
    rng = np.random.default_rng(3)
    X, Y, edges, priors = po.reference_session(rng, n=120, noise=False)
    priors[0, 1:13] = X[0]                          # the prior holds the truth, so the truth is the unique minimiser
    # threshold 0 relinearises every node at every update (plain Gauss-Newton); at 0.01 the final theta (+) delta keeps the
    # second-order error of the last linearisation point, as ISAM2 does
    out, stats, deltas = po.optimize(Y, edges, priors, n_updates=6, relin_threshold=0.0)
    for k in range(len(X)):
        np.testing.assert_allclose(po.log6(po.compose(po.inverse(X[k]), out[k])), 0, atol=1e-9)
    assert stats[0, 0] == 0 and (stats[1:, 0] == len(X)).all()
    assert stats[-1, 1] < 1e-12 * stats[0, 1]
    out, stats, deltas = po.optimize(Y, edges, priors)
    assert stats[1, 0] > 0 and stats[-1, 0] == 0          # the drift is above 0.01 at first, below it at the end


def test_schedule_keeps_small_deltas_unapplied():
    """A node whose |delta|_inf stays below the threshold keeps its linearisation point; the estimate is theta (+) delta."""
    rng = np.random.default_rng(4)
    X = po.trajectory(rng, 5)
    Y = po.drift(rng, X, rot=1e-4, tra=1e-3)
    edges = np.array([po.edge_row(k - 1, k, X[k - 1], X[k], np.full(6, 1e-4)) for k in range(1, 5)])
    priors = np.array([po.prior_row(0, X[0], np.full(6, 1e-9))])
    out, stats, deltas = po.optimize(Y, edges, priors, n_updates=3)
    assert (stats[:, 0] == 0).all()
    np.testing.assert_array_equal(deltas[0], deltas[2])
    np.testing.assert_allclose(out, np.array([po.retract(Y[k], deltas[0][k]) for k in range(5)]), atol=0)


def test_pgo_declared_and_exported():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    assert re.search(r"VBA_ERR_SINGULAR\s*=\s*10", hdr)
    assert re.search(r"int vba_pgo_optimize\(vba_ctx \*ctx, int n, double \*poses, int m, const double \*edges, int n_prior,", hdr)
    assert "vba_pgo_optimize" in capi.EXPORTS and capi.ERR_SINGULAR == 10
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    assert hasattr(capi.load(), "vba_pgo_optimize")
    assert capi.load().vba_status_string(10).decode().startswith("singular")


def test_pose_graph_adapter_compiles_and_links(tmp_path):
    """vba::PoseGraph (build_graph's gtsam::Values / NonlinearFactorGraph, LR:147-161, LR:36-43) compiles as plain C++17 against
    libvoxelba.so; its host-side bookkeeping (both add_edge overloads, priors, set_state) runs without a device."""
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    src = tmp_path / "pgo_check.cpp"
    src.write_text(r'''
#include "voxelba_adapter.hpp"
#include <cmath>
#include <cstdio>
int main() {
  vba::PoseGraph g;
  vba::IMUST x0, x1;
  x1.p[0] = 1.0; x1.R[0] = 0.0; x1.R[1] = -1.0; x1.R[3] = 1.0; x1.R[4] = 0.0;   // 90 degrees about z
  g.insert(0, x0); g.insert(1, x1);
  double v6[6] = {1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4};
  g.add_edge(0, 1, x0, x1, v6);                               // LR:147-153
  double rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tra[3] = {0.5, 0, 0};
  g.add_edge(0, 1, rot, tra, v6);                             // LR:155-161
  g.add_prior(0, x0, v6);
  if (g.size() != 2 || g.num_edges() != 2 || g.num_priors() != 1) return 2;
  if (g.edges()[3] != -1.0 || g.edges()[11] != 1.0 || g.edges()[20 + 11] != 0.5) return 3;   // rot = R1^T R2, tra = R1^T (p2 - p1)
  // ScanPose::set_state (LR:36-43): the velocity turns with the rotation change
  vba::IMUST s; s.v[0] = 2.0;
  double pose[12] = {0, -1, 0, 1, 0, 0, 0, 0, 1, 3, 4, 5};
  vba::set_state(s, pose);
  if (std::fabs(s.v[1] - 2.0) > 1e-15 || std::fabs(s.v[0]) > 1e-15 || s.p[2] != 5.0 || s.R[1] != -1.0) return 4;
  int (vba::PoseGraph::*fn)(vba::Context &, int, double) = &vba::PoseGraph::optimize;
  std::printf("ok %d\n", fn != nullptr);
  return 0;
}
''')
    exe = tmp_path / "pgo_check"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lvoxelba", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
