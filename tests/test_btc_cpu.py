"""Loop retrieval without a GPU: the C ABI's host pieces (vba_btc_default_config against read_parameters, BTC.cpp:3-68; vba_btc_create
refusing to run without a device) and known-answer tests of the numpy restatement in tests/btc_oracle.py that the GPU tests
compare against, including the quirks of the reference that the device must keep."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import btc_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.mark.parametrize("fly", [0, 1])
def test_default_config_is_read_parameters(capi, fly):
    assert bo.config_dict(capi.btc_default_config(fly)) == bo.read_parameters(fly)


def test_create_without_device(capi):
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a HIP device is present")
    except ImportError:
        pass
    h = C.c_void_p()
    cfg = capi.btc_default_config(0)
    assert capi.load().vba_btc_create(None, C.byref(cfg), C.byref(h)) == capi.ERR_NO_DEVICE


def _row(tri, frame, loc=None, summ=(10, 10, 10)):
    r = np.zeros(19)
    r[0:3] = tri
    r[6] = frame
    loc = np.arange(9, dtype=float).reshape(3, 3) if loc is None else np.asarray(loc, float)
    r[7:16] = loc.reshape(-1)
    r[3:6] = loc.mean(0)
    r[16:19] = summ
    return r


def _bits(n, v=0x3FF):
    return np.full((n, 3), v, dtype=np.uint64)


def _cfg(**kw):
    c = bo.read_parameters(0)
    c.update(kw)
    return c


def test_triangle_solver_recovers_transform():
    rng = np.random.default_rng(0)
    for det_fix in (False, True):
        for _ in range(20):
            a = rng.normal(size=3)
            R = bo.so3_exp(a)
            t = rng.normal(size=3) * 5
            loc = rng.normal(size=(1, 3, 3)) * 4
            ref = loc @ R.T + t
            Rs, ts = bo.triangle_solver(loc, loc[:, :, :].mean(1), ref, ref.mean(1))
            assert np.abs(Rs[0] - R).max() < 1e-12 and np.abs(ts[0] - t).max() < 1e-11
    # the det < 0 branch, provably taken.  A triangle minus its centroid has rank 2, which leaves the third singular vectors' sign
    # free; with center_ off the centroid (center_ is an input row field) the covariance has full rank, and a reference that is
    # the MIRROR image of the source (z -> -z) makes V U^T a reflection, which the branch turns into V diag(1, 1, -1) U^T
    loc = np.array([[[0.0, 0, 1], [3, 0, -1], [0, 4, 0.5]]])
    ref = loc * np.array([1.0, 1.0, -1.0])
    cen = np.zeros((1, 3))
    U, S, Vt = np.linalg.svd(loc[0].T @ ref[0])
    assert S.min() > 1e-3 and np.linalg.det(Vt.T @ U.T) < 0           # full rank: the sign is not free, the branch must run
    R, t = bo.triangle_solver(loc, cen, ref, cen)
    assert np.linalg.det(R[0]) > 0 and np.abs(R[0] @ R[0].T - np.eye(3)).max() < 1e-12
    K = np.diag([1.0, 1.0, -1.0])
    assert np.abs(R[0] - Vt.T @ K @ U.T).max() < 1e-12


def test_quirks_cells_truncation_and_duplicates():
    # database keys use (int)(t + 0.5); queries (int)(t + inc): C truncation, so a side in (0, 1) visits cell 0 twice
    db = bo.BtcDb(_cfg(skip_near_num=-1000))
    db.push_plane_cloud(np.zeros((1, 6), np.float32), 0)
    db.add_stds([_row([0.4, 0.4, 0.4], 0)], _bits(1))
    assert list(db.cells) == [(0, 0, 0)]
    qi, dj = db.match_list([_row([0.4, 0.4, 0.4], 0)], _bits(1))
    assert len(qi) == 8                                              # (int)(0.4 - 1) = (int)(0.4) = 0 on every axis: 2^3 visits
    # a side >= 1 visits each cell once: the same descriptor matches once
    db2 = bo.BtcDb(_cfg(skip_near_num=-1000))
    db2.push_plane_cloud(np.zeros((1, 6), np.float32), 0)
    db2.add_stds([_row([10.2, 20.2, 30.2], 0)], _bits(1))
    qi, dj = db2.match_list([_row([10.2, 20.2, 30.2], 0)], _bits(1))
    assert len(qi) == 1


def test_quirks_gate_to_cell_centre_and_signed_frames():
    # rough_dis_threshold large enough that only the gate can reject (|(11.9, ..) - (10, ..)| = 3.29 < 0.5 * 20.6)
    db = bo.BtcDb(_cfg(skip_near_num=30, rough_dis_threshold=0.5))
    db.push_plane_cloud(np.zeros((1, 6), np.float32), 0)
    db.add_stds([_row([10.0, 10.0, 10.0], 0)], _bits(1))           # key (10, 10, 10), centre 10.5
    # a query at 11.9: offset -1 reaches cell 10, whose centre is 1.4 * sqrt(3) = 2.42 > 1.5 away -> no visit
    qi, _ = db.match_list([_row([11.9, 11.9, 11.9], 100)], _bits(1))
    assert len(qi) == 0
    # at 11.3 the same cell's centre is 0.8 * sqrt(3) = 1.39 < 1.5 away: visited, and the match passes every other test
    qi, _ = db.match_list([_row([11.3, 11.3, 11.3], 100)], _bits(1))
    assert len(qi) == 1
    qi, _ = db.match_list([_row([10.0, 10.0, 10.0], 100)], _bits(1))
    assert len(qi) == 1
    # frame differences are signed ints: 20 - 0 is not > 30; a closed session (skip_near_num negative) matches every frame
    qi, _ = db.match_list([_row([10.0, 10.0, 10.0], 20)], _bits(1))
    assert len(qi) == 0
    db.cfg["skip_near_num"] = -(1 + 10)
    qi, _ = db.match_list([_row([10.0, 10.0, 10.0], 0)], _bits(1))
    assert len(qi) == 1


def test_quirks_similarity_nan_and_empty_cloud():
    assert np.isnan(bo.binary_similarity(np.uint64(0), np.uint64(0), 0, 0))
    assert bo.binary_similarity(np.uint64(0b1011), np.uint64(0b0011), 3, 2) == 2 * 2 / 5
    db = bo.BtcDb(_cfg(skip_near_num=-1000))
    db.push_plane_cloud(np.zeros((1, 6), np.float32), 0)
    db.add_stds([_row([10.0, 10.0, 10.0], 0, summ=(0, 0, 0))], _bits(1, 0))
    qi, _ = db.match_list([_row([10.0, 10.0, 10.0], 0, summ=(0, 0, 0))], _bits(1, 0))
    assert len(qi) == 0                                              # 0 / 0 = NaN is never similar
    # score = count / pl_cur.size(): NaN for an empty pl_cur
    assert np.isnan(db.plane_geometric_verify(np.zeros((0, 6), np.float32), db.clouds[0], np.eye(3), np.zeros(3)))
    # an empty query
    r, c = db.search_loop(np.zeros((0, 19)), np.zeros((0, 3), np.uint64), np.zeros((1, 6), np.float32))
    assert r["loop_id"] == -1 and r["score"] == 0 and c == []


def test_vote_floor_cap_and_ties():
    db = bo.BtcDb(_cfg(candidate_num=2))
    for f in range(6):
        db.push_plane_cloud(np.zeros((1, 6), np.float32), f)
    votes = np.array([4, 7, 5, 7, 9, 0])                             # frame 4 first, then the tie 1 / 3 by index; cap 2
    mf = np.repeat(np.arange(6), votes)
    assert db.candidates(mf) == [(4, 9), (1, 7)]
    db.cfg["candidate_num"] = 20
    assert db.candidates(mf) == [(4, 9), (1, 7), (3, 7), (2, 5)]     # 4 votes stay under the floor of 5


def test_skip_len_sampling():
    size = 120
    skip = size // 50 + 1
    use = size // skip
    assert (skip, use) == (3, 40)
    # a match list of 120 identical pairs: every sampled pair is tested, the first maximum (index 0) wins
    rows = np.array([_row([10.0, 20.0, 30.0], 100)])
    db = bo.BtcDb(_cfg())
    db.push_plane_cloud(np.zeros((1, 6), np.float32), 0)
    db.add_stds([_row([10.0, 20.0, 30.0], 0)], _bits(1))
    r = db.verify(rows, np.zeros(size, np.int64), np.zeros(size, np.int64), None)
    assert r["max_vote"] == 120 and r["max_vote_index"] == 0


def test_icp_converges_through_parameter_switch():
    rng = np.random.default_rng(1)
    normals = np.array([[0, 0, 1.0], [1, 0, 0], [0, 1, 0]])
    k = rng.integers(0, 3, 600)
    nrm = normals[k]
    pts = rng.uniform(-5, 5, (600, 3))
    pts[np.arange(600), k] = (k - 1) * 3.0                          # points on the planes z = -3, x = 0, y = 3
    tar = np.column_stack([pts, nrm]).astype(np.float32)
    Rt = bo.so3_exp([0.01, 0.02, -0.015]); tt = np.array([0.1, 0.05, -0.08])
    src = tar.copy()
    src[:, 0:3] = ((pts - tt) @ Rt).astype(np.float32)
    src[:, 3:6] = (nrm @ Rt).astype(np.float32)
    o = bo.icp_normal(src, tar, np.zeros(3), np.eye(3), 0.1)
    assert o["is_converge"] == 1 and o["ok"] == 1 and 2 <= o["iters"] < 20
    assert np.abs(o["R"] - Rt).max() < 1e-3 and np.abs(o["t"] - tt).max() < 1e-3


def test_ldlt6_twin_equals_host_solver(tmp_path):
    """vbh::ldlt_solve_fixed<6> (the device twin) gives the bits of vbh::ldlt_solve_inplace on the host."""
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include "vba_hostmath.hpp"
#include "vba_ldlt6.hpp"
#include <cstdio>
#include <cstring>
#include <random>
int main() {
  std::mt19937_64 g(7);
  std::normal_distribution<double> nd;
  int bad = 0;
  for (int it = 0; it < 2000; it++) {
    double J[6 * 9], A[36], B[36], b[6], x1[6], x2[6];
    for (double &v : J) v = nd(g);
    const int rank = it % 4 == 3 ? 4 : 6;                           // some singular systems too
    for (int r = 0; r < 6; r++) for (int c = 0; c < 6; c++) { double s = 0; for (int k = 0; k < rank; k++) s += J[r * 9 + k] * J[c * 9 + k]; A[r * 6 + c] = s; }
    if (it % 50 == 0) for (double &v : A) v = 0;
    for (double &v : b) v = nd(g);
    std::memcpy(B, A, sizeof(A));
    vbh::ldlt_solve_inplace(A, b, x1, 6);
    vbh::ldlt_solve_fixed<6>(B, b, x2);
    if (std::memcmp(x1, x2, sizeof(x1))) bad++;
  }
  std::printf("%d\n", bad);
  return 0;
}
''')
    exe = tmp_path / "t"
    inc = os.path.join(ROOT, "voxel-slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + inc, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "0"


def test_device_svd_restatement_equals_numpy(tmp_path):
    """btc_svd3 / the Kabsch step as the device runs it (vba_kernels_btc.hpp, compiled for the host) against numpy: the same
    rotation for general, rank-2 (triangle) and reflected covariances, the det < 0 branch included."""
    src = tmp_path / "s.cpp"
    src.write_text(r'''
#include <cstdio>
#include "vba_btc_svd.hpp"
int main() {
  double A[9];
  while (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf", A, A + 1, A + 2, A + 3, A + 4, A + 5, A + 6, A + 7, A + 8) == 9) {
    double U[9], S[3], V[9], R[9];
    vba::btc_svd3(A, U, S, V);
    vba::btc_kabsch(U, V, R);
    for (int k = 0; k < 9; k++) std::printf("%.17g ", R[k]);
    std::printf("\n");
  }
  return 0;
}
''')
    exe = tmp_path / "s"
    inc = os.path.join(ROOT, "voxel-slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + inc, str(src), "-o", str(exe)])
    rng = np.random.default_rng(5)
    mats = []
    for k in range(300):
        a = rng.normal(size=(3, 3)) * 4
        b = a @ bo.so3_exp(rng.normal(size=3)).T + rng.normal(size=3) * 0.01
        if k % 3 == 1:
            a -= a.mean(1, keepdims=True); b -= b.mean(1, keepdims=True)        # triangle minus centroid: rank 2
        if k % 3 == 2:
            b = b * np.array([[1.0], [1.0], [-1.0]])                              # mirrored: the det < 0 branch
        mats.append(a @ b.T)
    out = subprocess.run([str(exe)], input="\n".join(" ".join("%.17g" % v for v in m.ravel()) for m in mats) + "\n",
                         capture_output=True, text=True, check=True).stdout.split("\n")
    for m, line in zip(mats, out):
        R = np.array([float(v) for v in line.split()]).reshape(3, 3)
        U, S, Vt = np.linalg.svd(m)
        Rn = Vt.T @ U.T
        if np.linalg.det(Rn) < 0:
            Rn = Vt.T @ np.diag([1.0, 1.0, -1.0]) @ U.T
        assert np.abs(R - Rn).max() < 1e-10
