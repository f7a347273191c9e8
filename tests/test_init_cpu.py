"""Host-only pieces of vba_motion_init (Initialization::motion_init, voxelslam.cpp:617-819) against numpy restatements:
the backward IMU pose table of motion_blur (VS:508-544) and align_gravity (VS:470-497).  No device needed."""
import os

import numpy as np
import pytest

import init_oracle


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def _rot(rng, scale=1.0):
    w = rng.normal(0, scale, 3)
    return init_oracle.exp_dt(w, 1.0)


def _state(rng, with_v=True, g=(0.0, 0.0, -9.81)):
    x = np.zeros(25)
    x[0] = rng.uniform(0, 100)
    x[1:10] = _rot(rng).ravel()
    x[10:13] = rng.normal(0, 3, 3)
    x[13:16] = rng.normal(0, 1, 3) if with_v else 0.0
    x[16:19] = rng.normal(0, 0.01, 3)
    x[19:22] = rng.normal(0, 0.05, 3)
    x[22:25] = g
    return x


def _deque(rng, m, t0):
    t = t0 + np.cumsum(rng.uniform(0.004, 0.006, m))
    gyr = rng.normal(0, 0.3, (m, 3))
    acc = rng.normal(0, 0.2, (m, 3)) + np.array([0.0, 0.0, 1.0])
    return np.column_stack([t, gyr, acc])


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("with_v", [True, False])
def test_imu_poses_match_restatement(capi, seed, with_v):
    rng = np.random.default_rng(1000 + seed)
    m = int(rng.integers(2, 40))
    imu = _deque(rng, m, 50.0)
    xc, xl = _state(rng, with_v), _state(rng, with_v)
    beg = imu[0, 0] + rng.uniform(-0.02, 0.02)
    sg = float(rng.choice([1.0, 9.81, 9.7]))
    got = capi.init_imu_poses(imu, xc, xl, beg, sg)
    ref = init_oracle.imu_poses(imu, xc, xl, beg, sg)
    assert got.shape == (m - 1, 22)
    scale = np.maximum(np.abs(ref), 1.0)
    assert np.max(np.abs(got - ref) / scale) < 1e-12      # measured worst 5.3e-15
    assert np.all(np.diff(got[:, 0]) < 0)                  # push order: time descending


def test_imu_poses_short_deque(capi):
    rng = np.random.default_rng(7)
    assert capi.init_imu_poses(_deque(rng, 1, 0.0), _state(rng), _state(rng), 0.0).shape == (0, 22)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("gz_sign", [-1.0, 1.0])
def test_align_gravity_match_restatement(capi, seed, gz_sign):
    rng = np.random.default_rng(2000 + seed)
    n = int(rng.integers(1, 12))
    g = rng.normal(0, 1.0, 3)
    g[2] = gz_sign * (9.0 + rng.uniform(0, 1))          # both branches of n1[2] (VS:476-477)
    xs = np.stack([_state(rng, True, g) for _ in range(n)])
    got = capi.init_align_gravity(xs)
    ref = init_oracle.align_gravity(xs)
    assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)) < 1e-12   # measured worst 8.9e-16
    gn = np.linalg.norm(g)
    assert np.allclose(got[:, 22:25], [0.0, 0.0, np.sign(gz_sign) * gn], atol=1e-12)
    assert np.allclose(got[:, 0], xs[:, 0]) and np.allclose(got[:, 16:22], xs[:, 16:22])
