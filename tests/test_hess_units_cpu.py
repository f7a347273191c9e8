"""The shape header of the dense-tile Hessian pass (csrc/vba_hess_units.hpp) on the CPU: tests/host/hess_units_host.cpp is built by g++
with the address and undefined-behaviour sanitizers and run as a child process.
  * the unit table HessCfg2<W>::unit(wave, t), W = 2..16, against the decode the kernel ran per tile before (restated here), with every
    (upper-triangle tile, k-split) pair exactly once and UPW units to every wave;
  * the LDS budget of the epilogue's staging area;
  * group8_tree, the sum the epilogue forms of an aligned group of 8 staged columns, against a numpy emulation of the three
    data-parallel-primitive steps it replaced (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, an add after each)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WS = list(range(2, 17))


@pytest.fixture(scope="module")
def host():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_hess_units_"), "hess_units_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", out, os.path.join(HERE, "host", "hess_units_host.cpp")])
    return out


@pytest.fixture(scope="module")
def table(host):
    r = subprocess.run([host, "table"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    cfg, units = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "W":
            cfg[int(f[1])] = {f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}
        else:
            W, w, t, u, ta, tb, ks = map(int, f[1:])
            units.setdefault(W, {})[(w, t)] = (u, ta, tb, ks)
    assert sorted(cfg) == WS and sorted(units) == WS
    return cfg, units


def old_decode(c, wv, t):
    """what k_hessian2 computed per tile, per unit, from tid >> 6"""
    unit = wv * c["UPW"] + t
    u, ksp = unit % c["NU"], unit // c["NU"]
    p, ta = u, 0
    while p >= c["NT16"] - ta:
        p -= c["NT16"] - ta
        ta += 1
    return u, ta, ta + p, ksp


@pytest.mark.parametrize("W", WS)
def test_unit_table(table, W):
    c, un = table[0][W], table[1][W]
    assert c["NWV"] == 4 and c["NT16"] == (6 * W + 15) // 16 and c["NU"] == c["NT16"] * (c["NT16"] + 1) // 2
    assert c["NU"] * c["KS"] == c["NWV"] * c["UPW"] and c["KSTEPS"] * 4 * c["KS"] == c["NK"]
    assert sorted(un) == [(w, t) for w in range(c["NWV"]) for t in range(c["UPW"])]          # UPW units to every wave
    for (w, t), got in un.items():
        assert got == old_decode(c, w, t), (w, t)
    tiles = [(a, b) for a in range(c["NT16"]) for b in range(a, c["NT16"])]                  # row-major upper triangle, as tl_fetch numbers it
    assert sorted((ta, tb, ks) for _, ta, tb, ks in un.values()) == sorted((a, b, k) for a, b in tiles for k in range(c["KS"]))
    assert all(tiles[u] == (ta, tb) for u, ta, tb, _ in un.values())
    assert all(ta < 8 and tb < 8 and ks < 4 for _, ta, tb, ks in un.values())               # the kernel packs a unit into a byte


def test_every_distinct_shape_is_in_the_gpu_edge_cases(table):
    """tests/test_gpu_hess_edges.py runs W = 2, 3, 6, 10, 11, 16: every distinct (NU, KS, UPW), and the one window without PRESCALE"""
    cfg = table[0]
    shape = lambda W: (cfg[W]["NU"], cfg[W]["KS"], cfg[W]["UPW"])
    assert {shape(W) for W in WS} == {shape(W) for W in (2, 3, 6, 10, 11, 16)}
    assert [W for W in WS if not cfg[W]["PRESCALE"]] == [3]


def test_lds_budget(table):
    cfg = table[0]
    for W in WS:
        c = cfg[W]
        staged = (c["NU"] * 256 if c["KS"] > 1 else 0) + 28 * 257 + 8
        assert c["LDS_EPI"] == 8 * staged
        assert c["LDS_BYTES"] == max(c["LDS_MAIN"], c["LDS_EPI"]) <= 150 * 1024                # what the launch opts in to (kLiRideLds)
    assert cfg[10]["LDS_EPI"] < cfg[10]["LDS_MAIN"]                                           # the bench window's launch is unchanged
    assert [W for W in WS if cfg[W]["LDS_EPI"] > cfg[W]["LDS_MAIN"]] == [11, 12, 13, 14, 15, 16]   # these grow


def dpp_group8(x):
    """[N, 8] -> [N, 8]: the three steps of the former group8_sum on every aligned group of 8 lanes, each lane adding in its own order"""
    x = x + x[:, [1, 0, 3, 2, 5, 4, 7, 6]]          # quad_perm [1,0,3,2]
    x = x + x[:, [2, 3, 0, 1, 6, 7, 4, 5]]          # quad_perm [2,3,0,1]
    return x + x[:, ::-1]                           # row_half_mirror


def test_group8_tree_is_the_dpp_tree(host):
    rng = np.random.default_rng(8)
    N = 4096
    x = rng.normal(size=(N, 8)) * 2.0 ** rng.choice([-40, 0, 40], size=(N, 8))               # mixed magnitudes and signs
    x[:64] = np.abs(x[:64])
    x[64:128, 3:] = 0.0                                                                       # partly filled groups (+0.0 columns)
    x[128:192] = 0.0
    x[192:256, ::2] = -x[192:256, 1::2]                                                       # exact cancellation inside the pairs
    want = dpp_group8(x)
    assert all(np.array_equal(want[:, 0], want[:, k]) for k in range(8))                      # every lane of a group holds the same bits
    assert (want[:, 0] != np.cumsum(x, 1)[:, 7]).mean() > 0.25                                 # the association matters: not the left-to-right sum
    r = subprocess.run([host, "tree", str(N)], input=x.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-4000:]
    got = np.frombuffer(r.stdout, dtype=np.float64)
    assert got.shape == (N,) and np.array_equal(got, want[:, 0])
    assert np.array_equal(np.signbit(got), np.signbit(want[:, 0]))


def test_unknown_case_is_an_error(host):
    assert subprocess.run([host, "no_such_case"], capture_output=True, timeout=60).returncode == 2
