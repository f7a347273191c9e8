"""CPU-side checks of the surfel map and the registration against it (vba_surfel_map_build, vba_surfel_register, DESIGN.md section
26): the new prototypes, the key-of-mean property the map's key rests on, the restatement tests/surfreg_ref.py against the host
build of csrc/vba_surfreg_math.hpp (tests/host/surfreg_host.cpp) point for point and against exact sums, mutations of the
restatement, the loop from the starts of the tests with the conditions its fixtures must meet, and one sanitizer run of the host
program as a stand-alone binary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import export_voxel_ref as ev
import surfel_ref as sr
import surfreg_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("surfreg")
    return rr.build_host(d), d


@pytest.fixture(scope="module")
def scenes():
    """name -> dict(S, pnt, Rg, tg, per voxel: rec, cov, map)"""
    out = {}
    for name in ("near", "far"):
        _, S = rr.world(name)
        pnt, Rg, tg = rr.scan_of(S, name)
        per = {}
        for voxel in rr.VOXELS:
            rec, cov = rr.records_of(S, voxel)
            per[voxel] = dict(rec=rec, cov=cov, map=rr.Map(rec, cov, voxel, rr.SIGMA, rr.MIN_COUNT))
        out[name] = dict(S=S, pnt=pnt, Rg=Rg, tg=tg, per=per)
    return out


def test_new_prototypes(capi):
    from voxel_slam_amd import abi
    want = {"vba_surfel_map_create": "i:pp", "vba_surfel_map_destroy": "i:p", "vba_surfel_map_reserve": "i:pqq",
            "vba_surfel_map_allocations": "i:ppp", "vba_surfel_map_build": "i:pqppddip", "vba_surfel_map_build_from_kf": "i:pipiddip",
            "vba_surfel_map_size": "i:pppp", "vba_debug_surfel_map_read": "i:pqppppppp", "vba_surfel_reg_default_params": "v:p", "vba_surfel_register": "i:pqppppp",
            "vba_debug_surfel_reg_pass": "i:pqpppppppp"}
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    lib = capi.load()
    for name, proto in want.items():
        assert re.search(r"\b(?:int|void)\s+%s\s*\(" % name, hdr), name
        assert abi.PROTOTYPES.get(name) == proto and name in capi.EXPORTS and hasattr(lib, name), name
    for m in ("build", "build_from_kf", "register", "debug_pass", "reserve", "size"):
        assert hasattr(capi.SurfelMap, m), m
    p = capi.surfel_reg_default_params()
    assert (p.gate, p.neighbors, p.max_iter, p.min_matches, p.eps_rot, p.eps_tra) == (3.0, 7, 30, 50, 1e-5, 1e-5)
    assert C.sizeof(capi.SurfelRegReport) == 16 + 4 * 32 + 3 * 8 * 32 + 8 * 30 and C.sizeof(capi.SurfelRegParams) == 40
    # without an object every call is refused before it touches a device, outputs untouched
    n = C.c_int64(-77); a = C.c_int(-77); b = C.c_int64(-77); h = C.c_void_p(77)
    assert lib.vba_surfel_map_create(None, C.byref(h)) == capi.ERR_BAD_ARG and h.value == 77
    assert lib.vba_surfel_map_build(None, 1, None, None, 0.5, 0.02, 5, C.byref(n)) == capi.ERR_BAD_ARG and n.value == -77
    assert lib.vba_surfel_map_build_from_kf(None, 1, None, 1, 0.5, 0.02, 5, C.byref(n)) == capi.ERR_BAD_ARG and n.value == -77
    assert lib.vba_surfel_map_allocations(None, C.byref(a), C.byref(b)) == capi.ERR_BAD_ARG and (a.value, b.value) == (-77, -77)
    assert lib.vba_surfel_map_reserve(None, 1, 1) == capi.ERR_BAD_ARG and lib.vba_surfel_map_destroy(None) == capi.ERR_BAD_ARG
    R = np.eye(3); t = np.zeros(3)
    assert lib.vba_surfel_register(None, 1, None, C.byref(p), R.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), None) == capi.ERR_BAD_ARG
    assert np.array_equal(R, np.eye(3))


def test_arithmetic_header_is_shared():
    """the arithmetic is one header without kernels that the host program compiles, and the unit is built without contraction"""
    csrc = os.path.join(ROOT, "voxel-slam_amd", "csrc")
    math = open(os.path.join(csrc, "vba_surfreg_math.hpp")).read()
    assert "__global__" not in math and "hipStream_t" not in math
    assert "vba_surfreg_math.hpp" in open(os.path.join(csrc, "vba_kernels_surfreg.hpp")).read()
    assert "vba_surfreg_math.hpp" in open(os.path.join(ROOT, "tests", "host", "surfreg_host.cpp")).read()
    flags = [line for line in open(os.path.join(csrc, "Makefile")) if "-ffp-contract=off" in line and "UNITFLAGS" in line]
    assert len(flags) == 1 and "vba_surfreg.o" in flags[0].split(":")[0].split()


# ---------------------------------------------------------------- the key of the mean
def test_key_of_the_narrowed_mean_is_the_voxels_key(scenes, host):
    """what lets the map key a cell by its record alone: the f64 mean narrowed to float lies between the voxel's smallest and
    largest member, and the per-axis index is monotone in the float coordinate.  The key the shared header gives a record (the
    host program's) is the key of the record's voxel."""
    for name in ("near", "far"):
        S = scenes[name]["S"]
        for voxel in rr.VOXELS:
            pv = scenes[name]["per"][voxel]
            h = rr.host_run(host[0], host[1], pv["rec"], pv["cov"], scenes[name]["pnt"][:1], np.eye(3), np.zeros(3), voxel, min_count=1, tag="key")
            assert h["n_cells"] == len(pv["rec"]) and h["dup"] == 0
            assert np.array_equal(h["key"], rr.pack(rr.axis_keys(S[:, :3], voxel)[ev.centroids(S, voxel)[0]])), (name, voxel)
            first, cnt, vox, xyz, _ = ev.centroids(S, voxel)
            members = rr.axis_keys(S[:, :3], voxel)
            assert np.array_equal(members, members[first][vox])                      # (every member has its voxel's key)
            assert np.array_equal(rr.axis_keys(xyz, voxel), members[first]), (name, voxel)
            assert len(np.unique(rr.pack(members[first]))) == len(first)             # 21 bits per axis keep the voxels apart
            assert (members < 0).any()
    assert scenes["near"]["per"][0.5]["map"].n_cells == 151 and scenes["near"]["per"][1.0]["map"].n_cells == 56
    assert scenes["far"]["per"][0.5]["map"].n_cells == 151 and scenes["far"]["per"][1.0]["map"].n_cells in (54, 55, 56)


# ---------------------------------------------------------------- host program against the restatement, one pass
def _pass_case(scenes, host, name, voxel, nb, which="small"):
    sc = scenes[name]; pv = sc["per"][voxel]
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], which)
    ps = rr.one_pass(pv["map"], sc["pnt"], R0, t0, 3.0, nb)
    h = rr.host_run(host[0], host[1], pv["rec"], pv["cov"], sc["pnt"], R0, t0, voxel, neighbors=nb, max_iter=1, tag="pass")
    return sc, pv, R0, t0, ps, h


@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", rr.VOXELS)
def test_weight_by_residual_and_host_bits(scenes, host, name, voxel):
    sc, pv, R0, t0, ps, h = _pass_case(scenes, host, name, voxel, 1)
    mp = pv["map"]
    keep = mp.rows
    assert h["n_cells"] == mp.n_cells and h["dup"] == 0 and not mp.dup
    assert np.array_equal(h["key"][keep], mp.keys) and (np.delete(h["key"], keep) == np.uint64(2 ** 64 - 1)).all()
    assert np.array_equal(h["W"][keep], mp.W[keep])                                   # the header's bits
    worst = rr.weight_check(pv["cov"][keep], rr.SIGMA, mp.W[keep])
    print("%s voxel %g: %d cells, W residual / bar %.3f" % (name, voxel, mp.n_cells, worst))
    assert worst <= 1.0
    # W = C^-1 without sigma is another matrix altogether
    assert rr.weight_check(pv["cov"][keep][:20], rr.SIGMA, rr.weight(pv["cov"][keep][:20], rr.SIGMA, with_sigma=False)) > 1e6


@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", rr.VOXELS)
@pytest.mark.parametrize("nb", [1, 7])
def test_host_pass_equals_restatement(scenes, host, name, voxel, nb):
    sc, pv, R0, t0, ps, h = _pass_case(scenes, host, name, voxel, nb)
    assert not ps["ties"].any()                                                       # fixture condition: no candidate tie
    assert np.array_equal(h["cell"], ps["cell"]) and np.array_equal(h["gate"].astype(bool), ps["gate"])
    assert np.array_equal(h["terms"], ps["terms"])                                    # the 29 terms of every point, bit for bit
    n = len(sc["pnt"])
    assert 0.9 * n < ps["gate"].sum() < n and (ps["cell"] < 0).sum() < 0.05 * n
    exact, ab = rr.exact_sums(ps)
    bar = rr.sums_bar(int(ps["gate"].sum()), ab)
    for got, what in ((h["sums"], "host order"), (ps["sums"], "chain")):
        ratio = np.abs(got - exact) / np.maximum(bar, 1e-300)
        ratio[28] = 0.0 if got[28] == exact[28] else np.inf
        print("%s voxel %g neighbors %d %s: %d gated, worst sum error / bar %.4f" % (name, voxel, nb, what, ps["gate"].sum(), ratio.max()))
        assert ratio.max() <= 1.0
    bw, fw = rr.step_check(h["sums"], h["dx"])
    print("  step: backward %.3f forward %.3f of their bars" % (bw, fw))
    assert bw <= 1.0 and fw <= 1.0


# ---------------------------------------------------------------- mutations
def _beyond(ps, mut, hsums=None):
    """a mutation's sums leave the bar around the exact sums, and, given the host program's sums (which lie inside it), are more
    than two bars away from those"""
    exact, ab = rr.exact_sums(ps)
    bar = rr.sums_bar(int(ps["gate"].sum()), ab)
    out = (np.abs(mut["sums"] - exact) > bar).any()
    return out and (hsums is None or (np.abs(mut["sums"] - hsums) > 2 * bar).any())


def test_mutations_leave_the_bar(scenes, host):
    sc = scenes["near"]; pv = sc["per"][0.5]; mp = pv["map"]
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    ps = rr.one_pass(mp, sc["pnt"], R0, t0, 3.0, 7)
    hs = rr.host_run(host[0], host[1], pv["rec"], pv["cov"], sc["pnt"], R0, t0, 0.5, neighbors=7, max_iter=1, tag="mut")["sums"]
    assert not _beyond(ps, ps) and not _beyond(ps, dict(sums=hs))
    nosig = rr.Map(pv["rec"], pv["cov"], 0.5, rr.SIGMA, rr.MIN_COUNT, with_sigma=False)
    assert _beyond(ps, rr.one_pass(nosig, sc["pnt"], R0, t0, 3.0, 7), hs)                 # W = C^-1
    plus = rr.one_pass(mp, sc["pnt"], R0, t0, 3.0, 7, jsign=+1.0)                     # J = [+R hat(p) | I]
    assert _beyond(ps, plus, hs) and np.array_equal(plus["gate"], ps["gate"])
    lin = rr.one_pass(mp, sc["pnt"], R0, t0, 3.0, 7, gate_squared=False)              # m < gate
    assert lin["gate"].sum() < ps["gate"].sum() and _beyond(ps, lin, hs)
    allrec = rr.Map(pv["rec"], pv["cov"], 0.5, rr.SIGMA, rr.MIN_COUNT, ignore_min_count=True)   # min_count ignored
    assert allrec.n_cells > mp.n_cells
    extra = rr.one_pass(allrec, sc["pnt"], R0, t0, 3.0, 7)
    assert not np.array_equal(extra["cell"], ps["cell"]) and _beyond(ps, extra, hs)


def test_constructed_tie_goes_to_the_earlier_candidate(host):
    rec, cov, pnt, R, t = rr.tie_case()
    mp = rr.Map(rec, cov, 0.5, rr.SIGMA, 5)
    ps = rr.one_pass(mp, pnt, R, t, 3.0, 7)
    assert ps["ties"].all() and ps["gate"].all() and ps["cell"][0] == 1
    h = rr.host_run(host[0], host[1], rec, cov, pnt, R, t, 0.5, min_count=5, neighbors=7, max_iter=1, min_matches=1, tag="tie")
    assert h["cell"][0] == 1 and h["gate"][0] == 1 and np.array_equal(h["terms"], ps["terms"])
    later = rr.one_pass(mp, pnt, R, t, 3.0, 7, tie="later")
    other = rr.one_pass(mp, pnt, R, t, 3.0, 7, order=(rr.ORDER[1], rr.ORDER[0]) + rr.ORDER[2:])
    for mut in (later, other):
        assert mut["cell"][0] == 0 and _beyond(ps, mut)
    assert rr.one_pass(mp, pnt, R, t, 3.0, 1)["cell"][0] == 1 and not rr.one_pass(mp, pnt, R, t, 3.0, 1)["ties"].any()


# ---------------------------------------------------------------- the loop
def loop_inputs(scenes, case):
    name, which, nb = case
    voxel = rr.LOOP_VOXEL[which]
    sc = scenes[name]; pv = sc["per"][voxel]
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], which)
    return sc, pv, voxel, R0, t0


@pytest.mark.parametrize("case", rr.LOOP_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_loop_converges_to_the_generating_pose(scenes, host, case):
    sc, pv, voxel, R0, t0 = loop_inputs(scenes, case)
    nb = case[2]; n = len(sc["pnt"])
    lp = rr.loop(pv["map"], sc["pnt"], R0, t0, neighbors=nb)
    # conditions on the fixture (asserted on the restatement: on a failure change the start's seed, not the bar)
    eps = 1e-5
    assert lp["converged"] and not lp["lost"] and not lp["singular"] and lp["iters"] >= 3
    assert max(lp["step_rot"][-1], lp["step_tra"][-1]) < eps / 10
    assert max(lp["step_rot"][-2], lp["step_tra"][-2]) > 10 * eps
    h = rr.host_run(host[0], host[1], pv["rec"], pv["cov"], sc["pnt"], R0, t0, voxel, neighbors=nb, max_iter=30, tag="loop")
    assert h["converged"] == 1 and h["lost"] == 0 and h["singular"] == 0 and h["done"] == 1 and h["eig_ok"] == 1
    assert h["iters"] == lp["iters"] and list(h["matches"][:h["iters"]]) == lp["matches"]
    assert h["matches"][h["iters"] - 1] >= 0.95 * n
    dt, dr = rr.pose_distance(h["R"], h["t"], sc["Rg"], sc["tg"])
    print("%s %s neighbors %d voxel %g: %d iterations, matches %s, %.2e m %.2e rad from the generating pose, eig_tt %s"
          % (case[0], case[1], nb, voxel, h["iters"], list(h["matches"][:h["iters"]]), dt, dr, h["eig_tt"]))
    assert dt < voxel / 100 and dr < voxel / 100          # the line between convergence and a wrong basin (expected 1e-4 .. 1e-3: the estimator's bias)
    assert np.allclose(h["cost"][:h["iters"]], lp["cost"], rtol=1e-6) and h["eig_tt"][0] > 1e5
    assert np.linalg.eigvalsh(rr.unpack_H(h["H"])).min() > 1e5


def test_host_program_under_sanitizers(scenes, tmp_path):
    """the host program alone, a stand-alone binary with -fsanitize=address,undefined: one pass with misses and one loop"""
    exe = rr.build_host(tmp_path, sanitize=True)
    sc = scenes["near"]; pv = sc["per"][0.5]
    R0, t0 = rr.start_of(sc["Rg"], sc["tg"], "small")
    far_pts = np.concatenate([sc["pnt"][:300], sc["pnt"][:40] + 50.0])
    a = rr.host_run(exe, tmp_path, pv["rec"], pv["cov"], far_pts, R0, t0, 0.5, neighbors=7, max_iter=30, tag="san")
    assert a["converged"] == 1 and (a["cell"][300:] == -1).all()
    rec, cov, pnt, R, t = rr.tie_case()
    b = rr.host_run(exe, tmp_path, rec, cov, pnt, R, t, 0.5, neighbors=7, max_iter=2, min_matches=5, tag="san2")
    assert b["lost"] == 1 and b["iters"] == 1
