"""CPU-side checks of the prior-map odometry update (vba_odom_surfel_update): the new prototypes, the numpy
restatement tests/surfodom_ref.py against the host build of csrc/vba_surfreg_math.hpp + csrc/vba_odom_ekf.hpp
(tests/host/surfodom_host.cpp) point for point and sum for sum, the sums against exact sums, the EKF step against numpy's solve,
the loop cases with the conditions their fixtures must meet, mutations, and one sanitizer run of the host program as a stand-alone
binary."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surfodom_ref as so
import surfreg_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("surfodom")
    return so.build_host(d), d


@pytest.fixture(scope="module")
def scenes():
    """name -> dict(pnt, Rg, tg, per voxel: rec, cov, map)"""
    out = {}
    for name in ("near", "far"):
        _, S = rr.world(name)
        pnt, Rg, tg = rr.scan_of(S, name)
        per = {}
        for voxel in rr.VOXELS:
            rec, cov = rr.records_of(S, voxel)
            per[voxel] = dict(rec=rec, cov=cov, map=rr.Map(rec, cov, voxel, rr.SIGMA, rr.MIN_COUNT))
        out[name] = dict(pnt=pnt, Rg=Rg, tg=tg, per=per)
    return out


def _inputs(scenes, name, voxel, which):
    sc = scenes[name]; pv = sc["per"][voxel]
    R0, t0 = so.start_of(sc["Rg"], sc["tg"], which)
    return sc, pv, R0, t0, so.state_of(R0, t0), so.prior_cov()


def _host(host, pv, pnt, state, P, voxel, **kw):
    return so.host_run(host[0], host[1], pv["rec"], pv["cov"], pnt, state, P, voxel, **kw)


def test_new_prototypes(capi):
    from voxel_slam_amd import abi
    want = {"vba_surfel_odom_default_params": "v:p", "vba_odom_surfel_update": "i:ppipppppp", "vba_odom_surfel_update_on_state": "i:pppippppp",
            "vba_debug_odom_surfel_sums": "i:ppippppipppppp"}
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    lib = capi.load()
    for name, proto in want.items():
        assert re.search(r"\b(?:int|void)\s+%s\s*\(" % name, hdr), name
        assert abi.PROTOTYPES.get(name) == proto and name in capi.EXPORTS and hasattr(lib, name), name
    assert len(capi.EXPORTS) == 204 and capi.EXPORTS[-4:] == list(want)
    assert hasattr(capi.Context, "odom_surfel_update") and hasattr(capi.Context, "debug_odom_surfel_sums") and hasattr(capi.OdomState, "surfel_update")
    p = capi.surfel_odom_default_params()
    assert (p.gate, p.neighbors, p.min_matches, p.min_eig) == (3.0, 7, 30, 0.0) and C.sizeof(capi.SurfelOdomParams) == 24
    # without objects every call is refused before it touches a device, outputs untouched
    st = np.arange(25.0); cov = np.arange(225.0); ok = C.c_int(-77); nb = C.c_int(-77)
    sp, cp = st.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p)
    assert lib.vba_odom_surfel_update(None, None, 0, None, C.byref(p), sp, cp, C.byref(ok), None) == capi.ERR_BAD_ARG
    assert lib.vba_odom_surfel_update_on_state(None, None, None, 0, None, C.byref(p), C.byref(ok), None, sp) == capi.ERR_BAD_ARG
    assert lib.vba_debug_odom_surfel_sums(None, None, 1, sp, C.byref(p), sp, sp, 0, None, None, None, None, None, C.byref(nb)) == capi.ERR_BAD_ARG
    assert ok.value == -77 and nb.value == -77 and np.array_equal(st, np.arange(25.0)) and np.array_equal(cov, np.arange(225.0))


def test_kernel_and_arithmetic_are_shared():
    """the point loop's body exists once, for both kernels; the host program compiles the two arithmetic headers; the kernel unit is
    the one built without contraction and the build recipe has no new unit"""
    csrc = os.path.join(ROOT, "voxel-slam_amd", "csrc")
    k = open(os.path.join(csrc, "vba_kernels_surfreg.hpp")).read()
    assert k.count("sreg_point(") == 1 and k.count("sreg_accum_waves(") == 3 and "k_sodom_accum" in k
    hp = open(os.path.join(ROOT, "tests", "host", "surfodom_host.cpp")).read()
    assert "vba_surfreg_math.hpp" in hp and "vba_odom_ekf.hpp" in hp
    units = [line for line in open(os.path.join(csrc, "Makefile")) if line.startswith("UNITS")][0].split("=")[1].split()
    assert len(units) == 18 and "vba_surfreg" in units
    assert "k_sodom_accum" in open(os.path.join(csrc, "vba_surfreg.hip")).read() and "surfel_odom_queue" in open(os.path.join(csrc, "vba_ctx.hpp")).read()


def test_column_mapping_and_reduction_order():
    s = np.arange(1.0, 30.0)
    r = so.to34(s)
    assert np.array_equal(r[:21], s[:21]) and np.array_equal(r[21:27], -s[21:27]) and np.array_equal(r[27:33], s[15:21]) and r[33] == s[28]
    # the seven-group reduction is not the chain: values that round differently in the two orders
    rng = np.random.default_rng(0)
    part = rng.normal(size=(50, 34)) * 10.0 ** rng.integers(-8, 8, (50, 34))
    got = so.sum_partials(part)
    want = np.zeros(34)
    for c in range(34):
        g = [0.0] * 7
        for i in range(c, 50 * 34, 34):
            g[(i % 238) // 34] += part.reshape(-1)[i]
        w = g[0]
        for k in range(1, 7):
            w += g[k]
        want[c] = w
    assert np.array_equal(got, want) and not np.array_equal(got, np.add.accumulate(part, axis=0)[-1])
    assert np.array_equal(so.sum_partials(np.zeros((0, 34))), np.zeros(34))


# ---------------------------------------------------------------- host program against the restatement, one point loop
@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", rr.VOXELS)
@pytest.mark.parametrize("nb", [1, 7])
def test_host_point_loop_equals_restatement(scenes, host, name, voxel, nb):
    sc, pv, R0, t0, state, P = _inputs(scenes, name, voxel, "track")
    h = _host(host, pv, sc["pnt"], state, P, voxel, neighbors=nb, tag="pass")
    pl = so.point_loop(pv["map"], sc["pnt"], R0, t0, 3.0, nb)
    assert not pl["ps"]["ties"].any()
    assert np.array_equal(h["cell"], pl["cell"]) and np.array_equal(h["gate"].astype(bool), pl["gate"])
    assert h["nb"] == 7 and np.array_equal(h["partial"], pl["partial"]) and np.array_equal(h["cost"], pl["cost"])
    assert np.array_equal(h["sums"], pl["sums"])                                      # the 34 sums, bit for bit
    exact, bar = so.exact34(pl["ps"])
    ratio = np.abs(h["sums"] - exact) / np.maximum(bar, 1e-300)
    ratio[33] = 0.0 if h["sums"][33] == exact[33] else np.inf
    print("%s voxel %g neighbors %d: %d gated, worst sum error / bar %.4f" % (name, voxel, nb, pl["gate"].sum(), ratio.max()))
    assert ratio.max() <= 1.0 and 0.9 * len(sc["pnt"]) < h["sums"][33] < len(sc["pnt"])
    assert np.array_equal(h["sums"][27:33], h["sums"][15:21])                         # the same chain of the same terms


def test_host_point_loop_beyond_one_tile_per_lane(scenes, host):
    """more points than 1024 workgroups of 256 take at once: lanes chain over strided tiles (the restatement's order, the host's bits)"""
    sc, pv, R0, t0, state, P = _inputs(scenes, "near", 0.5, "track")
    n = 1024 * 256 + 257
    pnt = np.tile(sc["pnt"], (n // len(sc["pnt"]) + 1, 1))[:n]
    h = _host(host, pv, pnt, state, P, 0.5, neighbors=1, tag="cap")
    pl = so.point_loop(pv["map"], pnt, R0, t0, 3.0, 1)
    assert h["nb"] == 1024 and np.array_equal(h["cell"], pl["cell"]) and np.array_equal(h["partial"], pl["partial"]) and np.array_equal(h["sums"], pl["sums"])


# ---------------------------------------------------------------- the EKF step
@pytest.fixture(scope="module")
def ekf(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("surfodom_ekf")), "libodomekfhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", out, os.path.join(ROOT, "tests", "host", "odom_ekf_host.cpp")])
    return C.CDLL(out)


@pytest.mark.parametrize("name,voxel,which", [("near", 0.5, "small"), ("far", 1.0, "track"), ("near", 1.0, "fine")])
def test_step_against_numpy_solve(scenes, ekf, name, voxel, which):
    """the step of csrc/vba_odom_ekf.hpp on the sums of a point loop against np.linalg.inv, with the bar of tests/test_odom_ekf_cpu.py:
    100 kappa 15 eps of the solution's max-norm"""
    sc, pv, R0, t0, state, P = _inputs(scenes, name, voxel, which)
    s34 = so.point_loop(pv["map"], sc["pnt"], R0, t0, 3.0, 7)["sums"]
    cov_inv = np.ascontiguousarray(np.linalg.inv(P))
    p = lambda a: a.ctypes.data_as(DP)
    sol = np.zeros(15); G = np.zeros(90); K = np.zeros(90)
    ekf.odom_ekf_step_host(p(s34), p(cov_inv), p(state), p(state), p(sol), p(G), p(K))
    ref, G_ref, A = so.ekf_step(s34, cov_inv, state, state)
    kappa = np.linalg.cond(A)
    bar = 100 * kappa * 15 * EPS
    err = np.abs(sol - ref).max() / np.abs(ref).max()
    print("%s %g %s: kappa %.3g, solution error %.3g of its max-norm, bar %.3g" % (name, voxel, which, kappa, err, bar))
    assert err <= bar and np.abs(G.reshape(15, 6) - G_ref[:, :6]).max() <= bar * np.abs(G_ref).max()
    # the step moves towards the generating pose, and v, bg, ba move with it through the correlations of P
    d0 = np.linalg.norm(t0 - sc["tg"]); d1 = np.linalg.norm(t0 + sol[3:6] - sc["tg"])
    # (the fine start is as near as the estimator's bias, 1e-4 .. 7e-4 m: no step halves that)
    assert (which == "fine" or d1 < 0.5 * d0) and np.abs(sol[6:15]).min() > 0


# ---------------------------------------------------------------- the loop
@pytest.mark.parametrize("case", so.LOOP_CASES, ids=so.case_id)
def test_loop_cases(scenes, host, case):
    name, voxel, which, nb = case
    sc, pv, R0, t0, state, P = _inputs(scenes, name, voxel, which)
    lp = so.loop(pv["map"], sc["pnt"], state, P, neighbors=nb)
    # fixture condition (asserted on the restatement, not tuned on the device): no convergence decision that can change the stop
    # is near its threshold
    dec = so.decisive(lp)
    assert all(r < 0.5 or r > 2.0 for r in dec), dec
    assert lp["iterations"] == so.EXPECTED_ITERATIONS[which]
    h = _host(host, pv, sc["pnt"], state, P, voxel, neighbors=nb, tag="loop")
    assert h["iterations"] == lp["iterations"] and np.array_equal(h["match_num"], lp["match_num"]) and h["ok"] == lp["ok"] == 1
    assert h["rematch_num"] == lp["rematch_num"]
    assert 1516 <= h["match_num"][:h["iterations"]].min() and h["match_num"].max() <= 1550 and (h["match_num"][h["iterations"]:] == 0).all()
    dt, dr = so.pose_distance(h["state"], sc["Rg"], sc["tg"])
    print("%s: %d iterations, ratios %s, matches %s, %.2e m %.2e rad from the generating pose, eig %.3g"
          % (so.case_id(case), h["iterations"], ["%.3g" % r for r in lp["ratio"]], list(h["match_num"]), dt, dr, h["eig_min"]))
    assert dt < voxel / 100 and dr < voxel / 100
    assert 4.0e5 < h["eig_min"] < 5.5e5 and abs(h["eig_min"] - lp["eig_min"]) < 1e-9 * lp["eig_min"]
    # numpy's inverse against the header's elimination: within the bars the device is held to
    assert so.within(so.errors(lp, h), so.bars(case, h)), (so.errors(lp, h), so.bars(case, h))
    # the update is a MAP estimate: the covariance shrinks in the pose block and stays symmetric to rounding
    assert (np.diag(h["cov"])[:6] < np.diag(P)[:6]).all() and np.abs(h["cov"] - h["cov"].T).max() < 1e-12 * np.abs(P).max()
    assert np.abs(h["state"][13:22] - state[13:22]).min() > 0                         # v, bg, ba moved


@pytest.mark.parametrize("case", [("near", 0.5, "fine", 7), ("far", 1.0, "track", 1)], ids=so.case_id)
def test_spread_table_is_the_host_programs(scenes, host, case):
    """surfodom_ref.SPREAD is a measurement of the reference: measured again here on two cases"""
    name, voxel, which, nb = case
    sc, pv, R0, t0, state, P = _inputs(scenes, name, voxel, which)
    got = so.measure_spread(lambda s, c: _host(host, pv, sc["pnt"], s, c, voxel, neighbors=nb, tag="spread"), state, P)
    print(so.case_id(case), got)
    for g, w in zip(got, so.SPREAD[case]):
        assert g <= 2.0 * w + 1e-30 and (w == 0.0 or g >= 0.5 * w), (got, so.SPREAD[case])


def test_second_update_stops_after_two_iterations(scenes, host):
    """from the fine case's result (state and covariance) the next update converges at once: kept because the restatement shows both
    ratios below 1/2"""
    case = ("near", 0.5, "fine", 7)
    sc, pv, R0, t0, state, P = _inputs(scenes, *case[:3])
    a = _host(host, pv, sc["pnt"], state, P, 0.5, neighbors=7, tag="first")
    lp = so.loop(pv["map"], sc["pnt"], a["state"], a["cov"], neighbors=7)
    assert lp["iterations"] == 2 and max(lp["ratio"]) < 0.5, lp["ratio"]
    b = _host(host, pv, sc["pnt"], a["state"], a["cov"], 0.5, neighbors=7, tag="second")
    assert b["iterations"] == 2 and np.array_equal(b["match_num"], lp["match_num"]) and b["ok"] == 1
    assert np.abs(b["state"][10:13] - a["state"][10:13]).max() < 1e-5


def test_zero_matches_return_the_prediction(scenes, host):
    sc, pv, R0, t0, state, P = _inputs(scenes, "near", 0.5, "track")
    for pnt in (sc["pnt"] + 50.0, np.zeros((0, 3))):
        h = _host(host, pv, pnt, state, P, 0.5, tag="zero")
        assert h["iterations"] == 2 and h["ok"] == 0 and (h["match_num"] == 0).all() and h["eig_min"] == 0.0
        assert h["state"].tobytes() == state.tobytes() and h["cov"].tobytes() == P.tobytes() and not h["gate"].any()
    lp = so.loop(pv["map"], sc["pnt"] + 50.0, state, P)
    assert lp["iterations"] == 2 and lp["ok"] == 0


# ---------------------------------------------------------------- mutations
def test_mutations_leave_the_bar_or_change_a_decision(scenes, host):
    sc, pv, R0, t0, state, P = _inputs(scenes, "near", 0.5, "track")
    mp = pv["map"]
    pl = so.point_loop(mp, sc["pnt"], R0, t0, 3.0, 7)
    exact, bar = so.exact34(pl["ps"])
    hs = _host(host, pv, sc["pnt"], state, P, 0.5, neighbors=7, tag="mut")["sums"]

    def beyond(sums):
        return bool((np.abs(sums - exact) > bar).any() and (np.abs(sums - hs) > 2 * bar).any())

    assert not beyond(pl["sums"]) and not (np.abs(hs - exact) > bar).any()
    for what, kw in (("HTz without the sign flip", dict(flip=False)), ("columns 27..32 from 0..5", dict(w_from=0)), ("blocks swapped", dict(swap_blocks=True))):
        mut = so.point_loop(mp, sc["pnt"], R0, t0, 3.0, 7, map34=lambda w, kw=kw: so.to34(w, **kw))
        assert beyond(mut["sums"]), what
        # and the loop built on it misses the generating pose or reports another degeneracy figure
        lp = so.loop(mp, sc["pnt"], state, P, neighbors=7, map34=lambda w, kw=kw: so.to34(w, **kw))
        dt, dr = so.pose_distance(lp["state"], sc["Rg"], sc["tg"])
        assert dt > 0.005 or dr > 0.005 or not 4.0e5 < lp["eig_min"] < 5.5e5, (what, dt, dr, lp["eig_min"])
    lin = so.point_loop(mp, sc["pnt"], R0, t0, 3.0, 7, gate_squared=False)           # m < gate
    assert lin["gate"].sum() < pl["gate"].sum() and beyond(lin["sums"])
    allrec = rr.Map(pv["rec"], pv["cov"], 0.5, rr.SIGMA, rr.MIN_COUNT, ignore_min_count=True)   # min_count ignored
    extra = so.point_loop(allrec, sc["pnt"], R0, t0, 3.0, 7)
    assert not np.array_equal(extra["cell"], pl["cell"]) and beyond(extra["sums"])
    # the update launched with kd = 1: the forced rematch of iteration 2 is not counted (the stop iteration is the same expression
    # in both modes, so the decision that changes is rematch_num, which the track case shows)
    a = so.loop(mp, sc["pnt"], state, P, neighbors=7); b = so.loop(mp, sc["pnt"], state, P, neighbors=7, kd=1)
    assert (a["rematch_num"], b["rematch_num"]) == (1, 0)
    hk = _host(host, pv, sc["pnt"], state, P, 0.5, neighbors=7, kd=1, tag="kd")
    assert hk["rematch_num"] == 0 and _host(host, pv, sc["pnt"], state, P, 0.5, neighbors=7, tag="kd0")["rematch_num"] == 1


def test_host_program_under_sanitizers(scenes, tmp_path):
    """the host program alone, a stand-alone binary with -fsanitize=address,undefined: one loop with misses and one zero-match loop"""
    exe = so.build_host(tmp_path, sanitize=True)
    sc, pv, R0, t0, state, P = _inputs(scenes, "near", 0.5, "track")
    pnt = np.concatenate([sc["pnt"][:300], sc["pnt"][:40] + 50.0])
    a = so.host_run(exe, tmp_path, pv["rec"], pv["cov"], pnt, state, P, 0.5, neighbors=7, tag="san")
    assert a["iterations"] >= 3 and (a["cell"][300:] == -1).all() and a["match_num"][0] > 250
    b = so.host_run(exe, tmp_path, pv["rec"], pv["cov"], sc["pnt"][:40] + 50.0, state, P, 0.5, neighbors=7, tag="san2")
    assert b["iterations"] == 2 and b["ok"] == 0 and b["state"].tobytes() == state.tobytes()
