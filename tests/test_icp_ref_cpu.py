"""The reference of tests/icp_ref.py against the g++ build of the arithmetic the ICP kernels compile (csrc/vba_icp_math.hpp through
tests/host/icp_host.cpp): the counted roundings, the calibration of every bar on the whole corpus, the teeth, and the oracle's own
1-NN on the tie corpus.  No GPU."""
import numpy as np
import pytest

import btc_oracle as bo
import icp_ref as ir


def _run_host(case, slices):
    return ir.host_pass(case["src"], case["tar"], ir.start_state(case), slices or ir.own_slices(len(case["src"]), len(case["tar"])))


def test_counted_roundings_are_what_the_code_keeps():
    """the constants of the module docstring against the counts carried along the reference's order at a general pose"""
    Rt, tt, R, t, pa, ic = ir.scene_poses()["first_set"]
    src, tar = ir.scene_pair(65, 65, Rt, tt)
    c = ir.PassRef(R, t, pa, src, tar).counts
    assert (c["pi"], c["ni"], c["dv"], c["rr"], c["ninc"], c["nadd"], c["p2p"], c["jac"]) == (
        ir.K_PI, ir.K_NI, ir.K_DV, ir.K_RR, ir.K_NORMAL2, ir.K_NORMAL2, ir.K_P2P2, ir.K_JAC)
    assert np.array_equal(np.array(c["terms"], dtype=np.float64), ir.d_vector())
    # at the identity pose nothing of the transform rounds: the counts only shrink
    c0 = ir.PassRef(np.eye(3), np.zeros(3), pa, src, tar).counts
    assert c0["pi"] == 0 and c0["ni"] == 0 and all(a <= b for a, b in zip(c0["terms"], c["terms"]))


@pytest.mark.parametrize("cls", ir.CLASSES)
def test_host_build_calibrates_inside_every_bar(cls):
    """the g++ build of the shared header: every key, every clear decision, every bar, on the whole class; the worst ratios are printed"""
    worst = {}; unclear = 0; points = 0
    for case in ir.cases(cls):
        ref = ir.ref_of(case)
        for sl in case["slices"]:
            out = _run_host(case, sl)
            if case["done"]:
                assert out["rc"] == 1 and np.isnan(out["sums"]).all()
                continue
            f, g, ok = ir.check_case(case, out, sl)
            assert ok, (case["name"], sl, f, g)
            for k, v in ir.worst_ratios(f, g).items():
                worst[k] = max(worst.get(k, 0.0), v)
        unclear += int(ref.unclear.sum()); points += ref.ns
    print("ICP-CAL %s worst %s unclear %d of %d" % (cls, {k: round(v, 4) for k, v in worst.items()}, unclear, points))
    if cls != "threshold":
        assert unclear <= ir.UNCLEAR_CAP * max(points, 1)


def test_slice_plans_agree_bit_for_bit():
    case = ir.cases("slices")[0]
    outs = [_run_host(case, sl) for sl in case["slices"]]
    for o in outs[1:]:
        for k in ("key", "gate", "partial", "sums"):
            assert np.array_equal(o[k], outs[0][k]), k
    assert ir.own_slices(17000, 2200) == 8 and ir.own_slices(200, 2200) == 9 and ir.own_slices(200, 24000) == 94


def _bites(tooth):
    """the classes on which the restatement with this defect misses a bar, flips a clear decision, changes a key or a state"""
    hit = []
    for cls in ir.CLASSES:
        for case in ir.cases(cls):
            if case["done"] or len(case["src"]) > 1000:
                continue
            for sl in case["slices"]:
                sl = sl or ir.own_slices(len(case["src"]), len(case["tar"]))
                s0 = dict(R=case["R"], t=case["t"], paras=case["paras"], is_conv=case["is_conv"], done=0, iters=case["iters"])
                out = ir.restate_pass(s0, case["src"], case["tar"], sl, tooth)
                f, g, ok = ir.check_case(case, out, sl)
                if not ok:
                    hit.append(case["name"])
                    break
            if hit and hit[-1] == case["name"] and tooth is not None:
                return hit
    return hit


def test_restatement_without_a_defect_passes():
    assert _bites(None) == []


@pytest.mark.parametrize("tooth", ir.TEETH)
def test_tooth_bites(tooth):
    hit = _bites(tooth)
    print("ICP-TOOTH %s bites on %s" % (tooth, hit[:1]))
    assert hit, tooth


def test_state_table_of_the_host_build():
    """btc_icp_transition against the table of loop_refine.hpp:69, 121-130 on steps on both sides of 1e-3"""
    import ctypes as C
    lib = ir.host_lib()
    for rot in (0.0, 0.9e-3, 1.1e-3):
        for tra in (0.0, 0.9e-3, 1.1e-3):
            for ic in (0, 1):
                for it in (0, 18, 19):
                    dx = np.array([rot, 0, 0, 0, tra, 0], dtype=np.float64)
                    pa = np.array(ir.PARAS1, dtype=np.float64); a = C.c_int(ic); d = C.c_int(0); n = C.c_int(it)
                    lib.icp_host_transition(dx.ctypes.data_as(C.c_void_p), pa.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(d), C.byref(n))
                    want = ir.transition(dx, ir.PARAS1, ic, 0, it)
                    assert (tuple(pa), a.value, d.value, n.value) == want


def test_no_match_system_is_the_host_twins():
    """H = 0, g = 0: the step is what ldlt_solve_inplace returns (zeros), the pose stays, the pass counts as a small step"""
    case = [c for c in ir.cases("degenerate") if c["name"].endswith("gated_out")][0]
    out = _run_host(case, 1)
    assert not out["sums"].any() and not out["partial"].any() and not out["gate"].any()
    assert np.array_equal(out["dx"], ir.host_ldlt_inplace(np.zeros((6, 6)), np.zeros(6)), equal_nan=True)
    assert np.array_equal(out["dx"], np.zeros(6)) and out["state"]["is_conv"] == 1 and out["state"]["done"] == 0
    assert np.array_equal(out["state"]["R"], case["R"]) and np.array_equal(out["state"]["t"], case["t"])


def test_oracle_nn_answers_the_tie_corpus():
    """btc_oracle._nn_tree (kd-tree candidates, float minimum among them) against the brute-force contract, where nine or more points
    tie; and unchanged on the scenes it already served"""
    from scipy.spatial import cKDTree
    for case in ir.cases("ties") + ir.cases("scene")[-5:]:
        if not len(case["tar"]) or not len(case["src"]):
            continue
        q = ir.query(case["R"], case["t"], case["src"])
        tree = cKDTree(case["tar"][:, 0:3].astype(np.float64))
        idx = bo._nn_tree(tree, q, case["tar"][:, 0:3])
        assert np.array_equal(np.asarray(idx, np.int64), ir.key_index(ir.nn_keys(case["R"], case["t"], case["src"], case["tar"]))), case["name"]


def test_far_ties_are_made_by_the_float_cast():
    """ties_far does what it is built for: at 1000 m the float query ties lattice neighbours that the double query tells apart, so
    the nearest point in double precision is not the contract's answer for some queries"""
    case = [c for c in ir.cases("ties") if c["name"] == "ties_far"][0]
    p = case["src"][:, 0:3].astype(np.float64)
    qd = p @ case["R"].T + case["t"]                                # the query before its cast
    c = case["tar"][:, 0:3].astype(np.float64)
    dd = ((qd[:, None, :] - c[None]) ** 2).sum(axis=2)
    want = ir.key_index(ir.nn_keys(case["R"], case["t"], case["src"], case["tar"]))
    differ = dd.argmin(axis=1) != want
    assert differ.sum() >= 40, int(differ.sum())
    assert np.all(dd[np.arange(len(p)), want][differ] > dd.min(axis=1)[differ])       # farther in double, yet the contract's answer
