"""CPU companion of the pose-graph passes (tests/pgo_ref.py): the g++ build of csrc/vba_pgo_math.hpp under the production plan
(tests/host/pgo_host.cpp, -ffp-contract=off) against the double-double reference and its counted per-entry bars.  This is the calibration
of the bars; the device meets the same bars in tests/test_gpu_pgo_passes.py.
  * the counts the code keeps equal the pinned constants, the Taylor truncations equal TRUNC, every branch variable keeps its margin;
  * every slot of the F = 300 corpus within its bars, M = 0 entries exactly 0 (worst ratio per class printed);
  * the reference agrees with tests/pgo_oracle.py to 1e-12 where the latter is well conditioned;
  * cost and assembly replays equal the g++ build bit for bit; sub-calls of 1, 255, 256, 257 factors give the corpus call's bits;
  * solve calibration: the header's elimination plus a plain dense LDL^T inside solve_ref's bars on every graph;
  * the retraction within its counted bars in the closed-form branch;
  * teeth: every defect exceeds a bar."""
import numpy as np
import pytest

import pgo_oracle as po
import pgo_ref as R

CHART_TEETH = ("E_1.01", "F_sign", "D_1mc", "taylor_at_2", "Ad_T", "Ji_plus", "lam_col")
ELIM_TEETH = ("dup_skip", "sign_all", "sba_T", "bA_drop", "xa_xn")


@pytest.fixture(scope="module")
def lin():
    inp, ref = R.lin_ref()
    return inp, ref, R.host_step(*inp)


@pytest.fixture(scope="module")
def graphs():
    return {name: (g, R.host_step(*g, extra=True)) for name, g in R.solve_graphs().items()}


def test_counts_and_truncations_are_the_pinned_ones(lin):
    _, ref, _ = lin
    assert R.taylor_truncation() == R.TRUNC
    assert ref.counts() == R.COUNTS


def test_corpus_covers_every_class_and_keeps_its_margins(lin):
    inp, ref, _ = lin
    poses, edges, priors = inp
    assert ref.F == R.F_LIN == 300 and len(poses) + len({(min(a, b), max(a, b)) for a, b in edges[:, :2]}) > 256
    assert ref.margins() == [] and ref.branch_consistent() == []
    assert {R.lin_classes(f) for f in range(200)} == {R.lin_classes(f) for f in range(200, 300)} == \
        {(a, t) for a in range(len(R.ANGLES)) for t in range(len(R.TRANS))}
    assert set(ref.sigs) == {(b, s, t) for b in (True, False) for s, t in ((True, True), (False, True), (False, False))}
    assert (edges[:, 0] > edges[:, 1]).any() and (edges[:, 0] < edges[:, 1]).any()
    par = [tuple(edges[2 * g:2 * g + 2, 0]) for g in range(100)]
    assert any(a == b for a, b in par) and any(a != b for a, b in par)           # parallel edges of the same and of opposite orientation
    assert np.abs(poses[:, 9:]).max() > 500
    # the angle pgo_coeffs receives sits where the class says (the exactly-zero class: phi == 0 in every bit)
    for f, name, kind, x, bar, thr in ref.branch:
        if name.endswith("pgo_coeffs phi"):
            want = R.ANGLES[R.lin_classes(f)[0]]
            assert (x == 0.0) if want == 0.0 else abs(x / want - 1) < 1e-5, (f, x, want)
    for f in range(300):                                                        # residual translation exactly 0: v = 0, M(v) = 0 or exact data
        if R.lin_classes(f) == (0, 0):
            assert np.all(ref.e[f] == 0.0)


def test_every_slot_within_its_bars(lin):
    """calibration: the g++ build of the shared header, per entry"""
    _, ref, h = lin
    ratio, bad = ref.check(h["slot"])
    for a in range(len(R.ANGLES)):
        print("angle %-12.6g worst err / bar %.3g" % (R.ANGLES[a], max(ratio[f] for f in range(300) if R.lin_classes(f)[0] == a)))
    for t in range(len(R.TRANS)):
        print("translation %-6g worst err / bar %.3g" % (R.TRANS[t], max(ratio[f] for f in range(300) if R.lin_classes(f)[1] == t)))
    assert bad == []
    # M = 0 is met: the j side of every prior, and the rotation-translation block of Jr^-1 behind Hjj of a between factor is NOT zero in H
    assert np.all(ref.m[200:, 36:108] == 0.0) and np.all(ref.m[200:, 114:120] == 0.0)
    assert np.all(ref.Jjm[:200, :3, 3:] == 0.0) and np.all(ref.Jjk[:200, :3, 3:] == 0)


def test_jrinv_zero_blocks(lin):
    """the upper-right 3x3 of every Jr^-1 is exactly 0, and the lower-left one when v is exactly 0 with M = 0"""
    inp, ref, _ = lin
    rng = np.random.default_rng(3)
    for a in R.ANGLES:
        w = R._unit(rng) * a
        J = R.host_chart("jrinv", np.concatenate([w, rng.normal(size=3)])).reshape(6, 6)
        assert np.all(J[:3, 3:] == 0.0)
        J = R.host_chart("jrinv", np.concatenate([w, np.zeros(3)])).reshape(6, 6)
        assert np.all(J[3:, :3] == 0.0) and np.all(J[:3, 3:] == 0.0)
    vz = [f for f in range(300) if np.all(ref.Jjm[f, 3:, :3] == 0.0) and ref.fj[f] >= 0]
    assert len(vz) >= 10                                                        # corpus factors whose v carries M = 0


def test_reference_agrees_with_the_oracle_where_that_is_well_conditioned(lin):
    inp, ref, _ = lin
    poses, edges, priors = inp
    worst = 0.0
    for f in range(300):
        if R.ANGLES[R.lin_classes(f)[0]] not in (1e-3, 0.05, 0.5, 1.0, 2.0):
            continue
        if ref.fj[f] >= 0:
            e, Ji, Jj = po.between_jacobians(poses[ref.fi[f]], poses[ref.fj[f]], edges[f, 2:14])
        else:
            e, Ji = po.prior_jacobian(poses[ref.fi[f]], priors[f - 200, 1:13]); Jj = np.zeros((6, 6))
        for got, want in ((ref.e[f], e), (ref.Jj[f], Jj), (ref.Ji[f], Ji)):
            worst = max(worst, np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    print("reference against pgo_oracle: %.3g" % worst)
    assert worst <= 1e-12


def test_cost_and_assembly_replays_and_subcalls(lin):
    inp, ref, h = lin
    assert R.replay_cost(h["slot"]) == h["cost"]
    pairs, blk, g = R.replay_assemble(h["slot"], ref.fi, ref.fj, 200)
    assert np.array_equal(pairs, h["pairs"]) and np.array_equal(blk, h["blk"]) and np.array_equal(g, h["g"])
    assert len(blk) == 300
    for F in (1, 255, 256, 257):
        p, e, q, idx = R.lin_subcall(inp, F)
        assert len(idx) == F and np.array_equal(R.host_step(p, e, q)["slot"], h["slot"][idx])


def test_solve_calibration(graphs):
    """a plain f64 run of the shared header's elimination plus a dense LDL^T inside solve_ref's bars on every graph"""
    want = dict(chain2=(1, 1, 1), seg7=(2, 1, 7), cycle3=(1, 1, 3), skel11=(11, 0, 0), skel12=(12, 0, 0), hub65=(1, 65, 65))
    for name, ((Y, ed, pr), h) in graphs.items():
        n = len(Y)
        bw, fw, zeros = R.solve_ratios(h["blk"], h["g"], h["pairs"], n, h["dx"])
        mw = R.solve_ratios(h["blk"], h["g"], h["pairs"], n, R.model_solve(h["blk"], h["g"], h["plan"], n))
        d = h["plan"]["dims"]
        print("%-12s K %3d NP %3d S %3d: g++ backward %.3g forward %.3g; numpy model %.3g %.3g" % (name, d[0], d[1], d[3], bw, fw, mw[0], mw[1]))
        assert bw <= 1 and fw <= 1 and zeros and mw[0] <= 1 and mw[1] <= 1
        if name in want:
            assert (d[0], d[3], d[4]) == want[name]
    assert graphs["skel11"][1]["plan"]["dims"][1] == 72 and graphs["skel12"][1]["plan"]["dims"][1] == 72     # 66 padded to the panel, 72 whole
    assert graphs["skel11"][1]["plan"]["dims"][2] == 128                                                        # across the 64-row tile
    att = graphs["seg7"][1]["plan"]["seg_att"]
    assert att[0] >= 0 and att[1] >= 0 and att[0] != att[1]
    att = graphs["cycle3"][1]["plan"]["seg_att"]
    assert att[0] == att[1] >= 0
    assert (graphs["tail_branch"][1]["plan"]["seg_att"][0::2] < 0).sum() >= 2     # one-sided segments


def test_retraction_within_counted_bars():
    for a, (X, ed, pr) in zip(R.RETRACT_ANGLES, R.retract_graphs()):
        h = R.host_step(X, ed, pr)
        v, bar, k, taylor = R.retract_ref(X[0], h["dx"][0])
        assert not taylor and k == R.K_RETRACT
        ratio = (v.err_to(h["poses"][0]) / bar).max()
        print("prior %.1f rad away: |dx_w| %.3f, worst err / bar %.3g" % (a, np.linalg.norm(h["dx"][0, :3]), ratio))
        assert ratio <= 1


@pytest.mark.parametrize("tooth", CHART_TEETH)
def test_chart_and_linearisation_teeth(lin, tooth):
    inp, ref, _ = lin
    poses, edges, priors = inp
    lam = 1.0 / np.concatenate([edges[:, 14:20], priors[:, 13:19]])
    Z = np.concatenate([edges[:, 2:14], priors[:, 1:13]])
    model = lambda t: np.array([R.model_slot(poses[ref.fi[f]], poses[ref.fj[f]] if ref.fj[f] >= 0 else None, Z[f], lam[f], t) for f in range(300)])
    if tooth == CHART_TEETH[0]:
        assert ref.check(model(None))[1] == []                                  # the model itself is inside every bar
    ratio, bad = ref.check(model(tooth))
    print("%s: worst err / bar %.3g, %d factors over a bar" % (tooth, ratio.max(), (ratio > 1).sum()))
    assert ratio.max() > 1
    if tooth in ("E_1.01", "F_sign", "D_1mc"):                                  # they change the closed-form branch only
        assert all(not ref.sigs[f][2] for f in np.flatnonzero(ratio > 1))


def test_assembly_tooth(lin):
    _, ref, h = lin
    _, blk, _ = R.replay_assemble(h["slot"], ref.fi, ref.fj, 200, tooth="part3")
    assert not np.array_equal(blk, h["blk"])


@pytest.mark.parametrize("tooth", ELIM_TEETH)
def test_elimination_teeth(graphs, tooth):
    (Y, ed, pr), h = graphs["seg7"]
    n = len(Y)
    bw, fw, _ = R.solve_ratios(h["blk"], h["g"], h["pairs"], n, R.model_solve(h["blk"], h["g"], h["plan"], n, tooth))
    print("%s: backward ratio %.3g forward ratio %.3g" % (tooth, bw, fw))
    assert bw > 1 and fw > 1


def test_host_step_validates_like_the_library():
    inp, _ = R.lin_ref()
    poses, edges, priors = inp
    with pytest.raises(RuntimeError, match="2"):
        R.host_step(poses, edges, priors[:50])                                   # a component without a prior
    bad = edges.copy(); bad[0, 1] = bad[0, 0]
    with pytest.raises(RuntimeError, match="1"):
        R.host_step(poses, bad, priors)
