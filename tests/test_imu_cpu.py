"""CPU companion of the IMU factor pass (tests/imu_ref.py): the g++ build of csrc/vba_hostmath.hpp (tests/host/imu_host.cpp,
-ffp-contract=off) against the double-double reference and its per-entry bars, on the whole corpus (W = 2..16, both gravity modes, six
classes).  This is the calibration of the bars; the device meets the same bars in tests/test_gpu_imu.py.
  * the counts the code keeps equal the pinned constants; every branch variable of the reference keeps its margin to its threshold;
  * per factor: rr, joc, jtj, gg and r^T cov^-1 r within the bars (worst ratio per class printed);
  * a host model of the kernel's window assembly (imu_ref.model_assemble: block pairs, passes, border, corner, gradient, compact image
    read through li_hb_get) within the assembled bars, entries outside the pattern exactly 0;
  * the double-double path against mpmath throughout on a W = 3 window;
  * teeth: every defect listed in TEETH exceeds a bar on the class named there.  Exchanging u1 and u2 of the gravity border is the
    weakest of them: u1[R][k] = sum_f jtj_f(R, g_k) and u2[k][R] = sum_f jtj_f(g_k, R) are the two halves of a matrix that is symmetric
    up to the asymmetry of the bits of cov^-1 (inverse_pplu of an ill-conditioned cov: well above u), so the exchange is a
    transposition and shows only where that asymmetry exceeds the bars: on `smallangle`, whose exactly representable rotations leave
    few terms in M.  On the other classes it stays within the bars (measured 0.2 .. 0.5), which no bar of the form u M can change.
    The defect of that family that bites everywhere is a wrong index map: u2 written in u1's [15W][3] order (u2_in_u1_layout).
Nothing here needs a GPU."""
import mpmath
import numpy as np
import pytest

import imu_ref as I


@pytest.fixture(scope="module")
def corpus():
    return I.corpus_ref()


def _facs(ref, i, gravity):
    st, im, ci = ref.windows[i]
    return [I.host_factor(im[f], st[f], st[f + 1], ci[f], gravity) for f in range(len(im))]


def test_counts_are_the_pinned_constants(corpus):
    ref, _ = corpus
    assert ref.counts() == dict(D_RR=I.D_RR, D_JOC=I.D_JOC, D_CJ=I.D_CJ, D_HF=I.D_HF, D_GF=I.D_GF, D_QF=I.D_QF)


def test_branch_variables_keep_their_margin(corpus):
    """every branch variable of the reference a factor 1 +- 1e-3 (sign tests: 1e-3 absolute) from its threshold, no case left out; and
    the branches taken are those the reference's own values select"""
    ref, ix = corpus
    assert ref.margins() == []
    assert ref.branch_consistent() == []
    logs = {s[1] for s in ref.sigs}; quats = {s[3] for s in ref.sigs}; modes = {s[5] for s in ref.sigs}
    assert logs >= {"one", "gen"} and quats == {"pos", "0", "1", "2"} and modes == {"n0", "small", "gen"}      # every branch is met
    assert {s[0] for s in ref.sigs} == {True, False} and any(s[4] for s in ref.sigs)


def test_factors_within_bars(corpus):
    """calibration: the g++ build of the header, per factor"""
    ref, ix = corpus
    worst, bad = {}, []
    for (cls, W), i in ix.items():
        for gravity in (0, 1):
            for f, h in enumerate(_facs(ref, i, gravity)):
                fr = ref.factor(ref.off[i] + f, gravity)
                for k in ("rr", "joc", "jtj", "gg", "q"):
                    r = I.ratio(fr[k], h[k])
                    worst[(cls, k)] = max(worst.get((cls, k), 0.0), r)
                    if not r <= 1.0:
                        bad.append((cls, W, gravity, f, k, r))
    print("\nhost factor, worst ratio to bar:", {"%s/%s" % k: "%.3g" % v for k, v in sorted(worst.items())})
    assert not bad, bad[:8]


def test_identity_residual_is_exact(corpus):
    """a residual rotation that is the identity in every bit: rr[0:3] has shadow 0 in the reference and comes back exactly 0"""
    ref, ix = corpus
    seen = 0
    for (cls, W), i in ix.items():
        if cls != "smallangle":
            continue
        for f in range(W - 1):
            if ref.sigs[ref.off[i] + f][5] != "n0":
                continue
            seen += 1
            st, im, ci = ref.windows[i]
            assert not ref.rr.m[:3, ref.off[i] + f].any()
            assert not I.host_factor(im[f], st[f], st[f + 1], ci[f], 1)["rr"][:3].any()
    assert seen >= 3


def test_half_branch_reproduces_the_projects_approximation(corpus):
    """at 5e-4 rad so3_log takes f = 1/2: the reference follows it and so differs from the ideal log map by theta^2 / 6"""
    ref, ix = corpus
    seen = 0
    for (cls, W), i in ix.items():
        if cls != "smallangle":
            continue
        st, im, ci = ref.windows[i]
        for f in range(W - 1):
            m, _ = I.np_res_r(im[f], st[f], st[f + 1])
            K = np.array([m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
            th = np.arcsin(0.5 * np.linalg.norm(K))                         # the ideal angle (the antisymmetric part is sin theta * axis)
            if not 4e-4 < th < 6e-4:
                continue
            seen += 1
            w = ref.rr.v.f64()[:3, ref.off[i] + f]
            assert np.allclose(w, 0.5 * K, rtol=0, atol=1e-15)              # f = 1/2, not theta / (2 sin theta)
            rel = 1.0 - np.linalg.norm(w) / th
            assert abs(rel - th * th / 6) < 0.01 * th * th / 6, (rel, th * th / 6)
    assert seen >= 3


@pytest.mark.parametrize("gravity", [0, 1])
def test_window_model_within_bars(corpus, gravity):
    ref, ix = corpus
    worst, bad = {}, []
    for (cls, W), i in ix.items():
        H, g, rimu = I.model_assemble(W, gravity, _facs(ref, i, gravity))
        Ht, gt, rt = ref.window(i, gravity)
        assert not H[~I.pattern_mask(W, gravity)].any()
        q = I.check(Ht, gt, rt, H, g, rimu)
        for k, v in q.items():
            worst[(cls, k)] = max(worst.get((cls, k), 0.0), v)
        if not max(q.values()) <= 1.0:
            bad.append((cls, W, q))
    print("\nhost window model gravity=%d, worst ratio to bar:" % gravity, {"%s/%s" % k: "%.3g" % v for k, v in sorted(worst.items())})
    assert not bad, bad[:8]


def test_double_double_against_mpmath():
    """the double-double path against mpmath throughout (200 bits), one W = 3 window with every function live"""
    win = [I.window("offset", 3)]
    a = I.Ref(win)
    with mpmath.workprec(200):
        b = I.Ref(win, T=I.MP)
        for name in ("rr", "joc", "cj", "jtj", "gg", "q"):
            x, y = getattr(a, name), getattr(b, name)
            assert np.array_equal(x.k, y.k) and np.array_equal(x.z, y.z)
            d = np.array([float(abs(mpmath.mpf(float(h)) + mpmath.mpf(float(l)) - t))
                          for h, l, t in zip(x.v.hi.ravel(), x.v.lo.ravel(), y.v.a.ravel())]).reshape(x.m.shape)
            live = ~x.z
            assert np.all(d[live] <= 2.0 ** -90 * x.m[live]), (name, float((d[live] / x.m[live]).max()))
            assert np.allclose(x.m, y.m, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ teeth
def _alter(ref, i, gravity, what):
    """per-factor results of window i with one formula of imu_residual_jacobian altered (numpy f64 from the host's own joc / rr)"""
    st, im, ci = ref.windows[i]
    out = []
    for f in range(len(im)):
        h = I.host_factor(im[f], st[f], st[f + 1], ci[f], gravity)
        J = h["joc"].copy()
        res_r, rb = I.np_res_r(im[f], st[f], st[f + 1])
        R1, R2 = st[f, 1:10].reshape(3, 3), st[f + 1, 1:10].reshape(3, 3)
        Rbg = im[f, I.O_RBG:I.O_RBG + 9].reshape(3, 3)
        if what == "jr_inv_is_identity":
            JRi_host = J[0:3, 15:18].copy()
            J[0:3, 0:3] = -(R2.T @ R1); J[0:3, 15:18] = np.eye(3)
            J[0:3, 9:12] = np.linalg.solve(JRi_host, J[0:3, 9:12])          # JRi (res_r^T jr R_bg) with JRi taken out
        elif what == "jr_is_identity":
            J[0:3, 9:12] = -(J[0:3, 15:18] @ res_r.T @ Rbg)
        elif what == "dt_sign":
            J[3:6, 6:9] = -J[3:6, 6:9]
        out.append(I.np_factor(J, h["rr"], ci[f]))
    return out


TEETH = [                                       # (defect, classes it must bite on, quantity that must exceed its bar)
    ("drop_second_factor", ("consistent",), "H"),
    ("swap_offdiag", ("consistent",), "H"),
    ("swap_u1_u2", ("smallangle",), "H"),
    ("u2_in_u1_layout", ("offset",), "H"),
    ("corner_misses_last", ("consistent",), "H"),
    ("jr_inv_is_identity", ("bigangle", "offset"), "H"),
    ("jr_is_identity", ("offset",), "H"),
    ("dt_sign", ("consistent",), "H"),
    ("drop_gradient", ("consistent",), "g"),
]


@pytest.mark.parametrize("tooth,classes,qty", TEETH)
def test_teeth(corpus, tooth, classes, qty):
    ref, ix = corpus
    for cls in classes:
        for W in (3, 10):
            i = ix[(cls, W)]
            Ht, gt, rt = ref.window(i, 1)
            if tooth in ("jr_inv_is_identity", "jr_is_identity", "dt_sign"):
                H, g, rimu = I.model_assemble(W, 1, _alter(ref, i, 1, tooth))
            else:
                H, g, rimu = I.model_assemble(W, 1, _facs(ref, i, 1), tooth=tooth)
            q = I.check(Ht, gt, rt, H, g, rimu)
            assert q[qty] > 1.0, (tooth, cls, W, q)


def test_numpy_jtj_of_the_unaltered_jacobian_is_within_bars(corpus):
    """the control of the altered-formula teeth: the same numpy path with nothing altered stays within the bars"""
    ref, ix = corpus
    for cls in ("offset", "bigangle"):
        i = ix[(cls, 3)]
        H, g, rimu = I.model_assemble(3, 1, _alter(ref, i, 1, None))
        assert max(I.check(*ref.window(i, 1), H, g, rimu).values()) <= 1.0


def test_padded_k_slice_tooth(corpus):
    """the 16 x 16 x 4 tile loop as numpy: with the 16th k padded with zeros every block is within the factor's bars (lane 15's
    neighbour reads reach row / column 15 only); one non-zero entry in the padded slice of either operand exceeds them"""
    ref, ix = corpus
    i = ix[("offset", 3)]
    st, im, ci = ref.windows[i]
    F, nb = 2, 33
    facs = _facs(ref, i, 1)
    joc = np.concatenate([h["joc"].ravel() for h in facs] + [np.full(64, 7.0)])         # (slack: what lies behind is not zero)
    cj = np.concatenate([(ci[f] @ facs[f]["joc"]).ravel() for f in range(F)] + [np.full(64, 7.0)])
    for f in range(F):
        for ro, co in ((0, 0), (0, 15), (15, 0), (15, 15)):
            blk = ref.jtj[ro:ro + 15, co:co + 15, ref.off[i] + f]
            assert I.ratio(blk, I.tile_block(joc, cj, f, nb, ro, co)) <= 1.0
            assert I.ratio(blk, I.tile_block(joc, cj, f, nb, ro, co, poison=(3, 5))) > 1.0
