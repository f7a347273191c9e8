"""The reference and bars of tests/hess_ref.py, checked on the CPU before the device is held to them (tests/test_gpu_hess.py):
  * calibration: the f64 oracle (LidarFactor::acc_evaluate2, the same literal formula in doubles) stays within the bars on the whole
    corpus, every W in 2..16: the sub-ranges the device is run on and every voxel alone (which is where the count d binds);
  * the double-double arithmetic against mpmath at 50 digits;
  * the reference is the derivative it claims to be: central differences of sum coe * lambda_min in 60-digit arithmetic;
  * teeth: defects a wrong kernel could have, applied to the oracle's inputs or output, each exceed a bar."""
import mpmath
import numpy as np
import pytest

import hess_ref as R

WS = list(range(2, 17))


def _factor(oracle, st):
    f = oracle.Factor(st["W"])
    f.push(st["clusters"], st["fix"], st["coe"], st["eig_val"], st["eig_vec"], st["pcr_add"])
    return f


# ------------------------------------------------------------------------------------------------ calibration
@pytest.mark.parametrize("W", WS)
def test_oracle_within_bars(oracle, W):
    st = R.store(W)
    ref = R.ref_of(st, ("cpu", W))
    assert (ref.dH, ref.dG, ref.dR) == (R.D_H, R.D_G, R.D_R)         # the count of the module docstring is the count the code keeps
    V = len(st["coe"])
    assert V == 3 * R.hess2_tv(W) + 5 and set(st["cls"]) == set(R.CLASSES)
    f = _factor(oracle, st)
    w, bad = {}, []

    def add(cls, q, what):
        for k, v in q.items():
            w[(cls, k)] = max(w.get((cls, k), 0.0), v)
        if R.worst(q) > 1.0:
            bad.append((cls, what, q))

    for a, b in R.ranges(st):
        H, g, r = f.acc_evaluate2(st["poses"], a, b)
        add("range", ref.check(H, g, r, np.arange(a, b), sym=False), (a, b))
        assert np.array_equal(H[np.triu_indices(6 * W, 6)], H.T[np.triu_indices(6 * W, 6)])     # the mirror of the off-diagonal blocks
    for v in range(V):
        H, g, r = f.acc_evaluate2(st["poses"], v, v + 1)
        add(st["cls"][v], ref.check(H, g, r, [v], sym=False), v)
    print("\noracle W=%d worst ratio to bar: %s" % (W, {"%s/%s" % k: "%.3g" % v for k, v in sorted(w.items()) if k[1] != "zero"}))
    assert not bad, (W, len(bad), bad[:4])


@pytest.mark.parametrize("W", WS)
def test_oracle_within_bars_at_the_origin(oracle, W):
    """the store on which the bars are tightest (hess_ref.origin_store): every voxel alone and the whole store"""
    st = R.origin_store(W)
    ref = R.ref_of(st, ("cpu-origin", W))
    f = _factor(oracle, st)
    V = len(st["coe"])
    qs = [ref.check(*f.acc_evaluate2(st["poses"], a, b), np.arange(a, b), sym=False) for a, b in [(v, v + 1) for v in range(V)] + [(0, V)]]
    w = {}
    for cls, q in zip(list(st["cls"]) + ["all"], qs):
        for k in "Hgr":
            w[(cls, k)] = max(w.get((cls, k), 0.0), q[k])
    print("\noracle origin W=%d worst ratio to bar: %s" % (W, {"%s/%s" % k: "%.3g" % v for k, v in sorted(w.items())}))
    assert max(R.worst(q) for q in qs) <= 1.0, (W, w)


def test_lonely_and_fixonly_are_zero_in_exact_arithmetic():
    """a voxel seen by one frame only (no fixed cluster) has H = g = 0 for exact eigen-data; with the stored (f64 eigh) eigen-data the
    reference's terms cancel to a few roundings of their shadow, inside the bar around zero, so all a device may leave is residue
    within the bar; a voxel with no frame has no term at all"""
    st = R.store(5)
    ref = R.ref_of(st, ("cpu", 5))
    lone = np.flatnonzero(st["cls"] == "lonely")
    assert len(lone) >= 3
    for v in lone:
        (Hs, gs, _), _ = ref.sums([v])
        M = ref.HM[:, :, v]
        assert np.all(np.abs(Hs.f64()) <= (R.D_H + 1) * R.U * M) and M.max() > 0.0
        assert np.all(np.abs(gs.f64()) <= (R.D_G + 1) * R.U * ref.gM[:, v])
    for v in np.flatnonzero(st["cls"] == "fixonly"):
        assert not ref.HM[:, :, v].any() and not ref.gM[:, v].any() and ref.rM[v] > 0.0


def test_double_double_matches_mpmath():
    st = R.store(3)
    pick = np.concatenate([np.flatnonzero(st["cls"] == c)[:2] for c in R.CLASSES])
    sub = R.reorder(st, pick)
    dd = R.Ref(sub["clusters"], sub["coe"], sub["eig_val"], sub["eig_vec"], sub["pcr_add"], sub["poses"])
    with mpmath.workdps(50):
        mp = R.Ref(sub["clusters"], sub["coe"], sub["eig_val"], sub["eig_vec"], sub["pcr_add"], sub["poses"], T=R.MP)
        assert (mp.dH, mp.dG) == (dd.dH, dd.dG)
        assert np.allclose(mp.HM, dd.HM, rtol=1e-13, atol=0) and np.allclose(mp.gM, dd.gM, rtol=1e-13, atol=0)
        for v in range(len(pick)):
            (Hd, gd, rd), _ = dd.sums([v])
            (Hm, gm, rm), _ = mp.sums([v])
            for a, b, M in ((Hd, Hm, dd.HM[:, :, v]), (gd, gm, dd.gM[:, v]), (rd, rm, np.array([dd.rM[v]]))):
                # hi + lo against the 50-digit value: 2^-100 of the shadow (about 1e3 operations of 2^-104 each)
                err = np.array([float(abs(mpmath.mpf(float(h)) + mpmath.mpf(float(l)) - m)) for h, l, m in zip(a.hi.ravel(), a.lo.ravel(), b.a.ravel())])
                assert np.all(err <= 2.0 ** -100 * M.ravel()), (v, (err / np.maximum(M.ravel(), 1e-300)).max())


# ------------------------------------------------------------------------------------------------ finite differences
def _mp_exp(w):
    th = mpmath.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    K = mpmath.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return mpmath.eye(3)
    return mpmath.eye(3) + (mpmath.sin(th) / th) * K + ((1 - mpmath.cos(th)) / th ** 2) * (K * K)


def _mp_voxel(clusters_a, fix_a, R_, p_):
    """sums, covariance eigen-decomposition of one voxel under poses (R_, p_), all mpmath"""
    mpf = mpmath.mpf

    def unpack(c):
        return (mpmath.matrix([[mpf(float(c[0])), mpf(float(c[1])), mpf(float(c[2]))], [mpf(float(c[1])), mpf(float(c[3])), mpf(float(c[4]))],
                               [mpf(float(c[2])), mpf(float(c[4])), mpf(float(c[5]))]]),
                mpmath.matrix([mpf(float(c[6])), mpf(float(c[7])), mpf(float(c[8]))]), mpf(float(c[9])))

    P, v, N = unpack(fix_a)
    for i in range(len(R_)):
        Pi, vi, ni = unpack(clusters_a[i])
        if ni == 0:
            continue
        Rv = R_[i] * vi
        rp = Rv * p_[i].T
        P = P + R_[i] * Pi * R_[i].T + rp + rp.T + ni * (p_[i] * p_[i].T)
        v = v + Rv + ni * p_[i]
        N = N + ni
    c = v / N
    return P, v, N, P / N - c * c.T


def test_reference_is_the_second_derivative():
    """V = 3, W = 3, one voxel with a fixed cluster: gradient and Hessian of sum coe * lambda_min under R <- R Exp(dth), p <- p + dp (the
    parametrisation of tests/golden/make_golden.py) by central differences with h = 1e-15 in 60-digit arithmetic (truncation ~ h^2,
    rounding ~ 1e-60 / h^2) against the reference fed eigen-data of the same precision: 1e-12 of the shadow M per entry."""
    rng = np.random.default_rng(11)
    V, W = 3, 3
    poses = np.zeros((W, 12))
    for i in range(W):
        poses[i, :9] = R._rot(rng).ravel(); poses[i, 9:] = rng.normal(0, 1.0, 3)
    clusters = np.zeros((V, W, 10)); fix = np.zeros((V, 10))
    for a in range(V):
        n, t1, t2 = R._frame(rng)
        c0 = rng.uniform(-3, 3, 3)

        def patch(m):
            return c0 + np.outer(rng.uniform(-0.4, 0.4, m), t1) + np.outer(rng.uniform(-0.4, 0.4, m), t2) + np.outer(rng.normal(0, 0.02, m), n)
        for i in range(W):
            if (a, i) == (1, 2):
                continue                                                # one empty slot
            pert = poses[i].copy(); pert[9:] += rng.normal(0, 0.01, 3)
            pert[:9] = (pert[:9].reshape(3, 3) @ R._small_rot(rng.normal(0, 0.01, 3))).ravel()
            clusters[a, i] = R.cluster(R._body(patch(int(rng.integers(6, 30))), pert))
        if a == 0:
            fix[a] = R.cluster(patch(9))
    coe = rng.uniform(0.5, 1.5, V)
    n6 = 6 * W
    with mpmath.workdps(60):
        mpf = mpmath.mpf
        R0 = [mpmath.matrix(3, 3) for _ in range(W)]
        p0 = [mpmath.matrix([mpf(float(x)) for x in poses[i, 9:]]) for i in range(W)]
        for i in range(W):
            for k in range(9):
                R0[i][k // 3, k % 3] = mpf(float(poses[i, k]))

        def f(d):                                                       # d: dict index -> mpf step
            tot = mpf(0)
            Rn, pn = [], []
            for i in range(W):
                w = [d.get(6 * i + k, mpf(0)) for k in range(3)]
                Rn.append(R0[i] * _mp_exp(w))
                pn.append(p0[i] + mpmath.matrix([d.get(6 * i + 3 + k, mpf(0)) for k in range(3)]))
            for a in range(V):
                cov = _mp_voxel(clusters[a], fix[a], Rn, pn)[3]
                tot += mpf(float(coe[a])) * min(mpmath.eigsy(cov, eigvals_only=True))
            return tot

        h = mpf(10) ** -15
        g_fd = [(f({i: h}) - f({i: -h})) / (2 * h) for i in range(n6)]
        f0 = f({})
        H_fd = [[None] * n6 for _ in range(n6)]
        for i in range(n6):
            H_fd[i][i] = (f({i: h}) - 2 * f0 + f({i: -h})) / (h * h)
            for j in range(i + 1, n6):
                H_fd[i][j] = H_fd[j][i] = (f({i: h, j: h}) - f({i: h, j: -h}) - f({i: -h, j: h}) + f({i: -h, j: -h})) / (4 * h * h)
        # eigen-data of the same precision
        ev = [[] for _ in range(3)]; evec = [[] for _ in range(9)]; pa = [[] for _ in range(10)]
        for a in range(V):
            P, v, N, cov = _mp_voxel(clusters[a], fix[a], R0, p0)
            E, Q = mpmath.eigsy(cov)
            order = sorted(range(3), key=lambda k: E[k])
            for k in range(3):
                ev[k].append(E[order[k]])
            for r in range(3):
                for c in range(3):
                    evec[3 * r + c].append(Q[r, order[c]])
            for k, x in enumerate((P[0, 0], P[1, 0], P[2, 0], P[1, 1], P[2, 1], P[2, 2], v[0], v[1], v[2], N)):
                pa[k].append(x)
        as_mp = lambda rows: [R.MP(np.array(r, dtype=object)) for r in rows]
        ref = R.Ref(clusters, coe, as_mp(ev), as_mp(evec), as_mp(pa), poses, T=R.MP)
        (Hs, gs, rs), _ = ref.sums(np.arange(V))
        assert abs(rs.a[0] - f0) <= mpf(10) ** -40
        MH, Mg = ref.HM.sum(-1), ref.gM.sum(-1)
        worst_g = max(float(abs(g_fd[i] - gs.a[i])) / Mg[i] for i in range(n6))
        worst_H = max(float(abs(H_fd[i][j] - Hs.a[i, j])) / MH[i, j] for i in range(n6) for j in range(n6))
        # the check has teeth only if the values are not themselves below 1e-12 of the shadow
        assert max(float(abs(gs.a[i])) / Mg[i] for i in range(n6)) > 1e-4 and max(float(abs(Hs.a[i, j])) / MH[i, j] for i in range(n6) for j in range(n6)) > 1e-4
    print("\nfinite differences: worst |FD - ref| / M: g %.3g  H %.3g" % (worst_g, worst_H))
    assert worst_g <= 1e-12 and worst_H <= 1e-12


# ------------------------------------------------------------------------------------------------ teeth
TEETH_W = 5


def _bites(ref, st, H, g, r):
    """the largest ratio over the sub-ranges the device test checks"""
    return max(R.worst(ref.check(H[k], g[k], r[k], np.arange(a, b), sym=False)) for k, (a, b) in enumerate(R.ranges(st)))


def _oracle_ranges(oracle, st, ranges=None):
    f = _factor(oracle, st)
    out = [f.acc_evaluate2(st["poses"], a, b) for a, b in (ranges or R.ranges(st))]
    return [x[0] for x in out], [x[1] for x in out], [x[2] for x in out]


@pytest.fixture(scope="module")
def teeth(oracle):
    st = R.store(TEETH_W)
    ref = R.ref_of(st, ("cpu", TEETH_W))
    H, g, r = _oracle_ranges(oracle, st)
    assert _bites(ref, st, H, g, r) <= 1.0
    return st, ref, H, g, r


def _plane_voxel(st):
    """the first voxel of the second tile: a `plane` voxel, alone with an r-only voxel in the range [TV - 1, TV + 1)"""
    v = st["TV"]
    assert st["cls"][v] == "plane" and st["cls"][v - 1] == "fixonly"
    return v


def test_tooth_voxel_dropped(oracle, teeth):
    st, ref, *_ = teeth
    v = _plane_voxel(st)
    keep = np.delete(np.arange(len(st["coe"])), v)
    cut = R.reorder(st, keep)
    # the ranges of the full store, in the indices of the store without the voxel
    rg = [(a - (a > v), b - (b > v)) for a, b in R.ranges(st)]
    H, g, r = _oracle_ranges(oracle, cut, rg)
    assert _bites(ref, st, H, g, r) > 1.0


def test_tooth_frames_swapped(oracle, teeth):
    st, ref, *_ = teeth
    v = _plane_voxel(st)
    fr = np.flatnonzero(st["clusters"][v, :, 9] != 0.0)
    bad = dict(st); bad["clusters"] = st["clusters"].copy()
    bad["clusters"][v, [fr[0], fr[1]]] = st["clusters"][v, [fr[1], fr[0]]]
    assert _bites(ref, st, *_oracle_ranges(oracle, bad)) > 1.0


def test_tooth_block_transposed(teeth):
    st, ref, H, g, r = teeth
    v = _plane_voxel(st)
    fr = np.flatnonzero(st["clusters"][v, :, 9] != 0.0)
    i, j = 6 * fr[0], 6 * fr[1]
    H = [x.copy() for x in H]
    for x in H:
        blk = x[i:i + 6, j:j + 6].copy()
        x[i:i + 6, j:j + 6] = blk.T; x[j:j + 6, i:i + 6] = blk
    assert _bites(ref, st, H, g, r) > 1.0


def test_tooth_gradient_slot_dropped(teeth):
    st, ref, H, g, r = teeth
    v = _plane_voxel(st)
    i = int(np.flatnonzero(st["clusters"][v, :, 9] != 0.0)[0])
    g = [x.copy() for x in g]
    for x, (a, b) in zip(g, R.ranges(st)):
        if a <= v < b:
            x[6 * i:6 * i + 6] -= ref.g_slot[v, i]
    assert _bites(ref, st, H, g, r) > 1.0


def test_tooth_reciprocal_scaled(oracle):
    """2 / (l0 - l1) of one plane voxel times 1 + 2^-40, through the stored l1 (the difference keeps 2^-40 to 2^-52 / 2^-40).  It bites
    on the voxel alone in the store at the origin.  On the corpus (patches 1 to 100 m out, poses metres from the origin) it does NOT:
    the shadow of the literal formula, which carries world-frame second moments, is more than 2^13 / 36 = 227 times the term there, so
    2^-40 of the term is below 36 u M (DESIGN.md states this limit of a bar of the form u M)."""
    st = R.origin_store(TEETH_W)
    ref = R.ref_of(st, ("cpu-origin", TEETH_W))
    v = 0                                                               # the plane patch every frame sees
    assert st["cls"][v] == "plane"
    bad = dict(st); bad["eig_val"] = st["eig_val"].copy()
    l0, l1 = st["eig_val"][v, 0], st["eig_val"][v, 1]
    bad["eig_val"][v, 1] = l0 - (l0 - l1) / (1.0 + 2.0 ** -40)
    assert abs((l0 - l1) / (l0 - bad["eig_val"][v, 1]) - (1.0 + 2.0 ** -40)) < 2.0 ** -50
    good = ref.check(*_factor(oracle, st).acc_evaluate2(st["poses"], v, v + 1), [v], sym=False)
    q = ref.check(*_factor(oracle, bad).acc_evaluate2(st["poses"], v, v + 1), [v], sym=False)
    assert R.worst(good) <= 1.0 and q["H"] > 1.0, (good, q)


def test_tooth_hat_term_left_out(teeth):
    """- 1/2 hat(jjt) of one slot left out of its rot-rot block (coe * jjt is the slot's gradient)"""
    st, ref, H, g, r = teeth
    v = _plane_voxel(st)
    i = int(np.flatnonzero(st["clusters"][v, :, 9] != 0.0)[0])
    j = ref.g_slot[v, i, :3]
    hatj = np.array([[0, -j[2], j[1]], [j[2], 0, -j[0]], [-j[1], j[0], 0]])
    H = [x.copy() for x in H]
    for x, (a, b) in zip(H, R.ranges(st)):
        if a <= v < b:
            x[6 * i:6 * i + 3, 6 * i:6 * i + 3] += 0.5 * hatj
    assert _bites(ref, st, H, g, r) > 1.0
