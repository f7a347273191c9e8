"""The corpus, conversions, references and bars of tests/big_ref.py, checked on the CPU before the any-window path of the device is held
to them (tests/test_gpu_big.py):
  * calibration: the f64 oracle (LidarFactor::acc_evaluate2, any W) stays within the Hessian bars on store(W) and origin(W), W = 9, 17,
    25: the whole store, every class as a store of its own, every voxel of the origin store alone;
  * the CSR conversions invert each other;
  * the transform reference agrees with the oracle's PointCluster::transform within its own bar, and keeps the count D_T = 9;
  * teeth at W = 17: defects k_big_syrk, k_big_slot or k_big_diag could have, applied to the oracle's own H, g, r, each exceed a bar.
The issue that asked for these tests also listed a tooth "the six diagonal entries of one cross block read from the transposed block, on
a block where the halves differ by more than the bar".  No block of the corpus qualifies: the entries in question are H(6i+k, 6j+k) and
H(6j+k, 6i+k), and the oracle stores every off-diagonal block and its mirror from one value (asserted below), so the tooth is left out
instead of weakened.  On the device k_big_blockdiag's output is pinned bit for bit to the entries of the H the same call returned."""
import numpy as np
import pytest

import big_ref as B
import hess_ref as R

WS = [9, 17, 25]
TEETH_W = 17


def _factor(oracle, st):
    f = oracle.Factor(st["W"])
    f.push(st["clusters"], st["fix"], st["coe"], st["eig_val"], st["eig_vec"], st["pcr_add"])
    return f


class Worst:
    def __init__(self, site):
        self.site, self.w, self.bad = site, {}, []

    def add(self, cls, q, what=None):
        for k, v in q.items():
            self.w[(cls, k)] = max(self.w.get((cls, k), 0.0), v)
        if R.worst(q) > 1.0:
            self.bad.append((cls, what, q))

    def done(self):
        print("\n%s worst ratio to bar: %s" % (self.site, {"%s/%s" % k: "%.3g" % v for k, v in sorted(self.w.items()) if k[1] in "Hgr"}))
        assert not self.bad, (self.site, len(self.bad), self.bad[:4])


# ------------------------------------------------------------------------------------------------ corpus and calibration
@pytest.mark.parametrize("W", [2, 3, 8, 9, 16, 17, 25, 41])
def test_store_shape(W):
    st = B.store(W)
    cls, occ = st["cls"], st["clusters"][:, :, 9] != 0.0
    V = len(cls)
    assert V % B.VC == 5 and occ.any(1).all() and not st["fix"].any() and np.all(st["coe"] == 1.0)
    assert set(cls) == set(B.CLASSES)
    assert list(cls[-5:]) == ["full"] * 5 and occ[-5:].all()
    a = V - 5 - B.VC
    assert list(cls[a:V - 5]) == ["straddle"] * B.VC and a % B.VC == 0
    pair = np.flatnonzero(occ[a])
    assert len(pair) == 2 and np.all(occ[a:V - 5] == occ[a])
    if W > B.TF:
        assert list(pair) == [B.TF - 1, B.TF]
    else:
        assert pair[-1] == W - 1
    b = a - 2 * B.VC
    assert list(cls[b:a]) == ["skip"] * 2 * B.VC and np.all(np.flatnonzero(occ[b:a].any(0)) == [0, 1]) and occ[b:a, :2].all()
    assert (occ[cls == "lonely"].sum(1) == 1).all()
    if W == 41:                                                         # the voxels hess_ref gave a random mask: bands of 2 to 4 frames
        rnd = B._random_mask_kinds(list(R.store(W)["cls"]))
        keep = (R.store(W)["clusters"][:, :, 9] != 0.0).any(1) | rnd     # the voxels of hess_ref's corpus that store(W) keeps, in order
        fr = [np.flatnonzero(o) for o in occ[:keep.sum()][rnd[keep]]]
        assert len(fr) >= 5 and all(2 <= len(f) <= 4 and f[-1] - f[0] == len(f) - 1 for f in fr)
        assert all(2 <= len(np.flatnonzero(o)) <= 4 for o in occ[cls == "pad"])


@pytest.mark.parametrize("W", WS)
def test_oracle_within_bars(oracle, W):
    st = B.store(W)
    ref = B.ref_of(st, ("store", W))
    assert (ref.dH, ref.dG, ref.dR) == (R.D_H, R.D_G, R.D_R) == (35, 15, 1)
    V = len(st["cls"])
    rep = Worst("oracle any-window W=%d" % W)
    H, g, r = _factor(oracle, st).acc_evaluate2(st["poses"])
    rep.add("all", ref.check(H, g, r, np.arange(V), sym=False))
    iu = np.triu_indices(6 * W, 6)
    assert np.array_equal(H[iu], H.T[iu])                               # every off-diagonal block and its mirror: one value (module docstring)
    for cls in B.CLASSES:
        idx = np.flatnonzero(st["cls"] == cls)
        H, g, r = _factor(oracle, B.subset(st, idx)).acc_evaluate2(st["poses"])
        rep.add(cls, ref.check(H, g, r, idx, sym=False), cls)
    rep.done()


@pytest.mark.parametrize("W", WS)
def test_oracle_within_bars_at_the_origin(oracle, W):
    st = B.origin(W)
    ref = B.ref_of(st, ("origin", W))
    V = len(st["cls"])
    f = _factor(oracle, st)
    rep = Worst("oracle any-window origin W=%d" % W)
    for a, b in [(v, v + 1) for v in range(V)] + [(0, V)]:
        rep.add(st["cls"][a] if b - a == 1 else "all", ref.check(*f.acc_evaluate2(st["poses"], a, b), np.arange(a, b), sym=False), (a, b))
    rep.done()


# ------------------------------------------------------------------------------------------------ conversions
@pytest.mark.parametrize("W", [2, 9, 41])
def test_csr_round_trip(W):
    st = B.store(W)
    vptr, efr, ecl = B.to_csr(st["clusters"])
    assert vptr[0] == 0 and vptr[-1] == len(efr) == len(ecl) == int((st["clusters"][:, :, 9] != 0).sum())
    assert all(np.all(np.diff(efr[vptr[v]:vptr[v + 1]]) > 0) for v in range(len(vptr) - 1)) and np.all(ecl[:, 9] != 0.0)
    assert np.array_equal(B.to_dense(vptr, efr, ecl, W), st["clusters"])
    v2, f2, c2 = B.to_csr(B.to_dense(vptr, efr, ecl, W))
    assert np.array_equal(v2, vptr) and np.array_equal(f2, efr) and np.array_equal(c2, ecl)


# ------------------------------------------------------------------------------------------------ transform reference
def test_transform_reference(oracle):
    """D_T = 9 by hand (big_ref's docstring): R P 3, (R P) R^T 6, (R v) p^T 4, (N p) p^T 2, the four terms summed 7, 8, 9; v' 4.  The
    oracle's PointCluster::transform (the same order of operations in f64) stays within D_T u M of the double-double value."""
    st = B.store(9)
    vptr, efr, ecl = B.to_csr(st["clusters"])
    terms, d = B.transform_ref(ecl, st["poses"][efr])
    assert d == B.D_T == 9 and max(t.k for t in terms[6:]) == 4
    worst = 0.0
    for e in range(len(efr)):
        got = oracle.cluster_transform(ecl[e], st["poses"][efr[e]])
        assert got[9] == ecl[e, 9]
        for k in range(9):
            want = R.DD(terms[k].v.hi[e:e + 1], terms[k].v.lo[e:e + 1])
            worst = max(worst, float(want.err_to(got[k:k + 1])[0]) / (B.D_T * R.U * terms[k].m[e]))
    print("\noracle transform worst ratio to D_T u M: %.3g" % worst)
    assert worst <= 1.0
    # and the per-voxel sums of the host (numpy, another order of operations) stay within (D_T + n_v) u M
    q = B.check_sums(vptr, efr, ecl, st["poses"], st["pcr_add"])
    print("host sums worst ratio to bar: %s" % q)
    assert R.worst(q) <= 1.0
    bad = st["pcr_add"].copy(); bad[3, 0] *= 1.0 + 2.0 ** -40
    assert B.check_sums(vptr, efr, ecl, st["poses"], bad)["sums"] > 1.0
    l0 = st["eig_val"][:, 0]
    assert B.check_r(float(l0.sum()), l0) <= 1.0 and B.check_r(float(l0[:-1].sum()), l0) > 1.0


# ------------------------------------------------------------------------------------------------ teeth
@pytest.fixture(scope="module")
def teeth(oracle):
    st = B.store(TEETH_W)
    ref = B.ref_of(st, ("store", TEETH_W))
    H, g, r = _factor(oracle, st).acc_evaluate2(st["poses"])
    assert R.worst(ref.check(H, g, r, np.arange(len(st["cls"])), sym=False)) <= 1.0
    return st, ref, H, g, r


def _bites(teeth, H, g, r):
    st, ref = teeth[:2]
    return R.worst(ref.check(H, g, r, np.arange(len(st["cls"])), sym=False)) > 1.0


def _range_of(st, cls):
    idx = np.flatnonzero(st["cls"] == cls)
    assert np.all(np.diff(idx) == 1)
    return int(idx[0]), int(idx[-1]) + 1


def test_tooth_frame_of_part_tile_left_out(teeth):
    """frame 16, the one frame of the third tile at W = 17 (the guard f < b.W and r, c < n6)"""
    st, ref, H, g, r = teeth
    H, g = H.copy(), g.copy()
    H[96:102, :] = 0.0; H[:, 96:102] = 0.0; g[96:102] = 0.0
    assert _bites(teeth, H, g, r)


def test_tooth_last_chunk_left_out(oracle, teeth):
    """the last, part-filled chunk of 16 voxels (the slice arithmetic c1 = min(c0 + per, nchunk), v < b.V)"""
    st = teeth[0]
    V = len(st["cls"])
    H, g, r = _factor(oracle, st).acc_evaluate2(st["poses"], 0, (V - 1) // B.VC * B.VC)
    assert _bites(teeth, H, g, r)


def test_tooth_skip_run_added_twice(oracle, teeth):
    """the two chunks the tile pairs beyond (0, 0) skip, summed by two slices"""
    st, ref, H, g, r = teeth
    a, b = _range_of(st, "skip")
    assert a % B.VC == 0 and b - a == 2 * B.VC
    H2, g2, r2 = _factor(oracle, st).acc_evaluate2(st["poses"], a, b)
    assert _bites(teeth, H + H2, g, r) and _bites(teeth, H, g + g2, r) and _bites(teeth, H, g, r + r2)


def _one_voxel(oracle, st, ref):
    """a `full` voxel: its Hessian from big_ref.slot_terms (the kernel's split) meets the bars of the voxel alone"""
    v = _range_of(st, "full")[0]
    W = st["W"]
    parts = [B.slot_terms(st, v, i) for i in range(W)]
    Gm = np.concatenate([p[0] for p in parts], axis=1)                  # [3][6W]
    Hv = Gm.T @ (parts[0][1][:, None] * Gm)
    gv = np.concatenate([p[3] for p in parts])
    for i, p in enumerate(parts):
        Hv[6 * i:6 * i + 6, 6 * i:6 * i + 6] += p[2]
    q = ref.check(Hv, gv, st["eig_val"][v, 0], [v], sym=False)
    assert R.worst(q) <= 1.0, q
    return v, parts


def test_tooth_remainder_of_one_frame_left_out(oracle, teeth):
    """E of one entry (k_big_slot's es rows 0..20, summed per frame by k_big_diag) left out of its diagonal block"""
    st, ref, H, g, r = teeth
    v, parts = _one_voxel(oracle, st, ref)
    for i in (0, 7, 16):
        H2 = H.copy()
        H2[6 * i:6 * i + 6, 6 * i:6 * i + 6] -= parts[i][2]
        assert _bites(teeth, H2, g, r), i


def test_tooth_gradient_of_one_entry_left_out(oracle, teeth):
    """es rows 21..26 of one entry left out of g"""
    st, ref, H, g, r = teeth
    v, parts = _one_voxel(oracle, st, ref)
    for i in (0, 7, 16):
        assert np.allclose(parts[i][3], ref.g_slot[v, i], rtol=1e-6, atol=1e-9 * np.abs(ref.g_slot[v]).max())
        g2 = g.copy()
        g2[6 * i:6 * i + 6] -= ref.g_slot[v, i]
        assert _bites(teeth, H, g2, r), i
