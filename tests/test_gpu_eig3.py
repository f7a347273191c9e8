"""Device eigen-solver of the plane fit (eig3_sym_dev: the direct path of csrc/vba_eig3.hpp with the Jacobi fallback) against the
50-digit reference of tests/eig3_ref.py, through the C ABI at three of its sites:
  * K4, both forms (k_residual_s, and k_residual_v via residual_vpl_from = 1): the corpus pushed as voxels whose cluster sums give
    cov = A exactly (P = A, v = 0, N = 1), once as the fixed cluster and once in frame 0 under an identity pose;
  * the map's leaf fit (k_recut_leaf) and its refit in margi, on designed clouds (grid and disc patches, arcs, poles, blobs, tilted
    planes) 10-100 m from the origin;
  * the GBA build (k_gba_decide) on the same clouds split over the keyframes.
Two further sites, those of the any-window path, are covered in tests/test_gpu_big.py with the same corpus, clouds and bars: the residual
pass k_big_residual (test_eig3_corpus_through_the_residual_pass, and the eigen-data of every test_residual_pass case) and the hashed
build's k_gbab_decide (test_eig3_designed_clouds_through_the_build).
Where the device forms cov from sums in f64 the bars are scaled by the cancellation scale m2 = max|P/N| instead of |A|_2."""
import numpy as np
import pytest

import eig3_ref as R

pytestmark = pytest.mark.gpu

IDENT = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


@pytest.fixture(scope="module")
def corpus():
    items = R.corpus()
    return items, R.refs(items)


class Worst:
    """largest ratio to its bar per (class, bar), and the failures"""

    def __init__(self, site):
        self.site, self.w, self.bad = site, {}, []

    def add(self, cls, q, what=None):
        for k, v in q.items():
            self.w[(cls, k)] = max(self.w.get((cls, k), 0.0), v)
        if R.worst(q) > 1.0:
            self.bad.append((cls, what, q))

    def done(self):
        print("\n%s worst ratio to bar: %s" % (self.site, {"%s/%s" % k: "%.3g" % v for k, v in sorted(self.w.items())}))
        assert not self.bad, (self.site, len(self.bad), self.bad[:4])


# ------------------------------------------------------------------------------------------------ K4
@pytest.mark.parametrize("W", [2, 10, 16])
@pytest.mark.parametrize("vpl", [0, 1])
def test_k4_corpus(capi, corpus, W, vpl):
    items, refs = corpus
    A6 = np.array([R.tri(A) for _, A in items])
    V = len(A6)
    coe = np.random.default_rng(W).uniform(0.5, 2.0, V)
    z3 = np.zeros((V, 3)); z9 = np.tile(np.eye(3).ravel(), (V, 1)); z10 = np.zeros((V, 10)); z10[:, 9] = 1
    poses = np.tile(IDENT, (W, 1))
    o = capi.default_options()
    o.win_size = W
    o.max_voxels = max(int(o.max_voxels), V)
    if vpl:
        o.residual_vpl_from = 1                  # k_residual_v for every store of more than one voxel
    ctx = capi.Context(o)
    rep = Worst("K4-%s W=%d" % ("v" if vpl else "s", W))
    with_ref = {}
    try:
        for in_frame in (False, True):
            cl = np.zeros((V, W, 10)); fix = np.zeros((V, 10))
            if in_frame:
                cl[:, 0, :6] = A6; cl[:, 0, 9] = 1.0
            else:
                fix[:, :6] = A6; fix[:, 9] = 1.0
            ctx.clear()
            ctx.push_voxels(cl, fix, coe, z3, z9, z10)
            r = ctx.evaluate_only_residual(poses)
            ev, evec, pa = ctx.read_back()
            # the kernel saw A: pcr_add is what was pushed, bit for bit
            assert np.array_equal(pa[:, :6], A6) and np.all(pa[:, 6:9] == 0.0) and np.all(pa[:, 9] == 1.0)
            for (cls, _), ref, w, U in zip(items, refs, ev, evec):
                key = (id(ref), w.tobytes(), U.tobytes())
                if key not in with_ref:                # identical results are checked once
                    with_ref[key] = R.check(ref, w, U)
                rep.add(cls, with_ref[key], ref.w.tolist())
            # residual = sum coe * lambda0 against the reference's, within sum |coe| * C eps s
            with R.mpmath.workdps(R.MP_DPS):
                want = R.mpmath.fsum(R.mpmath.mpf(float(c)) * ref.w_mp[0] for c, ref in zip(coe, refs))
                tol = sum(abs(float(c)) * R.C_BAR * R.EPS * ref.s for c, ref in zip(coe, refs)) + R.TINY
                assert float(abs(R.mpmath.mpf(r) - want)) <= tol, (r, float(want), tol)
    finally:
        ctx.close()
    rep.done()


# ------------------------------------------------------------------------------------------------ designed clouds
VOX = 1.0


def _frame(rng):
    n = rng.normal(size=3); n /= np.linalg.norm(n)
    t1 = np.cross(n, rng.normal(size=3)); t1 /= np.linalg.norm(t1)
    return n, t1, np.cross(n, t1)


def clouds(seed=7, per_class=24):
    """(class, points) with one cluster per voxel of size VOX, 10-100 m from the origin"""
    rng = np.random.default_rng(seed)
    used, out = set(), []
    kinds = ("grid", "disc", "arc", "pole", "blob", "tilted")
    for kind in kinds:
        for _ in range(per_class):
            while True:
                d = rng.normal(size=3); d *= rng.uniform(10, 100) / np.linalg.norm(d)
                key = tuple(np.floor(d / VOX).astype(int))
                if key not in used:
                    used.add(key)
                    break
            c = (np.array(key) + 0.5) * VOX
            n, t1, t2 = _frame(rng)
            h = 0.35 * VOX
            if kind == "grid":                 # square grid: lambda1 = lambda2
                k = int(rng.integers(5, 9)); g = np.linspace(-h, h, k)
                a, b = np.meshgrid(g, g)
                p = np.outer(a.ravel(), t1) + np.outer(b.ravel(), t2)
            elif kind == "disc":               # rings at uniform angles: lambda1 = lambda2
                p = []
                for rr in (0.1, 0.2, 0.3):
                    th = np.linspace(0, 2 * np.pi, 12, endpoint=False)
                    p.append(np.outer(rr * np.cos(th), t1) + np.outer(rr * np.sin(th), t2))
                p = np.concatenate(p)
            elif kind == "arc":                # one scan ring on a wall: line-like
                R0 = rng.uniform(5, 30); th = np.linspace(-h / R0, h / R0, int(rng.integers(15, 40)))
                p = np.outer(R0 * np.sin(th), t1) + np.outer(R0 * (1 - np.cos(th)), t2)
            elif kind == "pole" and len(out) % 2:    # lambda0 ~ lambda1 << lambda2, noisy
                m = int(rng.integers(15, 40))
                p = np.outer(rng.uniform(-h, h, m), n) + np.outer(rng.normal(0, 0.01, m), t1) + np.outer(rng.normal(0, 0.01, m), t2)
            elif kind == "pole":               # square cross-section repeated along the axis: lambda0 = lambda1 (the Jacobi fallback)
                a = np.repeat(rng.uniform(-h, h, int(rng.integers(4, 10))), 4)
                th = np.tile(np.arange(4) * (np.pi / 2), len(a) // 4)
                p = np.outer(a, n) + np.outer(0.01 * np.cos(th), t1) + np.outer(0.01 * np.sin(th), t2)
            elif kind == "blob":
                p = np.clip(rng.normal(0, 0.1, (int(rng.integers(20, 50)), 3)), -h, h)
            else:                              # tilted rectangle, noisy
                m = int(rng.integers(20, 60)); e = rng.uniform(0.05, h, 2)
                p = np.outer(rng.uniform(-1, 1, m) * e[0], t1) + np.outer(rng.uniform(-1, 1, m) * e[1], t2) + np.outer(rng.normal(0, 0.003, m), n)
            out.append((kind, c + p))
    return out


def _near_threshold(w, mine, thre):
    return abs(w[0] - mine) <= 1e-9 * abs(mine) or (w[2] != 0 and abs(w[0] / w[2] - thre) <= 1e-9 * abs(thre))


def _check_sums(rep, cls, pa, w, U, normal=None):
    ref, m2 = R.ref_from_sums(pa)
    q = R.check(ref, w, U, scale=m2)
    if normal is not None and ref.gap[0] >= 1e-3 * m2:
        q["normal"] = R._sin(np.asarray(normal), ref.V[:, 0]) / (R.C_BAR * R.EPS * (m2 / ref.gap[0]))
    rep.add(cls, q, (pa[9], ref.w.tolist()))
    return ref


def _map_opts(capi, W):
    o = capi.default_options()
    o.win_size = W
    o.voxel_size = VOX
    o.max_layer = 2
    o.min_eigen_value = 0.0025
    for i in range(4):
        o.plane_eigen_value_thre[i] = 0.25
        o.min_point[i] = 5
    o.max_points = 100000
    return o


def test_map_leaf_fit_and_margi(capi):
    W = 4
    cs = clouds()
    pts = np.concatenate([p for _, p in cs])
    keymap = {tuple(np.floor(p[0] / VOX).astype(int)): kind for kind, p in cs}
    poses = np.tile(IDENT, (W, 1))
    o = _map_opts(capi, W)
    ctx = capi.Context(o)
    try:
        ctx.cut_voxel(0, pts, poses[0])
        ctx.recut(1, poses, multi=False)
        rec = Worst("map leaf fit")
        seen = set()
        d = ctx.dump_leaves()
        n_plane = 0
        for row in d:
            L = int(row[3])
            if row[5] <= o.min_point[L] or not np.any(row[13:22]):
                continue                        # no plane fit ran on this leaf
            cls = keymap[(int(row[0]), int(row[1]), int(row[2]))]
            seen.add(cls)
            ref = _check_sums(rec, cls, row[22:32], row[10:13], row[13:22], normal=row[35:38] if row[7] else None)
            if not _near_threshold(ref.w, o.min_eigen_value, o.plane_eigen_value_thre[L]):
                assert bool(row[7]) == R.plane_judge(ref.w, o.min_eigen_value, o.plane_eigen_value_thre[L]), (cls, ref.w, row[7])
            n_plane += int(row[7])
        assert seen == {"grid", "disc", "arc", "pole", "blob", "tilted"}, seen
        assert n_plane >= 24
        rec.done()
        # margi refits every plane leaf from its sums (the second map site)
        ctx.margi(1, poses)
        rem = Worst("map margi")
        for row in ctx.dump_leaves():
            if not row[7]:
                continue
            cls = keymap[(int(row[0]), int(row[1]), int(row[2]))]
            _check_sums(rem, cls, row[22:32], row[10:13], row[13:22])
        rem.done()
    finally:
        ctx.close()


def test_gba_build(capi):
    W = 4
    cs = clouds(seed=8)
    rng = np.random.default_rng(9)
    frames = [[] for _ in range(W)]
    for _, p in cs:                             # every cluster seen by several keyframes
        f = rng.integers(0, W, len(p))
        f[:W] = np.arange(W)
        for i in range(W):
            frames[i].append(p[f == i])
    clouds_w = [np.concatenate(fr) for fr in frames]
    poses = np.tile(IDENT, (W, 1))
    o = _map_opts(capi, W)
    ctx = capi.Context(o)
    try:
        n = ctx.gba_build(clouds_w, poses, VOX, 0.1, [0.25] * 4)
        assert n >= 24
        ev, evec, pa = ctx.read_back()
        rep = Worst("GBA build")
        for k in range(n):
            ref = _check_sums(rep, "factor", pa[k], ev[k], evec[k])
            assert R.plane_judge(ref.w, 0.1, 0.25) or _near_threshold(ref.w, 0.1, 0.25)
        rep.done()
    finally:
        ctx.close()
