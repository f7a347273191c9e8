"""Plain numpy restatement of vba_kf_surfel_export (include/voxelba.h) on top of tests/export_voxel_ref.py: the
same sequence S, the same groups, the same np.add.at chains; then the centred moments in the contract's operation order, the
assembly of the 12-float record from an eigen-decomposition, a 60-digit reference of the covariance, the derived bar on its entries
and the scene of the tests.  TEST INFRASTRUCTURE only.

numpy's elementwise operations round every product and sum on its own (nothing is fused), which is what the contract needs."""
import mpmath
import numpy as np

import eig3_ref as er
import export_voxel_ref as ev

U = 2.0 ** -53                       # unit roundoff of f64
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # xx xy xz yy yz zz
MP_DPS = 60


# ------------------------------------------------------------------------------------------------ moments
def products(d, pairs=PAIRS):
    return np.stack([d[:, i] * d[:, j] for i, j in pairs], axis=1)


def moments(S, voxel_size, centre="mean", inv_cnt=True, pairs=PAIRS, reverse=False):
    """dict of the per-voxel quantities of ALL voxels in first-occurrence order: first, cnt, vox (voxel of every record), c (f64
    mean), M (chains of the products in the order of S), C.  The keywords are the mutations of the CPU test: centre "float"
    centres on the narrowed mean, inv_cnt False divides by cnt, pairs reorders the products, reverse adds the chains backwards."""
    first, cnt, vox, _, sums = ev.centroids(S, voxel_size)
    a = S[:, :3].astype(np.float64)
    inv = 1.0 / cnt.astype(np.float64)
    c = sums * inv[:, None]
    cc = c.astype(np.float32).astype(np.float64) if centre == "float" else c
    p = products(a - cc[vox], pairs)
    M = np.zeros((len(first), 6))
    if reverse:
        np.add.at(M, vox[::-1], p[::-1])
    else:
        np.add.at(M, vox, p)                                  # unbuffered: ((0 + t_0) + t_1) + ... in the order of S
    C = M * inv[:, None] if inv_cnt else M / cnt[:, None].astype(np.float64)
    return dict(first=first, cnt=cnt, vox=vox, c=c, M=M, C=C)


def raw_moments(S, voxel_size):
    """the one-pass form the contract forbids: C = sum(a a^T) / N - c c^T"""
    first, cnt, vox, _, sums = ev.centroids(S, voxel_size)
    a = S[:, :3].astype(np.float64)
    inv = 1.0 / cnt.astype(np.float64)
    c = sums * inv[:, None]
    P = np.zeros((len(first), 6))
    np.add.at(P, vox, products(a))
    return P * inv[:, None] - products(c)


def sensors(sessions, S_kf, first):
    """x0.p of the keyframe of every voxel's first record"""
    p = np.concatenate([np.asarray(poses, dtype=np.float64).reshape(-1, 12)[:, 9:12] for _, poses, _ in sessions])
    return p[S_kf[first]]


def assemble(c, w, V, cnt, sensor, inten, orient="first", small=3):
    """the record of include/voxelba.h from an ascending eigen-decomposition (w [m][3], V [m][3][3] with the vectors in the
    columns).  orient "away" and small other than 3 are mutations."""
    w = np.maximum(np.asarray(w, dtype=np.float64), 0.0)
    n = np.asarray(V, dtype=np.float64)[:, :, 0].copy()
    v = sensor - c
    dot = (n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1]) + n[:, 2] * v[:, 2]
    flip = dot > 0.0 if orient == "away" else dot < 0.0
    n[flip] = -n[flip]
    n[cnt < small] = 0.0
    tr = (w[:, 0] + w[:, 1]) + w[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        plan = np.where(tr > 0.0, w[:, 0] / tr, 0.0)
    rec = np.concatenate([c, inten[:, None], n, np.sqrt(w), plan[:, None], cnt[:, None].astype(np.float64)], axis=1)
    return np.ascontiguousarray(rec.astype(np.float32))


def sym(C6):
    a = np.asarray(C6, dtype=np.float64)
    return np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])


# ------------------------------------------------------------------------------------------------ the exact covariance and the bar
def exact(S, first, cnt, vox):
    """(mean f64 [m][3], covariance f64 [m][6], D [m][3] = max |a - mean| per axis, A [m][3] = max |a| per axis) of the float
    records, every sum formed at 60 digits (exact: the terms are floats) and rounded once"""
    a = S[:, :3].astype(np.float64)
    m = len(first)
    members = [[] for _ in range(m)]
    for i, v in enumerate(vox):
        members[v].append(i)
    mean = np.zeros((m, 3)); cov = np.zeros((m, 6)); D = np.zeros((m, 3)); A = np.zeros((m, 3))
    with mpmath.workdps(MP_DPS):
        for v in range(m):
            pts = [[mpmath.mpf(float(a[i, k])) for k in range(3)] for i in members[v]]
            N = mpmath.mpf(len(pts))
            mu = [mpmath.fsum(p[k] for p in pts) / N for k in range(3)]
            dev = [[p[k] - mu[k] for k in range(3)] for p in pts]
            mean[v] = [float(x) for x in mu]
            cov[v] = [float(mpmath.fsum(d[i] * d[j] for d in dev) / N) for i, j in PAIRS]
            D[v] = [float(max(abs(d[k]) for d in dev)) for k in range(3)]
            A[v] = np.abs(a[members[v]]).max(axis=0)
    return mean, cov, D, A


def cov_bar(cnt, D, A):
    """Bound on |C_ij - exact| for sums formed in ANY order, by counting roundings (u = 2^-53, N = cnt, per axis A = max |a|,
    D = max |a - mean|):
      c   s is an N-term sum in any order, |ds| <= (N - 1) u N A; the reciprocal and the product add 2 u: e_c = (N + 1) u A;
      d   fl(a - c) with the perturbed c: e = e_c + u (D + e_c);
      p   |d~_i d~_j - d_i d_j| <= e_i D_j + D_i e_j + e_i e_j, and u D_i D_j for the product's own rounding;
      M   an N-term sum in any order: (N - 1) u N D_i D_j before the division;
      C   the reciprocal and the product: 2 u D_i D_j.
    In all e_i D_j + D_i e_j + e_i e_j + (N + 2) u D_i D_j, with 1 % for the terms of second order in u."""
    N = cnt.astype(np.float64)[:, None]
    e = (N + 1.0) * U * A
    e = e + U * (D + e)
    out = np.zeros((len(cnt), 6))
    for k, (i, j) in enumerate(PAIRS):
        out[:, k] = e[:, i] * D[:, j] + D[:, i] * e[:, j] + e[:, i] * e[:, j] + (N[:, 0] + 2.0) * U * D[:, i] * D[:, j]
    return 1.01 * out + er.TINY


def mean_bar(cnt, A):
    """|c - exact mean| <= (N + 1) u A (above), with the rounding of the exact mean itself"""
    return 1.01 * (cnt.astype(np.float64)[:, None] + 2.0) * U * A


# ------------------------------------------------------------------------------------------------ the record against a reference
F32 = 2.0 ** -24                     # half an ulp of a float, relative


def check_record(C6, rec, cnt, ref=None):
    """Ratios observed / bar of the eigen fields of one float record against the 50-digit eigen-decomposition of the double
    covariance C6 it was fitted to.  The bars are those of eig3_ref.check (C eps s on the eigenvalues, C eps s / gap on a vector, the
    pair's span for a close pair) carried through the square root, the quotient and the narrowing to float:
      |sqrt x - sqrt y| <= min(sqrt |x - y|, |x - y| / sqrt max(x, y));  a float is within 2^-24 of its double, relatively."""
    ref = er.Ref(sym(C6)) if ref is None else ref
    rec = np.asarray(rec, dtype=np.float64)
    bar = er.C_BAR * er.EPS * ref.s + er.TINY
    out = {}
    if not np.all(np.isfinite(rec)):
        return {"finite": np.inf}
    wr = np.maximum(ref.w, 0.0)
    sq = 0.0
    for i in range(3):
        root = np.sqrt(wr[i])
        b = min(np.sqrt(bar), bar / root if root > 0 else np.inf) + 2.0 * F32 * (root + np.sqrt(bar)) + er.TINY
        sq = max(sq, abs(rec[7 + i] - root) / b)
    out["sqrt"] = sq
    tr = wr.sum()
    if tr > 0:
        out["planarity"] = abs(rec[10] - wr[0] / tr) / (4.0 * bar / tr + 2.0 * F32)
    else:
        out["planarity"] = 0.0 if rec[10] == 0.0 else np.inf
    n = rec[4:7]
    if cnt < 3:
        out["normal"] = 0.0 if not n.any() else np.inf
        return out
    out["unit"] = abs(np.linalg.norm(n) - 1.0) / (1e-14 + 4.0 * F32)
    narrow = 4.0 * F32
    if ref.triple:
        out["normal"] = 0.0
    elif ref.pair is not None and 0 in ref.pair[:2]:
        bound = er.C_BAR * er.EPS * (ref.s / ref.pair[2])     # in the span of the pair: orthogonal to the third vector
        out["normal"] = abs(n @ ref.V[:, 2]) / (bound + narrow) if bound < 1.0 else 0.0
    else:
        bound = er.C_BAR * er.EPS * (ref.s / ref.gap[0])
        out["normal"] = er._sin(n, ref.V[:, 0]) / (bound + narrow) if bound < 1.0 else 0.0
    return out


# ------------------------------------------------------------------------------------------------ the scene
GRID = 2.0 ** -9                     # the keyframes' points are multiples of it and alone in a build voxel of this size
SHIFT = np.array([1000.5, -999.5, 1001.0])     # multiples of 0.5: the dense tile stays inside one voxel
N_KF = 6
SEED = 7


def scene(seed=SEED):
    """(clouds, poses): N_KF keyframes within +-2 m of the origin that see, in the world frame,
      three planar patches of 3 m x 3 m with 5 mm noise (a floor, a wall, an oblique one), spread over keyframes 1..5 at random, so
        that a voxel's records come from several keyframes and from both sides of 256-record boundaries;
      a dense floor tile of 420 records inside one 0.5 m voxel;  a blob;  a pole of 1 mm radius (two small eigenvalues closer than
        1e-5 of the large one: the solver's close-pair fallback);
    and in keyframe 0, whose rotation is the identity and whose translation is dyadic so that its world floats are exact:
      exactly collinear triples, single records and pairs, each alone in a 0.5 m voxel.
    Points are rounded to multiples of GRID in their keyframe's frame and are unique there, so a store built at voxel GRID keeps
    every one of them as it is."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    poses = [np.concatenate([np.eye(3).ravel(), [0.25, -0.5, 0.75]])]
    for _ in range(N_KF - 1):
        R = Rotation.from_rotvec(rng.uniform(-1.2, 1.2, 3)).as_matrix().ravel()
        poses.append(np.concatenate([R, rng.uniform(-2.0, 2.0, 3)]))
    poses = np.stack(poses)

    def patch(origin, t1, t2, n, ext, count):
        uv = rng.uniform(-ext, ext, (count, 2))
        return origin + np.outer(uv[:, 0], t1) + np.outer(uv[:, 1], t2) + np.outer(rng.normal(0, 0.005, count), n)

    ez = np.array([0.0, 0.0, 1.0]); ex = np.array([1.0, 0.0, 0.0]); ey = np.array([0.0, 1.0, 0.0])
    ob = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    o1 = np.cross(ob, ez); o1 /= np.linalg.norm(o1); o2 = np.cross(ob, o1)
    world = [
        patch(np.array([0.1, -0.2, -2.6]), ex, ey, ez, 1.5, 1300),             # floor, below every sensor
        patch(np.array([3.3, 0.3, 0.2]), ey, ez, ex, 1.5, 1300),               # wall, beyond every sensor in x
        patch(np.array([-3.5, -3.5, -3.5]), o1, o2, ob, 1.5, 1100),            # oblique
        patch(np.array([0.25, 0.25, -2.6]), ex, ey, ez, 0.15, 420),            # the dense tile: x, y in (0.1, 0.4)
        np.array([-4.2, 4.3, 1.2]) + rng.normal(0, 0.08, (300, 3)),            # blob
        np.array([4.3, -4.2, 0.0]) + np.stack([rng.normal(0, 0.001, 240), rng.normal(0, 0.001, 240), rng.uniform(-1.0, 1.0, 240)], axis=1),   # pole
    ]
    world = np.concatenate(world)
    owner = rng.integers(1, N_KF, len(world))
    clouds = []
    # keyframe 0: dyadic points, world = p + (0.25, -0.5, 0.75) exactly, far from everything else (y beyond 7 m)
    k0 = []
    for t in range(6):                                                        # collinear triples a, a + d, a + 2 d inside one 0.5 m voxel
        a = np.array([-6.0 + 1.0 * t, 8.0, 2.0]) + np.array([0.0625, 0.0625, 0.03125]) - poses[0][9:12]
        d = np.array([[0.0625, 0.03125, 0.125], [0.125, 0.0, 0.0], [0.0, 0.0625, 0.0625], [0.03125, 0.0625, -0.0078125], [0.0625, 0.0625, 0.0625],
                      [0.0, 0.0, 0.125]])[t]
        k0 += [a, a + d, a + 2 * d]
    for t in range(5):                                                        # single records
        k0.append(np.array([-6.0 + 1.0 * t, 10.0, 2.0]) + 0.125 - poses[0][9:12])
    for t in range(5):                                                        # pairs
        a = np.array([-6.0 + 1.0 * t, 12.0, 2.0]) + 0.125 - poses[0][9:12]
        k0 += [a, a + np.array([0.0625, 0.125, 0.03125])]
    clouds.append(np.array(k0))
    for k in range(1, N_KF):
        R = poses[k][:9].reshape(3, 3); t = poses[k][9:12]
        local = (world[owner == k] - t) @ R                                   # R^T (w - t)
        local = np.round(local / GRID) * GRID
        local[local == 0.0] = GRID                                            # (the store's merge moves a point by R^T R: a zero would not come back as zero)
        _, idx = np.unique(local, axis=0, return_index=True)
        clouds.append(np.ascontiguousarray(local[np.sort(idx)]))
    assert all(np.array_equal(c.astype(np.float32).astype(np.float64), c) for c in clouds)
    return clouds, poses


def shifted(poses):
    p = np.array(poses, dtype=np.float64)
    p[:, 9:12] += SHIFT
    return p


def surfels(sessions, jump, voxel_size, min_count, fit):
    """The whole restatement: (records float32 [m][12], cov f64 [m][6], counts int32 [m]) of the kept voxels.  fit(C [m][6]) ->
    (w [m][3], V [m][3][3]) is the eigen-solver: the host build of csrc/vba_surfel_fit.hpp in the tests."""
    S, kf = ev.sequence(sessions, jump)
    if len(S) == 0:
        return np.zeros((0, 12), np.float32), np.zeros((0, 6)), np.zeros(0, np.int32)
    mo = moments(S, voxel_size)
    keep = mo["cnt"] >= min_count
    c, C, cnt, first = mo["c"][keep], mo["C"][keep], mo["cnt"][keep], mo["first"][keep]
    sen = sensors(sessions, kf, first)
    w, V = fit(C)
    rec = assemble(c, w, V, cnt, sen, S[first, 3].astype(np.float64))
    return rec, C, cnt.astype(np.int32)


# ------------------------------------------------------------------------------------------------ the host build of the fit
def build_host(workdir, lib_path):
    """compile tests/host/export_surfel_host.cpp without contraction; returns the program's path"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "export_surfel_host")
    libdir = os.path.dirname(lib_path)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "export_surfel_host.cpp"), "-o", exe, "-L", libdir, "-lvoxelba",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def host_fit(exe, workdir, c, C, sensor, cnt, inten):
    """(records float32 [m][12], w [m][3], V [m][3][3]) of the program's fit mode"""
    import os
    import struct
    import subprocess
    m = len(cnt)
    rows = np.concatenate([c, C, sensor, np.asarray(cnt, dtype=np.float64)[:, None], np.asarray(inten, dtype=np.float64)[:, None]], axis=1)
    fin, fout = os.path.join(str(workdir), "fit_in.bin"), os.path.join(str(workdir), "fit_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<q", m)); f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
    r = subprocess.run([exe, "fit", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = open(fout, "rb").read()
    rec = np.frombuffer(raw, dtype=np.float32, count=12 * m).reshape(m, 12).copy()
    eig = np.frombuffer(raw, dtype=np.float64, count=12 * m, offset=48 * m).reshape(m, 12)
    return rec, eig[:, :3].copy(), eig[:, 3:].reshape(m, 3, 3).copy()


def host_solver(exe, workdir):
    """fit(C) -> (w, V) for surfels(): the program's decomposition of every row of C"""
    def fit(C):
        m = len(C)
        z = np.zeros((m, 3))
        _, w, V = host_fit(exe, workdir, z, C, z, np.full(m, 3), np.zeros(m))
        return w, V
    return fit
