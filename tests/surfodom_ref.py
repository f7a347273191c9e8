"""Plain numpy restatement of the prior-map odometry update (vba_odom_surfel_update, include/voxelba.h) on top
of tests/surfreg_ref.py: one point loop in the kernels' order (surfreg_ref.one_pass for the points, the lane chains, the butterfly,
(w0 + w1) + (w2 + w3), the 29 -> 34 column mapping, the seven-group reduction of odom_sum_partials), the EKF step and loop of
csrc/vba_odom_ekf.hpp with numpy's inverse, the priors, starts and cases of the tests, the measured spreads behind their bars, and
the driver of tests/host/surfodom_host.cpp.  TEST INFRASTRUCTURE only."""
import os
import struct
import subprocess

import numpy as np

import surfreg_ref as rr

ROW = 34
MAX_BLOCKS = 1024
MAX_ITER = 4
# column c of a row takes sum SRC[c] of the 29; columns 21..26 negated
SRC = np.array(list(range(27)) + list(range(15, 21)) + [28])
SIGN = np.where((np.arange(ROW) >= 21) & (np.arange(ROW) < 27), -1.0, 1.0)


# ------------------------------------------------------------------------------------------------ one point loop
def blocks(n):
    return min((n + 255) // 256, MAX_BLOCKS)


def wg_sums(terms):
    """[nb][29]: lane l of workgroup b adds the rows b * 256 + l, (b + nb) * 256 + l, ... in ascending order (a gated-out point's
    row is zero: x + 0 = x), a wave adds its lanes by the xor butterfly 32 .. 1, a workgroup its waves as (w0 + w1) + (w2 + w3)"""
    n = len(terms); nb = blocks(n)
    if nb == 0:
        return np.zeros((0, rr.PART))
    J = (n + nb * 256 - 1) // (nb * 256)
    T = np.zeros((J * nb * 256, rr.PART)); T[:n] = terms
    T = T.reshape(J, nb, 256, rr.PART)
    acc = np.zeros((nb, 256, rr.PART))
    for j in range(J):
        acc = acc + T[j]
    x = acc.reshape(nb, 4, 64, rr.PART)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[:, :, lanes ^ m, :]
    w = x[:, :, 0, :]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def to34(s29, flip=True, w_from=15, swap_blocks=False):
    """rows [..][29] -> [..][34].  Mutations: flip False (HTz = +J^T W d), w_from 0 (columns 27..32 from the rotation block),
    swap_blocks (rotation and translation blocks of HTH and HTz exchanged)"""
    s29 = np.asarray(s29, dtype=np.float64)
    src = SRC.copy(); src[27:33] = np.arange(w_from, w_from + 6)
    out = s29[..., src] * (SIGN if flip else 1.0)
    if swap_blocks:
        H = np.zeros(s29.shape[:-1] + (6, 6)); iu = np.triu_indices(6)
        H[..., iu[0], iu[1]] = out[..., :21]; H[..., iu[1], iu[0]] = out[..., :21]
        p = [3, 4, 5, 0, 1, 2]
        H = H[..., p, :][..., :, p]
        out = out.copy(); out[..., :21] = H[..., iu[0], iu[1]]; out[..., 21:27] = out[..., 21:27][..., p]
    return out


def sum_partials(partial):
    """[34] of rows [nb][34] in the order of odom_sum_partials: lane t < 238 adds the elements t, t + 238, ... of the flat array,
    lane c adds the seven group sums c, c + 34, ... in group order"""
    flat = np.asarray(partial, dtype=np.float64).reshape(-1)
    L = 7 * ROW
    K = (len(flat) + L - 1) // L
    pad = np.zeros(K * L); pad[:len(flat)] = flat
    rd = np.zeros(L)
    for k in range(K):
        rd = rd + pad[k * L:(k + 1) * L]
    g = rd.reshape(7, ROW)
    s = g[0].copy()
    for k in range(1, 7):
        s = s + g[k]
    return s


def point_loop(mp, pnt, R, t, gate=3.0, neighbors=7, map34=None, **mut):
    """dict(cell, gate, ps (the pass of surfreg_ref), partial [nb][34], cost [nb], sums [34]) of one point loop at (R, t)"""
    ps = rr.one_pass(mp, pnt, R, t, gate, neighbors, **mut)
    w = wg_sums(ps["terms"])
    partial = (map34 or to34)(w)
    return dict(cell=ps["cell"], gate=ps["gate"], ps=ps, partial=partial, cost=w[:, 27].copy(), sums=sum_partials(partial))


def exact34(ps):
    """(exact sums [34], bar [34]) of a pass: surfreg_ref.exact_sums and surfreg_ref.sums_bar through the column mapping (the bar of
    HTz is the bar of g, the bars of columns 27..32 those of sums 15..20, the count exact)"""
    exact, ab = rr.exact_sums(ps)
    bar = rr.sums_bar(int(ps["gate"].sum()), ab)
    return exact[SRC] * SIGN, bar[SRC]


# ------------------------------------------------------------------------------------------------ the EKF step and loop
def so3_log(R):
    tr = np.trace(R)
    theta = 0.0 if tr > 3.0 - 1e-6 else np.arccos(0.5 * (tr - 1))
    K = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return (0.5 if abs(theta) < 0.001 else 0.5 * theta / np.sin(theta)) * K


def unpack34(s34):
    HTH = rr.unpack_H(s34)
    n = s34[27:33]
    return HTH, np.array(s34[21:27]), np.array([[n[0], n[1], n[2]], [n[1], n[3], n[4]], [n[2], n[4], n[5]]]), int(s34[33])


def ekf_step(s34, cov_inv, xp, xc):
    """(solution [15], G [15][15], A) of VS:1053-1060 on the sums"""
    HTH, HTz, _, _ = unpack34(s34)
    A = cov_inv.copy(); A[:6, :6] += HTH
    K1 = np.linalg.inv(A)
    G = np.zeros((15, 15)); G[:, :6] = K1[:, :6] @ HTH
    vec = np.concatenate([so3_log(xc[1:10].reshape(3, 3).T @ xp[1:10].reshape(3, 3)), xp[10:22] - xc[10:22]])
    return K1[:, :6] @ HTz + vec - G[:, :6] @ vec[:6], G, A


def ratio_of(rot_add, tra_add):
    """the stop rule's own figure: below 1 the iteration has converged (VS:1072)"""
    return max(rot_add * 57.3 / 0.01, tra_add * 100 / 0.015)


def loop(mp, pnt, state, cov, gate=3.0, neighbors=7, min_matches=30, min_eig=0.0, kd=0, map34=None, **mut):
    """odom_ekf_iterate's loop around point_loop -> dict(state, cov, iterations, match_num [4], rot_add [4], tra_add [4], ratio
    (per iteration run), rematch (rematch_num before each iteration run), rematch_num, nnt, eig_min, ok)"""
    pnt = np.asarray(pnt, dtype=np.float64).reshape(-1, 3)
    xp = np.array(state, dtype=np.float64); xc = xp.copy(); P = np.array(cov, dtype=np.float64).reshape(15, 15)
    cov_inv = np.linalg.inv(P)
    out = dict(iterations=0, match_num=np.zeros(4, np.int64), rot_add=np.zeros(4), tra_add=np.zeros(4), ratio=[], rematch=[])
    rematch = 0; conv_once = False; nnt = np.zeros((3, 3)); Pn = P.copy()
    for it in range(MAX_ITER):
        s34 = point_loop(mp, pnt, xc[1:10].reshape(3, 3), xc[10:13], gate, neighbors, map34, **mut)["sums"] if len(pnt) else np.zeros(ROW)
        sol, G, _ = ekf_step(s34, cov_inv, xp, xc)
        _, _, nnt, match = unpack34(s34)
        xc = xc.copy()
        if np.linalg.norm(sol[:3]) >= 1e-11:
            xc[1:10] = (xc[1:10].reshape(3, 3) @ rr.so3_exp(sol[:3])).ravel()
        xc[10:22] += sol[3:]
        ra, ta = float(np.linalg.norm(sol[:3])), float(np.linalg.norm(sol[3:6]))
        out["rematch"].append(rematch); out["ratio"].append(ratio_of(ra, ta))
        out["rot_add"][it], out["tra_add"][it], out["match_num"][it] = ra, ta, match
        out["iterations"] = it + 1
        conv = ra * 57.3 < 0.01 and ta * 100 < 0.015
        if kd:
            if conv:
                rematch += 1; conv_once = True
        elif conv or (rematch == 0 and it == MAX_ITER - 2):
            rematch += 1
        if rematch >= 2 or it == MAX_ITER - 1:
            Pn = (np.eye(15) - G) @ P
            break
    eig = float(np.linalg.eigvalsh(nnt)[0])
    last = int(out["match_num"][out["iterations"] - 1])
    out.update(state=xc, cov=Pn, rematch_num=rematch, nnt=nnt, eig_min=eig, ok=int(last >= min_matches and eig >= min_eig))
    return out


# ------------------------------------------------------------------------------------------------ priors, starts, cases
D2 = np.repeat([1e-4, 1e-2, 1e-2, 1e-6, 1e-4], 3)
STARTS = {"fine": (0.0005, 0.005), "track": (0.02, 0.2), "small": (0.05, 0.5)}        # name -> (metres, degrees)
START_SEED = 4


def prior_cov():
    """a correlated 15 x 15 prior: the correlations make v, bg and ba move with the pose, which exercises G(:,0:6)"""
    M = np.random.default_rng(5).normal(size=(15, 15)) * 0.05
    Cm = np.eye(15) + 0.2 * (M + M.T)
    Cm = Cm @ Cm.T
    d = np.sqrt(np.diag(Cm))
    Cm = Cm / np.outer(d, d)
    D = np.sqrt(D2)
    return Cm * np.outer(D, D)


def start_of(Rg, tg, which):
    """surfreg_ref.start_of's recipe at the sizes of this update"""
    metres, degrees = STARTS[which]
    rng = np.random.default_rng(START_SEED)
    a = rng.normal(size=3); a *= np.deg2rad(degrees) / np.linalg.norm(a)
    b = rng.normal(size=3); b *= metres / np.linalg.norm(b)
    return Rg @ rr.so3_exp(a), tg + b


def state_of(R, p, v=(0.3, -0.2, 0.1), bg=(0.01, 0.02, -0.01), ba=(0.05, -0.03, 0.02)):
    s = np.zeros(25)
    s[0] = 12.5; s[1:10] = np.asarray(R).ravel(); s[10:13] = p; s[13:16] = v; s[16:19] = bg; s[19:22] = ba; s[22:25] = [0, 0, -9.8]
    return s


LOOP_CASES = [(scene, voxel, which, nb) for scene in ("near", "far") for voxel in rr.VOXELS for which in ("fine", "track", "small")
              for nb in (1, 7) if which != "small" or voxel == 0.5]
EXPECTED_ITERATIONS = {"fine": 3, "track": 4, "small": 4}


def case_id(c):
    return "%s-%g-%s-%d" % c


def decisive(lp):
    """the ratios of the iterations whose convergence decision can change the stop: 0 and 1, and 2 when rematch_num is already 1"""
    return [r for it, (r, m) in enumerate(zip(lp["ratio"], lp["rematch"])) if it < 2 or (it == 2 and m == 1)]


def pose_distance(state, Rg, tg):
    return rr.pose_distance(state[1:10].reshape(3, 3), state[10:13], Rg, tg)


def measure_spread(run, state, cov, seed=99, count=16, size=1e-12):
    """(largest spread of an R entry, a p component, a v / bg / ba component of the final state, a covariance entry relative to the
    largest, a rot_add slot, a tra_add slot) of `run(state, cov) -> loop dict` (the restatement or the host program, never the device)
    over `count` priors that differ from the case's by +-size in the six pose components; iterations and match_num[] must not move"""
    rng = np.random.default_rng(seed)
    S, P, ra, ta, its = [], [], [], [], set()
    for _ in range(count):
        sg = rng.choice([-1.0, 1.0], 6) * size
        st = np.array(state)
        st[1:10] = (st[1:10].reshape(3, 3) @ rr.so3_exp(sg[:3])).ravel(); st[10:13] += sg[3:]
        lp = run(st, cov)
        S.append(lp["state"]); P.append(np.asarray(lp["cov"]).ravel()); ra.append(lp["rot_add"]); ta.append(lp["tra_add"])
        its.add((int(lp["iterations"]), tuple(int(x) for x in lp["match_num"])))
    assert len(its) == 1, its
    S, P, ra, ta = np.array(S), np.array(P), np.array(ra), np.array(ta)
    sp = lambda a: float((a.max(0) - a.min(0)).max())
    return sp(S[:, 1:10]), sp(S[:, 10:13]), sp(S[:, 13:22]), sp(P) / float(np.abs(P).max()), sp(ra), sp(ta)


# measure_spread of every loop case, as measured on the host program.  The result is a MAP estimate that the
# prior takes part in: R and p move by the prior's small share of a 1e-12 change; v, bg, ba move with the pose step through the
# correlations of P, and rot_add[0], tra_add[0] are the distance from the start itself, so they show the 1e-12 changes whole
# (sqrt(3) 1e-12 per sign pattern).  The far scene's p (about 1000) moves by whole units in its last place: 0 or 1.1e-13.
SPREAD = {
    ("near", 0.5, "fine", 1): (9.69e-15, 2.08e-14, 1.95e-12, 6.60e-15, 3.07e-12, 2.60e-12),
    ("near", 0.5, "fine", 7): (9.44e-15, 1.98e-14, 1.95e-12, 7.31e-15, 2.40e-12, 3.02e-12),
    ("near", 0.5, "track", 1): (9.71e-15, 2.12e-14, 1.95e-12, 7.23e-15, 2.23e-12, 2.75e-12),
    ("near", 0.5, "track", 7): (9.52e-15, 2.01e-14, 1.95e-12, 5.70e-15, 2.44e-12, 2.75e-12),
    ("near", 0.5, "small", 1): (9.63e-15, 2.02e-14, 1.95e-12, 6.68e-15, 2.19e-12, 2.84e-12),
    ("near", 0.5, "small", 7): (9.55e-15, 2.08e-14, 1.95e-12, 6.11e-15, 2.16e-12, 2.83e-12),
    ("near", 1.0, "fine", 1): (1.10e-14, 1.95e-14, 1.94e-12, 9.14e-15, 3.24e-12, 2.57e-12),
    ("near", 1.0, "fine", 7): (1.10e-14, 1.91e-14, 1.94e-12, 1.19e-14, 2.65e-12, 2.45e-12),
    ("near", 1.0, "track", 1): (1.11e-14, 1.94e-14, 1.94e-12, 1.00e-14, 2.39e-12, 2.71e-12),
    ("near", 1.0, "track", 7): (1.10e-14, 2.01e-14, 1.94e-12, 9.43e-15, 2.38e-12, 2.67e-12),
    ("far", 0.5, "fine", 1): (9.71e-15, 0.00e+00, 1.95e-12, 6.79e-15, 3.08e-12, 2.66e-12),
    ("far", 0.5, "fine", 7): (1.07e-14, 0.00e+00, 1.95e-12, 9.27e-15, 2.43e-12, 3.09e-12),
    ("far", 0.5, "track", 1): (1.12e-14, 0.00e+00, 1.95e-12, 8.07e-15, 2.21e-12, 2.81e-12),
    ("far", 0.5, "track", 7): (8.99e-15, 0.00e+00, 1.95e-12, 6.34e-15, 2.47e-12, 2.81e-12),
    ("far", 0.5, "small", 1): (1.00e-14, 0.00e+00, 1.95e-12, 8.55e-15, 2.19e-12, 2.91e-12),
    ("far", 0.5, "small", 7): (9.91e-15, 0.00e+00, 1.95e-12, 8.44e-15, 2.17e-12, 2.90e-12),
    ("far", 1.0, "fine", 1): (1.34e-14, 1.14e-13, 1.95e-12, 6.85e-15, 2.57e-12, 2.56e-12),
    ("far", 1.0, "fine", 7): (1.15e-14, 0.00e+00, 1.95e-12, 1.09e-14, 3.08e-12, 2.96e-12),
    ("far", 1.0, "track", 1): (1.14e-14, 1.14e-13, 1.95e-12, 6.42e-15, 2.70e-12, 2.78e-12),
    ("far", 1.0, "track", 7): (1.25e-14, 0.00e+00, 1.94e-12, 7.89e-15, 2.67e-12, 2.80e-12),
}


def bars(case, h):
    """bars on |x - x'| for (R entries, p, v / bg / ba, covariance entries, rot_add slots, tra_add slots) against the host program's
    result h: 4 x the measured spread, never below 4 units in the last place of the compared numbers (1 for R, the largest |p|, the
    largest of v / bg / ba, the largest covariance entry, the slot itself)"""
    sR, sp, sv, sP, sra, sta = SPREAD[case]
    st = h["state"]; P = np.abs(np.asarray(h["cov"])).max()
    return dict(R=4 * max(sR, 2.0 ** -52), p=4 * max(sp, float(np.spacing(np.abs(st[10:13]).max()))),
                v=4 * max(sv, float(np.spacing(np.abs(st[13:22]).max()))), P=4 * max(sP * P, float(np.spacing(P))),
                rot=4 * np.maximum(sra, np.spacing(np.abs(h["rot_add"]))), tra=4 * np.maximum(sta, np.spacing(np.abs(h["tra_add"]))))


def errors(got, h):
    """the figures bars() bounds, of a result `got` against h"""
    a, b = np.asarray(got["state"]), np.asarray(h["state"])
    return dict(R=float(np.abs(a[1:10] - b[1:10]).max()), p=float(np.abs(a[10:13] - b[10:13]).max()), v=float(np.abs(a[13:22] - b[13:22]).max()),
                P=float(np.abs(np.asarray(got["cov"]).ravel() - np.asarray(h["cov"]).ravel()).max()),
                rot=np.abs(np.asarray(got["rot_add"]) - h["rot_add"]), tra=np.abs(np.asarray(got["tra_add"]) - h["tra_add"]))


def within(err, bar):
    return all(np.all(err[k] <= bar[k]) for k in bar)


# ------------------------------------------------------------------------------------------------ the host program
def build_host(workdir, sanitize=False):
    """compile tests/host/surfodom_host.cpp without contraction; returns the program's path"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "surfodom_host_san" if sanitize else "surfodom_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + flags +
                          [os.path.join(root, "tests", "host", "surfodom_host.cpp"), "-o", exe])
    return exe


def build_adapter(workdir, lib_path):
    """compile tests/host/surfodom_adapter_host.cpp against libvoxelba.so, as surfreg_ref.build_adapter does"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(workdir), "surfodom_adapter_host")
    libdir = os.path.dirname(lib_path)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "surfodom_adapter_host.cpp"), "-o", exe, "-L", libdir, "-lvoxelba",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def host_run(exe, workdir, rec, cov6, pnt, state, cov, voxel, sigma=rr.SIGMA, min_count=rr.MIN_COUNT, gate=3.0, neighbors=7, min_matches=30,
             min_eig=0.0, kd=0, tag="run"):
    """the program's output as a dict: n_cells, nb, the taps of iteration 0 (cell, gate, partial [nb][34], cost [nb], sums [34]) and
    the loop's result (state, cov [15][15], nnt, rot_add, tra_add, match_num, iterations, ok, rematch_num, eig_min)"""
    rec = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 12); cov6 = np.ascontiguousarray(cov6, dtype=np.float64).reshape(-1, 6)
    pnt = np.ascontiguousarray(pnt, dtype=np.float64).reshape(-1, 3)
    nr, n = len(rec), len(pnt)
    fin, fout = os.path.join(str(workdir), tag + "_in.bin"), os.path.join(str(workdir), tag + "_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qq4d4i", nr, n, voxel, sigma, gate, min_eig, min_count, neighbors, min_matches, kd))
        f.write(np.ascontiguousarray(state, dtype=np.float64).reshape(25).tobytes())
        f.write(np.ascontiguousarray(cov, dtype=np.float64).reshape(225).tobytes())
        f.write(rec.tobytes()); f.write(cov6.tobytes()); f.write(pnt.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    raw = open(fout, "rb").read()
    o = [0]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=o[0]).copy()
        o[0] += a.nbytes
        return a

    head = take(np.int64, 2)
    nb = int(head[1])
    out = dict(n_cells=int(head[0]), nb=nb)
    out["cell"] = take(np.int32, n); out["gate"] = take(np.uint8, n)
    out["partial"] = take(np.float64, ROW * nb).reshape(nb, ROW); out["cost"] = take(np.float64, nb); out["sums"] = take(np.float64, ROW)
    out["state"] = take(np.float64, 25); out["cov"] = take(np.float64, 225).reshape(15, 15); out["nnt"] = take(np.float64, 9).reshape(3, 3)
    out["rot_add"] = take(np.float64, 4); out["tra_add"] = take(np.float64, 4); out["match_num"] = take(np.int32, 4)
    ints = take(np.int32, 4)
    out["iterations"], out["ok"], out["rematch_num"] = int(ints[0]), int(ints[1]), int(ints[2])
    out["eig_min"] = float(take(np.float64, 1)[0])
    assert o[0] == len(raw), (o[0], len(raw))
    return out
