"""High-precision reference, magnitude shadow, rounding counts, bars and corpora for the passes of pose-graph optimisation
(csrc/vba_pgo_math.hpp under the kernels of csrc/vba_kernels_pgo.hpp; DESIGN.md §2, "What pins the pose-graph passes").  A helper shared
by tests/test_pgo_ref_cpu.py (the g++ build of the very header, tests/host/pgo_host.cpp: calibration and teeth) and
tests/test_gpu_pgo_passes.py (the device, through vba_debug_pgo_step).  No GPU code; nothing outside the repository is read.

Reference.  The literal formulas of DESIGN.md §12 "Conventions" on the doubles the kernel reads (poses, Z, lambda = fl(1 / var) as the
host plan forms it):  e = Log(Z^-1 Xi^-1 Xj) (prior: Log(P^-1 Xk)),  Jj = Jr^-1(e) = [[Ji3, 0], [-Ji3 Q Ji3, Ji3]] with Barfoot's Q,
Ji = -Jj Ad(Xj^-1 Xi),  H = J^T Lambda J,  g = J^T Lambda e,  cost = e^T Lambda e / 2.  The coefficient functions are the EXACT ones at
every angle (sin x / x ... (x - sin x - x^3/6) / x^5, and x / sin x of the log), by mpmath at 600 bits on the exact value of the
double-double angle: the device's Taylor series (below 0.2 rad, and below 1e-4 rad in the log) are held to their truncation error too.
sqrt, sin, cos, atan2 run in mpmath at 200 bits (imu_ref._fn); everything polynomial runs in the double-double arithmetic of
tests/hess_ref.py with the tracked type of tests/imu_ref.py (value, conditioned magnitude shadow M, rounding count k: reused, not
forked).

Counts.  k follows the order of operations of vba_pgo_math.hpp by imu_ref's rules (a +- b: max + 1; a * b, a / b: sum + 1; an exact
zero, the identity's 1 in a product, +-2^e: free; sqrt 1; a libm call LIBM_ULP = 4, assumed).  A coefficient X(phi) is a function of
one value:  k = k_phi + k_loc + T_X  and  M = max(M_loc, |X'(phi)| M_phi),  where (k_loc, M_loc) are counted along the branch's own
formula with phi as an exact input, and T_X is the truncation of the Taylor branch in units of u M_loc at the top of its range (0.2 rad;
1e-4 rad for the log's f), computed by mpmath (taylor_truncation()) and pinned in TRUNC; T_X = 0 in the closed-form branch.  The largest
k per quantity and coefficient branch over the linearisation corpus is pinned in COUNTS and asserted equal to what the code keeps.

Bars, per entry of every slot:  |x^ - x*| <= k u M, u = 2^-53; nothing is divided by a largest entry; an entry with M = 0 must be
exactly 0 (the upper-right 3x3 of every Jr^-1, so of H's translation-rotation pattern nothing is implied, but every entry of a prior's
Hjj, Hij, gj; and everything that an exactly-zero residual annihilates).

Corpus (lin_corpus): F = 300 factors in one launch: 200 edges on 100 node pairs (two parallel edges per pair, both orientations, i > j
included) and 100 priors, one per pair, so every component has one; n = 200 nodes, 300 blocks.  Factor f takes residual rotation class
f % 14 and residual translation class (f // 14) % 4, so every workgroup mixes them.  Z is the dependent quantity: Z = Xi^-1 Xj E^-1 for
the wanted residual E.  A pair one of whose factors wants a residual rotation of exactly 0 holds signed-permutation rotations and dyadic
positions (every product exact); a pair one of whose factors wants a residual translation of exactly 0 (and is not of that kind) sits
at the origin, so that v carries M = 0.  The switch classes sit at thr (1 -+ 1.001e-3): the MARGIN rule of imu_ref (strictly outside
thr (1 -+ 1e-3)) then holds whatever the last bit of the construction does."""
import ctypes as C
import math
import os

import mpmath
import numpy as np

import pgo_oracle as po
from hess_ref import DD, Tr, ZERO, U, add, neg, sc, sub
from imu_ref import LIBM_ULP, MARGIN, _cdiv, _Ctx, _dot, _fn, _hat, _matmul, _mul, _norm3, _sin, _cos

_CPREC = 600
ANGLES = (0.0, 1e-10, 1e-7, 1e-4 * (1 - 1.001e-3), 1e-4 * (1 + 1.001e-3), 1e-3, 0.05, 0.2 * (1 - 1.001e-3), 0.2 * (1 + 1.001e-3),
          0.5, 1.0, 2.0, 2.9, math.pi - 0.05)
TRANS = (0.0, 0.1, 10.0, 1e3)
F_LIN = 300
# counted by taylor_truncation() / Ref.counts(), asserted equal in tests/test_pgo_ref_cpu.py; never tuned
TRUNC = dict(A=1, B=1, C=1, D=6, E=1, F=1, f=1)
COUNTS = dict(taylor=dict(e=134, J=559, H=1123, g=698, c=273), closed=dict(e=115, J=476, H=957, g=596, c=235))


# ------------------------------------------------------------------------------------------------ exact coefficient functions
def _ex(name):
    def f(x):
        with mpmath.workprec(_CPREC):
            x = mpmath.mpf(x)
            if x == 0:
                return {"A": mpmath.mpf(1), "B": mpmath.mpf(1) / 2, "C": mpmath.mpf(1) / 6, "D": mpmath.mpf(1) / 12, "E": -mpmath.mpf(1) / 24,
                        "F": -mpmath.mpf(1) / 120, "f": mpmath.mpf(1)}[name]
            s, c = mpmath.sin(x), mpmath.cos(x)
            if name == "A":
                return s / x
            if name == "B":
                return (1 - c) / x ** 2
            if name == "C":
                return (x - s) / x ** 3
            if name == "D":
                return 1 / x ** 2 - (1 + c) / (2 * x * s)
            if name == "E":
                return (1 - x ** 2 / 2 - c) / x ** 4
            if name == "F":
                return (x - s - x ** 3 / 6) / x ** 5
            return x / s
    return f


def _dex(name):
    f = _ex(name)

    def df(x):
        with mpmath.workprec(_CPREC):
            x = mpmath.mpf(x)
            h = mpmath.mpf(2) ** -80 * max(abs(x), mpmath.mpf(2) ** -40)
            return (f(x + h) - f(x - h)) / (2 * h) if x - h > 0 else (f(x + h) - f(x)) / h
    return df


def _lit(C_, num, den):
    """the double constant num / den of the source text: one rounding"""
    return _cdiv(C_.inp(np.full(C_.V, float(num))), C_.inp(np.full(C_.V, float(den))))


def _horner(C_, t, dens):
    """1 - t / d0 * (1 - t / d1 * ( ... (1 - t / dn)))"""
    d = lambda x: C_.inp(np.full(C_.V, float(x)))
    acc = sub(C_.one, _cdiv(t, d(dens[-1])))
    for den in reversed(dens[:-1]):
        acc = sub(C_.one, _mul(_cdiv(t, d(den)), acc))
    return acc


def _local(C_, name, p, taylor):
    """coefficient `name` along the branch's formula of pgo_coeffs / pgo_log, phi = p an exact input: Tr (formula value, M_loc, k_loc)"""
    d = lambda x: C_.inp(np.full(C_.V, float(x)))
    t = _mul(p, p)
    if name == "f":
        if taylor:
            return add(C_.one, _mul(_cdiv(t, d(6)), add(C_.one, _cdiv(_mul(d(7), t), d(60)))))
        return _cdiv(p, _sin(p))
    if taylor:
        if name == "A":
            return _horner(C_, t, (6, 20, 42, 72, 110))
        if name == "B":
            return sc(_horner(C_, t, (12, 30, 56, 90, 132)), 0.5)
        if name == "C":
            return _cdiv(_horner(C_, t, (20, 42, 72, 110, 156)), d(6))
        if name == "D":
            acc = _lit(C_, 1, 47900160)
            for den in (1209600, 30240, 720, 12):
                acc = add(_lit(C_, 1, den), _mul(t, acc))
            return acc
        if name == "E":
            return neg(_cdiv(_horner(C_, t, (30, 56, 90, 132, 182)), d(24)))
        return neg(_cdiv(_horner(C_, t, (42, 72, 110, 156, 210)), d(120)))
    s, c = _sin(p), _cos(p)
    if name == "A":
        return _cdiv(s, p)
    if name == "B":
        return _cdiv(sub(C_.one, c), t)
    if name == "C":
        return _cdiv(sub(p, s), _mul(t, p))
    if name == "D":
        return sub(_cdiv(C_.one, t), _cdiv(add(C_.one, c), _mul(sc(p, 2.0), s)))
    if name == "E":
        return _cdiv(sub(sub(C_.one, sc(t, 0.5)), c), _mul(t, t))
    return _cdiv(sub(sub(p, s), _cdiv(_mul(t, p), d(6))), _mul(_mul(t, t), p))


def coeff(C_, name, phi, taylor):
    """X(phi): the exact function's value, k = k_phi + k_loc + T_X, M = max(M_loc, |X'| M_phi) (module docstring)"""
    pin = Tr(phi.v, phi.v.absf(), 0)
    loc = _local(C_, name, pin, taylor)
    ex = _fn([phi], _ex(name), [_dex(name)], 0)                 # M = max(|y|, |X'| M_phi), k = k_phi
    return Tr(ex.v, np.maximum(loc.m, ex.m), phi.k + loc.k + (TRUNC[name] if taylor else 0))


def taylor_truncation():
    """T_X: |series(x) - X(x)| / (u M_loc), rounded up, at the top of the Taylor range (the remainders grow with x)"""
    out = {}
    for name in "ABCDEFf":
        x = 1e-4 if name == "f" else 0.2
        C_ = _Ctx(1, DD)
        loc = _local(C_, name, C_.inp(np.array([x])), True)
        with mpmath.workprec(_CPREC):
            v = mpmath.mpf(float(loc.v.hi[0])) + mpmath.mpf(float(loc.v.lo[0]))
            out[name] = int(mpmath.ceil(abs(v - _ex(name)(mpmath.mpf(x))) / (mpmath.mpf(U) * mpmath.mpf(float(loc.m[0])))))
    return out


def coeff_bars(phi):
    """for DESIGN.md: bar / |value| of every coefficient at the f64 angle phi taken as exact (k_loc u M_loc / |X|)"""
    C_ = _Ctx(1, DD)
    p = C_.inp(np.array([phi]))
    out = {}
    for name in "ABCDEF":
        t = coeff(C_, name, p, phi < 0.2)
        out[name] = float(t.k * U * t.m[0] / t.v.absf()[0])
    return out


# ------------------------------------------------------------------------------------------------ the chart, in the device's order
def _inv(C_, X):
    R, p = X
    Rt = [[R[c][r] for c in range(3)] for r in range(3)]
    return Rt, [neg(_dot(Rt[i], p)) for i in range(3)]


def _comp(C_, X, Y):
    R = _matmul(X[0], Y[0])
    return R, [add(_dot(X[0][i], Y[1]), X[1][i]) for i in range(3)]


def _eye_plus(C_, r, c, x):
    return add(C_.one, x) if r == c else x


def _log(C_, X, sig, who):
    """xi = [omega; v] of pgo_log, and |omega| as pgo_coeffs receives it"""
    R, p = X
    a = [sub(R[2][1], R[1][2]), sub(R[0][2], R[2][0]), sub(R[1][0], R[0][1])]
    s2 = _norm3(a)
    x = sc(sub(add(add(R[0][0], R[1][1]), R[2][2]), C_.one), 0.5)
    phi = _fn([sc(s2, 0.5), x], mpmath.atan2, [lambda y, x_: x_ / (x_ * x_ + y * y), lambda y, x_: y / (x_ * x_ + y * y)], LIBM_ULP)
    C_.note(who + " pgo_log phi", "lt", phi, 1e-4)
    f = coeff(C_, "f", phi, sig["log_series"])
    w = [sc(_mul(f, ai), 0.5) for ai in a]
    W = _hat(w)
    WW = _matmul(W, W)
    nw = _norm3(w)
    C_.note(who + " pgo_coeffs phi", "lt", nw, 0.2)
    D = coeff(C_, "D", nw, sig["taylor"])
    v = []
    for i in range(3):
        s = ZERO
        for j in range(3):
            s = add(s, _mul(add(sub(C_.one if i == j else ZERO, sc(W[i][j], 0.5)), _mul(D, WW[i][j])), p[j]))
        v.append(s)
    return w + v, nw


def _jrinv(C_, xi, nw, sig, tooth=None):
    W, V = _hat(xi[:3]), _hat(xi[3:])
    k = {n: coeff(C_, n, nw, sig["taylor"]) for n in "CDEF"}
    WW, WV, VW = _matmul(W, W), _matmul(W, V), _matmul(V, W)
    WVW = _matmul(WV, W)
    WWV, VWW, WVWW, WWVW = _matmul(W, WV), _matmul(VW, W), _matmul(WVW, W), _matmul(W, WVW)
    three = C_.inp(np.full(C_.V, 3.0))
    e3f = sc(sub(k["E"], _mul(three, k["F"])), 0.5)
    Q = [[None] * 3 for _ in range(3)]
    Ji = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            q = neg(sc(V[r][c], 0.5))
            q = add(q, _mul(k["C"], sub(add(WV[r][c], VW[r][c]), WVW[r][c])))
            q = add(q, _mul(k["E"], sub(add(WWV[r][c], VWW[r][c]), _mul(three, WVW[r][c]))))
            Q[r][c] = sub(q, _mul(e3f, add(WVWW[r][c], WWVW[r][c])))
            Ji[r][c] = add(_eye_plus(C_, r, c, sc(W[r][c], 0.5)), _mul(k["D"], WW[r][c]))
    T2 = _matmul(_matmul(Ji, Q), Ji)
    J = [[ZERO] * 6 for _ in range(6)]
    for r in range(3):
        for c in range(3):
            J[r][c] = Ji[r][c]; J[3 + r][c] = neg(T2[r][c]); J[3 + r][3 + c] = Ji[r][c]
    return J


def factor_terms(Xi, Xj, Z, lam, sig):
    """the slot entries (list of 121 Tr over the V factors given, all of signature sig), e, Jj, Ji and the branch notes"""
    V = len(Z)
    C_ = _Ctx(V, DD)
    pose = lambda a: ([[C_.inp(a[:, 3 * r + c]) for c in range(3)] for r in range(3)], [C_.inp(a[:, 9 + k]) for k in range(3)])
    z, xi_ = pose(Z), pose(Xi)
    L = [C_.inp(lam[:, q]) for q in range(6)]
    Zi = _inv(C_, z)
    if sig["between"]:
        xj_ = pose(Xj)
        B = _comp(C_, Zi, _comp(C_, _inv(C_, xi_), xj_))
        e, nw = _log(C_, B, sig, "between")
        Jj = _jrinv(C_, e, nw, sig)
        A = _comp(C_, _inv(C_, xj_), xi_)
        PR = _matmul(_hat(A[1]), A[0])
        Ad = [[ZERO] * 6 for _ in range(6)]
        for r in range(3):
            for c in range(3):
                Ad[r][c] = A[0][r][c]; Ad[3 + r][c] = PR[r][c]; Ad[3 + r][3 + c] = A[0][r][c]
        Ji = [[neg(x) for x in row] for row in _matmul(Jj, Ad)]
    else:
        B = _comp(C_, Zi, xi_)
        e, nw = _log(C_, B, sig, "prior")
        Ji = _jrinv(C_, e, nw, sig)
        Jj = [[ZERO] * 6 for _ in range(6)]
    slot = [ZERO] * 121
    c = ZERO
    for q in range(6):
        c = add(c, _mul(_mul(e[q], e[q]), L[q]))
    slot[120] = sc(c, 0.5)
    for a in range(6):
        gi, gj = ZERO, ZERO
        for q in range(6):
            gi = add(gi, _mul(_mul(Ji[q][a], L[q]), e[q]))
            gj = add(gj, _mul(_mul(Jj[q][a], L[q]), e[q]))
        slot[108 + a], slot[114 + a] = gi, gj
        for b in range(6):
            hii, hjj, hij = ZERO, ZERO, ZERO
            for q in range(6):
                li = _mul(L[q], Ji[q][a])
                hii = add(hii, _mul(li, Ji[q][b]))
                hij = add(hij, _mul(li, Jj[q][b]))
                hjj = add(hjj, _mul(_mul(L[q], Jj[q][a]), Jj[q][b]))
            slot[6 * a + b], slot[36 + 6 * a + b], slot[72 + 6 * a + b] = hii, hjj, hij
    return slot, e, Jj, Ji, C_.branch


# ------------------------------------------------------------------------------------------------ the reference of a factor list
def signature(Xi, Xj, Z, between):
    """the branches the f64 chart (pgo_oracle, the device's transcription source) takes on this factor"""
    B = po.compose(po.inverse(Z), po.compose(po.inverse(Xi), Xj)) if between else po.compose(po.inverse(Z), Xi)
    R = B[:9].reshape(3, 3)
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    phi = np.arctan2(0.5 * np.linalg.norm(a), 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))
    w = po.so3_log(R)
    return (bool(between), bool(phi < 1e-4), bool(np.linalg.norm(w) < 0.2))


class Ref:
    """slots of the factors of one call: poses [n][12], edges [m][20], priors [k][19] (the arrays handed to the library)"""

    def __init__(self, poses, edges, priors):
        poses = np.asarray(poses, np.float64).reshape(-1, 12)
        edges = np.asarray(edges, np.float64).reshape(-1, 20); priors = np.asarray(priors, np.float64).reshape(-1, 19)
        m, F = len(edges), len(edges) + len(priors)
        fi = np.concatenate([edges[:, 0], priors[:, 0]]).astype(int)
        fj = np.concatenate([edges[:, 1], -np.ones(len(priors))]).astype(int)
        Z = np.concatenate([edges[:, 2:14], priors[:, 1:13]])
        lam = 1.0 / np.concatenate([edges[:, 14:20], priors[:, 13:19]])          # fl(1 / var), as the host plan forms it
        self.F, self.fi, self.fj = F, fi, fj
        self.sigs = [signature(poses[fi[f]], poses[fj[f]] if fj[f] >= 0 else None, Z[f], fj[f] >= 0) for f in range(F)]
        self.hi = np.zeros((F, 121)); self.lo = np.zeros((F, 121)); self.m = np.zeros((F, 121)); self.k = np.zeros((F, 121), dtype=np.int64)
        self.ke = np.zeros((F, 6), dtype=np.int64); self.kJ = np.zeros(F, dtype=np.int64)
        self.e = np.zeros((F, 6)); self.Jj = np.zeros((F, 6, 6)); self.Ji = np.zeros((F, 6, 6))
        self.Jjm = np.zeros((F, 6, 6)); self.Jjk = np.zeros((F, 6, 6), dtype=np.int64)
        self.branch = []
        for sg in sorted(set(self.sigs)):
            idx = np.flatnonzero([s == sg for s in self.sigs])
            sig = dict(between=sg[0], log_series=sg[1], taylor=sg[2])
            slot, e, Jj, Ji, br = factor_terms(poses[fi[idx]], poses[np.maximum(fj[idx], 0)], Z[idx], lam[idx], sig)
            for q, t in enumerate(slot):
                if t.v is not None:
                    self.hi[idx, q] = t.v.hi; self.lo[idx, q] = t.v.lo; self.m[idx, q] = t.m; self.k[idx, q] = t.k
            for q in range(6):
                if e[q].v is not None:
                    self.e[idx, q] = e[q].v.f64(); self.ke[idx, q] = e[q].k
            kj = 0
            for r in range(6):
                for c in range(6):
                    for M_, dst in ((Jj, self.Jj), (Ji, self.Ji)):
                        if M_[r][c].v is not None:
                            dst[idx, r, c] = M_[r][c].v.f64(); kj = max(kj, M_[r][c].k)
                    if Jj[r][c].v is not None:
                        self.Jjm[idx, r, c] = Jj[r][c].m; self.Jjk[idx, r, c] = Jj[r][c].k
            self.kJ[idx] = kj
            for name, kind, val, thr in br:
                x = val.v.f64()
                for i_, f in enumerate(idx):
                    self.branch.append((int(f), name, kind, float(x[i_]), float(val.k * U * val.m[i_]), thr))

    def value(self):
        return self.hi + self.lo

    def err(self, slot):
        return DD(self.hi, self.lo).err_to(slot)

    def bar(self):
        return self.k * U * self.m

    def check(self, slot):
        """(worst ratio err / bar per factor [F], list of violations (f, entry, value, reference, err, bar)).  M = 0: exactly 0."""
        slot = np.asarray(slot, np.float64).reshape(self.F, 121)
        err, bar = self.err(slot), self.bar()
        zero = self.m == 0.0
        ratio = np.where(zero, np.where(slot == 0.0, 0.0, np.inf), err / np.where(zero, 1.0, bar))
        bad = [(int(f), int(q), float(slot[f, q]), float(self.value()[f, q]), float(err[f, q]), float(bar[f, q]))
               for f, q in zip(*np.nonzero(~(ratio <= 1.0)))]
        return ratio.max(axis=1), bad

    def counts(self):
        out = {}
        for name, tay in (("taylor", True), ("closed", False)):
            ix = np.flatnonzero([s[2] == tay for s in self.sigs])
            if len(ix):
                out[name] = dict(e=int(self.ke[ix].max()), J=int(self.kJ[ix].max()), H=int(self.k[ix, :108].max()),
                                 g=int(self.k[ix, 108:120].max()), c=int(self.k[ix, 120].max()))
        return out

    def margins(self):
        """violations of imu_ref's corpus condition: every branch variable strictly outside thr (1 -+ MARGIN), its own bar below 1e-3 of
        its distance to the threshold"""
        return [(f, name, x, bar, thr) for f, name, kind, x, bar, thr in self.branch
                if (thr * (1 - MARGIN) <= x <= thr * (1 + MARGIN)) or not bar < 1e-3 * abs(x - thr)]

    def branch_consistent(self):
        bad = []
        for f, name, kind, x, bar, thr in self.branch:
            want = self.sigs[f][1] if name.endswith("pgo_log phi") else self.sigs[f][2]
            if want != (x < thr):
                bad.append((f, name, x, self.sigs[f]))
        return bad


# ------------------------------------------------------------------------------------------------ corpora
def _perm(rng):
    P = np.zeros((3, 3))
    P[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
    if np.linalg.det(P) < 0:
        P[0] = -P[0]
    return P


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def lin_classes(f):
    return f % len(ANGLES), (f // len(ANGLES)) % len(TRANS)


def lin_corpus(seed=20261020):
    """(poses [200][12], edges [200][20], priors [100][19]) of the module docstring"""
    rng = np.random.default_rng(seed)
    G = 100
    poses = np.zeros((2 * G, 12)); edges = np.zeros((2 * G, 20)); priors = np.zeros((G, 19))
    for g in range(G):
        fs = (2 * g, 2 * g + 1, 2 * G + g)
        cls = [lin_classes(f) for f in fs]
        exact = any(a == 0 for a, _ in cls)
        origin = (not exact) and any(t == 0 for _, t in cls)
        for k in (2 * g, 2 * g + 1):
            if exact:
                poses[k, :9] = _perm(rng).ravel(); poses[k, 9:] = rng.integers(-4096, 4097, 3) / 4.0
            else:
                poses[k, :9] = po.rand_rot(rng).ravel()
                poses[k, 9:] = 0.0 if origin else _unit(rng) * 10.0 ** rng.uniform(0, 3)
        if exact:                                         # a zero residual translation needs equal positions in a between factor
            poses[2 * g + 1, 9:] = poses[2 * g, 9:]

        def resid(a, t):
            if a == 0:
                R = np.eye(3)
            else:
                R = po.so3_exp(_unit(rng) * ANGLES[a])
            p = np.zeros(3) if t == 0 else (np.array([0.125, 0, 0]) * [1, 80, 8000][t - 1] if a == 0 and exact else _unit(rng) * TRANS[t])
            return np.concatenate([R.ravel(), p])

        for e_, f in enumerate(fs[:2]):
            fwd = (g % 2 == 0) if e_ == 0 else ((g % 2 == 0) ^ (g % 4 < 2))
            i, j = (2 * g, 2 * g + 1) if fwd else (2 * g + 1, 2 * g)
            E = resid(*cls[e_])
            Zp = po.compose(po.compose(po.inverse(poses[i]), poses[j]), po.inverse(E))
            edges[f] = np.concatenate([[i, j], Zp, 10.0 ** rng.uniform(-9, -2, 6)])
        E = resid(*cls[2])
        priors[g] = np.concatenate([[2 * g], po.compose(poses[2 * g], po.inverse(E)), 10.0 ** rng.uniform(-9, -2, 6)])
    return poses, edges, priors


_LIN = {}


def lin_ref():
    """(inputs, Ref) of the linearisation corpus, evaluated once per process"""
    if "r" not in _LIN:
        inp = lin_corpus()
        _LIN["r"] = (inp, Ref(*inp))
    return _LIN["r"]


# ---- solve graphs: the smallest that reach each path of the plan and of the elimination
def _graph(rng, n, pairs, prior_nodes, noise=1e-2):
    X = np.array([np.concatenate([po.rand_rot(rng).ravel(), rng.normal(0, 3, 3)]) for _ in range(n)])
    Y = np.array([po.retract(x, np.concatenate([rng.normal(0, noise, 3), rng.normal(0, 3 * noise, 3)])) for x in X])
    ed = [po.edge_row(i, j, X[i], X[j], 10.0 ** rng.uniform(-5, -2, 6)) for i, j in pairs]
    pr = [po.prior_row(k, X[k], 10.0 ** rng.uniform(-6, -3, 6)) for k in prior_nodes]
    return Y, np.array(ed).reshape(-1, 20), np.array(pr).reshape(-1, 19)


def solve_graphs(seed=20261021):
    """name -> (poses, edges, priors)"""
    rng = np.random.default_rng(seed)
    chain = lambda n: [(k, k + 1) for k in range(n - 1)]
    out = {}
    for n in (2, 3, 9):
        out["chain%d" % n] = _graph(rng, n, chain(n), [0])
    for L in (1, 2, 7):                                   # keyframes 0 and L + 1 (priors), L path nodes between them, orientations mixed
        out["seg%d" % L] = _graph(rng, L + 2, [(k, k + 1) if k % 2 == 0 else (k + 1, k) for k in range(L + 1)], [0, L + 1])
    out["cycle3"] = _graph(rng, 4, [(0, 1), (2, 1), (2, 3), (3, 0)], [0])
    out["tail_branch"] = _graph(rng, 9, [(0, 1), (1, 2), (2, 3), (3, 4), (2, 5), (6, 5), (2, 7), (7, 8)], [0])
    out["two_comp"] = _graph(rng, 7, [(0, 1), (1, 2), (2, 3), (4, 5), (6, 5)], [0, 5])
    out["parallel"] = _graph(rng, 4, [(0, 1), (1, 0), (0, 1), (1, 2), (3, 2), (2, 3)], [0])
    for K in (1, 3, 11, 12):
        out["skel%d" % K] = _graph(rng, K, chain(K), list(range(K)))
    out["hub65"] = _graph(rng, 66, [(0, k) if k % 2 else (k, 0) for k in range(1, 66)], [0])
    return out


def dense_system(blk, g, pairs, n):
    """(H, -g): the full 6n system of the assembled blocks (blk[n + p] = H(lo, hi), rows = the lower node id)"""
    H = np.zeros((6 * n, 6 * n))
    for k in range(n):
        H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = blk[k].reshape(6, 6)
    for p, (a, b) in enumerate(pairs):
        M_ = blk[n + p].reshape(6, 6)
        H[6 * a:6 * a + 6, 6 * b:6 * b + 6] = M_; H[6 * b:6 * b + 6, 6 * a:6 * a + 6] = M_.T
    return H, -np.asarray(g, np.float64).reshape(-1)


def replay_cost(slot):
    """k_pgo_cost's order over slot[:, 120]: 256 strided sums, then the 128 .. 1 tree; additions only"""
    c = np.asarray(slot, np.float64)[:, 120]
    red = np.zeros(256)
    for t in range(256):
        acc = 0.0
        for f in range(t, len(c), 256):
            acc = acc + c[f]
        red[t] = acc
    w = 128
    while w > 0:
        red[:w] = red[:w] + red[w:2 * w]
        w >>= 1
    return float(red[0])


def replay_assemble(slot, fi, fj, n, tooth=None):
    """(pairs [P][2], blk [n + P][36], g [n][6]): k_pgo_assemble's in-order sums of the slots (factor order; part 3 transposed; rows =
    the lower node id).  tooth 'part3': the reversed edge added untransposed."""
    slot = np.asarray(slot, np.float64)
    pairs = sorted({(min(i, j), max(i, j)) for i, j in zip(fi, fj) if j >= 0})
    pid = {p: k for k, p in enumerate(pairs)}
    blk = np.zeros((n + len(pairs), 36)); g = np.zeros((n, 6))
    for f, (i, j) in enumerate(zip(fi, fj)):
        blk[i] = blk[i] + slot[f, :36]; g[i] = g[i] + slot[f, 108:114]
        if j >= 0:
            blk[j] = blk[j] + slot[f, 36:72]; g[j] = g[j] + slot[f, 114:120]
            b = n + pid[(min(i, j), max(i, j))]
            Hij = slot[f, 72:108]
            blk[b] = blk[b] + (Hij if i < j or tooth == "part3" else Hij.reshape(6, 6).T.ravel())
    return np.array(pairs, dtype=np.int32).reshape(-1, 2), blk, g


# ------------------------------------------------------------------------------------------------ numpy models (for the teeth)
def model_slot(Xi, Xj, Z, lam, tooth=None):
    """one factor's slot [121] in plain f64 by the formulas of pgo_oracle (Xj None: a prior), with one of the defects of
    tests/test_pgo_ref_cpu.py"""
    def coeffs(phi):
        if tooth == "taylor_at_2":
            t = phi * phi
            k = list(po._coeffs(0.1))
            k[0] = 1 - t / 6 * (1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110))))
            k[1] = 0.5 * (1 - t / 12 * (1 - t / 30 * (1 - t / 56 * (1 - t / 90 * (1 - t / 132)))))
            k[2] = (1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110 * (1 - t / 156))))) / 6
            k[3] = 1 / 12 + t * (1 / 720 + t * (1 / 30240 + t * (1 / 1209600 + t * (1 / 47900160))))
            k[4] = -(1 - t / 30 * (1 - t / 56 * (1 - t / 90 * (1 - t / 132 * (1 - t / 182))))) / 24
            k[5] = -(1 - t / 42 * (1 - t / 72 * (1 - t / 110 * (1 - t / 156 * (1 - t / 210))))) / 120
            return k
        k = list(po._coeffs(phi))
        if phi >= 0.2:
            if tooth == "E_1.01":
                k[4] *= 1.01
            if tooth == "F_sign":
                k[5] = -k[5]
            if tooth == "D_1mc":
                k[3] = 1 / (phi * phi) - (1 - np.cos(phi)) / (2 * phi * np.sin(phi))
        return k

    def log6(X):
        w = po.so3_log(X[:9].reshape(3, 3)); W = po.hat(w)
        return np.concatenate([w, (np.eye(3) - 0.5 * W + coeffs(np.linalg.norm(w))[3] * (W @ W)) @ X[9:12]])

    def jr_inv(xi):
        W, V = po.hat(xi[:3]), po.hat(xi[3:])
        _, _, C_, D, E, F = coeffs(np.linalg.norm(xi[:3]))
        WW = W @ W
        Ji = np.eye(3) + 0.5 * W + D * WW
        WV, VW, WVW = W @ V, V @ W, W @ V @ W
        Q = -0.5 * V + C_ * (WV + VW - WVW) + E * (W @ WV + VW @ W - 3 * WVW) - 0.5 * (E - 3 * F) * (WVW @ W + W @ WVW)
        out = np.zeros((6, 6))
        out[:3, :3] = Ji; out[3:, 3:] = Ji; out[3:, :3] = -Ji @ Q @ Ji
        return out

    if Xj is not None:
        e = log6(po.compose(po.inverse(Z), po.compose(po.inverse(Xi), Xj)))
        Jj = jr_inv(e)
        Ad = po.adjoint(po.compose(po.inverse(Xj), Xi))
        if tooth == "Ad_T":
            Ad[3:, :3] = Ad[3:, :3].T.copy()
        Ji = Jj @ Ad if tooth == "Ji_plus" else -Jj @ Ad
    else:
        e = log6(po.compose(po.inverse(Z), Xi))
        Ji = jr_inv(e); Jj = np.zeros((6, 6))
    L = lambda J: (J * lam[None, :]) if tooth == "lam_col" else (lam[:, None] * J)
    s = np.zeros(121)
    s[:36] = (Ji.T @ L(Ji)).ravel(); s[36:72] = (Jj.T @ L(Jj)).ravel(); s[72:108] = (Ji.T @ L(Jj)).ravel()
    s[108:114] = L(Ji).T @ e if tooth == "lam_col" else Ji.T @ (lam * e)
    s[114:120] = L(Jj).T @ e if tooth == "lam_col" else Jj.T @ (lam * e)
    s[120] = 0.5 * np.sum(e * e * lam)
    return s


def model_solve(blk, g, plan, n, tooth=None):
    """dx [n][6]: the segment elimination, skeleton system and back-substitution of vba_pgo_math.hpp over the plan's tables in plain
    f64 (6x6 and skeleton solves by numpy), with one of the defects of tests/test_pgo_ref_cpu.py"""
    blk = np.asarray(blk, np.float64); g = np.asarray(g, np.float64).reshape(n, 6)

    def load(code):
        if code < 0:
            return np.zeros((6, 6))
        M_ = blk[code >> 1].reshape(6, 6)
        return M_.T.copy() if code & 1 else M_.copy()

    so, att = plan["seg_off"], plan["seg_att"]
    S, K = len(so) - 1, len(plan["skel_node"])
    segout, Ys = [], {}
    for s in range(S):
        Dup = np.zeros((6, 6)); bup = np.zeros(6); SAA = np.zeros((6, 6)); bA = np.zeros(6)
        E = load(plan["seg_ecode"][s])
        for o in range(so[s], so[s + 1]):
            node = plan["seg_nodes"][o]
            D = blk[node].reshape(6, 6) - (0.0 if tooth == "dup_skip" and o == so[s] + 1 else Dup)
            Cm = load(plan["seg_ccode"][o])
            Y = np.linalg.solve(D, np.concatenate([Cm, E, (-g[node] - bup)[:, None]], axis=1))
            Ys[o] = Y
            if att[2 * s] >= 0:
                SAA = SAA + E.T @ Y[:, 6:12]
                if tooth != "bA_drop":
                    bA = bA + E.T @ Y[:, 12]
            Dup = Cm.T @ Y[:, :6]; nE = Cm.T @ Y[:, 6:12]; bup = Cm.T @ Y[:, 12]
            E = -nE if (o + 1 < so[s + 1] and tooth != "sign_all") else nE
        segout.append((SAA, Dup, E.T.copy() if tooth == "sba_T" else E, bA, bup))
    A = np.zeros((6 * K, 6 * K)); rhs = np.zeros(6 * K)
    for b in range(len(plan["sb_base"])):
        p, q = plan["sb_pq"][2 * b], plan["sb_pq"][2 * b + 1]
        h = load(plan["sb_base"][b])
        r = -g[plan["skel_node"][p]].copy()
        for e_ in range(plan["sb_off"][b], plan["sb_off"][b + 1]):
            s, part = plan["sb_ent"][e_] >> 2, plan["sb_ent"][e_] & 3
            h = h - (segout[s][2].T if part == 3 else segout[s][part])
            if part < 2 and p == q:
                r = r - segout[s][3 + part]
        A[6 * p:6 * p + 6, 6 * q:6 * q + 6] = h
        if p != q:
            A[6 * q:6 * q + 6, 6 * p:6 * p + 6] = h.T
        else:
            rhs[6 * p:6 * p + 6] = r
    A = np.tril(A) + np.tril(A, -1).T                                          # the factorisation reads the lower triangle
    z = np.linalg.solve(A, rhs)
    dx = np.zeros((n, 6))
    for p in range(K):
        dx[plan["skel_node"][p]] = z[6 * p:6 * p + 6]
    for s in range(S):
        xa = z[6 * att[2 * s]:6 * att[2 * s] + 6] if att[2 * s] >= 0 else np.zeros(6)
        xn = z[6 * att[2 * s + 1]:6 * att[2 * s + 1] + 6]
        if tooth == "xa_xn":
            xa, xn = xn, xa
        for o in range(so[s + 1] - 1, so[s] - 1, -1):
            Y = Ys[o]
            x = Y[:, 12] - Y[:, :6] @ xn - Y[:, 6:12] @ xa
            xn = x
            dx[plan["seg_nodes"][o]] = x
    return dx


def solve_ratios(blk, g, pairs, n, dx):
    """solve_ref's (backward ratio, forward ratio, zero rows ok) of dx against the full system (H, -g) of the blocks given"""
    import solve_ref as sr
    H, b = dense_system(blk, g, pairs, n)
    return sr.ratios(H, b, np.asarray(dx, np.float64).reshape(-1))


# ------------------------------------------------------------------------------------------------ retraction: theta (+) Exp(dx)
def retract_ref(theta, dx):
    """(value [12], bar [12]) of pgo_retract on one node: X Exp(d) with the exact coefficient functions"""
    theta = np.asarray(theta, np.float64).reshape(1, 12); dx = np.asarray(dx, np.float64).reshape(1, 6)
    C_ = _Ctx(1, DD)
    xi = [C_.inp(dx[:, q]) for q in range(6)]
    X = ([[C_.inp(theta[:, 3 * r + c]) for c in range(3)] for r in range(3)], [C_.inp(theta[:, 9 + k]) for k in range(3)])
    W = _hat(xi[:3]); WW = _matmul(W, W)
    nw = _norm3(xi[:3])
    tay = bool(nw.v.f64()[0] < 0.2)
    k = {n_: coeff(C_, n_, nw, tay) for n_ in "ABC"}
    R = [[add(_eye_plus(C_, r, c, _mul(k["A"], W[r][c])), _mul(k["B"], WW[r][c])) for c in range(3)] for r in range(3)]
    Vm = [[add(_eye_plus(C_, r, c, _mul(k["B"], W[r][c])), _mul(k["C"], WW[r][c])) for c in range(3)] for r in range(3)]
    E = (R, [_dot(Vm[i], xi[3:]) for i in range(3)])
    Y = _comp(C_, X, E)
    flat = [Y[0][r][c] for r in range(3) for c in range(3)] + Y[1]
    val = np.array([t.v.f64()[0] for t in flat]); bar = np.array([t.k * U * t.m[0] for t in flat])
    lo = np.array([t.v.lo[0] for t in flat]); hi = np.array([t.v.hi[0] for t in flat])
    return DD(hi, lo), bar, max(t.k for t in flat), tay


# ------------------------------------------------------------------------------------------------ the g++ build
_LIB = None


def host_lib():
    """tests/host/pgo_host.cpp built by g++ -O2 -ffp-contract=off over csrc/vba_pgo_math.hpp and csrc/vba_pgo_plan.hpp (once per process)"""
    global _LIB
    if _LIB is None:
        import subprocess
        import tempfile
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = os.path.join(tempfile.mkdtemp(prefix="pgo_host_"), "libpgo_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(root, "tests", "host", "pgo_host.cpp"),
                               "-o", out])
        _LIB = C.CDLL(out)
        _LIB.pgo_host_step.restype = C.c_int
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_step(poses, edges, priors, extra=False):
    """vba_debug_pgo_step's outputs by the g++ build (plain LDL^T on the skeleton); extra: also segY, segout, Ab and the plan tables"""
    lib = host_lib()
    x = np.ascontiguousarray(poses, np.float64).reshape(-1, 12); n = len(x)
    e = np.ascontiguousarray(edges, np.float64).reshape(-1, 20); m = len(e)
    pr = np.ascontiguousarray(priors, np.float64).reshape(-1, 19)
    slot = np.full((m + len(pr), 121), np.nan); npairs = C.c_int(-1); pairs = np.full((max(m, 1), 2), -1, dtype=np.int32)
    blk = np.full((n + m, 36), np.nan); g = np.full((n, 6), np.nan); dx = np.full((n, 6), np.nan); cost = C.c_double(np.nan)
    out = np.full((n, 12), np.nan)
    segY = np.zeros((n, 78)); segout = np.zeros((n, 120)); Ab = np.zeros((6 * n + 9) * (6 * n + 72))
    st = lib.pgo_host_step(n, _p(x), m, _p(e), len(pr), _p(pr), _p(slot), C.byref(npairs), _p(pairs), _p(blk), _p(g), _p(dx), C.byref(cost),
                           _p(out), _p(segY), _p(segout), _p(Ab))
    if st != 0:
        raise RuntimeError("pgo_host_step: %d" % st)
    P = npairs.value
    r = dict(slot=slot, pairs=pairs[:P].copy(), blk=blk[:n + P].copy(), g=g, dx=dx, cost=cost.value, poses=out)
    if extra:
        tabs = []
        for w in range(13):
            L = lib.pgo_host_plan_vec(w, None)
            a = np.zeros(max(L, 1), dtype=np.int32)
            lib.pgo_host_plan_vec(w, _p(a))
            tabs.append(a[:L])
        names = ("seg_off", "seg_nodes", "seg_att", "seg_ecode", "seg_ccode", "skel_node", "sb_pq", "sb_base", "sb_off", "sb_ent", "blk_off",
                 "blk_ent", "dims")
        r.update(segY=segY, segout=segout, Ab=Ab, plan=dict(zip(names, tabs)))
    return r


def host_chart(name, x):
    lib = host_lib()
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros({"exp": 12, "log": 6, "jrinv": 36}[name])
    getattr(lib, "pgo_host_" + name)(_p(x), _p(out))
    return out


def host_coeffs(phi):
    lib = host_lib()
    lib.pgo_host_coeffs.argtypes = [C.c_double, C.c_void_p]
    out = np.zeros(6)
    lib.pgo_host_coeffs(float(phi), _p(out))
    return out


# ------------------------------------------------------------------------------------------------ sub-calls and retraction graphs
def lin_subcall(inp, F):
    """A call of F in (1, 255, 256, 257) factors whose factors are factors of the corpus, in its order: the first 85 pairs whole (255),
    then pair 85's prior (256) and its first edge (257); F = 1: pair 0's prior on its own.  (A literal prefix of the factor list holds
    edges only, or pairs without their prior: the plan refuses it as singular before anything is launched.)
    Returns (poses, edges, priors, idx) with idx[f'] the corpus factor that factor f' of the call is."""
    poses, edges, priors = inp
    m = len(edges)
    if F == 1:
        return poses[:1], edges[:0], priors[:1], np.array([m])
    G = 85
    ne = 2 * G + (1 if F == 257 else 0)
    npr = G + (1 if F >= 256 else 0)
    n = 2 * G + (0 if F == 255 else 1 if F == 256 else 2)
    assert ne + npr == F
    return poses[:n], edges[:ne], priors[:npr], np.concatenate([np.arange(ne), m + np.arange(npr)])


RETRACT_ANGLES = (0.5, 2.0, 3.0)
K_RETRACT = 23


def retract_graphs(seed=20261022):
    """n = 1 graphs whose prior lies RETRACT_ANGLES away, so that the step's rotation takes pgo_exp's closed-form branch"""
    rng = np.random.default_rng(seed)
    out = []
    for a in RETRACT_ANGLES:
        X = np.concatenate([po.rand_rot(rng).ravel(), rng.normal(0, 5, 3)])
        P = po.retract(X, np.concatenate([_unit(rng) * a, rng.normal(0, 1, 3)]))
        out.append((X.reshape(1, 12), np.zeros((0, 20)), po.prior_row(0, P, 10.0 ** rng.uniform(-6, -3, 6)).reshape(1, 19)))
    return out
