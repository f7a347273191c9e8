"""CPU-side checks of the surfel export of the global map (vba_kf_surfel_export): the new prototypes, the
restatement tests/surfel_ref.py against a 60-digit reference of the covariance and against mutations of itself, the one-pass
raw-moment form that must fail at 1000 m, the scene's own conditions, and tests/host/export_surfel_host.cpp: the fit header built by
g++ on the restated moments, and the adapter's message cuts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eig3_ref as er
import export_voxel_ref as ev
import surfel_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXELS = (0.5, 1.0)


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.fixture(scope="module")
def host(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("export_surfel")
    return sr.build_host(d, capi.LIB_PATH), d


@pytest.fixture(scope="module")
def scenes():
    """name -> (sessions, S, keyframe of every record, moments and exact reference per voxel size)"""
    clouds, poses = sr.scene()
    out = {}
    for name, P in (("near", poses), ("far", sr.shifted(poses))):
        sessions = [(clouds, P, 2.0)]
        S, kf = ev.sequence(sessions, 1)
        per = {}
        for voxel in VOXELS:
            mo = sr.moments(S, voxel)
            mean, cov, D, A = sr.exact(S, mo["first"], mo["cnt"], mo["vox"])
            per[voxel] = dict(mo=mo, mean=mean, cov=cov, D=D, A=A, bar=sr.cov_bar(mo["cnt"], D, A))
        out[name] = dict(sessions=sessions, S=S, kf=kf, per=per)
    return out


def test_new_prototypes(capi):
    from voxel_slam_amd import abi
    want = {"vba_kf_surfel_export_reserve": "i:pqq", "vba_kf_surfel_export_allocations": "i:ppp", "vba_kf_surfel_export": "i:pippidiqpppp"}
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    lib = capi.load()
    for name, proto in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert abi.PROTOTYPES.get(name) == proto and name in capi.EXPORTS and hasattr(lib, name), name
    names = list(abi.PROTOTYPES)
    assert names[names.index("vba_kf_voxel_export") + 1:][:3] == list(want)
    for m in ("kf_export_surfel", "kf_export_surfel_size", "kf_export_surfel_reserve", "kf_export_surfel_allocations"):
        assert hasattr(capi.Context, m), m
    assert "pub_globalmap_surfel" in open(os.path.join(ROOT, "include", "voxelba_adapter.hpp")).read()
    # without a context every call is refused before it touches a device, outputs untouched
    n = C.c_int64(-77); a = C.c_int(-77); b = C.c_int64(-77)
    assert lib.vba_kf_surfel_export(None, 1, None, None, 1, 0.5, 1, 0, None, None, None, C.byref(n)) == capi.ERR_BAD_ARG and n.value == -77
    assert lib.vba_kf_surfel_export_reserve(None, 100, 10) == capi.ERR_BAD_ARG
    assert lib.vba_kf_surfel_export_allocations(None, C.byref(a), C.byref(b)) == capi.ERR_BAD_ARG and (a.value, b.value) == (-77, -77)


# ---------------------------------------------------------------- the scene
def test_scene_holds_what_the_tests_need(scenes):
    clouds, poses = sr.scene()
    assert sum(len(c) for c in clouds) <= 6000 and len(clouds) == sr.N_KF
    assert all(len(np.unique(np.round(c / sr.GRID).astype(np.int64), axis=0)) == len(c) for c in clouds)     # alone in a build voxel
    for name in ("near", "far"):
        sc = scenes[name]
        S, kf = sc["S"], sc["kf"]
        assert (S[:, :3] < 0).any() and (S[:, :3] > 0).any()                  # negative coordinates
        if name == "far":
            assert np.abs(S[:, :3]).min(axis=0).min() > 900.0
        for voxel in VOXELS:
            mo = sc["per"][voxel]["mo"]
            cnt, vox, first = mo["cnt"], mo["vox"], mo["first"]
            lo = np.full(len(cnt), 1 << 40); hi = np.full(len(cnt), -1)
            np.minimum.at(lo, vox, kf); np.maximum.at(hi, vox, kf)
            rlo = np.full(len(cnt), 1 << 40); rhi = np.full(len(cnt), -1)
            np.minimum.at(rlo, vox, np.arange(len(S))); np.maximum.at(rhi, vox, np.arange(len(S)))
            print("%s voxel %g: %d records, %d voxels, counts 1/2/>=3: %d/%d/%d, largest %d, %d span keyframes, %d span a 256-record boundary"
                  % (name, voxel, len(S), len(cnt), (cnt == 1).sum(), (cnt == 2).sum(), (cnt >= 3).sum(), cnt.max(), (hi > lo).sum(),
                     (rhi // 256 > rlo // 256).sum()))
            assert (cnt == 1).sum() >= 5 and (cnt == 2).sum() >= 5 and cnt.max() > 256
            assert (hi > lo).sum() >= 20 and (rhi // 256 > rlo // 256).sum() >= 20
        # the exactly collinear triples: the exact covariance has rank one; the pole: two small eigenvalues
        per = sc["per"][0.5]
        tri = np.flatnonzero((per["mo"]["cnt"] == 3) & (per["mo"]["first"] < 18))
        assert len(tri) == 6
        for v in tri:
            w = np.linalg.eigvalsh(sr.sym(per["cov"][v]))
            assert w[2] > 1e-4 and abs(w[1]) <= 1e-15 * w[2] and abs(w[0]) <= 1e-15 * w[2]
        # and the restated covariance of a triple is that of the exact one: every operation on these dyadic numbers is exact
        # up to the division by 3
        assert np.abs(per["mo"]["C"][tri] - per["cov"][tri]).max() <= 4 * sr.U * np.abs(per["cov"][tri]).max()


# ---------------------------------------------------------------- the restatement against the exact covariance
@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", VOXELS)
def test_restatement_meets_the_derived_bar(scenes, name, voxel):
    per = scenes[name]["per"][voxel]
    mo = per["mo"]
    rc = np.abs(mo["c"] - per["mean"]) / sr.mean_bar(mo["cnt"], per["A"])
    rC = np.abs(mo["C"] - per["cov"]) / per["bar"]
    print("%s voxel %g: worst mean error / bar %.3g, worst covariance error / bar %.3g" % (name, voxel, rc.max(), rC.max()))
    assert rc.max() <= 1.0 and rC.max() <= 1.0
    # a sum in another order (the default mode's freedom) meets it too
    back = sr.moments(scenes[name]["S"], voxel, reverse=True)
    assert (np.abs(back["C"] - per["cov"]) / per["bar"]).max() <= 1.0


def test_raw_moments_miss_the_bar_at_1000_m(scenes):
    """the tooth: sum(a a^T) / N - c c^T cancels at the coordinates of a long session, the centred form does not"""
    for voxel in VOXELS:
        sc = scenes["far"]
        per = sc["per"][voxel]
        raw = np.abs(sr.raw_moments(sc["S"], voxel) - per["cov"]) / per["bar"]
        cen = np.abs(per["mo"]["C"] - per["cov"]) / per["bar"]
        multi = per["mo"]["cnt"] >= 2
        print("far voxel %g: raw moments worst error / bar %.3g (voxels over the bar: %d of %d), centred %.3g"
              % (voxel, raw.max(), (raw.max(axis=1) > 1).sum(), multi.sum(), cen.max()))
        # (not every voxel: the dyadic triples and pairs of keyframe 0 are exact in either form)
        assert raw.max() > 100.0 and (raw[multi].max(axis=1) > 1.0).mean() > 0.5
        assert cen.max() <= 1.0
        # and it is the shift that does it: the error of the raw form grows with the squared distance
        near = scenes["near"]["per"][voxel]
        nraw = np.abs(sr.raw_moments(scenes["near"]["S"], voxel) - near["cov"])
        assert np.abs(sr.raw_moments(sc["S"], voxel) - per["cov"]).max() > 1000.0 * nraw.max()


# ---------------------------------------------------------------- mutations
def _fit_np(Cs):
    w, V = np.linalg.eigh(np.stack([sr.sym(c) for c in Cs]))
    return w, V


def test_mutations_change_the_result(scenes):
    sc = scenes["far"]
    S, kf, sessions = sc["S"], sc["kf"], sc["sessions"]
    base = sc["per"][0.5]["mo"]
    same = sr.moments(S, 0.5)
    assert np.array_equal(same["C"], base["C"]) and np.array_equal(same["c"], base["c"])      # the scaffold is deterministic
    multi = base["cnt"] >= 2
    # 1. the products in another order (xx yy zz xy xz yz)
    m1 = sr.moments(S, 0.5, pairs=((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)))
    assert not np.array_equal(m1["C"], base["C"])
    # 2. centred on the narrowed mean
    m2 = sr.moments(S, 0.5, centre="float")
    assert (np.any(m2["C"] != base["C"], axis=1) == multi).all() or np.any(m2["C"] != base["C"], axis=1).sum() > 0.9 * multi.sum()
    # 3. M / cnt in place of M * (1 / cnt)
    m3 = sr.moments(S, 0.5, inv_cnt=False)
    assert np.any(m3["C"] != base["C"])
    # 4. the chain added backwards
    m4 = sr.moments(S, 0.5, reverse=True)
    assert np.any(m4["C"] != base["C"])
    # the record: orientation and the cnt < 3 rule (any eigen-solver shows these)
    keep = base["cnt"] >= 1
    c, Cm, cnt, first = base["c"][keep], base["C"][keep], base["cnt"][keep], base["first"][keep]
    sen = sr.sensors(sessions, kf, first)
    inten = S[first, 3].astype(np.float64)
    w, V = _fit_np(Cm)
    rec = sr.assemble(c, w, V, cnt, sen, inten)
    # 5. the normal away from the sensor
    r5 = sr.assemble(c, w, V, cnt, sen, inten, orient="away")
    big = cnt >= 3
    assert np.array_equal(r5[big, 4:7], -rec[big, 4:7]) and np.array_equal(r5[:, :4], rec[:, :4])
    # 6. the sensor of the LAST record's keyframe: some voxel's normal turns round, or none does and the rule is not exercised
    last = np.zeros(len(base["cnt"]), np.int64)
    np.maximum.at(last, base["vox"], np.arange(len(S)))
    sen_last = sr.sensors(sessions, kf, last[keep])
    assert np.any(sen_last != sen)
    # 7. cnt < 3 keeps its normal / cnt <= 3 loses it
    r7 = sr.assemble(c, w, V, cnt, sen, inten, small=1)
    assert np.any(r7[cnt < 3, 4:7] != 0.0) and not np.any(rec[cnt < 3, 4:7] != 0.0)
    r8 = sr.assemble(c, w, V, cnt, sen, inten, small=4)
    assert np.any(r8[cnt == 3, 4:7] != rec[cnt == 3, 4:7])
    # the fields a mutation must not touch
    assert np.array_equal(rec[:, 11], cnt.astype(np.float32)) and np.array_equal(rec[:, :3], c.astype(np.float32))
    assert np.array_equal(rec[:, :4], ev.export_voxel(sessions, 1, 0.5, 1)[0])


@pytest.mark.parametrize("name", ["near", "far"])
def test_every_orientation_is_decidable(scenes, host, name):
    """no voxel's normal is perpendicular to the line of sight of its first record's keyframe: |n . v| >= 1e-6 |v|, so that the
    sign of every normal of three records or more is a fact and not an accident of rounding"""
    exe, d = host
    sc = scenes[name]
    for voxel in VOXELS:
        for jump in (1, 3):
            S, kf = ev.sequence(sc["sessions"], jump)
            mo = sr.moments(S, voxel)
            big = mo["cnt"] >= 3
            w, V = sr.host_solver(exe, d)(mo["C"][big])
            v = sr.sensors(sc["sessions"], kf, mo["first"][big]) - mo["c"][big]
            rel = np.abs(np.einsum("ij,ij->i", V[:, :, 0], v)) / np.linalg.norm(v, axis=1)
            print("%s voxel %g jump %d: %d voxels of three records or more, smallest |n . v| / |v| = %.3g" % (name, voxel, jump, big.sum(), rel.min()))
            assert rel.min() >= 1e-6


# ---------------------------------------------------------------- the host build of the fit header
@pytest.mark.parametrize("name", ["near", "far"])
@pytest.mark.parametrize("voxel", VOXELS)
def test_host_fit_on_the_restated_moments(scenes, host, name, voxel):
    exe, d = host
    sc = scenes[name]
    mo = sc["per"][voxel]["mo"]
    sen = sr.sensors(sc["sessions"], sc["kf"], mo["first"])
    inten = sc["S"][mo["first"], 3].astype(np.float64)
    rec, w, V = sr.host_fit(exe, d, mo["c"], mo["C"], sen, mo["cnt"], inten)
    # the record is the assembly of the program's own decomposition, bit for bit: clamp, orientation, cnt < 3, narrowing
    assert np.array_equal(rec, sr.assemble(mo["c"], w, V, mo["cnt"], sen, inten))
    assert np.array_equal(rec[:, :4], ev.export_voxel(sc["sessions"], 1, voxel, 1)[0])
    # the decomposition against the 50-digit reference of the same double matrix, every voxel
    worst, fallback, noisy, rworst = {}, 0, 0, {}
    for v in range(len(w)):
        A = sr.sym(mo["C"][v])
        if not np.any(A):
            assert not np.any(w[v]) and np.array_equal(V[v], np.eye(3))
            continue
        ref = er.Ref(A)
        fallback += ref.dc1() <= er.THRESH
        noisy += ref.dc1() <= er.THRESH and mo["first"][v] >= len(sc["sessions"][0][0][0])      # not a voxel of keyframe 0: the pole
        for k, r in er.check(ref, w[v], V[v]).items():
            worst[k] = max(worst.get(k, 0.0), r)
        for k, r in sr.check_record(mo["C"][v], rec[v], mo["cnt"][v]).items():
            rworst[k] = max(rworst.get(k, 0.0), r)
    print("%s voxel %g: %d voxels, %d on the fallback's side of the pair test; worst ratios %s; of the float record %s"
          % (name, voxel, len(w), fallback, {k: "%.3g" % r for k, r in worst.items()}, {k: "%.3g" % r for k, r in rworst.items()}))
    assert max(worst.values()) <= 1.0 and max(rworst.values()) <= 1.0
    assert fallback >= 6                                                       # the triples at the least
    assert noisy >= 1 or voxel != 1.0                                          # and, in the longer voxels, the pole
    big = mo["cnt"] >= 3
    v = sen[big] - mo["c"][big]
    assert (np.einsum("ij,ij->i", rec[big, 4:7].astype(np.float64), v) > 0).all()   # toward the sensor
    assert not rec[~big, 4:7].any() and (rec[:, 7] <= rec[:, 8]).all() and (rec[:, 8] <= rec[:, 9]).all()
    assert (rec[:, 10] >= 0).all() and (rec[:, 10] <= np.float32(1.0 / 3.0) * (1 + 1e-6)).all()
    assert (rec[mo["cnt"] == 1, 7:11] == 0).all()


@pytest.mark.parametrize("n,interval,want", [(0, 5, [0]), (5, 5, [5]), (6, 5, [5, 6]), (11, 5, [5, 10, 11]), (3, 1, [1, 2, 3])])
def test_message_cuts(host, n, interval, want):
    r = subprocess.run([host[0], "cuts", str(n), str(interval)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split()] == want == ev.message_ends(n, interval)


def test_unknown_mode_is_an_error(host):
    assert subprocess.run([host[0], "nothing"], capture_output=True, timeout=60).returncode == 2
