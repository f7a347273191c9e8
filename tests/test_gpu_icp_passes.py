"""The passes of vba_btc_icp_normal on the MI355X, one iteration read back pass by pass through vba_debug_btc_icp_pass (the production
kernels and the host function the loop calls), against the per-pass reference of tests/icp_ref.py: 1-NN keys bit for bit, every clear
gate decision, the 35 sums of every workgroup and of the pass within counted bars, the solved step, the pose update and the state
table.  Calibration and teeth of the reference: tests/test_icp_ref_cpu.py."""
import numpy as np
import pytest

import icp_ref as ir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    o = capi.default_options()
    o.device = 0
    c = capi.Context(o)
    yield c
    c.close()


class Clouds:
    """the corpus clouds resident in one database, pushed once per distinct array"""

    def __init__(self, capi, ctx):
        self.db = ctx.btc_db(capi.btc_default_config(0)); self.frames = {}

    def frame(self, a):
        k = (a.shape, a.tobytes())
        if k not in self.frames:
            self.frames[k] = self.db.num_frames()
            self.db.push_plane_cloud(a, self.frames[k])
        return self.frames[k]


@pytest.fixture(scope="module")
def clouds(capi, ctx):
    c = Clouds(capi, ctx)
    yield c
    c.db.close()


def _run(capi, clouds, case, slices, state=None, prefill=None):
    st = state if state is not None else ir.start_state(case, capi.BtcIcpState)
    r = clouds.db.debug_icp_pass(clouds.frame(case["src"]), clouds.db, clouds.frame(case["tar"]), st, len(case["src"]), slices, prefill)
    r["raw_state"] = r["state"]; r["state"] = ir.state_dict(r["state"])
    return r


@pytest.mark.parametrize("cls", ir.CLASSES)
def test_passes_meet_the_reference(capi, clouds, cls):
    """every case of the class, every slice plan: keys, clear decisions, the bars on partial and sums, the step, the state"""
    worst = {}; unclear = 0; points = 0
    for case in ir.cases(cls):
        ref = ir.ref_of(case)
        for sl in case["slices"]:
            s0 = ir.start_state(case, capi.BtcIcpState)
            out = _run(capi, clouds, case, sl, s0)
            if case["done"]:
                # the launches return at once: the state comes back as it went in, nothing of the outputs is written
                assert bytes(out["raw_state"]) == bytes(s0)
                assert np.isnan(out["sums"]).all() and np.isnan(out["partial"]).all() and np.isnan(out["dx"]).all()
                assert (out["gate"] == 255).all() and not out["key"].any()
                continue
            if sl == 0:
                assert out["slices"] == ir.own_slices(len(case["src"]), len(case["tar"]))
            f, g, ok = ir.check_case(case, out, sl)
            assert ok, (case["name"], sl, f, g)
            for k, v in ir.worst_ratios(f, g).items():
                worst[k] = max(worst.get(k, 0.0), float(v))
        unclear += int(ref.unclear.sum()); points += ref.ns
    print("ICP-DEV %s worst %s unclear %d of %d" % (cls, {k: round(v, 4) for k, v in worst.items()}, unclear, points))
    if cls != "threshold":
        assert unclear <= ir.UNCLEAR_CAP * max(points, 1)


def test_every_slice_plan_returns_the_same_bits(capi, clouds):
    """nt = 2200 (9 tiles): 1, 2, 4 (the last slice empty), 8 (slices 5 to 7 empty), 9 slices, and the call's own choice at ns = 17 000
    (8 slices of 2 tiles, the same empty tail) and at ns = 200 (clamped to the 9 tiles)"""
    a, big, small = ir.cases("slices")
    outs = [_run(capi, clouds, a, sl) for sl in a["slices"]]
    assert [o["slices"] for o in outs] == [1, 2, 4, 8, 9]
    for o in outs[1:]:
        for k in ("key", "gate", "partial", "sums", "dx"):
            assert np.array_equal(o[k], outs[0][k]), k
    own = _run(capi, clouds, big, 0)
    assert own["slices"] == 8
    one = _run(capi, clouds, small, 1); nine = _run(capi, clouds, small, 0)
    assert nine["slices"] == 9
    for k in ("key", "gate", "partial", "sums", "dx"):
        assert np.array_equal(one[k], nine[k]), k
    # the plan is 1024 workgroups and max(ntile, 1) slices: requests beyond are refused with the state untouched
    s0 = ir.start_state(a, capi.BtcIcpState)
    for case, sl in ((a, 10), (big, 16), (a, -1)):
        st = capi.BtcIcpState.from_buffer_copy(s0)
        with pytest.raises(capi.VbaError) as e:
            clouds.db.debug_icp_pass(clouds.frame(case["src"]), clouds.db, clouds.frame(case["tar"]), st, len(case["src"]), sl)
        assert e.value.status == capi.ERR_BAD_ARG and bytes(st) == bytes(s0)


def test_partials_are_the_same_bits_run_to_run(capi, clouds):
    case = ir.cases("slices")[0]
    a = _run(capi, clouds, case, 0); b = _run(capi, clouds, case, 0)
    assert np.array_equal(a["partial"], b["partial"]) and np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["key"], b["key"])


@pytest.mark.parametrize("name", ["scene_offset_full", "scene_identity_full", "degenerate_parallel", "degenerate_gated_out", "_257_0", "_0_257"])
def test_chained_passes_are_the_public_call(capi, clouds, name):
    """twenty debug passes from the state vba_btc_icp_normal starts from reproduce it bit for bit: pose, eigenvalues, iterations, ok"""
    case = [c for cls in ("scene", "degenerate") for c in ir.cases(cls) if c["name"].endswith(name)][0]
    fs, ft = clouds.frame(case["src"]), clouds.frame(case["tar"])
    pub = clouds.db.icp_normal(fs, clouds.db, ft, case["t"], case["R"], 0.1)
    st = capi.BtcIcpState.start(case["t"], case["R"])
    for _ in range(20):
        st = clouds.db.debug_icp_pass(fs, clouds.db, ft, st, len(case["src"]))["state"]
    assert st.done == 1 and st.iters == pub["iters"]
    assert np.array_equal(np.array(st.R[:]).reshape(3, 3), pub["R"]) and np.array_equal(np.array(st.t[:]), pub["t"])
    assert np.array_equal(np.array(st.eig[:]), pub["eig"])
    assert pub["ok"] == (1 if (st.eig[0] > 0.1 and st.is_conv == 1) else 0)
    # the eigenvalues the loop ends with, against eig3_ref's bar on the mat_norm it ends with (degenerate_parallel: the Jacobi fallback)
    assert ir.eig_ratio(np.array(st.mat[:]), np.array(st.eig[:])) <= 1.0
    if name.startswith("degenerate") or name in ("_257_0", "_0_257"):
        assert pub["ok"] == 0 and np.all(np.isfinite(pub["R"])) and np.all(np.isfinite(pub["t"]))


def test_public_call_on_empty_and_degenerate_clouds_leaves_the_context_sound(capi, clouds):
    """nt = 0, ns = 0 and the degenerate clouds report ok == 0; a registration on the same context afterwards is what it was before"""
    good = [c for c in ir.cases("scene") if c["name"] == "scene_offset_full"][0]
    fs, ft = clouds.frame(good["src"]), clouds.frame(good["tar"])
    before = clouds.db.icp_normal(fs, clouds.db, ft, good["t"], good["R"], 0.1)
    assert before["ok"] == 1
    empty = clouds.frame(np.zeros((0, 6), dtype=np.float32))
    for a, b in ((fs, empty), (empty, ft), (empty, empty)):
        r = clouds.db.icp_normal(a, clouds.db, b, good["t"], good["R"], 0.1)
        assert r["ok"] == 0 and np.array_equal(r["R"], good["R"]) and np.array_equal(r["t"], good["t"]) and r["iters"] == 2
        assert np.array_equal(r["eig"], np.zeros(3))
    for case in ir.cases("degenerate"):
        r = clouds.db.icp_normal(clouds.frame(case["src"]), clouds.db, clouds.frame(case["tar"]), case["t"], case["R"], 0.1)
        assert r["ok"] == 0, case["name"]
    after = clouds.db.icp_normal(fs, clouds.db, ft, good["t"], good["R"], 0.1)
    for k in ("t", "R", "eig"):
        assert np.array_equal(before[k], after[k])
    assert before["iters"] == after["iters"] and after["ok"] == 1


def test_debug_pass_refuses_bad_arguments(capi, ctx, clouds):
    import ctypes as C
    lib = capi.load()
    case = ir.cases("scene")[0]
    fs, ft = clouds.frame(case["src"]), clouds.frame(case["tar"])
    s0 = ir.start_state(case, capi.BtcIcpState); st = capi.BtcIcpState.from_buffer_copy(s0)
    call = lambda a, fa, b, fb, s: lib.vba_debug_btc_icp_pass(a, fa, b, fb, s, 0, None, None, None, None, None, None)
    assert call(None, fs, clouds.db.h, ft, C.byref(st)) == capi.ERR_BAD_ARG
    assert call(clouds.db.h, fs, None, ft, C.byref(st)) == capi.ERR_BAD_ARG
    assert call(clouds.db.h, fs, clouds.db.h, ft, None) == capi.ERR_BAD_ARG
    assert call(clouds.db.h, -1, clouds.db.h, ft, C.byref(st)) == capi.ERR_BAD_ARG
    assert call(clouds.db.h, fs, clouds.db.h, clouds.db.num_frames(), C.byref(st)) == capi.ERR_BAD_ARG
    assert bytes(st) == bytes(s0)
    assert call(clouds.db.h, fs, clouds.db.h, ft, C.byref(st)) == capi.OK and st.iters == 1      # every output pointer may be NULL
