"""GPU tests of the initialisation odometry on a state resident in HBM: vba_odom_lio_state_estimation_kdtree_on_state
against vba_odom_lio_state_estimation_kdtree_resident, and vba_odom_state_export_scan against its numpy restatement
(tests/scan_export_ref.py).  The scene, the predictions (rng seed 17), the covariance and the bars are those of test_gpu_kd_resident.py.
Every comparison runs twin contexts fed the same sequence: twin A makes the resident call with state and covariance on the host, twin B
the on-state call.  The two differ only in where the image of the call is built, so whatever the loop reads and writes without atomics
is compared BIT FOR BIT; the map after a re-sampling in a context without the deterministic mode is held to the bars of
test_gpu_kd_resident.py only where the twins' maps may already differ in their order (the default-mode chain)."""
import ctypes as C

import numpy as np
import pytest

import imu_ekf_ref as R
from scan_export_ref import export_restated
from test_gpu_kd_resident import COV_BAR, STATE_BAR, _check_tree, _cov0, _ctx, _dev, env  # noqa: F401  (env: the module's fixture)

pytestmark = pytest.mark.gpu

REPORT_KEYS = ("iterations", "match_num", "rot_add", "tra_add", "nnt_eig_min")


class Twins:
    """Twin A (resident call, host state) and twin B (on-state call) with B's state object, which ``owner`` (default: B) creates."""

    def __init__(self, env, deterministic=0, owner=None):
        self.a, self.b = _ctx(env, deterministic), _ctx(env, deterministic)
        self.st = (owner or self.b).odom_state()

    def both(self, env, tag, pts, state, cov, want_state=True, bits=True, cov_a=None):
        """One call on each twin from (state, cov), B's set into its state object first (A from cov_a when given).  Returns A's
        (iterations, state, cov, report, map) and B's (iterations, state_out, state, cov, report, map); with ``bits`` everything must
        agree bit for bit."""
        dev = pts if hasattr(pts, "args") else _dev(env, pts)
        self.st.set(state, cov)
        return self.step(tag, dev, state, cov, want_state, bits, cov_a)

    def step(self, tag, dev, state, cov, want_state=True, bits=True, cov_a=None):
        """The same without the set: B runs on what its state object holds, which the caller says is (state, cov)."""
        it_a, st_a, cv_a, rep_a = self.a.lio_state_estimation_kdtree_resident(*dev.args, state, cov if cov_a is None else cov_a)
        it_b, rep_b, out_b = self.st.lio_state_estimation_kdtree(self.b, *dev.args, want_state=want_state)
        st_b, cv_b = self.st.get()
        ta, tb = self.a.kdtree_points(), self.b.kdtree_points()
        print("%s: n %d, iterations %d / %d, valid %s, map %d / %d" % (tag, dev.n, it_a, it_b, rep_b["match_num"][:it_b], len(ta), len(tb)))
        if bits:
            assert it_a == it_b, tag
            for k in REPORT_KEYS:
                np.testing.assert_array_equal(np.asarray(rep_a[k]), np.asarray(rep_b[k]), err_msg="%s report %s" % (tag, k))
            np.testing.assert_array_equal(st_b, st_a, err_msg=tag + " state")
            np.testing.assert_array_equal(cv_b.ravel(), cv_a.ravel(), err_msg=tag + " cov")
            if want_state:
                np.testing.assert_array_equal(out_b, st_a, err_msg=tag + " state_out")
            assert len(ta) == len(tb), tag
            np.testing.assert_array_equal(tb, ta, err_msg=tag + " map")
        return (it_a, st_a, cv_a, rep_a, ta), (it_b, out_b, st_b, cv_b, rep_b, tb)


def test_seeding(env):
    """99 points, then 1 point: both seed, nothing of the state moves, the maps are equal; the third call estimates on 100 points."""
    tw = Twins(env, deterministic=1)
    state, cov = env["states"][0], _cov0()
    p = env["pts"][0]
    for k, (pts, want) in enumerate(((p[:99], True), (p[99:100], False))):
        a, b = tw.both(env, "seed %d" % k, pts, state, cov, want_state=want)
        assert a[0] == b[0] == 0 and b[4]["iterations"] == 0 and np.all(b[4]["match_num"] == 0)
        np.testing.assert_array_equal(b[2], state); np.testing.assert_array_equal(b[3].ravel(), cov.ravel())      # st.get(): the bits that were set
        if want:
            np.testing.assert_array_equal(b[1], state)                                                          # state_out of a seeding call
        else:
            assert b[1] is None
        assert tw.a.kdtree_size() == tw.b.kdtree_size() == (99, 100)[k]
    a, b = tw.both(env, "first estimation on 100 points", env["pts"][1][:300], env["states"][1], cov)
    assert a[0] == b[0] >= 2 and (b[2] != env["states"][1]).any()


@pytest.mark.parametrize("deterministic", (0, 1))
def test_first_estimation(env, deterministic):
    """Both twins estimate on the same seeded map (the append keeps the order of the scan: no atomics decide anything)."""
    tw = Twins(env, deterministic)
    cov = _cov0()
    a, b = tw.both(env, "seed", env["pts"][0], env["states"][0], cov)
    assert a[0] == 0 and tw.b.kdtree_size() == len(env["pts"][0])
    a, b = tw.both(env, "scan 1", env["pts"][1], env["states"][1], cov)
    assert b[0] >= 3 and b[4]["match_num"][0] > 2000 and (b[2] != env["states"][1]).any() and (b[3] != cov).any()
    assert np.linalg.norm(b[2][10:13] - env["gt"][1]) < np.linalg.norm(env["states"][1][10:13] - env["gt"][1])


def test_chain_deterministic(env):
    """The five scans with the covariance chained through the state object in B and through the host in A: every call, and the map
    after every re-sampling, bit for bit; an empty scan on the live map at the end."""
    tw = Twins(env, deterministic=1)
    cov_a = _cov0()
    tw.st.set(env["states"][0], cov_a)
    iters = []
    for k in range(env["wl"].win_size):
        cov_b = tw.st.get()[1]                                     # B's covariance never comes from a result of A
        a, b = tw.both(env, "scan %d" % k, env["pts"][k], env["states"][k], cov_b, cov_a=cov_a)
        np.testing.assert_array_equal(cov_b.ravel(), np.ravel(cov_a))
        if a[0]:
            cov_a = a[2]
        iters.append(b[0])
    assert iters[0] == 0 and all(i >= 2 for i in iters[1:])
    # n == 0 on a live map: two iterations, the bits of state and covariance stay, the map is re-sampled as in A
    x, cv = tw.st.get()
    size = tw.b.kdtree_size()
    a, b = tw.step("empty scan", _dev(env, np.zeros((0, 3))), x, cv)
    assert a[0] == b[0] == 2 and np.all(b[4]["match_num"] == 0)
    np.testing.assert_array_equal(b[2], x); np.testing.assert_array_equal(b[3], cv); np.testing.assert_array_equal(b[1], x)
    assert tw.a.kdtree_size() == tw.b.kdtree_size() <= size


def test_chain_default_mode(env):
    """Without the deterministic mode the re-sampler's atomic insert promises no bits for the map, and the twins' maps may differ in
    their order from the second estimation on: B against A at the bars of test_gpu_kd_resident.py."""
    tw = Twins(env)
    cov_a = _cov0()
    tw.st.set(env["states"][0], cov_a)
    for k in range(env["wl"].win_size):
        cov_b = tw.st.get()[1]
        a, b = tw.both(env, "scan %d" % k, env["pts"][k], env["states"][k], cov_b, bits=False, cov_a=cov_a)
        scale = np.abs(a[2]).max()
        print("  B vs A: state %.3g, cov %.3g of max" % (np.abs(b[2] - a[1]).max(), np.abs(b[3].ravel() - a[2].ravel()).max() / scale))
        assert a[0] == b[0] == b[4]["iterations"]
        assert np.abs(b[2] - a[1]).max() < STATE_BAR and np.abs(b[1] - a[1]).max() < STATE_BAR
        assert np.abs(b[3].ravel() - a[2].ravel()).max() < COV_BAR * scale
        _check_tree("scan %d map" % k, b[5], a[4])
        if a[0]:
            cov_a = a[2]


@pytest.mark.parametrize("pose", ("m21", "scene"))
def test_behind_a_device_propagation(env, pose):
    """B: set, propagate, the on-state call.  A: the resident call on what a second state object returns after the same propagation.
    ``scene`` puts the m21 case at the predicted pose of scan 1, so that the loop finds its planes."""
    case = dict(R.corpus()["m21"])
    if pose == "scene":
        state = case["state"].copy(); state[1:13] = env["states"][1][1:13]; state[13:16] = [0.3, 0.1, 0.0]
        case["state"] = state
    tw = Twins(env, deterministic=1)
    tw.both(env, "seed", env["pts"][0], env["states"][0], _cov0())
    other = tw.a.odom_state()
    for st in (tw.st, other):
        st.set(case["state"], case["cov"])
        assert st.propagate(case["imu"], case["noise"], case["last_end"], case["beg"], case["end"], case["sg"]) > 0
    x, cv = other.get()
    assert (x != case["state"]).any() and (cv.ravel() != case["cov"]).any()
    a, b = tw.step("behind propagate (%s)" % pose, _dev(env, env["pts"][1]), x, cv)
    assert b[0] >= 2
    if pose == "scene":
        assert b[4]["match_num"][0] > 2000 and (b[2] != x).any()


def test_no_allocation_and_another_owner(env):
    """After kdtree_reserve and st.reserve nothing of the chain (propagation, update, export to a device buffer) allocates; the state
    object belongs to a third context of the same device and the bits are still A's."""
    import torch
    owner = _ctx(env, deterministic=1)
    tw = Twins(env, deterministic=1, owner=owner)
    assert tw.st.ctx is owner
    tw.b.kdtree_reserve(65536, 32768)
    tw.st.reserve(64)
    out = torch.zeros((max(len(p) for p in env["pts"]), 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    counters = (tw.b.kdtree_allocations(), tw.st.allocations())
    case = R.corpus()["m21"]
    cov = _cov0()
    tw.st.set(env["states"][0], cov)
    for k in range(env["wl"].win_size):
        cov_b = tw.st.get()[1]
        dev = _dev(env, env["pts"][k])
        a, b = tw.both(env, "scan %d" % k, dev, env["states"][k], cov_b)
        assert tw.st.export_scan(tw.b, *dev.args, intensity=1.0, out=out.data_ptr()) == dev.n
    tw.st.propagate(case["imu"], case["noise"], case["last_end"], case["beg"], case["end"], case["sg"])
    tw.b.synchronize(); owner.synchronize()
    assert (tw.b.kdtree_allocations(), tw.st.allocations()) == counters
    assert b[0] >= 2


def test_refusals(env):
    capi = env["capi"]
    ctx = _ctx(env)
    st = ctx.odom_state()
    state, cov = env["states"][0], _cov0()
    st.set(state, cov)
    dev = _dev(env, env["pts"][0][:64])
    f = ctx.lib.vba_odom_lio_state_estimation_kdtree_on_state
    it = C.c_int(7); ptr = C.c_void_p(dev.args[1])
    assert f(None, st.h, C.c_int(64), ptr, C.byref(it), None, None) == capi.ERR_BAD_ARG
    assert f(ctx.h, None, C.c_int(64), ptr, C.byref(it), None, None) == capi.ERR_BAD_ARG
    assert f(ctx.h, st.h, C.c_int(64), ptr, None, None, None) == capi.ERR_BAD_ARG
    assert f(ctx.h, st.h, C.c_int(-1), ptr, C.byref(it), None, None) == capi.ERR_BAD_ARG
    assert f(ctx.h, st.h, C.c_int(64), None, C.byref(it), None, None) == capi.ERR_BAD_ARG
    assert ctx.kdtree_size() == 0 and it.value == 7
    assert f(ctx.h, st.h, C.c_int(64), ptr, C.byref(it), None, None) == capi.OK             # report and state_out may be NULL
    assert ctx.kdtree_size() == 64 and it.value == 0
    assert f(ctx.h, st.h, C.c_int((1 << 28) - 63), ptr, C.byref(it), None, None) == capi.ERR_CAPACITY
    assert ctx.kdtree_size() == 64
    x, cv = st.get()
    np.testing.assert_array_equal(x, state); np.testing.assert_array_equal(cv.ravel(), cov.ravel())
    # a sharded context is accepted, as by the resident call: the point-cloud map is the context's and is not sharded
    sharded = _ctx(env)
    sharded.set_shard(0, 2)
    it_s, rep, out = st.lio_state_estimation_kdtree(sharded, *dev.args)
    assert it_s == 0 and sharded.kdtree_size() == 64
    np.testing.assert_array_equal(out, state)
    np.testing.assert_array_equal(sharded.kdtree_points(), ctx.kdtree_points())


# ------------------------------------------------------------------------------------------------ the published scan
@pytest.fixture(scope="module")
def exporter(env):
    ctx = _ctx(env)
    st = ctx.odom_state()
    st.set(env["states"][1], _cov0())
    return ctx, st, _dev(env, env["pts"][1])


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, None))
def test_export_scan(env, exporter, n):
    import torch
    ctx, st, dev = exporter
    n = dev.n if n is None else n
    ptr = dev.args[1] if n else 0
    want = export_restated(env["states"][1], dev.host[:n], 3.5)
    host = st.export_scan(ctx, n, ptr, intensity=3.5)
    assert host.shape == (n, 4) and host.dtype == np.float32
    np.testing.assert_array_equal(host, want)
    assert np.all(host[:, 3] == np.float32(3.5))
    out = torch.full((n + 1, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert st.export_scan(ctx, n, ptr, intensity=3.5, out=out.data_ptr()) == n
    ctx.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:n], want)
    assert np.all(got[n:] == -7.0)                                 # nothing past the n records


def test_export_scan_refusals(env, exporter):
    import torch
    capi = env["capi"]
    ctx, st, dev = exporter
    f = ctx.lib.vba_odom_state_export_scan
    n = 257
    m = C.c_int64(-1)
    host = np.full((n, 4), -7.0, dtype=np.float32)
    out = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ptr = C.c_void_p(dev.args[1])
    for target in (host.ctypes.data_as(C.c_void_p), C.c_void_p(out.data_ptr())):
        assert f(ctx.h, st.h, C.c_int(n), ptr, C.c_float(1.0), C.c_int64(n - 1), target, C.byref(m)) == capi.ERR_BAD_ARG
        assert f(ctx.h, st.h, C.c_int(-1), ptr, C.c_float(1.0), C.c_int64(n), target, C.byref(m)) == capi.ERR_BAD_ARG
        assert f(ctx.h, st.h, C.c_int(n), None, C.c_float(1.0), C.c_int64(n), target, C.byref(m)) == capi.ERR_BAD_ARG
        assert f(ctx.h, None, C.c_int(n), ptr, C.c_float(1.0), C.c_int64(n), target, C.byref(m)) == capi.ERR_BAD_ARG
        assert f(ctx.h, st.h, C.c_int(n), ptr, C.c_float(1.0), C.c_int64(n), target, None) == capi.ERR_BAD_ARG
    assert f(ctx.h, st.h, C.c_int(n), ptr, C.c_float(1.0), C.c_int64(n), None, C.byref(m)) == capi.ERR_BAD_ARG
    assert f(ctx.h, st.h, C.c_int(n - 1), ptr, C.c_float(1.0), C.c_int64(n), C.c_void_p(out.data_ptr() + 4), C.byref(m)) == capi.ERR_BAD_ARG   # misaligned
    ctx.synchronize()
    assert np.all(host == -7.0) and np.all(out.cpu().numpy() == -7.0)
    x, cv = st.get()
    np.testing.assert_array_equal(x, env["states"][1])


def test_export_after_an_update_uses_the_updated_pose(env):
    ctx = _ctx(env, deterministic=1)
    st = ctx.odom_state()
    st.set(env["states"][0], _cov0())
    st.lio_state_estimation_kdtree(ctx, *_dev(env, env["pts"][0]).args, want_state=False)
    dev = _dev(env, env["pts"][1])
    st.set(env["states"][1], _cov0())
    it, rep, x = st.lio_state_estimation_kdtree(ctx, *dev.args)
    assert it >= 2 and (x[1:13] != env["states"][1][1:13]).any()
    got = st.export_scan(ctx, *dev.args, intensity=0.0)
    np.testing.assert_array_equal(got, export_restated(x, dev.host))
    assert (got != export_restated(env["states"][1], dev.host)).any()
