"""CPU-side checks of the drop-in boundary: libvoxelba.so builds/loads, exports every symbol declared in
include/voxelba.h, binds each with the header's prototype (voxel-slam_amd/abi.py, held to the header here), fails loudly without a
GPU, and the host-side (non-device) entry points agree with the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


SCALAR_KINDS = {"int": "i", "int64_t": "q", "double": "d", "float": "f", "size_t": "z"}
PROTOTYPE = re.compile(r"(?<![\w*])((?:const\s+)?[A-Za-z_]\w*[\s*]+)(vba_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def parse_prototypes(text):
    """C declarations -> [(return type, name, [parameter types])], the types normalised ("const double *", "int64_t"), parameter
    names dropped.  Comments and preprocessor lines are stripped first; a typedef of a function pointer is no prototype."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)

    def norm(t, named):
        toks = t.replace("*", " * ").split()
        if named and toks[-1] != "*" and len(toks) > 1:      # the last word is the parameter's name
            toks = toks[:-1]
        return " ".join(toks)

    out = []
    for ret, name, params in PROTOTYPE.findall(text):
        params = params.strip()
        out.append((norm(ret, False), name, [] if params in ("", "void") else [norm(p, True) for p in params.split(",")]))
    return out


def kind_of(ctype, ret=False):
    """the rule of voxel-slam_amd/abi.py: a C type -> its letter; anything outside the closed set is an error"""
    if ctype == "const char *":
        return "s"
    if "*" in ctype or ctype == "vba_allreduce_fn":
        return "p"
    if ret and ctype == "void":
        return "v"
    return SCALAR_KINDS[ctype]


def header_prototypes():
    hdr = open(os.path.join(ROOT, "include", "voxelba.h")).read()
    return hdr, {name: kind_of(ret, True) + ":" + "".join(kind_of(p) for p in params) for ret, name, params in parse_prototypes(hdr)}


def test_parser_has_teeth():
    got = parse_prototypes("""
        #define VBA_OK 0
        typedef int (*vba_allreduce_fn)(void *user, void *dev, size_t n, void *stream);   /* no prototype */
        /* vba_in_a_comment(int x); */
        int vba_two_lines(vba_ctx *ctx, int n, const double *pnt,
                          int64_t first, double *out);
        int vba_inline(vba_ctx *ctx, vba_odom_report *report /* may be NULL */, float w);
        int vba_sessions(int n_db, vba_btc_db *const *dbs, const double **rows, vba_allreduce_fn fn);
        const char *vba_text(int status);     // a string back
        void vba_read(vba_ctx *ctx, const char *name, size_t n_bytes, long long *slots);
        int vba_none(void);
    """)
    assert got == [
        ("int", "vba_two_lines", ["vba_ctx *", "int", "const double *", "int64_t", "double *"]),
        ("int", "vba_inline", ["vba_ctx *", "vba_odom_report *", "float"]),
        ("int", "vba_sessions", ["int", "vba_btc_db * const *", "const double * *", "vba_allreduce_fn"]),
        ("const char *", "vba_text", ["int"]),
        ("void", "vba_read", ["vba_ctx *", "const char *", "size_t", "long long *"]),
        ("int", "vba_none", []),
    ]
    kinds = [kind_of(r, True) + ":" + "".join(kind_of(p) for p in ps) for r, _, ps in got]
    assert kinds == ["i:pipqp", "i:ppf", "i:ippp", "s:i", "v:pszp", "i:"]
    for outside in ("long long", "unsigned int", "void", "vba_options"):      # by value: not in the closed set
        with pytest.raises(KeyError):
            kind_of(outside)


def test_exports_match_header(capi):
    """abi.PROTOTYPES is the header: every function, its return kind and every parameter kind, in the header's order"""
    from voxel_slam_amd import abi
    hdr, parsed = header_prototypes()
    declared = set(re.findall(r"\b(vba_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"vba_allreduce_fn"}
    assert set(parsed) == declared and len(parsed) >= 176, set(parsed) ^ declared       # the parser skipped nothing
    lib = capi.load()
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert declared == set(capi.EXPORTS), declared ^ set(capi.EXPORTS)
    wrong = {s: (abi.PROTOTYPES.get(s), parsed[s]) for s in parsed if abi.PROTOTYPES.get(s) != parsed[s]}
    assert not wrong, wrong
    assert list(abi.PROTOTYPES) == list(parsed) == capi.EXPORTS                         # and in the same order
    assert set("".join(abi.PROTOTYPES.values())) - {":"} <= set(abi.KINDS)


def test_every_function_of_the_library_is_typed(capi):
    from voxel_slam_amd import abi
    _, parsed = header_prototypes()
    lib = capi.load()
    for name, proto in parsed.items():
        fn = getattr(lib, name)
        ret, params = proto.split(":")
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert list(fn.argtypes) == [abi.KINDS[k] for k in params] and fn.restype is abi.KINDS[ret], name
    typed = [k for k, v in vars(lib).items() if k.startswith("vba_")]      # what attribute access has bound so far
    assert set(typed) == set(parsed)


def test_int64_argument_arrives_whole(capi):
    """vba_kf_export_plan takes ``int64_t interval_size`` by value: cut to its low 32 bits, 2^33 + 2 is 2, every keyframe closes a
    message and n_msgs is 4 (what an untyped call with a bare integer gave)"""
    lib = capi.load()
    interval = 2 ** 33 + 2
    sizes = np.array([10, 10, 10], dtype=np.int32)
    ip = C.POINTER(C.c_int)

    def raw(iv):
        j = C.c_int(-77); nm = C.c_int(-77)
        kb = np.full(4, -77, dtype=np.int64); me = np.full(4, -77, dtype=np.int32)
        st = lib.vba_kf_export_plan(3, sizes.ctypes.data_as(ip), iv, 1, C.byref(j), kb.ctypes.data_as(C.POINTER(C.c_int64)), 4,
                                    me.ctypes.data_as(ip), C.byref(nm))
        return st, j.value, kb.tolist(), me.tolist(), nm.value

    bare = raw(interval)
    assert bare[0] == 0 and bare[4] == 1 and bare[3][0] == 3, bare
    assert bare == raw(C.c_int64(interval))
    j, kb, me = capi.kf_export_plan(sizes, interval_size=interval, jump=1)
    assert (j, kb.tolist(), me.tolist()) == (bare[1], bare[2], bare[3][:1])


def test_double_argument_arrives_as_a_double(capi):
    """vba_imu_ekf_propagate with its four by-value doubles as bare Python floats: the bits of the C.c_double call"""
    import imu_ekf_ref
    c = imu_ekf_ref.corpus()["m21"]
    lib = capi.load()
    dp = C.POINTER(C.c_double)
    imu = np.ascontiguousarray(c["imu"], dtype=np.float64); noise = np.ascontiguousarray(c["noise"], dtype=np.float64)
    scalars = [float(c[k]) for k in ("sg", "last_end", "beg", "end")]
    assert all(type(x) is float for x in scalars) and any(x != int(x) for x in scalars)

    def run(wrap):
        st = np.array(c["state"], dtype=np.float64); cov = np.array(c["cov"], dtype=np.float64)
        poses = np.zeros((len(imu), 22)); end = np.zeros(12); n = C.c_int(-7)
        r = lib.vba_imu_ekf_propagate(len(imu), imu.ctypes.data_as(dp), noise.ctypes.data_as(dp), *[wrap(x) for x in scalars],
                                      st.ctypes.data_as(dp), cov.ctypes.data_as(dp), poses.ctypes.data_as(dp), end.ctypes.data_as(dp), C.byref(n))
        assert r == capi.OK and n.value > 0
        return st, cov, poses, end, n.value

    a, b = run(lambda x: x), run(C.c_double)
    assert a[4] == b[4]
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(a[0], c["state"])          # the call did something


def test_wrong_kinds_are_refused(capi):
    lib = capi.load()
    with pytest.raises(C.ArgumentError):
        lib.vba_scanlog_release(None, C.c_int(0))        # the header says int64_t
    with pytest.raises(C.ArgumentError):
        lib.vba_scanlog_release(None, 0.5)
    assert lib.vba_scanlog_release(None, C.c_int64(0)) == capi.ERR_BAD_ARG


WRAPPED_BY_VALUE = re.compile(r"[(,]\s*C\.c_(int|int64|double|float|longlong|size_t)\(")
SETS_A_PROTOTYPE = re.compile(r"\.argtypes\s*=|\.restype\s*=")


def test_text_patterns_have_teeth():
    assert WRAPPED_BY_VALUE.search("lib.vba_map_slide(self.h, C.c_int(mgsize))") and WRAPPED_BY_VALUE.search("f(C.c_int64(n),\n  C.c_double(x))")
    assert WRAPPED_BY_VALUE.search("head = (ctx.h,\n        C.c_size_t(n))")
    for ok in ("n = C.c_int(); b = C.c_int64(-1)", "lib.f(self.h, C.c_void_p(d), C.byref(n))", '("win_size", C.c_int), ("x", C.c_double * 4)',
               "a.ctypes.data_as(C.POINTER(C.c_int))"):
        assert not WRAPPED_BY_VALUE.search(ok), ok
    assert SETS_A_PROTOTYPE.search("lib.vba_x.restype = C.c_char_p") and SETS_A_PROTOTYPE.search("fn.argtypes= [C.c_int]")
    assert not SETS_A_PROTOTYPE.search("assert fn.argtypes is not None and len(fn.argtypes) == 3 and fn.restype is None")


def test_binding_text(capi):
    pkg = os.path.dirname(capi.__file__)
    src = open(os.path.join(pkg, "capi.py")).read()
    assert not WRAPPED_BY_VALUE.findall(src)
    # prototypes are set in one place: the loop of capi.load() over the table
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            text = open(os.path.join(pkg, f)).read()
            hits = [m.start() for m in SETS_A_PROTOTYPE.finditer(text)]
            if f != "capi.py":
                assert not hits, f
                continue
            a = text.index("\ndef load():"); b = text.index("\ndef ", a + 1)
            assert len(hits) == 2 and all(a < h < b for h in hits), hits
    # one lifecycle: no create / destroy name is spelled out more than once
    for prefix in ("vba_btc", "vba_kf", "vba_loop_map", "vba_scanlog", "vba_scan_frame", "vba_init_window", "vba_odom_state"):
        for op in ("_create", "_destroy"):
            assert len(re.findall(r"\b%s%s\b" % (prefix, op), src)) <= 1, prefix + op


def test_no_device_is_a_loud_error(capi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    o = capi.default_options()
    with pytest.raises(capi.VbaError) as e:
        capi.Context(o)
    assert e.value.status == capi.ERR_NO_DEVICE


def test_default_options_are_avia_yaml(capi):
    o = capi.default_options()
    assert (o.win_size, o.max_layer, o.max_points, o.thread_num) == (10, 2, 100, 5)
    assert o.min_eigen_value == 0.0025 and o.imu_coef == 1e-4 and list(o.plane_eigen_value_thre) == [0.25] * 4


def test_shard_owner_is_a_partition(capi):
    rng = np.random.default_rng(0)
    keys = rng.integers(-200, 200, (4000, 3))
    for n in (1, 2, 4, 8):
        own = np.array([capi.shard_owner(k, n) for k in keys])
        assert own.min() >= 0 and own.max() < n
        cnt = np.bincount(own, minlength=n)
        assert cnt.min() > 0.7 * len(keys) / n      # roughly balanced contiguous bucket ranges


def _imu_inputs(seed=0):
    rng = np.random.default_rng(seed)
    n = 21
    t = np.arange(n) / 200.0
    gyr = rng.normal(0, 0.2, (n, 3)); acc = rng.normal(0, 0.5, (n, 3)) + np.array([0, 0, 9.8])
    bg = rng.normal(0, 0.01, 3); ba = rng.normal(0, 0.05, 3)
    nm = np.array([0.01] * 3 + [1.0] * 3); nw = np.array([1e-4] * 6)
    return t, gyr, acc, bg, ba, nm, nw


def test_host_imu_preintegration_matches_oracle(capi, oracle):
    args = _imu_inputs()
    a = capi.imu_preintegrate(*args)
    b = oracle.imu_preintegrate(*args)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-15)


def test_host_imu_give_evaluate_matches_oracle(capi, oracle):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    imu = capi.imu_preintegrate(*_imu_inputs(1))
    imu[67:73] = rng.normal(0, 1e-3, 6)      # dbg, dba
    def state(k):
        s = np.zeros(25)
        s[1:10] = Rotation.from_rotvec(rng.normal(0, 0.3, 3)).as_matrix().ravel()
        s[10:13] = rng.normal(0, 1, 3); s[13:16] = rng.normal(0, 1, 3)
        s[16:19] = rng.normal(0, 0.01, 3); s[19:22] = rng.normal(0, 0.05, 3); s[22:25] = [0, 0, -9.8]
        return s
    s1, s2 = state(0), state(1)
    for with_g in (False, True):
        ra, Ja, ga = capi.imu_give_evaluate(imu, s1, s2, with_g, True)
        rb, Jb, gb = oracle.imu_give_evaluate(imu, s1, s2, with_g, True)
        assert ra == pytest.approx(rb, rel=1e-10)
        assert np.allclose(Ja, Jb, rtol=1e-9, atol=1e-9 * np.abs(Jb).max())
        assert np.allclose(ga, gb, rtol=1e-9, atol=1e-9 * np.abs(gb).max())


def test_debug_plane_update_refuses_without_a_context(capi):
    """the diagnostic entry of tests/test_gpu_plane.py checks its arguments before it touches a device"""
    lib = capi.load()
    rows = np.zeros((1, 67)); out = np.full((1, 43), np.nan)
    st = lib.vba_debug_plane_update(None, C.c_int(1), rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert st == capi.ERR_BAD_ARG and np.isnan(out).all()


def test_debug_pgo_step_is_exported_typed_and_refuses_without_a_context(capi):
    """the diagnostic entry of tests/test_gpu_pgo_passes.py: declared with the other vba_debug_*, typed from abi.py, and as
    vba_pgo_optimize it checks its arguments before it touches a device"""
    from voxel_slam_amd import abi
    assert abi.PROTOTYPES["vba_debug_pgo_step"] == "i:pipipip" + "p" * 8
    assert hasattr(capi.Context, "debug_pgo_step")
    lib = capi.load()
    poses = np.zeros((1, 12)); pr = np.zeros((1, 19)); slot = np.full((1, 121), np.nan)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.vba_debug_pgo_step(None, C.c_int(1), p(poses), C.c_int(0), None, C.c_int(1), p(pr), p(slot), None, None, None, None, None, None, None)
    assert st == capi.ERR_BAD_ARG and np.isnan(slot).all()


def test_debug_btc_icp_pass_is_exported_typed_and_refuses_without_a_database(capi):
    """the diagnostic entry of tests/test_gpu_icp_passes.py: declared next to vba_btc_icp_normal (it takes database handles), typed from
    abi.py, its state struct the size of the device's, and it checks its arguments before it touches a device"""
    from voxel_slam_amd import abi
    assert abi.PROTOTYPES["vba_debug_btc_icp_pass"] == "i:pipipi" + "p" * 6
    names = list(abi.PROTOTYPES)
    assert names.index("vba_debug_btc_icp_pass") == names.index("vba_btc_icp_normal") + 1
    assert hasattr(capi.BtcDb, "debug_icp_pass") and C.sizeof(capi.BtcIcpState) == 216
    lib = capi.load()
    st = capi.BtcIcpState.start(np.zeros(3), np.eye(3)); before = bytes(st)
    sums = np.full(35, np.nan)
    rc = lib.vba_debug_btc_icp_pass(None, C.c_int(0), None, C.c_int(0), C.byref(st), C.c_int(0), None, None, None,
                                    sums.ctypes.data_as(C.c_void_p), None, None)
    assert rc == capi.ERR_BAD_ARG and np.isnan(sums).all() and bytes(st) == before
