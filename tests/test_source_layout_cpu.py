"""The source layout of libvoxelba.so as DESIGN.md states it ("Source layout"): one object per csrc/*.hip unit, every kernel header
compiled by exactly one unit, host launch code in the units and not in the kernel headers.  A text check over include lines, function
heads and file names; nothing is compiled.  Also its ownership rule: device and pinned buffers are members of the owning types of
vba_mem.hpp and free themselves, so the runtime's allocation and free calls appear only there."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "voxel-slam_amd", "csrc")

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
# the head of a host function that launches on a stream: `int name(... hipStream_t ...`, possibly over several lines
HOST_LAUNCH = re.compile(r"^(?:(?:static|inline)\s+)*int\s+(\w+)\s*\([^)]*\bhipStream_t\b", re.M)


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def reached(name, seen=None):
    """the files of csrc/ that `name` includes, directly or through another header of csrc/"""
    seen = set() if seen is None else seen
    for inc in INCLUDE.findall(read(name)):
        if "/" not in inc and inc not in seen and os.path.exists(os.path.join(CSRC, inc)):
            seen.add(inc)
            reached(inc, seen)
    return seen


def units():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, "*.hip")))


def kernel_headers():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "vba_kernels_*.hpp")))


def test_every_kernel_header_has_one_unit():
    assert len(units()) >= 10 and len(kernel_headers()) >= 10
    owners = {h: [] for h in kernel_headers()}
    for u in units():
        for inc in reached(u + ".hip"):
            if inc in owners:
                owners[inc].append(u)
    assert {h: o for h, o in owners.items() if len(o) != 1} == {}


def test_kernel_headers_hold_no_host_launch_code():
    assert HOST_LAUNCH.search("inline int map_ensure(MapStore &s,\n    hipStream_t st) {").group(1) == "map_ensure"
    assert HOST_LAUNCH.search("__global__ void k(int n) {}\nvoid f(hipStream_t s);") is None
    assert {h: HOST_LAUNCH.findall(read(h)) for h in kernel_headers() if HOST_LAUNCH.search(read(h))} == {}


def test_makefile_units_are_the_hip_files():
    m = re.search(r"^UNITS\s*=\s*(.*)$", read("Makefile"), re.M)
    assert m
    listed = m.group(1).split()
    assert len(listed) == len(set(listed))
    assert sorted(listed) == units()


# ---------------------------------------------------------------- buffer ownership ("Source layout": vba_mem.hpp)
FREE_CALL = re.compile(r"\bhip(?:Host)?Free\s*\(")
# a definition that starts in column 0: `struct Name`, or a function head `... name(`
TOP_LEVEL = re.compile(r"^(?:struct\s+(\w+)|[A-Za-z_][^\n;(]*?(~?\w+)\s*\()", re.M)
ALLOC_CALL = re.compile(r"\bhip(?:Host)?Malloc\s*\(")
# no owner keeps a free list of its own: the voxel map, the global-BA stores, the descriptor generator and the debug entry points'
# scoped DbgBufs hold owning members like everything else
FREE_ALLOWED = {}
# the two stamp buffers of the -DVBA_DIAG build: statics that live as long as the process and are never freed
ALLOC_ALLOWED = {"voxelba.hip": {"k3_stamps_buffer", "k4_stamps_buffer"}}


def call_sites(name, call):
    """{enclosing top-level definition: number of calls matching `call`} of one file"""
    text = read(name)
    heads = [(m.start(), m.group(1) or m.group(2)) for m in TOP_LEVEL.finditer(text)]
    out = {}
    for m in call.finditer(text):
        owner = [h for pos, h in heads if pos < m.start()][-1]
        out[owner] = out.get(owner, 0) + 1
    return out


def function_body(text, head):
    """the text between the braces of the definition whose head `head` matches"""
    i = text.index("{", re.search(head, text, re.M).end() - 1)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i:j + 1]
        j += 1


def test_free_and_allocation_calls_only_in_the_owning_types():
    assert FREE_CALL.search("if (p) hipHostFree (p);") and FREE_CALL.search("hipFree(q)") and not FREE_CALL.search("map_free(s)")
    assert ALLOC_CALL.search("e = hipHostMalloc ((void **)&p, n, 0);") and ALLOC_CALL.search("hipMalloc(&q, n)") and not ALLOC_CALL.search("hipMallocAsync(")
    assert call_sites("vba_mem.hpp", FREE_CALL) == {"Mem": 2} and call_sites("vba_mem.hpp", ALLOC_CALL) == {"Mem": 2}
    files = [f for f in sources() if f != "vba_mem.hpp"]
    assert "vba_stores.hpp" in files and "vba_btcgen.hpp" in files and len(files) > 40
    assert {f: set(call_sites(f, FREE_CALL)) for f in files if call_sites(f, FREE_CALL)} == FREE_ALLOWED
    assert {f: set(call_sites(f, ALLOC_CALL)) for f in files if call_sites(f, ALLOC_CALL)} == ALLOC_ALLOWED


def test_vba_destroy_lists_no_buffers():
    body = function_body(read("voxelba.hip"), r"^void vba_destroy\(vba_ctx \*c\) \{")
    assert "delete c;" in body and "hipStreamDestroy" in body
    assert not FREE_CALL.search(body)
    for handle, unit in (("vba_kf_destroy", "vba_kf.hip"), ("vba_btc_destroy", "vba_btc.hip"), ("vba_scan_frame_destroy", "vba_scan.hip"),
                         ("vba_loop_map_destroy", "vba_loop.hip")):
        assert not FREE_CALL.search(function_body(read(unit), r"^void %s\(\w+ \*\w+\) \{" % handle)), handle
    # the map's memory goes as a whole: map_free names the events it destroys and no buffer
    body = function_body(read("vba_map.hip"), r"^void map_free\(MapStore &s\) \{")
    assert "hipEventDestroy" in body and "MapMem()" in body
    assert not FREE_CALL.search(body) and not re.search(r"\.reset\(\)|\bs\.(?:v\.)?\w+\s*=\s*nullptr", body)
    assert "free_all" not in read("voxelba.hip") and "btcgen_free" not in read("vba_btc.hip")


def test_vba_mem_is_a_shared_header_without_kernels():
    assert "__global__" not in read("vba_mem.hpp")
    assert INCLUDE.findall(read("vba_mem.hpp")) == []          # the runtime's header only
    for u in units():
        direct = INCLUDE.findall(read(u + ".hip"))
        if "vba_mem.hpp" in reached(u + ".hip"):
            assert "vba_ctx.hpp" in direct or "vba_mem.hpp" in direct, u
    assert "vba_mem.hpp" in INCLUDE.findall(read("vba_ctx.hpp"))
    # no unit reaches it through a kernel header: the stores that hold owning members are host code of their own header
    assert [h for h in kernel_headers() if "vba_mem.hpp" in reached(h)] == []
    assert "vba_mem.hpp" in INCLUDE.findall(read("vba_stores.hpp")) and "vba_mem.hpp" not in reached("vba_types.hpp")
    assert [f for f in sources() if f != "vba_ctx.hpp" and "vba_stores.hpp" in INCLUDE.findall(read(f))] == []


# ---------------------------------------------------------------- where state lives ("Source layout": vba_sat.hpp, the handle headers)
HANDLE_HEADERS = ["vba_btc_db.hpp", "vba_kf_store.hpp", "vba_odom_state.hpp", "vba_scanlog.hpp"]
# what the BA core, the map and global BA never see: the satellites' context state, the handle structs and the two headers those pull
SATELLITE_ONLY = ["vba_sat.hpp"] + HANDLE_HEADERS + ["vba_btcgen.hpp", "vba_scanlog_ring.hpp"]
# the fields that left vba_ctx for CtxSat
MOVED_FIELDS = ("d_kdtree kd_n kd_cur d_kdscan kdscan_pts d_kdws kdws_pts kd_allocs kd_bytes d_odom h_odom d_odom_part d_btcq h_btcq d_btccnt "
                "d_icp h_icp d_icpkey d_icppart d_pgo d_pgoAb h_exp exp_ev exp_next d_exp d_expout exp_first exp_kbase vx d_init").split()


def test_the_slow_units_see_no_satellite_state():
    assert all(os.path.exists(os.path.join(CSRC, h)) for h in SATELLITE_ONLY)
    for unit in ("voxelba.hip", "vba_hba.hip"):
        assert sorted(reached(unit) & set(SATELLITE_ONLY)) == [], unit
    # the map launches k_odom_state_pose: it takes the declaration, not the state
    assert sorted(reached("vba_map.hip") & set(SATELLITE_ONLY)) == []
    assert "vba_odom_state_decl.hpp" in INCLUDE.findall(read("vba_map.hip"))
    decl = read("vba_odom_state_decl.hpp")
    assert "k_odom_state_pose" in decl and "struct vba_odom_state" not in decl and reached("vba_odom_state_decl.hpp") == set()
    assert "vba_ctx.hpp" in reached("voxelba.hip") and "vba_ctx.hpp" in reached("vba_hba.hip") and "vba_ctx.hpp" in reached("vba_map.hip")


def test_vba_ctx_holds_the_core_context_alone():
    text = read("vba_ctx.hpp")
    assert re.search(r"^struct vba_ctx \{", text, re.M) and re.search(r"^\s*CtxSat \*sat = nullptr;", text, re.M)
    assert re.findall(r"\bstruct\s+(vba_btc_db|vba_kf_store|vba_scanlog|vba_odom_state)\b", text) == []
    assert [f for f in MOVED_FIELDS if re.search(r"\b%s\b" % f, text)] == []
    assert len(MOVED_FIELDS) == 30 and re.search(r"\bvx\b", "} vx;") and not re.search(r"\bd_exp\b", "c->d_expout")
    assert sorted(reached("vba_ctx.hpp") & set(SATELLITE_ONLY)) == [] and "<mutex>" not in text
    # each handle struct is defined once, in the header named after it
    for h in HANDLE_HEADERS:
        struct = re.compile(r"^struct %s \{" % h[:-4], re.M)
        assert [f for f in sources() if struct.search(read(f))] == [h], h
    assert "vba_btcgen.hpp" in INCLUDE.findall(read("vba_btc_db.hpp"))
    assert "vba_scanlog_ring.hpp" in INCLUDE.findall(read("vba_scanlog.hpp")) and "<mutex>" in read("vba_scanlog.hpp")


def test_ctx_sat_has_one_header_and_a_host_only_unit():
    assert [f for f in sources() if re.search(r"\bstruct\s+CtxSat\s*\{", read(f))] == ["vba_sat.hpp"]
    members = re.findall(r"^  \} (\w+);", read("vba_sat.hpp"), re.M)
    assert members == ["kd", "odom", "btc", "pgo", "exp", "vx", "init"]
    assert "__global__" not in read("vba_sat.hip") and "__global__" not in read("vba_sat.hpp")
    assert [h for h in reached("vba_sat.hip") if h.startswith("vba_kernels_")] == []
    assert sorted(INCLUDE.findall(read("vba_sat.hip"))) == ["vba_ctx.hpp", "vba_sat.hpp"]
    for fn in ("ctx_sat_create", "ctx_sat_release"):
        assert [f for f in sources() if re.search(r"^(?:int|void) %s\(vba_ctx \*c\) \{" % fn, read(f), re.M)] == ["vba_sat.hip"], fn
        assert len(re.findall(r"\b%s\(c\)" % fn, read("voxelba.hip"))) == 1, fn
    # the units that read it are the owners of its members
    users = sorted(u for u in units() if "vba_sat.hpp" in reached(u + ".hip"))
    assert users == ["vba_btc", "vba_init", "vba_kf", "vba_odom", "vba_pgo", "vba_sat"]
    m = re.search(r"^DIAG_UNITS\s*=\s*(.*)$", read("Makefile"), re.M)
    assert m and "vba_sat" not in m.group(1).split()


def test_no_kernel_header_reaches_satellite_state_or_a_handle():
    assert len(kernel_headers()) >= 10
    assert {h: sorted((reached(h) | {h}) & set(SATELLITE_ONLY)) for h in kernel_headers() if (reached(h) | {h}) & set(SATELLITE_ONLY)} == {}
    assert {h: INCLUDE.findall(read(h)) for h in HANDLE_HEADERS + ["vba_sat.hpp"] if any(i.startswith("vba_kernels_") for i in reached(h))} == {}


def test_vba_destroy_releases_the_satellites_and_names_no_export_event():
    body = function_body(read("voxelba.hip"), r"^void vba_destroy\(vba_ctx \*c\) \{")
    assert "delete c;" in body and "hipStreamDestroy" in body
    assert "exp" not in re.sub(r"//[^\n]*", "", body)            # (no export event, ring or table by any spelling)
    # every hipEventDestroy that is left is one of the timing spans'
    assert re.findall(r"hipEventDestroy\(([^)]*)\)", body) == ["s.a", "s.b"]
    # released after the stream has drained and before it is destroyed
    sync, rel, gone = body.index("hipStreamSynchronize(c->stream)"), body.index("ctx_sat_release(c)"), body.index("hipStreamDestroy(c->stream)")
    assert sync < rel < gone < body.index("delete c;")
    # the export's events go with their struct
    exp = function_body(read("vba_sat.hpp"), r"^  struct Exp \{")
    assert re.search(r"~Exp\(\) \{ for \(hipEvent_t e : ev\) if \(e\) hipEventDestroy\(e\); \}", exp)


# ---------------------------------------------------------------- launch plumbing ("Source layout": vba_launch.hpp)
def sources():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))


def test_window_dispatch_and_lds_opt_in_live_in_vba_launch():
    case_macro = re.compile(r"#\s*define\s+VBA_\w+_CASE\b")
    assert case_macro.search("#define VBA_LI_CASE(WW) case WW:") and not case_macro.search("#define VBA_K4_TV 32")
    assert [f for f in sources() if case_macro.search(read(f))] == []
    assert [f for f in sources() if "hipFuncSetAttribute" in read(f)] == ["vba_launch.hpp"]
    assert [f for f in sources() if "attr_set" in read(f)] == []


def test_vba_launch_is_a_shared_header_without_kernels():
    assert "__global__" not in read("vba_launch.hpp")
    assert INCLUDE.findall(read("vba_launch.hpp")) == []       # the runtime's and the standard library's headers only
    assert "vba_launch.hpp" in INCLUDE.findall(read("vba_ctx.hpp"))
    # the units reach it through vba_ctx.hpp and nothing else, no kernel header reaches it
    assert [f for f in sources() if f != "vba_ctx.hpp" and "vba_launch.hpp" in INCLUDE.findall(read(f))] == []
    assert [h for h in kernel_headers() if "vba_launch.hpp" in reached(h)] == []


# ---------------------------------------------------------------- diagnostics run the production code
def test_debug_plane_update_runs_the_production_device_function():
    """vba_debug_plane_update pins plane_update_dev itself: one definition, called by the marginalisation and by the diagnostic
    kernel, whose host launch lives in the unit"""
    text = read("vba_kernels_map.hpp")
    assert len(re.findall(r"void plane_update_dev\(", text)) == 1
    body = function_body(text, r"^__global__ __launch_bounds__\(256\) void k_debug_plane_update\(")
    assert "plane_update_dev(m, id, add, ev, U);" in body
    assert "plane_update_dev(m, id, add, ev, U);" in function_body(text, r"^__device__ __forceinline__ int margi_leaf_body\([^;]*\) \{")
    assert [f for f in sources() if "k_debug_plane_update" in read(f)] == ["vba_kernels_map.hpp", "vba_map.hip"]


def test_debug_pgo_step_runs_the_production_plan_and_launches():
    """vba_debug_pgo_step pins the production pass: the arithmetic is written once, in the host-and-device header that the kernels and
    the g++ companion both compile; the plan, the upload and the launches of one update are each one function, called by
    vba_pgo_optimize and by the diagnostic entry"""
    math, kern, unit = read("vba_pgo_math.hpp"), read("vba_kernels_pgo.hpp"), read("vba_pgo.hip")
    assert "__global__" not in math and INCLUDE.findall(math) == [] and "hipStream_t" not in math
    assert "hip" not in read("vba_pgo_plan.hpp") and INCLUDE.findall(read("vba_pgo_plan.hpp")) == []
    for fn in ("pgo_coeffs", "pgo_exp", "pgo_log", "pgo_jrinv", "pgo_linearize_factor", "pgo_assemble_block", "pgo_ldl6", "pgo_ldl6_solve",
               "pgo_seg_elim", "pgo_seg_back", "pgo_skel_scatter_block", "pgo_retract"):
        assert len(re.findall(r"^VBE_HD \w+ %s\(" % fn, math, re.M)) == 1, fn
        assert [f for f in sources() if re.search(r"^\w[\w ]* %s\(" % fn, read(f), re.M)] == ["vba_pgo_math.hpp"], fn
    for call in ("pgo_linearize_factor(v, f);", "pgo_assemble_block(v, b);", "pgo_seg_elim(v, s)", "pgo_seg_back(v, s);",
                 "pgo_skel_scatter_block(v, b);", "pgo_retract(d, v.theta + (size_t)k * 12);"):
        assert call in kern, call
    assert "vba_pgo_math.hpp" in INCLUDE.findall(kern) and [f for f in sources() if "vba_pgo_math.hpp" in INCLUDE.findall(read(f))] == ["vba_kernels_pgo.hpp"]
    assert len(re.findall(r"hipLaunchKernelGGL\(k_pgo_linearize", unit)) == 1 and len(re.findall(r"= pgo_plan\(", unit)) == 1
    for entry in (r"^int vba_pgo_optimize\(", r"^int vba_debug_pgo_step\("):
        body = function_body(unit, entry)
        assert "pgo_prepare(c, n, poses, m, edges, n_prior, priors," in body and "pgo_update(c, v, " in body and "hipLaunchKernelGGL" not in body
    host = open(os.path.join(os.path.dirname(CSRC), "..", "tests", "host", "pgo_host.cpp")).read()
    assert "csrc/vba_pgo_math.hpp" in host and "csrc/vba_pgo_plan.hpp" in host


def test_debug_btc_icp_pass_runs_the_production_pass():
    """vba_debug_btc_icp_pass pins the production iteration: the per-point and per-step arithmetic is written once, in the
    host-and-device header that the kernels and the g++ companion both compile; the plan and the three launches of one iteration are
    one function, called by the loop of vba_btc_icp_normal and by the diagnostic entry"""
    math, kern, unit = read("vba_icp_math.hpp"), read("vba_kernels_btc.hpp"), read("vba_btc.hip")
    assert "__global__" not in math and "hipStream_t" not in math and "__shfl" not in math
    assert sorted(INCLUDE.findall(math)) == ["vba_btc_svd.hpp", "vba_hostmath.hpp", "vba_ldlt6.hpp"]
    for fn in ("btc_norm3", "btc_icp_query", "btc_icp_point", "btc_icp_solve_update", "btc_icp_transition"):
        assert len(re.findall(r"^BTC_HD [\w() ]+ %s\(" % fn, math, re.M)) == 1, fn
        assert [f for f in sources() if re.search(r"^\w[\w() ]* %s\(" % fn, read(f), re.M)] == ["vba_icp_math.hpp"], fn
    for kernel, call in (("k_btc_icp_nn", "btc_icp_query(st->R, st->t, "), ("k_btc_icp_accum", "btc_icp_point(st->R, st->t, st->paras, "),
                         ("k_btc_icp_step", "btc_icp_solve_update(acc, st->R, st->t, st->mat, dx);"),
                         ("k_btc_icp_step", "btc_icp_transition(dx, st->paras, &st->is_conv, &st->done, &st->iters);")):
        assert call in function_body(kern, r"^__global__ __launch_bounds__\(\d+\) void %s\(" % kernel), (kernel, call)
    assert [f for f in sources() if "vba_icp_math.hpp" in INCLUDE.findall(read(f))] == ["vba_kernels_btc.hpp"]
    for k in ("k_btc_icp_nn<<<", "k_btc_icp_accum<<<", "k_btc_icp_step<<<"):
        assert len(re.findall(re.escape(k), unit)) == 1 and k in function_body(unit, r"^static int btc_icp_pass\("), k
    # the slice plan is a pure function (the entry's refusal touches nothing); the pass plans, sizes and launches
    plan = function_body(unit, r"^static bool btc_icp_plan\(")
    assert "grow_keep" not in plan and "c->" not in plan and len(re.findall(r"btc_icp_plan\(cl, ", unit)) == 2
    body = function_body(unit, r"^static int btc_icp_pass\(")
    assert "btc_icp_plan(cl, want, &p)" in body and "btc_icp_ensure(c, cl, p)" in body
    for entry in (r"^int vba_btc_icp_normal\(", r"^int vba_debug_btc_icp_pass\("):
        body = function_body(unit, entry)
        assert "btc_icp_pass(c, cl, " in body and "<<<" not in body, entry
    assert "it < BTC_ICP_ITERS" in function_body(unit, r"^int vba_btc_icp_normal\(")
    host = open(os.path.join(os.path.dirname(CSRC), "..", "tests", "host", "icp_host.cpp")).read()
    assert "csrc/vba_icp_math.hpp" in host


# ---------------------------------------------------------------- the BA core's host side ("Source layout": voxelba.hip)
# a macro definition with its continuation lines: (name, body)
MACRO = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)((?:[^\n]*\\\n)*[^\n]*)", re.M)


def macros(name):
    return {m.group(1): m.group(2) for m in MACRO.finditer(read(name))}


def test_one_hip_check_macro():
    assert MACRO.search("#define A(x) do { \\\n  f(x); \\\n} while (0)\nint y;").group(2).endswith("while (0)")
    builders, users = [], []
    for f in sources():
        for name, body in macros(f).items():
            if "hipGetErrorString" in body and "VBA_ERR_HIP" in body:
                builders.append((f, name))
            elif "VBA_HIPCHK" in body:
                users.append((f, name, body.strip()))
    assert builders == [("vba_ctx.hpp", "VBA_HIPCHK")]
    assert users == [("vba_ctx.hpp", "HIPCHK", "VBA_HIPCHK")]
    # no unit keeps a check macro of its own; BGCHK hands the runtime's status on and builds no message
    own = sorted((f, n) for f in sources() for n in macros(f) if n.endswith("CHK"))
    assert own == [("vba_btcgen.hip", "BGCHK"), ("vba_ctx.hpp", "HIPCHK"), ("vba_ctx.hpp", "VBA_HIPCHK")]
    assert "hipGetErrorString" not in macros("vba_btcgen.hip")["BGCHK"]
    for f in ("vba_map.hip", "vba_hba.hip"):
        assert len(re.findall(r"\bVBA_HIPCHK\(err, ", read(f))) > 50, f


def test_core_call_paths_hold_no_printing():
    text = read("voxelba.hip")
    for head in (r"^int launch_residual\(", r"^int vba_lm_end\(", r"^static int li_ba_device\("):
        body = function_body(text, head)
        assert len(body) > 500 and "printf" not in body and "stderr" not in body, head
    assert "fprintf" in function_body(text, r"^void k4_stamps_dump\(")       # (the search does see a printer)


def test_sharded_trial_step_is_written_once():
    text = read("voxelba.hip")
    trial = re.compile(r"d_out\s*\+\s*\(\s*nout_tl\(")
    assert trial.search("c->d_out + (nout_tl(W) - 1)")
    step = function_body(text, r"^int sharded_trial_step\(")
    assert len(trial.findall(text)) == 1 and len(trial.findall(step)) == 1
    assert "k_lm_update" not in step and "k_li_update" not in step and "launch_update(" in step
    for head, kernel in ((r"^int vba_lm_iterate\(", "k_lm_update"), (r"^static int li_ba_device\(", "k_li_update")):
        body = function_body(text, head)
        m = re.search(r"sharded_trial_step\(c, p, V, \[&\]\(const double \*r\) \{ hipLaunchKernelGGL\((\w+),", body)
        assert m and m.group(1) == kernel, head
        assert "have_hess = true" not in body
    # "this rank still needs a Hessian pass" is one predicate
    assert len(re.findall(r"lm\.have_hess\)", text)) == 1 and "lm.have_hess)" in function_body(text, r"^bool needs_hessian_pass\(")
    for head in (r"^int vba_lm_iterate\(", r"^static bool li_imu_rides\(", r"^static int li_ba_device\("):
        assert "needs_hessian_pass(c)" in function_body(text, head), head


# ---------------------------------------------------------------- compaction, scan and var_world helpers ("Source layout": vba_common.hpp)
WG_HELPERS = ("wg_rank", "wg_count", "wg_append", "wg_scan_chunked", "wg_scan_strided", "var_world")


def kernel_body(name, kernel):
    return function_body(read(name), r"^__global__ __launch_bounds__\(\d+\) void %s\(" % kernel)


def test_workgroup_helpers_are_written_once_in_vba_common():
    for fn in WG_HELPERS:
        head = re.compile(r"^(?:\w+ )*(?:void|int) %s\(" % fn, re.M)
        assert head.search("__device__ __forceinline__ int %s(bool f" % fn) and not head.search("  const int r = %s(f, wsum, tot);" % fn)
        assert {f: len(head.findall(read(f))) for f in sources() if head.search(read(f))} == {"vba_common.hpp": 1}, fn
    assert [f for f in sources() if re.search(r"\bdet_wg_rank\b|\bdet_count\b", read(f))] == []
    assert "__global__" not in read("vba_common.hpp")


def test_count_and_emit_kernels_rank_through_the_helpers():
    for name, kernel, call in (("vba_kernels_scan.hpp", "k_ds_count", "wg_count("), ("vba_kernels_scan.hpp", "k_ds_emit", "wg_rank("),
                               ("vba_kernels_kf.hpp", "k_kf_emit", "wg_rank("), ("vba_kernels_init.hpp", "k_initw_count", "wg_count("),
                               ("vba_kernels_init.hpp", "k_initw_gather", "wg_rank("), ("vba_kernels_map.hpp", "k_fix_heads", "wg_append("),
                               ("vba_kernels_decode.hpp", "k_scan_decode", "wg_count(")):
        body = kernel_body(name, kernel)
        assert "__ballot(" not in body and "__popcll(" not in body and body.count(call) == 1, kernel
    # the emit kernels return their unflagged threads after the helper's barrier, never before it
    for name, kernel in (("vba_kernels_scan.hpp", "k_ds_emit"), ("vba_kernels_kf.hpp", "k_kf_emit"), ("vba_kernels_init.hpp", "k_initw_gather")):
        body = kernel_body(name, kernel)
        assert "return" not in body[:body.index("wg_rank(")] and "if (!f) return;" in body[body.index("wg_rank("):], kernel
    # the three list appends of the map: one per kernel, on its own counter
    text = read("vba_kernels_map.hpp")
    assert re.findall(r"wg_append\(\w+, wbase, &m\.cnt\[(\w+)\]\)", text) == ["CNT_WL", "CNT_SPLIT", "CNT_FACTORS"]
    assert len(re.findall(r"\bwg_append\(", "".join(read(f) for f in sources()))) == 4          # (and the definition)


def test_one_workgroup_scans_are_wrappers():
    for name, kernel, call in (("vba_kernels_map.hpp", "k_det_scan", "wg_scan_chunked(a, n, buf, wsum)"),
                               ("vba_btcgen.hip", "k_bg_scan", "wg_scan_chunked(a, n, buf, wsum)"),
                               ("vba_kernels_scan.hpp", "k_ds_scan", "wg_scan_strided(nb, blk, blk, part)"),
                               ("vba_kernels_big.hpp", "k_big_scan", "wg_scan_strided(n, in, out, part)")):
        body = kernel_body(name, kernel)
        assert "__shfl_up" not in body and not re.search(r"\bfor\b", body) and body.count(call) == 1, kernel
        assert re.findall(r"part\[", body) in ([], ["part["]), kernel                        # (its declaration at the most)
    assert "k_det_scan's algorithm" not in read("vba_btcgen.hip")


def test_var_world_is_called_by_both_stagings():
    for name, kernel in (("vba_kernels_init.hpp", "k_init_blur"), ("vba_kernels_map.hpp", "k_scan_to_soa_pvec_update")):
        body = kernel_body(name, kernel)
        assert body.count("var_world(") == 1 and "ph[" not in body and "PR[" not in body and "RV[" not in body, kernel
    fn = function_body(read("vba_common.hpp"), r"^__device__ __forceinline__ void var_world\(")
    assert "#pragma clang fp contract(off)" in fn and "ph[3 * r]" in fn
    # the calcBodyVar half stays a twin (default contraction in k_var_init, contract(off) in k_init_blur): DESIGN.md says so
    assert "#pragma clang fp contract(off)" in kernel_body("vba_kernels_init.hpp", "k_init_blur")


# ---------------------------------------------------------------- the drivers of vba_hba_global ("Source layout": vba_hba.hip)
def test_hba_plan_is_a_device_free_header_of_one_unit():
    plan = read("vba_hba_plan.hpp")
    assert "hip" not in plan and INCLUDE.findall(plan) == [] and "vba_ctx" not in plan and "__global__" not in plan
    assert [f for f in sources() if "vba_hba_plan.hpp" in INCLUDE.findall(read(f))] == ["vba_hba.hip"]
    host = open(os.path.join(os.path.dirname(CSRC), "..", "tests", "host", "hba_plan_host.cpp")).read()
    assert "csrc/vba_hba_plan.hpp" in host
    assert [f for f in sources() if "std::thread" in read(f)] == ["vba_hba_plan.hpp"]


def test_hba_global_pieces_are_written_once():
    unit = read("vba_hba.hip")
    add_edge = re.compile(r"\bvba_hba_add_edge\(")
    assert add_edge.search("const int st = vba_hba_add_edge(cx, P.wdsize,") and not add_edge.search("// (vba_gba_build, vba_hba_add_edge, vba_hba_global)")
    assert call_sites("vba_hba.hip", add_edge) == {"vba_hba_add_edge": 1, "hba_window": 1, "hba_top": 1}         # (its own head, and two calls)
    shift = re.compile(r"\bo\[[01]\]\s*\+=")
    assert shift.search("o[0] += start; o[1] += start;") and not shift.search("o[0] = i; o[1] = j;")
    assert not shift.search(unit)
    assert call_sites("vba_hba.hip", re.compile(r"\bhba_append_edges\(")) == {"hba_collect": 1, "hba_bottom_sequential": 1, "hba_top": 1}
    assert len(re.findall(r"^inline int hba_append_edges\(", read("vba_hba_plan.hpp"), re.M)) == 1
    # the record index is the plan's: no product with meta_chunk in the unit (a byte count for a copy is not an index)
    product = re.compile(r"\bmeta_chunk\s*\*(?!\s*sizeof\b)|\*\s*(?:\(\w+\)\s*)?(?:\w+(?:\.|->))*meta_chunk\b")
    assert product.search("meta[(size_t)(w % NR) * meta_chunk + 2]") and product.search("d_meta + P.meta_chunk * (size_t)rank") and product.search("NR * P.meta_chunk")
    assert not product.search("P.meta_chunk * sizeof(double)") and not product.search("ctx_allgather(c, d_meta, P.meta_chunk)")
    assert not product.search(unit)
    # the early stop is wired into the worker driver through the header's pieces, which tests/host/hba_plan_host.cpp runs
    workers = function_body(unit, r"^static int hba_bottom_workers\(")
    for call in ("hba_gate(kf_ready, P.win[w].start + P.wdsize, stop_after, w)", "hba_stop_at(stop_after, w)", "hba_upload_wanted(P, stop_after.load(), k0)",
                 "hba_run_lanes(P.KL, stop_after, work, upload)", "stop_after{P.n_win}"):
        assert workers.count(call) == 1, call
    body = function_body(unit, r"^int vba_hba_global\(")
    assert "hba_plan(" in body and "d_hba_all.ensure(P.need)" in body and "hba_top(" in body
    for driver in ("hba_bottom_sequential", "hba_bottom_workers", "hba_bottom_replicas"):
        assert driver + "(" in body and len(re.findall(r"^static int %s\(" % driver, unit, re.M)) == 1, driver
    assert "for (" not in body and "hipMemcpyAsync" not in body


# ---------------------------------------------------------------- the frame of an odometry update ("Source layout": vba_odom.hip)
ODOM_ENTRIES = ("vba_odom_lio_state_estimation_resident", "vba_odom_lio_state_estimation_kdtree_resident", "vba_odom_surfel_update",
                "vba_odom_lio_state_estimation_on_state", "vba_odom_lio_state_estimation_kdtree_on_state", "vba_odom_surfel_update_on_state")


def launches(kernel):
    """{file: launches of `kernel` in either spelling} over csrc/"""
    pat = re.compile(r"hipLaunchKernelGGL\(\s*\(?%s\b|\b%s\s*<<<" % (kernel, kernel))
    assert pat.search("hipLaunchKernelGGL(%s, dim3(1)," % kernel) and pat.search("%s<<<nb, 256, 0, st>>>(n)" % kernel)
    assert not pat.search("hipLaunchKernelGGL(%s_dev, dim3(1)," % kernel) and not pat.search("// the reduction of %s stored" % kernel)
    return {f: len(pat.findall(read(f))) for f in sources() if pat.search(read(f))}


def test_odometry_frame_is_written_once():
    assert launches("k_odom_update") == {"vba_odom.hip": 1}
    assert launches("k_odom_commit_dev") == {"vba_odom.hip": 1}
    assert launches("k_odom_sums") == {"vba_odom.hip": 1}
    rng = re.compile(r"offsetof\(\s*vbh::OdomEkf\s*,\s*x_curr\s*\)")
    assert rng.search("r0 = offsetof(vbh::OdomEkf, x_curr), r1") and not rng.search("offsetof(vbh::OdomEkf, R)")
    assert {f: len(rng.findall(read(f))) for f in sources() if rng.search(read(f))} == {"vba_odom.hip": 1}
    unit = read("vba_odom.hip")
    assert "k_odom_update" in function_body(unit, r"^static int odom_loop_queue\(") and "k_odom_sums" in function_body(unit, r"^static int odom_sums_run\(")
    assert "k_odom_commit_dev" in function_body(unit, r"^static int odom_end_state\(")
    assert rng.search(function_body(unit, r"^static int odom_result_download\("))


def test_the_map_exports_its_point_loop_alone():
    gone = re.compile(r"\bmap_odom_(?:resident|queue|debug_sums)\b")
    assert gone.search("st = map_odom_queue(c->map, s") and not gone.search("nb = map_odom_point_loop(s, st")
    assert [f for f in sources() if gone.search(read(f))] == []
    assert re.findall(r"\bmap_odom_\w+", read("vba_ctx.hpp")) == ["map_odom_point_loop"]
    # the map unit uploads no image and downloads no result block
    img = re.compile(r"hipMemcpyAsync\([^;]*\bOdomEkf\b")
    assert img.search("VBA_HIPCHK(err, hipMemcpyAsync(d_S, h_img, sizeof(vbh::OdomEkf), hipMemcpyHostToDevice, st));")
    assert not img.search("hipMemcpyAsync(a, b, n, hipMemcpyDefault, st);\n  const vbh::OdomEkf *d_S;")
    assert not img.search(read("vba_map.hip")) and img.search(read("vba_odom.hip"))
    assert sorted(reached("vba_map.hip") & set(SATELLITE_ONLY)) == []


def test_odometry_entry_points_run_the_frame():
    unit = read("vba_odom.hip")
    launch = re.compile(r"hipLaunchKernelGGL\(\s*k_odom_update\b")
    assert launch.search(function_body(unit, r"^static int odom_loop_queue\("))        # (the search does see the launch)
    for entry in ODOM_ENTRIES:
        body = function_body(unit, r"^int %s\(" % entry)
        assert len(body) > 300 and not launch.search(body) and "offsetof" not in body, entry
