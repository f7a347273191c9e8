"""The launch plumbing of csrc/vba_launch.hpp on the CPU: the window dispatch for_window and the per-device LDS opt-in.
tests/host/launch_host.cpp is built by g++ against the runtime's headers only (its own stub stands in for hipFuncSetAttribute, nothing
of the HIP runtime is linked), once with the address and undefined-behaviour sanitizers and once with the thread sanitizer, and run
as a child process, one case per run."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SANITIZERS = {"asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
CASES = ["window_2_16", "window_2_10", "opt_in", "opt_in_failure", "opt_in_out_of_range", "opt_in_instances", "opt_in_threads"]


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def launch_host(request):
    out = os.path.join(tempfile.mkdtemp(prefix="vba_launch_"), "launch_host_" + request.param)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-pthread"] + SANITIZERS[request.param] +
                          ["-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-o", out, os.path.join(HERE, "host", "launch_host.cpp")])
    return out


@pytest.mark.parametrize("case", CASES)
def test_launch(launch_host, case):
    r = subprocess.run([launch_host, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""                     # no sanitizer report (no data race in the threaded case)


def test_unknown_case_is_an_error(launch_host):
    assert subprocess.run([launch_host, "no_such_case"], capture_output=True, timeout=60).returncode == 2
