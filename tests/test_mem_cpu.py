"""The owning buffer types of csrc/vba_mem.hpp on the CPU: tests/host/mem_host.cpp is built by g++ with the address and
undefined-behaviour sanitizers against the runtime's headers only (its own stubs stand in for the eight runtime calls, nothing of the
HIP runtime is linked) and run as a child process, one case per run.  Every case also fails when a block is still live at its end."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def mem_host():
    out = os.path.join(tempfile.mkdtemp(prefix="vba_mem_"), "mem_host")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I" + ROCM_INCLUDE, "-o", out, os.path.join(HERE, "host", "mem_host.cpp")])
    return out


@pytest.mark.parametrize("case", ["ensure", "failed_ensure", "move", "reset", "grow_keep", "grow_keep_alloc_fails", "grow_keep_copy_fails",
                                  "family_grow", "family_alloc_fails", "family_copy_fails"])
def test_mem(mem_host, case):
    r = subprocess.run([mem_host, case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""                     # no sanitizer report, no leak report at exit


def test_unknown_case_is_an_error(mem_host):
    assert subprocess.run([mem_host, "no_such_case"], capture_output=True, timeout=60).returncode == 2
