"""The source layout of libvoxelba.so as DESIGN.md states it ("Source layout"): one object per csrc/*.hip unit, every kernel header
compiled by exactly one unit, host launch code in the units and not in the kernel headers.  A text check over include lines, function
heads and file names; nothing is compiled."""
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
