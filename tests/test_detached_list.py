"""The detached calls with both sides by address list, walked on the CPU by
tests/native/detached_list.cpp: the rules the kernels run
(mercury_amd/csrc/launch_plan.h) and a plain emulation of what a wave reads and
writes per entry, against a model written from the header text -- hash_offset
16 and 13, L = 0 .. hash_offset + 8, every message and every payload alone in
an exactly sized heap allocation, the allocations handed over in shuffled
order, a NULL address for every slotless message and every empty payload, all
four arrays of exactly `count` entries, and both wrap cases.  Then the key
space (the both_lists field names six kernels and moves no pinned count) and
the host front's call shape.  Run plain and under AddressSanitizer + UBSan (a
stand-alone program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
# what the walk holds of each verdict by construction (two hash offsets): five lengths with a slot x eight
# non-empty payloads sealed and left alone, ... x one flipped payload bit, five x nine with a flipped slot bit,
# every L < hash_offset + 4, five x two empty payloads with a good slot, and 32 x 2 wraps
AT_LEAST = {"good": 80, "payload": 80, "slot": 90, "noslot": 900, "empty": 20, "wrapped": 128}


@pytest.mark.parametrize("name,flags", [
    ("detached_list", ["-O2"]),
    ("detached_list_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_detached_list_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "detached_list.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # every verdict was among them, not vacuously
    m = re.search(r"(\d+) entries: good (\d+) payload (\d+) slot (\d+) noslot (\d+) empty (\d+) wrapped (\d+)", r.stdout)
    assert m, r.stdout
    got = dict(zip(["good", "payload", "slot", "noslot", "empty", "wrapped"], map(int, m.groups()[1:])))
    assert all(got[k] >= v for k, v in AT_LEAST.items()), (got, r.stdout)
