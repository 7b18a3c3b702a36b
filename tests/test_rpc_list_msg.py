"""The RPC message calls by address list, walked on the CPU by
tests/native/rpc_list_msg.cpp: the rules the kernels run
(mercury_amd/csrc/launch_plan.h) and a plain emulation of what each of the four
calls reads and writes of a list, against a model written from the header text
-- both kinds, L = 0 .. payload_offset + 8, R = L - payload_offset - 1 .. + 1,
every message alone in an exactly sized heap allocation, the allocations handed
over in shuffled order, a NULL address for every message shorter than a core
header, and both arrays of exactly `count` entries.  Then the key space (the
list field names twelve kernels and moves no pinned count) and the host
front's call shape.  Run plain and under AddressSanitizer + UBSan (a
stand-alone program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name,flags", [
    ("rpc_list_msg", ["-O2"]),
    ("rpc_list_msg_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_rpc_list_msg_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "rpc_list_msg.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # every verdict was among them, not vacuously
    m = re.search(r"(\d+) messages: ok (\d+) payload (\d+) header (\d+) short (\d+) deferred (\d+) misfit (\d+)", r.stdout)
    assert m and all(int(g) >= 100 for g in m.groups()), r.stdout
