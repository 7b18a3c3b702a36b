"""The message calls' rules in mercury_amd/csrc/seg_plan.h (seg_msg_layout,
seg_msg_fits, seg_msg_gate, seg_msg_seal_decide, seg_msg_open_decide) walked on
the CPU by tests/native/segmsg_plan.cpp over random tables: fit decisions and
the accumulator / gate slots against a naive model, with objects without
segments, objects of empty segments, messages one byte long and one byte
short, and messages shorter than payload_offset among them.  Run plain and
under AddressSanitizer + UBSan (a stand-alone program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name,flags", [
    ("segmsg_plan", ["-O2"]),
    ("segmsg_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_segmsg_plan_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "segmsg_plan.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # every kind of message the issue names was among the tables, not vacuously
    m = re.search(r"(\d+) tables, (\d+) messages: (\d+) fit, (\d+) do not; (\d+) without segments, (\d+) all empty, "
                  r"(\d+) one byte long, (\d+) one byte short, (\d+) shorter than the headers", r.stdout)
    assert m and all(int(g) > 100 for g in m.groups()), r.stdout
