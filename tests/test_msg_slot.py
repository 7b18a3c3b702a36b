"""The detached message calls' slot rule (mercury_amd/csrc/launch_plan.h:
msg_slot_ok, msg_slot_at -- which eager messages carry their four hash bytes,
and where) walked on the CPU by tests/native/msg_slot.cpp against a naive
model: message lengths 0 .. hash_offset + 8 for hash_offset in {0, 1, 16, 17},
every message alone in an exactly sized allocation, so a byte read or written
past a short message's end is the sanitizer's.  Run plain and under
AddressSanitizer + UBSan (a stand-alone program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name,flags", [
    ("msg_slot", ["-O2"]),
    ("msg_slot_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_msg_slot_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "msg_slot.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # both kinds of message were among them, not vacuously
    m = re.search(r"(\d+) messages: (\d+) with a slot, (\d+) without", r.stdout)
    assert m and int(m.group(2)) >= 4 * 5 * 16 and int(m.group(3)) >= 4 * 4 * 16, r.stdout
