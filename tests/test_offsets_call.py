"""The call shape of every offsets-shaped entry point (mercury_amd/csrc/
offsets_call.h: what a call must supply, whether its method is checked ahead of
the device, and the kernels' argument it becomes -- the code
mchecksum_gpu.hip's offsets_call runs) checked on the CPU by
tests/native/offsets_call.cpp against a table written out by hand: each of the
thirteen entry points, every union member of BatchArgs by name, the 64-bit RPC
payload offset, bswap only for an MSB-first verify.  Run plain and under
AddressSanitizer + UBSan (a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name,flags", [
    ("offsets_call", ["-O2"]),
    ("offsets_call_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_offsets_call_shapes(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "offsets_call.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "13 call shapes: all checks passed" in r.stdout
