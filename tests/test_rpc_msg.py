"""The RPC message calls' rules (mercury_amd/csrc/launch_plan.h:
rpc_verify_class, rpc_seal_class, rpc_hashes_payload and the header pack's
per-byte CRC-16 terms -- the code the kernels run) walked on the CPU by
tests/native/rpc_msg.cpp against a model written from the contract: both
kinds, L = 0 .. payload_offset + 8, (payload_offset, hash_offset) = (20, 16),
(24, 16), (21, 17), MORE_DATA set and clear, each hash right and wrong, every
message alone in an exactly sized allocation.  Run plain and under
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
    ("rpc_msg", ["-O2"]),
    ("rpc_msg_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_rpc_msg_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "rpc_msg.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # every verdict was among them, not vacuously
    m = re.search(r"(\d+) messages: ok (\d+) payload (\d+) header (\d+) short (\d+) deferred (\d+)", r.stdout)
    assert m and all(int(g) >= 100 for g in m.groups()), r.stdout
