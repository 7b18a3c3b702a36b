"""The rules of the RPC message calls of an XDR build (mercury_amd/csrc/
launch_plan.h: rpc_xdr_verify_class, rpc_xdr_seal_class, rpc_xdr_unpack_class,
rpc_xdr_pack_class and the tests that decide whether a walk starts -- the code
the kernels run) walked on the CPU by tests/native/rpc_xdr_msg.cpp against a
model written from the contract: both kinds, L = 0 .. payload_offset + 20 with
the schema ending one byte past the message, at its end and with slack, the
other range one byte short, exact and one byte long, MORE_DATA set and clear,
each hash right and wrong, every buffer alone in an exactly sized allocation.
Run plain and under AddressSanitizer + UBSan (a stand-alone program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name,flags", [
    ("rpc_xdr_msg", ["-O2"]),
    ("rpc_xdr_msg_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_rpc_xdr_msg_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "rpc_xdr_msg.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # every verdict was among them, not vacuously
    m = re.search(r"(\d+) messages: ok (\d+) payload (\d+) header (\d+) short (\d+) deferred (\d+); unpack misfit (\d+)",
                  r.stdout)
    assert m and all(int(g) >= 100 for g in m.groups()), r.stdout
