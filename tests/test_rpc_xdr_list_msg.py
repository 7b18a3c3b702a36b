"""The frame of the RPC message calls of an XDR build by address list
(mercury_amd/csrc/launch_plan.h: rpc_xdr_list_len, rpc_xdr_list_at, around the
table form's ladders and gates -- the code the kernels run) walked on the CPU
by tests/native/rpc_xdr_list_msg.cpp against a model written from the
contract: every class of every ladder for both kinds, L at 0, 15, 16,
payload_offset - 1 and from payload_offset on, entries at NULL and entries
whose end wraps the address space, every message byte read and written through
an accessor that aborts outside what the contract allows for the class.  Run
plain and under AddressSanitizer + UBSan (a stand-alone program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name,flags", [
    ("rpc_xdr_list_msg", ["-O2"]),
    ("rpc_xdr_list_msg_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_rpc_xdr_list_msg_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "rpc_xdr_list_msg.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # every verdict, both kinds of empty entry and the header-only reads were among them, not vacuously
    m = re.search(r"(\d+) messages: ok (\d+) payload (\d+) header (\d+) short (\d+) deferred (\d+); unpack misfit (\d+); "
                  r"null (\d+) wrapped (\d+) header-only (\d+)", r.stdout)
    assert m and all(int(g) >= 100 for g in m.groups()), r.stdout
