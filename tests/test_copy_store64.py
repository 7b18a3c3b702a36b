"""Which bytes the CRC-64 copy kernels' payload loops store, and where: the
rule the kernels compile (mercury_amd/csrc/crc_gpu_pack_store.h) walked on the
CPU over the 8-byte-word window geometry, for every source residue x
destination residue x length (tests/native/test_copy_store64.cpp) -- every
payload byte written exactly once, nothing else written, every piece called
clean wholly inside the payload.  Run plain and under AddressSanitizer + UBSan
(a stand-alone program: the sanitizers see the walk's own loads and stores)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra"]


@pytest.mark.parametrize("name,flags", [
    ("test_copy_store64", ["-O2"]),
    ("test_copy_store64_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_copy_store64_rule(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "test_copy_store64.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # 16 x 16 residues x (2101 + 3) lengths, both payload loops
    assert r.stdout.startswith("538624 cases,"), r.stdout
