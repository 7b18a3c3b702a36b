"""Host half of the streaming and verifying segment calls
(mchecksum_gpu_update_segments and its gather / scatter forms,
mchecksum_gpu_verify_segments, mchecksum_gpu_state_verify): the code the
kernels share with the host, run on the CPU.

* tests/native/test_seg_update.c: the seed term an update call presets
  (crc_gpu_seed.h, mck_seg_seed) plus the chunk pass's contributions, staged
  over random segmentations, against the oracle's streaming register.
* tests/native/seg_verify.cpp: the fail-closed decision of the compare and the
  place of its values in the workspace (seg_plan.h), plain and as a
  stand-alone program under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
CSRC = os.path.join(ROOT, "mercury_amd", "csrc")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def test_segment_update_algebra_against_the_oracle():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "test_seg_update")
    srcs = [os.path.join(ROOT, "tests", "native", "test_seg_update.c"), os.path.join(ROOT, "oracle", "crc_oracle.c"),
            *(os.path.join(CSRC, f) for f in ("mchecksum_cpu.c", "mchecksum_models.c", "crc_tables.c"))]
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", *INC, "-I" + os.path.join(ROOT, "oracle"), *srcs, "-o", exe,
                    "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    m = re.search(r"(\d+) stages \((\d+) without bytes\), (\d+) segments", r.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), r.stdout


@pytest.mark.parametrize("name,flags", [
    ("seg_verify", ["-O2"]),
    ("seg_verify_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_verify_decision_fails_closed(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "seg_verify.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
