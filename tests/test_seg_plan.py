"""The arithmetic of the segment passes (mercury_amd/csrc/seg_plan.h) walked on
the CPU by tests/native/seg_plan.cpp.  Where the gather / scatter kernels put
every chunk of a scatter-gather object: the chunk cut and the store rule
(crc_gpu_pack_store.h) over random segment lists, in both directions and both
window geometries -- every destination byte written exactly once with the
right source byte, no guard byte touched.  The workspace layout against the
closed form of the ABI.  The chunk record of the in-order walk and of the
random-access locate: equal to a brute-force reference on a trusted scan's
tables, and inside the caller's memory on tables that cannot be trusted.  Run
plain and under AddressSanitizer + UBSan (a stand-alone program: the
sanitizers see the walk's own loads and stores)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]
CXX = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.mark.parametrize("name,flags", [
    ("seg_plan", ["-O2"]),
    ("seg_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
])
def test_seg_plan_walk(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    src = os.path.join(ROOT, "tests", "native", "seg_plan.cpp")
    subprocess.run([*CXX, *flags, *INC, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    # (4 + 3 * 8 shapes) x {whole list, sub-range} x 2 directions x 2 geometries
    assert r.stdout.startswith("224 layouts,"), r.stdout
    # the record checks ran, and the stale-table runs were not vacuous: some
    # records were yielded (and checked) and some skipped
    m = re.search(r"(\d+) records of trusted scans; stale tables: (\d+) records yielded, (\d+) skipped", r.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), r.stdout
