"""The copy kernels' key (copy_plan.h: which of the 10 copy kernels a
copy_offsets / update_copy_offsets call launches) checked on the host, with the
host compiler: the light / full / non-temporal thresholds of the offsets plan
for both widths and both operations, the MCHECKSUM_GPU_LIGHT and _NT overrides,
and that copy_key_valid states exactly the 10 kernels there are.  The GPU side
is tests/test_gpu_copy.py, which runs every one of them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "copy_plan.cpp")


def test_copy_plan_matches_the_recorded_policy(tmp_path):
    exe = str(tmp_path / "copy_plan")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc"), SRC,
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
