"""The launch plan (launch_plan.h: which batch kernel a call launches, with how
many lanes per payload, which grid, and whether it takes a work-queue slot)
checked on the host, with the host compiler, against a table of literal expectations: the headline, C2
and C3 shapes, both sides of every threshold, every override setting, and that
a plan depends only on the settings snapshot passed in.  The GPU side is the
parity tests, which run the kernels these plans select."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "launch_plan.cpp")


def test_launch_plan_matches_the_recorded_policy(tmp_path):
    exe = str(tmp_path / "launch_plan")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc"), SRC,
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout
