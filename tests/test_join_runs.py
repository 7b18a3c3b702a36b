"""Host half of mchecksum_gpu_combine_runs: the join over (register, length)
elements the kernel runs (mercury_amd/csrc/crc_gpu_seed.h) against the
streaming API, on the CPU, in every bracketing that keeps the chunks in order
-- the kernel's own included (tests/native/test_join_runs.c)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "test")
CPU_SRC = [os.path.join(ROOT, "mercury_amd", "csrc", f) for f in ("mchecksum_cpu.c", "mchecksum_models.c",
                                                                   "crc_tables.c")]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mercury_amd", "csrc")]


def test_join_algebra_in_every_bracketing():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "test_join_runs")
    src = os.path.join(ROOT, "tests", "native", "test_join_runs.c")
    subprocess.run(["gcc", "-O2", "-std=c11", "-Wall", *INC, src, *CPU_SRC, "-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
