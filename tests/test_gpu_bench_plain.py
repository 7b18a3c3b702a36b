"""A plain bench.py run on the GPU: it times the steps asked for, checks and
measures nothing else, and --dump-outputs writes the last timed step's CRCs,
which equal the oracle's for every payload.  Config c2 (65536 x 4 KiB, four
rotated copies: 1 GiB), the smallest device config."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_c2_line_and_dumped_crcs(tmp_path, oracle_mod):
    import torch
    torch.cuda.empty_cache()  # the child allocates its own batch
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "3",
           "--warmup", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    print(json.dumps(res))
    assert res["steps"] == 3 and res["warmup"] == 2 and res["n_gpus"] == 1
    assert res["value"] > 0 and res["unit"] == "GiB/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    # value and ms_per_step describe the same timed steps: 256 MiB per step
    assert abs(res["value"] - 0.25 / (res["ms_per_step"] * 1e-3)) < 0.01 * res["value"]
    assert res["roofline"]["kernel_ms"] > 0 and "cold" in res["roofline"]["cache"]
    # what only --full runs is absent
    assert res["parity"].startswith("unchecked (plain run")
    assert not {"cpu_baseline", "rotation", "c5_strong", "e2e"} & set(res)
    assert os.listdir(tmp_path) == ["crcs.npy"]
    got = np.load(tmp_path / "crcs.npy")
    assert got.dtype == np.float64 and got.shape == (65536,)
    want = oracle_mod.splitmix_batch_fixed("crc32c", 0x4D43310000000002, 4096, 4096, 0, 65536, variant="sse42",
                                           nthreads=16)
    assert np.array_equal(got.astype(np.uint64), want.astype(np.uint64))
