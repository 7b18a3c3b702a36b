"""bench.py's plain / --full split and --dump-outputs, on the CPU: the c1
config (host streaming API, no GPU) run as a command, and dump_outputs on
arrays of every kind the GPU configs hand it."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_c1_line_times_the_steps_asked_for_and_nothing_else(tmp_path, oracle_mod):
    import struct
    O = oracle_mod
    res = _bench("--config", "c1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "d"))
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["value"] > 0 and res["unit"] == "GiB/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    # value and ms_per_step describe the same 3 timed steps
    assert abs(res["value"] - 1024 * 4100 / (res["ms_per_step"] * 1e-3) / 2**30) < 0.01 * res["value"]
    assert "cpu_baseline" not in res and res["parity"].startswith("unchecked (plain run")
    # the dumped outputs are exact float64 and equal the oracle's
    host = O.splitmix_bytes(1024 * 4096, 0x4D43310000000001)
    want = [O.crc("crc32c", struct.pack("<I", 4096) + host[i * 4096:(i + 1) * 4096].tobytes()) for i in range(1024)]
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in sorted(os.listdir(tmp_path / "d"))}
    assert sorted(got) == ["first_crc_hi", "first_crc_lo", "xor_of_crcs_hi", "xor_of_crcs_lo"]
    assert all(a.dtype == np.float64 and a.shape == (1,) for a in got.values())
    assert got["first_crc_hi"][0] == 0 and got["first_crc_lo"][0] == want[0]
    assert got["xor_of_crcs_lo"][0] == np.bitwise_xor.reduce(np.array(want, dtype=np.uint64))


def test_full_c1_line_carries_the_baseline_and_the_oracle_verdict():
    res = _bench("--config", "c1", "--steps", "3", "--warmup", "1", "--full")
    assert res["steps"] == 3
    assert res["parity"].startswith("bit-exact (all 1024 payloads"), res["parity"]
    cb = res["cpu_baseline"]
    assert cb["value"] > 0 and cb["kind"] == "port" and cb["cores"] == 1


def test_zero_steps_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1", "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_is_exact_for_every_output_type(tmp_path):
    import bench
    crc32 = np.array([-1, 0, 0x7FFFFFFF, -0x80000000], dtype=np.int32)  # CRC-32s sit in signed words
    crc64 = np.array([-1, 1 << 62, 0x0123456789ABCDEF], dtype=np.int64)
    status = np.array([0, 1, 255], dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), {"crcs": crc32, "wide": crc64, "status": status})
    load = lambda n: np.load(tmp_path / (n + ".npy"))  # noqa: E731
    assert sorted(os.listdir(tmp_path)) == ["crcs.npy", "status.npy", "wide_hi.npy", "wide_lo.npy"]
    assert load("crcs").dtype == np.float64
    assert np.array_equal(load("crcs").astype(np.uint32), crc32.view(np.uint32))
    assert np.array_equal(load("status"), [0, 1, 255])
    back = (load("wide_hi").astype(np.uint64) << np.uint64(32)) | load("wide_lo").astype(np.uint64)
    assert np.array_equal(back, crc64.view(np.uint64))


def test_dump_outputs_cuts_a_large_output_to_the_same_sample_every_time(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 1000)
    a = np.arange(5000, dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "a"), {"crcs": a, "more": a[::-1].copy()})
    bench.dump_outputs(str(tmp_path / "b"), {"crcs": a, "more": a[::-1].copy()})
    s = np.load(tmp_path / "a" / "crcs.npy")
    assert s.size == 468 and np.all(np.diff(s) > 0)  # 2 files share the limit; positions in order
    assert np.array_equal(np.load(tmp_path / "a" / "more.npy"), 4999 - s)  # the same positions in every array
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 8 * 1000  # the limit holds for the files as written, headers included
    for f in ("crcs.npy", "more.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
