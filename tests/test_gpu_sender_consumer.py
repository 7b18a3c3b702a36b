"""The sender side of the batch ABI from C on the MI355X: build/hg_seal_consumer
(tests/native/hg_seal_consumer.c, built by `make` with one compiler line) packs
4096 requests from a device argument buffer with mchecksum_gpu_pack_messages
on a hipStream_t it created, seals their core headers, runs the receiver's two
verify calls, and compares every payload hash with hg_proc's streaming
sequence (an mchecksum_update per field, src/mercury_proc.h:124-181), every
core-header hash with the per-field CRC16 and every payload with its source."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "hg_seal_consumer")


def test_c_sender_packs_and_seals_like_mercury(gpu):
    assert os.access(EXE, os.X_OK), "build/hg_seal_consumer missing: run make"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
    assert "payload hashes 0 differ, core-header hashes 0 differ, payloads 0 differ" in r.stdout
    assert "statuses flagged 0; receiver flagged 0 / 0" in r.stdout
