"""The receiver's copying call from C on the MI355X: build/hg_unpack_consumer
(tests/native/hg_unpack_consumer.c, built by `make` with one compiler line)
packs 4096 requests into a device receive buffer, unpacks them with
mchecksum_gpu_unpack_messages on a hipStream_t it created and checks that the
bytes round-trip with every status 0; then it flips one payload bit and checks
that exactly that message reads 1."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "hg_unpack_consumer")


def test_c_receiver_unpacks_and_finds_the_flipped_bit(gpu):
    assert os.access(EXE, os.X_OK), "build/hg_unpack_consumer missing: run make"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout.splitlines()
    assert "as sent: 4096 messages" in r.stdout and "one payload bit flipped: 4096 messages" in r.stdout
    assert r.stdout.count("payloads 0 differ, statuses 0 wrong") == 2
