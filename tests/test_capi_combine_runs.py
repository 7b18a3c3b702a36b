"""C ABI of mchecksum_gpu_combine_runs (include/mchecksum_gpu.h): exported and
bound, its argument checks in combine's order (NULL pointers and the caps,
then the device, then the method), and the wrapper's refusal of host tensors.
CPU only: nothing here launches a kernel."""
import ctypes
import subprocess

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAME = "mchecksum_gpu_combine_runs"


def _bufs():
    return dict(crc=(ctypes.c_uint64 * 8)(), lens=(ctypes.c_uint64 * 8)(), nchunks=8,
                first=(ctypes.c_uint64 * 4)(0, 3, 3, 8), nruns=3, out=(ctypes.c_uint64 * 3)())


def _call(L, method=b"crc32c", crc=None, lens=None, nchunks=0, first=None, nruns=0, out=None, out_len=None):
    return L.mchecksum_gpu_combine_runs(method, crc, lens, nchunks, first, nruns, out, out_len, None)


def test_symbol_is_exported_and_bound(product_lib):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NAME in exported and NAME in _lib.GPU_SYMBOLS
    assert len(getattr(product_lib, NAME).argtypes) == 9


def test_argument_checks_come_before_the_device_and_the_method(product_lib):
    L = product_lib
    ok = _bufs()
    cases = [(dict(ok, **{k: None}), b"NULL") for k in ("crc", "lens", "first", "out")]  # each required pointer in turn
    cases += [(dict(nchunks=8), b"NULL")]  # chunks need their tables even when there are no runs
    cases += [(dict(ok, nruns=(1 << 31) + 1), b"2^31"), (dict(ok, nchunks=(1 << 31) + 1), b"2^31")]
    for kw, why in cases:
        for method in (b"crc32c", b"crc64-ecma182", b"crc16", b"no-such-crc"):
            assert _call(L, method, **kw) == EINVAL, (kw, why)
            assert why in (L.mchecksum_gpu_last_error() or b""), why
    # no runs: no launch (so host buffers are safe here even with a device), but the checks come first
    assert _call(L, **dict(ok, nruns=0, first=None, out=None)) in (0, ENODEV)
    assert _call(L, **dict(ok, nruns=0, nchunks=1 << 31)) in (0, ENODEV)  # exactly 2^31 is within the cap
    assert _call(L) in (0, ENODEV)  # no runs, no chunks, no buffers
    for method in (b"crc16", b"no-such-crc"):
        assert _call(L, method) in (EMETHOD, ENODEV)


def test_wrapper_refuses_host_tensors():
    """The wrapper's tensor checks come before any library call: tables that
    are not on a device are an error, not a fallback."""
    import torch

    from mercury_amd import gpu as G
    crc = torch.zeros(8, dtype=torch.int32)
    lens = torch.ones(8, dtype=torch.int64)
    first = torch.tensor([0, 3, 3, 8], dtype=torch.int64)
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", crc, lens, first, run_first_host=[0, 3, 3, 8])
