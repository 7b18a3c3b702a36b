"""C ABI of the overflow-RPC entry points (include/mchecksum_gpu.h):
mchecksum_gpu_verify_detached_messages, mchecksum_gpu_seal_detached_messages,
mchecksum_gpu_state_verify_messages and mchecksum_gpu_state_seal_messages --
exported, and their checks in the documented order: arguments (EINVAL), then
the method (EMETHOD, ahead of the device, so a wrong method reads the same with
and without a GPU), then the device (ENODEV).  CPU only: nothing here launches
a kernel."""
import ctypes
import subprocess

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAMES = ("mchecksum_gpu_verify_detached_messages", "mchecksum_gpu_seal_detached_messages",
         "mchecksum_gpu_state_verify_messages", "mchecksum_gpu_state_seal_messages")
BAD_METHODS = (b"crc64", b"crc16", b"crc64-ecma182", b"no-such-crc")
BIG = (1 << 31) + 1


class _Bufs:
    def __init__(self):
        self.msgs = ctypes.create_string_buffer(256)
        self.pay = ctypes.create_string_buffer(256)
        self.state = (ctypes.c_uint32 * 4)()
        self.mo = (ctypes.c_uint64 * 2)(0, 52)
        self.po = (ctypes.c_uint64 * 2)(0, 64)


def _calls(L, b, method=b"crc32c", count=1, msgs=True, mo=True, pay=True, po=True, state=True):
    """The four calls as thunks, with any required pointer NULLed."""
    m, o = (b.msgs if msgs else None), (b.mo if mo else None)
    p, q = (b.pay if pay else None), (b.po if po else None)
    s = b.state if state else None
    return {
        "verify_detached": lambda: L.mchecksum_gpu_verify_detached_messages(method, m, o, 16, p, q, count, None, None, None),
        "seal_detached": lambda: L.mchecksum_gpu_seal_detached_messages(method, m, o, 16, p, q, count, None, None),
        "state_verify": lambda: L.mchecksum_gpu_state_verify_messages(method, s, count, m, o, 16, None, None, None),
        "state_seal": lambda: L.mchecksum_gpu_state_seal_messages(method, s, count, m, o, 16, None, None),
    }


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def test_detached_symbols_are_exported_and_bound(product_lib):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in exported and n in _lib.GPU_SYMBOLS
        assert getattr(product_lib, n).argtypes, n


@pytest.mark.parametrize("null", ["msgs", "mo", "pay", "po", "state"])
def test_null_required_pointer(product_lib, null):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, **{null: False}).items():
        uses = {"verify_detached": ("msgs", "mo", "pay", "po"), "seal_detached": ("msgs", "mo", "pay", "po"),
                "state_verify": ("msgs", "mo", "state"), "state_seal": ("msgs", "mo", "state")}[name]
        if null not in uses:
            continue
        assert call() == EINVAL, (name, null)
        assert b"NULL" in _err(L), (name, _err(L))


def test_count_cap_and_hash_offset_cap(product_lib):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, count=BIG).items():
        assert call() == EINVAL, name
        assert b"2^31" in _err(L), (name, _err(L))
    big = (1 << 30) + 1
    assert L.mchecksum_gpu_verify_detached_messages(b"crc32c", b.msgs, b.mo, big, b.pay, b.po, 1, None, None, None) == EINVAL
    assert L.mchecksum_gpu_seal_detached_messages(b"crc32c", b.msgs, b.mo, big, b.pay, b.po, 1, None, None) == EINVAL
    assert L.mchecksum_gpu_state_verify_messages(b"crc32c", b.state, 1, b.msgs, b.mo, big, None, None, None) == EINVAL
    assert L.mchecksum_gpu_state_seal_messages(b"crc32c", b.state, 1, b.msgs, b.mo, big, None, None) == EINVAL
    assert b"hash_offset" in _err(L)


@pytest.mark.parametrize("method", BAD_METHODS)
def test_einval_outranks_the_method(product_lib, method):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, method=method, count=BIG).items():
        assert call() == EINVAL, name
    for name, call in _calls(L, b, method=method, mo=False).items():
        assert call() == EINVAL, name


@pytest.mark.parametrize("method", BAD_METHODS)
def test_method_checks(product_lib, method):
    """Every method but a 32-bit model is refused, on an empty batch too, and
    ahead of the device: the same code with and without a GPU."""
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, method=method).items():
        assert call() == EMETHOD, (name, method)
        assert _err(L), name
    for name, call in _calls(L, b, method=method, count=0, msgs=False, mo=False, pay=False, po=False, state=False).items():
        assert call() == EMETHOD, (name, method)


def test_without_a_device_the_calls_refuse(product_lib):
    """ENODEV on a box without a GPU, after the argument and method checks, on
    an empty batch too; with one, well-formed calls on host memory are not made
    here (tests/test_gpu_detached.py runs them)."""
    import torch
    L, b = product_lib, _Bufs()
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    for method in (b"crc32c", b"crc32"):
        for name, call in _calls(L, b, method=method).items():
            assert call() == ENODEV, (name, method)
            assert b"no HIP device" in _err(L)
    for name, call in _calls(L, b, count=0, msgs=False, mo=False, pay=False, po=False, state=False).items():
        assert call() == ENODEV, name


def test_empty_batch_needs_no_buffers(product_lib):
    """count == 0 with NULL buffers passes the argument checks: 0 with a
    device, ENODEV without one -- never EINVAL."""
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, count=0, msgs=False, mo=False, pay=False, po=False, state=False).items():
        assert call() in (0, ENODEV), name
