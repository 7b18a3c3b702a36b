"""C ABI of the detached calls with both sides by address list
(include/mchecksum_gpu.h): mchecksum_gpu_verify_detached_message_list,
_seal_detached_message_list, _state_verify_message_list and
_state_seal_message_list -- exported, bound, and their checks in the table
calls' order: arguments (EINVAL; every array is a required pointer with
count > 0), then the method (EMETHOD, ahead of the device, so a wrong method
reads the same with and without a GPU), then the device (ENODEV).  count == 0
needs no buffers but passes those checks first.  CPU only: nothing here
launches a kernel."""
import ctypes
import subprocess

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAMES = ("mchecksum_gpu_verify_detached_message_list", "mchecksum_gpu_seal_detached_message_list",
         "mchecksum_gpu_state_verify_message_list", "mchecksum_gpu_state_seal_message_list")
BAD_METHODS = (b"crc64", b"crc16", b"no-such-crc", b"")
BIG = (1 << 31) + 1
MSG_POINTERS = ("maddr", "mlen")
PAYLOAD_POINTERS = ("paddr", "plen")


class _Bufs:
    def __init__(self):
        self.msg = ctypes.create_string_buffer(64)
        self.pay = ctypes.create_string_buffer(256)
        self.maddr = (ctypes.c_uint64 * 1)(ctypes.addressof(self.msg))
        self.mlen = (ctypes.c_uint64 * 1)(52)
        self.paddr = (ctypes.c_uint64 * 1)(ctypes.addressof(self.pay))
        self.plen = (ctypes.c_uint64 * 1)(200)
        self.state = (ctypes.c_uint32 * 1)(0)


def _calls(L, b, method=b"crc32c", count=1, maddr=True, mlen=True, paddr=True, plen=True, state=True, hash_=16):
    """The four calls as thunks, with any required pointer NULLed."""
    ma, ml = (b.maddr if maddr else None), (b.mlen if mlen else None)
    pa, pl = (b.paddr if paddr else None), (b.plen if plen else None)
    st = b.state if state else None
    return {
        "verify": lambda: L.mchecksum_gpu_verify_detached_message_list(method, ma, ml, hash_, pa, pl, count, None, None, None),
        "seal": lambda: L.mchecksum_gpu_seal_detached_message_list(method, ma, ml, hash_, pa, pl, count, None, None),
        "state_verify": lambda: L.mchecksum_gpu_state_verify_message_list(method, st, count, ma, ml, hash_, None, None, None),
        "state_seal": lambda: L.mchecksum_gpu_state_seal_message_list(method, st, count, ma, ml, hash_, None, None),
    }


_NONE = dict(maddr=False, mlen=False, paddr=False, plen=False, state=False)


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def test_detached_list_symbols_are_exported_and_bound(product_lib):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in exported and n in _lib.GPU_SYMBOLS
        assert getattr(product_lib, n).argtypes, n
    # the table calls' argument lists, with (addr, len) where they have (buf, offsets)
    for n in NAMES:
        table = n.replace("_message_list", "_messages")
        assert len(getattr(product_lib, n).argtypes) == len(getattr(product_lib, table).argtypes), n


def test_python_wrappers_exist():
    from mercury_amd import gpu
    for n in ("verify_detached_message_list", "seal_detached_message_list", "state_verify_message_list",
              "state_seal_message_list", "rpc_message_list"):
        assert callable(getattr(gpu, n)), n


@pytest.mark.parametrize("null", MSG_POINTERS)
def test_null_message_pointer(product_lib, null):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, **{null: False}).items():
        assert call() == EINVAL, (name, null)
        assert b"NULL" in _err(L), (name, _err(L))


@pytest.mark.parametrize("null", PAYLOAD_POINTERS)
def test_null_payload_pointer(product_lib, null):
    L, b = product_lib, _Bufs()
    calls = _calls(L, b, **{null: False})
    for name in ("verify", "seal"):
        assert calls[name]() == EINVAL, (name, null)
        assert b"NULL" in _err(L), (name, _err(L))


def test_null_state_pointer(product_lib):
    L, b = product_lib, _Bufs()
    calls = _calls(L, b, state=False)
    for name in ("state_verify", "state_seal"):
        assert calls[name]() == EINVAL, name
        assert b"NULL" in _err(L), (name, _err(L))


def test_count_cap(product_lib):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, count=BIG).items():
        assert call() == EINVAL, name
        assert b"2^31" in _err(L), (name, _err(L))


@pytest.mark.parametrize("hash_", [(1 << 30) + 1, 1 << 35])
def test_hash_offset_cap(product_lib, hash_):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, hash_=hash_).items():
        assert call() == EINVAL, (name, hash_)
        assert b"hash_offset" in _err(L), (name, _err(L))
    for name, call in _calls(L, b, hash_=hash_, count=0, **_NONE).items():
        assert call() == EINVAL, (name, hash_)


@pytest.mark.parametrize("method", BAD_METHODS)
def test_einval_outranks_the_method(product_lib, method):
    L, b = product_lib, _Bufs()
    for bad in (dict(count=BIG), dict(maddr=False), dict(mlen=False), dict(hash_=(1 << 30) + 1)):
        for name, call in _calls(L, b, method=method, **bad).items():
            assert call() == EINVAL, (name, bad)
    for bad in (dict(paddr=False), dict(plen=False)):
        calls = _calls(L, b, method=method, **bad)
        assert calls["verify"]() == EINVAL and calls["seal"]() == EINVAL, bad


@pytest.mark.parametrize("method", BAD_METHODS)
def test_method_checks(product_lib, method):
    """Refused ahead of the device, on an empty batch too: the same code with
    and without a GPU."""
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, method=method).items():
        assert call() == EMETHOD, (name, method)
        assert _err(L), name
    for name, call in _calls(L, b, method=method, count=0, **_NONE).items():
        assert call() == EMETHOD, (name, method)


def test_without_a_device_the_calls_refuse(product_lib):
    """ENODEV on a box without a GPU, after the argument and method checks, on
    an empty batch too; with one, well-formed calls on host memory are not made
    here (tests/test_gpu_detached_list.py runs them on device memory)."""
    import torch
    L, b = product_lib, _Bufs()
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    for method in (b"crc32c", b"crc32"):
        for hash_ in (0, 16, 13, 1 << 30):
            for name, call in _calls(L, b, method=method, hash_=hash_).items():
                assert call() == ENODEV, (name, method)
                assert b"no HIP device" in _err(L)
    for name, call in _calls(L, b, count=0, **_NONE).items():
        assert call() == ENODEV, name


def test_empty_batch_needs_no_buffers(product_lib):
    """count == 0 with NULL arrays passes the argument checks: 0 with a
    device, ENODEV without one -- never EINVAL."""
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, count=0, **_NONE).items():
        assert call() in (0, ENODEV), name
