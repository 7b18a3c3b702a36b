"""C ABI of the RPC message calls by address list (include/mchecksum_gpu.h):
mchecksum_gpu_verify_rpc_message_list, _seal_, _unpack_ and
_pack_rpc_message_list -- exported, bound, and their checks in the table
calls' order: arguments (EINVAL; dev_msg_addr and dev_msg_len are required
pointers with count > 0), then the two methods (EMETHOD, ahead of the device,
so a wrong method reads the same with and without a GPU), then the device
(ENODEV).  count == 0 needs no buffers but passes those checks first.  CPU
only: nothing here launches a kernel."""
import ctypes
import subprocess

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
REQUEST, RESPONSE = 0, 1
NAMES = ("mchecksum_gpu_verify_rpc_message_list", "mchecksum_gpu_seal_rpc_message_list",
         "mchecksum_gpu_unpack_rpc_message_list", "mchecksum_gpu_pack_rpc_message_list")
BAD_METHODS = ((b"crc32c", b"crc32c"), (b"crc16", b"crc64"), (b"crc16", b"crc16"), (b"no-such-crc", b"crc32c"),
               (b"crc16", b"no-such-crc"), (b"crc64", b"crc32c"))
BIG = (1 << 31) + 1
LIST_POINTERS = ("addr", "lens")
COPY_POINTERS = ("other", "oo")


class _Bufs:
    def __init__(self):
        self.buf = ctypes.create_string_buffer(256)
        self.addr = (ctypes.c_uint64 * 1)(ctypes.addressof(self.buf))
        self.lens = (ctypes.c_uint64 * 1)(84)
        self.other = ctypes.create_string_buffer(256)    # the destination of an unpack, the source of a pack
        self.oo = (ctypes.c_uint64 * 2)(0, 64)


def _calls(L, b, hm=b"crc16", pm=b"crc32c", kind=REQUEST, count=1, addr=True, lens=True, other=True, oo=True, pay=20,
           hash_=16):
    """The four calls as thunks, with any required pointer NULLed."""
    a, n = (b.addr if addr else None), (b.lens if lens else None)
    x, xo = (b.other if other else None), (b.oo if oo else None)
    return {
        "verify": lambda: L.mchecksum_gpu_verify_rpc_message_list(hm, pm, kind, a, n, count, pay, hash_, None, None, None),
        "seal": lambda: L.mchecksum_gpu_seal_rpc_message_list(hm, pm, kind, a, n, count, pay, hash_, None, None),
        "unpack": lambda: L.mchecksum_gpu_unpack_rpc_message_list(hm, pm, kind, a, n, count, pay, hash_, x, xo, None,
                                                                  None, None),
        "pack": lambda: L.mchecksum_gpu_pack_rpc_message_list(hm, pm, kind, x, xo, a, n, count, pay, hash_, None, None),
    }


_NONE = dict(addr=False, lens=False, other=False, oo=False)


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def test_rpc_list_symbols_are_exported_and_bound(product_lib):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in exported and n in _lib.GPU_SYMBOLS
        assert getattr(product_lib, n).argtypes, n
    # the table calls' argument lists, with (addr, len) where they have (buf, offsets)
    assert len(product_lib.mchecksum_gpu_verify_rpc_message_list.argtypes) == 11
    assert len(product_lib.mchecksum_gpu_seal_rpc_message_list.argtypes) == 10
    assert len(product_lib.mchecksum_gpu_unpack_rpc_message_list.argtypes) == 13
    assert len(product_lib.mchecksum_gpu_pack_rpc_message_list.argtypes) == 12


def test_python_wrappers_exist():
    from mercury_amd import gpu
    for n in ("verify_rpc_message_list", "seal_rpc_message_list", "unpack_rpc_message_list", "pack_rpc_message_list",
              "rpc_message_list"):
        assert callable(getattr(gpu, n)), n


@pytest.mark.parametrize("null", LIST_POINTERS)
def test_null_list_pointer(product_lib, null):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, **{null: False}).items():
        assert call() == EINVAL, (name, null)
        assert b"NULL" in _err(L), (name, _err(L))


@pytest.mark.parametrize("null", COPY_POINTERS)
def test_null_other_side_pointer(product_lib, null):
    L, b = product_lib, _Bufs()
    calls = _calls(L, b, **{null: False})
    for name in ("unpack", "pack"):
        assert calls[name]() == EINVAL, (name, null)
        assert b"NULL" in _err(L), (name, _err(L))


@pytest.mark.parametrize("kind", [-1, 2, 7])
def test_unknown_kind(product_lib, kind):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, kind=kind).items():
        assert call() == EINVAL, (name, kind)
        assert b"kind" in _err(L), (name, _err(L))
    for name, call in _calls(L, b, kind=kind, count=0, **_NONE).items():
        assert call() == EINVAL, (name, kind)


def test_count_cap(product_lib):
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, count=BIG).items():
        assert call() == EINVAL, name
        assert b"2^31" in _err(L), (name, _err(L))


@pytest.mark.parametrize("pay,hash_", [
    (20, 15),                     # hash_offset < 16: inside the core header
    (20, 0),
    (20, 17),                     # hash_offset + 4 > payload_offset
    (19, 16),
    (16, 16),
    ((1 << 30) + 5, (1 << 30) + 1),   # hash_offset > 2^30
    (1 << 40, 1 << 35),
])
def test_offset_rules(product_lib, pay, hash_):
    L, b = product_lib, _Bufs()
    for kind in (REQUEST, RESPONSE):
        for name, call in _calls(L, b, kind=kind, pay=pay, hash_=hash_).items():
            assert call() == EINVAL, (name, pay, hash_)
            assert b"hash_offset" in _err(L), (name, _err(L))
        for name, call in _calls(L, b, kind=kind, pay=pay, hash_=hash_, count=0, **_NONE).items():
            assert call() == EINVAL, (name, pay, hash_)


@pytest.mark.parametrize("hm,pm", BAD_METHODS)
def test_einval_outranks_the_methods(product_lib, hm, pm):
    L, b = product_lib, _Bufs()
    for bad in (dict(count=BIG), dict(addr=False), dict(lens=False), dict(kind=2), dict(hash_=15), dict(pay=19)):
        for name, call in _calls(L, b, hm=hm, pm=pm, **bad).items():
            assert call() == EINVAL, (name, bad)


@pytest.mark.parametrize("hm,pm", BAD_METHODS)
def test_method_checks(product_lib, hm, pm):
    """Refused ahead of the device, on an empty batch too: the same code with
    and without a GPU."""
    L, b = product_lib, _Bufs()
    for kind in (REQUEST, RESPONSE):
        for name, call in _calls(L, b, hm=hm, pm=pm, kind=kind).items():
            assert call() == EMETHOD, (name, hm, pm)
            assert _err(L), name
        for name, call in _calls(L, b, hm=hm, pm=pm, kind=kind, count=0, **_NONE).items():
            assert call() == EMETHOD, (name, hm, pm)


def test_without_a_device_the_calls_refuse(product_lib):
    """ENODEV on a box without a GPU, after the argument and method checks, on
    an empty batch too; with one, well-formed calls on host memory are not made
    here (tests/test_gpu_rpc_list.py runs them on device memory)."""
    import torch
    L, b = product_lib, _Bufs()
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    for hm, pm in ((b"crc16", b"crc32c"), (b"crc16-kermit", b"crc32"), (b"crc16-ibm-3740", b"crc32c")):
        for kind in (REQUEST, RESPONSE):
            for name, call in _calls(L, b, hm=hm, pm=pm, kind=kind, pay=24, hash_=20).items():
                assert call() == ENODEV, (name, hm, pm)
                assert b"no HIP device" in _err(L)
    for name, call in _calls(L, b, count=0, **_NONE).items():
        assert call() == ENODEV, name


def test_empty_batch_needs_no_buffers(product_lib):
    """count == 0 with NULL buffers passes the argument checks: 0 with a
    device, ENODEV without one -- never EINVAL."""
    L, b = product_lib, _Bufs()
    for name, call in _calls(L, b, count=0, **_NONE).items():
        assert call() in (0, ENODEV), name
