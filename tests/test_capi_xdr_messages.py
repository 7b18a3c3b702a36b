"""C ABI of the XDR-mode message calls (include/mchecksum_gpu.h):
mchecksum_gpu_verify_xdr_messages, _seal_xdr_messages, _unpack_xdr_messages.

No GPU here: the symbols exist and the argument checks come in the header's
order -- MCHECKSUM_GPU_EINVAL (-1) before the method's MCHECKSUM_GPU_EMETHOD
(-3), before the device's MCHECKSUM_GPU_ENODEV (-2)."""
import ctypes

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAMES = ("mchecksum_gpu_verify_xdr_messages", "mchecksum_gpu_seal_xdr_messages", "mchecksum_gpu_unpack_xdr_messages")


def _calls(L, buf, offs):
    """name -> call(method, fields, nfields, buf, offs, count, pay, hash) with
    valid values for the arguments each call has beside those."""
    return {
        "verify": lambda m, f, nf, b, o, n, p, h: L.mchecksum_gpu_verify_xdr_messages(m, f, nf, b, o, n, p, h, None,
                                                                                      None, None),
        "seal": lambda m, f, nf, b, o, n, p, h: L.mchecksum_gpu_seal_xdr_messages(m, f, nf, b, o, n, p, h, None, None),
        "unpack": lambda m, f, nf, b, o, n, p, h: L.mchecksum_gpu_unpack_xdr_messages(m, f, nf, b, o, n, p, h, buf, offs,
                                                                                      None, None, None),
    }


def _fields(schema):
    from mercury_amd._lib import XdrField
    return (XdrField * max(1, len(schema)))(*[XdrField(k, z) for k, z in schema])


def test_symbols_exist(product_lib):
    from mercury_amd import _lib
    for n in NAMES:
        assert hasattr(product_lib, n), n
        assert n in _lib.GPU_SYMBOLS


@pytest.mark.parametrize("name", ["verify", "seal", "unpack"])
def test_einval_outranks_the_method(product_lib, name):
    L = product_lib
    buf = ctypes.create_string_buffer(64)
    offs = (ctypes.c_uint64 * 2)(0, 64)
    call = _calls(L, buf, offs)[name]
    ok = _fields([(0, 4), (2, 0)])
    # a method that would be refused (crc64) and one that would pass (crc32c): EINVAL either way
    for method in (b"crc64", b"crc32c", b"nonesuch"):
        cases = [
            (lambda: call(method, ok, 2, None, offs, 1, 20, 16), "NULL"),
            (lambda: call(method, ok, 2, buf, None, 1, 20, 16), "NULL"),
            (lambda: call(method, None, 2, buf, offs, 1, 20, 16), "NULL"),
            (lambda: call(method, ok, 2, buf, offs, 1, 18, 16), "hash_offset"),
            (lambda: call(method, ok, 2, buf, offs, 1, 16, 20), "hash_offset"),
            (lambda: call(method, ok, 2, buf, offs, 0, 19, 16), "hash_offset"),  # also at count == 0
            (lambda: call(method, _fields([(0, 3)]), 1, buf, offs, 1, 20, 16), "schema"),
            (lambda: call(method, _fields([(9, 1)]), 1, buf, offs, 1, 20, 16), "schema"),
            (lambda: call(method, _fields([(5, 2), (0, 4)]), 2, buf, offs, 1, 20, 16), "schema"),
            (lambda: call(method, _fields([(0, 4)] * 65), 65, buf, offs, 1, 20, 16), "schema"),
            (lambda: call(method, ok, 2, buf, offs, (1 << 31) + 1, 20, 16), "2^31"),
        ]
        for c, why in cases:
            assert c() == EINVAL, (method, why)
            assert why.encode() in L.mchecksum_gpu_last_error(), (why, L.mchecksum_gpu_last_error())
    if name == "unpack":
        f = L.mchecksum_gpu_unpack_xdr_messages
        assert f(b"crc64", ok, 2, buf, offs, 1, 20, 16, None, offs, None, None, None) == EINVAL
        assert f(b"crc64", ok, 2, buf, offs, 1, 20, 16, buf, None, None, None, None) == EINVAL


@pytest.mark.parametrize("name", ["verify", "seal", "unpack"])
@pytest.mark.parametrize("method", [b"crc64", b"crc16", b"crc64-ecma182", b"nonesuch"])
def test_other_methods_are_refused(product_lib, name, method):
    """The header slot is 32 bits: 64-bit, 16-bit and MSB-first models and
    unknown names give EMETHOD, before the device is looked for."""
    L = product_lib
    buf = ctypes.create_string_buffer(64)
    offs = (ctypes.c_uint64 * 2)(0, 64)
    call = _calls(L, buf, offs)[name]
    assert call(method, _fields([(0, 4), (2, 0)]), 2, buf, offs, 1, 20, 16) == EMETHOD
    assert call(method, None, 0, None, None, 0, 20, 16) == EMETHOD  # an empty batch passes the same checks
    assert L.mchecksum_gpu_last_error()


@pytest.mark.parametrize("name", ["verify", "seal", "unpack"])
def test_no_device_is_an_error(product_lib, name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    L = product_lib
    buf = ctypes.create_string_buffer(64)
    offs = (ctypes.c_uint64 * 2)(0, 64)
    call = _calls(L, buf, offs)[name]
    assert call(b"crc32c", _fields([(0, 4), (2, 0)]), 2, buf, offs, 1, 20, 16) == ENODEV
    assert call(b"crc32c", None, 0, None, None, 0, 20, 16) == ENODEV
    assert call(b"crc32", None, 0, None, None, 0, 4, 0) == ENODEV
    assert b"device" in L.mchecksum_gpu_last_error()
