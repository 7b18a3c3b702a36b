"""C ABI of the XDR-mode sender and the size calls (include/mchecksum_gpu.h):
mchecksum_gpu_pack_xdr_messages, _xdr_encoded_sizes, _xdr_decoded_sizes, and
the schema kind MCHECKSUM_XDR_SINT.

No GPU here: the symbols exist and the argument checks come in the header's
order -- MCHECKSUM_GPU_EINVAL (-1) before the method's MCHECKSUM_GPU_EMETHOD
(-3), before the device's MCHECKSUM_GPU_ENODEV (-2)."""
import ctypes

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAMES = ("mchecksum_gpu_pack_xdr_messages", "mchecksum_gpu_xdr_encoded_sizes", "mchecksum_gpu_xdr_decoded_sizes")
SINT = 6
# (schema, nfields) that every XDR entry point refuses, as tests/test_capi_xdr_messages.py lists them,
# and kind 6 with a size no integer has
BAD_SCHEMAS = [[(0, 3)], [(9, 1)], [(5, 2), (0, 4)], [(0, 4)] * 65, [(SINT, 3)]]


def _fields(schema):
    from mercury_amd._lib import XdrField
    return (XdrField * max(1, len(schema)))(*[XdrField(k, z) for k, z in schema])


def _bufs():
    return (ctypes.create_string_buffer(64), (ctypes.c_uint64 * 2)(0, 64), ctypes.create_string_buffer(64),
            (ctypes.c_uint64 * 2)(0, 64))


def _schema_calls(L):
    """Every XDR entry point as call(fields, nfields) with otherwise valid
    arguments, a method it supports and one message."""
    src, soff, buf, off = _bufs()
    out = (ctypes.c_uint64 * 1)()
    keep = (src, soff, buf, off, out)
    m = b"crc32c"
    return keep, {
        "checksum_xdr": lambda f, nf: L.mchecksum_gpu_checksum_xdr(m, f, nf, buf, off, 1, out, None, None),
        "verify": lambda f, nf: L.mchecksum_gpu_verify_xdr_messages(m, f, nf, buf, off, 1, 20, 16, None, None, None),
        "seal": lambda f, nf: L.mchecksum_gpu_seal_xdr_messages(m, f, nf, buf, off, 1, 20, 16, None, None),
        "unpack": lambda f, nf: L.mchecksum_gpu_unpack_xdr_messages(m, f, nf, buf, off, 1, 20, 16, src, soff, None,
                                                                    None, None),
        "pack": lambda f, nf: L.mchecksum_gpu_pack_xdr_messages(m, f, nf, src, soff, buf, off, 1, 20, 16, None, None),
        "encoded_sizes": lambda f, nf: L.mchecksum_gpu_xdr_encoded_sizes(f, nf, src, soff, 1, out, None, None),
        "decoded_sizes": lambda f, nf: L.mchecksum_gpu_xdr_decoded_sizes(f, nf, buf, off, 1, 20, out, None, None,
                                                                         None),
    }


def test_symbols_exist(product_lib):
    from mercury_amd import _lib, gpu
    for n in NAMES:
        assert hasattr(product_lib, n), n
        assert n in _lib.GPU_SYMBOLS
    assert gpu.XDR_SINT == SINT == _lib.XDR_SINT


def test_pack_einval_outranks_the_method(product_lib):
    L = product_lib
    src, soff, buf, off = _bufs()
    f = L.mchecksum_gpu_pack_xdr_messages
    ok = _fields([(0, 4), (2, 0)])
    # a method that would be refused (crc64), one that would pass (crc32c) and an unknown one: EINVAL either way
    for method in (b"crc64", b"crc32c", b"nonesuch"):
        cases = [
            (lambda: f(method, None, 2, src, soff, buf, off, 1, 20, 16, None, None), "NULL"),
            (lambda: f(method, ok, 2, None, soff, buf, off, 1, 20, 16, None, None), "NULL"),
            (lambda: f(method, ok, 2, src, None, buf, off, 1, 20, 16, None, None), "NULL"),
            (lambda: f(method, ok, 2, src, soff, None, off, 1, 20, 16, None, None), "NULL"),
            (lambda: f(method, ok, 2, src, soff, buf, None, 1, 20, 16, None, None), "NULL"),
            (lambda: f(method, ok, 2, src, soff, buf, off, 1, 18, 16, None, None), "hash_offset"),
            (lambda: f(method, ok, 2, src, soff, buf, off, 1, 16, 20, None, None), "hash_offset"),
            (lambda: f(method, ok, 2, src, soff, buf, off, 0, 19, 16, None, None), "hash_offset"),  # also at count == 0
            (lambda: f(method, None, 0, None, None, None, None, 0, 16, 20, None, None), "hash_offset"),
            (lambda: f(method, ok, 2, src, soff, buf, off, (1 << 31) + 1, 20, 16, None, None), "2^31"),
        ]
        cases += [(lambda s=s: f(method, _fields(s), len(s), src, soff, buf, off, 1, 20, 16, None, None), "schema")
                  for s in BAD_SCHEMAS]
        for c, why in cases:
            assert c() == EINVAL, (method, why)
            assert why.encode() in L.mchecksum_gpu_last_error(), (why, L.mchecksum_gpu_last_error())


@pytest.mark.parametrize("name", ["encoded_sizes", "decoded_sizes"])
def test_size_calls_einval_comes_first(product_lib, name):
    L = product_lib
    src, soff, buf, off = _bufs()
    out = (ctypes.c_uint64 * 1)()
    ok = _fields([(0, 4), (2, 0)])
    if name == "encoded_sizes":
        def call(f, nf, b, o, n, sizes):
            return L.mchecksum_gpu_xdr_encoded_sizes(f, nf, b, o, n, sizes, None, None)
    else:
        def call(f, nf, b, o, n, sizes):
            return L.mchecksum_gpu_xdr_decoded_sizes(f, nf, b, o, n, 20, sizes, None, None, None)
    cases = [
        (lambda: call(None, 2, buf, off, 1, out), "NULL"),
        (lambda: call(ok, 2, None, off, 1, out), "NULL"),
        (lambda: call(ok, 2, buf, None, 1, out), "NULL"),
        (lambda: call(ok, 2, buf, off, 1, None), "NULL"),
        (lambda: call(ok, 2, buf, off, (1 << 31) + 1, out), "2^31"),
    ]
    cases += [(lambda s=s: call(_fields(s), len(s), buf, off, 1, out), "schema") for s in BAD_SCHEMAS]
    for c, why in cases:
        assert c() == EINVAL, why
        assert why.encode() in L.mchecksum_gpu_last_error(), (why, L.mchecksum_gpu_last_error())


@pytest.mark.parametrize("size", [1, 2, 4, 8])
def test_sint_passes_every_schema_check(product_lib, size):
    """(6, 1|2|4|8) is a valid field for all XDR entry points, old and new: the
    call gets past MCHECKSUM_GPU_EINVAL and ends at the device check (no GPU
    here) -- or, with a method the call does not take, at the method's."""
    import torch
    L = product_lib
    keep, calls = _schema_calls(L)
    schema = [(0, 4), (SINT, size), (2, 0)]
    for name, call in calls.items():
        rc = call(_fields(schema), len(schema))
        assert rc != EINVAL, (name, L.mchecksum_gpu_last_error())
        if not torch.cuda.is_available():
            assert rc == ENODEV, (name, rc)
    src, soff, buf, off = _bufs()
    f = _fields(schema)
    assert L.mchecksum_gpu_pack_xdr_messages(b"crc64", f, 3, src, soff, buf, off, 1, 20, 16, None, None) == EMETHOD
    assert L.mchecksum_gpu_seal_xdr_messages(b"crc64", f, 3, buf, off, 1, 20, 16, None, None) == EMETHOD
    assert L.mchecksum_gpu_checksum_xdr(b"crc16", f, 3, buf, off, 1, buf, None, None) == EMETHOD
    # (6, 3) and kind 9 stay refused everywhere
    for name, call in calls.items():
        assert call(_fields([(SINT, 3)]), 1) == EINVAL, name
        assert call(_fields([(9, 1)]), 1) == EINVAL, name


@pytest.mark.parametrize("method", [b"crc64", b"crc16", b"crc64-ecma182", b"nonesuch"])
def test_other_methods_are_refused(product_lib, method):
    """The header slot is 32 bits: 64-bit, 16-bit and MSB-first models and
    unknown names give EMETHOD, before the device is looked for."""
    L = product_lib
    src, soff, buf, off = _bufs()
    f = L.mchecksum_gpu_pack_xdr_messages
    assert f(method, _fields([(0, 4), (2, 0)]), 2, src, soff, buf, off, 1, 20, 16, None, None) == EMETHOD
    assert f(method, None, 0, None, None, None, None, 0, 20, 16, None, None) == EMETHOD  # an empty batch too
    assert L.mchecksum_gpu_last_error()


def test_no_device_is_an_error(product_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    L = product_lib
    src, soff, buf, off = _bufs()
    out = (ctypes.c_uint64 * 1)()
    ok = _fields([(0, 4), (2, 0)])
    f = L.mchecksum_gpu_pack_xdr_messages
    assert f(b"crc32c", ok, 2, src, soff, buf, off, 1, 20, 16, None, None) == ENODEV
    assert f(b"crc32c", None, 0, None, None, None, None, 0, 20, 16, None, None) == ENODEV
    assert f(b"crc32", None, 0, None, None, None, None, 0, 4, 0, None, None) == ENODEV
    assert b"device" in L.mchecksum_gpu_last_error()
    assert L.mchecksum_gpu_xdr_encoded_sizes(ok, 2, src, soff, 1, out, None, None) == ENODEV
    assert L.mchecksum_gpu_xdr_encoded_sizes(None, 0, None, None, 0, None, None, None) == ENODEV
    assert L.mchecksum_gpu_xdr_decoded_sizes(ok, 2, buf, off, 1, 20, out, None, None, None) == ENODEV
    assert L.mchecksum_gpu_xdr_decoded_sizes(None, 0, None, None, 0, 20, None, None, None, None) == ENODEV
    assert b"device" in L.mchecksum_gpu_last_error()
