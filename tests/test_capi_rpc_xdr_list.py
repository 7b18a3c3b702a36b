"""The argument checks of the RPC message calls of an XDR build by address list
(include/mchecksum_gpu.h: mchecksum_gpu_verify_rpc_xdr_message_list, _seal_,
_unpack_, _pack_) through ctypes: the four symbols, and the table calls' order
of checks -- EINVAL first (a NULL dev_msg_addr or dev_msg_len with count > 0
and the other NULL pointers, kind, the offsets rules, a bad schema, count >
2^31), then both methods' EMETHOD ahead of the device, then ENODEV.  No compute
on a GPU here: with a device the last step answers 0 for an empty batch,
without one -2."""
import ctypes

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
XDR_INT, XDR_OPAQUE_LEN, XDR_SKIP_IF_ZERO = 0, 2, 5
NAMES = ("verify", "seal", "unpack", "pack")
SCHEMA = [(XDR_INT, 8), (XDR_SKIP_IF_ZERO, 1), (XDR_OPAQUE_LEN, 0)]


@pytest.fixture(scope="module")
def calls(product_lib):
    """name -> f(header_method, payload_method, kind, fields, nfields, addr, len, count, payload_offset, hash_offset,
    other, other_offsets): the four calls behind one argument list, every other output NULL."""
    from mercury_amd._lib import XdrField
    L = product_lib

    def fields_of(schema):
        return (XdrField * max(1, len(schema)))(*[XdrField(k, z) for k, z in schema])

    def verify(hm, pm, kind, f, nf, addr, lens, count, pay, hash_, other, other_off):
        return L.mchecksum_gpu_verify_rpc_xdr_message_list(hm, pm, kind, f, nf, addr, lens, count, pay, hash_, None, None, None)

    def seal(hm, pm, kind, f, nf, addr, lens, count, pay, hash_, other, other_off):
        return L.mchecksum_gpu_seal_rpc_xdr_message_list(hm, pm, kind, f, nf, addr, lens, count, pay, hash_, None, None)

    def unpack(hm, pm, kind, f, nf, addr, lens, count, pay, hash_, other, other_off):
        return L.mchecksum_gpu_unpack_rpc_xdr_message_list(hm, pm, kind, f, nf, addr, lens, count, pay, hash_, other,
                                                           other_off, None, None, None)

    def pack(hm, pm, kind, f, nf, addr, lens, count, pay, hash_, other, other_off):
        return L.mchecksum_gpu_pack_rpc_xdr_message_list(hm, pm, kind, f, nf, other, other_off, addr, lens, count, pay, hash_,
                                                         None, None)

    return {"verify": verify, "seal": seal, "unpack": unpack, "pack": pack}, fields_of, L


def test_symbols_are_exported(product_lib):
    for name in NAMES:
        fn = getattr(product_lib, f"mchecksum_gpu_{name}_rpc_xdr_message_list")
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == list(getattr(product_lib, f"mchecksum_gpu_{name}_rpc_xdr_messages").argtypes)


def _good(fields_of):
    buf = ctypes.create_string_buffer(256)
    other = ctypes.create_string_buffer(256)
    addr = (ctypes.c_uint64 * 1)(ctypes.addressof(buf))
    lens = (ctypes.c_uint64 * 1)(64)
    other_off = (ctypes.c_uint64 * 2)(0, 16)
    return dict(hm=b"crc16", pm=b"crc32c", kind=0, f=fields_of(SCHEMA), nf=len(SCHEMA), addr=addr, lens=lens, count=1,
                pay=20, hash_=16, other=other, other_off=other_off, keep=buf)


def _call(fn, a):
    return fn(a["hm"], a["pm"], a["kind"], a["f"], a["nf"], a["addr"], a["lens"], a["count"], a["pay"], a["hash_"],
              a["other"], a["other_off"])


@pytest.mark.parametrize("name", NAMES)
def test_einval_comes_first(calls, name):
    """Each EINVAL case alone -- with methods that would be EMETHOD, so the order shows on any machine."""
    fns, fields_of, L = calls
    from mercury_amd._lib import XdrField
    cases = [
        (dict(addr=None), "NULL"),
        (dict(lens=None), "NULL"),
        (dict(f=None), "NULL"),
        (dict(kind=2), "kind"),
        (dict(kind=-1), "kind"),
        (dict(hash_=15, pay=20), "hash_offset"),           # inside the core header
        (dict(hash_=17, pay=20), "hash_offset"),           # hash_offset + 4 > payload_offset
        (dict(hash_=(1 << 30) + 1, pay=(1 << 30) + 8), "hash_offset"),
        (dict(count=(1 << 31) + 1), "2^31"),
        (dict(f=fields_of([(XDR_INT, 3)]), nf=1), "schema"),
        (dict(f=fields_of([(XDR_SKIP_IF_ZERO, 1)]), nf=1), "schema"),  # skips past the schema's end
        (dict(f=fields_of([(9, 4)]), nf=1), "schema"),
        (dict(f=(XdrField * 65)(), nf=65), "schema"),
    ]
    if name in ("unpack", "pack"):
        cases += [(dict(other=None), "NULL"), (dict(other_off=None), "NULL")]
    for change, why in cases:
        for bad_methods in (dict(), dict(hm=b"crc32c"), dict(pm=b"crc64"), dict(hm=b"nope", pm=b"nope")):
            a = _good(fields_of)
            a.update(change)
            a.update(bad_methods)
            assert _call(fns[name], a) == EINVAL, (change, bad_methods)
            assert why.encode() in L.mchecksum_gpu_last_error(), (why, L.mchecksum_gpu_last_error())


@pytest.mark.parametrize("name", NAMES)
def test_emethod_comes_before_the_device(calls, name):
    """A header_method that is not a 16-bit model, a payload_method that is not a reflected 32-bit one (a 64-bit one
    among them) and unknown names are EMETHOD with or without a device: -3 here, never -2."""
    fns, fields_of, L = calls
    for change in (dict(hm=b"crc32c"), dict(hm=b"crc64"), dict(hm=b"adler32"), dict(hm=b"no-such-crc"), dict(hm=None),
                   dict(pm=b"crc64"), dict(pm=b"crc64-ecma182"), dict(pm=b"crc16"), dict(pm=b"no-such-crc"),
                   dict(pm=None), dict(hm=b"crc16-ibm-3740", pm=b"crc64-ecma182")):
        for count in (1, 0):
            a = _good(fields_of)
            a.update(change)
            a["count"] = count
            assert _call(fns[name], a) == EMETHOD, (change, count)
            assert b"hash" in L.mchecksum_gpu_last_error(), L.mchecksum_gpu_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_needs_no_arrays_but_passes_the_checks(calls, name):
    fns, fields_of, L = calls
    import torch
    a = _good(fields_of)
    a.update(count=0, addr=None, lens=None, other=None, other_off=None)
    want = 0 if (torch.cuda.is_available() and L.mchecksum_gpu_available()) else ENODEV
    assert _call(fns[name], a) == want
    for hm, pm in ((b"crc16-kermit", b"crc32c"), (b"crc16-ibm-3740", b"crc32")):  # both header bit orders
        assert _call(fns[name], dict(a, hm=hm, pm=pm)) == want
    # ... the checks first: EINVAL, then EMETHOD
    for change, rc in ((dict(kind=5), EINVAL), (dict(hash_=12), EINVAL), (dict(f=fields_of([(XDR_INT, 5)]), nf=1), EINVAL),
                       (dict(hm=b"crc32c"), EMETHOD), (dict(pm=b"crc64"), EMETHOD)):
        b = dict(a)
        b.update(change)
        assert _call(fns[name], b) == rc, change
    # with arrays and a message, a machine without a device says so last of all
    if want == ENODEV:
        assert _call(fns[name], _good(fields_of)) == ENODEV
        assert b"device" in L.mchecksum_gpu_last_error()
