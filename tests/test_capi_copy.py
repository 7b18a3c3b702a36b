"""C ABI of the copy-and-checksum entry points (include/mchecksum_gpu.h):
mchecksum_gpu_copy_offsets and mchecksum_gpu_update_copy_offsets -- exported
and bound, their argument checks in checksum_offsets' / update_offsets' order
(NULL pointers and the count, then the device, then the method), and the
wrappers' host checks of the two tables, which run before any device check.
CPU only: nothing here launches a kernel."""
import ctypes
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAMES = ("mchecksum_gpu_copy_offsets", "mchecksum_gpu_update_copy_offsets")


def _bufs():
    src = ctypes.create_string_buffer(256)
    dst = ctypes.create_string_buffer(256)
    so = (ctypes.c_uint64 * 2)(0, 64)
    ds = (ctypes.c_uint64 * 1)(8)
    out = (ctypes.c_uint64 * 1)(0)
    return dict(src=src, so=so, dst=dst, ds=ds, out=out)


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def _call(L, name, method=b"crc32c", src=None, so=None, dst=None, ds=None, count=1, out=None):
    return getattr(L, name)(method, src, so, dst, ds, count, out, None)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_bound(product_lib, name):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert name in exported and name in _lib.GPU_SYMBOLS
    assert len(getattr(product_lib, name).argtypes) == 8


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks(product_lib, name):
    L = product_lib
    ok = _bufs()
    cases = [(dict(ok, **{k: None}), "NULL") for k in ("src", "so", "dst", "ds", "out")]  # each required pointer in turn
    cases += [(dict(ok, count=(1 << 31) + 1), "2^31")]
    for kw, why in cases:
        for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):  # an argument error outranks the method's
            assert _call(L, name, method, **kw) == EINVAL, (kw, why)
            assert why.encode() in _err(L), (why, _err(L))


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_needs_no_buffers_but_passes_the_checks_first(product_lib, name):
    import torch
    L = product_lib
    assert _call(L, name, count=0) in (0, ENODEV)
    assert _call(L, name, b"crc64", count=0) in (0, ENODEV)
    if torch.cuda.is_available():
        assert _call(L, name, b"crc16", count=0) == EMETHOD
        assert _call(L, name, b"no-such-crc", count=0) == EMETHOD
    else:
        assert _call(L, name, b"crc16", count=0) == ENODEV


@pytest.mark.parametrize("name", NAMES)
def test_without_a_device_the_call_refuses(product_lib, name):
    """ENODEV on a box without a GPU, for crc16 too: the device check comes
    before the method's.  With a device, well-formed calls on host memory are
    not made here (tests/test_gpu_copy.py runs them)."""
    import torch
    L = product_lib
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):
        assert _call(L, name, method, **_bufs()) == ENODEV, method
        assert b"no HIP device" in _err(L)


@pytest.mark.parametrize("fn", ["copy_offsets", "update_copy_offsets"])
def test_wrappers_check_the_tables_on_the_host_first(product_lib, fn):
    """With both host tables given the wrappers refuse, with ValueError and
    before they look at any device: overlapping destinations, a destination
    past the end of dst, a destination inside the source view of a shared
    storage.  (Host tensors: a table that passed would be refused next, as not
    on a device.)"""
    import torch

    from mercury_amd import gpu as G
    call = getattr(G, fn)
    store = torch.zeros(8192, dtype=torch.uint8)
    src, dst = store[:4096], torch.zeros(1000, dtype=torch.uint8)
    so = np.array([10, 110, 110, 400], dtype=np.uint64)  # 100, 0 and 290 bytes
    sod = torch.from_numpy(so.astype(np.int64))
    state = torch.zeros(3, dtype=torch.int32)

    def run(dst_t, starts):
        ds = np.asarray(starts, dtype=np.uint64)
        return call("crc32c", src, sod, dst_t, torch.from_numpy(ds.astype(np.int64)), state, offsets_host=so,
                    dst_starts_host=ds)

    with pytest.raises(ValueError, match="overlap"):
        run(dst, [300, 0, 399 - 289])  # the third range ends inside the first
    with pytest.raises(ValueError, match="overlap"):
        run(dst, [0, 50, 99])  # one byte shared; the empty chunk in between is no range
    with pytest.raises(ValueError, match="past the end"):
        run(dst, [0, 0, 711])  # 711 + 290 = 1001
    with pytest.raises(ValueError, match="source"):
        run(store, [4096, 0, 399])  # dst shares src's storage: [399, 689) lies in the source range [10, 400)
    with pytest.raises(ValueError, match="one entry more"):
        run(dst, [0, 100])
    # tables that pass get as far as the device checks
    for dst_t, starts in ((dst, [0, 50, 100]), (dst, [710, 5, 100]), (store, [4096, 0, 400]), (store, [4096, 0, 5000])):
        with pytest.raises(G.GpuChecksumError, match="device"):
            run(dst_t, starts)
