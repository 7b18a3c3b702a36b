"""C ABI of the per-field message calls (include/mchecksum_gpu.h):
mchecksum_gpu_pack_segment_messages, mchecksum_gpu_unpack_segment_messages and
mchecksum_gpu_segment_messages_work_size -- exported and bound, the argument
checks in the order the header gives (NULL pointers, the header layout, the
object cap, the segment cap, the workspace; then the method, crc32c only; then
the device), the empty batch, and the size function.  CPU only: nothing here
launches a kernel."""
import ctypes
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
PACK, UNPACK = "mchecksum_gpu_pack_segment_messages", "mchecksum_gpu_unpack_segment_messages"
NAMES = (PACK, UNPACK)
NSEG, NOBJ = 3, 2
SIZE_MAX = ctypes.c_size_t(-1).value


def _bufs(L):
    ws = L.mchecksum_gpu_segment_messages_work_size(NSEG, NOBJ)
    return dict(addr=(ctypes.c_uint64 * NSEG)(), len=(ctypes.c_uint64 * NSEG)(), first=(ctypes.c_uint64 * 3)(0, 2, 3),
                buf=ctypes.create_string_buffer(256), off=(ctypes.c_uint64 * 3)(0, 20, 40),
                work=(ctypes.c_uint64 * (ws // 8 + 2))(), ws=ws, status=(ctypes.c_uint8 * NOBJ)(),
                mism=(ctypes.c_uint32 * 1)())


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def _addr(x):
    return ctypes.addressof(x) if x is not None and not isinstance(x, int) else x


def _call(L, name, method=b"crc32c", addr=None, len=None, nseg=NSEG, first=None, nobj=NOBJ, buf=None, off=None,
          pay=20, hoff=16, work=None, ws=0, status=None, mism=None):
    a, ln, f, b, o, w, st, mi = (_addr(v) for v in (addr, len, first, buf, off, work, status, mism))
    if name == PACK:
        return getattr(L, name)(method, a, ln, nseg, f, nobj, b, o, pay, hoff, w, ws, st, None)
    return getattr(L, name)(method, b, o, nobj, pay, hoff, a, ln, nseg, f, w, ws, st, mi, None)


def test_symbols_are_exported_and_bound(product_lib):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, nargs in ((PACK, 14), (UNPACK, 15), ("mchecksum_gpu_segment_messages_work_size", 2)):
        assert name in exported and name in _lib.GPU_SYMBOLS
        assert len(getattr(product_lib, name).argtypes) == nargs


def test_wrappers_are_reachable():
    from mercury_amd import gpu as G
    assert callable(G.SegmentBatch.pack_messages) and callable(G.SegmentBatch.unpack_messages)
    assert callable(G.pack_segment_messages) and callable(G.unpack_segment_messages)


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks(product_lib, name):
    L = product_lib
    ok = _bufs(L)
    cases = [(dict(ok, **{k: None}), "NULL") for k in ("addr", "len", "first", "buf", "off", "work")]
    cases += [(dict(ok, pay=20, hoff=17), "hash_offset")]
    cases += [(dict(ok, pay=3, hoff=0), "hash_offset")]
    cases += [(dict(ok, nobj=(1 << 31) + 1), "2^31")]
    cases += [(dict(ok, nseg=1 << 32), "2^32")]
    cases += [(dict(ok, nseg=(1 << 40) + 1), "2^32")]
    cases += [(dict(ok, ws=ok["ws"] - 8), "workspace")]  # short
    cases += [(dict(ok, ws=L.mchecksum_gpu_segments_work_size(NSEG)), "workspace")]  # the plain segment calls' size
    cases += [(dict(ok, work=ctypes.addressof(ok["work"]) + 4), "workspace")]  # misaligned
    for kw, why in cases:
        for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):  # an argument error outranks the method's
            assert _call(L, name, method, **kw) == EINVAL, (kw, why)
            assert why.encode() in _err(L), (why, _err(L))
    # the order among them: NULL, the header layout, the object cap, the segment cap, the workspace
    bad = dict(ok, hoff=17, nobj=(1 << 31) + 1, nseg=1 << 32, ws=0)
    assert _call(L, name, **dict(bad, buf=None)) == EINVAL and b"NULL" in _err(L)
    assert _call(L, name, **bad) == EINVAL and b"hash_offset" in _err(L)
    assert _call(L, name, **dict(bad, hoff=16)) == EINVAL and b"2^31" in _err(L)
    assert _call(L, name, **dict(bad, hoff=16, nobj=NOBJ)) == EINVAL and b"2^32" in _err(L)
    assert _call(L, name, **dict(bad, hoff=16, nobj=NOBJ, nseg=NSEG)) == EINVAL and b"workspace" in _err(L)
    # the optional outputs are no argument errors
    assert _call(L, name, **dict(ok, status=None, mism=None)) in (0, ENODEV)
    # no segments at all: the segment arrays may be NULL
    none = dict(ok, nseg=0, addr=None, len=None, first=(ctypes.c_uint64 * 3)(0, 0, 0),
                ws=L.mchecksum_gpu_segment_messages_work_size(0, NOBJ))
    assert _call(L, name, **none) in (0, ENODEV)


@pytest.mark.parametrize("name", NAMES)
def test_method_is_checked_after_the_arguments_and_before_the_device(product_lib, name):
    """crc32c only, as pack_messages: every other name -- a known method or
    not -- is EMETHOD, on a box without a GPU too."""
    L = product_lib
    ok = _bufs(L)
    for method in (b"crc64", b"crc32", b"crc16", b"no-such-crc"):
        assert _call(L, name, method, **ok) == EMETHOD, method
        assert _call(L, name, method, nobj=0) == EMETHOD, method  # an empty batch passes the same checks


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_needs_no_buffers(product_lib, name):
    """nobj == 0 with every buffer NULL (the workspace included) is valid: 0
    with a device, ENODEV without one -- never EINVAL; the layout check still
    applies."""
    L = product_lib
    assert _call(L, name, nobj=0) in (0, ENODEV)
    assert _call(L, name, nobj=0, nseg=0) in (0, ENODEV)
    assert _call(L, name, nobj=0, hoff=17) == EINVAL and b"hash_offset" in _err(L)


@pytest.mark.parametrize("name", NAMES)
def test_without_a_device_the_call_refuses(product_lib, name):
    import torch
    L = product_lib
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    assert _call(L, name, **_bufs(L)) == ENODEV
    assert b"no HIP device" in _err(L)


def test_work_size(product_lib):
    L = product_lib
    size, seg = L.mchecksum_gpu_segment_messages_work_size, L.mchecksum_gpu_segments_work_size
    prev = 0
    for nseg in (0, 1, 2, 1023, 1024, 1025, 4096, 100000, 1 << 24, (1 << 32) - 1):
        row = [size(nseg, nobj) for nobj in (0, 1, 2, 7, 8, 9, 1000, 1 << 20, 1 << 31)]
        assert row == sorted(row), (nseg, row)  # monotonic in nobj ...
        assert row[0] >= prev  # ... and in nseg
        prev = row[0]
        assert all(r >= seg(nseg) and r % 8 == 0 and r != SIZE_MAX for r in row)
        # per object: the accumulator word (4 bytes) and the gate (1 byte), no more than rounding on top
        assert size(nseg, 1000) - size(nseg, 0) == 4000 + 1000
    assert size(1 << 32, 1) == SIZE_MAX and size(1 << 40, 1) == SIZE_MAX
    assert size(1, (1 << 31) + 1) == SIZE_MAX
    assert size((1 << 32) - 1, 1 << 31) != SIZE_MAX


def test_host_table_checks_of_the_wrappers(product_lib):
    """SegmentBatch.pack_messages / .unpack_messages check host tables before
    they look at any device (a batch filled in by hand, as
    tests/test_capi_segcopy.py does)."""
    import torch

    from mercury_amd import gpu as G
    store = torch.zeros(8192, dtype=torch.uint8)
    segs = [store[0:100], store[200:250], store[300:300], store[400:470]]
    b = G.SegmentBatch.__new__(G.SegmentBatch)
    b.nseg, b.nobj, b.device = 4, 3, torch.device("cpu")
    b._addr = np.array([t.data_ptr() for t in segs], dtype=np.uint64)
    b._cap = np.array([t.numel() for t in segs], dtype=np.int64)
    b._lens = b._cap.copy()
    b._first = np.array([0, 2, 2, 4], dtype=np.int64)  # N = 150, 0, 70
    data = torch.zeros(400, dtype=torch.uint8)
    for fn in (b.pack_messages, b.unpack_messages):
        with pytest.raises(ValueError, match="entries"):
            fn(data, [0, 170, 190])
        with pytest.raises(ValueError, match="non-decreasing"):
            fn(data, [0, 170, 160, 280])
        with pytest.raises(ValueError, match="past the end of data"):
            fn(data, [0, 170, 190, 401])
        with pytest.raises(ValueError, match="segment"):
            fn(store, [320, 490, 510, 600])  # message 0's payload [340, 490) runs over the segment at 400
        # tables that pass get as far as the device checks; a message that does not fit is no range
        for tbl in ([0, 170, 190, 280], [0, 170, 190, 400], [10, 10, 30, 120]):
            with pytest.raises(G.GpuChecksumError, match="device"):
                fn(data, tbl)
