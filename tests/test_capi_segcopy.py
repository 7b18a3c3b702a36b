"""C ABI of the gather / scatter entry points (include/mchecksum_gpu.h):
mchecksum_gpu_gather_segments and mchecksum_gpu_scatter_segments -- exported
and bound, their argument checks in checksum_segments' order (NULL pointers,
then the segment cap, then the workspace, then the device, then the method),
and the wrappers' pure host check of the tables.  CPU only: nothing here
launches a kernel."""
import ctypes
import subprocess

import numpy as np
import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAMES = ("mchecksum_gpu_gather_segments", "mchecksum_gpu_scatter_segments")
NSEG = 3


def _bufs(L):
    ws = L.mchecksum_gpu_segments_work_size(NSEG)
    return dict(addr=(ctypes.c_uint64 * NSEG)(), len=(ctypes.c_uint64 * NSEG)(), first=(ctypes.c_uint64 * 2)(0, NSEG),
                flat=ctypes.create_string_buffer(256), starts=(ctypes.c_uint64 * 1)(8),
                work=(ctypes.c_uint64 * (ws // 8 + 2))(), out=(ctypes.c_uint64 * 1)(0), ws=ws)


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def _addr(x):
    return ctypes.addressof(x) if x is not None and not isinstance(x, int) else x


def _call(L, name, method=b"crc32c", addr=None, len=None, nseg=NSEG, first=None, nobj=1, flat=None, starts=None,
          work=None, ws=0, out=None):
    a = [_addr(v) for v in (addr, len, first, flat, starts, work, out)]
    if name.endswith("gather_segments"):
        return getattr(L, name)(method, a[0], a[1], nseg, a[2], nobj, a[3], a[4], a[5], ws, a[6], None)
    return getattr(L, name)(method, a[3], a[4], a[0], a[1], nseg, a[2], nobj, a[5], ws, a[6], None)


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_exported_and_bound(product_lib, name):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert name in exported and name in _lib.GPU_SYMBOLS
    assert len(getattr(product_lib, name).argtypes) == 12


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks(product_lib, name):
    L = product_lib
    ok = _bufs(L)
    # each required pointer in turn
    cases = [(dict(ok, **{k: None}), "NULL") for k in ("addr", "len", "first", "flat", "starts", "work", "out")]
    cases += [(dict(ok, nseg=(1 << 40) + 1), "2^40")]
    cases += [(dict(ok, ws=ok["ws"] - 8), "workspace")]  # short
    cases += [(dict(ok, work=ctypes.addressof(ok["work"]) + 4), "workspace")]  # misaligned
    for kw, why in cases:
        for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):  # an argument error outranks the method's
            assert _call(L, name, method, **kw) == EINVAL, (kw, why)
            assert why.encode() in _err(L), (why, _err(L))
    # NULL pointers outrank the cap and the workspace; the cap outranks the workspace
    assert _call(L, name, **dict(ok, flat=None, nseg=(1 << 40) + 1, ws=0)) == EINVAL and b"NULL" in _err(L)
    assert _call(L, name, **dict(ok, nseg=(1 << 40) + 1, ws=0)) == EINVAL and b"2^40" in _err(L)


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_needs_no_buffers_but_passes_the_checks_first(product_lib, name):
    """nobj == 0: the contiguous side, its table and the output may be NULL;
    the table of first segments and the workspace still may not."""
    import torch
    L = product_lib
    ok = _bufs(L)
    none = dict(ok, nobj=0, flat=None, starts=None, out=None)
    assert _call(L, name, **none) in (0, ENODEV)
    assert _call(L, name, b"crc64", **none) in (0, ENODEV)
    assert _call(L, name, **dict(none, nseg=0, addr=None, len=None, ws=L.mchecksum_gpu_segments_work_size(0))) in (0, ENODEV)
    assert _call(L, name, **dict(none, first=None)) == EINVAL
    assert _call(L, name, **dict(none, ws=8)) == EINVAL
    if torch.cuda.is_available():
        assert _call(L, name, b"crc16", **none) == EMETHOD
        assert _call(L, name, b"no-such-crc", **none) == EMETHOD
    else:
        assert _call(L, name, b"crc16", **none) == ENODEV


@pytest.mark.parametrize("name", NAMES)
def test_without_a_device_the_call_refuses(product_lib, name):
    """ENODEV on a box without a GPU, for crc16 and unknown methods too: the
    device check comes before the method's.  With a device, well-formed calls
    on host memory are not made here (tests/test_gpu_segcopy.py runs them)."""
    import torch
    L = product_lib
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):
        assert _call(L, name, method, **_bufs(L)) == ENODEV, method
        assert b"no HIP device" in _err(L)


def test_host_table_check_is_pure():
    """_check_segment_tables needs no device and no tensors: addresses and
    lengths as numbers."""
    from mercury_amd.gpu import _check_segment_tables as check
    # 5 segments at "addresses" 1000.., objects {0,1}, {} and {2,3}; segment 4 outside every object
    addr = np.array([1000, 2000, 3000, 3100, 5000], dtype=np.uint64)
    lens = np.array([100, 50, 0, 70, 500], dtype=np.int64)
    first = [0, 2, 2, 4]  # N = 150, 0, 70
    flat_addr, flat_bytes = 100000, 400

    def run(starts, addr=addr, flat_addr=flat_addr, flat_bytes=flat_bytes, first=first):
        check(flat_bytes, flat_addr, np.asarray(starts, dtype=np.uint64), addr, lens, first)

    run([0, 0, 150])  # back to back; the empty object's start is no range
    run([250, 999999, 0])  # any order; an empty object may point anywhere
    run([70, 0, 0])
    run([0, 0, 330])  # ends on the last byte
    run([], first=[3])  # no objects
    with pytest.raises(ValueError, match="overlap"):
        run([0, 0, 149])  # one byte shared
    with pytest.raises(ValueError, match="overlap"):
        run([60, 0, 0])
    with pytest.raises(ValueError, match="past the end"):
        run([0, 0, 331])
    with pytest.raises(ValueError, match="past the end"):
        run([251, 0, 0])
    with pytest.raises(ValueError, match="entries"):
        run([0, 150])
    with pytest.raises(ValueError, match="entries"):
        run([0, 0, 150, 300])
    # the contiguous tensor shares the segments' storage
    with pytest.raises(ValueError, match="segment"):
        run([0, 0, 200], flat_addr=900, flat_bytes=5000)  # [900, 1050) runs into segment 0 at 1000
    with pytest.raises(ValueError, match="segment"):
        run([1200, 0, 3169], flat_addr=0, flat_bytes=9000)  # [3169, 3239): the last byte of segment 3
    run([1200, 0, 3170], flat_addr=0, flat_bytes=9000)  # right behind segment 3
    run([1200, 0, 5100], flat_addr=0, flat_bytes=9000)  # inside segment 4, which belongs to no object
    run([1100, 0, 2990], flat_addr=0, flat_bytes=9000)  # over the empty segment 2's address, up to segment 3


@pytest.mark.parametrize("fn", ["gather", "scatter"])
def test_wrappers_check_the_tables_on_the_host_first(product_lib, fn):
    """SegmentBatch.gather / .scatter run that check with the batch's current
    lengths (set_lengths moves them) before they look at any device.  Without
    a device a batch cannot be built, so the check is driven through a batch
    whose tables are filled in by hand."""
    import torch

    from mercury_amd import gpu as G
    store = torch.zeros(8192, dtype=torch.uint8)
    segs = [store[0:100], store[200:250], store[300:300], store[400:470]]
    b = G.SegmentBatch.__new__(G.SegmentBatch)
    b.nseg, b.nobj, b.device = 4, 3, torch.device("cpu")
    b._addr = np.array([t.data_ptr() for t in segs], dtype=np.uint64)
    b._cap = np.array([t.numel() for t in segs], dtype=np.int64)
    b._lens = b._cap.copy()
    b._first = np.array([0, 2, 2, 4], dtype=np.int64)
    flat = torch.zeros(400, dtype=torch.uint8)

    def run(flat_t, starts):
        out = torch.zeros(3, dtype=torch.int32)
        return getattr(b, fn)("crc32c", flat_t, starts, out)

    with pytest.raises(ValueError, match="overlap"):
        run(flat, [0, 0, 149])
    with pytest.raises(ValueError, match="past the end"):
        run(flat, [0, 0, 331])
    with pytest.raises(ValueError, match="entries"):
        run(flat, [0, 150])
    with pytest.raises(ValueError, match="segment"):
        run(store, [1000, 0, 350])  # [350, 420) runs into the segment at 400
    # tables that pass get as far as the device checks
    for flat_t, starts in ((flat, [0, 0, 150]), (flat, [250, 7, 0]), (store, [1000, 0, 2000])):
        with pytest.raises(G.GpuChecksumError, match="device"):
            run(flat_t, starts)
    # shorter current lengths: what overlapped now fits
    b._lens = np.array([100, 49, 0, 70], dtype=np.int64)
    with pytest.raises(G.GpuChecksumError, match="device"):
        run(flat, [0, 0, 149])
