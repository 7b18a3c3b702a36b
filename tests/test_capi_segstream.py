"""C ABI of the streaming and verifying segment entry points
(include/mchecksum_gpu.h): mchecksum_gpu_update_segments,
_update_gather_segments, _update_scatter_segments, _verify_segments and
mchecksum_gpu_state_verify -- exported and bound; the four segment calls check
their arguments in checksum_segments' order (NULL pointers, the segment cap,
the workspace, the device, the method), state_verify in state_get's.  CPU
only: nothing here launches a kernel."""
import ctypes
import subprocess

import pytest

EINVAL, ENODEV, EMETHOD = -1, -2, -3
UPDATE, GATHER, SCATTER, VERIFY = ("mchecksum_gpu_update_segments", "mchecksum_gpu_update_gather_segments",
                                   "mchecksum_gpu_update_scatter_segments", "mchecksum_gpu_verify_segments")
SEG_NAMES = (UPDATE, GATHER, SCATTER, VERIFY)
STATE_VERIFY = "mchecksum_gpu_state_verify"
NARGS = {UPDATE: 10, GATHER: 12, SCATTER: 12, VERIFY: 12, STATE_VERIFY: 7}
NSEG = 3


def _bufs(L):
    ws = L.mchecksum_gpu_segments_work_size(NSEG)
    return dict(addr=(ctypes.c_uint64 * NSEG)(), len=(ctypes.c_uint64 * NSEG)(), first=(ctypes.c_uint64 * 2)(0, NSEG),
                flat=ctypes.create_string_buffer(256), starts=(ctypes.c_uint64 * 1)(8),
                work=(ctypes.c_uint64 * (ws // 8 + 2))(), word=(ctypes.c_uint64 * 1)(0),
                status=(ctypes.c_uint8 * 1)(0), mism=(ctypes.c_uint32 * 1)(0), ws=ws)


def _required(name):
    """The pointers a call with nobj > 0 may not leave out ("word": the states,
    or verify's expected values)."""
    req = ["addr", "len", "first", "work", "word"]
    return req + ["flat", "starts"] if name in (GATHER, SCATTER) else req


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def _addr(x):
    return ctypes.addressof(x) if x is not None and not isinstance(x, int) else x


def _call(L, name, method=b"crc32c", addr=None, len=None, nseg=NSEG, first=None, nobj=1, flat=None, starts=None,
          work=None, ws=0, word=None, status=None, mism=None):
    a, ln, f, fl, st, w, wd, stat, mm = [_addr(v) for v in (addr, len, first, flat, starts, work, word, status, mism)]
    fn = getattr(L, name)
    if name == UPDATE:
        return fn(method, a, ln, nseg, f, nobj, w, ws, wd, None)
    if name == GATHER:
        return fn(method, a, ln, nseg, f, nobj, fl, st, w, ws, wd, None)
    if name == SCATTER:
        return fn(method, fl, st, a, ln, nseg, f, nobj, w, ws, wd, None)
    return fn(method, a, ln, nseg, f, nobj, w, ws, wd, stat, mm, None)


@pytest.mark.parametrize("name", SEG_NAMES + (STATE_VERIFY,))
def test_symbol_is_exported_and_bound(product_lib, name):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert name in exported and name in _lib.GPU_SYMBOLS
    assert len(getattr(product_lib, name).argtypes) == NARGS[name]


@pytest.mark.parametrize("name", SEG_NAMES)
def test_argument_checks(product_lib, name):
    L = product_lib
    ok = _bufs(L)
    cases = [(dict(ok, **{k: None}), "NULL") for k in _required(name)]
    cases += [(dict(ok, nseg=(1 << 40) + 1), "2^40")]
    cases += [(dict(ok, ws=ok["ws"] - 8), "workspace")]  # short
    cases += [(dict(ok, work=ctypes.addressof(ok["work"]) + 4), "workspace")]  # misaligned
    for kw, why in cases:
        for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):  # an argument error outranks the method's
            assert _call(L, name, method, **kw) == EINVAL, (kw, why)
            assert why.encode() in _err(L), (why, _err(L))
    # NULL pointers outrank the cap and the workspace; the cap outranks the workspace
    assert _call(L, name, **dict(ok, word=None, nseg=(1 << 40) + 1, ws=0)) == EINVAL and b"NULL" in _err(L)
    assert _call(L, name, **dict(ok, nseg=(1 << 40) + 1, ws=0)) == EINVAL and b"2^40" in _err(L)


def test_verify_takes_fewer_than_2_pow_32_segments(product_lib):
    """verify_segments keeps its values in the map's region of the workspace,
    and from 2^32 segments on there is no map: refused where the cap is
    checked -- after the NULL pointers, before the workspace, the device and
    the method.  The update calls take such a list as checksum_segments does."""
    L = product_lib
    ok = _bufs(L)
    for method in (b"crc32c", b"crc16", b"no-such-crc"):
        assert _call(L, VERIFY, method, **dict(ok, nseg=1 << 32, ws=0)) == EINVAL and b"2^32" in _err(L)
    assert _call(L, VERIFY, **dict(ok, nseg=1 << 32, ws=0, word=None)) == EINVAL and b"NULL" in _err(L)
    assert _call(L, VERIFY, **dict(ok, nseg=(1 << 32) - 1, ws=0)) == EINVAL and b"workspace" in _err(L)
    assert _call(L, UPDATE, **dict(ok, nseg=1 << 32, ws=0)) == EINVAL and b"workspace" in _err(L)


@pytest.mark.parametrize("name", SEG_NAMES)
def test_optional_and_empty(product_lib, name):
    """nobj == 0: the states / expected values (and the contiguous side) may
    be NULL, the first-segment table and the workspace still may not; the
    checks run first and no launch follows.  verify's status and counter are
    optional at any nobj."""
    import torch
    L = product_lib
    ok = _bufs(L)
    none = dict(ok, nobj=0, flat=None, starts=None, word=None, status=None, mism=None)
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
        # status and counter left out: not an argument error (the device check is what refuses)
        assert _call(L, name, **dict(ok, status=None, mism=None)) == ENODEV


@pytest.mark.parametrize("name", SEG_NAMES)
def test_without_a_device_the_call_refuses(product_lib, name):
    """ENODEV on a box without a GPU, for crc16 and unknown methods too: the
    device check comes before the method's.  With a device, well-formed calls
    on host memory are not made here (tests/test_gpu_segstream.py runs them)."""
    import torch
    L = product_lib
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):
        assert _call(L, name, method, **_bufs(L)) == ENODEV, method
        assert b"no HIP device" in _err(L)


def test_state_verify_arguments(product_lib):
    """state_get's order: NULL pointers (states and expected values, when
    count > 0), the count cap, the device, the method; count == 0 needs no
    buffers; status and counter are optional."""
    import torch
    L = product_lib
    fn = L.mchecksum_gpu_state_verify
    st, ex = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)()
    stat, mism = (ctypes.c_uint8 * 2)(), (ctypes.c_uint32 * 1)()
    a = ctypes.addressof
    for method in (b"crc32c", b"crc64", b"crc16", b"no-such-crc"):
        assert fn(method, None, 2, a(ex), a(stat), a(mism), None) == EINVAL and b"NULL" in _err(L)
        assert fn(method, a(st), 2, None, a(stat), a(mism), None) == EINVAL and b"NULL" in _err(L)
        assert fn(method, a(st), (1 << 31) + 1, a(ex), None, None, None) == EINVAL and b"2^31" in _err(L)
    if torch.cuda.is_available():
        assert fn(b"crc32c", None, 0, None, None, None, None) == 0
        assert fn(b"crc16", None, 0, None, None, None, None) == EMETHOD
        assert fn(b"no-such-crc", a(st), 2, a(ex), None, None, None) == EMETHOD
    else:
        for method in (b"crc32c", b"crc16", b"no-such-crc"):
            assert fn(method, None, 0, None, None, None, None) == ENODEV
            assert fn(method, a(st), 2, a(ex), None, None, None) == ENODEV
            assert b"no HIP device" in _err(L)
