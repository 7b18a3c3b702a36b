"""C ABI of the receiver's copying entry point (include/mchecksum_gpu.h):
mchecksum_gpu_unpack_messages -- exported and bound, its argument checks in
the sender calls' order (layout, then method, then device), so that every
error reads the same with and without a GPU.  CPU only: nothing here launches
a kernel."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAME = "mchecksum_gpu_unpack_messages"


def _bufs():
    buf = ctypes.create_string_buffer(256)
    dst = ctypes.create_string_buffer(256)
    mo = (ctypes.c_uint64 * 2)(0, 84)
    do = (ctypes.c_uint64 * 2)(0, 64)
    return buf, mo, dst, do


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def _call(L, method=b"crc32c", buf=None, mo=None, count=1, pay=20, hsh=16, dst=None, do=None):
    return L.mchecksum_gpu_unpack_messages(method, buf, mo, count, pay, hsh, dst, do, None, None, None)


def test_symbol_is_exported_and_bound(product_lib):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NAME in exported and NAME in _lib.GPU_SYMBOLS
    assert len(getattr(product_lib, NAME).argtypes) == 11


def test_argument_checks(product_lib):
    L = product_lib
    buf, mo, dst, do = _bufs()
    ok = dict(buf=buf, mo=mo, dst=dst, do=do)
    cases = [(dict(ok, pay=18), "hash_offset"),  # the hash slot overlaps the payload
             (dict(ok, pay=19), "hash_offset")]
    cases += [(dict(ok, **{k: None}), "NULL") for k in ("buf", "mo", "dst", "do")]  # each required pointer in turn
    cases += [(dict(ok, count=(1 << 31) + 1), "2^31")]
    for kw, why in cases:
        assert _call(L, **kw) == EINVAL, (kw, why)
        assert why.encode() in _err(L), (why, _err(L))


def test_method_checks_come_before_the_device(product_lib):
    L = product_lib
    buf, mo, dst, do = _bufs()
    for m in (b"crc64", b"crc16"):
        assert _call(L, m, buf, mo, dst=dst, do=do) == EMETHOD, m
    assert _call(L, b"crc64", buf, mo, dst=dst, do=do) == EMETHOD
    assert b"crc32c only" in _err(L)
    assert _call(L, b"no-such-crc", buf, mo, dst=dst, do=do) == EMETHOD
    assert b"unknown hash method" in _err(L)
    # a layout error outranks a method error
    assert _call(L, b"crc64", buf, mo, pay=18, dst=dst, do=do) == EINVAL
    assert _call(L, b"crc64", None, mo, dst=dst, do=do) == EINVAL


def test_empty_batch_needs_no_buffers_but_passes_the_checks_first(product_lib):
    L = product_lib
    assert _call(L, count=0) in (0, ENODEV)
    assert _call(L, count=0, pay=18) == EINVAL
    assert _call(L, b"crc64", count=0) == EMETHOD
    assert _call(L, b"crc64", count=0, pay=18) == EINVAL


def test_without_a_device_the_call_refuses(product_lib):
    """ENODEV on a box without a GPU; with one, well-formed calls on host
    memory are not made here (tests/test_gpu_receiver.py runs them)."""
    import torch
    L = product_lib
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    buf, mo, dst, do = _bufs()
    assert _call(L, b"crc32c", buf, mo, dst=dst, do=do) == ENODEV
    assert b"no HIP device" in _err(L)


def test_compiled_receiver_is_built_in_tree_and_refuses_without_a_device(product_lib):
    """`make` leaves build/hg_unpack_consumer (tests/native/hg_unpack_consumer.c)
    for the GPU box; without a device it sees the entry point refuse."""
    import torch
    exe = os.path.join(ROOT, "build", "hg_unpack_consumer")
    assert os.access(exe, os.X_OK), "run make"
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("NODEV"), r.stdout
