"""C ABI of the sender entry points (include/mchecksum_gpu.h):
mchecksum_gpu_seal_messages, mchecksum_gpu_pack_messages and
mchecksum_gpu_seal_core_headers -- exported, and their argument checks in the
order of their verify twins, with the method checked before the device (so a
wrong method reads the same with and without a GPU).  CPU only: nothing here
launches a kernel."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, EMETHOD = -1, -2, -3
NAMES = ("mchecksum_gpu_seal_messages", "mchecksum_gpu_pack_messages", "mchecksum_gpu_seal_core_headers")


def _bufs():
    buf = ctypes.create_string_buffer(256)
    src = ctypes.create_string_buffer(256)
    mo = (ctypes.c_uint64 * 2)(0, 84)
    so = (ctypes.c_uint64 * 2)(0, 64)
    return buf, src, mo, so


def _err(L):
    return L.mchecksum_gpu_last_error() or b""


def test_sender_symbols_are_exported_and_bound(product_lib):
    from mercury_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in NAMES:
        assert n in exported and n in _lib.GPU_SYMBOLS
        assert getattr(product_lib, n).argtypes, n


def test_without_a_device_the_calls_refuse(product_lib):
    """ENODEV on a box without a GPU; with one, well-formed calls on host
    memory are not made here (tests/test_gpu_sender.py runs them)."""
    import torch
    L = product_lib
    if torch.cuda.is_available():
        assert L.mchecksum_gpu_available() == 1
        return
    buf, src, mo, so = _bufs()
    assert L.mchecksum_gpu_seal_messages(b"crc32c", buf, mo, 1, 20, 16, None, None) == ENODEV
    assert L.mchecksum_gpu_pack_messages(b"crc32c", src, so, buf, mo, 1, 20, 16, None, None) == ENODEV
    assert L.mchecksum_gpu_seal_core_headers(b"crc16", 0, buf, mo, 1, None, None) == ENODEV
    assert b"no HIP device" in _err(L)


def test_argument_checks(product_lib):
    L = product_lib
    buf, src, mo, so = _bufs()
    cases = [
        # hash slot overlapping the payload
        (lambda: L.mchecksum_gpu_seal_messages(b"crc32c", buf, mo, 1, 18, 16, None, None), "hash_offset"),
        (lambda: L.mchecksum_gpu_pack_messages(b"crc32c", src, so, buf, mo, 1, 19, 16, None, None), "hash_offset"),
        # NULL with count > 0, each pointer in turn
        (lambda: L.mchecksum_gpu_seal_messages(b"crc32c", None, mo, 1, 20, 16, None, None), "NULL"),
        (lambda: L.mchecksum_gpu_seal_messages(b"crc32c", buf, None, 1, 20, 16, None, None), "NULL"),
        (lambda: L.mchecksum_gpu_pack_messages(b"crc32c", None, so, buf, mo, 1, 20, 16, None, None), "NULL"),
        (lambda: L.mchecksum_gpu_pack_messages(b"crc32c", src, None, buf, mo, 1, 20, 16, None, None), "NULL"),
        (lambda: L.mchecksum_gpu_pack_messages(b"crc32c", src, so, None, mo, 1, 20, 16, None, None), "NULL"),
        (lambda: L.mchecksum_gpu_pack_messages(b"crc32c", src, so, buf, None, 1, 20, 16, None, None), "NULL"),
        (lambda: L.mchecksum_gpu_seal_core_headers(b"crc16", 0, None, mo, 1, None, None), "NULL"),
        (lambda: L.mchecksum_gpu_seal_core_headers(b"crc16", 0, buf, None, 1, None, None), "NULL"),
        # the count cap and the kind, as the verify twins
        (lambda: L.mchecksum_gpu_seal_messages(b"crc32c", buf, mo, (1 << 31) + 1, 20, 16, None, None), "2^31"),
        (lambda: L.mchecksum_gpu_pack_messages(b"crc32c", src, so, buf, mo, (1 << 31) + 1, 20, 16, None, None), "2^31"),
        (lambda: L.mchecksum_gpu_seal_core_headers(b"crc16", 7, buf, mo, 1, None, None), "kind"),
    ]
    for call, why in cases:
        assert call() == EINVAL, why
        assert why.encode() in _err(L), (why, _err(L))


def test_method_checks(product_lib):
    L = product_lib
    buf, src, mo, so = _bufs()
    assert L.mchecksum_gpu_seal_messages(b"crc64", buf, mo, 1, 20, 16, None, None) == EMETHOD
    assert b"crc32c only" in _err(L)
    assert L.mchecksum_gpu_pack_messages(b"crc64", src, so, buf, mo, 1, 20, 16, None, None) == EMETHOD
    assert b"crc32c only" in _err(L)
    assert L.mchecksum_gpu_seal_messages(b"crc16", buf, mo, 1, 20, 16, None, None) == EMETHOD
    assert L.mchecksum_gpu_pack_messages(b"no-such-crc", src, so, buf, mo, 1, 20, 16, None, None) == EMETHOD
    assert L.mchecksum_gpu_seal_core_headers(b"crc32c", 0, buf, mo, 1, None, None) == EMETHOD
    assert b"16-bit" in _err(L)


def test_empty_batch_needs_no_buffers_but_passes_the_checks_first(product_lib):
    """count == 0 with NULL buffers is valid (0 with a device, ENODEV without
    one) -- after the argument checks, in verify_messages' order: layout, then
    method, then device."""
    L = product_lib
    assert L.mchecksum_gpu_seal_messages(b"crc32c", None, None, 0, 20, 16, None, None) in (0, ENODEV)
    assert L.mchecksum_gpu_pack_messages(b"crc32c", None, None, None, None, 0, 20, 16, None, None) in (0, ENODEV)
    assert L.mchecksum_gpu_seal_messages(b"crc32c", None, None, 0, 18, 16, None, None) == EINVAL
    assert L.mchecksum_gpu_pack_messages(b"crc32c", None, None, None, None, 0, 18, 16, None, None) == EINVAL
    assert L.mchecksum_gpu_seal_messages(b"crc64", None, None, 0, 20, 16, None, None) == EMETHOD
    assert L.mchecksum_gpu_pack_messages(b"crc64", None, None, None, None, 0, 20, 16, None, None) == EMETHOD
    # a layout error outranks a method error
    assert L.mchecksum_gpu_seal_messages(b"crc64", None, None, 0, 18, 16, None, None) == EINVAL
    # seal_core_headers keeps verify_core_headers' rule: the table pointer is always needed
    mo = (ctypes.c_uint64 * 1)(0)
    assert L.mchecksum_gpu_seal_core_headers(b"crc16", 1, None, mo, 0, None, None) in (0, ENODEV)
    assert L.mchecksum_gpu_seal_core_headers(b"crc16", 1, None, None, 0, None, None) == EINVAL
    assert L.mchecksum_gpu_seal_core_headers(b"crc16", 7, None, mo, 0, None, None) == EINVAL


def test_compiled_sender_is_built_in_tree_and_refuses_without_a_device(product_lib):
    """`make` leaves build/hg_seal_consumer (tests/native/hg_seal_consumer.c)
    for the GPU box; without a device it sees all three entry points refuse."""
    import torch
    exe = os.path.join(ROOT, "build", "hg_seal_consumer")
    assert os.access(exe, os.X_OK), "run make"
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("NODEV"), r.stdout
