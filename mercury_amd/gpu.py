"""Batch checksums of device-resident payloads on MI355X (include/mchecksum_gpu.h).

Thin torch-facing wrappers over the C ABI: torch only provides device memory
and streams here.  Every function checks tensor shapes, dtypes and bounds on
the host before the kernel launch and raises on any error -- there is no CPU
fallback.  Offsets tables live on the device: they are bounds-checked when a
host copy is passed (offsets_host=...), otherwise trusted, as in the C ABI.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import load_bench_library, load_library

_WIDTH = {"crc32c": 4, "crc32": 4, "crc64": 8}


class GpuChecksumError(RuntimeError):
    pass


def _lib():
    return load_library()


def _err(rc: int, what: str):
    msg = _lib().mchecksum_gpu_last_error()
    raise GpuChecksumError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def out_dtype(method: str) -> torch.dtype:
    w = _WIDTH.get(method, 8 if method.startswith("crc64") else 4)
    return torch.int32 if w == 4 else torch.int64


def _stream_handle(stream, device=None) -> int:
    """hipStream_t for a call on `device` (the data tensor's device): None =
    that device's current stream; a torch stream must belong to it."""
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream
    if hasattr(stream, "cuda_stream"):
        if device is not None and getattr(stream, "device", device) != device:
            raise GpuChecksumError(f"stream belongs to {stream.device}, data to {device}")
        return stream.cuda_stream
    return int(stream)


def _same_device(data: torch.Tensor, **tensors):
    """Every tensor argument must live on data's device: the library launches
    on the current device, which _on(data) makes data's."""
    for name, t in tensors.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.device != data.device):
            raise GpuChecksumError(f"{name} must be a tensor on {data.device}")


def _on(data: torch.Tensor):
    """Make data's device current for the call (the C library picks its table
    pack and queue slot from hipGetDevice())."""
    return torch.cuda.device(data.device)


def _check_device_u8(t: torch.Tensor, name: str):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GpuChecksumError(f"{name} must be a device (cuda/hip) tensor")
    if not t.is_contiguous():
        raise GpuChecksumError(f"{name} must be contiguous")


def gpu_available() -> bool:
    return bool(_lib().mchecksum_gpu_available())


def queue_faults() -> int:
    """Work-queue protocol faults the batch kernels counted on the current
    device since load (bounded waits that gave up; 0 when healthy).
    Synchronizes the device."""
    return int(_lib().mchecksum_gpu_queue_faults())


QSTAT_KEYS = ("slot", "noslot", "reaped", "busy_skip", "in_flight")


def queue_stats() -> dict:
    """Work-queue slot bookkeeping of the current device (mchecksum_gpu_queue_stats):
    launches given a slot, launches without one (graph captures, no idle slot),
    slots reaped back into the idle pool, busy in-flight slots looked at while
    reaping, slots handed out and not yet reaped."""
    import ctypes
    buf = (ctypes.c_longlong * len(QSTAT_KEYS))()
    rc = _lib().mchecksum_gpu_queue_stats(buf, len(QSTAT_KEYS))
    if rc:
        _err(rc, "queue_stats")
    return dict(zip(QSTAT_KEYS, (int(v) for v in buf)))


def set_error_word(word: torch.Tensor | None) -> None:
    """Fail-closed report (mchecksum_gpu_set_error_word): every later batch call
    of this host thread adds 1 to `word` (a one-element device int32 tensor the
    caller zeroes) when its launch could not hash every payload.  None turns
    the report off.  Keep the tensor alive while it is set."""
    if word is not None and (word.dtype != torch.int32 or not word.is_cuda or word.numel() < 1):
        raise GpuChecksumError("error word must be a device int32 tensor")
    _lib().mchecksum_gpu_set_error_word(word.data_ptr() if word is not None else None)


def prepare(method: str = "crc32c") -> None:
    rc = _lib().mchecksum_gpu_prepare(method.encode())
    if rc != 0:
        _err(rc, f"mchecksum_gpu_prepare({method})")


def lanes_per_payload(method: str, length: int) -> int:
    return int(_lib().mchecksum_gpu_lanes_per_payload(method.encode(), length))


def checksum_fixed(method: str, data: torch.Tensor, length: int, count: int | None = None,
                   stride: int | None = None, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """CRC of payload i = data[i*stride : i*stride+length] for i < count.

    Returns a device tensor (int32 for crc32c, int64 for crc64) holding the
    host-order CRC values (reinterpret as unsigned)."""
    _check_device_u8(data, "data")
    nbytes = data.numel() * data.element_size()
    stride = length if stride is None else stride
    if count is None:
        count = nbytes // stride if stride else 0
    if count and (count - 1) * stride + length > nbytes:
        raise GpuChecksumError("batch extends past the end of data")
    if count > 1 and stride < length:
        raise GpuChecksumError("stride smaller than length")
    if out is None:
        out = torch.empty(count, dtype=out_dtype(method), device=data.device)
    elif out.numel() < count or out.dtype != out_dtype(method) or not out.is_cuda or not out.is_contiguous():
        raise GpuChecksumError("out tensor has the wrong size, dtype or device, or is not contiguous")
    _same_device(data, out=out)
    with _on(data):
        rc = _lib().mchecksum_gpu_checksum_fixed(method.encode(), data.data_ptr(), stride, length, count,
                                                 out.data_ptr(), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_checksum_fixed")
    return out


def _check_offsets(data, offsets, offsets_host):
    if offsets.dtype != torch.int64 or not offsets.is_cuda or not offsets.is_contiguous():
        raise GpuChecksumError("offsets must be a contiguous device int64 tensor")
    if offsets_host is not None:
        import numpy as np
        oh = np.asarray(offsets_host, dtype=np.uint64)
        if len(oh) != offsets.numel():
            raise GpuChecksumError("offsets_host does not match offsets")
        if len(oh) > 1 and (np.any(oh[1:] < oh[:-1])):
            raise GpuChecksumError("offsets must be non-decreasing")
        if len(oh) and int(oh[-1]) > data.numel() * data.element_size():
            raise GpuChecksumError("offsets extend past the end of data")


def checksum_offsets(method: str, data: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor | None = None,
                     stream=None, offsets_host=None) -> torch.Tensor:
    """CRC of payload i = data[offsets[i] : offsets[i+1]] (offsets: count+1 int64).

    Pass offsets_host (a host copy) to have the table validated before launch."""
    _check_device_u8(data, "data")
    _check_offsets(data, offsets, offsets_host)
    count = offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("offsets needs at least one entry")
    if out is None:
        out = torch.empty(count, dtype=out_dtype(method), device=data.device)
    elif out.numel() < count or out.dtype != out_dtype(method) or not out.is_cuda or not out.is_contiguous():
        raise GpuChecksumError("out tensor has the wrong size, dtype or device, or is not contiguous")
    _same_device(data, offsets=offsets, out=out)
    with _on(data):
        rc = _lib().mchecksum_gpu_checksum_offsets(method.encode(), data.data_ptr(), offsets.data_ptr(), count,
                                                   out.data_ptr(), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_checksum_offsets")
    return out


def _check_state(t, method: str, count: int, name: str):
    if (not isinstance(t, torch.Tensor) or t.numel() < count or t.dtype != out_dtype(method) or not t.is_cuda
            or not t.is_contiguous()):
        raise GpuChecksumError(f"{name} tensor has the wrong size, dtype or device, or is not contiguous")


def state_init(method: str, count: int, device=None, stream=None) -> torch.Tensor:
    """Running state of `count` streams (mchecksum_gpu_state_init): a device
    tensor of the method's size, opaque -- feed it to update_offsets and read
    it with state_get."""
    if count < 0:
        raise GpuChecksumError("count must not be negative")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise GpuChecksumError("device must be a cuda/hip device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    state = torch.empty(count, dtype=out_dtype(method), device=device)
    with _on(state):
        rc = _lib().mchecksum_gpu_state_init(method.encode(), state.data_ptr(), count, _stream_handle(stream, device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_state_init")
    return state


def update_offsets(method: str, data: torch.Tensor, offsets: torch.Tensor, state: torch.Tensor, stream=None,
                   offsets_host=None) -> torch.Tensor:
    """Advance state[i] over data[offsets[i] : offsets[i+1]] in place (an empty
    chunk leaves it unchanged).  Returns state."""
    _check_device_u8(data, "data")
    _check_offsets(data, offsets, offsets_host)
    count = offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("offsets needs at least one entry")
    _check_state(state, method, count, "state")
    _same_device(data, offsets=offsets, state=state)
    with _on(data):
        rc = _lib().mchecksum_gpu_update_offsets(method.encode(), data.data_ptr(), offsets.data_ptr(), count,
                                                 state.data_ptr(), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_update_offsets")
    return state


def _check_copy_tables(src, dst, offsets_host, dst_starts_host):
    """Host check of a copy call's two tables (ValueError): every destination
    range inside dst, the ranges pairwise disjoint, and disjoint from the source
    range -- compared by address, so a dst that shares src's storage is
    covered.  Runs before the device checks: it needs no device."""
    import numpy as np
    so = np.asarray(offsets_host, dtype=np.uint64).astype(np.int64)
    ds = np.asarray(dst_starts_host, dtype=np.uint64).astype(np.int64)
    if so.ndim != 1 or ds.ndim != 1 or len(so) != len(ds) + 1:
        raise ValueError("offsets_host needs one entry more than dst_starts_host")
    if np.any(so < 0) or np.any(ds < 0) or np.any(so[1:] < so[:-1]):
        raise ValueError("offsets must be non-decreasing")
    lens = so[1:] - so[:-1]
    if np.any(ds + lens > dst.numel() * dst.element_size()):
        raise ValueError("a destination range extends past the end of dst")
    live = lens > 0
    lo, hi = ds[live], (ds + lens)[live]
    order = np.argsort(lo, kind="stable")
    lo, hi = lo[order], hi[order]
    if np.any(hi[:-1] > lo[1:]):
        raise ValueError("two destination ranges overlap")
    if lo.size and src.device == dst.device:
        s0, s1 = src.data_ptr() + int(so[0]), src.data_ptr() + int(so[-1])
        d = dst.data_ptr()
        if np.any((lo + d < s1) & (hi + d > s0)):
            raise ValueError("a destination range overlaps the source range")


def _copy_call(name, method, src, src_offsets, dst, dst_starts, out, stream, offsets_host, dst_starts_host):
    if not isinstance(src, torch.Tensor) or not isinstance(dst, torch.Tensor):
        raise GpuChecksumError("src and dst must be tensors")
    if offsets_host is not None and dst_starts_host is not None:
        _check_copy_tables(src, dst, offsets_host, dst_starts_host)
    _check_device_u8(src, "src")
    _check_device_u8(dst, "dst")
    _check_offsets(src, src_offsets, offsets_host)
    count = src_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("src_offsets needs at least one entry")
    if (not isinstance(dst_starts, torch.Tensor) or dst_starts.dtype != torch.int64 or not dst_starts.is_cuda
            or not dst_starts.is_contiguous() or dst_starts.numel() != count):
        raise GpuChecksumError("dst_starts must be a contiguous device int64 tensor of count elements")
    _check_state(out, method, count, "out" if name == "mchecksum_gpu_copy_offsets" else "state")
    _same_device(src, src_offsets=src_offsets, dst=dst, dst_starts=dst_starts, out=out)
    with _on(src):
        rc = getattr(_lib(), name)(method.encode(), src.data_ptr(), src_offsets.data_ptr(), dst.data_ptr(),
                                   dst_starts.data_ptr(), count, out.data_ptr(), _stream_handle(stream, src.device))
    if rc != 0:
        _err(rc, name)
    return out


def copy_offsets(method: str, src: torch.Tensor, src_offsets: torch.Tensor, dst: torch.Tensor,
                 dst_starts: torch.Tensor, out: torch.Tensor | None = None, stream=None, offsets_host=None,
                 dst_starts_host=None) -> torch.Tensor:
    """checksum_offsets that also copies, in one pass: chunk i = src[src_offsets[i]
    : src_offsets[i+1]] (n_i bytes) goes to dst[dst_starts[i] : dst_starts[i] +
    n_i] and its CRC to out[i].  dst_starts (count int64) may be in any order;
    only those bytes of dst are written.  The destination ranges must not
    overlap one another or the source: with both host tables given that, and
    that every range lies inside dst, is checked here (ValueError) before any
    launch; otherwise the tables are trusted as in the C ABI."""
    if out is None and isinstance(src, torch.Tensor) and isinstance(src_offsets, torch.Tensor):
        out = torch.empty(max(src_offsets.numel() - 1, 0), dtype=out_dtype(method), device=src.device)
    return _copy_call("mchecksum_gpu_copy_offsets", method, src, src_offsets, dst, dst_starts, out, stream,
                      offsets_host, dst_starts_host)


def update_copy_offsets(method: str, src: torch.Tensor, src_offsets: torch.Tensor, dst: torch.Tensor,
                        dst_starts: torch.Tensor, state: torch.Tensor, stream=None, offsets_host=None,
                        dst_starts_host=None) -> torch.Tensor:
    """update_offsets that also copies, in one pass: state[i] is advanced over
    chunk i, which goes to dst[dst_starts[i] : ...] (copy_offsets' layout, rules
    and host checks).  An empty chunk writes nothing and leaves its state
    unchanged.  Returns state."""
    return _copy_call("mchecksum_gpu_update_copy_offsets", method, src, src_offsets, dst, dst_starts, state, stream,
                      offsets_host, dst_starts_host)


def state_get(method: str, state: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """The CRC of every stream's bytes so far (host-order values, as the
    checksum_* calls return them).  The state is left as it is."""
    count = state.numel() if isinstance(state, torch.Tensor) else 0
    _check_state(state, method, count, "state")
    if out is None:
        out = torch.empty(count, dtype=out_dtype(method), device=state.device)
    _check_state(out, method, count, "out")
    _same_device(state, out=out)
    with _on(state):
        rc = _lib().mchecksum_gpu_state_get(method.encode(), state.data_ptr(), count, out.data_ptr(),
                                            _stream_handle(stream, state.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_state_get")
    return out


def _verdict_buffers(count: int, device, status, mismatches):
    """The status / counter pair of a verify call: None allocates (status
    starts "failed", the counter at zero), False passes NULL to the library, a
    tensor is used as it is (the call adds to a counter the caller zeroed)."""
    if status is None:
        status = torch.ones(max(count, 0), dtype=torch.uint8, device=device)
    elif status is not False and (not isinstance(status, torch.Tensor) or status.dtype != torch.uint8
                                  or status.numel() < count or not status.is_cuda or not status.is_contiguous()):
        raise GpuChecksumError("status must be a contiguous device uint8 tensor of at least count elements")
    if mismatches is None:
        mismatches = torch.zeros(1, dtype=torch.int32, device=device)
    elif mismatches is not False and (not isinstance(mismatches, torch.Tensor) or mismatches.dtype != torch.int32
                                      or not mismatches.is_cuda or mismatches.numel() < 1):
        raise GpuChecksumError("mismatches must be a device int32 tensor")
    for name, t in (("status", status), ("mismatches", mismatches)):
        if t is not False and t.device != device:
            raise GpuChecksumError(f"{name} must be on {device}")
    return status, mismatches


def _ptr(t):
    return t.data_ptr() if t is not False else None


def state_verify(method: str, state: torch.Tensor, expected: torch.Tensor, status=None, mismatches=None,
                 stream=None):
    """state_get and the compare in one launch (mchecksum_gpu_state_verify):
    returns (status uint8 per stream: 1 = the stream's CRC so far differs from
    expected[i], mismatch count tensor).  status / mismatches: None allocates,
    False leaves that output out, a tensor is reused (the count is added to).
    The states are left as they are.  It cannot know whether an earlier update
    failed: check the error word first."""
    count = state.numel() if isinstance(state, torch.Tensor) else 0
    _check_state(state, method, count, "state")
    _check_state(expected, method, count, "expected")
    _same_device(state, expected=expected)
    status, mism = _verdict_buffers(count, state.device, status, mismatches)
    with _on(state):
        rc = _lib().mchecksum_gpu_state_verify(method.encode(), state.data_ptr(), count, expected.data_ptr(),
                                               _ptr(status), _ptr(mism), _stream_handle(stream, state.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_state_verify")
    return status, mism


def combine(method: str, crc_a: torch.Tensor, crc_b: torch.Tensor, len_b: torch.Tensor,
            out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """CRC(A_i || B_i) from crc_a[i] = CRC(A_i), crc_b[i] = CRC(B_i) and
    len_b[i] = the bytes of B_i (device int64).  out may be crc_a or crc_b."""
    count = crc_a.numel() if isinstance(crc_a, torch.Tensor) else 0
    _check_state(crc_a, method, count, "crc_a")
    _check_state(crc_b, method, count, "crc_b")
    if (not isinstance(len_b, torch.Tensor) or len_b.dtype != torch.int64 or not len_b.is_cuda
            or not len_b.is_contiguous() or len_b.numel() < count):
        raise GpuChecksumError("len_b must be a contiguous device int64 tensor of at least count elements")
    if out is None:
        out = torch.empty(count, dtype=out_dtype(method), device=crc_a.device)
    _check_state(out, method, count, "out")
    _same_device(crc_a, crc_b=crc_b, len_b=len_b, out=out)
    with _on(crc_a):
        rc = _lib().mchecksum_gpu_combine(method.encode(), crc_a.data_ptr(), crc_b.data_ptr(), len_b.data_ptr(), count,
                                          out.data_ptr(), _stream_handle(stream, crc_a.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_combine")
    return out


def _check_i64_table(t, name: str, count: int | None = None):
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous()
            or (count is not None and t.numel() < count)):
        raise GpuChecksumError(f"{name} must be a contiguous device int64 tensor"
                               + (f" of at least {count} elements" if count is not None else ""))


def combine_runs(method: str, crc: torch.Tensor, lens: torch.Tensor, run_first: torch.Tensor,
                 out: torch.Tensor | None = None, out_len=None, stream=None, run_first_host=None):
    """The CRC of every run of chunks, in one launch (mchecksum_gpu_combine_runs):
    chunk k has the finalized CRC crc[k] and lens[k] bytes (device int64); run
    j is chunks run_first[j] : run_first[j+1] (nruns + 1 non-decreasing device
    int64 indices <= the number of chunks), and out[j] the CRC of those chunks'
    bytes concatenated in order.  A zero-length chunk counts for nothing,
    whatever its CRC word; an empty run gets the CRC of the empty message.

    Returns out -- or (out, out_len) when out_len is given: True for a new
    tensor, or a device int64 tensor of nruns elements, which receives every
    run's byte total.  (out, out_len) are valid (crc, lens) of a further call.
    out and out_len must not overlap crc, lens or run_first.  Pass
    run_first_host (a host copy) to have the table validated before launch;
    otherwise it is trusted, as in the C ABI."""
    nchunks = crc.numel() if isinstance(crc, torch.Tensor) else 0
    _check_state(crc, method, nchunks, "crc")
    _check_i64_table(lens, "lens", nchunks)
    _check_i64_table(run_first, "run_first")
    nruns = run_first.numel() - 1
    if nruns < 0:
        raise GpuChecksumError("run_first needs at least one entry")
    if run_first_host is not None:
        import numpy as np
        fh = np.asarray(run_first_host, dtype=np.uint64)
        if fh.ndim != 1 or len(fh) != run_first.numel():
            raise GpuChecksumError("run_first_host does not match run_first")
        if np.any(fh[1:] < fh[:-1]):
            raise GpuChecksumError("run_first must be non-decreasing")
        if int(fh[-1]) > nchunks:
            raise GpuChecksumError("run_first extends past the last chunk")
    if out is None:
        out = torch.empty(nruns, dtype=out_dtype(method), device=crc.device)
    _check_state(out, method, nruns, "out")
    if out_len is True:
        out_len = torch.empty(nruns, dtype=torch.int64, device=crc.device)
    elif out_len is False:
        out_len = None
    if out_len is not None:
        _check_i64_table(out_len, "out_len", nruns)
    _same_device(crc, lens=lens, run_first=run_first, out=out, out_len=out_len)
    with _on(crc):
        rc = _lib().mchecksum_gpu_combine_runs(method.encode(), crc.data_ptr(), lens.data_ptr(), nchunks,
                                               run_first.data_ptr(), nruns, out.data_ptr(),
                                               out_len.data_ptr() if out_len is not None else None,
                                               _stream_handle(stream, crc.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_combine_runs")
    return out if out_len is None else (out, out_len)


def verify_offsets(method: str, data: torch.Tensor, offsets: torch.Tensor, expected: torch.Tensor,
                   stream=None, offsets_host=None):
    """Returns (status uint8 per payload: 1 = mismatch, mismatch count tensor)."""
    _check_device_u8(data, "data")
    _check_offsets(data, offsets, offsets_host)
    count = offsets.numel() - 1
    if expected.numel() < count or expected.dtype != out_dtype(method) or not expected.is_cuda:
        raise GpuChecksumError("expected has the wrong size, dtype or device")
    _same_device(data, offsets=offsets, expected=expected)
    # status starts "failed": only a hashed payload's verdict overwrites it
    status = torch.ones(count, dtype=torch.uint8, device=data.device)
    mism = torch.zeros(1, dtype=torch.int32, device=data.device)
    with _on(data):
        rc = _lib().mchecksum_gpu_verify_offsets(method.encode(), data.data_ptr(), offsets.data_ptr(), count,
                                                 expected.data_ptr(), status.data_ptr(), mism.data_ptr(),
                                                 _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_offsets")
    return status, mism


def verify_messages(data: torch.Tensor, msg_offsets: torch.Tensor, payload_offset: int = 20, hash_offset: int = 16,
                    method: str = "crc32c", stream=None, offsets_host=None, status=None, mismatches=None):
    """Verify received RPC messages in place: payload after payload_offset,
    expected CRC = network-order u32 at hash_offset (Mercury: 16 B core header,
    4 B HG header).  Returns (status uint8 per message: 1 = fails, count).
    Pass preallocated `status` (uint8, >= count) and `mismatches` (int32, one
    element, zeroed by the caller; the call adds to it) to reuse buffers."""
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    if status is None:
        status = torch.ones(max(count, 0), dtype=torch.uint8, device=data.device)
    elif status.dtype != torch.uint8 or status.numel() < count or not status.is_cuda:
        raise GpuChecksumError("status must be a device uint8 tensor of at least count elements")
    mism = torch.zeros(1, dtype=torch.int32, device=data.device) if mismatches is None else mismatches
    if mism.dtype != torch.int32 or not mism.is_cuda:
        raise GpuChecksumError("mismatches must be a device int32 tensor")
    _same_device(data, msg_offsets=msg_offsets, status=status, mismatches=mism)
    with _on(data):
        rc = _lib().mchecksum_gpu_verify_messages(method.encode(), data.data_ptr(), msg_offsets.data_ptr(), count,
                                                  payload_offset, hash_offset, status.data_ptr(), mism.data_ptr(),
                                                  _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_messages")
    return status, mism


def unpack_messages(data: torch.Tensor, msg_offsets: torch.Tensor, dst: torch.Tensor, dst_offsets: torch.Tensor,
                    payload_offset: int = 20, hash_offset: int = 16, method: str = "crc32c", stream=None,
                    offsets_host=None, dst_offsets_host=None, status=None, mismatches=None):
    """verify_messages that also copies the payloads out, in one pass: payload
    i = data[msg_offsets[i] + payload_offset : msg_offsets[i+1]] goes to
    dst[dst_offsets[i] : dst_offsets[i+1]] and its CRC is compared with the
    network-order u32 at msg_offsets[i] + hash_offset.  Returns (status uint8
    per message, count) with verify_messages' buffer-reuse rules.  Status 1 =
    the CRC differs (the destination then holds the bytes as received) or the
    message does not fit its destination exactly (nothing of it is written).
    Only destination bytes of fitting messages are written.  `data` and `dst`
    must not overlap; with both host tables given, the fit rule and the
    overlap of the two ranges are checked here, otherwise the tables are
    trusted as in the C ABI."""
    _check_device_u8(data, "data")
    _check_device_u8(dst, "dst")
    _check_offsets(data, msg_offsets, offsets_host)
    _check_offsets(dst, dst_offsets, dst_offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0 or dst_offsets.numel() != count + 1:
        raise GpuChecksumError("msg_offsets and dst_offsets need the same number (>= 1) of entries")
    if offsets_host is not None and dst_offsets_host is not None and count:
        import numpy as np
        mo, do = np.asarray(offsets_host, dtype=np.uint64), np.asarray(dst_offsets_host, dtype=np.uint64)
        if np.any(mo[1:] - mo[:-1] != do[1:] - do[:-1] + np.uint64(payload_offset)):
            raise GpuChecksumError("a message does not fit its destination: message size != payload_offset + "
                                   "destination size")
        s0, d0 = data.data_ptr() + int(mo[0]), dst.data_ptr() + int(do[0])
        if s0 < d0 + int(do[-1] - do[0]) and d0 < s0 + int(mo[-1] - mo[0]):
            raise GpuChecksumError("the message and destination ranges overlap")
    if status is None:
        status = torch.ones(max(count, 0), dtype=torch.uint8, device=data.device)
    elif status.dtype != torch.uint8 or status.numel() < count or not status.is_cuda:
        raise GpuChecksumError("status must be a device uint8 tensor of at least count elements")
    mism = torch.zeros(1, dtype=torch.int32, device=data.device) if mismatches is None else mismatches
    if mism.dtype != torch.int32 or not mism.is_cuda:
        raise GpuChecksumError("mismatches must be a device int32 tensor")
    _same_device(data, msg_offsets=msg_offsets, dst=dst, dst_offsets=dst_offsets, status=status, mismatches=mism)
    with _on(data):
        rc = _lib().mchecksum_gpu_unpack_messages(method.encode(), data.data_ptr(), msg_offsets.data_ptr(), count,
                                                  payload_offset, hash_offset, dst.data_ptr(), dst_offsets.data_ptr(),
                                                  status.data_ptr(), mism.data_ptr(),
                                                  _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_unpack_messages")
    return status, mism


def _sender_status(data: torch.Tensor, count: int, status):
    """Status of a sealing call: starts "not sealed", only a sealed message's
    verdict overwrites it."""
    if status is None:
        return torch.ones(max(count, 0), dtype=torch.uint8, device=data.device)
    if (not isinstance(status, torch.Tensor) or status.dtype != torch.uint8 or status.numel() < count
            or not status.is_cuda or not status.is_contiguous()):
        raise GpuChecksumError("status must be a contiguous device uint8 tensor of at least count elements")
    return status


def seal_messages(data: torch.Tensor, msg_offsets: torch.Tensor, payload_offset: int = 20, hash_offset: int = 16,
                  method: str = "crc32c", stream=None, offsets_host=None, status=None) -> torch.Tensor:
    """Sender side of verify_messages, in place: store the CRC of each message's
    payload (from payload_offset on) network-order at hash_offset.  Returns
    status (uint8 per message: 1 = shorter than payload_offset, not written).
    Only the 4 hash bytes of each sealed message are written.  Pass a
    preallocated `status` (uint8, >= count, filled with ones) to reuse it."""
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("msg_offsets needs at least one entry")
    status = _sender_status(data, count, status)
    _same_device(data, msg_offsets=msg_offsets, status=status)
    with _on(data):
        rc = _lib().mchecksum_gpu_seal_messages(method.encode(), data.data_ptr(), msg_offsets.data_ptr(), count,
                                                payload_offset, hash_offset, status.data_ptr(),
                                                _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_messages")
    return status


def pack_messages(src: torch.Tensor, src_offsets: torch.Tensor, data: torch.Tensor, msg_offsets: torch.Tensor,
                  payload_offset: int = 20, hash_offset: int = 16, method: str = "crc32c", stream=None,
                  src_offsets_host=None, offsets_host=None, status=None) -> torch.Tensor:
    """Pack, hash and seal in one pass: payload i = src[src_offsets[i] :
    src_offsets[i+1]] is copied behind the headers of message i of `data`
    (data[msg_offsets[i] + payload_offset : msg_offsets[i+1]]) and its CRC
    stored network-order at msg_offsets[i] + hash_offset.  Returns status
    (uint8 per message: 1 = the payload does not fit its message exactly, not
    written).  Only payload and hash bytes are written; the caller fills the
    other header bytes.  `src` and `data` must not overlap; with both host
    tables given, the fit rule and the overlap of the two ranges are checked
    here, otherwise the tables are trusted as in the C ABI."""
    _check_device_u8(src, "src")
    _check_device_u8(data, "data")
    _check_offsets(src, src_offsets, src_offsets_host)
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0 or src_offsets.numel() != count + 1:
        raise GpuChecksumError("src_offsets and msg_offsets need the same number (>= 1) of entries")
    if src_offsets_host is not None and offsets_host is not None and count:
        import numpy as np
        so, mo = np.asarray(src_offsets_host, dtype=np.uint64), np.asarray(offsets_host, dtype=np.uint64)
        if np.any(mo[1:] - mo[:-1] != so[1:] - so[:-1] + np.uint64(payload_offset)):
            raise GpuChecksumError("a payload does not fit its message: message size != payload_offset + payload size")
        s0, d0 = src.data_ptr() + int(so[0]), data.data_ptr() + int(mo[0])
        if s0 < d0 + int(mo[-1] - mo[0]) and d0 < s0 + int(so[-1] - so[0]):
            raise GpuChecksumError("the source and destination ranges overlap")
    status = _sender_status(data, count, status)
    _same_device(data, src=src, src_offsets=src_offsets, msg_offsets=msg_offsets, status=status)
    with _on(data):
        rc = _lib().mchecksum_gpu_pack_messages(method.encode(), src.data_ptr(), src_offsets.data_ptr(),
                                                data.data_ptr(), msg_offsets.data_ptr(), count, payload_offset,
                                                hash_offset, status.data_ptr(), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_pack_messages")
    return status


def _check_detached(msgs, msg_offsets, offsets_host, hash_offset: int) -> int:
    """The eager messages of a detached call; returns count."""
    _check_device_u8(msgs, "msgs")
    _check_offsets(msgs, msg_offsets, offsets_host)
    if hash_offset < 0 or hash_offset > 1 << 30:
        raise GpuChecksumError("hash_offset must lie in 0..2^30")
    count = msg_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("msg_offsets needs at least one entry")
    return count


def _seal_status(msgs: torch.Tensor, count: int, status):
    """_sender_status, with False for no status array at all."""
    return False if status is False else _sender_status(msgs, count, status)


def verify_detached_messages(msgs: torch.Tensor, msg_offsets: torch.Tensor, payloads: torch.Tensor,
                             payload_offsets: torch.Tensor, hash_offset: int = 16, method: str = "crc32c", stream=None,
                             offsets_host=None, payload_offsets_host=None, status=None, mismatches=None):
    """Verify overflow RPCs (mchecksum_gpu_verify_detached_messages): payload
    i = payloads[payload_offsets[i] : payload_offsets[i+1]] lies outside its
    message, and the expected CRC is the network-order u32 at msg_offsets[i] +
    hash_offset of `msgs`, the eager messages.  Returns (status uint8 per
    message: 1 = the CRC differs or the message is shorter than hash_offset +
    4, mismatch count tensor).  status / mismatches: None allocates, False
    leaves that output out, a tensor is reused (the count is added to).
    Nothing is written to either buffer.  offsets_host / payload_offsets_host
    (host copies) have the tables validated before launch."""
    count = _check_detached(msgs, msg_offsets, offsets_host, hash_offset)
    _check_device_u8(payloads, "payloads")
    _check_offsets(payloads, payload_offsets, payload_offsets_host)
    if payload_offsets.numel() != count + 1:
        raise GpuChecksumError("msg_offsets and payload_offsets need the same number (>= 1) of entries")
    status, mism = _verdict_buffers(count, msgs.device, status, mismatches)
    _same_device(msgs, msg_offsets=msg_offsets, payloads=payloads, payload_offsets=payload_offsets,
                 status=None if status is False else status, mismatches=None if mism is False else mism)
    with _on(msgs):
        rc = _lib().mchecksum_gpu_verify_detached_messages(method.encode(), msgs.data_ptr(), msg_offsets.data_ptr(),
                                                           hash_offset, payloads.data_ptr(), payload_offsets.data_ptr(),
                                                           count, _ptr(status), _ptr(mism),
                                                           _stream_handle(stream, msgs.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_detached_messages")
    return status, mism


def seal_detached_messages(msgs: torch.Tensor, msg_offsets: torch.Tensor, payloads: torch.Tensor,
                           payload_offsets: torch.Tensor, hash_offset: int = 16, method: str = "crc32c", stream=None,
                           offsets_host=None, payload_offsets_host=None, status=None):
    """Sender side of verify_detached_messages: store the CRC of payload i
    network-order in the 4 bytes at msg_offsets[i] + hash_offset of `msgs`.
    Returns status (uint8 per message: 1 = shorter than hash_offset + 4, not
    written; False passes none and returns False).  Only those 4 bytes of each
    sealed message are written; `payloads` is only read."""
    count = _check_detached(msgs, msg_offsets, offsets_host, hash_offset)
    _check_device_u8(payloads, "payloads")
    _check_offsets(payloads, payload_offsets, payload_offsets_host)
    if payload_offsets.numel() != count + 1:
        raise GpuChecksumError("msg_offsets and payload_offsets need the same number (>= 1) of entries")
    status = _seal_status(msgs, count, status)
    _same_device(msgs, msg_offsets=msg_offsets, payloads=payloads, payload_offsets=payload_offsets,
                 status=None if status is False else status)
    with _on(msgs):
        rc = _lib().mchecksum_gpu_seal_detached_messages(method.encode(), msgs.data_ptr(), msg_offsets.data_ptr(),
                                                         hash_offset, payloads.data_ptr(), payload_offsets.data_ptr(),
                                                         count, _ptr(status), _stream_handle(stream, msgs.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_detached_messages")
    return status


def state_verify_messages(state: torch.Tensor, msgs: torch.Tensor, msg_offsets: torch.Tensor, hash_offset: int = 16,
                          method: str = "crc32c", stream=None, offsets_host=None, status=None, mismatches=None):
    """state_verify with the expected values read from the eager messages'
    hash slots (mchecksum_gpu_state_verify_messages): the end of a pull hashed
    in stages (state_init, then update_offsets / update_copy_offsets / segment
    updates).  Returns (status, mismatch count) as verify_detached_messages;
    the states are left as they are.  It cannot know whether an earlier update
    failed: check the error word first."""
    count = _check_detached(msgs, msg_offsets, offsets_host, hash_offset)
    _check_state(state, method, count, "state")
    status, mism = _verdict_buffers(count, msgs.device, status, mismatches)
    _same_device(msgs, msg_offsets=msg_offsets, state=state, status=None if status is False else status,
                 mismatches=None if mism is False else mism)
    with _on(msgs):
        rc = _lib().mchecksum_gpu_state_verify_messages(method.encode(), state.data_ptr(), count, msgs.data_ptr(),
                                                        msg_offsets.data_ptr(), hash_offset, _ptr(status), _ptr(mism),
                                                        _stream_handle(stream, msgs.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_state_verify_messages")
    return status, mism


def state_seal_messages(state: torch.Tensor, msgs: torch.Tensor, msg_offsets: torch.Tensor, hash_offset: int = 16,
                        method: str = "crc32c", stream=None, offsets_host=None, status=None):
    """The sender's mirror of state_verify_messages: store the CRC each state
    has reached network-order in its message's hash slot.  Returns status as
    seal_detached_messages; the states are left as they are."""
    count = _check_detached(msgs, msg_offsets, offsets_host, hash_offset)
    _check_state(state, method, count, "state")
    status = _seal_status(msgs, count, status)
    _same_device(msgs, msg_offsets=msg_offsets, state=state, status=None if status is False else status)
    with _on(msgs):
        rc = _lib().mchecksum_gpu_state_seal_messages(method.encode(), state.data_ptr(), count, msgs.data_ptr(),
                                                      msg_offsets.data_ptr(), hash_offset, _ptr(status),
                                                      _stream_handle(stream, msgs.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_state_seal_messages")
    return status


# statuses of the RPC message calls (include/mchecksum_gpu.h, MCHECKSUM_GPU_RPC_*)
RPC_OK, RPC_PAYLOAD, RPC_HEADER, RPC_SHORT, RPC_DEFERRED, RPC_FAULT, RPC_CLASSES = range(7)


def _check_rpc(data, msg_offsets, offsets_host, kind: str, payload_offset: int, hash_offset: int):
    """The messages of an RPC message call; returns (count, the kind's number)."""
    from ._lib import CORE_HEADER_REQUEST, CORE_HEADER_RESPONSE
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    k = {"request": CORE_HEADER_REQUEST, "response": CORE_HEADER_RESPONSE}.get(kind)
    if k is None:
        raise GpuChecksumError('kind must be "request" or "response"')
    if hash_offset < 16 or hash_offset > 1 << 30 or hash_offset + 4 > payload_offset:
        raise GpuChecksumError("hash_offset must lie in 16..2^30 and hash_offset + 4 must not exceed payload_offset")
    count = msg_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("msg_offsets needs at least one entry")
    return count, k


def _rpc_status(data: torch.Tensor, count: int, status):
    """Status of an RPC message call: None allocates (every message starts as
    FAULT, "not vouched for"), False passes none, a tensor is used as it is."""
    if status is None:
        return torch.full((max(count, 0),), RPC_FAULT, dtype=torch.uint8, device=data.device)
    return False if status is False else _sender_status(data, count, status)


def verify_rpc_messages(data: torch.Tensor, msg_offsets: torch.Tensor, kind: str = "request",
                        payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                        method: str = "crc32c", stream=None, offsets_host=None, status=None, counts=None):
    """Check whole RPC messages as Mercury does, in one launch
    (mchecksum_gpu_verify_rpc_messages): the core header's CRC-16, then its
    flags, then -- unless MORE_DATA says the payload is elsewhere -- the CRC of
    data[msg_offsets[i] + payload_offset : msg_offsets[i+1]] against the
    network-order u32 at hash_offset.  Returns (status uint8 per message: RPC_OK,
    RPC_PAYLOAD, RPC_HEADER, RPC_SHORT, RPC_DEFERRED or RPC_FAULT; counts, int32
    per class).  status / counts: None allocates, False leaves that output out,
    a tensor is reused (counts are added to).  Nothing is written to `data`."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    status = _rpc_status(data, count, status)
    if counts is None:
        counts = torch.zeros(RPC_CLASSES, dtype=torch.int32, device=data.device)
    elif counts is not False and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32
                                  or not counts.is_cuda or not counts.is_contiguous() or counts.numel() < RPC_CLASSES):
        raise GpuChecksumError("counts must be a contiguous device int32 tensor of at least RPC_CLASSES elements")
    _same_device(data, msg_offsets=msg_offsets, status=None if status is False else status,
                 counts=None if counts is False else counts)
    with _on(data):
        rc = _lib().mchecksum_gpu_verify_rpc_messages(header_method.encode(), method.encode(), k, data.data_ptr(),
                                                      msg_offsets.data_ptr(), count, payload_offset, hash_offset,
                                                      _ptr(status), _ptr(counts), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_rpc_messages")
    return status, counts


def seal_rpc_messages(data: torch.Tensor, msg_offsets: torch.Tensor, kind: str = "request",
                      payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                      method: str = "crc32c", stream=None, offsets_host=None, status=None):
    """Sender side of verify_rpc_messages, in place: the payload CRC
    network-order at hash_offset and the core header's CRC-16 at 12 (request) or
    4 (response); with MORE_DATA set, the header's CRC-16 alone (RPC_DEFERRED:
    the HG slot is seal_detached_messages').  Returns status (uint8 per message:
    RPC_OK, RPC_DEFERRED, RPC_SHORT = nothing written, or RPC_FAULT; False
    passes none and returns False).  Only those 2 or 6 bytes are written."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    status = _rpc_status(data, count, status)
    _same_device(data, msg_offsets=msg_offsets, status=None if status is False else status)
    with _on(data):
        rc = _lib().mchecksum_gpu_seal_rpc_messages(header_method.encode(), method.encode(), k, data.data_ptr(),
                                                    msg_offsets.data_ptr(), count, payload_offset, hash_offset,
                                                    _ptr(status), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_rpc_messages")
    return status


# the copying RPC calls' seventh status and their count words (MCHECKSUM_GPU_COPY_RPC_MISFIT, _CLASSES)
RPC_MISFIT, RPC_COPY_CLASSES = 6, 7


def _check_rpc_copy(data, msg_offsets, offsets_host, other, other_offsets, other_host, names):
    """The second buffer and table of a copying RPC call.  With both host
    tables, the two ranges must not overlap; the fit rule is not raised on:
    RPC_MISFIT is a verdict of these calls."""
    _check_device_u8(other, names[0])
    _check_offsets(other, other_offsets, other_host)
    count = msg_offsets.numel() - 1
    if other_offsets.numel() != count + 1:
        raise GpuChecksumError(f"msg_offsets and {names[1]} need the same number (>= 1) of entries")
    if offsets_host is not None and other_host is not None and count:
        import numpy as np
        mo, oo = np.asarray(offsets_host, dtype=np.uint64), np.asarray(other_host, dtype=np.uint64)
        m0, o0 = data.data_ptr() + int(mo[0]), other.data_ptr() + int(oo[0])
        if m0 < o0 + int(oo[-1] - oo[0]) and o0 < m0 + int(mo[-1] - mo[0]):
            raise GpuChecksumError(f"the message and {names[0]} ranges overlap")


def unpack_rpc_messages(data: torch.Tensor, msg_offsets: torch.Tensor, dst: torch.Tensor, dst_offsets: torch.Tensor,
                        kind: str = "request", payload_offset: int = 20, hash_offset: int = 16,
                        header_method: str = "crc16", method: str = "crc32c", stream=None, offsets_host=None,
                        dst_offsets_host=None, status=None, counts=None):
    """verify_rpc_messages that also copies the payloads out, in one launch
    (mchecksum_gpu_unpack_rpc_messages): the payload of an eager, whole message
    whose size is payload_offset + its destination's goes to
    dst[dst_offsets[i] : dst_offsets[i+1]] as received -- whatever the header's
    and the payload's CRC turn out to be; look at the status first.  Returns
    (status uint8 per message: RPC_OK, RPC_PAYLOAD, RPC_HEADER, RPC_SHORT,
    RPC_DEFERRED, RPC_MISFIT or RPC_FAULT; counts, int32 per class,
    RPC_COPY_CLASSES words).  Nothing of a DEFERRED, SHORT or MISFIT message's
    destination is written.  status / counts as for verify_rpc_messages.  `data`
    and `dst` must not overlap; with both host tables given that is checked
    here (the fit is not: a misfit is a verdict)."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    _check_rpc_copy(data, msg_offsets, offsets_host, dst, dst_offsets, dst_offsets_host, ("dst", "dst_offsets"))
    status = _rpc_status(data, count, status)
    if counts is None:
        counts = torch.zeros(RPC_COPY_CLASSES, dtype=torch.int32, device=data.device)
    elif counts is not False and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32
                                  or not counts.is_cuda or not counts.is_contiguous()
                                  or counts.numel() < RPC_COPY_CLASSES):
        raise GpuChecksumError("counts must be a contiguous device int32 tensor of at least RPC_COPY_CLASSES elements")
    _same_device(data, msg_offsets=msg_offsets, dst=dst, dst_offsets=dst_offsets,
                 status=None if status is False else status, counts=None if counts is False else counts)
    with _on(data):
        rc = _lib().mchecksum_gpu_unpack_rpc_messages(header_method.encode(), method.encode(), k, data.data_ptr(),
                                                      msg_offsets.data_ptr(), count, payload_offset, hash_offset,
                                                      dst.data_ptr(), dst_offsets.data_ptr(), _ptr(status),
                                                      _ptr(counts), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_unpack_rpc_messages")
    return status, counts


def pack_rpc_messages(src: torch.Tensor, src_offsets: torch.Tensor, data: torch.Tensor, msg_offsets: torch.Tensor,
                      kind: str = "request", payload_offset: int = 20, hash_offset: int = 16,
                      header_method: str = "crc16", method: str = "crc32c", stream=None, src_offsets_host=None,
                      offsets_host=None, status=None):
    """seal_rpc_messages that also copies the payloads in, in one launch
    (mchecksum_gpu_pack_rpc_messages): the caller has filled every header byte
    of `data` but the two hashes.  An eager, whole message whose size is
    payload_offset + its source's gets src[src_offsets[i] : src_offsets[i+1]]
    behind its headers, the payload CRC at hash_offset and the core header's
    CRC-16 (RPC_OK); one with MORE_DATA set the header's CRC-16 alone
    (RPC_DEFERRED, its source range is not read); RPC_SHORT and RPC_MISFIT
    messages are not written.  Returns status (uint8 per message, or RPC_FAULT;
    False passes none and returns False).  `src` and `data` must not overlap;
    with both host tables given that is checked here (the fit is not)."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    _check_rpc_copy(data, msg_offsets, offsets_host, src, src_offsets, src_offsets_host, ("src", "src_offsets"))
    status = _rpc_status(data, count, status)
    _same_device(data, src=src, src_offsets=src_offsets, msg_offsets=msg_offsets,
                 status=None if status is False else status)
    with _on(data):
        rc = _lib().mchecksum_gpu_pack_rpc_messages(header_method.encode(), method.encode(), k, src.data_ptr(),
                                                    src_offsets.data_ptr(), data.data_ptr(), msg_offsets.data_ptr(),
                                                    count, payload_offset, hash_offset, _ptr(status),
                                                    _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_pack_rpc_messages")
    return status


def rpc_message_list(parts, device=None, with_host: bool = False):
    """The two arrays of the *_rpc_message_list calls from a list of
    (tensor, start, length): message i is the `length` bytes `start` bytes into
    `tensor` (a contiguous device tensor; its data_ptr() is the allocation's
    address), in the order given -- any tensors, any order, gaps as they come.
    Returns (msg_addr, msg_len), device int64 tensors; with_host=True also the
    two host arrays (numpy uint64), for the wrappers' overlap checks.  The
    tensors in `parts` must stay alive while the arrays are in use: the arrays
    hold addresses, not references."""
    import numpy as np
    addr, lens = np.zeros(len(parts), dtype=np.uint64), np.zeros(len(parts), dtype=np.uint64)
    for i, (t, start, length) in enumerate(parts):
        _check_device_u8(t, f"parts[{i}][0]")
        if device is None:
            device = t.device
        if t.device != device:
            raise GpuChecksumError(f"parts[{i}] lies on {t.device}, the list on {device}")
        if start < 0 or length < 0 or start + length > t.numel() * t.element_size():
            raise GpuChecksumError(f"parts[{i}] extends past the end of its tensor")
        addr[i], lens[i] = t.data_ptr() + start, length
    if device is None:
        raise GpuChecksumError("an empty list needs a device")
    dev = (torch.from_numpy(addr.view(np.int64)).to(device), torch.from_numpy(lens.view(np.int64)).to(device))
    return dev + (addr, lens) if with_host else dev


def _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind: str, payload_offset: int, hash_offset: int,
                    written: bool):
    """The message side of an RPC message-list call; returns (count, the kind's
    number).  With both host arrays, messages that are written must not overlap
    one another."""
    from ._lib import CORE_HEADER_REQUEST, CORE_HEADER_RESPONSE
    _check_i64_table(msg_addr, "msg_addr")
    count = msg_addr.numel()
    _check_i64_table(msg_len, "msg_len", count)
    if msg_len.numel() != count:
        raise GpuChecksumError("msg_addr and msg_len need the same number of entries")
    k = {"request": CORE_HEADER_REQUEST, "response": CORE_HEADER_RESPONSE}.get(kind)
    if k is None:
        raise GpuChecksumError('kind must be "request" or "response"')
    if hash_offset < 16 or hash_offset > 1 << 30 or hash_offset + 4 > payload_offset:
        raise GpuChecksumError("hash_offset must lie in 16..2^30 and hash_offset + 4 must not exceed payload_offset")
    if (addr_host is None) != (len_host is None):
        raise GpuChecksumError("addr_host and len_host go together")
    if addr_host is not None:
        import numpy as np
        ah, lh = np.asarray(addr_host, dtype=np.uint64), np.asarray(len_host, dtype=np.uint64)
        if len(ah) != count or len(lh) != count:
            raise GpuChecksumError("addr_host / len_host do not match msg_addr / msg_len")
        if written and count > 1:
            order = np.argsort(ah, kind="stable")
            a, n = ah[order], lh[order]
            if np.any((a[:-1] + n[:-1] > a[1:]) & (n[:-1] > 0) & (n[1:] > 0)):
                raise GpuChecksumError("messages that are written overlap one another")
    return count, k


def _check_rpc_list_copy(addr_host, len_host, count, other, other_offsets, other_host, names):
    """The table side of a copying RPC message-list call (_check_rpc_copy's
    checks): with all host copies, no message may overlap the other range."""
    _check_device_u8(other, names[0])
    _check_offsets(other, other_offsets, other_host)
    if other_offsets.numel() != count + 1:
        raise GpuChecksumError(f"{names[1]} needs one entry more than msg_addr")
    if addr_host is not None and other_host is not None and count:
        import numpy as np
        ah, lh = np.asarray(addr_host, dtype=np.uint64), np.asarray(len_host, dtype=np.uint64)
        oo = np.asarray(other_host, dtype=np.uint64)
        o0, o1 = other.data_ptr() + int(oo[0]), other.data_ptr() + int(oo[-1])
        if o1 > o0 and np.any((lh > 0) & (ah < np.uint64(o1)) & (ah + lh > np.uint64(o0))):
            raise GpuChecksumError(f"a message and the {names[0]} range overlap")


def _rpc_counts(counts, classes: int, device):
    if counts is None:
        return torch.zeros(classes, dtype=torch.int32, device=device)
    if counts is not False and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32
                                or not counts.is_cuda or not counts.is_contiguous() or counts.numel() < classes):
        raise GpuChecksumError(f"counts must be a contiguous device int32 tensor of at least {classes} elements")
    return counts


def verify_rpc_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, kind: str = "request",
                            payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                            method: str = "crc32c", stream=None, addr_host=None, len_host=None, status=None,
                            counts=None):
    """verify_rpc_messages with the messages addressed by a list
    (mchecksum_gpu_verify_rpc_message_list): message i is the msg_len[i] bytes at
    the device address msg_addr[i] (device int64 tensors, rpc_message_list
    builds them) -- in any number of allocations, in any order, with any gaps.
    Rules, statuses and counts are verify_rpc_messages'; returns (status, counts).
    A message shorter than 16 bytes is RPC_SHORT and its address is not used."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, False)
    status = _rpc_status(msg_addr, count, status)
    counts = _rpc_counts(counts, RPC_CLASSES, msg_addr.device)
    _same_device(msg_addr, msg_len=msg_len, status=None if status is False else status,
                 counts=None if counts is False else counts)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_verify_rpc_message_list(header_method.encode(), method.encode(), k,
                                                          msg_addr.data_ptr(), msg_len.data_ptr(), count,
                                                          payload_offset, hash_offset, _ptr(status), _ptr(counts),
                                                          _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_rpc_message_list")
    return status, counts


def seal_rpc_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, kind: str = "request",
                          payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                          method: str = "crc32c", stream=None, addr_host=None, len_host=None, status=None):
    """seal_rpc_messages with the messages addressed by a list
    (mchecksum_gpu_seal_rpc_message_list), written through their addresses: the
    same 2 or 6 bytes of a message, no others.  The messages must not overlap
    one another; with both host arrays given that is checked here.  Returns
    status as seal_rpc_messages does."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, True)
    status = _rpc_status(msg_addr, count, status)
    _same_device(msg_addr, msg_len=msg_len, status=None if status is False else status)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_seal_rpc_message_list(header_method.encode(), method.encode(), k,
                                                        msg_addr.data_ptr(), msg_len.data_ptr(), count,
                                                        payload_offset, hash_offset, _ptr(status),
                                                        _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_rpc_message_list")
    return status


def unpack_rpc_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, dst: torch.Tensor,
                            dst_offsets: torch.Tensor, kind: str = "request", payload_offset: int = 20,
                            hash_offset: int = 16, header_method: str = "crc16", method: str = "crc32c", stream=None,
                            addr_host=None, len_host=None, dst_offsets_host=None, status=None, counts=None):
    """unpack_rpc_messages with the messages addressed by a list
    (mchecksum_gpu_unpack_rpc_message_list); the destination stays
    dst[dst_offsets[i] : dst_offsets[i+1]].  Rules, statuses, counts and what is
    written are unpack_rpc_messages'; returns (status, counts).  No message may
    overlap `dst`; with all three host copies given that is checked here."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, False)
    _check_rpc_list_copy(addr_host, len_host, count, dst, dst_offsets, dst_offsets_host, ("dst", "dst_offsets"))
    status = _rpc_status(msg_addr, count, status)
    counts = _rpc_counts(counts, RPC_COPY_CLASSES, msg_addr.device)
    _same_device(msg_addr, msg_len=msg_len, dst=dst, dst_offsets=dst_offsets,
                 status=None if status is False else status, counts=None if counts is False else counts)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_unpack_rpc_message_list(header_method.encode(), method.encode(), k,
                                                          msg_addr.data_ptr(), msg_len.data_ptr(), count,
                                                          payload_offset, hash_offset, dst.data_ptr(),
                                                          dst_offsets.data_ptr(), _ptr(status), _ptr(counts),
                                                          _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_unpack_rpc_message_list")
    return status, counts


def pack_rpc_message_list(src: torch.Tensor, src_offsets: torch.Tensor, msg_addr: torch.Tensor,
                          msg_len: torch.Tensor, kind: str = "request", payload_offset: int = 20,
                          hash_offset: int = 16, header_method: str = "crc16", method: str = "crc32c", stream=None,
                          src_offsets_host=None, addr_host=None, len_host=None, status=None):
    """pack_rpc_messages with the messages addressed by a list
    (mchecksum_gpu_pack_rpc_message_list): the headers are read and the
    payloads and hashes written through the addresses; the source stays
    src[src_offsets[i] : src_offsets[i+1]].  Rules, statuses and what is written
    are pack_rpc_messages'; returns status.  The messages must not overlap one
    another or `src`; with the host copies given that is checked here."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, True)
    _check_rpc_list_copy(addr_host, len_host, count, src, src_offsets, src_offsets_host, ("src", "src_offsets"))
    status = _rpc_status(msg_addr, count, status)
    _same_device(msg_addr, msg_len=msg_len, src=src, src_offsets=src_offsets,
                 status=None if status is False else status)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_pack_rpc_message_list(header_method.encode(), method.encode(), k, src.data_ptr(),
                                                        src_offsets.data_ptr(), msg_addr.data_ptr(),
                                                        msg_len.data_ptr(), count, payload_offset, hash_offset,
                                                        _ptr(status), _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_pack_rpc_message_list")
    return status


# the (addr, len) pair of either side of the *_detached_message_list calls: rpc_message_list under the name it has there
address_list = rpc_message_list


def _check_addr_list(addr, lens, addr_host, len_host, names, count=None):
    """One address list of a detached list call, and its host copies if given
    (the two go together); returns (count, host addresses, host lengths)."""
    _check_i64_table(addr, names[0], count)
    if count is None:
        count = addr.numel()
    _check_i64_table(lens, names[1], count)
    if addr.numel() != count or lens.numel() != count:
        raise GpuChecksumError(f"{names[0]} and {names[1]} need the same number of entries as the other arrays")
    if (addr_host is None) != (len_host is None):
        raise GpuChecksumError(f"the host copies of {names[0]} and {names[1]} go together")
    if addr_host is None:
        return count, None, None
    import numpy as np
    ah, lh = np.asarray(addr_host, dtype=np.uint64), np.asarray(len_host, dtype=np.uint64)
    if len(ah) != count or len(lh) != count:
        raise GpuChecksumError(f"the host copies do not match {names[0]} / {names[1]}")
    return count, ah, lh


def _check_msg_list(msg_addr, msg_len, addr_host, len_host, hash_offset: int, written: bool, count=None) -> int:
    """The eager messages of a detached list call; returns count.  With both
    host arrays, the slots that a seal writes must not overlap one another."""
    if hash_offset < 0 or hash_offset > 1 << 30:
        raise GpuChecksumError("hash_offset must lie in 0..2^30")
    count, ah, lh = _check_addr_list(msg_addr, msg_len, addr_host, len_host, ("msg_addr", "msg_len"), count)
    if written and ah is not None and count > 1:
        import numpy as np
        with np.errstate(over="ignore"):
            slots = np.sort(ah[(ah + lh >= ah) & (lh >= np.uint64(hash_offset + 4))])  # (each + hash_offset: the same order)
        if np.any(slots[1:] - slots[:-1] < np.uint64(4)):
            raise GpuChecksumError("hash slots that are written overlap one another")
    return count


def verify_detached_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, payload_addr: torch.Tensor,
                                 payload_len: torch.Tensor, hash_offset: int = 16, method: str = "crc32c", stream=None,
                                 addr_host=None, len_host=None, payload_addr_host=None, payload_len_host=None,
                                 status=None, mismatches=None):
    """verify_detached_messages with both sides addressed by lists
    (mchecksum_gpu_verify_detached_message_list): eager message i is the
    msg_len[i] bytes at the device address msg_addr[i], payload i the
    payload_len[i] bytes at payload_addr[i] -- four device int64 tensors of
    `count` entries (rpc_message_list builds either pair), every payload and
    every message wherever it lies.  Verdicts are verify_detached_messages';
    returns (status, mismatch count).  A message without its slot and an empty
    payload are never dereferenced (their addresses may be 0); a payload whose
    end wraps the address space fails its entry."""
    count = _check_msg_list(msg_addr, msg_len, addr_host, len_host, hash_offset, False)
    _check_addr_list(payload_addr, payload_len, payload_addr_host, payload_len_host, ("payload_addr", "payload_len"), count)
    status, mism = _verdict_buffers(count, msg_addr.device, status, mismatches)
    _same_device(msg_addr, msg_len=msg_len, payload_addr=payload_addr, payload_len=payload_len,
                 status=None if status is False else status, mismatches=None if mism is False else mism)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_verify_detached_message_list(method.encode(), msg_addr.data_ptr(), msg_len.data_ptr(),
                                                               hash_offset, payload_addr.data_ptr(),
                                                               payload_len.data_ptr(), count, _ptr(status), _ptr(mism),
                                                               _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_detached_message_list")
    return status, mism


def seal_detached_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, payload_addr: torch.Tensor,
                               payload_len: torch.Tensor, hash_offset: int = 16, method: str = "crc32c", stream=None,
                               addr_host=None, len_host=None, payload_addr_host=None, payload_len_host=None,
                               status=None):
    """Sender side of verify_detached_message_list
    (mchecksum_gpu_seal_detached_message_list): the CRC of payload i is stored
    network-order in the 4 bytes at msg_addr[i] + hash_offset, through the
    address; no other byte is written.  The slots must not overlap one another;
    with both host arrays of the messages given that is checked here.  Returns
    status as seal_detached_messages does."""
    count = _check_msg_list(msg_addr, msg_len, addr_host, len_host, hash_offset, True)
    _check_addr_list(payload_addr, payload_len, payload_addr_host, payload_len_host, ("payload_addr", "payload_len"), count)
    status = _seal_status(msg_addr, count, status)
    _same_device(msg_addr, msg_len=msg_len, payload_addr=payload_addr, payload_len=payload_len,
                 status=None if status is False else status)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_seal_detached_message_list(method.encode(), msg_addr.data_ptr(), msg_len.data_ptr(),
                                                             hash_offset, payload_addr.data_ptr(), payload_len.data_ptr(),
                                                             count, _ptr(status), _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_detached_message_list")
    return status


def state_verify_message_list(state: torch.Tensor, msg_addr: torch.Tensor, msg_len: torch.Tensor, hash_offset: int = 16,
                              method: str = "crc32c", stream=None, addr_host=None, len_host=None, status=None,
                              mismatches=None):
    """state_verify_messages with the eager messages addressed by a list
    (mchecksum_gpu_state_verify_message_list): the end of a pull hashed in
    stages whose update_segments calls took the payloads by address.  Returns
    (status, mismatch count) as verify_detached_message_list."""
    count = _check_msg_list(msg_addr, msg_len, addr_host, len_host, hash_offset, False)
    _check_state(state, method, count, "state")
    status, mism = _verdict_buffers(count, msg_addr.device, status, mismatches)
    _same_device(msg_addr, msg_len=msg_len, state=state, status=None if status is False else status,
                 mismatches=None if mism is False else mism)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_state_verify_message_list(method.encode(), state.data_ptr(), count,
                                                            msg_addr.data_ptr(), msg_len.data_ptr(), hash_offset,
                                                            _ptr(status), _ptr(mism),
                                                            _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_state_verify_message_list")
    return status, mism


def state_seal_message_list(state: torch.Tensor, msg_addr: torch.Tensor, msg_len: torch.Tensor, hash_offset: int = 16,
                            method: str = "crc32c", stream=None, addr_host=None, len_host=None, status=None):
    """The sender's mirror of state_verify_message_list
    (mchecksum_gpu_state_seal_message_list): the CRC each state has reached,
    stored network-order in its message's slot through the address.  Returns
    status as seal_detached_message_list."""
    count = _check_msg_list(msg_addr, msg_len, addr_host, len_host, hash_offset, True)
    _check_state(state, method, count, "state")
    status = _seal_status(msg_addr, count, status)
    _same_device(msg_addr, msg_len=msg_len, state=state, status=None if status is False else status)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_state_seal_message_list(method.encode(), state.data_ptr(), count, msg_addr.data_ptr(),
                                                          msg_len.data_ptr(), hash_offset, _ptr(status),
                                                          _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_state_seal_message_list")
    return status


def _torch_owned(stream, handle: int, device) -> bool:
    """Whether `handle` (the hipStream_t a call ran on, given `stream` as passed)
    is a stream torch created and never destroys: a torch.cuda.Stream from its
    pool (not an ExternalStream wrapping a caller's handle) or the device's
    default stream.  With stream=None the current stream may wrap an external
    handle, which torch cannot tell apart here, so only the default stream
    counts."""
    if stream is None:
        return handle == torch.cuda.default_stream(device).cuda_stream
    return type(stream) is torch.cuda.Stream


class SegmentBatch:
    """A scatter-gather batch prepared once: object j = the concatenation of
    segments[obj_first[j]:obj_first[j+1]] (default: one object), each segment a
    contiguous 1-D uint8 device tensor (views of larger buffers are fine) --
    the bulk-handle shape, HG_Bulk_create's (buf_ptrs, buf_sizes) in device
    memory.  The segment table and the scan workspace stay on the device, so
    `checksum` is one C-ABI call (no host work per launch).  Keep the segment
    tensors alive while the batch is in use.  Calls share the one workspace,
    so a call on another stream than the previous call's first waits for it
    (the C ABI requires a workspace per concurrent call)."""

    def __init__(self, segments, obj_first=None, device=None):
        import numpy as np
        addr, lens, dev = [], [], device
        for t in segments:
            _check_device_u8(t, "segment")
            if t.dim() != 1:
                raise GpuChecksumError("segments must be 1-D byte tensors")
            dev = t.device if dev is None else dev
            if t.device != dev:
                raise GpuChecksumError("segments must share one device")
            addr.append(t.data_ptr())
            lens.append(t.numel())
        self.nseg = len(addr)
        first = np.asarray([0, self.nseg] if obj_first is None else obj_first, dtype=np.int64)
        if first.ndim != 1 or len(first) < 1 or np.any(first[1:] < first[:-1]) or first[0] < 0 \
                or first[-1] > self.nseg:
            raise GpuChecksumError("obj_first must be non-decreasing indices into segments")
        self.nobj = len(first) - 1
        self.device = dev if dev is not None else torch.device("cuda", torch.cuda.current_device())
        self.bytes = int(np.sum(np.asarray(lens, dtype=np.int64)[first[0]:first[-1]])) if self.nseg else 0
        self._cap = np.asarray(lens, dtype=np.int64)  # each segment's size as given: set_lengths stays within it
        self._addr = np.asarray(addr, dtype=np.uint64)  # host copies of the tables, for gather's / scatter's checks:
        self._lens = self._cap.copy()                    # the current lengths (set_lengths keeps them) ...
        self._first = first.copy()                       # ... and the objects' first segments
        self._span = (int(first[0]), int(first[-1]))
        self.meta = torch.from_numpy(np.concatenate([np.asarray(addr, dtype=np.uint64).view(np.int64),
                                                     np.asarray(lens, dtype=np.int64), first])).to(self.device)
        # (the message calls' size: the segment calls' plus two words' worth per object)
        need = _lib().mchecksum_gpu_segment_messages_work_size(self.nseg, self.nobj)
        self.work = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)
        self._starts = None  # the starts table of the last gather / scatter: alive for a captured call's replays
        self._last = None  # (stream handle, its torch stream, event after the call or None) of the last call

    def set_lengths(self, lens, stream=None) -> None:
        """Overwrite the device length table in place: segment s now covers the
        first lens[s] bytes of the tensor it was built from.  For a captured
        `checksum` (every replay scans the table again) and for tests: the
        copy is enqueued on `stream` (default: the current one) and nothing
        else happens per call -- order it before the replay that should see
        it and after the one before.  Not while that stream is capturing."""
        import numpy as np
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        if lens.ndim != 1 or len(lens) != self.nseg:
            raise GpuChecksumError(f"set_lengths needs {self.nseg} lengths")
        if np.any(lens < 0) or np.any(lens > self._cap):
            raise GpuChecksumError("a length is negative or larger than its segment")
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            stream = torch.cuda.ExternalStream(int(stream), device=self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):  # (None: the current stream stays)
            if torch.cuda.is_current_stream_capturing():
                raise GpuChecksumError("set_lengths during graph capture: the copy would bake these lengths in")
            self.meta[self.nseg:2 * self.nseg].copy_(torch.from_numpy(lens))
        self._lens = lens.copy()
        self.bytes = int(np.sum(lens[self._span[0]:self._span[1]])) if self.nseg else 0

    def _out(self, method: str, out):
        if out is None:
            out = torch.empty(self.nobj, dtype=out_dtype(method), device=self.device)
        elif out.numel() < self.nobj or out.dtype != out_dtype(method) or not out.is_cuda or not out.is_contiguous():
            raise GpuChecksumError("out tensor has the wrong size, dtype or device, or is not contiguous")
        if out.device != self.device:
            raise GpuChecksumError(f"out must be on {self.device}")
        return out

    def _run(self, name: str, stream, call) -> None:
        """One C-ABI call on the batch's workspace: call(stream handle) -> rc,
        ordered after the previous call's use of the workspace."""
        with torch.cuda.device(self.device):
            h = _stream_handle(stream, self.device)
            # (graph capture: replays are ordered by the graph's user; no events)
            track = not torch.cuda.is_current_stream_capturing()
            s = (torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream(self.device)) if track else None
            if track and self._last is not None and self._last[0] != h:
                # the workspace is still the previous call's: this stream waits
                # for it.  On a stream torch owns (its pool's or the default
                # stream: never destroyed) the event is recorded now, at the
                # switch, after everything queued so far -- not after every
                # call (a marker packet between the kernels costs ~3 us); any
                # other stream (a raw handle, a torch.cuda.ExternalStream, or
                # a current stream that may be one) may be destroyed by then,
                # so its event was recorded right after the call.
                ev = self._last[2]
                if ev is None:
                    ev = torch.cuda.Event()
                    ev.record(self._last[1])
                s.wait_event(ev)
            rc = call(h)
            if rc == 0 and track:
                ev = None
                if not _torch_owned(stream, h, self.device):
                    ev = torch.cuda.Event()
                    ev.record(s)
                self._last = (h, s, ev)
        if rc != 0:
            _err(rc, name)

    def checksum(self, method: str, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        out = self._out(method, out)
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_checksum_segments", stream,
                  lambda h: _lib().mchecksum_gpu_checksum_segments(method.encode(), base, base + 8 * n, n,
                                                                   base + 16 * n, self.nobj, self.work.data_ptr(),
                                                                   self.work.numel() * 8, out.data_ptr(), h))
        return out

    def _flat(self, flat, starts, starts_host, what: str):
        """Checks of gather's dst / scatter's src and its starts table; returns
        the device starts tensor.  The host check of the tables comes first
        (ValueError, no device needed): of a host sequence, or of starts_host
        beside a device tensor, which is otherwise trusted as in the C ABI."""
        import numpy as np
        if not isinstance(flat, torch.Tensor):
            raise GpuChecksumError(f"{what} must be a tensor")
        sh = starts_host if isinstance(starts, torch.Tensor) else np.asarray(starts)
        if sh is not None:
            _check_segment_tables(flat.numel() * flat.element_size(), flat.data_ptr(), sh, self._addr, self._lens,
                                  self._first)
        _check_device_u8(flat, what)
        if flat.device != self.device:
            raise GpuChecksumError(f"{what} must be on {self.device}")
        if isinstance(starts, torch.Tensor):
            if (starts.dtype != torch.int64 or starts.device != self.device or not starts.is_contiguous()
                    or starts.numel() != self.nobj):
                raise GpuChecksumError(f"{what}_starts must be a contiguous int64 tensor of nobj elements on "
                                       f"{self.device}")
            return starts
        return torch.from_numpy(np.ascontiguousarray(sh, dtype=np.uint64).view(np.int64)).to(self.device)

    def gather(self, method: str, dst: torch.Tensor, dst_starts, out: torch.Tensor | None = None,
               stream=None, dst_starts_host=None) -> torch.Tensor:
        """checksum that also linearises, in one pass: object j's segments, in
        order, go to dst[dst_starts[j] : dst_starts[j] + N_j] (N_j = the sum
        of its current segment lengths) and its CRC to out[j].  dst_starts:
        nobj byte offsets in any order -- a host sequence, uploaded here, or a
        device int64 tensor (for a call captured into a graph, and to reuse
        one table).  Only those bytes of dst are written.  A host sequence, or
        dst_starts_host beside a device tensor, is checked before any launch
        (ValueError): every range inside dst, the ranges disjoint from one
        another and from every segment; a device tensor alone is trusted, as
        in the C ABI."""
        st = self._flat(dst, dst_starts, dst_starts_host, "dst")
        out = self._out(method, out)
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_gather_segments", stream,
                  lambda h: _lib().mchecksum_gpu_gather_segments(method.encode(), base, base + 8 * n, n, base + 16 * n,
                                                                 self.nobj, dst.data_ptr(), st.data_ptr(),
                                                                 self.work.data_ptr(), self.work.numel() * 8,
                                                                 out.data_ptr(), h))
        self._starts = st  # (kept alive for a captured call's replays)
        return out

    def scatter(self, method: str, src: torch.Tensor, src_starts, out: torch.Tensor | None = None,
                stream=None, src_starts_host=None) -> torch.Tensor:
        """The reverse of gather: object j = src[src_starts[j] : src_starts[j]
        + N_j] is spread over its segments in order -- the segment tensors are
        written, exactly their current lengths -- and its CRC goes to out[j].
        gather's rules for src_starts and its host checks."""
        st = self._flat(src, src_starts, src_starts_host, "src")
        out = self._out(method, out)
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_scatter_segments", stream,
                  lambda h: _lib().mchecksum_gpu_scatter_segments(method.encode(), src.data_ptr(), st.data_ptr(), base,
                                                                  base + 8 * n, n, base + 16 * n, self.nobj,
                                                                  self.work.data_ptr(), self.work.numel() * 8,
                                                                  out.data_ptr(), h))
        self._starts = st
        return out

    def _state(self, method: str, state):
        _check_state(state, method, self.nobj, "state")
        if state.device != self.device:
            raise GpuChecksumError(f"state must be on {self.device}")
        return state

    def update(self, method: str, state: torch.Tensor, stream=None) -> torch.Tensor:
        """checksum as one stage of a stream: state[j] (state_init's element,
        the one update_offsets advances) is advanced in place over object j's
        segments in order, their current lengths; an object with no bytes
        keeps its state.  Read the values with state_get or compare them with
        state_verify.  Returns state."""
        state = self._state(method, state)
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_update_segments", stream,
                  lambda h: _lib().mchecksum_gpu_update_segments(method.encode(), base, base + 8 * n, n, base + 16 * n,
                                                                 self.nobj, self.work.data_ptr(),
                                                                 self.work.numel() * 8, state.data_ptr(), h))
        return state

    def update_gather(self, method: str, dst: torch.Tensor, dst_starts, state: torch.Tensor, stream=None,
                      dst_starts_host=None) -> torch.Tensor:
        """gather as one stage of a stream: the bytes go where gather puts
        them (its rules and host checks) and state[j] is advanced over them.
        Returns state."""
        st = self._flat(dst, dst_starts, dst_starts_host, "dst")
        state = self._state(method, state)
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_update_gather_segments", stream,
                  lambda h: _lib().mchecksum_gpu_update_gather_segments(method.encode(), base, base + 8 * n, n,
                                                                        base + 16 * n, self.nobj, dst.data_ptr(),
                                                                        st.data_ptr(), self.work.data_ptr(),
                                                                        self.work.numel() * 8, state.data_ptr(), h))
        self._starts = st
        return state

    def update_scatter(self, method: str, src: torch.Tensor, src_starts, state: torch.Tensor, stream=None,
                       src_starts_host=None) -> torch.Tensor:
        """scatter as one stage of a stream (scatter's rules and host checks):
        the segment tensors are written and state[j] is advanced over object
        j's bytes.  Returns state."""
        st = self._flat(src, src_starts, src_starts_host, "src")
        state = self._state(method, state)
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_update_scatter_segments", stream,
                  lambda h: _lib().mchecksum_gpu_update_scatter_segments(method.encode(), src.data_ptr(), st.data_ptr(),
                                                                         base, base + 8 * n, n, base + 16 * n,
                                                                         self.nobj, self.work.data_ptr(),
                                                                         self.work.numel() * 8, state.data_ptr(), h))
        self._starts = st
        return state

    def verify(self, method: str, expected: torch.Tensor, status=None, mismatches=None, stream=None):
        """checksum with the compare on the device: returns (status uint8 per
        object: 1 = its CRC differs from expected[j], mismatch count tensor).
        status / mismatches: None allocates, False leaves that output out, a
        tensor is reused (the count is added to).  Fails closed: a call that
        could not hash every byte flags every object and adds nobj."""
        _check_state(expected, method, self.nobj, "expected")
        if expected.device != self.device:
            raise GpuChecksumError(f"expected must be on {self.device}")
        status, mism = _verdict_buffers(self.nobj, self.device, status, mismatches)
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_verify_segments", stream,
                  lambda h: _lib().mchecksum_gpu_verify_segments(method.encode(), base, base + 8 * n, n, base + 16 * n,
                                                                 self.nobj, self.work.data_ptr(),
                                                                 self.work.numel() * 8, expected.data_ptr(),
                                                                 _ptr(status), _ptr(mism), h))
        return status, mism

    def _messages(self, data, msg_offsets, msg_offsets_host, payload_offset: int):
        """Checks of a message call's buffer and message table; returns the
        device table (int64, nobj + 1 entries).  A host sequence, or
        msg_offsets_host beside a device tensor, is checked first (ValueError,
        no device needed): non-decreasing, inside `data`, and -- for the
        messages that fit, the only ones touched -- _check_segment_tables'
        rules on the payload ranges; a device tensor alone is trusted, as in
        the C ABI."""
        import numpy as np
        if not isinstance(data, torch.Tensor):
            raise GpuChecksumError("data must be a tensor")
        mh = msg_offsets_host if isinstance(msg_offsets, torch.Tensor) else msg_offsets
        if mh is not None:
            mh = np.asarray(mh)
            if mh.ndim != 1 or len(mh) != self.nobj + 1:
                raise ValueError(f"the message table needs {self.nobj + 1} entries, one more than objects")
            mh = mh.astype(np.uint64).astype(np.int64)
            if np.any(mh < 0) or np.any(mh[1:] < mh[:-1]):
                raise ValueError("message offsets must be non-negative and non-decreasing")
            if int(mh[-1]) > data.numel() * data.element_size():
                raise ValueError("message offsets extend past the end of data")
            first = np.asarray(self._first, dtype=np.int64)
            P = np.concatenate([[0], np.cumsum(self._lens)]).astype(np.int64)
            fits = mh[1:] - mh[:-1] == payload_offset + P[first[1:]] - P[first[:-1]]
            lens = np.asarray(self._lens, dtype=np.int64).copy()
            for j in np.nonzero(~fits)[0]:  # a message that does not fit is no range
                lens[first[j]:first[j + 1]] = 0
            _check_segment_tables(data.numel() * data.element_size(), data.data_ptr(), mh[:-1] + payload_offset,
                                  self._addr, lens, first)
        _check_device_u8(data, "data")
        if data.device != self.device:
            raise GpuChecksumError(f"data must be on {self.device}")
        if isinstance(msg_offsets, torch.Tensor):
            if (msg_offsets.dtype != torch.int64 or msg_offsets.device != self.device
                    or not msg_offsets.is_contiguous() or msg_offsets.numel() != self.nobj + 1):
                raise GpuChecksumError(f"msg_offsets must be a contiguous int64 tensor of nobj + 1 elements on "
                                       f"{self.device}")
            return msg_offsets
        return torch.from_numpy(np.ascontiguousarray(mh, dtype=np.int64)).to(self.device)

    def _msg_work(self):
        """The message calls' workspace: the scan's plus two words' worth per
        object (mchecksum_gpu_segment_messages_work_size)."""
        need = _lib().mchecksum_gpu_segment_messages_work_size(self.nseg, self.nobj)
        if self.work.numel() * 8 < need:
            raise GpuChecksumError("the batch's workspace is too small for a message call")
        return self.work

    def pack_messages(self, data: torch.Tensor, msg_offsets, payload_offset: int = 20, hash_offset: int = 16,
                      status=None, stream=None, msg_offsets_host=None) -> torch.Tensor:
        """pack_messages field by field, in one pass: object j's segments, in
        order and at their current lengths, are copied behind the headers of
        message j (data[msg_offsets[j] + payload_offset : msg_offsets[j+1]])
        and their CRC-32C is stored network-order at msg_offsets[j] +
        hash_offset -- HG_PROC_TYPE per field, then hg_set_struct.  Returns
        status (uint8 per message: 1 = the message is not exactly
        payload_offset + N_j bytes long; nothing of it is written).  Only
        payload and hash bytes of fitting messages are written; the caller
        fills the other header bytes.  msg_offsets: nobj + 1 byte offsets, a
        host sequence (uploaded here) or a device int64 tensor (for a captured
        call, and to reuse one table); host tables are checked before any
        launch (_messages).  status: None allocates, False leaves it out, a
        tensor is reused."""
        mo = self._messages(data, msg_offsets, msg_offsets_host, payload_offset)
        if status is not False:
            status = _sender_status(data, self.nobj, status)
            if status.device != self.device:
                raise GpuChecksumError(f"status must be on {self.device}")
        work = self._msg_work()
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_pack_segment_messages", stream,
                  lambda h: _lib().mchecksum_gpu_pack_segment_messages(b"crc32c", base, base + 8 * n, n, base + 16 * n,
                                                                       self.nobj, data.data_ptr(), mo.data_ptr(),
                                                                       payload_offset, hash_offset, work.data_ptr(),
                                                                       work.numel() * 8, _ptr(status), h))
        self._starts = mo  # (kept alive for a captured call's replays)
        return status

    def unpack_messages(self, data: torch.Tensor, msg_offsets, payload_offset: int = 20, hash_offset: int = 16,
                        status=None, mismatches=None, stream=None, msg_offsets_host=None):
        """The receiver's mirror of pack_messages: message j's payload is
        spread over object j's segments in order -- the segment tensors are
        written, exactly their current lengths -- and its CRC-32C is compared
        with the network-order u32 at msg_offsets[j] + hash_offset
        (HG_PROC_TYPE per field on HG_DECODE, then hg_get_struct).  Returns
        (status, mismatches) like verify_messages: status 1 = the CRC differs
        (the segments then hold the bytes as received: look at the status
        before the bytes) or the message does not fit (none of its segments'
        bytes is written).  `data` is never written.  status / mismatches:
        None allocates, False leaves that output out, a tensor is reused (the
        count is added to).  Fails closed as verify: a call that could not
        scan its tables writes nothing, flags every message and adds nobj."""
        mo = self._messages(data, msg_offsets, msg_offsets_host, payload_offset)
        status, mism = _verdict_buffers(self.nobj, self.device, status, mismatches)
        work = self._msg_work()
        base, n = self.meta.data_ptr(), self.nseg
        self._run("mchecksum_gpu_unpack_segment_messages", stream,
                  lambda h: _lib().mchecksum_gpu_unpack_segment_messages(b"crc32c", data.data_ptr(), mo.data_ptr(),
                                                                         self.nobj, payload_offset, hash_offset, base,
                                                                         base + 8 * n, n, base + 16 * n,
                                                                         work.data_ptr(), work.numel() * 8,
                                                                         _ptr(status), _ptr(mism), h))
        self._starts = mo
        return status, mism


def _check_segment_tables(flat_bytes: int, flat_addr: int, starts, seg_addr, seg_lens, first) -> None:
    """Host check of a gather / scatter call (ValueError), callable without a
    device: `starts` has one entry per object; object j's range [starts[j],
    starts[j] + N_j) -- N_j the sum of seg_lens over [first[j], first[j+1]) --
    lies inside the contiguous tensor of flat_bytes bytes at address
    flat_addr; the ranges of two objects do not overlap; and no range overlaps
    a segment of [first[0], first[-1]), compared by address, so a contiguous
    tensor that shares the segments' storage is covered.  Empty objects and
    empty segments are no ranges."""
    import numpy as np
    first = np.asarray(first, dtype=np.int64)
    lens = np.asarray(seg_lens, dtype=np.int64)
    addr = np.asarray(seg_addr, dtype=np.uint64).astype(np.int64)
    starts = np.asarray(starts)
    nobj = len(first) - 1
    if starts.ndim != 1 or len(starts) != nobj:
        raise ValueError(f"the starts table needs {nobj} entries, one per object")
    starts = starts.astype(np.uint64).astype(np.int64) if nobj else np.zeros(0, dtype=np.int64)
    if np.any(starts < 0):
        raise ValueError("a start is negative")
    P = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = P[first[1:]] - P[first[:-1]]
    live = n > 0
    if np.any((starts + n)[live] > flat_bytes):
        raise ValueError("an object's range extends past the end of the contiguous tensor")
    lo, hi = starts[live], (starts + n)[live]
    order = np.argsort(lo, kind="stable")
    lo, hi = lo[order], hi[order]
    if np.any(hi[:-1] > lo[1:]):
        raise ValueError("two objects' ranges overlap")
    if lo.size:
        sl = slice(int(first[0]), int(first[-1]))
        s0, s1 = addr[sl][lens[sl] > 0], (addr[sl] + lens[sl])[lens[sl] > 0]
        a, b = lo + flat_addr, hi + flat_addr  # sorted, disjoint: a segment overlaps one iff it does its neighbours
        i = np.searchsorted(b, s0, side="right")  # first range that ends after the segment's start
        if np.any((i < a.size) & (a[np.minimum(i, a.size - 1)] < s1)):
            raise ValueError("an object's range overlaps a segment")


def _after_one_shot(b, stream):
    # the batch's device table and workspace are freed on return: the caching
    # allocator orders their reuse after this launch on the current stream;
    # another stream must be recorded
    if stream is not None:
        if isinstance(stream, torch.cuda.Stream):
            b.meta.record_stream(stream)
            b.work.record_stream(stream)
            if b._starts is not None:
                b._starts.record_stream(stream)
        else:
            torch.cuda.synchronize(b.device)


def gather_segments(method: str, segments, dst: torch.Tensor, dst_starts, obj_first=None,
                    out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """One-shot SegmentBatch(segments, obj_first).gather(method, dst, dst_starts)."""
    b = SegmentBatch(segments, obj_first)
    out = b.gather(method, dst, dst_starts, out, stream)
    _after_one_shot(b, stream)
    return out


def scatter_segments(method: str, src: torch.Tensor, src_starts, segments, obj_first=None,
                     out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """One-shot SegmentBatch(segments, obj_first).scatter(method, src, src_starts)."""
    b = SegmentBatch(segments, obj_first)
    out = b.scatter(method, src, src_starts, out, stream)
    _after_one_shot(b, stream)
    return out


def pack_segment_messages(segments, obj_first, data: torch.Tensor, msg_offsets, payload_offset: int = 20,
                          hash_offset: int = 16, status=None, stream=None) -> torch.Tensor:
    """One-shot SegmentBatch(segments, obj_first).pack_messages(data, msg_offsets, ...)."""
    b = SegmentBatch(segments, obj_first)
    status = b.pack_messages(data, msg_offsets, payload_offset, hash_offset, status, stream)
    _after_one_shot(b, stream)
    return status


def unpack_segment_messages(data: torch.Tensor, msg_offsets, segments, obj_first, payload_offset: int = 20,
                            hash_offset: int = 16, status=None, mismatches=None, stream=None):
    """One-shot SegmentBatch(segments, obj_first).unpack_messages(data, msg_offsets, ...)."""
    b = SegmentBatch(segments, obj_first)
    verdict = b.unpack_messages(data, msg_offsets, payload_offset, hash_offset, status, mismatches, stream)
    _after_one_shot(b, stream)
    return verdict


def checksum_segments(method: str, segments, obj_first=None, out: torch.Tensor | None = None,
                      stream=None) -> torch.Tensor:
    """One-shot SegmentBatch(segments, obj_first).checksum(method)."""
    b = SegmentBatch(segments, obj_first)
    out = b.checksum(method, out, stream)
    _after_one_shot(b, stream)
    return out


def verify_core_headers(data: torch.Tensor, msg_offsets: torch.Tensor, kind: str = "request",
                        method: str = "crc16", stream=None, offsets_host=None):
    """Check the CRC16 of each message's 16-byte Mercury core header
    (kind "request" or "response").  Returns (status uint8 per message, count)."""
    from ._lib import CORE_HEADER_REQUEST, CORE_HEADER_RESPONSE
    k = {"request": CORE_HEADER_REQUEST, "response": CORE_HEADER_RESPONSE}.get(kind)
    if k is None:
        raise GpuChecksumError("kind must be 'request' or 'response'")
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    _same_device(data, msg_offsets=msg_offsets)
    status = torch.ones(max(count, 0), dtype=torch.uint8, device=data.device)
    mism = torch.zeros(1, dtype=torch.int32, device=data.device)
    with _on(data):
        rc = _lib().mchecksum_gpu_verify_core_headers(method.encode(), k, data.data_ptr(), msg_offsets.data_ptr(),
                                                      count, status.data_ptr(), mism.data_ptr(),
                                                      _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_core_headers")
    return status, mism


def seal_core_headers(data: torch.Tensor, msg_offsets: torch.Tensor, kind: str = "request",
                      method: str = "crc16", stream=None, offsets_host=None, status=None) -> torch.Tensor:
    """Sender side of verify_core_headers: store the CRC16 of each message's
    16-byte Mercury core header (kind "request" or "response") big-endian in
    its hash field.  Returns status (uint8 per message: 1 = shorter than a
    header, not written)."""
    from ._lib import CORE_HEADER_REQUEST, CORE_HEADER_RESPONSE
    k = {"request": CORE_HEADER_REQUEST, "response": CORE_HEADER_RESPONSE}.get(kind)
    if k is None:
        raise GpuChecksumError("kind must be 'request' or 'response'")
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("msg_offsets needs at least one entry")
    status = _sender_status(data, count, status)
    _same_device(data, msg_offsets=msg_offsets, status=status)
    with _on(data):
        rc = _lib().mchecksum_gpu_seal_core_headers(method.encode(), k, data.data_ptr(), msg_offsets.data_ptr(),
                                                    count, status.data_ptr(), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_core_headers")
    return status


XDR_INT, XDR_OPAQUE, XDR_OPAQUE_LEN, XDR_RAW, XDR_RAW_LEN, XDR_SKIP_IF_ZERO = 0, 1, 2, 3, 4, 5
XDR_SINT = 6  # XDR_INT for a signed type: pack_xdr_messages sign-extends it, every other call treats it as XDR_INT


def checksum_xdr(method: str, data: torch.Tensor, msg_offsets: torch.Tensor, schema, status: bool = False,
                 stream=None, offsets_host=None, out: torch.Tensor | None = None):
    """Proc checksum of messages serialized in XDR mode (include/mchecksum_gpu.h,
    mchecksum_gpu_checksum_xdr): schema = [(kind, size), ...] with the XDR_*
    kinds.  Returns the CRC tensor, or (CRCs, status) with status=True
    (status 1 = the schema runs past the message)."""
    from ._lib import XdrField
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    _same_device(data, msg_offsets=msg_offsets)
    count = msg_offsets.numel() - 1
    fields = (XdrField * max(1, len(schema)))(*[XdrField(int(k), int(z)) for k, z in schema])
    if out is None:
        out = torch.empty(max(count, 0), dtype=out_dtype(method), device=data.device)
    elif (out.numel() < count or out.dtype != out_dtype(method) or out.device != data.device
          or not out.is_contiguous()):
        raise GpuChecksumError("out tensor has the wrong size, dtype or device, or is not contiguous")
    st = torch.ones(max(count, 0), dtype=torch.uint8, device=data.device) if status else None
    with _on(data):
        rc = _lib().mchecksum_gpu_checksum_xdr(method.encode(), fields, len(schema), data.data_ptr(),
                                               msg_offsets.data_ptr(), count, out.data_ptr(),
                                               st.data_ptr() if st is not None else None,
                                               _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_checksum_xdr")
    return (out, st) if status else out


def _xdr_fields(schema):
    from ._lib import XdrField
    return (XdrField * max(1, len(schema)))(*[XdrField(int(k), int(z)) for k, z in schema])


def verify_xdr_messages(method: str, data: torch.Tensor, msg_offsets: torch.Tensor, schema, payload_offset: int = 20,
                        hash_offset: int = 16, stream=None, offsets_host=None, status=None, mismatches=None):
    """verify_messages for a Mercury built with XDR encoding
    (mchecksum_gpu_verify_xdr_messages): each message's proc buffer starts at
    payload_offset and is walked with checksum_xdr's schema; the value is
    compared with the network-order u32 at hash_offset.  Returns (status uint8
    per message: 1 = short, truncated or a different CRC; count).  status and
    mismatches: None allocates, False passes NULL, a tensor is reused (the
    call adds to a counter the caller zeroed)."""
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("msg_offsets needs at least one entry")
    status, mism = _verdict_buffers(count, data.device, status, mismatches)
    _same_device(data, msg_offsets=msg_offsets)
    with _on(data):
        rc = _lib().mchecksum_gpu_verify_xdr_messages(method.encode(), _xdr_fields(schema), len(schema),
                                                      data.data_ptr(), msg_offsets.data_ptr(), count, payload_offset,
                                                      hash_offset, _ptr(status), _ptr(mism),
                                                      _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_xdr_messages")
    return status, mism


def seal_xdr_messages(method: str, data: torch.Tensor, msg_offsets: torch.Tensor, schema, payload_offset: int = 20,
                      hash_offset: int = 16, stream=None, offsets_host=None, status=None) -> torch.Tensor:
    """Sender side of verify_xdr_messages, in place
    (mchecksum_gpu_seal_xdr_messages): the proc checksum of each message is
    stored network-order at hash_offset.  Returns status (uint8 per message: 1
    = short or truncated, not written).  Only the 4 hash bytes of each sealed
    message are written.  Pass a preallocated `status` (uint8, >= count,
    filled with ones) to reuse it."""
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("msg_offsets needs at least one entry")
    status = _sender_status(data, count, status)
    _same_device(data, msg_offsets=msg_offsets, status=status)
    with _on(data):
        rc = _lib().mchecksum_gpu_seal_xdr_messages(method.encode(), _xdr_fields(schema), len(schema),
                                                    data.data_ptr(), msg_offsets.data_ptr(), count, payload_offset,
                                                    hash_offset, status.data_ptr(),
                                                    _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_xdr_messages")
    return status


def unpack_xdr_messages(method: str, data: torch.Tensor, msg_offsets: torch.Tensor, schema, dst: torch.Tensor,
                        dst_offsets: torch.Tensor, payload_offset: int = 20, hash_offset: int = 16, stream=None,
                        offsets_host=None, dst_offsets_host=None, status=None, mismatches=None):
    """verify_xdr_messages that also decodes, in one pass
    (mchecksum_gpu_unpack_xdr_messages): the hashed stream of message i -- its
    non-XDR image: every integer's host-order bytes, every byte array without
    its pad -- goes to dst[dst_offsets[i] : dst_offsets[i+1]].  Returns
    (status, count) with verify_xdr_messages' buffer rules.  Status 1 = the
    CRC differs (the destination then holds the bytes as decoded) or the
    message is short, truncated or its decoded length is not its slot's
    (nothing of it is written).  The decoded lengths depend on the data, so
    only the tables' bounds are checked here; with both host tables given the
    two ranges must not overlap."""
    _check_device_u8(data, "data")
    _check_device_u8(dst, "dst")
    _check_offsets(data, msg_offsets, offsets_host)
    _check_offsets(dst, dst_offsets, dst_offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0 or dst_offsets.numel() != count + 1:
        raise GpuChecksumError("msg_offsets and dst_offsets need the same number (>= 1) of entries")
    if offsets_host is not None and dst_offsets_host is not None and count:
        import numpy as np
        mo, do = np.asarray(offsets_host, dtype=np.uint64), np.asarray(dst_offsets_host, dtype=np.uint64)
        s0, d0 = data.data_ptr() + int(mo[0]), dst.data_ptr() + int(do[0])
        if s0 < d0 + int(do[-1] - do[0]) and d0 < s0 + int(mo[-1] - mo[0]):
            raise GpuChecksumError("the message and destination ranges overlap")
    status, mism = _verdict_buffers(count, data.device, status, mismatches)
    _same_device(data, msg_offsets=msg_offsets, dst=dst, dst_offsets=dst_offsets)
    with _on(data):
        rc = _lib().mchecksum_gpu_unpack_xdr_messages(method.encode(), _xdr_fields(schema), len(schema),
                                                      data.data_ptr(), msg_offsets.data_ptr(), count, payload_offset,
                                                      hash_offset, dst.data_ptr(), dst_offsets.data_ptr(),
                                                      _ptr(status), _ptr(mism), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_unpack_xdr_messages")
    return status, mism


def pack_xdr_messages(method: str, src: torch.Tensor, src_offsets: torch.Tensor, data: torch.Tensor,
                      msg_offsets: torch.Tensor, schema, payload_offset: int = 20, hash_offset: int = 16, stream=None,
                      src_offsets_host=None, offsets_host=None, status=None) -> torch.Tensor:
    """pack_messages for a Mercury built with XDR encoding, the mirror of
    unpack_xdr_messages (mchecksum_gpu_pack_xdr_messages): image i =
    src[src_offsets[i] : src_offsets[i+1]] -- every integer's host-order
    bytes, every byte array without its pad, in schema order -- is encoded to
    XDR behind the headers of message i of `data`, hashed in the same read
    and its CRC stored network-order at msg_offsets[i] + hash_offset.  XDR_SINT
    fields are sign-extended into their 32-bit word, XDR_INT ones
    zero-extended.  Returns status (uint8 per message: 1 = the schema does not
    consume the image exactly or the message is not payload_offset + the
    encoded length long: nothing of it is written).  The encoded lengths
    depend on the data (xdr_encoded_sizes computes them), so only the tables'
    bounds are checked here; with both host tables given the two ranges must
    not overlap."""
    _check_device_u8(src, "src")
    _check_device_u8(data, "data")
    _check_offsets(src, src_offsets, src_offsets_host)
    _check_offsets(data, msg_offsets, offsets_host)
    count = msg_offsets.numel() - 1
    if count < 0 or src_offsets.numel() != count + 1:
        raise GpuChecksumError("src_offsets and msg_offsets need the same number (>= 1) of entries")
    if src_offsets_host is not None and offsets_host is not None and count:
        import numpy as np
        so, mo = np.asarray(src_offsets_host, dtype=np.uint64), np.asarray(offsets_host, dtype=np.uint64)
        s0, d0 = src.data_ptr() + int(so[0]), data.data_ptr() + int(mo[0])
        if s0 < d0 + int(mo[-1] - mo[0]) and d0 < s0 + int(so[-1] - so[0]):
            raise GpuChecksumError("the source and destination ranges overlap")
    status = _sender_status(data, count, status)
    _same_device(data, src=src, src_offsets=src_offsets, msg_offsets=msg_offsets, status=status)
    with _on(data):
        rc = _lib().mchecksum_gpu_pack_xdr_messages(method.encode(), _xdr_fields(schema), len(schema), src.data_ptr(),
                                                    src_offsets.data_ptr(), data.data_ptr(), msg_offsets.data_ptr(),
                                                    count, payload_offset, hash_offset, status.data_ptr(),
                                                    _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_pack_xdr_messages")
    return status


def _xdr_sizes_out(data: torch.Tensor, count: int):
    return (torch.empty(max(count, 0), dtype=torch.int64, device=data.device),
            torch.empty(max(count, 0), dtype=torch.uint8, device=data.device))


def xdr_encoded_sizes(src: torch.Tensor, src_offsets: torch.Tensor, schema, stream=None, src_offsets_host=None):
    """The XDR length pack_xdr_messages would write for each image
    (mchecksum_gpu_xdr_encoded_sizes), computed on the device from the image's
    integers.  Returns (sizes int64, status uint8): 0 and status 1 where the
    schema does not consume the image exactly.  torch.cumsum of payload_offset
    + sizes is the message table."""
    _check_device_u8(src, "src")
    _check_offsets(src, src_offsets, src_offsets_host)
    _same_device(src, src_offsets=src_offsets)
    count = src_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("src_offsets needs at least one entry")
    sizes, status = _xdr_sizes_out(src, count)
    with _on(src):
        rc = _lib().mchecksum_gpu_xdr_encoded_sizes(_xdr_fields(schema), len(schema), src.data_ptr(),
                                                    src_offsets.data_ptr(), count, sizes.data_ptr(), status.data_ptr(),
                                                    _stream_handle(stream, src.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_xdr_encoded_sizes")
    return sizes, status


def xdr_decoded_sizes(data: torch.Tensor, msg_offsets: torch.Tensor, schema, payload_offset: int = 20, stream=None,
                      offsets_host=None):
    """The decoded length of each XDR-mode message -- what its slot in
    unpack_xdr_messages' destination table must be -- and the XDR bytes the
    schema consumed from payload_offset on (mchecksum_gpu_xdr_decoded_sizes).
    Returns (sizes int64, wire_sizes int64, status uint8): zeros and status 1
    where the message is shorter than payload_offset or the schema runs past
    it."""
    _check_device_u8(data, "data")
    _check_offsets(data, msg_offsets, offsets_host)
    _same_device(data, msg_offsets=msg_offsets)
    count = msg_offsets.numel() - 1
    if count < 0:
        raise GpuChecksumError("msg_offsets needs at least one entry")
    sizes, status = _xdr_sizes_out(data, count)
    wire = torch.empty_like(sizes)
    with _on(data):
        rc = _lib().mchecksum_gpu_xdr_decoded_sizes(_xdr_fields(schema), len(schema), data.data_ptr(),
                                                    msg_offsets.data_ptr(), count, payload_offset, sizes.data_ptr(),
                                                    wire.data_ptr(), status.data_ptr(),
                                                    _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_xdr_decoded_sizes")
    return sizes, wire, status


def verify_rpc_xdr_messages(data: torch.Tensor, msg_offsets: torch.Tensor, schema, kind: str = "request",
                            payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                            method: str = "crc32c", stream=None, offsets_host=None, status=None, counts=None):
    """verify_rpc_messages for a Mercury built with XDR encoding, in one launch
    (mchecksum_gpu_verify_rpc_xdr_messages): the core header's CRC-16, then its
    flags, then -- unless MORE_DATA says the payload is elsewhere -- the proc
    checksum of the fields behind payload_offset, walked with checksum_xdr's
    schema, against the network-order u32 at hash_offset.  Returns (status
    uint8 per message: RPC_OK, RPC_PAYLOAD, RPC_HEADER, RPC_SHORT -- no whole
    core header, shorter than payload_offset, or than its own fields need --,
    RPC_DEFERRED or RPC_FAULT; counts, int32 per class).  status / counts as
    for verify_rpc_messages.  Nothing is written to `data`."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    status = _rpc_status(data, count, status)
    counts = _rpc_counts(counts, RPC_CLASSES, data.device)
    _same_device(data, msg_offsets=msg_offsets, status=None if status is False else status,
                 counts=None if counts is False else counts)
    with _on(data):
        rc = _lib().mchecksum_gpu_verify_rpc_xdr_messages(header_method.encode(), method.encode(), k,
                                                          _xdr_fields(schema), len(schema), data.data_ptr(),
                                                          msg_offsets.data_ptr(), count, payload_offset, hash_offset,
                                                          _ptr(status), _ptr(counts),
                                                          _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_rpc_xdr_messages")
    return status, counts


def seal_rpc_xdr_messages(data: torch.Tensor, msg_offsets: torch.Tensor, schema, kind: str = "request",
                          payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                          method: str = "crc32c", stream=None, offsets_host=None, status=None):
    """Sender side of verify_rpc_xdr_messages, in place
    (mchecksum_gpu_seal_rpc_xdr_messages): the proc checksum network-order at
    hash_offset and the core header's CRC-16 at 12 (request) or 4 (response);
    with MORE_DATA set, the header's CRC-16 alone (RPC_DEFERRED).  Returns
    status (uint8 per message: RPC_OK, RPC_DEFERRED, RPC_SHORT = nothing
    written, or RPC_FAULT; False passes none and returns False).  Only those 2
    or 6 bytes are written."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    status = _rpc_status(data, count, status)
    _same_device(data, msg_offsets=msg_offsets, status=None if status is False else status)
    with _on(data):
        rc = _lib().mchecksum_gpu_seal_rpc_xdr_messages(header_method.encode(), method.encode(), k,
                                                        _xdr_fields(schema), len(schema), data.data_ptr(),
                                                        msg_offsets.data_ptr(), count, payload_offset, hash_offset,
                                                        _ptr(status), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_rpc_xdr_messages")
    return status


def unpack_rpc_xdr_messages(data: torch.Tensor, msg_offsets: torch.Tensor, schema, dst: torch.Tensor,
                            dst_offsets: torch.Tensor, kind: str = "request", payload_offset: int = 20,
                            hash_offset: int = 16, header_method: str = "crc16", method: str = "crc32c", stream=None,
                            offsets_host=None, dst_offsets_host=None, status=None, counts=None):
    """verify_rpc_xdr_messages that also decodes, in one launch
    (mchecksum_gpu_unpack_rpc_xdr_messages): the non-XDR image of an eager,
    whole message whose decoded length is its destination's goes to
    dst[dst_offsets[i] : dst_offsets[i+1]] as received -- whatever the header's
    and the payload's CRC turn out to be; look at the status first.  Returns
    (status uint8 per message: verify_rpc_xdr_messages' or RPC_MISFIT; counts,
    int32 per class, RPC_COPY_CLASSES words).  Nothing of a DEFERRED, SHORT or
    MISFIT message's destination is written.  The decoded lengths depend on the
    data (xdr_decoded_sizes computes them); `data` and `dst` must not overlap,
    which is checked here with both host tables given."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    _check_rpc_copy(data, msg_offsets, offsets_host, dst, dst_offsets, dst_offsets_host, ("dst", "dst_offsets"))
    status = _rpc_status(data, count, status)
    counts = _rpc_counts(counts, RPC_COPY_CLASSES, data.device)
    _same_device(data, msg_offsets=msg_offsets, dst=dst, dst_offsets=dst_offsets,
                 status=None if status is False else status, counts=None if counts is False else counts)
    with _on(data):
        rc = _lib().mchecksum_gpu_unpack_rpc_xdr_messages(header_method.encode(), method.encode(), k,
                                                          _xdr_fields(schema), len(schema), data.data_ptr(),
                                                          msg_offsets.data_ptr(), count, payload_offset, hash_offset,
                                                          dst.data_ptr(), dst_offsets.data_ptr(), _ptr(status),
                                                          _ptr(counts), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_unpack_rpc_xdr_messages")
    return status, counts


def pack_rpc_xdr_messages(src: torch.Tensor, src_offsets: torch.Tensor, data: torch.Tensor, msg_offsets: torch.Tensor,
                          schema, kind: str = "request", payload_offset: int = 20, hash_offset: int = 16,
                          header_method: str = "crc16", method: str = "crc32c", stream=None, src_offsets_host=None,
                          offsets_host=None, status=None):
    """seal_rpc_xdr_messages that also encodes, in one launch
    (mchecksum_gpu_pack_rpc_xdr_messages): the caller has filled every header
    byte of `data` but the two hashes.  An eager, whole message whose size is
    payload_offset + the XDR length of its image src[src_offsets[i] :
    src_offsets[i+1]] (pack_xdr_messages' image and schema rules) gets the XDR
    bytes behind its headers, the proc checksum at hash_offset and the core
    header's CRC-16 (RPC_OK); one with MORE_DATA set the header's CRC-16 alone
    (RPC_DEFERRED, its image is not read); RPC_SHORT and RPC_MISFIT messages
    are not written.  Returns status (uint8 per message, or RPC_FAULT; False
    passes none and returns False).  `src` and `data` must not overlap, which
    is checked here with both host tables given."""
    count, k = _check_rpc(data, msg_offsets, offsets_host, kind, payload_offset, hash_offset)
    _check_rpc_copy(data, msg_offsets, offsets_host, src, src_offsets, src_offsets_host, ("src", "src_offsets"))
    status = _rpc_status(data, count, status)
    _same_device(data, src=src, src_offsets=src_offsets, msg_offsets=msg_offsets,
                 status=None if status is False else status)
    with _on(data):
        rc = _lib().mchecksum_gpu_pack_rpc_xdr_messages(header_method.encode(), method.encode(), k,
                                                        _xdr_fields(schema), len(schema), src.data_ptr(),
                                                        src_offsets.data_ptr(), data.data_ptr(),
                                                        msg_offsets.data_ptr(), count, payload_offset, hash_offset,
                                                        _ptr(status), _stream_handle(stream, data.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_pack_rpc_xdr_messages")
    return status


def verify_rpc_xdr_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, schema, kind: str = "request",
                                payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                                method: str = "crc32c", stream=None, addr_host=None, len_host=None, status=None,
                                counts=None):
    """verify_rpc_xdr_messages with the messages addressed by a list
    (mchecksum_gpu_verify_rpc_xdr_message_list): message i is the msg_len[i]
    bytes at the device address msg_addr[i] (device int64 tensors,
    rpc_message_list builds them) -- in any number of allocations, in any
    order, with any gaps.  Schema, rules, statuses and counts are
    verify_rpc_xdr_messages'; returns (status, counts).  A message shorter than
    16 bytes is RPC_SHORT and its address is not used."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, False)
    status = _rpc_status(msg_addr, count, status)
    counts = _rpc_counts(counts, RPC_CLASSES, msg_addr.device)
    _same_device(msg_addr, msg_len=msg_len, status=None if status is False else status,
                 counts=None if counts is False else counts)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_verify_rpc_xdr_message_list(header_method.encode(), method.encode(), k,
                                                              _xdr_fields(schema), len(schema), msg_addr.data_ptr(),
                                                              msg_len.data_ptr(), count, payload_offset, hash_offset,
                                                              _ptr(status), _ptr(counts),
                                                              _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_verify_rpc_xdr_message_list")
    return status, counts


def seal_rpc_xdr_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, schema, kind: str = "request",
                              payload_offset: int = 20, hash_offset: int = 16, header_method: str = "crc16",
                              method: str = "crc32c", stream=None, addr_host=None, len_host=None, status=None):
    """seal_rpc_xdr_messages with the messages addressed by a list
    (mchecksum_gpu_seal_rpc_xdr_message_list), written through their addresses:
    the same 2 or 6 bytes of a message, no others.  The messages must not
    overlap one another; with both host arrays given that is checked here.
    Returns status as seal_rpc_xdr_messages does."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, True)
    status = _rpc_status(msg_addr, count, status)
    _same_device(msg_addr, msg_len=msg_len, status=None if status is False else status)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_seal_rpc_xdr_message_list(header_method.encode(), method.encode(), k,
                                                            _xdr_fields(schema), len(schema), msg_addr.data_ptr(),
                                                            msg_len.data_ptr(), count, payload_offset, hash_offset,
                                                            _ptr(status), _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_seal_rpc_xdr_message_list")
    return status


def unpack_rpc_xdr_message_list(msg_addr: torch.Tensor, msg_len: torch.Tensor, schema, dst: torch.Tensor,
                                dst_offsets: torch.Tensor, kind: str = "request", payload_offset: int = 20,
                                hash_offset: int = 16, header_method: str = "crc16", method: str = "crc32c",
                                stream=None, addr_host=None, len_host=None, dst_offsets_host=None, status=None,
                                counts=None):
    """unpack_rpc_xdr_messages with the messages addressed by a list
    (mchecksum_gpu_unpack_rpc_xdr_message_list); the destination stays
    dst[dst_offsets[i] : dst_offsets[i+1]].  Schema, rules, statuses, counts and
    what is written are unpack_rpc_xdr_messages'; returns (status, counts).  No
    message may overlap `dst`; with all three host copies given that is checked
    here."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, False)
    _check_rpc_list_copy(addr_host, len_host, count, dst, dst_offsets, dst_offsets_host, ("dst", "dst_offsets"))
    status = _rpc_status(msg_addr, count, status)
    counts = _rpc_counts(counts, RPC_COPY_CLASSES, msg_addr.device)
    _same_device(msg_addr, msg_len=msg_len, dst=dst, dst_offsets=dst_offsets,
                 status=None if status is False else status, counts=None if counts is False else counts)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_unpack_rpc_xdr_message_list(header_method.encode(), method.encode(), k,
                                                              _xdr_fields(schema), len(schema), msg_addr.data_ptr(),
                                                              msg_len.data_ptr(), count, payload_offset, hash_offset,
                                                              dst.data_ptr(), dst_offsets.data_ptr(), _ptr(status),
                                                              _ptr(counts), _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_unpack_rpc_xdr_message_list")
    return status, counts


def pack_rpc_xdr_message_list(src: torch.Tensor, src_offsets: torch.Tensor, msg_addr: torch.Tensor,
                              msg_len: torch.Tensor, schema, kind: str = "request", payload_offset: int = 20,
                              hash_offset: int = 16, header_method: str = "crc16", method: str = "crc32c", stream=None,
                              src_offsets_host=None, addr_host=None, len_host=None, status=None):
    """pack_rpc_xdr_messages with the messages addressed by a list
    (mchecksum_gpu_pack_rpc_xdr_message_list): the headers are read and the XDR
    bytes and hashes written through the addresses; the images stay
    src[src_offsets[i] : src_offsets[i+1]].  Schema, rules, statuses and what is
    written are pack_rpc_xdr_messages'; returns status.  The messages must not
    overlap one another or `src`; with the host copies given that is checked
    here."""
    count, k = _check_rpc_list(msg_addr, msg_len, addr_host, len_host, kind, payload_offset, hash_offset, True)
    _check_rpc_list_copy(addr_host, len_host, count, src, src_offsets, src_offsets_host, ("src", "src_offsets"))
    status = _rpc_status(msg_addr, count, status)
    _same_device(msg_addr, msg_len=msg_len, src=src, src_offsets=src_offsets,
                 status=None if status is False else status)
    with _on(msg_addr):
        rc = _lib().mchecksum_gpu_pack_rpc_xdr_message_list(header_method.encode(), method.encode(), k,
                                                            _xdr_fields(schema), len(schema), src.data_ptr(),
                                                            src_offsets.data_ptr(), msg_addr.data_ptr(),
                                                            msg_len.data_ptr(), count, payload_offset, hash_offset,
                                                            _ptr(status), _stream_handle(stream, msg_addr.device))
    if rc != 0:
        _err(rc, "mchecksum_gpu_pack_rpc_xdr_message_list")
    return status


def fill_splitmix(t: torch.Tensor, seed: int, first_word: int = 0, stream=None) -> torch.Tensor:
    """Fill a device tensor with the synthetic payload bytes of SURVEY.md 8(d)."""
    _check_device_u8(t, "tensor")
    if t.data_ptr() % 16:
        raise GpuChecksumError("tensor must be 16-byte aligned")
    B = load_bench_library()
    with _on(t):
        rc = B.mck_bench_fill_splitmix(t.data_ptr(), t.numel() * t.element_size(), seed & (2**64 - 1),
                                       first_word, _stream_handle(stream, t.device))
    if rc != 0:
        raise GpuChecksumError(f"fill_splitmix failed rc={rc}")
    return t


class HostGate:
    """Test utility (libmchecksum_bench.so): a kernel that holds a stream until
    the host calls release() -- one wave polling a word of coherent host
    memory -- or until max_seconds pass, which `expired` then reports.  Used
    to keep launches queued for exactly as long as a test needs."""

    def __init__(self):
        self._B = load_bench_library()
        self._mem = self._B.mck_bench_host_alloc(8)
        if not self._mem:
            raise GpuChecksumError("hipHostMalloc failed")
        self._flag = ctypes.c_uint32.from_address(self._mem)
        self._exp = ctypes.c_uint32.from_address(self._mem + 4)

    def hold(self, stream, max_seconds: float = 20.0) -> None:
        self._flag.value = 0
        self._exp.value = 0
        h = _stream_handle(stream)
        if self._B.mck_bench_gate(self._mem, self._mem + 4, float(max_seconds), h) != 0:
            raise GpuChecksumError("gate launch failed")

    def release(self) -> None:
        self._flag.value = 1

    @property
    def expired(self) -> bool:
        return bool(self._exp.value)

    def close(self) -> None:
        if self._mem:
            self.release()
            torch.cuda.synchronize()
            self._B.mck_bench_host_free(self._mem)
            self._mem = None


def as_unsigned(x: torch.Tensor):
    """Device CRC tensor -> numpy unsigned array on the host."""
    import numpy as np
    a = x.detach().cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint64)
