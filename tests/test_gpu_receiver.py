"""Receiver side on the GPU (include/mchecksum_gpu.h): unpack_messages copies
every payload out of the receive buffer and verifies it in the same pass --
HG_PROC_TYPE on HG_DECODE (src/mercury_proc.h:124-143,162-181) followed by
hg_get_struct's compare (src/mercury.c:565-573).  The hashes in the messages
come from the streaming API (mchecksum_update / get); every destination byte is
compared with the bytes received, and every byte the call must not write with
its value before the call.
"""
import ctypes
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLIB = os.path.join(ROOT, "build", "libmchecksum_qfault.so")
CORE_HDR, HG_HDR = 16, 4
PAY = CORE_HDR + HG_HDR
CANARY = 0xEE
SEED = 9
# (message buffer, destination) base shifts: (dst - src) mod 4 = 0, 1, 3, 2; the 20-byte headers step
# (dst - src) mod 16 by 4 from one message to the next
SHIFTS = ((0, 0), (1, 2), (2, 1), (3, 1))
SRC_LEAD, DST_LEAD, TAIL = 48, 80, 96
BIG = (65535, 65536, 65537, 70001, 66000, 67891, 69999, 68000)


def _stream_crc(data):
    from mercury_amd import Checksum
    ck = Checksum("crc32c")
    ck.update(data)
    return ck.get()


def _tables(lens, msg_start, dst_start):
    mo = np.zeros(len(lens) + 1, dtype=np.uint64)
    mo[1:] = np.cumsum(np.asarray(lens) + PAY)
    do = np.zeros(len(lens) + 1, dtype=np.uint64)
    do[1:] = np.cumsum(lens)
    return mo + np.uint64(msg_start), do + np.uint64(dst_start)


def _messages(rng, mo, nbytes):
    """The receive buffer: random bytes, and behind every message's headers the
    streaming API's CRC of its payload, network order."""
    buf = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    for a, b in zip(mo[:-1].astype(np.int64), mo[1:].astype(np.int64)):
        if b - a >= PAY:
            buf[a + CORE_HDR:a + PAY] = np.frombuffer(struct.pack(">I", _stream_crc(buf[a + PAY:b].tobytes())), dtype=np.uint8)
    return buf


def build_case():
    """~4000 messages with payloads of 0..2100 bytes and eight of 65535..70001,
    back to back from a non-zero offset; their destinations back to back from a
    non-zero offset.  Pure numpy: the residue coverage is asserted here."""
    rng = np.random.default_rng(SEED)
    lens = rng.integers(0, 2101, 4000)
    lens[4 + rng.choice(3990, 8, replace=False)] = BIG
    lens[:4] = (0, 1, 2100, 16)
    lens[-1] = 777
    mo, do = _tables(lens, 37, 5)
    buf = _messages(rng, mo, int(mo[-1]) + 11)
    buf.setflags(write=False)
    # every source residue and every relative misalignment occurs (bases 16-byte aligned + shift)
    sres, rel = set(), set()
    live = lens > 0
    for ss, ds in SHIFTS:
        s_at = mo[:-1].astype(np.int64) + PAY + SRC_LEAD + ss
        d_at = do[:-1].astype(np.int64) + DST_LEAD + ds
        sres |= set((s_at[live] % 16).tolist())
        rel |= set(((d_at[live] - s_at[live]) % 16).tolist())
    assert sres == set(range(16)) and rel == set(range(16)), (sorted(sres), sorted(rel))
    return buf, mo, do, lens


@pytest.fixture(scope="module")
def case():
    return build_case()


def _expected_dst(buf, mo, do, skip=()):
    """The destination view (it ends with the last payload): canary, then the
    payloads as they sit in buf."""
    want = np.full(int(do[-1]), CANARY, dtype=np.uint8)
    for i in range(len(mo) - 1):
        if i not in skip:
            want[int(do[i]):int(do[i + 1])] = buf[int(mo[i]) + PAY:int(mo[i + 1])]
    return want


def _device(torch, buf, ss, ds, ndst):
    """(message base, message view, destination base, destination view) on 16-byte-aligned bases."""
    sbase = torch.full((SRC_LEAD + 4 + buf.size + TAIL,), 0x11, dtype=torch.uint8, device="cuda")
    dbase = torch.full((DST_LEAD + 4 + ndst + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
    assert sbase.data_ptr() % 16 == 0 and dbase.data_ptr() % 16 == 0
    sview = sbase[SRC_LEAD + ss:SRC_LEAD + ss + buf.size]
    dview = dbase[DST_LEAD + ds:DST_LEAD + ds + ndst]  # ends with the last payload: no padding
    sview.copy_(torch.from_numpy(np.array(buf)))
    return sbase, sview, dbase, dview


def _check_dst(dbase, ds, want, mo_or_do, what=""):
    got = dbase.cpu().numpy()
    lo, hi = DST_LEAD + ds, DST_LEAD + ds + want.size
    diff = np.nonzero(got[lo:hi] != want)[0]
    assert diff.size == 0, (f"{what}: {diff.size} destination bytes differ, first at {diff[:4]} "
                            f"(message {np.searchsorted(mo_or_do, diff[0], side='right') - 1})")
    assert np.all(got[:lo] == CANARY) and np.all(got[hi:] == CANARY), f"{what}: a byte outside the destination view was written"


@pytest.mark.parametrize("light,nt", [("0", None), ("1", None), ("0", "1")])
def test_unpack_messages(gpu, case, light, nt, monkeypatch):
    import torch
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)
    buf, mo, do, lens = case
    mod, dod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo, do))
    want = _expected_dst(buf, mo, do)
    assert np.all(want[:int(do[0])] == CANARY)  # the bytes before the first payload are canary too
    for ss, ds in SHIFTS:
        sbase, sview, dbase, dview = _device(torch, buf, ss, ds, int(do[-1]))
        sbefore = sbase.cpu().numpy()
        status, mism = gpu.unpack_messages(sview, mod, dview, dod, offsets_host=mo, dst_offsets_host=do)
        _check_dst(dbase, ds, want, do, f"shifts {ss}/{ds}")
        assert np.array_equal(sbase.cpu().numpy(), sbefore), "the message buffer changed"
        assert int(status.sum().item()) == 0 and int(mism.item()) == 0


@pytest.mark.parametrize("light", ["0", "1"])
def test_unpack_corrupted(gpu, case, light, monkeypatch):
    """One payload bit flipped in some messages (a 1-byte one, a 65 KiB one,
    the last), one hash-slot bit in others (the empty payload among them):
    status 1 exactly there, and every destination holds the bytes received."""
    import torch
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    clean, mo, do, lens = case
    n = len(lens)
    big = int(np.nonzero(lens == 70001)[0][0])
    pay_hits = {1: 0, big: 40000, 2: 2099, n - 1: 776}  # message: payload byte
    hash_hits = {0: 0, 3: 3, 1000: 1}  # message: hash byte
    assert lens[0] == 0 and lens[1] == 1 and all(lens[i] > b for i, b in pay_hits.items())
    buf = np.array(clean)
    for i, b in pay_hits.items():
        buf[int(mo[i]) + PAY + b] ^= 0x04
    for i, b in hash_hits.items():
        buf[int(mo[i]) + CORE_HDR + b] ^= 0x80
    bad = sorted(set(pay_hits) | set(hash_hits))
    mod, dod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo, do))
    ss, ds = SHIFTS[1]
    sbase, sview, dbase, dview = _device(torch, buf, ss, ds, int(do[-1]))
    status, mism = gpu.unpack_messages(sview, mod, dview, dod, offsets_host=mo, dst_offsets_host=do)
    assert np.nonzero(status.cpu().numpy())[0].tolist() == bad
    assert int(mism.item()) == len(bad)
    _check_dst(dbase, ds, _expected_dst(buf, mo, do), do, "corrupted batch")


@pytest.mark.parametrize("kind", ["minus1", "plus1", "short"])
def test_unpack_misfit(gpu, kind):
    """A message one byte smaller or larger than headers + destination, or
    shorter than its headers: status 1, one mismatch, its destination still
    canary, its neighbours unpacked."""
    import torch
    rng = np.random.default_rng(12)
    dlens = np.array([300, 17, 1500, 0, 64])
    sizes = dlens + PAY
    sizes[2] = {"minus1": sizes[2] - 1, "plus1": sizes[2] + 1, "short": PAY - 10}[kind]
    mo = np.zeros(6, dtype=np.uint64)
    mo[1:] = np.cumsum(sizes)
    mo += 3
    do = np.zeros(6, dtype=np.uint64)
    do[1:] = np.cumsum(dlens)
    do += 9
    buf = _messages(rng, mo, int(mo[-1]))
    s = torch.zeros(buf.size + 64, dtype=torch.uint8, device="cuda")
    s[:buf.size].copy_(torch.from_numpy(buf))
    d = torch.full((int(do[-1]) + 32,), CANARY, dtype=torch.uint8, device="cuda")
    mod, dod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo, do))
    # (the host check refuses the tables outright when both copies are given)
    with pytest.raises(gpu.GpuChecksumError, match="does not fit"):
        gpu.unpack_messages(s, mod, d, dod, offsets_host=mo, dst_offsets_host=do)
    status, mism = gpu.unpack_messages(s, mod, d, dod)
    assert status.cpu().tolist() == [0, 0, 1, 0, 0]
    assert int(mism.item()) == 1
    want = np.full(int(do[-1]) + 32, CANARY, dtype=np.uint8)
    want[:int(do[-1])] = _expected_dst(buf, mo, do, skip=(2,))
    assert np.array_equal(d.cpu().numpy(), want)
    assert np.array_equal(s[:buf.size].cpu().numpy(), buf)


def test_unpack_host_checks(gpu):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    mo = np.array([50, 170], dtype=np.uint64)
    do = np.array([0, 100], dtype=np.uint64)
    mod, dod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo, do))
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.unpack_messages(buf, mod, buf, dod, offsets_host=mo, dst_offsets_host=do)
    with pytest.raises(gpu.GpuChecksumError, match="hash_offset"):
        gpu.unpack_messages(buf, mod, buf[2048:], dod, payload_offset=18)  # hash overlaps payload
    with pytest.raises(gpu.GpuChecksumError, match="crc32c only"):
        gpu.unpack_messages(buf, mod, buf[2048:], dod, method="crc64")


def test_graph_pack_unpack(gpu):
    """pack_messages -> unpack_messages captured on one stream; each replay
    moves the source's current bytes through the message buffer."""
    import torch
    gpu.prepare("crc32c")
    rng = np.random.default_rng(22)
    lens = rng.integers(0, 3000, 1500)  # > 1024 messages: the throughput kernels, on the static split
    lens[:3] = (0, 70000, 5)
    mo, so = _tables(lens, 0, 0)
    do = so + np.uint64(13)
    fills = [rng.integers(0, 256, size=int(so[-1]), dtype=np.uint8) for _ in range(2)]
    src = torch.zeros(int(so[-1]) + 64, dtype=torch.uint8, device="cuda")
    msg = torch.zeros(int(mo[-1]) + 16, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(int(do[-1]), dtype=torch.uint8, device="cuda")
    sod, mod, dod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (so, mo, do))
    n = len(lens)
    pstat = torch.ones(n, dtype=torch.uint8, device="cuda")
    ustat = torch.ones(n, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.pack_messages(src, sod, msg, mod, status=pstat)
        gpu.unpack_messages(msg, mod, dst, dod, status=ustat, mismatches=mism)
    torch.cuda.synchronize()
    for fill in fills:
        with torch.cuda.stream(s):
            src[:fill.size].copy_(torch.from_numpy(fill))
            dst.fill_(CANARY)
            pstat.fill_(1)
            ustat.fill_(1)
            mism.zero_()
            g.replay()
        s.synchronize()
        got = dst.cpu().numpy()
        assert np.all(got[:13] == CANARY)
        assert np.array_equal(got[13:], fill)
        assert int(mism.item()) == 0
        assert int(pstat.sum().item()) == 0 and int(ustat.sum().item()) == 0


def test_unpack_fault_fails_closed(gpu, case, monkeypatch):
    """The fault-injection build in its give-up mode (a wave drops one unit, as
    one whose bounded wait timed out would; no stall): the error word gets 1,
    the counter at least count, and every message with status 0 has its bytes
    in the destination."""
    import torch
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    L = ctypes.CDLL(QLIB)
    c = ctypes
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    L.mchecksum_gpu_unpack_messages.argtypes = [c.c_char_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t,
                                                c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_set_error_word.argtypes = [c.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = c.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    monkeypatch.delenv("MCHECKSUM_GPU_QFAULT_MODE", raising=False)  # the give-up, not a stall
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", "0")
    L.mchecksum_gpu_reload_settings()
    try:
        buf, mo, do, lens = case  # > 1024 messages: the launch takes the work queue
        n = len(lens)
        mod, dod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo, do))
        ss, ds = SHIFTS[2]
        sbase, sview, dbase, dview = _device(torch, buf, ss, ds, int(do[-1]))
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")  # stale "verified" everywhere
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        faults0 = L.mchecksum_gpu_queue_faults()
        assert L.mchecksum_gpu_prepare(b"crc32c") == 0
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_unpack_messages(b"crc32c", sview.data_ptr(), mod.data_ptr(), n, PAY, CORE_HDR,
                                                 dview.data_ptr(), dod.data_ptr(), status.data_ptr(), mism.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        assert int(mism.item()) >= n
        st = status.cpu().numpy()
        assert set(np.unique(st).tolist()) <= {0, 1} and int(st.sum()) >= 1
        got = dbase.cpu().numpy()
        lo = DST_LEAD + ds
        view = got[lo:lo + int(do[-1])]
        want = _expected_dst(buf, mo, do)
        copied = np.array([np.array_equal(view[int(a):int(b)], want[int(a):int(b)]) for a, b in zip(do[:-1], do[1:])])
        assert np.all(copied[st == 0]), "a message reads as verified without its bytes in the destination"
        missing = np.nonzero(~copied)[0]
        assert missing.size <= 1  # only the dropped unit went uncopied ...
        for i in missing:  # ... and nothing of it was written
            assert np.all(view[int(do[i]):int(do[i + 1])] == CANARY)
        assert np.all(got[:lo + int(do[0])] == CANARY) and np.all(got[lo + int(do[-1]):] == CANARY)
    finally:
        monkeypatch.undo()
        L.mchecksum_gpu_reload_settings()


def test_unpack_payload_past_2_gib(gpu):
    """A payload of more than 2^31 bytes takes the 64-bit-length loop
    (payload32_generic), which stores by the same rule; between two small
    neighbours, message buffer and destination misaligned by an odd number of
    bytes.  The hashes in the messages are the streaming API's over the host
    copy of the payloads, so status 0 says the kernel computed the same."""
    import torch

    from mercury_amd import _lib
    big = (1 << 31) + 4096 * 3 + 5
    lens = np.array([100, big, 4097])
    mo, do = _tables(lens, 16, 7)
    assert int(mo[1] + PAY - do[1]) % 2 == 1
    pay = torch.empty(int(lens.sum()) + 64, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(pay, 0xB18)
    host = pay.cpu().numpy()
    L = _lib.load_library()
    msg = torch.full((int(mo[-1]) + 48,), 0x33, dtype=torch.uint8, device="cuda")
    at = 0
    for i in range(3):
        ln, m = int(lens[i]), int(mo[i])
        obj, val = ctypes.c_void_p(), ctypes.c_uint32(0)
        assert L.mchecksum_init(b"crc32c", ctypes.byref(obj)) == 0
        assert L.mchecksum_update(obj, host.ctypes.data + at, ln) == 0
        assert L.mchecksum_get(obj, ctypes.byref(val), 4, 1) == 0
        L.mchecksum_destroy(obj)
        msg[m + CORE_HDR:m + PAY].copy_(torch.from_numpy(np.frombuffer(struct.pack(">I", val.value), dtype=np.uint8).copy()))
        msg[m + PAY:m + PAY + ln].copy_(pay[at:at + ln])
        at += ln
    del host
    dst = torch.full((int(do[-1]),), CANARY, dtype=torch.uint8, device="cuda")
    mod, dod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo, do))
    status, mism = gpu.unpack_messages(msg, mod, dst, dod, offsets_host=mo, dst_offsets_host=do)
    assert status.cpu().tolist() == [0, 0, 0] and int(mism.item()) == 0
    assert bool((dst[:int(do[0])] == CANARY).all())
    assert torch.equal(dst[int(do[0]):], pay[:int(lens.sum())])
