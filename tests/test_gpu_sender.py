"""Sender side on the GPU (include/mchecksum_gpu.h): seal_messages stores the
payload hashes in place, pack_messages copies device-resident payloads behind
their headers and hashes them in the same pass, seal_core_headers stores the
core headers' CRC16.  Every value is compared bit for bit with the streaming
API's (what HG_PROC_TYPE + hg_set_struct produce, src/mercury_proc.h:124-181,
src/mercury.c:699-707), every byte the calls must not write with its value
before the call, and the receiver's verify calls must pass on the result.
"""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLIB = os.path.join(ROOT, "build", "libmchecksum_qfault.so")
CORE_HDR, HG_HDR = 16, 4
PAY = CORE_HDR + HG_HDR
EDGE_LENS = (0, 1, 3, 4, 15, 16, 17, 1023, 1024, 1025, 65535, 65536, 70000)


def _stream_crc(chunks):
    from mercury_amd import Checksum
    ck = Checksum("crc32c")
    for c in chunks:
        ck.update(c)
    return ck.get()


def _encode_message(rng, payload_len):
    """tests/test_gpu_rpc.py's message (core header, HG header, then the proc
    fields streamed through the drop-in API), with the payload length given
    exactly: a u32 length field and the raw bytes from 4 bytes on, raw bytes
    alone below that."""
    raw = rng.integers(0, 256, size=payload_len, dtype=np.uint8).tobytes()
    fields = (raw[:4], raw[4:]) if payload_len >= 4 else (raw,)
    crc = _stream_crc(fields)
    core = rng.integers(0, 256, size=CORE_HDR, dtype=np.uint8).tobytes()
    return core + struct.pack(">I", crc) + raw, crc


def _batch(rng, n, first=()):
    msgs, crcs = [], []
    for i in range(n):
        if i < len(first):
            ln = first[i]
        else:
            ln = int(rng.integers(0, 9000)) if i % 7 else int(rng.integers(0, 70000))
        m, c = _encode_message(rng, ln)
        msgs.append(m)
        crcs.append(c)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return b"".join(msgs), off, crcs


def _slots(off):
    """Index array of the 4 hash bytes of every message."""
    starts = off[:-1].astype(np.int64) + CORE_HDR
    return (starts[:, None] + np.arange(4)[None, :]).ravel()


@pytest.fixture(scope="module")
def sealed_batch():
    """700 messages, the edge payload lengths first; `want` = the messages as
    the host sender leaves them + 64 canary bytes; `blank` = the same with
    every hash slot 0xA5.  Shared and never modified."""
    rng = np.random.default_rng(2025)
    buf, off, crcs = _batch(rng, 700, EDGE_LENS)
    want = np.concatenate([np.frombuffer(buf, dtype=np.uint8), np.full(64, 0x5C, dtype=np.uint8)])
    blank = want.copy()
    blank[_slots(off)] = 0xA5
    assert set(EDGE_LENS) <= set((off[1:] - off[:-1] - PAY).astype(np.int64).tolist())
    want.setflags(write=False)
    blank.setflags(write=False)
    return want, blank, off


@pytest.mark.parametrize("light,nt", [("0", None), ("1", None), ("0", "1")])
def test_seal_messages_in_place(gpu, sealed_batch, light, nt, monkeypatch):
    import torch
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)
    want, blank, off = sealed_batch
    t = torch.from_numpy(blank.copy()).cuda()
    offs = torch.from_numpy(off.astype(np.int64)).cuda()
    status = gpu.seal_messages(t, offs, offsets_host=off)
    got = t.cpu().numpy()
    slots = _slots(off)
    bad = np.nonzero(got[slots].reshape(-1, 4) != want[slots].reshape(-1, 4))[0]
    assert bad.size == 0, f"hash slots of messages {sorted(set(bad.tolist()))[:8]} differ from the streaming API's"
    assert np.array_equal(got, want), "a byte outside the hash slots changed"
    assert int(status.sum().item()) == 0
    vstatus, mism = gpu.verify_messages(t, offs, offsets_host=off)
    assert int(mism.item()) == 0 and int(vstatus.sum().item()) == 0


def test_seal_short_message(gpu, sealed_batch):
    import torch
    want, blank, off = sealed_batch
    n0 = int(off[1])
    table = np.array([0, 10, 10 + n0], dtype=np.uint64)
    host = np.full(10 + n0 + 64, 0x77, dtype=np.uint8)
    host[10:10 + n0] = blank[:n0]
    t = torch.from_numpy(host.copy()).cuda()
    status = gpu.seal_messages(t, torch.from_numpy(table.astype(np.int64)).cuda(), offsets_host=table)
    assert status.cpu().tolist() == [1, 0]
    host[10:10 + n0] = want[:n0]
    assert np.array_equal(t.cpu().numpy(), host)  # the 10 bytes and the pad untouched, message 0 sealed


# ---- pack ----
PACK_SEED = 7
PACK_SHIFTS = ((0, 0), (1, 2), (2, 1), (3, 1))  # (source, destination) base shifts: dst - src = 0, 1, 3, 2 mod 4
SRC_LEAD, DST_LEAD, TAIL = 48, 80, 96


@pytest.fixture(scope="module")
def pack_case():
    """~4000 payloads of 0..2100 bytes and eight of 65535..70001, back to back
    in a source buffer; their messages back to back in the destination.
    Tables are relative to the (shifted) views; reference CRCs from the
    streaming API, computed once."""
    rng = np.random.default_rng(PACK_SEED)
    lens = rng.integers(0, 2101, 4000)
    big = np.array([65535, 65536, 65537, 70001, 66000, 67891, 69999, 68000])
    lens[4 + rng.choice(3996, 8, replace=False)] = big
    lens[:4] = (0, 1, 2100, 16)
    so = np.zeros(len(lens) + 1, dtype=np.uint64)
    so[1:] = np.cumsum(lens)
    so += 5  # the first payload does not start the buffer
    mo = np.zeros(len(lens) + 1, dtype=np.uint64)
    mo[1:] = np.cumsum(lens + PAY)
    mo += 37
    src = rng.integers(0, 256, size=int(so[-1]) + 11, dtype=np.uint8)
    crcs = [_stream_crc((src[int(a):int(b)].tobytes(),)) for a, b in zip(so[:-1], so[1:])]
    src.setflags(write=False)
    # every source residue and every relative misalignment occurs (bases 16-byte aligned + shift)
    sres, rel = set(), set()
    for ss, ds in PACK_SHIFTS:
        s_at = so[:-1].astype(np.int64) + SRC_LEAD + ss
        d_at = mo[:-1].astype(np.int64) + PAY + DST_LEAD + ds
        live = lens > 0
        sres |= set((s_at[live] % 16).tolist())
        rel |= set(((d_at[live] - s_at[live]) % 16).tolist())
    assert sres == set(range(16)) and rel == set(range(16)), (sorted(sres), sorted(rel))
    return src, so, mo, crcs


def _expected_dst(src, so, mo, crcs, nbytes, skip=()):
    want = np.full(nbytes, 0xEE, dtype=np.uint8)
    for i in range(len(crcs)):
        if i in skip:
            continue
        a, b = int(mo[i]), int(mo[i + 1])
        want[a + PAY:b] = src[int(so[i]):int(so[i + 1])]
        want[a + CORE_HDR:a + PAY] = np.frombuffer(struct.pack(">I", crcs[i]), dtype=np.uint8)
    return want


@pytest.mark.parametrize("light", ["0", "1"])
def test_pack_messages(gpu, pack_case, light, monkeypatch):
    import torch
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    src, so, mo, crcs = pack_case
    sod = torch.from_numpy(so.astype(np.int64)).cuda()
    mod = torch.from_numpy(mo.astype(np.int64)).cuda()
    nsrc, ndst = src.size, int(mo[-1])
    want = _expected_dst(src, so, mo, crcs, ndst)
    for ss, ds in PACK_SHIFTS:
        sbase = torch.full((SRC_LEAD + 4 + nsrc + TAIL,), 0x11, dtype=torch.uint8, device="cuda")
        dbase = torch.full((DST_LEAD + 4 + ndst + TAIL,), 0xEE, dtype=torch.uint8, device="cuda")
        assert sbase.data_ptr() % 16 == 0 and dbase.data_ptr() % 16 == 0
        sview = sbase[SRC_LEAD + ss:SRC_LEAD + ss + nsrc]
        dview = dbase[DST_LEAD + ds:DST_LEAD + ds + ndst]  # ends with the last message: no padding
        sview.copy_(torch.from_numpy(src.copy()))
        sbefore = sbase.cpu().numpy()
        status = gpu.pack_messages(sview, sod, dview, mod, src_offsets_host=so, offsets_host=mo)
        got = dbase.cpu().numpy()
        inside = got[DST_LEAD + ds:DST_LEAD + ds + ndst]
        diff = np.nonzero(inside != want)[0]
        assert diff.size == 0, (f"shifts {ss}/{ds}: {diff.size} destination bytes differ, first at {diff[:4]} "
                                f"(message {np.searchsorted(mo, diff[0], side='right') - 1})")
        assert np.all(got[:DST_LEAD + ds] == 0xEE) and np.all(got[DST_LEAD + ds + ndst:] == 0xEE), \
            "a byte before the first or after the last message was written"
        assert np.array_equal(sbase.cpu().numpy(), sbefore), "the source changed"
        assert int(status.sum().item()) == 0
        vstatus, mism = gpu.verify_messages(dview, mod, offsets_host=mo)
        assert int(mism.item()) == 0 and int(vstatus.sum().item()) == 0


@pytest.mark.parametrize("delta", [-1, 1])
def test_pack_misfit(gpu, delta):
    """A message one byte smaller or larger than header + payload: status 1,
    its region untouched, its neighbours packed."""
    import torch
    rng = np.random.default_rng(11)
    lens = np.array([300, 17, 1500, 0, 64])
    so = np.zeros(6, dtype=np.uint64)
    so[1:] = np.cumsum(lens)
    sizes = lens + PAY
    sizes[2] += delta
    mo = np.zeros(6, dtype=np.uint64)
    mo[1:] = np.cumsum(sizes)
    mo += 3
    src = rng.integers(0, 256, size=int(so[-1]), dtype=np.uint8)
    crcs = [_stream_crc((src[int(a):int(b)].tobytes(),)) for a, b in zip(so[:-1], so[1:])]
    d = torch.full((int(mo[-1]) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.zeros(src.size + 64, dtype=torch.uint8, device="cuda")
    s[:src.size].copy_(torch.from_numpy(src))
    sod, mod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (so, mo))
    # (the host check refuses the table outright when both copies are given)
    with pytest.raises(gpu.GpuChecksumError):
        gpu.pack_messages(s, sod, d, mod, src_offsets_host=so, offsets_host=mo)
    status = gpu.pack_messages(s, sod, d, mod)
    assert status.cpu().tolist() == [0, 0, 1, 0, 0]
    want = _expected_dst(src, so, mo, crcs, int(mo[-1]) + 32, skip=(2,))
    assert np.array_equal(d.cpu().numpy(), want)


def test_pack_host_checks(gpu):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    so = np.array([0, 100], dtype=np.uint64)
    mo = np.array([50, 170], dtype=np.uint64)
    sod, mod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (so, mo))
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.pack_messages(buf, sod, buf, mod, src_offsets_host=so, offsets_host=mo)
    with pytest.raises(gpu.GpuChecksumError):
        gpu.pack_messages(buf, sod, buf[2048:], mod, payload_offset=18)  # hash overlaps payload
    with pytest.raises(gpu.GpuChecksumError):
        gpu.seal_messages(buf, mod, method="crc64")
    with pytest.raises(gpu.GpuChecksumError):
        gpu.seal_core_headers(buf, mod, method="crc32c")


# ---- core headers ----
CRC16_VARIANTS = ["crc16-arc", "crc16-ibm-3740", "crc16-xmodem", "crc16-kermit", "crc16-umts", "crc16-t10-dif"]


@pytest.mark.parametrize("variant", CRC16_VARIANTS)
@pytest.mark.parametrize("kind", ["request", "response"])
def test_seal_core_headers(gpu, kind, variant, monkeypatch):
    import torch
    monkeypatch.setenv("MCHECKSUM_CRC16_VARIANT", variant)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "core_headers.json")))
    rng = np.random.default_rng(3)
    hash_at = 12 if kind == "request" else 4
    want_msgs, blank_msgs = [], []
    for e in g[kind]:
        wire = bytes.fromhex(e["wire_fields"]) + struct.pack(">H", int(e[variant], 16))
        assert len(wire) == hash_at + 2 == e["hash_offset"] + 2
        body = rng.integers(0, 256, size=16 - len(wire) + int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        want_msgs.append(wire + body)
        blank_msgs.append(wire[:hash_at] + b"\xff\xff" + body)
    short = rng.integers(0, 256, size=15, dtype=np.uint8).tobytes()
    want_msgs.append(short)
    blank_msgs.append(short)
    off = np.zeros(len(want_msgs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in want_msgs])
    tail = b"\x5c" * 64
    want = np.frombuffer(b"".join(want_msgs) + tail, dtype=np.uint8)
    t = torch.from_numpy(np.frombuffer(b"".join(blank_msgs) + tail, dtype=np.uint8).copy()).cuda()
    offs = torch.from_numpy(off.astype(np.int64)).cuda()
    status = gpu.seal_core_headers(t, offs, kind=kind, offsets_host=off)
    assert np.array_equal(t.cpu().numpy(), want)
    n = len(want_msgs) - 1
    assert status.cpu().tolist() == [0] * n + [1]
    vstatus, mism = gpu.verify_core_headers(t, offs[:n + 1].contiguous(), kind=kind)
    assert int(mism.item()) == 0 and int(vstatus.sum().item()) == 0


# ---- graph ----
def test_graph_pack_seal_verify(gpu):
    """pack_messages -> seal_core_headers -> verify_messages captured on one
    stream; each replay packs the source's current bytes."""
    import torch
    gpu.prepare("crc32c")
    gpu.prepare("crc16")
    rng = np.random.default_rng(21)
    lens = rng.integers(0, 3000, 1500)  # > 1024 messages: the throughput kernels, on the static split
    lens[:3] = (0, 70000, 5)
    so = np.zeros(len(lens) + 1, dtype=np.uint64)
    so[1:] = np.cumsum(lens)
    mo = np.zeros(len(lens) + 1, dtype=np.uint64)
    mo[1:] = np.cumsum(lens + PAY)
    fills = [rng.integers(0, 256, size=int(so[-1]), dtype=np.uint8) for _ in range(2)]
    src = torch.zeros(int(so[-1]) + 64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(int(mo[-1]), dtype=torch.uint8, device="cuda")
    sod, mod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (so, mo))
    n = len(lens)
    pstat = torch.ones(n, dtype=torch.uint8, device="cuda")
    hstat = torch.ones(n, dtype=torch.uint8, device="cuda")
    vstat = torch.ones(n, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.pack_messages(src, sod, dst, mod, status=pstat)
        gpu.seal_core_headers(dst, mod, status=hstat)
        gpu.verify_messages(dst, mod, status=vstat, mismatches=mism)
    torch.cuda.synchronize()
    for fill in fills:
        with torch.cuda.stream(s):
            src[:fill.size].copy_(torch.from_numpy(fill))
            for st in (pstat, hstat, vstat):
                st.fill_(1)
            mism.zero_()
            g.replay()
        s.synchronize()
        got = dst.cpu().numpy()
        crcs = [_stream_crc((fill[int(a):int(b)].tobytes(),)) for a, b in zip(so[:-1], so[1:])]
        for i in range(n):
            a, b = int(mo[i]), int(mo[i + 1])
            assert got[a + CORE_HDR:a + PAY].tobytes() == struct.pack(">I", crcs[i]), i
            assert np.array_equal(got[a + PAY:b], fill[int(so[i]):int(so[i + 1])]), i
        assert int(mism.item()) == 0
        assert int(pstat.sum().item()) == 0 and int(hstat.sum().item()) == 0 and int(vstat.sum().item()) == 0
        hs, hm = gpu.verify_core_headers(dst, mod)
        assert int(hm.item()) == 0 and int(hs.sum().item()) == 0


# ---- fail closed ----
def test_seal_fault_fails_closed(gpu, sealed_batch, monkeypatch):
    """The fault-injection build in its give-up mode (a wave drops one unit, as
    one whose bounded wait timed out would; no stall): the error word gets 1,
    some status reads 1, and every message with status 0 carries its hash."""
    import torch
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    L = ctypes.CDLL(QLIB)
    c = ctypes
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    L.mchecksum_gpu_seal_messages.argtypes = [c.c_char_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t,
                                              c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_set_error_word.argtypes = [c.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = c.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    monkeypatch.delenv("MCHECKSUM_GPU_QFAULT_MODE", raising=False)  # the give-up, not a stall
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", "0")
    L.mchecksum_gpu_reload_settings()
    try:
        want, blank, off = sealed_batch
        # the 700 messages three times over: > 1024, so the launch takes the work queue
        reps, nb = 3, int(off[-1])
        table = np.concatenate([off[:-1] + np.uint64(r * nb) for r in range(reps)] + [[np.uint64(reps * nb)]])
        table = table.astype(np.uint64)
        n = len(table) - 1
        t = torch.from_numpy(np.concatenate([blank[:nb]] * reps + [blank[nb:]])).cuda()
        offs = torch.from_numpy(table.astype(np.int64)).cuda()
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")  # stale "sealed" everywhere
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        faults0 = L.mchecksum_gpu_queue_faults()
        assert L.mchecksum_gpu_prepare(b"crc32c") == 0
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_seal_messages(b"crc32c", t.data_ptr(), offs.data_ptr(), n, PAY, CORE_HDR,
                                               status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        st = status.cpu().numpy()
        assert set(np.unique(st).tolist()) <= {0, 1} and int(st.sum()) >= 1
        got = t.cpu().numpy()
        slots = _slots(table).reshape(-1, 4)
        full = np.concatenate([want[:nb]] * reps)
        ok = np.all(got[slots] == full[slots], axis=1)
        assert np.all(ok[st == 0]), "a message reads as sealed without its hash"
        assert int((~ok).sum()) <= 1  # only the dropped unit went unsealed
        # nothing but hash slots was written
        got[slots.ravel()] = 0
        ref = np.concatenate([blank[:nb]] * reps + [blank[nb:]])
        ref[slots.ravel()] = 0
        assert np.array_equal(got, ref)
    finally:
        monkeypatch.undo()
        L.mchecksum_gpu_reload_settings()


def test_pack_payload_past_2_gib(gpu):
    """A payload of more than 2^31 bytes takes the 64-bit-length loop
    (payload32_generic), which stores by the same rule; between two small
    neighbours, source and destination misaligned by an odd number of bytes."""
    import torch

    from mercury_amd import _lib
    big = (1 << 31) + 4096 * 3 + 5
    lens = np.array([100, big, 4097])
    so = np.zeros(4, dtype=np.uint64)
    so[1:] = np.cumsum(lens)
    so += 7
    mo = np.zeros(4, dtype=np.uint64)
    mo[1:] = np.cumsum(lens + PAY)
    mo += 16
    src = torch.empty(int(so[-1]) + 64, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(src, 0xB17)
    dst = torch.full((int(mo[-1]) + 48,), 0xEE, dtype=torch.uint8, device="cuda")
    sod, mod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (so, mo))
    status = gpu.pack_messages(src, sod, dst, mod, src_offsets_host=so, offsets_host=mo)
    assert status.cpu().tolist() == [0, 0, 0]
    # the streaming API over the source bytes, in place (no 2 GiB Python copies)
    host = src.cpu().numpy()
    L = _lib.load_library()
    for i in range(3):
        a, b = int(so[i]), int(so[i + 1])
        obj, val = ctypes.c_void_p(), ctypes.c_uint32(0)
        assert L.mchecksum_init(b"crc32c", ctypes.byref(obj)) == 0
        assert L.mchecksum_update(obj, host.ctypes.data + a, b - a) == 0
        assert L.mchecksum_get(obj, ctypes.byref(val), 4, 1) == 0
        L.mchecksum_destroy(obj)
        m = int(mo[i])
        assert dst[m + CORE_HDR:m + PAY].cpu().numpy().tobytes() == struct.pack(">I", val.value), i
        assert torch.equal(dst[m + PAY:int(mo[i + 1])], src[a:b]), i
        assert bool((dst[m:m + CORE_HDR] == 0xEE).all()), i
    assert bool((dst[:int(mo[0])] == 0xEE).all()) and bool((dst[int(mo[-1]):] == 0xEE).all())
    vstatus, mism = gpu.verify_messages(dst, mod, offsets_host=mo)
    assert int(mism.item()) == 0 and int(vstatus.sum().item()) == 0
