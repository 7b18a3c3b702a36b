"""Overflow RPCs on the GPU (include/mchecksum_gpu.h): the payload lies outside
its message -- Mercury's extra buffer, pulled by bulk -- and the hash that
covers it in the short eager message (src/mercury.c:699-707, 715-776, 544-573).
verify_detached_messages and seal_detached_messages hash the payloads where
they lie; state_verify_messages and state_seal_messages end a transfer hashed
in stages.  Every value is compared with the live oracle's, every byte the
calls must not write with its value before the call.
"""
import ctypes
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLIB = os.path.join(ROOT, "build", "libmchecksum_qfault.so")
HASH = 16
LENS = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 4096, 4097, 65541)
COUNT = 193
RUNTS = {7: 19, 60: 19, 131: 19, 100: 0}  # messages too short for their slot
PAY_BASE, MSG_BASE = 3, 5                 # odd: nothing starts aligned by construction
LAYOUTS = [("0", None), ("1", None), ("0", "1")]  # full, light, non-temporal


class Batch:
    """The ragged batch of the issue, on the host, read-only: `pay` the payload
    buffer with its table `po`, `blank` the eager messages (random bytes, the
    slot included) with their table `mo`, `crc` the oracle's values, `sealed`
    the messages as a correct seal leaves them."""


def make_batch(oracle_mod):
    rng = np.random.default_rng(20261020)
    b = Batch()
    lens = np.array([LENS[i % len(LENS)] for i in range(COUNT)])
    b.po = np.zeros(COUNT + 1, dtype=np.uint64)
    b.po[1:] = np.cumsum(lens)
    b.po += np.uint64(PAY_BASE)
    assert set((b.po[:-1][lens > 0] % 16).tolist()) == set(range(16)), "payload starts miss a residue mod 16"
    b.pay = rng.integers(0, 256, size=int(b.po[-1]) + 7, dtype=np.uint8)
    sizes = rng.integers(20, 53, COUNT)
    for i, n in RUNTS.items():
        sizes[i] = n
    b.mo = np.zeros(COUNT + 1, dtype=np.uint64)
    b.mo[1:] = np.cumsum(sizes)
    b.mo += np.uint64(MSG_BASE)
    b.blank = rng.integers(0, 256, size=int(b.mo[-1]) + 9, dtype=np.uint8)
    b.short = np.zeros(COUNT, dtype=bool)
    b.short[list(RUNTS)] = True
    assert np.array_equal(b.short, sizes < HASH + 4)
    b.crc = oracle_mod.batch_offsets("crc32c", b.pay, b.po).astype(np.uint32)
    b.sealed = b.blank.copy()
    for i in np.nonzero(~b.short)[0]:
        at = int(b.mo[i]) + HASH
        b.sealed[at:at + 4] = np.frombuffer(struct.pack(">I", int(b.crc[i])), dtype=np.uint8)
    for a in (b.po, b.pay, b.mo, b.blank, b.short, b.crc, b.sealed):
        a.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def batch(oracle_mod):
    return make_batch(oracle_mod)


def _dev(a):
    """A device copy whose element 0 is 16-byte aligned (so the odd bases stay odd)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _tables(b):
    import torch
    return (torch.from_numpy(b.mo.astype(np.int64)).cuda(), torch.from_numpy(b.po.astype(np.int64)).cuda())


def _force(monkeypatch, light, nt):
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)


def _corrupt(b, msgs, pay):
    """One payload bit flipped in five messages, one hash bit in five others,
    and a byte behind the slot (descriptor bytes) in three more.  Returns the
    expected status."""
    live = [i for i in range(COUNT) if not b.short[i] and int(b.po[i + 1] - b.po[i]) > 0]
    pay_bad, hash_bad = live[3:53:10], live[5:55:10]
    desc = [i for i in live[8::10] if int(b.mo[i + 1] - b.mo[i]) > HASH + 4][:3]
    assert len(pay_bad) == len(hash_bad) == 5 and len(desc) == 3 and not set(pay_bad) & set(hash_bad)
    for k, i in enumerate(pay_bad):
        n = int(b.po[i + 1] - b.po[i])
        pay[int(b.po[i]) + (k * 977) % n] ^= 1 << (k % 8)
    for k, i in enumerate(hash_bad):
        msgs[int(b.mo[i]) + HASH + k % 4] ^= 0x80 >> k
    for i in desc:
        msgs[int(b.mo[i]) + HASH + 4] ^= 0xFF
    want = b.short.copy()
    want[pay_bad] = True
    want[hash_bad] = True
    return want.astype(np.uint8)


@pytest.mark.parametrize("light,nt", LAYOUTS)
def test_seal_then_verify(gpu, batch, light, nt, monkeypatch):
    """Every instantiation the dispatcher can pick (light, full, non-temporal x
    seal, verify) against the oracle."""
    import torch
    _force(monkeypatch, light, nt)
    b = batch
    msgs, pay = _dev(b.blank), _dev(b.pay)
    mod, pod = _tables(b)
    status = gpu.seal_detached_messages(msgs, mod, pay, pod, hash_offset=HASH, offsets_host=b.mo,
                                        payload_offsets_host=b.po)
    got = msgs.cpu().numpy()
    slots = (b.mo[:-1].astype(np.int64)[~b.short, None] + HASH + np.arange(4)[None, :])
    bad = np.nonzero(np.any(got[slots] != b.sealed[slots], axis=1))[0]
    assert bad.size == 0, f"hash slots of {bad.size} messages differ from the oracle's, first {bad[:8]}"
    assert np.array_equal(got, b.sealed), "a byte outside the hash slots changed"
    assert np.array_equal(pay.cpu().numpy(), b.pay), "the payload buffer changed"
    assert np.array_equal(status.cpu().numpy(), b.short.astype(np.uint8))
    # the receiver: clean but for the short messages, which are counted
    vstatus, mism = gpu.verify_detached_messages(msgs, mod, pay, pod, hash_offset=HASH, offsets_host=b.mo,
                                                 payload_offsets_host=b.po)
    assert np.array_equal(vstatus.cpu().numpy(), b.short.astype(np.uint8))
    assert int(mism.item()) == len(RUNTS)
    # ten corrupted messages, and descriptor bytes that no hash covers
    hm, hp = b.sealed.copy(), b.pay.copy()
    want = _corrupt(b, hm, hp)
    msgs, pay = _dev(hm), _dev(hp)
    vstatus, mism = gpu.verify_detached_messages(msgs, mod, pay, pod, hash_offset=HASH)
    assert np.array_equal(vstatus.cpu().numpy(), want)
    assert int(mism.item()) == 10 + len(RUNTS)
    none, mism = gpu.verify_detached_messages(msgs, mod, pay, pod, hash_offset=HASH, status=False)
    assert none is False and int(mism.item()) == 10 + len(RUNTS)
    vstatus, none = gpu.verify_detached_messages(msgs, mod, pay, pod, hash_offset=HASH, mismatches=False)
    assert none is False and np.array_equal(vstatus.cpu().numpy(), want)
    assert np.array_equal(msgs.cpu().numpy(), hm) and np.array_equal(pay.cpu().numpy(), hp), "a verify wrote"
    torch.cuda.synchronize()


def _stage_cuts(b, rng):
    """Two cut points per payload, anywhere in it (its ends included)."""
    n = (b.po[1:] - b.po[:-1]).astype(np.int64)
    c = np.sort(np.stack([rng.integers(0, n + 1), rng.integers(0, n + 1)]), axis=0)
    return np.stack([np.zeros_like(n), c[0], c[1], n])  # 4 x COUNT


@pytest.mark.parametrize("copy", [False, True], ids=["update_offsets", "update_copy_offsets"])
def test_streaming_route(gpu, batch, copy):
    """state_init, three stages cut at arbitrary bytes, state_seal_messages:
    the bytes seal_detached_messages writes; state_verify_messages: its
    verdicts after the same corruptions."""
    import torch
    b = batch
    rng = np.random.default_rng(77)
    cuts = _stage_cuts(b, rng)
    mod, _ = _tables(b)
    start = b.po[:-1].astype(np.int64)

    def feed(pay_host, state, dst):
        for k in range(3):
            n = cuts[k + 1] - cuts[k]
            so = np.zeros(COUNT + 1, dtype=np.int64)
            so[1:] = np.cumsum(n)
            so += 1 + k  # every stage buffer starts at another odd or even byte
            stage = np.zeros(int(so[-1]) + 16, dtype=np.uint8)
            for i in range(COUNT):
                stage[so[i]:so[i + 1]] = pay_host[start[i] + cuts[k][i]:start[i] + cuts[k + 1][i]]
            sd, sod = _dev(stage), torch.from_numpy(so).cuda()
            if copy:
                gpu.update_copy_offsets("crc32c", sd, sod, dst, torch.from_numpy(start + cuts[k]).cuda(), state)
            else:
                gpu.update_offsets("crc32c", sd, sod, state, offsets_host=so)

    state = gpu.state_init("crc32c", COUNT)
    dst = torch.zeros(b.pay.size, dtype=torch.uint8, device="cuda")
    feed(b.pay, state, dst)
    if copy:  # the stages also reassembled the payloads
        lo, hi = int(b.po[0]), int(b.po[-1])
        assert np.array_equal(dst.cpu().numpy()[lo:hi], b.pay[lo:hi])
    before = state.clone()
    msgs = _dev(b.blank)
    status = gpu.state_seal_messages(state, msgs, mod, hash_offset=HASH, offsets_host=b.mo)
    assert np.array_equal(msgs.cpu().numpy(), b.sealed), "not the bytes seal_detached_messages writes"
    assert np.array_equal(status.cpu().numpy(), b.short.astype(np.uint8))
    vstatus, mism = gpu.state_verify_messages(state, msgs, mod, hash_offset=HASH)
    assert np.array_equal(vstatus.cpu().numpy(), b.short.astype(np.uint8)) and int(mism.item()) == len(RUNTS)
    # the same corruptions, streamed
    hm, hp = b.sealed.copy(), b.pay.copy()
    want = _corrupt(b, hm, hp)
    state2 = gpu.state_init("crc32c", COUNT)
    feed(hp, state2, dst)
    msgs = _dev(hm)
    vstatus, mism = gpu.state_verify_messages(state2, msgs, mod, hash_offset=HASH, offsets_host=b.mo)
    assert np.array_equal(vstatus.cpu().numpy(), want) and int(mism.item()) == 10 + len(RUNTS)
    none, mism = gpu.state_verify_messages(state2, msgs, mod, hash_offset=HASH, status=False)
    assert none is False and int(mism.item()) == 10 + len(RUNTS)
    vstatus, none = gpu.state_verify_messages(state2, msgs, mod, hash_offset=HASH, mismatches=False)
    assert none is False and np.array_equal(vstatus.cpu().numpy(), want)
    assert np.array_equal(msgs.cpu().numpy(), hm), "a verify wrote"
    assert torch.equal(state, before), "the states changed"


def test_agrees_with_the_eager_calls(gpu, batch):
    """Payloads that also lie behind their headers: verify_detached_messages on
    (headers, a copy of the payloads) gives verify_messages' statuses."""
    import torch
    b = batch
    rng = np.random.default_rng(5)
    PAY = HASH + 4
    n = (b.po[1:] - b.po[:-1]).astype(np.int64)
    eo = np.zeros(COUNT + 1, dtype=np.uint64)
    eo[1:] = np.cumsum(n + PAY)
    eo += np.uint64(9)
    eager = rng.integers(0, 256, size=int(eo[-1]) + 16, dtype=np.uint8)
    for i in range(COUNT):
        a = int(eo[i])
        eager[a + PAY:int(eo[i + 1])] = b.pay[int(b.po[i]):int(b.po[i + 1])]
        eager[a + HASH:a + PAY] = np.frombuffer(struct.pack(">I", int(b.crc[i])), dtype=np.uint8)
    for k, i in enumerate(range(4, COUNT, 17)):  # hashes and payload bytes that do not match
        a = int(eo[i])
        eager[a + HASH + k % 4] ^= 1
        if n[i + 1]:
            eager[int(eo[i + 1]) + PAY + int(n[i + 1]) // 2] ^= 0x10
    ed, eod = _dev(eager), torch.from_numpy(eo.astype(np.int64)).cuda()
    want, wm = gpu.verify_messages(ed, eod, payload_offset=PAY, hash_offset=HASH, offsets_host=eo)
    assert 10 < int(wm.item()) < COUNT
    # the payloads copied out, byte-packed; the eager buffer serves as the headers
    copy = np.zeros(b.pay.size, dtype=np.uint8)
    for i in range(COUNT):
        copy[int(b.po[i]):int(b.po[i + 1])] = eager[int(eo[i]) + PAY:int(eo[i + 1])]
    _, pod = _tables(b)
    got, gm = gpu.verify_detached_messages(ed, eod, _dev(copy), pod, hash_offset=HASH, offsets_host=eo,
                                           payload_offsets_host=b.po)
    assert torch.equal(got, want) and int(gm.item()) == int(wm.item())


def test_graph_seal_and_verify(gpu, batch, oracle_mod):
    """A captured seal_detached + verify_detached pair on one stream: each of
    three replays seals and verifies the payloads' current bytes."""
    import torch
    gpu.prepare("crc32c")
    b = batch
    msgs, pay = _dev(b.blank), _dev(b.pay)
    mod, pod = _tables(b)
    sstat = torch.ones(COUNT, dtype=torch.uint8, device="cuda")
    vstat = torch.ones(COUNT, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.seal_detached_messages(msgs, mod, pay, pod, hash_offset=HASH, status=sstat)
        gpu.verify_detached_messages(msgs, mod, pay, pod, hash_offset=HASH, status=vstat, mismatches=mism)
    torch.cuda.synchronize()
    host = b.pay.copy()
    for r in range(3):
        host[int(b.po[0]) + r:int(b.po[-1]):97] ^= 0x21 + r  # bytes of most payloads change
        with torch.cuda.stream(s):
            pay.copy_(torch.from_numpy(host))
            msgs.copy_(torch.from_numpy(b.blank.copy()))
            sstat.fill_(1)
            vstat.fill_(1)
            mism.zero_()
            g.replay()
        s.synchronize()
        crc = oracle_mod.batch_offsets("crc32c", host, b.po).astype(np.uint32)
        got = msgs.cpu().numpy()
        for i in np.nonzero(~b.short)[0]:
            at = int(b.mo[i]) + HASH
            assert got[at:at + 4].tobytes() == struct.pack(">I", int(crc[i])), (r, i)
        assert np.array_equal(sstat.cpu().numpy(), b.short.astype(np.uint8))
        assert np.array_equal(vstat.cpu().numpy(), b.short.astype(np.uint8))
        assert int(mism.item()) == len(RUNTS)


def test_fault_fails_closed(gpu, batch, monkeypatch):
    """The fault-injection build in its give-up mode (a wave drops one unit, as
    one whose bounded wait timed out would; no stall): each call bumps the
    error word once, the verify adds `count` to its counter, and every status
    the launch could not vouch for is 1."""
    import torch
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    L = ctypes.CDLL(QLIB)
    c = ctypes
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    L.mchecksum_gpu_seal_detached_messages.argtypes = [c.c_char_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p,
                                                       c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_verify_detached_messages.argtypes = [c.c_char_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p,
                                                         c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_set_error_word.argtypes = [c.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = c.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    monkeypatch.delenv("MCHECKSUM_GPU_QFAULT_MODE", raising=False)  # the give-up, not a stall
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", "0")
    L.mchecksum_gpu_reload_settings()
    try:
        b = batch
        # the batch twelve times over: > 1024 messages, so the launch takes the work queue
        reps, npay, nmsg = 12, int(b.po[-1] - b.po[0]), int(b.mo[-1] - b.mo[0])
        po = np.concatenate([b.po[:-1] + np.uint64(r * npay) for r in range(reps)] + [[b.po[0] + np.uint64(reps * npay)]])
        mo = np.concatenate([b.mo[:-1] + np.uint64(r * nmsg) for r in range(reps)] + [[b.mo[0] + np.uint64(reps * nmsg)]])
        po, mo = po.astype(np.uint64), mo.astype(np.uint64)
        n = len(po) - 1
        assert n == reps * COUNT > 1024
        lo, hi = int(b.po[0]), int(b.po[-1])
        pay_h = np.concatenate([b.pay[:lo]] + [b.pay[lo:hi]] * reps + [np.zeros(16, dtype=np.uint8)])
        lo, hi = int(b.mo[0]), int(b.mo[-1])
        blank_h = np.concatenate([b.blank[:lo]] + [b.blank[lo:hi]] * reps + [b.blank[hi:]])
        sealed_h = np.concatenate([b.sealed[:lo]] + [b.sealed[lo:hi]] * reps + [b.sealed[hi:]])
        short = np.tile(b.short, reps)
        slots = mo[:-1].astype(np.int64)[~short, None] + HASH + np.arange(4)[None, :]
        pay, msgs = _dev(pay_h), _dev(blank_h)
        pod, mod = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (po, mo))
        stream = torch.cuda.current_stream().cuda_stream
        assert L.mchecksum_gpu_prepare(b"crc32c") == 0
        # seal: stale "sealed" everywhere
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        faults0 = L.mchecksum_gpu_queue_faults()
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_seal_detached_messages(b"crc32c", msgs.data_ptr(), mod.data_ptr(), HASH, pay.data_ptr(),
                                                        pod.data_ptr(), n, status.data_ptr(), stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        st = status.cpu().numpy()
        assert set(np.unique(st).tolist()) <= {0, 1} and np.all(st[short] == 1)
        got = msgs.cpu().numpy()
        ok = np.all(got[slots] == sealed_h[slots], axis=1)
        assert np.all(ok[st[~short] == 0]), "a message reads as sealed without its hash"
        assert int((~ok).sum()) <= 1  # only the dropped unit went unsealed
        got[slots.ravel()] = 0
        ref = blank_h.copy()
        ref[slots.ravel()] = 0
        assert np.array_equal(got, ref), "a byte outside the hash slots changed"
        # verify, on correctly sealed messages with a genuine mismatch every 7th: stale "pass" everywhere
        hm = sealed_h.copy()
        bad = np.arange(0, n, 7)
        bad = bad[~short[bad]]
        hm[mo[bad].astype(np.int64) + HASH] ^= 1
        msgs = _dev(hm)
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        word.zero_()
        faults0 = L.mchecksum_gpu_queue_faults()
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_verify_detached_messages(b"crc32c", msgs.data_ptr(), mod.data_ptr(), HASH,
                                                          pay.data_ptr(), pod.data_ptr(), n, status.data_ptr(),
                                                          mism.data_ptr(), stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        st = status.cpu().numpy()
        truth = short.copy()
        truth[bad] = True
        assert int(mism.item()) >= n, "a faulted verify must not read as clean"
        assert set(np.unique(st).tolist()) <= {0, 1}
        assert np.all(st[truth] == 1), "a real mismatch read as verified"
        # `count` once, and one more per failing message that was hashed: all of them, or all
        # but one when the dropped unit is itself a failing message (which unit is dropped, and
        # how many statuses the sweep overtook, depends on the run; neither is asserted)
        assert n + int(truth.sum()) - 1 <= int(mism.item()) <= n + int(truth.sum())
    finally:
        monkeypatch.undo()
        L.mchecksum_gpu_reload_settings()


def test_empty_batches(gpu):
    """count == 0 with NULL buffers is valid for all four calls."""
    import torch

    from mercury_amd import _lib
    L = _lib.load_library()
    s = torch.cuda.current_stream().cuda_stream
    assert L.mchecksum_gpu_verify_detached_messages(b"crc32c", None, None, HASH, None, None, 0, None, None, s) == 0
    assert L.mchecksum_gpu_seal_detached_messages(b"crc32c", None, None, HASH, None, None, 0, None, s) == 0
    assert L.mchecksum_gpu_state_verify_messages(b"crc32c", None, 0, None, None, HASH, None, None, s) == 0
    assert L.mchecksum_gpu_state_seal_messages(b"crc32c", None, 0, None, None, HASH, None, s) == 0
    # ... and through the wrappers, with one-entry tables
    e8 = torch.zeros(0, dtype=torch.uint8, device="cuda")
    t1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    st, mm = gpu.verify_detached_messages(e8, t1, e8, t1)
    assert st.numel() == 0 and int(mm.item()) == 0
    assert gpu.seal_detached_messages(e8, t1, e8, t1).numel() == 0
    state = gpu.state_init("crc32c", 0)
    st, mm = gpu.state_verify_messages(state, e8, t1)
    assert st.numel() == 0 and int(mm.item()) == 0
    assert gpu.state_seal_messages(state, e8, t1).numel() == 0
