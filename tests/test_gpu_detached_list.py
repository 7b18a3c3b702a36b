"""The detached calls with both sides by address list (include/mchecksum_gpu.h:
mchecksum_gpu_verify_detached_message_list, _seal_detached_message_list,
_state_verify_message_list, _state_seal_message_list) on the GPU.

Layout under test: the payloads of a batch are spread over three separate torch
allocations plus five allocations that hold one payload each (the
per-handle extra buffers), the eager messages over two other allocations, and
both lists are handed over in an order shuffled across the buffers.  Neighbours
in a buffer are 0..37 bytes apart; payload starts and slot positions fall at
every residue mod 16 (so some slots straddle a 16-byte granule); every buffer
begins and ends with guard bytes.  Gaps and guards hold a non-zero pattern: a
seal must leave it intact (whole buffers are compared), and a verify that
hashed any of it would get another CRC.  Half the empty payloads and every
message of length 0 have a NULL address.

Two oracles.  The expected statuses and bytes come from the rules written out
here (`model_*`) over the live oracle's CRCs; and the same bytes laid
contiguously go through the table calls (verify_detached_messages,
seal_detached_messages), which must give the same statuses, mismatch count and
bytes.  The bar is bit-exact.

Payloads of 2 GiB and more are not run here: that branch (payload32_generic
behind `n < 2^31`) is the table form's code, instantiated unchanged, and the
list form adds nothing to it but the address."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HASH = 16
# payload lengths: the smallest at which the payload loop differs (empty, under a word, under and over a 16-byte
# piece, around one 1 KiB step, several steps, more than the 8-deep load ring holds), and one above 1 MiB
PLENS = (0, 1, 3, 15, 16, 17, 1023, 1024, 1025, 4096, 65536 + 3)
BIG = (1 << 20) + 5
OWN = (17, 1025, 4096, 65536 + 3, BIG)   # payloads that get an allocation of their own
ARMS = [("1", None), ("0", None), ("0", "1")]  # light, full, non-temporal
NPBUF, NMBUF = 3, 2
GUARD = 48   # pattern bytes kept before the first and behind the last entry of a buffer
# RPC messages of the end-to-end flow (a request: flags at 10, HG_CORE_MORE_DATA = bit 0)
RPC_PAY, RPC_FLAGS_AT, RPC_OK, RPC_DEFERRED = 20, 10, 0, 4


def pattern(n, k=0):
    """The gap and guard bytes: never zero, so hashing one changes a CRC."""
    return ((np.arange(n, dtype=np.int64) * 7 + 13 + k) % 251 + 1).astype(np.uint8)


def _be32(v):
    return np.frombuffer(struct.pack(">I", v), dtype=np.uint8)


def model_seal(m, crc, hash_off):
    """One eager message (a uint8 array, changed in place) and its payload's CRC; returns the status."""
    if m.size < hash_off + 4:
        return 1
    m[hash_off:hash_off + 4] = _be32(crc)
    return 0


def model_verify(m, crc, hash_off):
    if m.size < hash_off + 4:
        return 1
    return 0 if struct.unpack(">I", bytes(m[hash_off:hash_off + 4]))[0] == crc else 1


class Batch:
    """Host side of one batch, read-only.  In LIST order: `N`, `L` the payloads'
    and messages' lengths; `pay` the payloads as the sender holds them, `blank`
    its messages (slots random), `sealed` the model's seal of them; `rpay`,
    `rmsg` what the receiver finds -- sealed, then the plants; `pwhere[i]`,
    `mwhere[i]` = (buffer, start), ("own",) or None for a NULL address."""


def _place(rng, idx, sizes, nbuf, stride, null):
    """Entries idx over nbuf buffers: entry i goes to buffer (i * stride + 1) % nbuf -- neighbours in the list are
    not neighbours in memory --, inside a buffer in an order of its own, 0..37 bytes apart, and the starts run
    through every residue mod 16.  Returns (where, buffer sizes)."""
    where, buf_size, turn = {}, [], 0
    for k in range(nbuf):
        mine = [i for i in idx if (i * stride + 1) % nbuf == k]
        mine = [mine[j] for j in rng.permutation(len(mine))]
        at = GUARD + k
        for i in mine:
            if i in null:
                where[i] = None
                continue
            at += (turn - at) % 16 + 16 * int(rng.integers(0, 2))   # 0..31 <= 37, and the start's residue is turn's
            turn = (turn + 1) % 16
            where[i] = (k, at)
            at += int(sizes[i])
        buf_size.append(at + GUARD)
    return where, buf_size


def make_batch(O, count=None, hash_off=HASH, seed=0):
    rng = np.random.default_rng(20261021 + seed)
    b = Batch()
    b.hash = hash_off
    if count is None:
        # nine entries per payload length: j = 0 gets a payload bit flipped, j = 1 a slot bit, j = 3 has no slot,
        # j = 4 no message at all; every empty payload keeps a good slot
        Ls = [52, hash_off + 4, 52, hash_off + 3, 0, 52, hash_off + 4, 52, 52]
        ent = [(N, Ls[j] if N else (52, hash_off + 4)[j % 2], j) for N in PLENS for j in range(9)] + [(BIG, 52, 8)]
    else:
        Ls = [52, hash_off + 4, 52, hash_off + 3, 52, 0, 52, 52]
        # (of every 24 entries one gets a payload bit flipped and one a slot bit; of every 40 one payload is empty)
        ent = [(0 if i % 40 == 7 else int(rng.integers(1, 600)), Ls[i % 8], i % 8 + (2 if i % 24 >= 8 else 0))
               for i in range(count)]
    ent = [ent[k] for k in rng.permutation(len(ent))]   # list position -> entry: the lists are shuffled
    n = b.n = len(ent)
    b.N = np.array([e[0] for e in ent], dtype=np.int64)
    b.L = np.array([e[1] for e in ent], dtype=np.int64)
    slot = b.L >= hash_off + 4
    b.flip_payload = [i for i in range(n) if ent[i][2] == 0 and b.N[i] > 0 and slot[i]]
    b.flip_slot = [i for i in range(n) if ent[i][2] == 1 and b.N[i] > 0 and slot[i]]
    b.own = [i for i in range(n) if count is None and ent[i][2] == 8 and b.N[i] in OWN]
    null_pay = {i for i in range(n) if b.N[i] == 0 and i % 2 == 0}
    b.pwhere, b.pbuf_size = _place(rng, [i for i in range(n) if i not in b.own], b.N, NPBUF, 5, null_pay)
    for i in b.own:
        b.pwhere[i] = ("own",)
    b.mwhere, b.mbuf_size = _place(rng, list(range(n)), b.L, NMBUF, 3, {i for i in range(n) if b.L[i] == 0})
    b.pay = [rng.integers(0, 256, size=int(s), dtype=np.uint8) for s in b.N]
    b.blank = [rng.integers(0, 256, size=int(s), dtype=np.uint8) for s in b.L]
    b.crc = [O.crc("crc32c", p) for p in b.pay]
    b.sealed = [m.copy() for m in b.blank]
    b.sstat = np.array([model_seal(m, c, hash_off) for m, c in zip(b.sealed, b.crc)], dtype=np.uint8)
    # the receiver's batch: sealed, then one flipped bit per plant, each in an entry of its own
    b.rpay, b.rmsg, b.rcrc = [p.copy() for p in b.pay], [m.copy() for m in b.sealed], list(b.crc)
    for i in b.flip_payload:
        b.rpay[i][(977 * (i + 1)) % b.N[i]] ^= 1 << (i % 8)
        b.rcrc[i] = O.crc("crc32c", b.rpay[i])
    for i in b.flip_slot:
        b.rmsg[i][hash_off + i % 4] ^= 1 << (i % 8)
    b.vstat = np.array([model_verify(m, c, hash_off) for m, c in zip(b.rmsg, b.rcrc)], dtype=np.uint8)
    planted = set(b.flip_payload) | set(b.flip_slot)
    assert np.array_equal(b.vstat, np.array([not slot[i] or i in planted for i in range(n)], dtype=np.uint8))
    b.empty_good = [i for i in range(n) if b.N[i] == 0 and b.vstat[i] == 0]
    # by construction: at least 8 of each plant
    assert min(len(b.flip_payload), len(b.flip_slot), int((~slot).sum()), len(b.empty_good)) >= 8
    if count is None:
        assert len(b.own) == 5 and any(b.N[i] == BIG for i in b.own)
        assert {w[1] % 16 for i, w in b.pwhere.items() if w and w[0] != "own" and b.N[i]} == set(range(16))
        assert {(w[1] + hash_off) % 16 for i, w in b.mwhere.items() if w and slot[i]} == set(range(16))
        assert any(w is None for w in b.pwhere.values()) and any(w is None for w in b.mwhere.values())
    return b


_cache = {}


def batch_of(O, count=None, hash_off=HASH):
    if (count, hash_off) not in _cache:
        _cache[count, hash_off] = make_batch(O, count, hash_off)
    return _cache[count, hash_off]


def scatter(where, buf_size, items, k0=0):
    """The host buffers with `items` at their places, the pattern everywhere else."""
    bufs = [pattern(s, k + k0) for k, s in enumerate(buf_size)]
    for i, m in enumerate(items):
        w = where[i]
        if w and w[0] != "own":
            bufs[w[0]][w[1]:w[1] + m.size] = m
    return bufs


def contiguous(items):
    """The same bytes laid end to end at an odd base, in list order: (bytes, table)."""
    t = np.zeros(len(items) + 1, dtype=np.uint64)
    t[1:] = np.cumsum([m.size for m in items])
    t += np.uint64(3)
    return np.concatenate([pattern(3)] + list(items) + [np.zeros(16, dtype=np.uint8)]), t


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _table(tab):
    import torch
    return torch.from_numpy(np.asarray(tab).astype(np.uint64).view(np.int64).copy()).cuda()


class Side:
    """One side of a call on the device: the buffers, the allocations of single
    entries, and the (addr, len) pair over them, with host copies."""


def device_side(gpu, where, hbufs, items):
    import torch
    s = Side()
    s.dev = [_dev(h) for h in hbufs]
    assert len({t.data_ptr() for t in s.dev}) == len(hbufs)
    s.own, parts, null = {}, [], []
    for i, m in enumerate(items):
        w = where[i]
        if w is None:
            parts.append((s.dev[0], 0, 0))
            null.append(i)
        elif w[0] == "own":
            s.own[i] = _dev(m)          # an allocation of exactly the payload's bytes
            parts.append((s.own[i], 0, m.size))
        else:
            parts.append((s.dev[w[0]], w[1], m.size))
    s.addr, s.len, s.ah, s.lh = gpu.rpc_message_list(parts, with_host=True)
    if null:
        s.ah[null] = 0                  # a slotless message, an empty payload: a NULL address
        s.addr = _table(s.ah)
    assert s.addr.dtype == s.len.dtype == torch.int64 and s.addr.numel() == s.len.numel() == len(items)
    assert np.any(np.diff(s.ah.astype(np.int64)) < 0), "the list is in address order"
    s.parts = parts
    return s


def sides(gpu, b, msgs, pays):
    m = device_side(gpu, b.mwhere, scatter(b.mwhere, b.mbuf_size, msgs, 3), msgs)
    p = device_side(gpu, b.pwhere, scatter(b.pwhere, b.pbuf_size, pays), pays)
    return m, p


def same_buffers(side, want, what):
    for k, w in enumerate(want):
        bad = np.nonzero(side.dev[k].cpu().numpy() != w)[0]
        assert bad.size == 0, f"{what}: buffer {k}: {bad.size} bytes differ, first at {bad[:4]}"


def _force(monkeypatch, light, nt):
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)


def check_verify(gpu, b):
    m, p = sides(gpu, b, b.rmsg, b.rpay)
    st, mm = gpu.verify_detached_message_list(m.addr, m.len, p.addr, p.len, hash_offset=b.hash, addr_host=m.ah,
                                              len_host=m.lh, payload_addr_host=p.ah, payload_len_host=p.lh)
    (cm, mo), (cp, po) = contiguous(b.rmsg), contiguous(b.rpay)
    tst, tmm = gpu.verify_detached_messages(_dev(cm), _table(mo), _dev(cp), _table(po), hash_offset=b.hash,
                                            offsets_host=mo, payload_offsets_host=po)
    got = st.cpu().numpy()
    assert np.array_equal(got, b.vstat), np.nonzero(got != b.vstat)[0][:8]
    assert np.array_equal(got, tst.cpu().numpy())
    assert int(mm.item()) == int(b.vstat.sum()) == int(tmm.item())
    same_buffers(m, scatter(b.mwhere, b.mbuf_size, b.rmsg, 3), "a verify wrote the messages")
    same_buffers(p, scatter(b.pwhere, b.pbuf_size, b.rpay), "a verify wrote the payloads")
    return m, p, got


def check_seal(gpu, b):
    m, p = sides(gpu, b, b.blank, b.pay)
    st = gpu.seal_detached_message_list(m.addr, m.len, p.addr, p.len, hash_offset=b.hash, addr_host=m.ah,
                                        len_host=m.lh, payload_addr_host=p.ah, payload_len_host=p.lh)
    assert np.array_equal(st.cpu().numpy(), b.sstat)
    # whole buffers against the model's: every gap and guard byte among them
    same_buffers(m, scatter(b.mwhere, b.mbuf_size, b.sealed, 3), "seal")
    same_buffers(p, scatter(b.pwhere, b.pbuf_size, b.pay), "a seal wrote the payloads")
    (cm, mo), (cp, po) = contiguous(b.blank), contiguous(b.pay)
    cdev = _dev(cm)
    tst = gpu.seal_detached_messages(cdev, _table(mo), _dev(cp), _table(po), hash_offset=b.hash, offsets_host=mo,
                                     payload_offsets_host=po)
    assert np.array_equal(tst.cpu().numpy(), b.sstat)
    assert np.array_equal(cdev.cpu().numpy(), contiguous(b.sealed)[0])
    # the round trip: what was sealed verifies, through the same lists
    vst, vmm = gpu.verify_detached_message_list(m.addr, m.len, p.addr, p.len, hash_offset=b.hash)
    assert np.array_equal(vst.cpu().numpy(), b.sstat) and int(vmm.item()) == int(b.sstat.sum())
    return m, p


@pytest.mark.parametrize("light,nt", ARMS)
@pytest.mark.parametrize("hash_off", [HASH, 13])
def test_verify(gpu, oracle_mod, hash_off, light, nt, monkeypatch):
    """Sealed entries with the plants -- one payload bit, one slot bit, no
    slot (hash_offset + 3 bytes, and no message at all), empty payloads with a
    good slot: statuses and the mismatch count equal the model's and the table
    call's, and nothing is written."""
    _force(monkeypatch, light, nt)
    check_verify(gpu, batch_of(oracle_mod, None, hash_off))


@pytest.mark.parametrize("light,nt", ARMS)
@pytest.mark.parametrize("hash_off", [HASH, 13])
def test_seal_and_round_trip(gpu, oracle_mod, hash_off, light, nt, monkeypatch):
    """Seal through the lists: the message buffers equal the model's byte for
    byte (4 bytes per entry with a slot, the pattern intact), the table call
    writes the same bytes, and a verify of the result passes wherever a slot
    was written."""
    _force(monkeypatch, light, nt)
    check_seal(gpu, batch_of(oracle_mod, None, hash_off))


@pytest.mark.parametrize("count", [1024, 1025])
def test_default_rules(gpu, oracle_mod, count):
    """1,024 entries: the largest count of the light layout; 1,025: the
    smallest that leaves it (plan_offsets: light up to kRecvQueueBatch) and so
    takes the work queue.  Small payloads; nothing is forced: this is the plan a
    caller gets."""
    b = batch_of(oracle_mod, count)
    assert b.n == count
    check_verify(gpu, b)
    check_seal(gpu, b)


def test_graph_replay(gpu, oracle_mod):
    """One captured verify after prepare.  A replay reads the arrays' current
    contents: all four rewritten in place -- entry i names entry n - 1 - i, and
    every payload of two bytes or more is one byte shorter, another CRC --, the
    same graph gives the eager call's and the model's statuses for those."""
    import torch
    O = oracle_mod
    gpu.prepare("crc32c")
    b = batch_of(O)
    m, p = sides(gpu, b, b.rmsg, b.rpay)
    n = b.n
    status = torch.ones(n, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.verify_detached_message_list(m.addr, m.len, p.addr, p.len, status=status, mismatches=mism)
    torch.cuda.synchronize()
    rev = np.arange(n)[::-1]
    plh2 = p.lh[rev].copy()
    plh2[plh2 >= 2] -= np.uint64(1)
    first = (m.ah.copy(), m.lh.copy(), p.ah.copy(), p.lh.copy())
    second = (m.ah[rev].copy(), m.lh[rev].copy(), p.ah[rev].copy(), plh2)
    for r, arrays in enumerate((first, second)):
        with torch.cuda.stream(s):
            for t, a in zip((m.addr, m.len, p.addr, p.len), arrays):
                t.copy_(torch.from_numpy(a.view(np.int64)))
            status.fill_(1)
            mism.zero_()
            g.replay()
        s.synchronize()
        got, gmm = status.cpu().numpy(), int(mism.item())
        est, emm = gpu.verify_detached_message_list(m.addr, m.len, p.addr, p.len)
        assert np.array_equal(got, est.cpu().numpy()) and gmm == int(emm.item()), r
        if r == 0:
            assert np.array_equal(got, b.vstat)
        else:
            want = np.array([model_verify(b.rmsg[j], O.crc("crc32c", b.rpay[j][:int(plh2[i])]), b.hash)
                             for i, j in enumerate(rev)], dtype=np.uint8)
            assert np.array_equal(got, want) and gmm == int(want.sum()) and not np.array_equal(got, b.vstat[rev])


def test_streamed_route(gpu, oracle_mod):
    """state_init, update_segments over the payloads' own addresses, then
    state_verify_message_list / state_seal_message_list over the messages':
    statuses, the count and every written byte equal the one-shot calls'."""
    b = batch_of(oracle_mod)

    def states(p):
        segs = [t[start:start + size] for t, start, size in p.parts]   # the same addresses, one segment per payload
        sb = gpu.SegmentBatch(segs, obj_first=np.arange(b.n + 1))
        return sb.update("crc32c", gpu.state_init("crc32c", b.n))

    m, p, one_shot = check_verify(gpu, b)
    st, mm = gpu.state_verify_message_list(states(p), m.addr, m.len, hash_offset=b.hash, addr_host=m.ah, len_host=m.lh)
    assert np.array_equal(st.cpu().numpy(), one_shot) and int(mm.item()) == int(one_shot.sum())
    same_buffers(m, scatter(b.mwhere, b.mbuf_size, b.rmsg, 3), "a state verify wrote the messages")
    m, p = sides(gpu, b, b.blank, b.pay)
    st = gpu.state_seal_message_list(states(p), m.addr, m.len, hash_offset=b.hash, addr_host=m.ah, len_host=m.lh)
    assert np.array_equal(st.cpu().numpy(), b.sstat)
    same_buffers(m, scatter(b.mwhere, b.mbuf_size, b.sealed, 3), "state seal")


def test_flow_end_to_end(gpu):
    """a mixed drain goes through verify_rpc_message_list,
    the host takes the DEFERRED indices, and the sub-list built from the same
    host arrays goes to verify_detached_message_list with the payloads in
    allocations of their own -- sealed by the same two calls on the sender."""
    import torch
    rng = np.random.default_rng(42)
    n = 40
    more = np.zeros(n, dtype=bool)
    more[rng.choice(n, size=12, replace=False)] = True
    msgs = []
    for i in range(n):
        h = rng.integers(0, 256, size=52 if more[i] else RPC_PAY + int(rng.integers(0, 300)), dtype=np.uint8)
        h[RPC_FLAGS_AT] = (h[RPC_FLAGS_AT] & 0xFE) | int(more[i])
        msgs.append(h)
    where, at = [], [GUARD, GUARD]
    for i, h in enumerate(msgs):                # two receive buffers, gaps between the messages
        k = i % 2
        at[k] += int(rng.integers(0, 38))
        where.append((k, at[k]))
        at[k] += h.size
    hbufs = [pattern(a + GUARD, k) for k, a in enumerate(at)]
    for (k, a), h in zip(where, msgs):
        hbufs[k][a:a + h.size] = h
    dev = [_dev(h) for h in hbufs]
    addr, lens, ah, lh = gpu.rpc_message_list([(dev[k], a, h.size) for (k, a), h in zip(where, msgs)], with_host=True)
    idx = np.nonzero(more)[0]
    extra = [torch.from_numpy(rng.integers(0, 256, size=int(s), dtype=np.uint8)).cuda()
             for s in rng.integers(1, 70000, size=idx.size)]   # one allocation per handle
    paddr, plen = gpu.rpc_message_list([(t, 0, t.numel()) for t in extra])
    # the sender: header hashes of all, payload hashes of the eager ones; then the detached slots by sub-list
    sst = gpu.seal_rpc_message_list(addr, lens, addr_host=ah, len_host=lh).cpu().numpy()
    assert np.array_equal(sst, np.where(more, RPC_DEFERRED, RPC_OK))
    sub_addr, sub_len = _table(ah[idx]), _table(lh[idx])
    dst = gpu.seal_detached_message_list(sub_addr, sub_len, paddr, plen, addr_host=ah[idx], len_host=lh[idx])
    assert not dst.cpu().numpy().any()
    # the receiver
    vst, _ = gpu.verify_rpc_message_list(addr, lens, addr_host=ah, len_host=lh)
    vst = vst.cpu().numpy()
    deferred = np.nonzero(vst == RPC_DEFERRED)[0]          # on the host: it issues the bulk pulls
    assert np.array_equal(deferred, idx) and np.all(vst[~more] == RPC_OK)
    st, mm = gpu.verify_detached_message_list(_table(ah[deferred]), _table(lh[deferred]), paddr, plen)
    assert not st.cpu().numpy().any() and int(mm.item()) == 0
    extra[5][extra[5].numel() // 2] ^= 0x20
    st, mm = gpu.verify_detached_message_list(_table(ah[deferred]), _table(lh[deferred]), paddr, plen)
    assert np.array_equal(st.cpu().numpy(), np.arange(idx.size) == 5) and int(mm.item()) == 1


def test_empty_batch_and_wrapper_checks(gpu):
    """count == 0 with NULL arrays is a valid call of all four; with host copies
    the wrappers refuse slots that overlap one another (a seal's only) and
    arrays that do not match."""
    import torch
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    assert e.data_ptr() == 0
    st, mm = gpu.verify_detached_message_list(e, e, e, e)
    assert st.numel() == 0 and int(mm.item()) == 0
    assert gpu.seal_detached_message_list(e, e, e, e).numel() == 0
    state = gpu.state_init("crc32c", 0)
    st, mm = gpu.state_verify_message_list(state, e, e)
    assert st.numel() == 0 and int(mm.item()) == 0
    assert gpu.state_seal_message_list(state, e, e).numel() == 0
    L = gpu._lib()
    assert L.mchecksum_gpu_verify_detached_message_list(b"crc32c", None, None, 16, None, None, 0, None, None, None) == 0
    assert L.mchecksum_gpu_seal_detached_message_list(b"crc32c", None, None, 16, None, None, 0, None, None) == 0
    assert L.mchecksum_gpu_state_verify_message_list(b"crc32c", None, 0, None, None, 16, None, None, None) == 0
    assert L.mchecksum_gpu_state_seal_message_list(b"crc32c", None, 0, None, None, 16, None, None) == 0
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    addr, lens, ah, lh = gpu.rpc_message_list([(buf, 0, 100), (buf, 2, 100)], with_host=True)
    paddr, plen = gpu.rpc_message_list([(buf, 1000, 10), (buf, 2000, 10)])
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.seal_detached_message_list(addr, lens, paddr, plen, addr_host=ah, len_host=lh)
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.state_seal_message_list(gpu.state_init("crc32c", 2), addr, lens, addr_host=ah, len_host=lh)
    gpu.verify_detached_message_list(addr, lens, paddr, plen, addr_host=ah, len_host=lh)   # (read only: they may)
    with pytest.raises(gpu.GpuChecksumError, match="at least 2 elements"):
        gpu.verify_detached_message_list(addr, lens, paddr[:1], plen[:1])
    with pytest.raises(gpu.GpuChecksumError, match="hash_offset"):
        gpu.verify_detached_message_list(addr, lens, paddr, plen, hash_offset=(1 << 30) + 1)
