"""The RPC message calls by address list (include/mchecksum_gpu.h:
mchecksum_gpu_verify_rpc_message_list, _seal_, _unpack_, _pack_) on the GPU.

Layout under test: the messages of a batch are spread over three separate
torch allocations, handed over in an order shuffled across the buffers, with
gaps of 0..37 bytes between neighbours and message starts at every residue
mod 16.  The gaps hold a non-zero pattern: a seal or a pack must leave it
intact (whole buffers are compared), and a verify or an unpack that hashed any
of it would get another CRC.

Two oracles.  The expected statuses and bytes come from the rules written out
here (`model_*`) over the live oracle's CRCs; and the same messages laid
contiguously go through the table calls (verify_rpc_messages, ...), which must
give the same statuses, counts and bytes.  The bar is bit-exact."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, PAYLOAD, HEADER, SHORT, DEFERRED, FAULT, MISFIT, CLASSES = range(8)
PAY, HASH = 20, 16
# payload lengths: the smallest at which the payload loop differs (empty, under a word, under and over a 16-byte
# piece, around one 1 KiB step, several steps, and more than the 8-deep load ring holds)
PLENS = (0, 1, 3, 15, 16, 17, 1023, 1024, 1025, 4096, 65536 + 3)
KINDS = ("request", "response")
FLAGS_AT = {"request": 10, "response": 1}
HASH_AT = {"request": 12, "response": 4}
ARMS = [("1", None), ("0", None), ("0", "1")]  # light, full, non-temporal
NBUF = 3
GUARD = 48   # pattern bytes kept before the first and behind the last message of a buffer
OBASE = 5    # the other side's odd base


def image(kind, h):
    """The host-order field image hg_core_header_*_proc hashes, from the 16 wire bytes."""
    if kind == "request":
        return bytes(h[0:2]) + struct.pack("<Q", struct.unpack(">Q", bytes(h[2:10]))[0]) + bytes(h[10:12])
    return bytes(h[0:2]) + struct.pack("<H", struct.unpack(">H", bytes(h[2:4]))[0])


def _be(fmt, v):
    return np.frombuffer(struct.pack(fmt, v), dtype=np.uint8)


def pattern(n, k=0):
    """The gap and guard bytes: never zero, so hashing one changes a CRC."""
    return ((np.arange(n, dtype=np.int64) * 7 + 13 + k) % 251 + 1).astype(np.uint8)


def model_seal(O, m, kind):
    """One message (a uint8 array, changed in place); returns its status."""
    L = m.size
    if L < 16:
        return SHORT
    more = bool(m[FLAGS_AT[kind]] & 1)
    if not more and L < PAY:
        return SHORT
    if not more:
        m[HASH:HASH + 4] = _be(">I", O.crc("crc32c", m[PAY:]))
    at = HASH_AT[kind]
    m[at:at + 2] = _be(">H", O.crc("crc16", image(kind, m[:16])))
    return DEFERRED if more else OK


def model_verify(O, m, kind, R=None):
    """The receiver's rule ladder; R: the destination's size of an unpack (None: a verify)."""
    L = m.size
    if L < 16:
        return SHORT
    at = HASH_AT[kind]
    if O.crc("crc16", image(kind, m[:16])) != int(m[at]) << 8 | int(m[at + 1]):
        return HEADER
    if m[FLAGS_AT[kind]] & 1:
        return DEFERRED
    if L < PAY:
        return SHORT
    if R is not None and L != PAY + R:
        return MISFIT
    return OK if O.crc("crc32c", m[PAY:]) == struct.unpack(">I", bytes(m[HASH:HASH + 4]))[0] else PAYLOAD


def copies(m, kind, R):
    """Whether the payload moves: it does not wait for the verdicts."""
    L = m.size
    return L >= 16 and not (m[FLAGS_AT[kind]] & 1) and L >= PAY and L == PAY + R


def model_pack(O, m, kind, src):
    L, R = m.size, src.size
    if L < 16:
        return SHORT
    at = HASH_AT[kind]
    if m[FLAGS_AT[kind]] & 1:
        m[at:at + 2] = _be(">H", O.crc("crc16", image(kind, m[:16])))
        return DEFERRED
    if L < PAY:
        return SHORT
    if L != PAY + R:
        return MISFIT
    m[PAY:] = src
    m[HASH:HASH + 4] = _be(">I", O.crc("crc32c", src))
    m[at:at + 2] = _be(">H", O.crc("crc16", image(kind, m[:16])))
    return OK


class Batch:
    """Host side of one kind's batch, read-only.  `blank`: the messages as a
    sender fills them (hashes and payload places random), in LIST order;
    `recv`: as a receiver finds them -- sealed, then the plants; `where[i]` =
    (buffer, start) of message i; `R[i]`: the other range's size; `src`: the
    payloads a pack copies in (a packed table at OBASE)."""


def make_batch(O, kind, count=None, seed=0):
    rng = np.random.default_rng(20261021 + KINDS.index(kind) + seed)
    b = Batch()
    b.kind = kind
    if count is None:
        # seven of each payload length but the largest (three), then the special sizes
        plen = [n for n in PLENS[:-1] for _ in range(7)] + [PLENS[-1]] * 3
        sizes = [PAY + n for n in plen]
        b.runts = list(range(len(sizes), len(sizes) + 5))
        sizes += [0, 7, 15, 16, 19]           # L < 16, and L in 16..payload_offset - 1 (eager: SHORT by rule 4)
        b.defer = list(range(len(sizes), len(sizes) + 4))
        sizes += [16, 16 + 3, 16 + 40, 16 + 1500]   # MORE_DATA set: garbage behind the core header
    else:
        sizes = [PAY + int(n) for n in rng.integers(0, 4097 - PAY, size=count)]  # messages of <= 4 KiB
        b.runts, b.defer = [], [int(i) for i in rng.choice(count, size=count // 50, replace=False)]
    n = len(sizes)
    order = rng.permutation(n)                # list position -> message: the list is shuffled
    sizes = [sizes[j] for j in order]
    inv = np.argsort(order)
    b.runts = sorted(int(inv[j]) for j in b.runts)
    b.defer = sorted(int(inv[j]) for j in b.defer)
    b.n, b.sizes = n, np.array(sizes, dtype=np.int64)
    b.blank = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in sizes]
    for i, m in enumerate(b.blank):
        if m.size >= 16:
            m[FLAGS_AT[kind]] = (m[FLAGS_AT[kind]] & 0xFE) | (1 if i in b.defer else 0)
    # where they lie: buffer (i * 5 + 1) % 3 -- neighbours in the list are not neighbours in memory --, and inside a
    # buffer in an order of its own, gaps of 0..37 bytes
    b.where = [None] * n
    b.buf_size = []
    for k in range(NBUF):
        mine = [i for i in range(n) if (i * 5 + 1) % NBUF == k]
        mine = [mine[j] for j in rng.permutation(len(mine))]
        at = GUARD + k                        # (the buffers' first messages start at different residues too)
        for i in mine:
            at += int(rng.integers(0, 38))
            b.where[i] = (k, at)
            at += sizes[i]
        b.buf_size.append(at + GUARD)
    eager = [i for i in range(n) if i not in b.runts and i not in b.defer]
    b.live = [i for i in eager if sizes[i] > PAY]
    if count is None:
        starts = {(b.where[i][1]) % 16 for i in eager}
        assert starts == set(range(16)), "message starts miss a residue mod 16"
    # the other side: R fits, but for the planted misfits (R = L - payload_offset + 1 and - 1) and the special sizes
    b.R = np.maximum(b.sizes - PAY, 0)
    for i in b.runts:
        b.R[i] = 3
    for i in b.defer:
        b.R[i] = 7
    b.misfits = [b.live[3], b.live[11]] if count is None else [b.live[5], b.live[77]]
    b.R[b.misfits[0]] += 1
    b.R[b.misfits[1]] -= 1
    b.t = np.zeros(n + 1, dtype=np.uint64)
    b.t[1:] = np.cumsum(b.R)
    b.t += np.uint64(OBASE)
    b.src = rng.integers(0, 256, size=int(b.t[-1]) + GUARD, dtype=np.uint8)
    b.dst0 = pattern(int(b.t[-1]) + GUARD, 3)
    # the receiver's batch: sealed by the model, then the plants, each in a message of its own
    b.recv = [m.copy() for m in b.blank]
    for m in b.recv:
        model_seal(O, m, kind)
    b.plants = {}
    if count is None:
        for i in b.runts:                     # an eager message of 16..19 bytes with a good header hash: SHORT by rule 4
            m = b.recv[i]
            if m.size >= 16:
                at = HASH_AT[kind]
                m[at:at + 2] = _be(">H", O.crc("crc16", image(kind, m[:16])))
        take = iter(i for i in b.live[20:] if i not in b.misfits)
        p = b.plants
        p["payload_bit"], p["payload_hash"], p["header_field"], p["header_hash"] = (next(take) for _ in range(4))
        m = b.recv[p["payload_bit"]]
        m[PAY + (977 % (m.size - PAY))] ^= 0x10
        b.recv[p["payload_hash"]][HASH + 2] ^= 0x01
        b.recv[p["header_field"]][0] ^= 0x04
        b.recv[p["header_hash"]][HASH_AT[kind] + 1] ^= 0x80
    b.vstat = np.array([model_verify(O, m, kind) for m in b.recv], dtype=np.uint8)
    b.ustat = np.array([model_verify(O, m, kind, int(b.R[i])) for i, m in enumerate(b.recv)], dtype=np.uint8)
    b.udst = b.dst0.copy()
    for i, m in enumerate(b.recv):
        if copies(m, kind, int(b.R[i])):
            b.udst[int(b.t[i]):int(b.t[i + 1])] = m[PAY:]
    b.sealed = [m.copy() for m in b.blank]
    b.sstat = np.array([model_seal(O, m, kind) for m in b.sealed], dtype=np.uint8)
    b.packed = [m.copy() for m in b.blank]
    b.pstat = np.array([model_pack(O, m, kind, b.src[int(b.t[i]):int(b.t[i + 1])]) for i, m in enumerate(b.packed)],
                       dtype=np.uint8)
    if count is None:
        p = b.plants
        assert b.vstat[p["payload_bit"]] == PAYLOAD and b.vstat[p["payload_hash"]] == PAYLOAD
        assert b.vstat[p["header_field"]] == HEADER and b.vstat[p["header_hash"]] == HEADER
        assert set(b.vstat.tolist()) == {OK, PAYLOAD, HEADER, SHORT, DEFERRED}
        assert set(b.ustat.tolist()) == {OK, PAYLOAD, HEADER, SHORT, DEFERRED, MISFIT}
        assert sorted(b.vstat[b.runts].tolist()) == [SHORT] * 5
        assert set(b.sstat.tolist()) == {OK, SHORT, DEFERRED} and set(b.pstat.tolist()) == {OK, SHORT, DEFERRED, MISFIT}
    assert all(b.ustat[i] == MISFIT and b.pstat[i] == MISFIT for i in b.misfits)
    assert all(b.vstat[i] == DEFERRED and b.pstat[i] == DEFERRED for i in b.defer)
    return b


_cache = {}


def batch_of(O, kind, count=None):
    if (kind, count) not in _cache:
        _cache[kind, count] = make_batch(O, kind, count)
    return _cache[kind, count]


def scatter(b, msgs):
    """The three host buffers with `msgs` at their places, the pattern everywhere else."""
    bufs = [pattern(s, k) for k, s in enumerate(b.buf_size)]
    for (k, at), m in zip(b.where, msgs):
        bufs[k][at:at + m.size] = m
    return bufs


def contiguous(msgs):
    """The same messages laid end to end at an odd base, in list order: (bytes, table)."""
    mo = np.zeros(len(msgs) + 1, dtype=np.uint64)
    mo[1:] = np.cumsum([m.size for m in msgs])
    mo += np.uint64(3)
    return np.concatenate([pattern(3)] + list(msgs) + [np.zeros(16, dtype=np.uint8)]), mo


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _table(tab):
    import torch
    return torch.from_numpy(np.asarray(tab).astype(np.int64)).cuda()


def device_list(gpu, b, bufs):
    """Three separate device allocations and the two arrays over them."""
    import torch
    dev = [_dev(h) for h in bufs]
    assert len({t.data_ptr() for t in dev}) == NBUF
    parts = [(dev[k], at, int(b.sizes[i])) for i, (k, at) in enumerate(b.where)]
    addr, lens, ah, lh = gpu.rpc_message_list(parts, with_host=True)
    assert addr.dtype == lens.dtype == torch.int64 and addr.numel() == lens.numel() == b.n
    assert np.any(np.diff(ah.astype(np.int64)) < 0), "the list is in address order"
    return dev, addr, lens, ah, lh


def counts_of(status, n):
    return np.bincount(status, minlength=n)[:n]


def _force(monkeypatch, light, nt):
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)


def check_receiver(gpu, b):
    kind = b.kind
    hbufs = scatter(b, b.recv)
    dev, addr, lens, ah, lh = device_list(gpu, b, hbufs)
    cbuf, mo = contiguous(b.recv)
    cdev, mod, tod = _dev(cbuf), _table(mo), _table(b.t)
    # verify: the list, the model, the table call on the same messages laid contiguously
    st, cn = gpu.verify_rpc_message_list(addr, lens, kind=kind, addr_host=ah, len_host=lh)
    tst, tcn = gpu.verify_rpc_messages(cdev, mod, kind=kind, offsets_host=mo)
    got = st.cpu().numpy()
    assert np.array_equal(got, b.vstat), np.nonzero(got != b.vstat)[0][:8]
    assert np.array_equal(got, tst.cpu().numpy())
    assert cn.numel() == 6 and np.array_equal(cn.cpu().numpy(), counts_of(b.vstat, 6))
    assert np.array_equal(cn.cpu().numpy(), tcn.cpu().numpy()) and int(cn.sum().item()) == b.n
    # unpack
    dst, tdst = _dev(b.dst0), _dev(b.dst0)
    st, cn = gpu.unpack_rpc_message_list(addr, lens, dst, tod, kind=kind, addr_host=ah, len_host=lh, dst_offsets_host=b.t)
    tst, tcn = gpu.unpack_rpc_messages(cdev, mod, tdst, tod, kind=kind, offsets_host=mo, dst_offsets_host=b.t)
    got = st.cpu().numpy()
    assert np.array_equal(got, b.ustat), np.nonzero(got != b.ustat)[0][:8]
    assert np.array_equal(got, tst.cpu().numpy())
    assert cn.numel() == 7 and np.array_equal(cn.cpu().numpy(), counts_of(b.ustat, 7))
    assert np.array_equal(cn.cpu().numpy(), tcn.cpu().numpy())
    gd = dst.cpu().numpy()
    bad = np.nonzero(gd != b.udst)[0]
    assert bad.size == 0, f"{bad.size} destination bytes differ from the model's, first at {bad[:4]}"
    assert np.array_equal(gd, tdst.cpu().numpy())
    for k in range(NBUF):
        assert np.array_equal(dev[k].cpu().numpy(), hbufs[k]), "a receiver call wrote a message buffer"


def check_sender(gpu, b):
    kind = b.kind
    # seal: whole buffers against the model's -- every gap and guard byte among them
    hbufs = scatter(b, b.blank)
    dev, addr, lens, ah, lh = device_list(gpu, b, hbufs)
    st = gpu.seal_rpc_message_list(addr, lens, kind=kind, addr_host=ah, len_host=lh)
    assert np.array_equal(st.cpu().numpy(), b.sstat)
    want = scatter(b, b.sealed)
    for k in range(NBUF):
        bad = np.nonzero(dev[k].cpu().numpy() != want[k])[0]
        assert bad.size == 0, f"buffer {k}: {bad.size} bytes differ from the model's seal, first at {bad[:4]}"
    cbuf, mo = contiguous(b.blank)
    cdev, mod, tod = _dev(cbuf), _table(mo), _table(b.t)
    tst = gpu.seal_rpc_messages(cdev, mod, kind=kind, offsets_host=mo)
    assert np.array_equal(tst.cpu().numpy(), b.sstat)
    assert np.array_equal(cdev.cpu().numpy(), contiguous(b.sealed)[0])
    # pack
    dev, addr, lens, ah, lh = device_list(gpu, b, hbufs)
    src = _dev(b.src)
    st = gpu.pack_rpc_message_list(src, tod, addr, lens, kind=kind, src_offsets_host=b.t, addr_host=ah, len_host=lh)
    assert np.array_equal(st.cpu().numpy(), b.pstat)
    want = scatter(b, b.packed)
    for k in range(NBUF):
        bad = np.nonzero(dev[k].cpu().numpy() != want[k])[0]
        assert bad.size == 0, f"buffer {k}: {bad.size} bytes differ from the model's pack, first at {bad[:4]}"
    assert np.array_equal(src.cpu().numpy(), b.src), "a pack wrote the source"
    cdev = _dev(cbuf)
    tst = gpu.pack_rpc_messages(src, tod, cdev, mod, kind=kind, src_offsets_host=b.t, offsets_host=mo)
    assert np.array_equal(tst.cpu().numpy(), b.pstat)
    assert np.array_equal(cdev.cpu().numpy(), contiguous(b.packed)[0])
    return dev, addr, lens, tod


@pytest.mark.parametrize("light,nt", ARMS)
@pytest.mark.parametrize("kind", KINDS)
def test_verify_and_unpack(gpu, oracle_mod, kind, light, nt, monkeypatch):
    """Sealed messages with the plants -- one payload bit, one stored payload
    hash, one header field, one header hash, each in a message of its own --,
    MORE_DATA with garbage behind the header, L < 16, L in 16..19, and the
    misfits R = L - payload_offset + 1 and - 1: statuses, counts and every
    destination byte equal the model's and the table calls'."""
    _force(monkeypatch, light, nt)
    check_receiver(gpu, batch_of(oracle_mod, kind))


@pytest.mark.parametrize("light,nt", ARMS)
@pytest.mark.parametrize("kind", KINDS)
def test_seal_pack_and_round_trip(gpu, oracle_mod, kind, light, nt, monkeypatch):
    """Seal and pack through the list: the three buffers equal the model's byte
    for byte (the gaps' pattern and the garbage behind a MORE_DATA header
    intact).  Then the round trip over the same list: verify reads OK or
    DEFERRED wherever pack said so, and unpack brings every OK payload back."""
    _force(monkeypatch, light, nt)
    O = oracle_mod
    b = batch_of(O, kind)
    dev, addr, lens, tod = check_sender(gpu, b)
    vst, vcn = gpu.verify_rpc_message_list(addr, lens, kind=kind)
    vst = vst.cpu().numpy()
    good = (b.pstat == OK) | (b.pstat == DEFERRED)
    assert np.array_equal(vst[good], b.pstat[good]) and int(vcn.sum().item()) == b.n
    dst = _dev(b.dst0)
    ust, ucn = gpu.unpack_rpc_message_list(addr, lens, dst, tod, kind=kind)
    ust, gd = ust.cpu().numpy(), dst.cpu().numpy()
    assert np.array_equal(ust[good], b.pstat[good]) and int(ucn.sum().item()) == b.n
    nok = 0
    for i in np.nonzero(b.pstat == OK)[0]:
        lo, hi = int(b.t[i]), int(b.t[i + 1])
        assert np.array_equal(gd[lo:hi], b.src[lo:hi]), i
        nok += hi > lo
    assert nok > 60
    # a batch whose every range fits: all OK or DEFERRED, the counts sum to count, all payloads back
    R = np.where(b.sizes >= PAY, b.sizes - PAY, 0)
    keep = [i for i in range(b.n) if b.sizes[i] >= PAY or i in b.defer]
    parts = [(dev[b.where[i][0]], b.where[i][1], int(b.sizes[i])) for i in keep]
    a2, l2 = gpu.rpc_message_list(parts)
    t2 = np.zeros(len(keep) + 1, dtype=np.uint64)
    t2[1:] = np.cumsum(R[keep])
    src2 = np.random.default_rng(7).integers(0, 256, size=int(t2[-1]) + 16, dtype=np.uint8)
    s2, t2d, d2 = _dev(src2), _table(t2), _dev(pattern(int(t2[-1]) + 16))
    pst = gpu.pack_rpc_message_list(s2, t2d, a2, l2, kind=kind).cpu().numpy()
    vst, vcn = gpu.verify_rpc_message_list(a2, l2, kind=kind)
    ust, ucn = gpu.unpack_rpc_message_list(a2, l2, d2, t2d, kind=kind)
    deferred = np.array([i in b.defer for i in keep])
    assert np.array_equal(pst, np.where(deferred, DEFERRED, OK))
    assert np.array_equal(vst.cpu().numpy(), pst) and np.array_equal(ust.cpu().numpy(), pst)
    assert int(vcn.sum().item()) == int(ucn.sum().item()) == len(keep)
    assert int(vcn[OK].item()) + int(vcn[DEFERRED].item()) == len(keep)
    got = d2.cpu().numpy()
    for j in range(len(keep)):
        lo, hi = int(t2[j]), int(t2[j + 1])
        if not deferred[j]:
            assert np.array_equal(got[lo:hi], src2[lo:hi]), j


@pytest.mark.parametrize("kind", KINDS)
def test_queue_path(gpu, oracle_mod, kind):
    """1,025 messages of up to 4 KiB: the smallest count that leaves the light
    layout (plan_offsets: light up to kRecvQueueBatch = 1,024 messages) and so
    takes the work queue (dyn_policy: every offsets batch of the full layout).
    Nothing is forced: this is the plan a caller gets."""
    b = batch_of(oracle_mod, kind, 1025)
    assert b.n == 1025
    check_receiver(gpu, b)
    check_sender(gpu, b)


def test_graph_replay(gpu, oracle_mod):
    """One captured verify_rpc_message_list after prepare of both methods.  A
    replay reads the arrays' current contents: rewritten in place to point at
    other messages of other lengths, the same graph gives the eager call's
    statuses and counts for those."""
    import torch
    O, kind = oracle_mod, "request"
    gpu.prepare("crc32c")
    gpu.prepare("crc16")
    b = batch_of(O, kind)
    hbufs = scatter(b, b.recv)
    dev, addr, lens, ah, lh = device_list(gpu, b, hbufs)
    n = b.n
    status = torch.full((n,), FAULT, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(6, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.verify_rpc_message_list(addr, lens, kind=kind, status=status, counts=counts)
    torch.cuda.synchronize()
    # first replay: the list as captured; second: entry i names message n - 1 - i, and every eager message with a
    # payload of two bytes or more is one byte shorter (another length, another CRC: PAYLOAD, or SHORT below 20)
    rev = np.arange(n)[::-1]
    ah2, lh2 = ah[rev].copy(), lh[rev].copy()
    cut = lh2 >= PAY + 2
    lh2[cut] -= np.uint64(1)
    for r, (a, l) in enumerate(((ah, lh), (ah2, lh2))):
        with torch.cuda.stream(s):
            addr.copy_(torch.from_numpy(a.view(np.int64)))
            lens.copy_(torch.from_numpy(l.view(np.int64)))
            status.fill_(FAULT)
            counts.zero_()
            g.replay()
        s.synchronize()
        got, gcn = status.cpu().numpy(), counts.cpu().numpy()
        est, ecn = gpu.verify_rpc_message_list(addr, lens, kind=kind)
        assert np.array_equal(got, est.cpu().numpy()), r
        assert np.array_equal(gcn, ecn.cpu().numpy()) and int(gcn.sum()) == n, r
        if r == 0:
            assert np.array_equal(got, b.vstat)
        else:
            want = np.array([model_verify(O, b.recv[j][:int(lh2[i])], kind) for i, j in enumerate(rev)], dtype=np.uint8)
            assert np.array_equal(got, want) and not np.array_equal(got, b.vstat[rev])


def test_wrapper_checks(gpu, oracle_mod):
    """With host copies of the arrays the wrappers refuse written messages that
    overlap one another and a message that overlaps the other side; empty lists
    are valid calls."""
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    other = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    addr, lens, ah, lh = gpu.rpc_message_list([(buf, 0, 100), (buf, 90, 100)], with_host=True)
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.seal_rpc_message_list(addr, lens, addr_host=ah, len_host=lh)
    gpu.verify_rpc_message_list(addr, lens, addr_host=ah, len_host=lh)  # (read only: they may)
    t = torch.tensor([0, 80, 160], dtype=torch.int64, device="cuda")
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.pack_rpc_message_list(other, t, addr, lens, src_offsets_host=[0, 80, 160], addr_host=ah, len_host=lh)
    addr, lens, ah, lh = gpu.rpc_message_list([(buf, 0, 100), (buf, 200, 100)], with_host=True)
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.unpack_rpc_message_list(addr, lens, buf, t, addr_host=ah, len_host=lh, dst_offsets_host=[250, 330, 410])
    with pytest.raises(gpu.GpuChecksumError, match="past the end"):
        gpu.rpc_message_list([(buf, 4000, 100)])
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    t1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    e8 = torch.zeros(0, dtype=torch.uint8, device="cuda")
    st, cn = gpu.verify_rpc_message_list(e, e)
    assert st.numel() == 0 and cn.numel() == 6 and int(cn.sum().item()) == 0
    assert gpu.seal_rpc_message_list(e, e).numel() == 0
    st, cn = gpu.unpack_rpc_message_list(e, e, e8, t1)
    assert st.numel() == 0 and cn.numel() == 7
    assert gpu.pack_rpc_message_list(e8, t1, e, e).numel() == 0
