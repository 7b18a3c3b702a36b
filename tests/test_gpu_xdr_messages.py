"""XDR-mode messages verified, sealed and unpacked in place on the GPU
(include/mchecksum_gpu.h: mchecksum_gpu_verify_xdr_messages,
_seal_xdr_messages, _unpack_xdr_messages).

A message is header bytes with the big-endian hash at byte 16, then the XDR
proc buffer from payload_offset on, then a few slack bytes (a slice of a
multi-recv buffer).  The oracle is oracle.xdr_encode / xdr_hashed_stream / crc,
as in test_xdr.py: a message verifies when it is at least payload_offset long,
the schema fits in it and crc(hashed stream) equals the header hash; it
unpacks to exactly the hashed stream when that is as long as its slot."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLIB = os.path.join(ROOT, "build", "libmchecksum_qfault.so")

# the kernels a call can take: "0" the latency layout, "1" the throughput layout
# with default loads, "1-nt" the same with non-temporal loads (MCHECKSUM_GPU_NT=1:
# what a batch of 8192 messages and more takes by itself; the latency layout
# has no such variant)
LAYOUTS = ["0", "1", "1-nt"]
HASH = 16
# The throughput layout's step loop (payload32_g64: fields of kXdrFastMin = 256
# bytes and more) moves 1024 bytes a step through a ring of kRingOff = 8 steps:
# one step, two steps, the ring's fill (8 KiB) and two rings (16 KiB: the first
# length whose steady loop, which loads a step as it folds one, runs at all),
# each with its neighbours.  The start alignment shifts the step count by one.
RING_LENS = [1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385]
# the edges of the 4-byte pad, the 64 lane ranges and kXdrFastMin = 256; then the ring's
LENS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000] + RING_LENS
BIG = 70001
NMSG = 300
# messages RING_AT + 2k and RING_AT + 2k + 1 carry RING_LENS[k] whatever the draw: an
# odd and an even message start each, so an odd source and an odd destination address
RING_AT = 104
SENTINEL = 0xA5


def _path(monkeypatch, layout):
    """Select the kernel of LAYOUTS' entry `layout` (the library re-reads its
    settings on every change made through this monkeypatch)."""
    monkeypatch.setenv("MCHECKSUM_GPU_XDR_FAST", layout[0])
    if layout.endswith("-nt"):
        monkeypatch.setenv("MCHECKSUM_GPU_NT", "1")
    else:
        monkeypatch.delenv("MCHECKSUM_GPU_NT", raising=False)


def _forced_len(i):
    """The length message i of a NMSG batch carries whatever the draw, or None."""
    if i % 97 == 5:
        return BIG
    k = (i - RING_AT) // 2
    return RING_LENS[k] if 0 <= k < len(RING_LENS) else None


def _schemas(O):
    I, OP, OPL, RAW, RAWL, SKIP = (O.XDR_INT, O.XDR_OPAQUE, O.XDR_OPAQUE_LEN, O.XDR_RAW, O.XDR_RAW_LEN,
                                   O.XDR_SKIP_IF_ZERO)
    return {
        "iovec": [(I, 4), (OPL, 0)],
        "mixed": [(I, 1), (I, 2), (I, 4), (I, 8), (I, 8), (SKIP, 3), (OPL, 0), (I, 1), (I, 1),
                  (I, 8), (RAWL, 0), (OP, 7), (RAW, 5), (I, 2)],
        "empty": [],
    }


def _values(rng, schema, O, force):
    """Random field values; an INT that a length-driven field or a SKIP reads
    is drawn from LENS (`force`, unless None: the first such INT is that)."""
    vals, last, f = [], None, 0
    while f < len(schema):
        kind, size = schema[f]
        if kind == O.XDR_SKIP_IF_ZERO:
            if last == 0:
                f += size
            f += 1
            continue
        nxt = schema[f + 1][0] if f + 1 < len(schema) else None
        if kind == O.XDR_INT:
            if nxt in (O.XDR_OPAQUE_LEN, O.XDR_RAW_LEN, O.XDR_SKIP_IF_ZERO):
                v = force if force is not None else int(rng.choice(LENS))
                force = None
            else:
                v = int(rng.integers(-(1 << (8 * size - 1)), 1 << (8 * size - 1)))
            vals.append(v)
            last = v & ((1 << (8 * size)) - 1)
        else:
            n = last if kind in (O.XDR_OPAQUE_LEN, O.XDR_RAW_LEN) else size
            vals.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        f += 1
    return vals


class Batch:
    """Messages (hash slots zero) whose starts fall on every residue mod 16."""

    def __init__(self, O, kind, pay, seed, count=NMSG, forced=_forced_len):
        self.kind, self.pay, self.schema = kind, pay, _schemas(O)[kind]
        rng = np.random.default_rng(seed)
        self.msgs, self.xdr_len, pos = [], [], 0
        for i in range(count):
            xdr = O.xdr_encode(self.schema, _values(rng, self.schema, O, forced(i)))
            hdr = bytearray(rng.integers(0, 256, pay, dtype=np.uint8).tobytes())
            hdr[HASH:HASH + 4] = b"\0\0\0\0"
            n = pay + len(xdr)
            slack = (i + 1 - (pos + n)) % 16  # message i starts at residue i mod 16
            self.msgs.append(bytes(hdr) + xdr + rng.integers(0, 256, slack, dtype=np.uint8).tobytes())
            self.xdr_len.append(len(xdr))
            pos += n + slack
        self._crc, self._streams = {}, None

    def streams(self, O):
        if self._streams is None:
            self._streams = [O.xdr_hashed_stream(self.schema, m[self.pay:]) for m in self.msgs]
        return self._streams

    def crcs(self, O, method):
        if method not in self._crc:
            self._crc[method] = [O.crc(method, s) for s in self.streams(O)]
        return self._crc[method]

    def sealed(self, O, method):
        return [_with_hash(m, c) for m, c in zip(self.msgs, self.crcs(O, method))]


_batches = {}


def _batch(O, kind, pay):
    if (kind, pay) not in _batches:
        _batches[kind, pay] = Batch(O, kind, pay, 1000 + pay + len(kind))
    return _batches[kind, pay]


def _with_hash(m, crc):
    return m[:HASH] + int(crc).to_bytes(4, "big") + m[HASH + 4:]


def _flip(m, at, bit=0x10):
    return m[:at] + bytes([m[at] ^ bit]) + m[at + 1:]


def _table(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return off


def _upload(msgs):
    import torch
    off = _table(msgs)
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    data = torch.zeros(blob.size + 64, dtype=torch.uint8, device="cuda")
    if blob.size:
        data[:blob.size].copy_(torch.from_numpy(blob.copy()))
    return data, torch.from_numpy(off).cuda(), off, blob


def _verdicts(O, method, schema, pay, msgs):
    """Per message: (fails, hashed stream or None), by the oracle."""
    out = []
    for m in msgs:
        s = O.xdr_hashed_stream(schema, m[pay:]) if len(m) >= pay else None
        bad = s is None or O.crc(method, s) != int.from_bytes(m[HASH:HASH + 4], "big")
        out.append((bad, s))
    return out


CASES = [("iovec", 20), ("mixed", 23), ("iovec", 23), ("mixed", 20)]


# ------------------------------------------------------------ round trip ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", ["crc32c", "crc32"])
@pytest.mark.parametrize("kind,pay", CASES)
def test_seal_then_verify_round_trip(gpu, oracle_mod, kind, pay, method, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O = oracle_mod
    b = _batch(O, kind, pay)
    assert {int(o) % 16 for o in _table(b.msgs)[:-1]} == set(range(16))
    data, offs, off, blob = _upload(b.msgs)
    if kind == "iovec":  # the body lies behind the headers and the u32 length: every ring length at an odd address
        assert {b.xdr_len[i] - 4 for i in range(NMSG) if (off[i] + pay + 4) % 2} >= {n + -n % 4 for n in RING_LENS}
    st = gpu.seal_xdr_messages(method, data, offs, b.schema, payload_offset=pay, offsets_host=off)
    torch.cuda.synchronize()
    assert int(st.sum().item()) == 0
    got = data.cpu().numpy()
    want = np.frombuffer(b"".join(b.sealed(O, method)), dtype=np.uint8)
    slots = (off[:-1, None] + HASH + np.arange(4)[None, :]).ravel()
    assert np.array_equal(got[slots], want[slots]), "a stored hash is not the oracle's CRC, big-endian"
    rest = np.ones(blob.size, dtype=bool)
    rest[slots] = False
    assert np.array_equal(got[:blob.size][rest], blob[rest]), "a byte outside the hash slots was written"
    assert not got[blob.size:].any()
    st, mism = gpu.verify_xdr_messages(method, data, offs, b.schema, payload_offset=pay, offsets_host=off)
    torch.cuda.synchronize()
    assert int(st.sum().item()) == 0 and int(mism.item()) == 0


# -------------------------------------------------------- exact failures ----

def _damaged(O, b, method):
    """The sealed batch with one bit flipped in an INT, an opaque body, a pad
    byte and a hash slot, three messages truncated (by 1 byte, by 5 bytes, to
    half) and one shorter than payload_offset.  Returns (messages, {what:
    index})."""
    msgs, pay = b.sealed(O, method), b.pay
    used = set()

    def pick(ok, start):
        i = next(i for i in range(start, NMSG) if i not in used and ok(i))
        used.add(i)
        return i

    if b.kind == "iovec":
        # u32 length then the bytes: body at pay + 4, pad behind it
        lens = [int.from_bytes(m[pay:pay + 4], "big") for m in msgs]
        body = pick(lambda i: lens[i] == 257, 10)
        padm = pick(lambda i: lens[i] % 4 != 0, 10)
        body_at, pad_at = pay + 4 + 100, pay + 4 + lens[padm]
    else:
        # the schema ends (OP, 7) = 7 bytes + 1 pad, (RAW, 5), (I, 2) in 4 bytes
        body, padm = pick(lambda i: True, 20), pick(lambda i: True, 30)
        body_at = pay + b.xdr_len[body] - 4 - 5 - 8 + 2
        pad_at = pay + b.xdr_len[padm] - 4 - 5 - 1
    idx = {"int": pick(lambda i: True, 3), "body": body, "pad": padm, "hash": pick(lambda i: True, 40)}
    msgs[idx["int"]] = _flip(msgs[idx["int"]], pay + 3)  # the low byte of the first INT
    msgs[body] = _flip(msgs[body], body_at)
    msgs[padm] = _flip(msgs[padm], pad_at)               # not hashed: must still verify
    msgs[idx["hash"]] = _flip(msgs[idx["hash"]], HASH + 2)
    for what, cut in (("cut1", 1), ("cut5", 5), ("half", None)):
        i = idx[what] = pick(lambda i: b.xdr_len[i] > 8, 50)
        n = pay + b.xdr_len[i]
        msgs[i] = msgs[i][:n - cut] if cut else msgs[i][:n // 2]
    idx["short"] = pick(lambda i: True, 80)
    msgs[idx["short"]] = msgs[idx["short"]][:pay - 3]
    idx["used"] = used
    return msgs, idx


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_verify_flags_exactly_the_failures(gpu, oracle_mod, kind, pay, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O, method = oracle_mod, "crc32c"
    b = _batch(O, kind, pay)
    msgs, idx = _damaged(O, b, method)
    want = np.array([bad for bad, _ in _verdicts(O, method, b.schema, pay, msgs)], dtype=np.uint8)
    # the oracle's verdicts: everything damaged but the pad flip, which is not hashed
    assert want[idx["pad"]] == 0 and want.sum() == 7
    assert all(want[idx[k]] == 1 for k in ("int", "body", "hash", "cut1", "cut5", "half", "short"))
    data, offs, off, blob = _upload(msgs)
    st, mism = gpu.verify_xdr_messages(method, data, offs, b.schema, payload_offset=pay, offsets_host=off)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), want)
    assert int(mism.item()) == int(want.sum())
    # without statuses, then without a counter
    _, mism = gpu.verify_xdr_messages(method, data, offs, b.schema, payload_offset=pay, status=False)
    st, none = gpu.verify_xdr_messages(method, data, offs, b.schema, payload_offset=pay, mismatches=False)
    torch.cuda.synchronize()
    assert int(mism.item()) == int(want.sum()) and none is False
    assert np.array_equal(st.cpu().numpy(), want)
    assert np.array_equal(data.cpu().numpy()[:blob.size], blob), "verify wrote to the buffer"
    # sealing the damaged batch: the short and truncated ones are refused and not written
    st = gpu.seal_xdr_messages(method, data, offs, b.schema, payload_offset=pay)
    torch.cuda.synchronize()
    trunc = np.array([s is None for _, s in _verdicts(O, method, b.schema, pay, msgs)], dtype=np.uint8)
    assert np.array_equal(st.cpu().numpy(), trunc)
    got = data.cpu().numpy()
    for i in np.nonzero(trunc)[0]:
        assert np.array_equal(got[off[i]:off[i + 1]], blob[off[i]:off[i + 1]])


# ---------------------------------------------------------------- unpack ----

def _unpack_case(O, b, method):
    """(messages, msg table, dst table, expected status, expected dst image,
    guard mask).  After every message comes an empty one (no bytes: it fails)
    whose slot is a guard gap sized so that the next slot starts on the next
    residue mod 16; three slots do not fit their message (one byte too long,
    one too short, zero length)."""
    msgs, idx = _damaged(O, b, method)
    verd = _verdicts(O, method, b.schema, b.pay, msgs)
    all_msgs, slots = [], []
    whole = [i for i in range(100, NMSG) if i not in idx["used"] and len(verd[i][1]) > 1]
    misfit = {whole[0]: 1, whole[1]: -1, whole[2]: None}
    for i, (m, (bad, s)) in enumerate(zip(msgs, verd)):
        n = len(s) if s is not None else 10
        if i in misfit:
            assert s is not None and len(s) > 1
            n = n + misfit[i] if misfit[i] else 0
        all_msgs += [m, b""]
        slots += [n, 0]
    lead = 37
    doff = np.zeros(len(slots) + 1, dtype=np.int64)
    doff[0] = lead
    for k in range(len(slots)):
        if k % 2 == 1:  # the gap: the next real slot starts at residue (k + 1) / 2 mod 16
            slots[k] = ((k + 1) // 2 - int(doff[k])) % 16 + 16 * (k % 4 == 1)
        doff[k + 1] = doff[k] + slots[k]
    total = int(doff[-1]) + 29
    want = np.full(total, SENTINEL, dtype=np.uint8)
    status = np.ones(len(slots), dtype=np.uint8)
    for i, (bad, s) in enumerate(verd):
        k = 2 * i
        if s is not None and len(s) == slots[k]:
            want[doff[k]:doff[k + 1]] = np.frombuffer(s, dtype=np.uint8)
            status[k] = bad
    assert {int(d) % 16 for d in doff[0:-1:2]} == set(range(16))
    return all_msgs, doff, status, want, idx


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", ["crc32c", "crc32"])
@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_unpack_decodes_and_verifies(gpu, oracle_mod, kind, pay, method, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O = oracle_mod
    b = _batch(O, kind, pay)
    msgs, doff, want_st, want, idx = _unpack_case(O, b, method)
    data, offs, off, blob = _upload(msgs)
    if kind == "iovec":  # every ring length is read at an odd address, and stored at one (entry 2i is message i)
        body = {i: int(doff[2 * i + 1] - doff[2 * i]) - 4 for i in range(RING_AT, NMSG)}
        assert {n for i, n in body.items() if (off[2 * i] + pay + 4) % 2} >= set(RING_LENS)
        assert {n for i, n in body.items() if (doff[2 * i] + 4) % 2} >= set(RING_LENS)
    dst = torch.full((want.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    st, mism = gpu.unpack_xdr_messages(method, data, offs, b.schema, dst, torch.from_numpy(doff).cuda(),
                                       payload_offset=pay, offsets_host=off, dst_offsets_host=doff)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} destination bytes differ, first at {bad[:5]}"
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert int(mism.item()) == int(want_st.sum())
    # a corrupted message that fits is flagged and holds the bytes as decoded
    k = 2 * idx["hash"]
    assert want_st[k] == 1 and doff[k + 1] > doff[k] and np.any(want[doff[k]:doff[k + 1]] != SENTINEL)
    assert np.array_equal(data.cpu().numpy()[:blob.size], blob), "unpack wrote to the source"


# ------------------------------------------------- the default count rule ----
# With no setting, a batch takes the throughput layout past 1024 messages and
# its non-temporal kernel from 8192 on (launch_plan.h: nt_by_count): 8192 is the
# smallest count that runs xdr_msg_fast_kernel<OP, true> by itself, 8191 the
# largest that runs <OP, false>.

RULE_COUNTS = [8191, 8192]
RULE_BIG_AT = 4100
RULE_LARGE = [n for n in LENS if n >= 256]


def _rule_len(i):
    """iovec lengths under 64; about every 64th message (every 63rd: coprime
    to the 16 start residues) carries the next of LENS' lengths from 256 up,
    and one carries BIG."""
    if i == RULE_BIG_AT:
        return BIG
    if i % 63 == 9:
        return RULE_LARGE[(i // 63) % len(RULE_LARGE)]
    return (37 * i + 11) % 64


def _rule_batch(O):
    if "rule" not in _batches:
        _batches["rule"] = Batch(O, "iovec", 20, 4242, count=RULE_COUNTS[-1], forced=_rule_len)
    return _batches["rule"]


def _no_settings(monkeypatch):
    monkeypatch.delenv("MCHECKSUM_GPU_XDR_FAST", raising=False)
    monkeypatch.delenv("MCHECKSUM_GPU_NT", raising=False)


def _rule_damage(O, b, method, count):
    """The first `count` sealed messages with a body byte flipped in BIG and in
    a 16 KiB body, a hash byte flipped in a tiny message and the last message
    cut by a byte; the oracle's verdict for each: (messages, bad)."""
    msgs, pay = b.sealed(O, method)[:count], b.pay
    big16 = next(i for i in range(count) if b.xdr_len[i] == 4 + 16384)
    msgs[RULE_BIG_AT] = _flip(msgs[RULE_BIG_AT], pay + 4 + 60001)
    msgs[big16] = _flip(msgs[big16], pay + 4 + 9000)
    msgs[77] = _flip(msgs[77], HASH + 1)
    last = next(i for i in range(count - 1, 0, -1) if b.xdr_len[i] > 4)
    msgs[last] = msgs[last][:pay + b.xdr_len[last] - 1]
    bad = np.zeros(count, dtype=np.uint8)  # (sealed with the oracle's CRC: the others verify by construction)
    for i in (RULE_BIG_AT, big16, 77, last):
        bad[i] = _verdicts(O, method, b.schema, pay, [msgs[i]])[0][0]
    assert bad.sum() == 4
    return msgs, bad


@pytest.mark.parametrize("count", RULE_COUNTS)
def test_seal_by_the_default_count_rule(gpu, oracle_mod, count, monkeypatch):
    import torch
    _no_settings(monkeypatch)
    O, method = oracle_mod, "crc32c"
    b = _rule_batch(O)
    assert {int(o) % 16 for o in _table(b.msgs)[:-1]} == set(range(16))
    data, offs, off, blob = _upload(b.msgs[:count])
    st = gpu.seal_xdr_messages(method, data, offs, b.schema, payload_offset=b.pay, offsets_host=off)
    torch.cuda.synchronize()
    assert int(st.sum().item()) == 0
    got = data.cpu().numpy()
    want = np.frombuffer(b"".join(b.sealed(O, method)[:count]), dtype=np.uint8)
    bad = np.nonzero(got[:blob.size] != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ from the oracle's sealed messages, first at {bad[:5]}"
    assert not got[blob.size:].any()


@pytest.mark.parametrize("count", RULE_COUNTS)
def test_verify_by_the_default_count_rule(gpu, oracle_mod, count, monkeypatch):
    import torch
    _no_settings(monkeypatch)
    O, method = oracle_mod, "crc32c"
    b = _rule_batch(O)
    msgs, want = _rule_damage(O, b, method, count)
    data, offs, off, blob = _upload(msgs)
    st, mism = gpu.verify_xdr_messages(method, data, offs, b.schema, payload_offset=b.pay, offsets_host=off)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), want)
    assert int(mism.item()) == int(want.sum())
    assert np.array_equal(data.cpu().numpy()[:blob.size], blob), "verify wrote to the buffer"


@pytest.mark.parametrize("count", RULE_COUNTS)
def test_unpack_by_the_default_count_rule(gpu, oracle_mod, count, monkeypatch):
    """Every slot is as long as its message's hashed stream, but one (a 8 KiB
    body's, a byte longer: not written); slots start 37 bytes in and follow
    one another, so their starts fall on every residue mod 16."""
    import torch
    _no_settings(monkeypatch)
    O, method = oracle_mod, "crc32c"
    b = _rule_batch(O)
    msgs, bad = _rule_damage(O, b, method, count)
    verd = [(0, s) for s in b.streams(O)[:count]]
    for i in np.nonzero(bad)[0]:
        verd[i] = _verdicts(O, method, b.schema, b.pay, [msgs[i]])[0]
    misfit = next(i for i in range(count) if b.xdr_len[i] == 4 + 8192)
    slots = [len(s) if s is not None else 10 for _, s in verd]
    slots[misfit] += 1
    doff = np.concatenate([[37], 37 + np.cumsum(slots)]).astype(np.int64)
    assert {int(d) % 16 for d in doff[:-1]} == set(range(16))
    want = np.full(int(doff[-1]) + 29, SENTINEL, dtype=np.uint8)
    want_st = np.ones(count, dtype=np.uint8)
    for i, (fails, s) in enumerate(verd):
        if s is not None and i != misfit:
            want[doff[i]:doff[i + 1]] = np.frombuffer(s, dtype=np.uint8)
            want_st[i] = fails
    assert want_st.sum() == 5
    data, offs, off, blob = _upload(msgs)
    dst = torch.full((want.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    st, mism = gpu.unpack_xdr_messages(method, data, offs, b.schema, dst, torch.from_numpy(doff).cuda(),
                                       payload_offset=b.pay, offsets_host=off, dst_offsets_host=doff)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    wrong = np.nonzero(got != want)[0]
    assert wrong.size == 0, f"{wrong.size} destination bytes differ, first at {wrong[:5]}"
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert int(mism.item()) == int(want_st.sum())
    assert np.array_equal(data.cpu().numpy()[:blob.size], blob), "unpack wrote to the source"


# --------------------------------------------- empty batch, empty schema ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_empty_batch_and_empty_schema(gpu, oracle_mod, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O = oracle_mod
    schema = _schemas(O)["iovec"]
    data = torch.zeros(64, dtype=torch.uint8, device="cuda")
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    st, mism = gpu.verify_xdr_messages("crc32c", data, one, schema)
    assert st.numel() == 0 and int(mism.item()) == 0
    assert gpu.seal_xdr_messages("crc32c", data, one, schema).numel() == 0
    st, mism = gpu.unpack_xdr_messages("crc32c", data, one, schema, data, one)
    assert st.numel() == 0 and int(mism.item()) == 0
    # no fields: every message hashes the empty stream
    b = Batch(O, "empty", 20, 77, count=40)
    empty = O.crc("crc32c", b"")
    assert b.crcs(O, "crc32c") == [empty] * 40
    data, offs, off, blob = _upload(b.msgs)
    assert int(gpu.seal_xdr_messages("crc32c", data, offs, [], offsets_host=off).sum().item()) == 0
    got = data.cpu().numpy()
    for o in off[:-1]:
        assert int.from_bytes(got[o + HASH:o + HASH + 4].tobytes(), "big") == empty
    st, mism = gpu.verify_xdr_messages("crc32c", data, offs, [], offsets_host=off)
    assert int(st.sum().item()) == 0 and int(mism.item()) == 0
    # unpack: only zero-length slots fit
    sl = np.zeros(40, dtype=np.int64)
    sl[[3, 17]] = (1, 9)
    doff = np.zeros(41, dtype=np.int64)
    doff[1:] = np.cumsum(sl)
    doff += 5
    dst = torch.full((int(doff[-1]) + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    st, mism = gpu.unpack_xdr_messages("crc32c", data, offs, [], dst, torch.from_numpy(doff).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), (sl != 0).astype(np.uint8)) and int(mism.item()) == 2
    assert bool((dst == SENTINEL).all().item())


# ---------------------------------------------------------- graph replay ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_graph_replay_reads_current_contents(gpu, oracle_mod, layout, monkeypatch):
    """verify and unpack captured after prepare(): a replay judges the bytes
    and the tables as they are at that moment."""
    import torch
    _path(monkeypatch, layout)
    O, method, pay = oracle_mod, "crc32c", 20
    gpu.prepare(method)
    b = _batch(O, "iovec", pay)
    good = b.sealed(O, method)
    data, offs, off, blob = _upload(good)
    n = len(good)

    def dst_table(verd):
        d = np.zeros(n + 1, dtype=np.int64)
        d[1:] = np.cumsum([len(s) if s is not None else 0 for _, s in verd])
        return d + 3

    verd0 = _verdicts(O, method, b.schema, pay, good)
    doff = dst_table(verd0)
    doffs = torch.from_numpy(doff).cuda()
    dst = torch.full((int(doff[-1]) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    vst, ust = (torch.ones(n, dtype=torch.uint8, device="cuda") for _ in range(2))
    vm, um = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.verify_xdr_messages(method, data, offs, b.schema, payload_offset=pay, status=vst, mismatches=vm)
        gpu.unpack_xdr_messages(method, data, offs, b.schema, dst, doffs, payload_offset=pay, status=ust,
                                mismatches=um)
    torch.cuda.synchronize()

    def replay_and_check(msgs, doff):
        verd = _verdicts(O, method, b.schema, pay, msgs)
        with torch.cuda.stream(s):
            for t in (vm, um):
                t.zero_()
            dst.fill_(SENTINEL)
            g.replay()
        torch.cuda.synchronize()
        want_v = np.array([bad for bad, _ in verd], dtype=np.uint8)
        fits = np.array([s_ is not None and len(s_) == doff[i + 1] - doff[i] for i, (_, s_) in enumerate(verd)])
        want_u = np.where(fits, want_v, 1).astype(np.uint8)
        assert np.array_equal(vst.cpu().numpy(), want_v) and int(vm.item()) == int(want_v.sum())
        assert np.array_equal(ust.cpu().numpy(), want_u) and int(um.item()) == int(want_u.sum())
        want = np.full(dst.numel(), SENTINEL, dtype=np.uint8)
        for i, (_, s_) in enumerate(verd):
            if fits[i]:
                want[doff[i]:doff[i + 1]] = np.frombuffer(s_, dtype=np.uint8)
        assert np.array_equal(dst.cpu().numpy(), want)
        return int(want_v.sum()), int(want_u.sum())

    assert replay_and_check(good, doff) == (0, 0)
    # new contents: a flipped body byte and a flipped hash
    lens = [int.from_bytes(m[pay:pay + 4], "big") for m in good]
    i1 = next(i for i in range(NMSG) if lens[i] >= 63)
    bad = list(good)
    bad[i1] = _flip(bad[i1], pay + 4 + 7)
    bad[9] = _flip(bad[9], HASH)
    with torch.cuda.stream(s):
        data[:blob.size].copy_(torch.from_numpy(np.frombuffer(b"".join(bad), dtype=np.uint8).copy()))
    assert replay_and_check(bad, doff) == (2, 2)
    # new tables: message 12 loses its last XDR bytes to message 13, and slot 20 grows by one
    off2, doff2 = off.copy(), doff.copy()
    cut = len(good[12]) - (pay + b.xdr_len[12]) + 2
    assert b.xdr_len[12] > 4
    off2[13] -= cut
    doff2[21:] += 1
    moved = [bytes(bad_) for bad_ in bad]
    moved[12], moved[13] = bad[12][:-cut], bad[12][-cut:] + bad[13]
    with torch.cuda.stream(s):
        offs.copy_(torch.from_numpy(off2))
        doffs.copy_(torch.from_numpy(doff2))
    nv, nu = replay_and_check(moved, doff2)
    assert nv > 2 and nu > nv  # the cut broke messages 12 and 13; slot 20 no longer fits


# ------------------------------------------------ checksum_xdr unchanged ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_checksum_xdr_values_after_the_message_calls(gpu, oracle_mod, kind, pay, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O = oracle_mod
    b = _batch(O, kind, pay)
    data, offs, off, blob = _upload(b.msgs)
    gpu.seal_xdr_messages("crc32c", data, offs, b.schema, payload_offset=pay)
    gpu.verify_xdr_messages("crc32c", data, offs, b.schema, payload_offset=pay)
    # checksum_xdr's messages start at the proc buffer: the same bytes, each from its payload_offset on
    bodies = [m[pay:] for m in b.msgs]
    bdata, boffs, boff, _ = _upload(bodies)
    for method in ("crc32c", "crc64"):
        got = gpu.as_unsigned(gpu.checksum_xdr(method, bdata, boffs, b.schema, offsets_host=boff))
        want = [O.crc(method, O.xdr_hashed_stream(b.schema, m)) for m in bodies]
        assert got.tolist() == want


# ----------------------------------------------------------- fail closed ----

def test_verify_fault_fails_closed(gpu, oracle_mod, monkeypatch):
    """The fault-injecting build (build/libmchecksum_qfault.so) in its give-up
    mode: workgroup 3 drops one message of the throughput layout's queue.  The
    call adds 1 to the error word and `count` to the counter, and every status
    reads 1 -- over a batch in which every message verifies."""
    import torch
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    from mercury_amd._lib import XdrField
    L = ctypes.CDLL(QLIB)
    c = ctypes
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    L.mchecksum_gpu_verify_xdr_messages.argtypes = [c.c_char_p, c.POINTER(XdrField), c.c_size_t, c.c_void_p, c.c_void_p,
                                                    c.c_size_t, c.c_size_t, c.c_size_t, c.c_void_p, c.c_void_p,
                                                    c.c_void_p]
    L.mchecksum_gpu_set_error_word.argtypes = [c.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = c.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    monkeypatch.delenv("MCHECKSUM_GPU_QFAULT_MODE", raising=False)  # the give-up, not a stall
    monkeypatch.delenv("MCHECKSUM_GPU_XDR_FAST", raising=False)     # > 1024 messages: the throughput layout
    L.mchecksum_gpu_reload_settings()
    try:
        O, pay, n = oracle_mod, 20, 20000
        rng = np.random.default_rng(9)
        body = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
        hdr = bytes(HASH) + b"\0\0\0\0"
        kinds = [O.xdr_encode(_schemas(O)["iovec"], [k, body[:k]]) for k in (0, 5, 64, 300)]
        sealed = [_with_hash(hdr + x, O.crc("crc32c", O.xdr_hashed_stream(_schemas(O)["iovec"], x))) for x in kinds]
        msgs = [sealed[i % 4] for i in range(n)]
        data, offs, off, blob = _upload(msgs)
        fields = (XdrField * 2)(XdrField(O.XDR_INT, 4), XdrField(O.XDR_OPAQUE_LEN, 0))
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")  # stale "verified" everywhere
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        faults0 = L.mchecksum_gpu_queue_faults()
        assert L.mchecksum_gpu_prepare(b"crc32c") == 0
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_verify_xdr_messages(b"crc32c", fields, 2, data.data_ptr(), offs.data_ptr(), n, pay, HASH,
                                                     status.data_ptr(), mism.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        assert int(mism.item()) == n
        assert bool((status == 1).all().item())
    finally:
        monkeypatch.undo()
        L.mchecksum_gpu_reload_settings()
