"""XDR-mode sender on the GPU: encode, hash and seal in one pass, and the two
size calls (include/mchecksum_gpu.h: mchecksum_gpu_pack_xdr_messages,
_xdr_encoded_sizes, _xdr_decoded_sizes, MCHECKSUM_XDR_SINT).

The oracle is oracle.xdr_encode / xdr_hashed_stream / crc, as in
test_gpu_xdr_messages.py: wire = xdr_encode(schema, values), image =
xdr_hashed_stream(schema, wire) -- the non-XDR image the call reads -- and the
sealed hash is crc(method, image).  xdr_encode masks the Python integer to its
slot: a negative value gives the sign-extended word (SINT), a non-negative one
below 2^(8 size) the zero-extended word (INT).  The oracle knows no kind 6 and
treats every non-INT kind as bytes, so it gets the schema with SINT mapped to
INT.  What a call must do with given tables is worked out by _expect(), from
the oracle and the tables alone.

Both tables are contiguous, so the batches that put image and message starts
on chosen residues mod 16 separate the messages by gap entries: a few source
bytes and a slot shorter than the headers, which never fits (status 1, not
written).

Not tested: fields of 2^31 bytes and more, which take the lane-range path by
construction (the step loop's lengths are 31 bits) -- too slow for a unit
test."""
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
# The throughput layout's copying step loop (payload32_g64: fields of kXdrFastMin
# = 256 bytes and more) moves 1024 bytes a step through a ring of kRingOff = 8
# steps: one step, two steps, the ring's fill (8 KiB) and two rings (16 KiB: the
# first length whose steady loop, which loads a step as it folds one, runs at
# all), each with its neighbours.  The start alignment shifts the step count by one.
RING_LENS = [1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385]
# the edges of the 4-byte pad, the 64 lane ranges and kXdrFastMin = 256; then the ring's
LENS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000] + RING_LENS
BIG = 70001
NMSG = 300
# messages RING_AT + 2k and RING_AT + 2k + 1 carry RING_LENS[k] whatever the draw: an
# odd and an even image start each, over message starts of both parities (Batch)
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
I, OP, OPL, RAW, RAWL, SKIP, S = 0, 1, 2, 3, 4, 5, 6  # MCHECKSUM_XDR_*; S = MCHECKSUM_XDR_SINT

SCHEMAS = {
    "iovec": [(I, 4), (OPL, 0)],
    "mixed": [(I, 1), (S, 1), (I, 2), (S, 2), (I, 4), (S, 4), (S, 8), (I, 8), (SKIP, 3), (OPL, 0), (I, 1), (S, 1),
              (I, 8), (RAWL, 0), (OP, 7), (RAW, 5), (S, 2)],
    "empty": [],
}
CASES = [("iovec", 20), ("mixed", 23), ("iovec", 23), ("mixed", 20)]


def _osch(schema):
    """The schema as the oracle takes it: SINT is INT there."""
    return [(I if k == S else k, z) for k, z in schema]


def _values(rng, schema, force):
    """Random field values; an integer that a length-driven field or a SKIP
    reads is drawn from LENS (`force`, unless None: the first such is that).  INT values are
    non-negative over the whole unsigned range, SINT values over the signed."""
    vals, last, f = [], None, 0
    while f < len(schema):
        kind, size = schema[f]
        if kind == SKIP:
            if last == 0:
                f += size
            f += 1
            continue
        nxt = schema[f + 1][0] if f + 1 < len(schema) else None
        if kind in (I, S):
            if nxt in (OPL, RAWL, SKIP):
                v = force if force is not None else int(rng.choice(LENS))
                force = None
            elif kind == S:
                v = int(rng.integers(-(1 << (8 * size - 1)), 1 << (8 * size - 1), dtype=np.int64))
            else:
                v = int(rng.integers(0, 1 << (8 * size), dtype=np.uint64))
            vals.append(v)
            last = v & ((1 << (8 * size)) - 1)
        else:
            n = last if kind in (OPL, RAWL) else size
            vals.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        f += 1
    return vals


def _parse_image(schema, img):
    """The values of a non-XDR image, or None when the schema does not consume
    it exactly."""
    pos, last, vals, f = 0, 0, [], 0
    while f < len(schema):
        kind, size = schema[f]
        f += 1
        if kind == SKIP:
            if last == 0:
                f += size
            continue
        if kind in (I, S):
            if pos + size > len(img):
                return None
            last = int.from_bytes(img[pos:pos + size], "little")
            vals.append(last - (1 << (8 * size)) if kind == S and last >> (8 * size - 1) else last)
            pos += size
            continue
        n = last if kind in (OPL, RAWL) else size
        if pos + n > len(img):
            return None
        vals.append(img[pos:pos + n])
        pos += n
    return vals if pos == len(img) else None


def _expect(O, schema, pay, method, src, soff, prefill, moff):
    """(the destination buffer after the call, the statuses): a message fits
    when the schema consumes its image exactly and its slot is pay + the
    oracle's wire length; then the wire and the hash are written, else
    nothing."""
    want, status, osch = prefill.copy(), np.ones(len(soff) - 1, dtype=np.uint8), _osch(schema)
    for i in range(len(soff) - 1):
        if soff[i + 1] < soff[i] or moff[i + 1] < moff[i]:
            continue
        img = src[soff[i]:soff[i + 1]].tobytes()
        vals = _parse_image(schema, img)
        if vals is None:
            continue
        wire = O.xdr_encode(osch, vals)
        assert O.xdr_hashed_stream(osch, wire) == img
        m0 = int(moff[i])
        if moff[i + 1] - m0 != pay + len(wire):
            continue
        want[m0 + pay:m0 + pay + len(wire)] = np.frombuffer(wire, dtype=np.uint8)
        want[m0 + HASH:m0 + HASH + 4] = np.frombuffer(int(O.crc(method, img)).to_bytes(4, "big"), dtype=np.uint8)
        status[i] = 0
    return want, status


def _table(sizes, lead=0):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    return off + lead


class Batch:
    """NMSG messages: values, oracle wires and images; entry 2i of the tables
    is message i, entry 2i + 1 a gap sized so that image i starts on residue
    i mod 16 and message i on residue (i // 16) mod 16."""

    def __init__(self, O, kind, pay, seed, count=NMSG, forced=_forced_len):
        self.kind, self.pay, self.schema = kind, pay, SCHEMAS[kind]
        self.rng = rng = np.random.default_rng(seed)
        osch = _osch(self.schema)
        self.values = [_values(rng, self.schema, forced(i)) for i in range(count)]
        self.wires = [O.xdr_encode(osch, v) for v in self.values]
        self.images = [O.xdr_hashed_stream(osch, w) for w in self.wires]
        self.parts, self.slots, spos, mpos = [], [], 0, 0
        for i in range(count):
            img, slot = self.images[i], pay + len(self.wires[i])
            spos, mpos = spos + len(img), mpos + slot
            gs, gm = (i + 1 - spos) % 16, ((i + 1) // 16 - mpos) % 16
            self.parts += [img, rng.integers(0, 256, gs, dtype=np.uint8).tobytes()]
            self.slots += [slot, gm]
            spos, mpos = spos + gs, mpos + gm
        assert max(self.slots[1::2]) < pay  # a gap never fits

    def tables(self):
        return _table([len(p) for p in self.parts]), _table(self.slots)

    def src(self, parts=None):
        return np.frombuffer(b"".join(parts or self.parts), dtype=np.uint8).copy()

    def prefill(self, moff, tail=37):
        """Sentinel bytes, random bytes where the real messages' headers are."""
        buf = np.full(int(moff[-1]) + tail, SENTINEL, dtype=np.uint8)
        for k in range(0, len(moff) - 1, 2):
            n = min(self.pay, int(moff[k + 1] - moff[k]))
            buf[moff[k]:moff[k] + n] = self.rng.integers(0, 256, n, dtype=np.uint8)
        return buf


_batches = {}


def _batch(O, kind, pay):
    if (kind, pay) not in _batches:
        _batches[kind, pay] = Batch(O, kind, pay, 2000 + pay + len(kind))
    return _batches[kind, pay]


def _dev(a, pad=0):
    import torch
    a = np.array(a)  # (a writable copy: torch takes no read-only arrays)
    t = torch.zeros(a.size + pad, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a))
    return t


def _pack_and_check(gpu, O, schema, pay, method, src, soff, prefill, moff, check_tables=True):
    """One call over fresh device copies, compared byte for byte; returns (data,
    device message table, expected statuses)."""
    import torch
    want, want_st = _expect(O, schema, pay, method, src, soff, prefill, moff)
    dsrc, data = _dev(src, 64), _dev(prefill)
    soffs, moffs = _dev(soff), _dev(moff)
    host = dict(src_offsets_host=soff, offsets_host=moff) if check_tables else {}
    st = gpu.pack_xdr_messages(method, dsrc, soffs, data, moffs, schema, payload_offset=pay, **host)
    torch.cuda.synchronize()
    got = data.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes of the buffer differ from the oracle's, first at {bad[:5]}"
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert np.array_equal(dsrc.cpu().numpy()[:src.size], src), "pack wrote to the source"
    return data, moffs, want_st


# ----------------------------------------------------------- exact bytes ----

def test_sign_and_zero_extension_by_hand(gpu, oracle_mod):
    """INT values with the top bit of their size set are zero-extended, negative
    SINT values sign-extended: the wire bytes written out by hand."""
    import torch
    schema = [(I, 1), (S, 1), (I, 2), (S, 2), (I, 4), (S, 4), (S, 8), (S, 1)]
    image = (bytes([0x80, 0x80]) + (0x8000).to_bytes(2, "little") + (0xFFFE).to_bytes(2, "little")
             + (0x80000000).to_bytes(4, "little") + (0xFFFFFFFF).to_bytes(4, "little")
             + (-2 & (2**64 - 1)).to_bytes(8, "little") + bytes([0x7F]))
    wire = bytes.fromhex("00000080 ffffff80 00008000 fffffffe 80000000 ffffffff fffffffffffffffe 0000007f")
    assert wire == oracle_mod.xdr_encode(_osch(schema), [0x80, -128, 0x8000, -2, 0x80000000, -1, -2, 0x7F])
    for layout in ("0", "1"):  # (integers only: no field reaches the step loop, whose loads MCHECKSUM_GPU_NT picks)
        os.environ["MCHECKSUM_GPU_XDR_FAST"] = layout
        try:
            gpu._lib().mchecksum_gpu_reload_settings()
            src, data = _dev(np.frombuffer(image, dtype=np.uint8), 64), torch.zeros(20 + len(wire), dtype=torch.uint8,
                                                                                      device="cuda")
            soffs, moffs = _dev(np.array([0, len(image)])), _dev(np.array([0, 20 + len(wire)]))
            st = gpu.pack_xdr_messages("crc32c", src, soffs, data, moffs, schema)
            assert st.tolist() == [0]
            got = data.cpu().numpy().tobytes()
            assert got[20:] == wire
            assert got[16:20] == int(oracle_mod.crc("crc32c", image)).to_bytes(4, "big") and got[:16] == bytes(16)
        finally:
            del os.environ["MCHECKSUM_GPU_XDR_FAST"]
            gpu._lib().mchecksum_gpu_reload_settings()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", ["crc32c", "crc32"])
@pytest.mark.parametrize("kind,pay", CASES)
def test_pack_writes_exactly_the_wire_and_the_hash(gpu, oracle_mod, kind, pay, method, layout, monkeypatch):
    _path(monkeypatch, layout)
    O = oracle_mod
    b = _batch(O, kind, pay)
    soff, moff = b.tables()
    if kind == "iovec":
        assert {(int(s) % 16, int(m) % 16) for s, m in zip(soff[0:-1:2], moff[0:-1:2])} == {
            (s, m) for s in range(16) for m in range(16)}
        # the body lies behind the u32 length on both sides: every ring length is read at an odd address
        # and, in one of the two iovec cases (the message starts of a parity differ by payload_offset),
        # stored at one
        odd = [{len(b.images[i]) - 4 for i in range(RING_AT, NMSG) if (soff[2 * i] + 4) % 2 and (moff[2 * i] + pay + 4) % 2 == p}
               for p in (0, 1)]
        assert odd[0] | odd[1] >= set(RING_LENS) and odd[0] and odd[1]
    else:
        # both extensions occur for every size below 8
        ints = [[v for (k, z), v in zip([e for e in b.schema if e[0] != SKIP], vals)] for vals in b.values]
        assert all(any(row[c] >= 1 << (8 * z - 1) for row in ints) for c, z in ((0, 1), (2, 2), (4, 4)))
        assert all(any(row[c] < 0 for row in ints) for c, z in ((1, 1), (3, 2), (5, 4)))
    _, _, st = _pack_and_check(gpu, O, b.schema, pay, method, b.src(), soff, b.prefill(moff), moff)
    assert not st[0::2].any() and st[1::2].all()  # every message packed, every gap entry refused


# ------------------------------------------------- the default count rule ----
# With no setting, a batch takes the throughput layout past 1024 messages and
# its non-temporal kernel from 8192 on (launch_plan.h: nt_by_count): 8192 is the
# smallest count that runs xdr_pack_fast_kernel<true> by itself, 8191 the
# largest that runs <false>.

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


@pytest.mark.parametrize("count", RULE_COUNTS)
def test_pack_by_the_default_count_rule(gpu, oracle_mod, count, monkeypatch):
    """Messages alone, no gap entries: entry i is message i.  Two do not fit
    (a 16 KiB body's slot a byte long, a tiny one's image a byte short); every
    byte of the buffer and every status as the oracle and the tables say."""
    monkeypatch.delenv("MCHECKSUM_GPU_XDR_FAST", raising=False)
    monkeypatch.delenv("MCHECKSUM_GPU_NT", raising=False)
    O = oracle_mod
    if "rule" not in _batches:
        # (payload_offset 23: a slot is 27 bytes and a multiple of 4, so the message starts take every residue)
        _batches["rule"] = Batch(O, "iovec", 23, 4343, count=RULE_COUNTS[-1], forced=_rule_len)
    b = _batches["rule"]
    images, slots = list(b.images[:count]), list(b.slots[0:2 * count:2])
    long16 = next(i for i in range(count) if len(images[i]) == 4 + 16384)
    slots[long16] += 1
    assert len(images[78]) > 4
    images[78] = images[78][:-1]
    # images from byte 0 on, messages from byte 7 on: both sides' starts fall on every residue mod 16
    soff, moff = _table([len(x) for x in images]), _table(slots, 7)
    assert {int(o) % 16 for o in soff[:-1]} == {int(o) % 16 for o in moff[:-1]} == set(range(16))
    prefill = np.full(int(moff[-1]) + 37, SENTINEL, dtype=np.uint8)
    _, _, st = _pack_and_check(gpu, O, b.schema, b.pay, "crc32c", b.src(images), soff, prefill, moff)
    assert np.nonzero(st)[0].tolist() == sorted([78, long16])


# ------------------------------------------------------------ round trip ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_round_trip_through_verify_and_unpack(gpu, oracle_mod, kind, pay, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O, method = oracle_mod, "crc32c"
    b = _batch(O, kind, pay)
    # the messages alone (no gap entries), so that every entry verifies
    soff, moff = _table([len(x) for x in b.images]), _table(b.slots[0::2])
    src = b.src(b.images)
    prefill = np.full(int(moff[-1]) + 16, SENTINEL, dtype=np.uint8)
    data, moffs, st = _pack_and_check(gpu, O, b.schema, pay, method, src, soff, prefill, moff)
    assert not st.any()
    vst, mism = gpu.verify_xdr_messages(method, data, moffs, b.schema, payload_offset=pay, offsets_host=moff)
    assert int(vst.sum().item()) == 0 and int(mism.item()) == 0
    dst = torch.full((src.size + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    ust, mism = gpu.unpack_xdr_messages(method, data, moffs, b.schema, dst, _dev(soff), payload_offset=pay,
                                        offsets_host=moff, dst_offsets_host=soff)
    torch.cuda.synchronize()
    assert int(ust.sum().item()) == 0 and int(mism.item()) == 0
    got = dst.cpu().numpy()
    assert np.array_equal(got[:src.size], src), "unpack did not return the source image"
    assert (got[src.size:] == SENTINEL).all()


# ----------------------------------------------------------- exact misfits ----

MISFITS = ("long", "short", "empty_slot", "trailing", "cut1", "half", "len_past", "below_pay")


def _misfit_case(O, b):
    """The batch with one message of each MISFITS kind: (src, soff, moff,
    {kind: entry index})."""
    parts, slots, idx = list(b.parts), list(b.slots), {}
    # messages whose image holds a length integer followed by at least 8 bytes
    at = 0 if b.kind == "iovec" else 1 + 1 + 2 + 2 + 4 + 4 + 8
    nlen = 4 if b.kind == "iovec" else 8
    whole = [i for i in range(20, NMSG) if int.from_bytes(b.images[i][at:at + nlen], "little") in (63, 64, 65, 255)]
    for what, i in zip(MISFITS, whole[::3]):
        k, img = 2 * i, b.images[i]
        idx[what] = k
        if what == "long":
            slots[k] += 1
        elif what == "short":
            slots[k] -= 1
        elif what == "empty_slot":
            slots[k] = 0
        elif what == "trailing":
            parts[k] = img + b"\0"
        elif what == "cut1":
            parts[k] = img[:-1]
        elif what == "half":
            parts[k] = img[:len(img) // 2]
        elif what == "len_past":
            n = int.from_bytes(img[at:at + nlen], "little") + 5
            parts[k] = img[:at] + n.to_bytes(nlen, "little") + img[at + nlen:]
        else:
            slots[k] = b.pay - 3
    assert len(idx) == len(MISFITS)
    return b.src(parts), _table([len(p) for p in parts]), _table(slots), idx


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_misfits_are_exact(gpu, oracle_mod, kind, pay, layout, monkeypatch):
    _path(monkeypatch, layout)
    O = oracle_mod
    b = _batch(O, kind, pay)
    src, soff, moff, idx = _misfit_case(O, b)
    _, _, st = _pack_and_check(gpu, O, b.schema, pay, "crc32c", src, soff, b.prefill(moff), moff)
    # by the oracle and the tables: the eight damaged messages, and the gap entries
    assert all(st[k] == 1 for k in idx.values())
    assert int(st[0::2].sum()) == len(MISFITS) and st[1::2].all()


# ----------------------------------------------------------------- sizes ----

@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_sizes_match_the_oracle(gpu, oracle_mod, kind, pay):
    import torch
    O = oracle_mod
    b = _batch(O, kind, pay)
    osch = _osch(b.schema)
    src, soff, moff, idx = _misfit_case(O, b)
    want = np.zeros(len(soff) - 1, dtype=np.int64)
    for i in range(len(want)):
        vals = _parse_image(b.schema, src[soff[i]:soff[i + 1]].tobytes())
        want[i] = -1 if vals is None else len(O.xdr_encode(osch, vals))
    assert (want[[idx[w] for w in ("trailing", "cut1", "half", "len_past")]] == -1).all()
    sizes, st = gpu.xdr_encoded_sizes(_dev(src, 64), _dev(soff), b.schema, src_offsets_host=soff)
    assert np.array_equal(st.cpu().numpy(), (want < 0).astype(np.uint8))
    assert np.array_equal(sizes.cpu().numpy(), np.maximum(want, 0))
    # the receiver's: sealed messages with slack behind them, three truncated, one shorter than its headers
    msgs = [bytes(pay) + w + bytes(i % 7) for i, w in enumerate(b.wires)]
    cut = [i for i in range(NMSG) if len(b.wires[i]) > 8][:3]
    msgs[cut[0]] = msgs[cut[0]][:pay + len(b.wires[cut[0]]) - 1]
    msgs[cut[1]] = msgs[cut[1]][:pay + len(b.wires[cut[1]]) - 5]
    msgs[cut[2]] = msgs[cut[2]][:pay + len(b.wires[cut[2]]) // 2]
    msgs[90] = msgs[90][:pay - 3]
    streams = [O.xdr_hashed_stream(osch, m[pay:]) if len(m) >= pay else None for m in msgs]
    assert sum(s is None for s in streams) == 4
    want_d = np.array([0 if s is None else len(s) for s in streams], dtype=np.int64)
    want_w = np.array([0 if s is None else len(w) for s, w in zip(streams, b.wires)], dtype=np.int64)
    off = _table([len(m) for m in msgs])
    dsz, wsz, st = gpu.xdr_decoded_sizes(_dev(np.frombuffer(b"".join(msgs), dtype=np.uint8), 64), _dev(off), b.schema,
                                         payload_offset=pay, offsets_host=off)
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), np.array([s is None for s in streams], dtype=np.uint8))
    assert np.array_equal(dsz.cpu().numpy(), want_d) and np.array_equal(wsz.cpu().numpy(), want_w)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_tables_from_the_size_calls_fit(gpu, oracle_mod, kind, pay, layout, monkeypatch):
    """Sender and receiver build their tables on the device (torch.cumsum of the
    size calls' results): every message fits, no host-side length is used."""
    import torch
    _path(monkeypatch, layout)
    O, method = oracle_mod, "crc32"
    b = _batch(O, kind, pay)
    src, soff = b.src(b.images), _table([len(x) for x in b.images])
    dsrc, soffs = _dev(src, 64), _dev(soff)
    sizes, st = gpu.xdr_encoded_sizes(dsrc, soffs, b.schema)
    assert int(st.sum().item()) == 0
    moffs = torch.zeros(NMSG + 1, dtype=torch.int64, device="cuda")
    moffs[1:] = torch.cumsum(sizes + pay, 0)
    # (an upper bound on the wire: every image byte in a 4-byte slot at the most, an 8-byte one in 8)
    data = torch.full((4 * src.size + NMSG * pay + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = gpu.pack_xdr_messages(method, dsrc, soffs, data, moffs, b.schema, payload_offset=pay)
    assert int(st.sum().item()) == 0
    assert np.array_equal(moffs.cpu().numpy(), _table(b.slots[0::2]))
    dsz, wsz, st = gpu.xdr_decoded_sizes(data, moffs, b.schema, payload_offset=pay)
    assert int(st.sum().item()) == 0 and torch.equal(wsz, sizes)
    doffs = torch.zeros(NMSG + 1, dtype=torch.int64, device="cuda")
    doffs[1:] = torch.cumsum(dsz, 0)
    assert torch.equal(doffs, soffs)
    dst = torch.full((src.size + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    st, mism = gpu.unpack_xdr_messages(method, data, moffs, b.schema, dst, doffs, payload_offset=pay)
    torch.cuda.synchronize()
    assert int(st.sum().item()) == 0 and int(mism.item()) == 0
    assert np.array_equal(dst.cpu().numpy()[:src.size], src)


# --------------------------------------------- empty batch, empty schema ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_empty_batch_and_empty_schema(gpu, oracle_mod, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O, schema = oracle_mod, SCHEMAS["iovec"]
    data = torch.zeros(64, dtype=torch.uint8, device="cuda")
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert gpu.pack_xdr_messages("crc32c", src, one, data, one, schema).numel() == 0
    assert all(t.numel() == 0 for t in gpu.xdr_encoded_sizes(src, one, schema))
    assert all(t.numel() == 0 for t in gpu.xdr_decoded_sizes(data, one, schema))
    # no fields: an empty image in a slot of exactly the headers is sealed with the CRC of nothing
    n, pay = 40, 20
    img = np.zeros(n, dtype=np.int64)
    img[[3, 17]] = (1, 9)      # non-empty images: misfits
    slots = np.full(n, pay, dtype=np.int64)
    slots[[5, 21]] = (pay + 1, pay - 1)
    soff, moff = _table(img, 3), _table(slots, 7)
    rng = np.random.default_rng(5)
    srcb = rng.integers(0, 256, int(soff[-1]), dtype=np.uint8)
    prefill = rng.integers(0, 256, int(moff[-1]) + 9, dtype=np.uint8)
    _, _, st = _pack_and_check(gpu, O, [], pay, "crc32c", srcb, soff, prefill, moff)
    assert st.tolist() == [int(i in (3, 17, 5, 21)) for i in range(n)]
    sizes, est = gpu.xdr_encoded_sizes(_dev(srcb, 64), _dev(soff), [])
    assert not sizes.any().item() and est.tolist() == [int(i in (3, 17)) for i in range(n)]


# ---------------------------------------------------------- graph replay ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_graph_replay_reads_current_contents(gpu, oracle_mod, layout, monkeypatch):
    """Captured after prepare(): a replay packs the source contents and follows
    both tables as they are at that moment."""
    import torch
    _path(monkeypatch, layout)
    O, method, pay = oracle_mod, "crc32c", 20
    gpu.prepare(method)
    b = _batch(O, "iovec", pay)
    src, soff = b.src(b.images), _table([len(x) for x in b.images])
    moff = _table(b.slots[0::2], 5)
    prefill = np.full(int(moff[-1]) + 24, SENTINEL, dtype=np.uint8)
    dsrc, data, soffs, moffs = _dev(src, 64), _dev(prefill), _dev(soff), _dev(moff)
    st = torch.ones(NMSG, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.pack_xdr_messages(method, dsrc, soffs, data, moffs, b.schema, payload_offset=pay, status=st)
    torch.cuda.synchronize()

    def replay_and_check(src, soff, moff):
        want, want_st = _expect(O, b.schema, pay, method, src, soff, prefill, moff)
        with torch.cuda.stream(s):
            dsrc[:src.size].copy_(torch.from_numpy(src))
            soffs.copy_(torch.from_numpy(soff))
            moffs.copy_(torch.from_numpy(moff))
            data.copy_(torch.from_numpy(prefill))
            st.fill_(1)
            g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(data.cpu().numpy(), want)
        assert np.array_equal(st.cpu().numpy(), want_st)
        return int(want_st.sum())

    assert replay_and_check(src, soff, moff) == 0
    # new contents of the same shape: every body byte changed
    src2 = src.copy()
    for i in range(NMSG):
        src2[soff[i] + 4:soff[i + 1]] ^= 0x5A
    assert replay_and_check(src2, soff, moff) == 0
    # new tables: image 12 loses its last byte to image 13, and slot 20 grows by one
    assert len(b.images[12]) > 4
    soff2, moff2 = soff.copy(), moff.copy()
    soff2[13] -= 1
    moff2[21:] += 1
    assert replay_and_check(src2, soff2, moff2) >= 2


# ------------------------------------------------ existing calls unchanged ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind,pay", CASES[:2])
def test_existing_calls_after_pack_and_with_sint(gpu, oracle_mod, kind, pay, layout, monkeypatch):
    import torch
    _path(monkeypatch, layout)
    O = oracle_mod
    b = _batch(O, kind, pay)
    osch = _osch(b.schema)
    src, soff, moff = b.src(b.images), _table([len(x) for x in b.images]), _table(b.slots[0::2])
    dsrc, soffs, moffs = _dev(src, 64), _dev(soff), _dev(moff)
    data = torch.zeros(int(moff[-1]) + 64, dtype=torch.uint8, device="cuda")
    assert int(gpu.pack_xdr_messages("crc32c", dsrc, soffs, data, moffs, b.schema, payload_offset=pay).sum().item()) == 0
    # checksum_xdr's messages start at the proc buffer
    boff = _table([len(w) for w in b.wires])
    bdata, boffs = _dev(np.frombuffer(b"".join(b.wires), dtype=np.uint8), 64), _dev(boff)
    for method in ("crc32c", "crc64"):
        want = [O.crc(method, x) for x in b.images]
        for schema in (osch, b.schema):
            got = gpu.as_unsigned(gpu.checksum_xdr(method, bdata, boffs, schema, offsets_host=boff))
            assert got.tolist() == want
    # SINT in place of INT: verify, seal and unpack as with INT
    for schema in (osch, b.schema):
        sealed = data.clone()
        sealed[_dev(moff[:-1] + HASH)] = 0
        assert int(gpu.seal_xdr_messages("crc32c", sealed, moffs, schema, payload_offset=pay).sum().item()) == 0
        assert torch.equal(sealed, data)
        vst, mism = gpu.verify_xdr_messages("crc32c", sealed, moffs, schema, payload_offset=pay)
        assert int(vst.sum().item()) == 0 and int(mism.item()) == 0
        dst = torch.zeros(src.size + 16, dtype=torch.uint8, device="cuda")
        ust, mism = gpu.unpack_xdr_messages("crc32c", sealed, moffs, schema, dst, soffs, payload_offset=pay)
        assert int(ust.sum().item()) == 0 and int(mism.item()) == 0
        assert np.array_equal(dst.cpu().numpy()[:src.size], src)


# ----------------------------------------------------------- fail closed ----

def test_pack_fault_fails_closed(gpu, oracle_mod, monkeypatch):
    """The fault-injecting build (build/libmchecksum_qfault.so) in its give-up
    mode, as test_gpu_xdr_messages.py::test_verify_fault_fails_closed:
    workgroup 3 drops one message of the throughput layout's queue.  The call
    returns 0, adds 1 to the error word and to the fault count, and every
    status reads 1 -- over a batch in which every message fits."""
    import torch
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    from mercury_amd._lib import XdrField
    L = ctypes.CDLL(QLIB)
    c = ctypes
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    L.mchecksum_gpu_pack_xdr_messages.argtypes = [c.c_char_p, c.POINTER(XdrField), c.c_size_t, c.c_void_p, c.c_void_p,
                                                  c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t,
                                                  c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_set_error_word.argtypes = [c.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = c.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    monkeypatch.delenv("MCHECKSUM_GPU_QFAULT_MODE", raising=False)  # the give-up, not a stall
    monkeypatch.delenv("MCHECKSUM_GPU_XDR_FAST", raising=False)     # > 1024 messages: the throughput layout
    L.mchecksum_gpu_reload_settings()
    try:
        pay, n = 20, 20000
        rng = np.random.default_rng(9)
        body = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
        images = [k.to_bytes(4, "little") + body[:k] for k in (0, 5, 64, 300)]
        wires = [oracle_mod.xdr_encode(SCHEMAS["iovec"], [k, body[:k]]) for k in (0, 5, 64, 300)]
        src = np.frombuffer(b"".join(images) * (n // 4), dtype=np.uint8)
        soff = _table([len(images[i % 4]) for i in range(n)])
        moff = _table([pay + len(wires[i % 4]) for i in range(n)])
        dsrc, soffs, moffs = _dev(src, 64), _dev(soff), _dev(moff)
        data = torch.zeros(int(moff[-1]) + 64, dtype=torch.uint8, device="cuda")
        fields = (XdrField * 2)(XdrField(I, 4), XdrField(OPL, 0))
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")  # stale "packed" everywhere
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        faults0 = L.mchecksum_gpu_queue_faults()
        assert L.mchecksum_gpu_prepare(b"crc32c") == 0
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_pack_xdr_messages(b"crc32c", fields, 2, dsrc.data_ptr(), soffs.data_ptr(),
                                                   data.data_ptr(), moffs.data_ptr(), n, pay, HASH, status.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        assert bool((status == 1).all().item())
    finally:
        monkeypatch.undo()
        L.mchecksum_gpu_reload_settings()
