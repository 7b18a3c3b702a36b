"""Whole RPC messages of an XDR build on the GPU (include/mchecksum_gpu.h:
mchecksum_gpu_verify_rpc_xdr_messages, _seal_, _unpack_, _pack_): every case
in the latency layout and in the throughput layout (MCHECKSUM_GPU_XDR_FAST=0/1),
both kinds, 70 messages -- more than a wave's lanes, five workgroups of the
throughput layout -- at mixed byte addresses, some with slack behind the
schema's end.

Expected values are worked out here, from the contract and the oracle alone
(oracle.xdr_encode, xdr_hashed_stream, crc): _ladder() reads a message's bytes
and says what each call must answer and write.  Every class is in each batch;
buffers are canaries with guard bands, and after a call every byte outside
what the ladder allows is unchanged and every byte inside is the CPU's."""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, PAYLOAD, HEADER, SHORT, DEFERRED, FAULT, MISFIT = range(7)
I, OP, OPL, RAW, RAWL, SKIP, S = 0, 1, 2, 3, 4, 5, 6  # MCHECKSUM_XDR_*
# u8, u32, a u64 length, the bytes unless it is 0, a raw field, a signed 16-bit integer
SCHEMA = [(I, 1), (I, 4), (I, 8), (SKIP, 1), (OPL, 0), (RAW, 6), (S, 2)]
OSCHEMA = [(I if k == S else k, z) for k, z in SCHEMA]  # the oracle's kinds: SINT is INT there
KINDS = ["request", "response"]
FRAME = {"request": (20, 16), "response": (23, 17)}  # payload_offset, hash_offset
FLAGS_AT = {"request": 10, "response": 1}
HASH_AT = {"request": 12, "response": 4}
COUNT, GUARD, CANARY = 70, 64, 0xA5
LAYOUTS = ["0", "1"]


def _fast_min():
    src = open(os.path.join(ROOT, "mercury_amd", "csrc", "mchecksum_gpu_ext.hip")).read()
    return int(re.search(r"constexpr uint64_t kXdrFastMin = (\d+);", src).group(1))


def _lens():
    k = _fast_min()
    return [0, 1, 3, 4, 5, 63, 64, 65, k - 1, k, k + 3]


def hdr_crc16(O, kind, h):
    """The core header's CRC-16: over the host-order field image."""
    if kind == "request":
        img = bytes(h[0:2]) + bytes(h[2:10])[::-1] + bytes(h[10:12])
    else:
        img = bytes(h[0:2]) + bytes(h[2:4])[::-1]
    return O.crc("crc16", img)


def _ladder(O, msg, kind):
    """What the bytes of one message are: (more, header good, stream or None).  stream: the decoded image of an
    eager message that holds payload_offset bytes and its own fields."""
    pay, _ = FRAME[kind]
    L = len(msg)
    if L < 16:
        return None
    more = bool(msg[FLAGS_AT[kind]] & 1)
    at = HASH_AT[kind]
    good = hdr_crc16(O, kind, msg) == int.from_bytes(bytes(msg[at:at + 2]), "big")
    stream = None if more or L < pay else O.xdr_hashed_stream(OSCHEMA, bytes(msg[pay:]))
    return more, good, stream


def model_verify(O, msg, kind, R=None):
    """The receiver's class; with R (unpack), also the bytes its destination range gets, or None."""
    pay, hash_ = FRAME[kind]
    f = _ladder(O, msg, kind)
    if f is None:
        return SHORT, None
    more, good, stream = f
    written = stream if stream is not None and R is not None and len(stream) == R else None
    if not good:
        return HEADER, written
    if more:
        return DEFERRED, None
    if stream is None:
        return SHORT, None
    if R is not None and len(stream) != R:
        return MISFIT, None
    ok = O.crc("crc32c", stream) == int.from_bytes(bytes(msg[hash_:hash_ + 4]), "big")
    return (OK if ok else PAYLOAD), written


def model_seal(O, msg, kind):
    """The sender's class in place, and the message afterwards."""
    pay, hash_ = FRAME[kind]
    out = bytearray(msg)
    f = _ladder(O, msg, kind)
    if f is None:
        return SHORT, out
    more, _, stream = f
    if not more and stream is None:
        return SHORT, out
    if not more:
        out[hash_:hash_ + 4] = O.crc("crc32c", stream).to_bytes(4, "big")
    out[HASH_AT[kind]:HASH_AT[kind] + 2] = hdr_crc16(O, kind, out).to_bytes(2, "big")
    return (DEFERRED if more else OK), out


def _parse_image(img):
    """The values of a non-XDR image of SCHEMA, or None when the schema does not consume it exactly."""
    pos, last, vals, f = 0, 0, [], 0
    while f < len(SCHEMA):
        kind, size = SCHEMA[f]
        f += 1
        if kind == SKIP:
            if last == 0:
                f += size
            continue
        n = size if kind in (I, S, RAW) else last
        if pos + n > len(img):
            return None
        if kind in (I, S):
            last = int.from_bytes(img[pos:pos + n], "little")
            vals.append(last - (1 << (8 * n)) if kind == S and last >> (8 * n - 1) else last)
        else:
            vals.append(bytes(img[pos:pos + n]))
        pos += n
    return vals if pos == len(img) else None


def model_pack(O, msg, kind, img):
    pay, hash_ = FRAME[kind]
    out = bytearray(msg)
    L = len(msg)
    if L < 16:
        return SHORT, out
    if msg[FLAGS_AT[kind]] & 1:
        out[HASH_AT[kind]:HASH_AT[kind] + 2] = hdr_crc16(O, kind, out).to_bytes(2, "big")
        return DEFERRED, out
    if L < pay:
        return SHORT, out
    vals = _parse_image(bytes(img))
    wire = O.xdr_encode(OSCHEMA, vals) if vals is not None else None
    if wire is None or L != pay + len(wire):
        return MISFIT, out
    out[pay:] = wire
    out[hash_:hash_ + 4] = O.crc("crc32c", bytes(img)).to_bytes(4, "big")
    out[HASH_AT[kind]:HASH_AT[kind] + 2] = hdr_crc16(O, kind, out).to_bytes(2, "big")
    return OK, out


def _values(rng, n):
    v = [int(rng.integers(0, 256)), int(rng.integers(0, 1 << 32)), n]
    if n:
        v.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    return v + [rng.integers(0, 256, 6, dtype=np.uint8).tobytes(), -int(rng.integers(1, 1 << 15))]


class Batch:
    """70 messages of one kind.  rx: as received (sealed by the model, then damaged by intent), with the
    destination table of an unpack; tx: blank headers and the images of a pack."""


# what message i is meant to be (the expectation never reads this: _ladder reads the bytes)
INTENTS = ["ok", "ok", "payload", "ok", "header", "ok", "header_more", "short15", "ok", "short_pay", "short_schema", "ok",
           "deferred16", "deferred_big", "misfit_long", "ok", "misfit_short", "ok", "slack", "ok"]


@functools.lru_cache(maxsize=None)
def batch_of(kind):
    from oracle import oracle as O
    O.lib()
    rng = np.random.default_rng(20240611 + KINDS.index(kind))
    pay, hash_ = FRAME[kind]
    lens = _lens()
    b = Batch()
    rx, tx, imgs, R = [], [], [], []
    for i in range(COUNT):
        what = INTENTS[i % len(INTENTS)]
        n = lens[(i * 7 + i // len(INTENTS)) % len(lens)]
        vals = _values(rng, n)
        wire = O.xdr_encode(OSCHEMA, vals)
        img = O.xdr_hashed_stream(OSCHEMA, wire)
        assert _parse_image(img) == vals
        head = bytearray(rng.integers(0, 256, pay, dtype=np.uint8).tobytes())
        head[FLAGS_AT[kind]] &= 0xFE
        msg = head + bytearray(wire)
        if what == "slack":
            msg += rng.integers(0, 256, 1 + i % 5, dtype=np.uint8).tobytes()  # bytes behind the schema's end
        if what in ("header_more", "deferred16", "deferred_big"):
            msg[FLAGS_AT[kind]] |= 1
        if what == "short15":
            msg = msg[:15]
        elif what == "short_pay":
            msg = msg[:pay - 1]
        elif what == "short_schema":
            msg = msg[:-1]  # the schema runs one byte past the end
        elif what == "deferred16":
            msg = msg[:16]
        elif what == "deferred_big":
            msg = msg[:16] + bytearray(rng.integers(0, 256, 333, dtype=np.uint8).tobytes())  # garbage behind the header
        # sender side: the blank message (hashes unset) and its image
        blank = bytearray(msg)
        if what == "slack":
            blank = blank[:pay + len(wire)]  # (the sender's messages carry no slack)
        image = bytearray(img)
        if what == "misfit_long":
            image += b"\x00"
        elif what == "misfit_short":
            blank = blank[:-1]
        tx.append(blank)
        imgs.append(image)
        # receiver side: sealed by the model, then damaged
        _, sealed = model_seal(O, msg, kind)
        if len(sealed) >= 16:  # (a SHORT message too arrives under a good header)
            sealed[HASH_AT[kind]:HASH_AT[kind] + 2] = hdr_crc16(O, kind, sealed).to_bytes(2, "big")
        if what == "payload":
            sealed[pay + 4 + (i % 4)] ^= 1 << (i % 8)      # one bit of the u32
        elif what in ("header", "header_more"):
            sealed[3] ^= 0x10                               # one bit of the id / the cookie
        rx.append(sealed)
        R.append(len(img) + (1 if what == "misfit_long" else -1 if what == "misfit_short" else 0))
    b.rx, b.tx, b.imgs = rx, tx, imgs

    def table(parts, base):
        return np.cumsum([base] + [len(p) for p in parts]).astype(np.uint64)

    b.mo, b.to = table(rx, GUARD + 1), table(tx, GUARD + 1)      # the first message starts at an odd address
    b.do, b.so = np.cumsum([GUARD + 3] + R).astype(np.uint64), table(imgs, GUARD + 3)

    def flat(parts, off):
        a = np.full(int(off[-1]) + GUARD, CANARY, dtype=np.uint8)
        for p, o in zip(parts, off):
            a[int(o):int(o) + len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        return a

    b.rx_buf, b.tx_buf, b.src_buf = flat(rx, b.mo), flat(tx, b.to), flat(imgs, b.so)
    b.dst0 = np.full(int(b.do[-1]) + GUARD, CANARY, dtype=np.uint8)
    return b


def _msgs(buf, off):
    return [buf[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def expect_verify(O, buf, off, kind):
    return np.array([model_verify(O, m, kind)[0] for m in _msgs(buf, off)], dtype=np.uint8)


def expect_unpack(O, buf, off, kind, dst0, do):
    want, dst = [], dst0.copy()
    for i, m in enumerate(_msgs(buf, off)):
        c, w = model_verify(O, m, kind, R=int(do[i + 1] - do[i]))
        want.append(c)
        if w is not None:
            dst[int(do[i]):int(do[i + 1])] = np.frombuffer(w, dtype=np.uint8)
    return np.array(want, dtype=np.uint8), dst


def expect_seal(O, buf, off, kind):
    want, out = [], buf.copy()
    for i, m in enumerate(_msgs(buf, off)):
        c, after = model_seal(O, m, kind)
        want.append(c)
        out[int(off[i]):int(off[i + 1])] = np.frombuffer(bytes(after), dtype=np.uint8)
    return np.array(want, dtype=np.uint8), out


def expect_pack(O, buf, off, kind, src, so):
    want, out = [], buf.copy()
    for i, m in enumerate(_msgs(buf, off)):
        c, after = model_pack(O, m, kind, src[int(so[i]):int(so[i + 1])])
        want.append(c)
        out[int(off[i]):int(off[i + 1])] = np.frombuffer(bytes(after), dtype=np.uint8)
    return np.array(want, dtype=np.uint8), out


def counts_of(st, classes):
    return np.bincount(st, minlength=classes).astype(np.int32)


def _dev(a):
    import torch
    return torch.from_numpy(a.copy()).cuda()


def _table(t):
    import torch
    return torch.from_numpy(np.asarray(t).astype(np.int64)).cuda()


def _layout(monkeypatch, layout):
    monkeypatch.setenv("MCHECKSUM_GPU_XDR_FAST", layout)  # (this monkeypatch reloads the library's settings, and restores them)


def _changed(a, b):
    return int(np.count_nonzero(a != b))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_verify(gpu, oracle_mod, monkeypatch, kind, layout):
    O, b = oracle_mod, batch_of(kind)
    _layout(monkeypatch, layout)
    pay, hash_ = FRAME[kind]
    want = expect_verify(O, b.rx_buf, b.mo, kind)
    assert set(want) == {OK, PAYLOAD, HEADER, SHORT, DEFERRED}
    # a corrupt header under MORE_DATA is HEADER; both SHORT rules and the schema's; DEFERRED at L = 16 and large
    for i in range(COUNT):
        what = INTENTS[i % len(INTENTS)]
        assert want[i] == {"payload": PAYLOAD, "header": HEADER, "header_more": HEADER, "short15": SHORT, "short_pay": SHORT,
                           "short_schema": SHORT, "deferred16": DEFERRED, "deferred_big": DEFERRED}.get(what, OK), (i, what)
    data, mo = _dev(b.rx_buf), _table(b.mo)
    st, counts = gpu.verify_rpc_xdr_messages(data, mo, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_)
    assert np.array_equal(st.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), counts_of(want, 6))
    assert np.array_equal(data.cpu().numpy(), b.rx_buf)
    # the two-call route: the header verdict on every message; the payload verdict on the eager, header-good ones
    hst, _ = gpu.verify_core_headers(data, mo, kind=kind)
    assert np.array_equal(hst.cpu().numpy()[[len(m) >= 16 for m in b.rx]] != 0,
                          (want == HEADER)[[len(m) >= 16 for m in b.rx]])
    xst, _ = gpu.verify_xdr_messages("crc32c", data, mo, SCHEMA, payload_offset=pay, hash_offset=hash_)
    both = np.isin(want, (OK, PAYLOAD, SHORT)) & np.array([len(m) >= 16 for m in b.rx])
    assert np.array_equal(xst.cpu().numpy()[both] != 0, want[both] != OK)
    # either output may be left out
    st2, none = gpu.verify_rpc_xdr_messages(data, mo, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_, counts=False)
    assert none is False and np.array_equal(st2.cpu().numpy(), want)
    none, c2 = gpu.verify_rpc_xdr_messages(data, mo, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_, status=False)
    assert none is False and np.array_equal(c2.cpu().numpy(), counts_of(want, 6))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_unpack(gpu, oracle_mod, monkeypatch, kind, layout):
    O, b = oracle_mod, batch_of(kind)
    _layout(monkeypatch, layout)
    pay, hash_ = FRAME[kind]
    want, want_dst = expect_unpack(O, b.rx_buf, b.mo, kind, b.dst0, b.do)
    assert set(want) == {OK, PAYLOAD, HEADER, SHORT, DEFERRED, MISFIT}
    # decoded as received: a PAYLOAD message's range and a fitting HEADER message's are written, no other bad one's
    for i in range(COUNT):
        wrote = _changed(want_dst[int(b.do[i]):int(b.do[i + 1])], b.dst0[int(b.do[i]):int(b.do[i + 1])]) > 0
        what = INTENTS[i % len(INTENTS)]
        assert wrote == (want[i] in (OK, PAYLOAD) or what == "header"), (i, what)
    data, mo, dst, do = _dev(b.rx_buf), _table(b.mo), _dev(b.dst0), _table(b.do)
    st, counts = gpu.unpack_rpc_xdr_messages(data, mo, SCHEMA, dst, do, kind=kind, payload_offset=pay, hash_offset=hash_)
    assert np.array_equal(st.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), counts_of(want, 7))
    assert np.array_equal(dst.cpu().numpy(), want_dst)  # guard bands and skipped ranges included
    assert np.array_equal(data.cpu().numpy(), b.rx_buf)
    dst2 = _dev(b.dst0)
    none, none2 = gpu.unpack_rpc_xdr_messages(data, mo, SCHEMA, dst2, do, kind=kind, payload_offset=pay, hash_offset=hash_,
                                              status=False, counts=False)
    assert none is False and none2 is False and np.array_equal(dst2.cpu().numpy(), want_dst)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_seal(gpu, oracle_mod, monkeypatch, kind, layout):
    O, b = oracle_mod, batch_of(kind)
    _layout(monkeypatch, layout)
    pay, hash_ = FRAME[kind]
    # the sender's messages with slack allowed: the received ones with both hashes overwritten
    blank = b.rx_buf.copy()
    for i in range(COUNT):
        m0, L = int(b.mo[i]), len(b.rx[i])
        if L >= 16:
            blank[m0 + HASH_AT[kind]:m0 + HASH_AT[kind] + 2] = (0x5A, 0xC3)
        if L >= hash_ + 4:
            blank[m0 + hash_:m0 + hash_ + 4] = (1, 2, 3, 4)
    want, want_buf = expect_seal(O, blank, b.mo, kind)
    assert set(want) == {OK, SHORT, DEFERRED}
    for i in range(COUNT):  # exactly 6, 2 or 0 bytes of a message may change
        a, z = int(b.mo[i]), int(b.mo[i + 1])
        assert _changed(want_buf[a:z], blank[a:z]) <= {OK: 6, DEFERRED: 2, SHORT: 0}[want[i]]
    data, mo = _dev(blank), _table(b.mo)
    st = gpu.seal_rpc_xdr_messages(data, mo, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_)
    assert np.array_equal(st.cpu().numpy(), want)
    assert np.array_equal(data.cpu().numpy(), want_buf)
    # what it sealed, the receiver reads so: OK and DEFERRED, and SHORT where nothing was written
    rst, _ = gpu.verify_rpc_xdr_messages(data, mo, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_)
    rst = rst.cpu().numpy()
    assert np.array_equal(rst[want != SHORT], want[want != SHORT])
    data2 = _dev(blank)
    assert gpu.seal_rpc_xdr_messages(data2, mo, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_, status=False) is False
    assert np.array_equal(data2.cpu().numpy(), want_buf)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_pack_and_round_trip(gpu, oracle_mod, monkeypatch, kind, layout):
    O, b = oracle_mod, batch_of(kind)
    _layout(monkeypatch, layout)
    pay, hash_ = FRAME[kind]
    want, want_buf = expect_pack(O, b.tx_buf, b.to, kind, b.src_buf, b.so)
    assert set(want) == {OK, SHORT, DEFERRED, MISFIT}
    for i in range(COUNT):
        what = INTENTS[i % len(INTENTS)]
        assert want[i] == {"short15": SHORT, "short_pay": SHORT, "short_schema": MISFIT, "deferred16": DEFERRED,
                           "deferred_big": DEFERRED, "header_more": DEFERRED, "misfit_long": MISFIT,
                           "misfit_short": MISFIT}.get(what, OK), (i, what)
    data, to, src, so = _dev(b.tx_buf), _table(b.to), _dev(b.src_buf), _table(b.so)
    st = gpu.pack_rpc_xdr_messages(src, so, data, to, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_)
    assert np.array_equal(st.cpu().numpy(), want)
    assert np.array_equal(data.cpu().numpy(), want_buf)  # XDR bytes, pads, 6 or 2 hash bytes; every other byte as it was
    assert np.array_equal(src.cpu().numpy(), b.src_buf)
    # pack -> verify: all OK / DEFERRED where packed
    rst, _ = gpu.verify_rpc_xdr_messages(data, to, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_)
    rst = rst.cpu().numpy()
    done = np.isin(want, (OK, DEFERRED))
    assert np.array_equal(rst[done], want[done])
    # pack -> unpack returns the source images
    back0 = np.full(b.src_buf.size, CANARY, dtype=np.uint8)
    back = _dev(back0)
    ust, _ = gpu.unpack_rpc_xdr_messages(data, to, SCHEMA, back, so, kind=kind, payload_offset=pay, hash_offset=hash_)
    ust, back = ust.cpu().numpy(), back.cpu().numpy()
    assert np.array_equal(ust[done], want[done])
    for i in range(COUNT):
        a, z = int(b.so[i]), int(b.so[i + 1])
        if want[i] == OK:
            assert np.array_equal(back[a:z], b.src_buf[a:z]), i
        elif ust[i] not in (OK, PAYLOAD, HEADER):
            assert np.all(back[a:z] == CANARY), i
    data2 = _dev(b.tx_buf)
    assert gpu.pack_rpc_xdr_messages(src, so, data2, to, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_,
                                     status=False) is False
    assert np.array_equal(data2.cpu().numpy(), want_buf)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_graph_replay(gpu, oracle_mod, monkeypatch, layout):
    """verify and pack captured after prepare() of both methods: each replay reads the buffers' current contents."""
    import torch
    O, kind = oracle_mod, "request"
    _layout(monkeypatch, layout)
    gpu.prepare("crc32c")
    gpu.prepare("crc16")
    b = batch_of(kind)
    pay, hash_ = FRAME[kind]
    rx, mo = _dev(b.rx_buf), _table(b.mo)
    tx, to, src, so = _dev(b.tx_buf), _table(b.to), _dev(b.src_buf), _table(b.so)
    vst = torch.full((COUNT,), FAULT, dtype=torch.uint8, device="cuda")
    pst = torch.full((COUNT,), FAULT, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(6, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.verify_rpc_xdr_messages(rx, mo, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_, status=vst, counts=counts)
        gpu.pack_rpc_xdr_messages(src, so, tx, to, SCHEMA, kind=kind, payload_offset=pay, hash_offset=hash_, status=pst)
    torch.cuda.synchronize()
    hrx, htx, hsrc = b.rx_buf.copy(), b.tx_buf.copy(), b.src_buf.copy()
    for r in range(2):
        k = (1, 3)[r]                                       # an OK message of both batches
        hrx[int(b.mo[k]) + FLAGS_AT[kind]] ^= 1             # its flags byte: inside the header's image -> HEADER
        hrx[int(b.mo[k + 20]) + pay + 5] ^= 0x40            # a payload byte of another -> PAYLOAD
        htx[int(b.to[k]) + FLAGS_AT[kind]] ^= 1             # the sender's message becomes DEFERRED
        hsrc[int(b.so[k + 20]) + 2] ^= 0x11                 # a byte of an image's u32
        want_v = expect_verify(O, hrx, b.mo, kind)
        want_p, want_tx = expect_pack(O, htx, b.to, kind, hsrc, b.so)
        assert want_v[k] == HEADER and want_v[k + 20] == PAYLOAD and want_p[k] == DEFERRED and want_p[k + 20] == OK
        with torch.cuda.stream(s):
            rx.copy_(torch.from_numpy(hrx))
            tx.copy_(torch.from_numpy(htx))
            src.copy_(torch.from_numpy(hsrc))
            vst.fill_(FAULT)
            pst.fill_(FAULT)
            counts.zero_()
            g.replay()
        s.synchronize()
        assert np.array_equal(vst.cpu().numpy(), want_v), r
        assert np.array_equal(counts.cpu().numpy(), counts_of(want_v, 6)), r
        assert np.array_equal(pst.cpu().numpy(), want_p), r
        assert np.array_equal(tx.cpu().numpy(), want_tx), r
