"""Whole RPC messages of an XDR build by address list (include/mchecksum_gpu.h:
mchecksum_gpu_verify_rpc_xdr_message_list, _seal_, _unpack_, _pack_) on the GPU.

The messages are tests/test_gpu_rpc_xdr.py's: 70 of each kind over its
seven-entry schema, opaque lengths on both sides of the fast-field threshold,
every class in each batch, some with slack behind the schema's end.  Here they
lie as a drain leaves them: spread over three separate torch allocations,
listed in an order shuffled across the buffers, with gaps of 0..37 bytes of a
never-zero pattern, message starts at every residue mod 16, guard bands before
the first and behind the last message of a buffer.  Two entries have no bytes
at all: one of 7 bytes at address 0 (SHORT: its address is never used) and one
whose end wraps the address space (L = 0).

Two oracles.  The rules written out in test_gpu_rpc_xdr.py (model_*, over the
live oracle's xdr_hashed_stream, xdr_encode and crc) say what each message
must answer and hold afterwards; and the same messages laid contiguously go
through the table calls (verify_rpc_xdr_messages, ...), the wrapped entry as a
message of no bytes: statuses, counts and written bytes must agree with both,
bit for bit.  Whole buffers are compared, so every gap and guard byte too.

Arms: the latency layout, the throughput layout, and the throughput layout
with non-temporal loads (MCHECKSUM_GPU_XDR_FAST=0/1, MCHECKSUM_GPU_NT=1)."""
import functools

import numpy as np
import pytest

import test_gpu_rpc_xdr as X
from test_gpu_rpc_xdr import DEFERRED, FAULT, FRAME, HASH_AT, HEADER, INTENTS, KINDS, MISFIT, OK, PAYLOAD, SCHEMA, SHORT

pytestmark = pytest.mark.gpu

ARMS = ["0", "1", "1-nt"]
NBUF, GUARD = 3, 48
NULL_LEN = 7                                  # the entry at address 0
WRAP_ADDR, WRAP_LEN = (1 << 64) - 8, 64       # the entry whose end passes the end of the address space
N = X.COUNT + 2


def pattern(n, k=0):
    """The gap and guard bytes: never zero, so hashing one changes a CRC."""
    return ((np.arange(n, dtype=np.int64) * 7 + 13 + k) % 251 + 1).astype(np.uint8)


def _arr(m):
    return np.frombuffer(bytes(m), dtype=np.uint8).copy()


def _arm(monkeypatch, arm):
    monkeypatch.setenv("MCHECKSUM_GPU_XDR_FAST", arm[0])  # (this monkeypatch reloads the library's settings)
    if arm.endswith("-nt"):
        monkeypatch.setenv("MCHECKSUM_GPU_NT", "1")
    else:
        monkeypatch.delenv("MCHECKSUM_GPU_NT", raising=False)


class Lay:
    """One kind's batch in LIST order, read-only.  rx / blank / tx: the
    messages as received, as a sealing sender holds them (slack allowed), as a
    packing sender holds them; imgs, R: the other side.  where[p] = (buffer,
    start) of list entry p, or None for the two entries without bytes."""


def _place(rng, sizes, real):
    """Buffer (j * 5 + 1) % 3 for message j -- list neighbours are not memory neighbours --, an order of its own
    inside each buffer, gaps of 0..37 bytes."""
    where, buf_size = [None] * len(sizes), []
    for k in range(NBUF):
        mine = [p for p in range(len(sizes)) if real[p] and (p * 5 + 1) % NBUF == k]
        mine = [mine[j] for j in rng.permutation(len(mine))]
        at = GUARD + k
        for p in mine:
            at += int(rng.integers(0, 38))
            where[p] = (k, at)
            at += sizes[p]
        buf_size.append(at + GUARD)  # (no message lies flush against the end of its allocation)
    return where, buf_size


@functools.lru_cache(maxsize=None)
def lay_of(kind, shuffle=0):
    from oracle import oracle as O
    O.lib()
    b = X.batch_of(kind)
    pay, hash_ = FRAME[kind]
    rng = np.random.default_rng(20261021 + 97 * shuffle + KINDS.index(kind))
    v = Lay()
    v.kind = kind
    # entry order before the shuffle: the 70 messages, the NULL entry, the wrapped entry
    rx = [_arr(m) for m in b.rx] + [pattern(NULL_LEN, 5), np.zeros(0, dtype=np.uint8)]
    tx = [_arr(m) for m in b.tx] + [pattern(NULL_LEN, 5), np.zeros(0, dtype=np.uint8)]
    imgs = [_arr(m) for m in b.imgs] + [pattern(3, 1), pattern(5, 2)]
    R = [int(x) for x in np.diff(b.do.astype(np.int64))] + [3, 5]
    what = [INTENTS[i % len(INTENTS)] for i in range(X.COUNT)] + ["null", "wrap"]
    # the sealing sender's messages: the received ones with both hashes overwritten
    blank = [m.copy() for m in rx]
    for m in blank:
        if m.size >= 16:
            m[HASH_AT[kind]:HASH_AT[kind] + 2] = (0x5A, 0xC3)
        if m.size >= hash_ + 4:
            m[hash_:hash_ + 4] = (1, 2, 3, 4)
    order = rng.permutation(N)                # list position -> entry: the list is shuffled
    pick = lambda seq: [seq[j] for j in order]
    v.rx, v.tx, v.blank, v.imgs, v.R, v.what = pick(rx), pick(tx), pick(blank), pick(imgs), pick(R), pick(what)
    v.null, v.wrap = v.what.index("null"), v.what.index("wrap")
    real = [w not in ("null", "wrap") for w in v.what]
    v.rx_where, v.rx_size = _place(rng, [m.size for m in v.rx], real)
    v.tx_where, v.tx_size = _place(rng, [m.size for m in v.tx], real)
    starts = {v.rx_where[p][1] % 16 for p in range(N) if real[p]}
    assert starts == set(range(16)), "message starts miss a residue mod 16"
    v.do = np.cumsum([GUARD + 3] + v.R).astype(np.uint64)
    v.so = np.cumsum([GUARD + 3] + [m.size for m in v.imgs]).astype(np.uint64)
    v.dst0 = pattern(int(v.do[-1]) + GUARD, 3)
    v.src = pattern(int(v.so[-1]) + GUARD, 4)
    for p, m in enumerate(v.imgs):
        v.src[int(v.so[p]):int(v.so[p]) + m.size] = m
    # the model's answers, from the messages' bytes
    v.vwant = np.array([X.model_verify(O, m, kind)[0] for m in v.rx], dtype=np.uint8)
    v.uwant, v.udst = [], v.dst0.copy()
    for p, m in enumerate(v.rx):
        c, w = X.model_verify(O, m, kind, R=v.R[p])
        v.uwant.append(c)
        if w is not None:
            v.udst[int(v.do[p]):int(v.do[p + 1])] = np.frombuffer(w, dtype=np.uint8)
    v.uwant = np.array(v.uwant, dtype=np.uint8)
    sealed = [X.model_seal(O, m, kind) for m in v.blank]
    v.swant, v.sealed = np.array([c for c, _ in sealed], dtype=np.uint8), [_arr(m) for _, m in sealed]
    packed = [X.model_pack(O, m, kind, v.imgs[p]) for p, m in enumerate(v.tx)]
    v.pwant, v.packed = np.array([c for c, _ in packed], dtype=np.uint8), [_arr(m) for _, m in packed]
    # every class is in every batch, whatever the generator does
    assert set(v.vwant) == {OK, PAYLOAD, HEADER, SHORT, DEFERRED}
    assert set(v.uwant) == {OK, PAYLOAD, HEADER, SHORT, DEFERRED, MISFIT}
    assert set(v.swant) == {OK, SHORT, DEFERRED} and set(v.pwant) == {OK, SHORT, DEFERRED, MISFIT}
    for w in ("short15", "short_pay", "short_schema", "null", "wrap"):  # all three meanings of SHORT, and the two empty entries
        at = [p for p in range(N) if v.what[p] == w]
        assert at and all(v.vwant[p] == SHORT and v.uwant[p] == SHORT and v.swant[p] == SHORT for p in at), w
    assert all(v.pwant[p] == MISFIT for p in range(N) if v.what[p] in ("short_schema", "misfit_long", "misfit_short"))
    # (misfit_long: the schema does not consume the image; misfit_short: the message is not payload_offset + the XDR bytes)
    big = [p for p in range(N) if v.what[p] == "deferred_big"]
    assert big and all(v.vwant[p] == DEFERRED and v.uwant[p] == DEFERRED and v.pwant[p] == DEFERRED and
                       v.R[p] != v.rx[p].size - pay and v.imgs[p].size != v.tx[p].size - pay for p in big)
    return v


def scatter(where, size, msgs):
    """The three host buffers with `msgs` at their places, the pattern everywhere else."""
    bufs = [pattern(s, k) for k, s in enumerate(size)]
    for w, m in zip(where, msgs):
        if w is not None:
            bufs[w[0]][w[1]:w[1] + m.size] = m
    return bufs


def contiguous(msgs):
    """The same messages end to end at an odd base, in list order: (bytes, table)."""
    mo = np.zeros(len(msgs) + 1, dtype=np.uint64)
    mo[1:] = np.cumsum([m.size for m in msgs])
    mo += np.uint64(3)
    return np.concatenate([pattern(3)] + list(msgs) + [pattern(GUARD, 9)]), mo


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _table(t):
    import torch
    return torch.from_numpy(np.asarray(t).astype(np.uint64).view(np.int64).copy()).cuda()


def host_list(v, dev, where, msgs):
    """The two host arrays over the device buffers `dev`: addresses and lengths, the two empty entries among them."""
    ah, lh = np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.uint64)
    for p, w in enumerate(where):
        if w is not None:
            ah[p], lh[p] = dev[w[0]].data_ptr() + w[1], msgs[p].size
    ah[v.null], lh[v.null] = 0, NULL_LEN
    ah[v.wrap], lh[v.wrap] = WRAP_ADDR, WRAP_LEN
    return ah, lh


def device_list(v, where, bufs, msgs):
    """Three separate device allocations and the two arrays over them."""
    dev = [_dev(h) for h in bufs]
    assert len({t.data_ptr() for t in dev}) == NBUF
    ah, lh = host_list(v, dev, where, msgs)
    real = np.array([w is not None for w in where])
    assert np.any(np.diff(ah[real].astype(np.int64)) < 0), "the list is in address order"
    return dev, _table(ah), _table(lh), ah, lh


def counts_of(st, classes):
    return np.bincount(st, minlength=classes).astype(np.int32)


def same_buffers(dev, want, what):
    for k in range(NBUF):
        bad = np.nonzero(dev[k].cpu().numpy() != want[k])[0]
        assert bad.size == 0, f"buffer {k}: {bad.size} bytes differ from {what}, first at {bad[:4]}"


def frame(kind):
    pay, hash_ = FRAME[kind]
    return dict(kind=kind, payload_offset=pay, hash_offset=hash_)


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", KINDS)
def test_verify(gpu, monkeypatch, kind, arm):
    v = lay_of(kind)
    _arm(monkeypatch, arm)
    hbufs = scatter(v.rx_where, v.rx_size, v.rx)
    dev, addr, lens, ah, lh = device_list(v, v.rx_where, hbufs, v.rx)
    st, counts = gpu.verify_rpc_xdr_message_list(addr, lens, SCHEMA, addr_host=ah, len_host=lh, **frame(kind))
    got = st.cpu().numpy()
    assert np.array_equal(got, v.vwant), np.nonzero(got != v.vwant)[0][:8]
    assert counts.numel() == 6 and np.array_equal(counts.cpu().numpy(), counts_of(v.vwant, 6))
    same_buffers(dev, hbufs, "what they held: a verify wrote")
    cbuf, mo = contiguous(v.rx)
    tst, tcn = gpu.verify_rpc_xdr_messages(_dev(cbuf), _table(mo), SCHEMA, **frame(kind))
    assert np.array_equal(got, tst.cpu().numpy()) and np.array_equal(counts.cpu().numpy(), tcn.cpu().numpy())


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", KINDS)
def test_unpack(gpu, monkeypatch, kind, arm):
    v = lay_of(kind)
    _arm(monkeypatch, arm)
    hbufs = scatter(v.rx_where, v.rx_size, v.rx)
    dev, addr, lens, ah, lh = device_list(v, v.rx_where, hbufs, v.rx)
    dst, do = _dev(v.dst0), _table(v.do)
    st, counts = gpu.unpack_rpc_xdr_message_list(addr, lens, SCHEMA, dst, do, addr_host=ah, len_host=lh,
                                                 dst_offsets_host=v.do, **frame(kind))
    got = st.cpu().numpy()
    assert np.array_equal(got, v.uwant), np.nonzero(got != v.uwant)[0][:8]
    assert counts.numel() == 7 and np.array_equal(counts.cpu().numpy(), counts_of(v.uwant, 7))
    gd = dst.cpu().numpy()
    bad = np.nonzero(gd != v.udst)[0]  # (the DEFERRED, SHORT and MISFIT ranges and the guards keep their pattern)
    assert bad.size == 0, f"{bad.size} destination bytes differ from the model's, first at {bad[:4]}"
    same_buffers(dev, hbufs, "what they held: an unpack wrote")
    cbuf, mo = contiguous(v.rx)
    tdst = _dev(v.dst0)
    tst, tcn = gpu.unpack_rpc_xdr_messages(_dev(cbuf), _table(mo), SCHEMA, tdst, do, **frame(kind))
    assert np.array_equal(got, tst.cpu().numpy()) and np.array_equal(counts.cpu().numpy(), tcn.cpu().numpy())
    assert np.array_equal(gd, tdst.cpu().numpy())


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", KINDS)
def test_seal(gpu, monkeypatch, kind, arm):
    v = lay_of(kind)
    _arm(monkeypatch, arm)
    hbufs = scatter(v.rx_where, v.rx_size, v.blank)
    dev, addr, lens, ah, lh = device_list(v, v.rx_where, hbufs, v.blank)
    st = gpu.seal_rpc_xdr_message_list(addr, lens, SCHEMA, addr_host=ah, len_host=lh, **frame(kind))
    assert np.array_equal(st.cpu().numpy(), v.swant)
    same_buffers(dev, scatter(v.rx_where, v.rx_size, v.sealed), "the model's seal")
    cbuf, mo = contiguous(v.blank)
    cdev = _dev(cbuf)
    tst = gpu.seal_rpc_xdr_messages(cdev, _table(mo), SCHEMA, **frame(kind))
    assert np.array_equal(tst.cpu().numpy(), v.swant)
    assert np.array_equal(cdev.cpu().numpy(), contiguous(v.sealed)[0])
    # what it sealed, the receiver reads so through the same list
    rst, _ = gpu.verify_rpc_xdr_message_list(addr, lens, SCHEMA, **frame(kind))
    rst = rst.cpu().numpy()
    assert np.array_equal(rst[v.swant != SHORT], v.swant[v.swant != SHORT])


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("kind", KINDS)
def test_pack_and_round_trip(gpu, monkeypatch, kind, arm):
    v = lay_of(kind)
    _arm(monkeypatch, arm)
    hbufs = scatter(v.tx_where, v.tx_size, v.tx)
    dev, addr, lens, ah, lh = device_list(v, v.tx_where, hbufs, v.tx)
    src, so = _dev(v.src), _table(v.so)
    st = gpu.pack_rpc_xdr_message_list(src, so, addr, lens, SCHEMA, src_offsets_host=v.so, addr_host=ah, len_host=lh,
                                       **frame(kind))
    assert np.array_equal(st.cpu().numpy(), v.pwant)
    same_buffers(dev, scatter(v.tx_where, v.tx_size, v.packed), "the model's pack")  # XDR bytes, pads, 6 or 2 hash bytes
    assert np.array_equal(src.cpu().numpy(), v.src), "a pack wrote the source"
    cbuf, mo = contiguous(v.tx)
    cdev = _dev(cbuf)
    tst = gpu.pack_rpc_xdr_messages(src, so, cdev, _table(mo), SCHEMA, **frame(kind))
    assert np.array_equal(tst.cpu().numpy(), v.pwant)
    assert np.array_equal(cdev.cpu().numpy(), contiguous(v.packed)[0])
    # pack -> verify and unpack over the same list: OK / DEFERRED where packed, every OK image back
    done = np.isin(v.pwant, (OK, DEFERRED))
    rst, _ = gpu.verify_rpc_xdr_message_list(addr, lens, SCHEMA, **frame(kind))
    assert np.array_equal(rst.cpu().numpy()[done], v.pwant[done])
    back = _dev(pattern(v.src.size, 6))
    ust, _ = gpu.unpack_rpc_xdr_message_list(addr, lens, SCHEMA, back, so, **frame(kind))
    ust, back = ust.cpu().numpy(), back.cpu().numpy()
    assert np.array_equal(ust[done], v.pwant[done])
    for p in np.nonzero(v.pwant == OK)[0]:
        a, z = int(v.so[p]), int(v.so[p + 1])
        assert np.array_equal(back[a:z], v.src[a:z]), p


@pytest.mark.parametrize("arm", ["0", "1"])
def test_no_outputs_and_empty(gpu, monkeypatch, arm):
    """dev_status and dev_counts NULL: the bytes are written all the same.  count == 0: a valid call of each."""
    import torch
    kind = "request"
    v = lay_of(kind)
    _arm(monkeypatch, arm)
    hbufs = scatter(v.rx_where, v.rx_size, v.rx)
    dev, addr, lens, _, _ = device_list(v, v.rx_where, hbufs, v.rx)
    assert gpu.verify_rpc_xdr_message_list(addr, lens, SCHEMA, status=False, counts=False, **frame(kind)) == (False, False)
    dst, do = _dev(v.dst0), _table(v.do)
    none = gpu.unpack_rpc_xdr_message_list(addr, lens, SCHEMA, dst, do, status=False, counts=False, **frame(kind))
    assert none == (False, False) and np.array_equal(dst.cpu().numpy(), v.udst)
    hbufs = scatter(v.rx_where, v.rx_size, v.blank)
    dev, addr, lens, _, _ = device_list(v, v.rx_where, hbufs, v.blank)
    assert gpu.seal_rpc_xdr_message_list(addr, lens, SCHEMA, status=False, **frame(kind)) is False
    same_buffers(dev, scatter(v.rx_where, v.rx_size, v.sealed), "the model's seal")
    hbufs = scatter(v.tx_where, v.tx_size, v.tx)
    dev, addr, lens, _, _ = device_list(v, v.tx_where, hbufs, v.tx)
    assert gpu.pack_rpc_xdr_message_list(_dev(v.src), _table(v.so), addr, lens, SCHEMA, status=False, **frame(kind)) is False
    same_buffers(dev, scatter(v.tx_where, v.tx_size, v.packed), "the model's pack")
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    t1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    e8 = torch.zeros(0, dtype=torch.uint8, device="cuda")
    st, cn = gpu.verify_rpc_xdr_message_list(e, e, SCHEMA)
    assert st.numel() == 0 and cn.numel() == 6 and int(cn.sum().item()) == 0
    assert gpu.seal_rpc_xdr_message_list(e, e, SCHEMA).numel() == 0
    st, cn = gpu.unpack_rpc_xdr_message_list(e, e, SCHEMA, e8, t1)
    assert st.numel() == 0 and cn.numel() == 7 and int(cn.sum().item()) == 0
    assert gpu.pack_rpc_xdr_message_list(e8, t1, e, e, SCHEMA).numel() == 0


def test_wrapper_checks(gpu):
    """With host copies of the arrays the wrappers refuse written messages that overlap one another and a message
    that overlaps the other side, as the plain list wrappers do."""
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    other = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    addr, lens, ah, lh = gpu.rpc_message_list([(buf, 0, 100), (buf, 90, 100)], with_host=True)
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.seal_rpc_xdr_message_list(addr, lens, SCHEMA, addr_host=ah, len_host=lh)
    gpu.verify_rpc_xdr_message_list(addr, lens, SCHEMA, addr_host=ah, len_host=lh)  # (read only: they may)
    t = torch.tensor([0, 80, 160], dtype=torch.int64, device="cuda")
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.pack_rpc_xdr_message_list(other, t, addr, lens, SCHEMA, src_offsets_host=[0, 80, 160], addr_host=ah, len_host=lh)
    addr, lens, ah, lh = gpu.rpc_message_list([(buf, 0, 100), (buf, 200, 100)], with_host=True)
    with pytest.raises(gpu.GpuChecksumError, match="overlap"):
        gpu.unpack_rpc_xdr_message_list(addr, lens, SCHEMA, buf, t, addr_host=ah, len_host=lh,
                                        dst_offsets_host=[250, 330, 410])


@pytest.mark.parametrize("arm", ["0", "1"])
def test_graph_replay(gpu, monkeypatch, arm):
    """A verify and an unpack captured after prepare() of both methods.  A replay reads the arrays' current
    contents: rewritten in place to another shuffle of the messages in other allocations (the destination table
    with them), the same graph answers for those."""
    import torch
    kind = "request"
    _arm(monkeypatch, arm)
    gpu.prepare("crc32c")
    gpu.prepare("crc16")
    lays = [lay_of(kind), lay_of(kind, 1)]
    assert not np.array_equal(lays[0].vwant, lays[1].vwant) and lays[0].rx_where != lays[1].rx_where
    keep = []  # both drains' buffers stay allocated: the second lies elsewhere
    for v in lays:
        hbufs = scatter(v.rx_where, v.rx_size, v.rx)
        dev = [_dev(h) for h in hbufs]
        keep.append((dev, hbufs) + host_list(v, dev, v.rx_where, v.rx))
    assert not {t.data_ptr() for t in keep[0][0]} & {t.data_ptr() for t in keep[1][0]}
    addr, lens = _table(keep[0][2]), _table(keep[0][3])
    do = _table(lays[0].do)
    dst = torch.zeros(max(v.dst0.size for v in lays), dtype=torch.uint8, device="cuda")
    vst = torch.full((N,), FAULT, dtype=torch.uint8, device="cuda")
    ust = torch.full((N,), FAULT, dtype=torch.uint8, device="cuda")
    vcn = torch.zeros(6, dtype=torch.int32, device="cuda")
    ucn = torch.zeros(7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.verify_rpc_xdr_message_list(addr, lens, SCHEMA, status=vst, counts=vcn, **frame(kind))
        gpu.unpack_rpc_xdr_message_list(addr, lens, SCHEMA, dst, do, status=ust, counts=ucn, **frame(kind))
    torch.cuda.synchronize()
    for r, v in enumerate(lays):
        dev, hbufs, ah, lh = keep[r]
        with torch.cuda.stream(s):
            addr.copy_(torch.from_numpy(ah.view(np.int64)))
            lens.copy_(torch.from_numpy(lh.view(np.int64)))
            do.copy_(torch.from_numpy(v.do.view(np.int64)))
            dst[:v.dst0.size].copy_(torch.from_numpy(v.dst0))
            vst.fill_(FAULT)
            ust.fill_(FAULT)
            vcn.zero_()
            ucn.zero_()
            g.replay()
        s.synchronize()
        assert np.array_equal(vst.cpu().numpy(), v.vwant), r
        assert np.array_equal(vcn.cpu().numpy(), counts_of(v.vwant, 6)), r
        assert np.array_equal(ust.cpu().numpy(), v.uwant), r
        assert np.array_equal(ucn.cpu().numpy(), counts_of(v.uwant, 7)), r
        assert np.array_equal(dst[:v.dst0.size].cpu().numpy(), v.udst), r
        same_buffers(dev, hbufs, "what they held")
