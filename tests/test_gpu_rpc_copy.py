"""Whole RPC messages with the payload moved in the same pass
(include/mchecksum_gpu.h): mchecksum_gpu_unpack_rpc_messages and
mchecksum_gpu_pack_rpc_messages -- the receiver's and the sender's rules of
verify_rpc_messages / seal_rpc_messages with unpack_messages' / pack_messages'
copy, in one launch.  Every expected status and byte comes from the live
oracle's CRCs, over the field image this file builds from the wire bytes and
over the payloads; the rules are written out here (`model_unpack`,
`model_pack`, `seal_in_place`), not taken from the library."""
import ctypes
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLIB = os.path.join(ROOT, "build", "libmchecksum_qfault.so")
OK, PAYLOAD, HEADER, SHORT, DEFERRED, FAULT, MISFIT, CLASSES = range(8)
PAY, HASH = 20, 16
LENS = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 4096, 4097, 65541)
COUNT = 193
BASE = 3                                        # the message buffer's odd base
OBASE = 5                                       # ... and the other buffer's own (destination of an unpack, source of a pack)
RUNTS = {7: 0, 60: 15, 100: 16, 131: 19}        # message sizes; the last two are eager and hold a whole core header
DEFER = {20: 0, 33: 3, 46: 4, 59: 40, 72: 24, 85: 4, 98: 52, 111: 28}  # MORE_DATA set: bytes behind the core header
RUNT_R, DEFER_R = 3, 7                          # their ranges on the other side: never touched, whatever their size
DEFER_FITS = 59                                 # ... but this one's would fit, were the message eager (16 + 40 = PAY + 36)
MISFITS = {10: +1, 37: -1, 64: None, 150: +1, 171: -1}  # R = L - PAY + 1 / - 1; None: R = 0 for a non-empty payload
LAYOUTS = [("0", None), ("1", None), ("0", "1")]  # full, light, non-temporal
KINDS = ("request", "response")
FLAGS_AT = {"request": 10, "response": 1}
HASH_AT = {"request": 12, "response": 4}
COVERED = {"request": 12, "response": 4}        # image bytes; the hash's own two bytes follow them
GUARD = 16                                      # bytes kept behind the last range of every buffer


def image(kind, h):
    """The host-order field image hg_core_header_*_proc hashes, from the 16 wire bytes."""
    if kind == "request":  # hg, protocol, id (u64, big-endian on the wire), flags, cookie
        return bytes(h[0:2]) + struct.pack("<Q", struct.unpack(">Q", bytes(h[2:10]))[0]) + bytes(h[10:12])
    return bytes(h[0:2]) + struct.pack("<H", struct.unpack(">H", bytes(h[2:4]))[0])  # ret_code, flags, cookie (u16)


def _be(fmt, v):
    return np.frombuffer(struct.pack(fmt, v), dtype=np.uint8)


def _range(tab, i):
    """(start, length) of range i; a table that runs backwards holds an empty range."""
    a, e = int(tab[i]), int(tab[i + 1])
    return a, max(e - a, 0)


def model_unpack(O, buf, mo, t, dst0, kind, hm="crc16", pm="crc32c"):
    """The receiver: (statuses, the destination's bytes, a mask of the bytes written)."""
    dst, wrote = dst0.copy(), np.zeros(dst0.size, dtype=bool)
    out = np.zeros(len(mo) - 1, dtype=np.uint8)
    for i in range(len(mo) - 1):
        a, L = _range(mo, i)
        d, R = _range(t, i)
        more = L >= 16 and bool(buf[a + FLAGS_AT[kind]] & 1)
        # what is written does not wait for the verdicts
        fits = L >= 16 and not more and L >= PAY and L == PAY + R
        if fits:
            dst[d:d + R] = buf[a + PAY:a + L]
            wrote[d:d + R] = True
        # the status: the first rule that matches
        if L < 16:
            out[i] = SHORT
            continue
        at = a + HASH_AT[kind]
        if O.crc(hm, image(kind, buf[a:a + 16])) != int(buf[at]) << 8 | int(buf[at + 1]):
            out[i] = HEADER
        elif more:
            out[i] = DEFERRED
        elif L < PAY:
            out[i] = SHORT
        elif L != PAY + R:
            out[i] = MISFIT
        elif O.crc(pm, buf[a + PAY:a + L]) != struct.unpack(">I", bytes(buf[a + HASH:a + HASH + 4]))[0]:
            out[i] = PAYLOAD
    return out, dst, wrote


def model_pack(O, blank, mo, src, t, kind, hm="crc16", pm="crc32c"):
    """The sender: (the packed bytes, statuses, a mask of the bytes a pack may write)."""
    buf, may = blank.copy(), np.zeros(blank.size, dtype=bool)
    out = np.zeros(len(mo) - 1, dtype=np.uint8)
    for i in range(len(mo) - 1):
        a, L = _range(mo, i)
        s, R = _range(t, i)
        if L < 16:
            out[i] = SHORT
            continue
        at = a + HASH_AT[kind]
        if buf[a + FLAGS_AT[kind]] & 1:
            out[i] = DEFERRED
        elif L < PAY:
            out[i] = SHORT
            continue
        elif L != PAY + R:
            out[i] = MISFIT
            continue
        else:
            buf[a + PAY:a + L] = src[s:s + R]
            buf[a + HASH:a + HASH + 4] = _be(">I", O.crc(pm, src[s:s + R]))
            may[a + PAY:a + L] = True
            may[a + HASH:a + HASH + 4] = True
        buf[at:at + 2] = _be(">H", O.crc(hm, image(kind, buf[a:a + 16])))
        may[at:at + 2] = True
    return buf, out, may


def seal_in_place(O, blank, mo, kind, hm="crc16", pm="crc32c"):
    """A correct sender's batch with the payloads already in place: both hashes
    of an eager message that holds its headers, the header's of a deferred one."""
    buf = blank.copy()
    for i in range(len(mo) - 1):
        a, L = _range(mo, i)
        if L < 16:
            continue
        more = bool(buf[a + FLAGS_AT[kind]] & 1)
        if not more and L < PAY:
            continue
        if not more:
            buf[a + HASH:a + HASH + 4] = _be(">I", O.crc(pm, buf[a + PAY:a + L]))
        at = a + HASH_AT[kind]
        buf[at:at + 2] = _be(">H", O.crc(hm, image(kind, buf[a:a + 16])))
    return buf


def sentinel(n):
    return ((np.arange(n, dtype=np.int64) * 7 + 13) % 251).astype(np.uint8)


class Batch:
    """193 messages of one kind in one buffer at an odd base, on the host,
    read-only: `blank` (every header byte filled, the two hashes and the
    payload places random), its table `mo`; the other side's table `t` at an odd
    base of its own, packed without gaps, with the misfits; `src`, the payloads
    a pack copies in; `sealed`, the batch as a correct sender leaves it with
    blank's payload bytes; `ustat` / `udst` / `uwrote`, what an unpack of
    `sealed` into the sentinel destination `dst0` gives; `packed` / `pstat` /
    `may`, what a pack of `src` into `blank` gives."""


def make_batch(O, kind, hm="crc16", pm="crc32c", plain=False):
    """plain: all eager, all fitting, no runt that holds a core header -- the
    batch on which the existing two-call routes agree with these calls."""
    rng = np.random.default_rng(20261022 + KINDS.index(kind))
    b = Batch()
    b.kind, b.hm, b.pm = kind, hm, pm
    defer = {} if plain else DEFER
    runts = {i: n for i, n in RUNTS.items() if n < 16} if plain else RUNTS
    misfits = {} if plain else MISFITS
    b.defer = sorted(defer)
    plen = np.array([LENS[i % len(LENS)] for i in range(COUNT)])
    sizes = PAY + plen
    for i, n in runts.items():
        sizes[i] = n
    for i, n in defer.items():
        sizes[i] = 16 + n
    b.mo = np.zeros(COUNT + 1, dtype=np.uint64)
    b.mo[1:] = np.cumsum(sizes)
    b.mo += np.uint64(BASE)
    R = sizes - PAY
    for i in runts:
        R[i] = RUNT_R
    for i in defer:
        R[i] = DEFER_R
    if not plain:
        R[DEFER_FITS] = sizes[DEFER_FITS] - PAY
    for i, d in misfits.items():
        assert i not in runts and i not in defer and plen[i] > 0
        R[i] = 0 if d is None else R[i] + d
    b.t = np.zeros(COUNT + 1, dtype=np.uint64)
    b.t[1:] = np.cumsum(R)
    b.t += np.uint64(OBASE)
    eager = np.array([i not in runts and i not in defer for i in range(COUNT)])
    fit = eager & np.array([i not in misfits for i in range(COUNT)])
    live = fit & (plen > 0)
    # every alignment of a payload's start, on the message side and on the other side independently (the device
    # copies start 16-byte aligned, _dev)
    for name, starts in (("message", b.mo[:-1].astype(np.int64) + PAY), ("other", b.t[:-1].astype(np.int64))):
        assert set((starts[live] % 16).tolist()) == set(range(16)), f"{name} side: payload starts miss a residue mod 16"
    b.live = [i for i in range(COUNT) if live[i]]
    b.blank = rng.integers(0, 256, size=int(b.mo[-1]) + GUARD, dtype=np.uint8)
    for i in range(COUNT):
        if sizes[i] >= 16:
            f = int(b.mo[i]) + FLAGS_AT[kind]
            b.blank[f] = (b.blank[f] & 0xFE) | (1 if i in defer else 0)
    b.src = rng.integers(0, 256, size=int(b.t[-1]) + GUARD, dtype=np.uint8)
    b.dst0 = sentinel(int(b.t[-1]) + GUARD)
    b.sealed = seal_in_place(O, b.blank, b.mo, kind, hm, pm)
    b.ustat, b.udst, b.uwrote = model_unpack(O, b.sealed, b.mo, b.t, b.dst0, kind, hm, pm)
    b.packed, b.pstat, b.may = model_pack(O, b.blank, b.mo, b.src, b.t, kind, hm, pm)
    # the batch holds what the tests below claim to cover
    if not plain:
        assert {OK, SHORT, DEFERRED, MISFIT} <= set(b.ustat.tolist()) <= {OK, SHORT, DEFERRED, MISFIT, HEADER}
        assert set(b.pstat.tolist()) == {OK, SHORT, DEFERRED, MISFIT}
        assert all(b.ustat[i] == MISFIT and b.pstat[i] == MISFIT for i in misfits)
        assert all(b.ustat[i] == DEFERRED and b.pstat[i] == DEFERRED for i in defer)
        assert [int(b.pstat[i]) for i in sorted(runts)] == [SHORT] * 4 and b.ustat[7] == SHORT and b.ustat[60] == SHORT
        assert not b.uwrote[:OBASE].any() and not b.uwrote[int(b.t[-1]):].any()
        for i in list(misfits) + list(defer) + list(runts):
            d, n = _range(b.t, i)
            assert not b.uwrote[d:d + n].any(), i
    assert all(b.ustat[i] == OK and b.pstat[i] == OK for i in b.live)
    for a in (b.mo, b.t, b.blank, b.src, b.dst0, b.sealed, b.ustat, b.udst, b.uwrote, b.packed, b.pstat, b.may):
        a.setflags(write=False)
    return b


_cache = {}


def batch_of(O, kind, hm="crc16", pm="crc32c", plain=False):
    key = (kind, hm, pm, plain)
    if key not in _cache:
        _cache[key] = make_batch(O, kind, hm, pm, plain)
    return _cache[key]


def corrupt(O, b, tables=True, flags=True):
    """The plants on the sealed batch, each at fixed indices.  Returns (bytes,
    message table, destination table, the model's statuses, destination and
    written mask).  tables=False leaves both tables as they are, flags=False every flags bit."""
    buf, mo, t = b.sealed.copy(), b.mo.copy(), b.t.copy()
    kind = b.kind
    ncov = COVERED[kind]
    take = iter(b.live[2:])

    def with_next():
        """A live index whose successor is live too; the successor is taken out of the pool."""
        while True:
            i = next(take)
            if i + 1 in b.live:
                assert next(take) == i + 1
                return i

    plan = {
        "payload": [next(take) for _ in range(3)],
        "covered": [next(take) for _ in range(ncov)],
        "more_on": [next(take)],
        "back_msg": [with_next()],
    }
    next(take), next(take)  # (the two table plants keep apart)
    plan["back_dst"] = [with_next()]
    if b.defer:
        plan["more_off"] = [DEFER_FITS, 72]
        plan["misfit_hdr"] = [150]
    flat = [i for v in plan.values() for i in v]
    assert len(flat) == len(set(flat)), "the planted sets overlap"
    at = lambda i: int(b.mo[i])
    n = lambda i: int(b.mo[i + 1] - b.mo[i]) - PAY
    for k, i in enumerate(plan["payload"]):
        buf[at(i) + PAY + (k * 977) % n(i)] ^= 1 << (k % 8)
    for k, i in enumerate(plan["covered"]):
        buf[at(i) + k] ^= 1 << ((k + 1) % 8) if k != FLAGS_AT[kind] else 0x02  # (bit 0 of flags: its own plant)
    if not flags:
        del plan["more_on"]
    for i in plan.get("more_on", []) + plan.get("more_off", []):
        buf[at(i) + FLAGS_AT[kind]] ^= 1  # the only flipped bit
    for i in plan.get("misfit_hdr", []):
        buf[at(i) + 0] ^= 4
    if tables:
        i = plan["back_msg"][0]
        assert i + 1 not in flat and i + 1 in b.live
        mo[i + 1] = mo[i] - np.uint64(1)   # message i runs backwards; message i + 1 starts inside message i - 1
        j = plan["back_dst"][0]
        assert j + 1 not in flat and j + 1 in b.live and abs(i - j) > 2
        t[j + 1] = t[j] - np.uint64(1)     # range j runs backwards: empty
    st, dst, wrote = model_unpack(O, buf, mo, t, b.dst0, kind, b.hm, b.pm)
    for name, idx in plan.items():
        for i in idx:
            d, R = _range(b.t, i)
            copied = bool(wrote[d:d + R].all()) and R > 0
            untouched = not wrote[d:d + R].any()
            if name == "payload":
                assert st[i] == PAYLOAD and copied and not np.array_equal(dst[d:d + R], b.udst[d:d + R])
            elif name == "covered":
                assert st[i] == HEADER and copied
            elif name == "more_on":
                assert st[i] == HEADER and untouched
            elif name == "more_off":
                assert st[i] == HEADER and (copied if i == DEFER_FITS else untouched)
            elif name == "misfit_hdr":
                assert st[i] == HEADER and untouched
            elif tables and name == "back_msg":
                assert st[i] == SHORT and untouched
            elif tables and name == "back_dst":
                assert st[i] == MISFIT and untouched
    assert PAYLOAD in st and HEADER in st and SHORT in st
    return buf, mo, t, st, dst, wrote


def counts_of(status, n=CLASSES):
    return np.bincount(status, minlength=n)[:n]


def _dev(a):
    """A device copy whose element 0 is 16-byte aligned (so the odd bases stay odd)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _table(tab):
    import torch
    return torch.from_numpy(np.asarray(tab).astype(np.int64)).cuda()


def _force(monkeypatch, light, nt):
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)


def _kw(b):
    return dict(kind=b.kind, payload_offset=PAY, hash_offset=HASH, header_method=b.hm, method=b.pm)


def check_unpack(gpu, b, buf, mo, t, want, want_dst, host_tables=True, options=False):
    data, dst = _dev(buf), _dev(b.dst0)
    mod, tod = _table(mo), _table(t)
    hosts = dict(offsets_host=mo, dst_offsets_host=t) if host_tables else {}
    status, counts = gpu.unpack_rpc_messages(data, mod, dst, tod, **hosts, **_kw(b))
    got = status.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert counts.numel() == CLASSES and np.array_equal(counts.cpu().numpy(), counts_of(want))
    gd = dst.cpu().numpy()
    bad = np.nonzero(gd != want_dst)[0]
    assert bad.size == 0, f"{bad.size} destination bytes differ from the model's, first at {bad[:4]}"
    assert np.array_equal(data.cpu().numpy(), buf), "an unpack wrote the message buffer"
    if options:
        dst = _dev(b.dst0)
        none, counts = gpu.unpack_rpc_messages(data, mod, dst, tod, status=False, **_kw(b))
        assert none is False and np.array_equal(counts.cpu().numpy(), counts_of(want))
        assert np.array_equal(dst.cpu().numpy(), want_dst)
        status, none = gpu.unpack_rpc_messages(data, mod, dst, tod, counts=False, **_kw(b))
        assert none is False and np.array_equal(status.cpu().numpy(), want)


@pytest.mark.parametrize("light,nt", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_unpack_sealed_batch(gpu, oracle_mod, kind, light, nt, monkeypatch):
    """A correctly sealed batch: statuses, the seven counts and every
    destination byte -- the guards before t[0] and after t[count] and every
    DEFERRED, SHORT and MISFIT range among them -- equal the model."""
    _force(monkeypatch, light, nt)
    b = batch_of(oracle_mod, kind)
    check_unpack(gpu, b, b.sealed, b.mo, b.t, b.ustat, b.udst, options=True)


@pytest.mark.parametrize("light,nt", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_unpack_corrupted_batch(gpu, oracle_mod, kind, light, nt, monkeypatch):
    """The plants: a payload bit (PAYLOAD, copied as received), covered header
    bytes (HEADER, copied), the flags bit eager -> deferred (HEADER, untouched)
    and deferred -> eager (HEADER, copied iff it then fits), a misfit with a
    corrupt header (HEADER, untouched), a message table entry that runs
    backwards (SHORT) and a destination table entry that does (MISFIT)."""
    _force(monkeypatch, light, nt)
    b = batch_of(oracle_mod, kind)
    buf, mo, t, want, want_dst, _ = corrupt(oracle_mod, b)
    check_unpack(gpu, b, buf, mo, t, want, want_dst, host_tables=False)


def check_pack(gpu, b, blank, mo, src, t, want_buf, want_stat, may, options=False):
    data, sdev = _dev(blank), _dev(src)
    mod, tod = _table(mo), _table(t)
    status = gpu.pack_rpc_messages(sdev, tod, data, mod, src_offsets_host=t, offsets_host=mo, **_kw(b))
    got = data.cpu().numpy()
    bad = np.nonzero(got[may] != want_buf[may])[0]
    assert bad.size == 0, f"{bad.size} packed bytes differ from the model's"
    assert np.array_equal(got[~may], blank[~may]), "a byte outside the R + 6 / 2 permitted bytes changed"
    assert np.array_equal(got, want_buf)
    assert np.array_equal(status.cpu().numpy(), want_stat), np.nonzero(status.cpu().numpy() != want_stat)[0][:8]
    assert np.array_equal(sdev.cpu().numpy(), src), "a pack wrote the source"
    if options:
        d2 = _dev(blank)
        assert gpu.pack_rpc_messages(sdev, tod, d2, mod, status=False, **_kw(b)) is False
        assert np.array_equal(d2.cpu().numpy(), want_buf)
    return data, mod, tod


@pytest.mark.parametrize("light,nt", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_pack_then_verify_and_unpack(gpu, oracle_mod, kind, light, nt, monkeypatch):
    """Pack into `blank`: the buffer equals the model's, only bytes of its
    may-write mask changed, the source is unchanged; verify_rpc_messages reads
    OK or DEFERRED wherever pack said so; and unpack_rpc_messages into a fresh
    destination brings the source bytes back for every OK message."""
    _force(monkeypatch, light, nt)
    b = batch_of(oracle_mod, kind)
    data, mod, tod = check_pack(gpu, b, b.blank, b.mo, b.src, b.t, b.packed, b.pstat, b.may, options=True)
    vstat, _ = gpu.verify_rpc_messages(data, mod, offsets_host=b.mo, **_kw(b))
    vstat = vstat.cpu().numpy()
    good = (b.pstat == OK) | (b.pstat == DEFERRED)
    assert np.array_equal(vstat[good], b.pstat[good])
    # the round trip
    want, want_dst, wrote = model_unpack(oracle_mod, b.packed, b.mo, b.t, b.dst0, kind, b.hm, b.pm)
    assert np.array_equal(want[good], b.pstat[good])
    dst = _dev(b.dst0)
    status, counts = gpu.unpack_rpc_messages(data, mod, dst, tod, offsets_host=b.mo, dst_offsets_host=b.t, **_kw(b))
    assert np.array_equal(status.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), counts_of(want))
    gd = dst.cpu().numpy()
    assert np.array_equal(gd, want_dst)
    nok = 0
    for i in np.nonzero(b.pstat == OK)[0]:
        d, R = _range(b.t, i)
        assert np.array_equal(gd[d:d + R], b.src[d:d + R]), i
        nok += R > 0
    assert nok > 100


@pytest.mark.parametrize("kind", KINDS)
def test_agrees_with_the_existing_calls(gpu, oracle_mod, kind):
    """On an all-eager, all-fitting batch: unpack statuses are 0 exactly where
    unpack_messages and verify_core_headers both give 0, with identical
    destination bytes; pack's bytes are pack_messages' followed by
    seal_core_headers'."""
    b = batch_of(oracle_mod, kind, plain=True)
    buf, mo, t, want, want_dst, _ = corrupt(oracle_mod, b, tables=False, flags=False)
    assert DEFERRED not in want and MISFIT not in want and PAYLOAD in want and HEADER in want
    data, mod, tod = _dev(buf), _table(mo), _table(t)
    d_old, d_new = _dev(b.dst0), _dev(b.dst0)
    ms, _ = gpu.unpack_messages(data, mod, d_old, tod, payload_offset=PAY, hash_offset=HASH)
    hs, _ = gpu.verify_core_headers(data, mod, kind=kind, offsets_host=mo)
    st, _ = gpu.unpack_rpc_messages(data, mod, d_new, tod, kind=kind)
    ms, hs, st = ms.cpu().numpy(), hs.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st, want)
    assert np.array_equal(st == OK, (ms == 0) & (hs == 0)) and (st == OK).sum() > 100
    assert np.array_equal(d_new.cpu().numpy(), d_old.cpu().numpy())
    assert np.array_equal(d_new.cpu().numpy(), want_dst)
    # the sender
    src = _dev(b.src)
    old, new = _dev(b.blank), _dev(b.blank)
    gpu.pack_messages(src, tod, old, mod, payload_offset=PAY, hash_offset=HASH)
    gpu.seal_core_headers(old, mod, kind=kind)
    st = gpu.pack_rpc_messages(src, tod, new, mod, kind=kind)
    assert np.array_equal(new.cpu().numpy(), old.cpu().numpy())
    assert np.array_equal(new.cpu().numpy(), b.packed) and np.array_equal(st.cpu().numpy(), b.pstat)


@pytest.mark.parametrize("kind,hm,pm", [("request", "crc16-kermit", "crc32c"), ("response", "crc16-kermit", "crc32c"),
                                        ("request", "crc16-ibm-3740", "crc32c"), ("response", "crc16-ibm-3740", "crc32c"),
                                        ("request", "crc16", "crc32"), ("response", "crc16", "crc32")])
def test_header_models(gpu, oracle_mod, kind, hm, pm):
    """A reflected and an MSB-first 16-bit header method, and crc32 as the payload method."""
    b = batch_of(oracle_mod, kind, hm, pm)
    check_pack(gpu, b, b.blank, b.mo, b.src, b.t, b.packed, b.pstat, b.may)
    buf, mo, t, want, want_dst, _ = corrupt(oracle_mod, b)
    check_unpack(gpu, b, buf, mo, t, want, want_dst, host_tables=False)


def repeat(tab, buf, reps):
    """A buffer's ranges `reps` times over: (bytes, table); the guard bytes behind the last range are zeros."""
    lo, hi = int(tab[0]), int(tab[-1])
    n = hi - lo
    out = np.concatenate([tab[:-1] + np.uint64(r * n) for r in range(reps)] + [[tab[0] + np.uint64(reps * n)]]).astype(np.uint64)
    return np.concatenate([buf[:lo]] + [buf[lo:hi]] * reps + [np.zeros(GUARD, dtype=buf.dtype)]), out


@pytest.mark.parametrize("kind", KINDS)
def test_queue_path(gpu, oracle_mod, kind, monkeypatch):
    """The batch twelve times over: > 1024 messages, so the full layout takes the work queue."""
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", "0")
    b, reps = batch_of(oracle_mod, kind), 12
    hbuf, _, _, want, want_dst, _ = corrupt(oracle_mod, b, tables=False)
    big, mo = repeat(b.mo, hbuf, reps)
    wdst, t = repeat(b.t, want_dst, reps)
    dst0, _ = repeat(b.t, b.dst0, reps)
    assert len(mo) - 1 == reps * COUNT > 1024
    data, dst, mod, tod = _dev(big), _dev(dst0), _table(mo), _table(t)
    st, counts = gpu.unpack_rpc_messages(data, mod, dst, tod, kind=kind, offsets_host=mo, dst_offsets_host=t)
    want = np.tile(want, reps)
    assert np.array_equal(st.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), counts_of(want))
    assert np.array_equal(dst.cpu().numpy(), wdst)
    blank, _ = repeat(b.mo, b.blank, reps)
    packed, _ = repeat(b.mo, b.packed, reps)
    src, _ = repeat(b.t, b.src, reps)
    data = _dev(blank)
    st = gpu.pack_rpc_messages(_dev(src), tod, data, mod, kind=kind, src_offsets_host=t, offsets_host=mo)
    assert np.array_equal(data.cpu().numpy(), packed)
    assert np.array_equal(st.cpu().numpy(), np.tile(b.pstat, reps))


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay(gpu, oracle_mod, kind):
    """A captured pack + unpack pair on one stream: each replay packs and
    unpacks the buffers' and the tables' current contents."""
    import torch
    O = oracle_mod
    gpu.prepare("crc32c")
    gpu.prepare("crc16")
    b = batch_of(O, kind)
    data, src, dst = _dev(b.blank), _dev(b.src), _dev(b.dst0)
    mod, tod = _table(b.mo), _table(b.t)
    pstat = torch.full((COUNT,), FAULT, dtype=torch.uint8, device="cuda")
    ustat = torch.full((COUNT,), FAULT, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(CLASSES, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.pack_rpc_messages(src, tod, data, mod, kind=kind, status=pstat)
        gpu.unpack_rpc_messages(data, mod, dst, tod, kind=kind, status=ustat, counts=counts)
    torch.cuda.synchronize()
    host, hsrc, mo = b.blank.copy(), b.src.copy(), b.mo.copy()
    for r in range(3):
        hsrc[OBASE + r:int(b.t[-1]):97] ^= 0x21 + r                      # bytes of most payloads change
        host[int(b.mo[b.live[5 + r]]) + FLAGS_AT[kind]] ^= 1             # an eager message becomes deferred
        host[int(b.mo[(DEFER_FITS, 72, 98)[r]]) + FLAGS_AT[kind]] ^= 1   # ... and a deferred one eager (the first then fits)
        k = b.live[20 + 7 * r]
        mo[k] += np.uint64(2 + r)                                        # message k - 1 grows, message k starts later, at other bytes
        want_bytes, want_p, _ = model_pack(O, host, mo, hsrc, b.t, kind)
        want_u, want_dst, _ = model_unpack(O, want_bytes, mo, b.t, b.dst0, kind)
        assert want_p[DEFER_FITS] == OK and want_p[b.live[5]] == DEFERRED
        with torch.cuda.stream(s):
            data.copy_(torch.from_numpy(host))
            src.copy_(torch.from_numpy(hsrc))
            dst.copy_(torch.from_numpy(b.dst0.copy()))
            mod.copy_(torch.from_numpy(mo.astype(np.int64)))
            pstat.fill_(FAULT)
            ustat.fill_(FAULT)
            counts.zero_()
            g.replay()
        s.synchronize()
        assert np.array_equal(data.cpu().numpy(), want_bytes), r
        assert np.array_equal(pstat.cpu().numpy(), want_p), r
        assert np.array_equal(dst.cpu().numpy(), want_dst), r
        assert np.array_equal(ustat.cpu().numpy(), want_u), r
        assert np.array_equal(counts.cpu().numpy(), counts_of(want_u)), r


def test_fault_fails_closed(gpu, oracle_mod, monkeypatch):
    """The fault-injection build in its give-up mode (a wave drops one unit, as
    one whose bounded wait timed out would; no stall): each call bumps the
    error word once, the unpack adds `count` to the FAULT class, no failing
    message reads OK or DEFERRED, and neither call writes outside what the
    model allows."""
    import torch
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    L = ctypes.CDLL(QLIB)
    c = ctypes
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    L.mchecksum_gpu_unpack_rpc_messages.argtypes = [c.c_char_p, c.c_char_p, c.c_int, c.c_void_p, c.c_void_p, c.c_size_t,
                                                    c.c_size_t, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                    c.c_void_p]
    L.mchecksum_gpu_pack_rpc_messages.argtypes = [c.c_char_p, c.c_char_p, c.c_int, c.c_void_p, c.c_void_p, c.c_void_p,
                                                  c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t, c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_set_error_word.argtypes = [c.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = c.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    monkeypatch.delenv("MCHECKSUM_GPU_QFAULT_MODE", raising=False)  # the give-up, not a stall
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", "0")
    L.mchecksum_gpu_reload_settings()
    try:
        kind = "request"
        b, reps = batch_of(oracle_mod, kind), 12
        blank, mo = repeat(b.mo, b.blank, reps)
        src, t = repeat(b.t, b.src, reps)
        packed, _ = repeat(b.mo, b.packed, reps)
        may, _ = repeat(b.mo, b.may, reps)
        want_p = np.tile(b.pstat, reps)
        n = len(mo) - 1
        assert n == reps * COUNT > 1024
        mod, tod = _table(mo), _table(t)
        stream = torch.cuda.current_stream().cuda_stream
        assert L.mchecksum_gpu_prepare(b"crc32c") == 0 and L.mchecksum_gpu_prepare(b"crc16") == 0
        # pack: stale OK everywhere
        data, sdev = _dev(blank), _dev(src)
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        faults0 = L.mchecksum_gpu_queue_faults()
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_pack_rpc_messages(b"crc16", b"crc32c", 0, sdev.data_ptr(), tod.data_ptr(), data.data_ptr(),
                                                   mod.data_ptr(), n, PAY, HASH, status.data_ptr(), stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        st, got = status.cpu().numpy(), data.cpu().numpy()
        assert np.all((st == want_p) | (st == FAULT)), "a status is neither the true one nor FAULT"
        assert np.array_equal(got[~may], blank[~may]), "a byte outside the may-write mask changed"
        assert np.array_equal(sdev.cpu().numpy(), src), "a pack wrote the source"
        # a message that reads OK or DEFERRED holds everything the model's does
        a = mo[:-1].astype(np.int64)
        for i in np.nonzero((st == OK) | (st == DEFERRED))[0]:
            lo, hi = int(mo[i]), int(mo[i + 1])
            assert np.array_equal(got[lo:hi], packed[lo:hi]), f"message {i} reads as packed and is not"
        # unpack, on the sealed batch with the plants: stale OK everywhere
        hbuf, _, _, want, want_dst, wrote = corrupt(oracle_mod, b, tables=False)
        big, _ = repeat(b.mo, hbuf, reps)
        wdst, _ = repeat(b.t, want_dst, reps)
        wrote, _ = repeat(b.t, wrote, reps)
        dst0, _ = repeat(b.t, b.dst0, reps)
        want = np.tile(want, reps)
        data, dst = _dev(big), _dev(dst0)
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(CLASSES, dtype=torch.int32, device="cuda")
        word.zero_()
        faults0 = L.mchecksum_gpu_queue_faults()
        L.mchecksum_gpu_set_error_word(word.data_ptr())
        try:
            rc = L.mchecksum_gpu_unpack_rpc_messages(b"crc16", b"crc32c", 0, data.data_ptr(), mod.data_ptr(), n, PAY, HASH,
                                                     dst.data_ptr(), tod.data_ptr(), status.data_ptr(), counts.data_ptr(),
                                                     stream)
        finally:
            L.mchecksum_gpu_set_error_word(None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(word.item()) == 1
        assert L.mchecksum_gpu_queue_faults() - faults0 == 1
        st, cn, gd = status.cpu().numpy(), counts.cpu().numpy(), dst.cpu().numpy()
        assert int(cn[FAULT]) == n, "a faulted unpack adds count to the FAULT class"
        assert np.all((st == want) | (st == FAULT)), "a status is neither the true one nor FAULT"
        failing = (want != OK) & (want != DEFERRED)
        assert not np.any((st[failing] == OK) | (st[failing] == DEFERRED)), "a failing message read as good"
        # every message that was hashed is counted in its class: all of them, or all but the dropped unit
        truth = np.bincount(want, minlength=CLASSES)
        for k in (OK, PAYLOAD, HEADER, SHORT, DEFERRED, MISFIT):
            assert cn[k] <= truth[k], k
        assert n - 1 <= int(cn.sum()) - n <= n
        assert np.array_equal(gd[~wrote], dst0[~wrote]), "a destination byte outside the model's ranges changed"
        for i in np.nonzero(st == OK)[0]:
            d, R = _range(t, i)
            assert np.array_equal(gd[d:d + R], wdst[d:d + R]), f"message {i} reads OK and its payload is not there"
        assert np.array_equal(data.cpu().numpy(), big), "an unpack wrote the message buffer"
    finally:
        monkeypatch.undo()
        L.mchecksum_gpu_reload_settings()


def test_empty_batches(gpu):
    """count == 0 with NULL buffers is valid for both calls, for both kinds."""
    import torch

    from mercury_amd import _lib
    L = _lib.load_library()
    s = torch.cuda.current_stream().cuda_stream
    for kind in (0, 1):
        assert L.mchecksum_gpu_unpack_rpc_messages(b"crc16", b"crc32c", kind, None, None, 0, PAY, HASH, None, None, None,
                                                   None, s) == 0
        assert L.mchecksum_gpu_pack_rpc_messages(b"crc16", b"crc32c", kind, None, None, None, None, 0, PAY, HASH, None,
                                                 s) == 0
    # ... and through the wrappers, with one-entry tables
    e8 = torch.zeros(0, dtype=torch.uint8, device="cuda")
    t1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    for kind in KINDS:
        st, cn = gpu.unpack_rpc_messages(e8, t1, e8, t1, kind=kind)
        assert st.numel() == 0 and cn.numel() == gpu.RPC_COPY_CLASSES == CLASSES and int(cn.sum().item()) == 0
        assert gpu.pack_rpc_messages(e8, t1, e8, t1, kind=kind).numel() == 0
