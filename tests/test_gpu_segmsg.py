"""Per-field message pack and unpack on the GPU
(mchecksum_gpu_pack_segment_messages / _unpack_segment_messages through
SegmentBatch.pack_messages / .unpack_messages and the one-shot wrappers).

Every image is built on the host: the expected message buffer of a pack (a
guard pattern in the headers, around and between what may be written, 64 bytes
either side) and the expected segment arena of an unpack (guards between and
around the segments), compared byte for byte; the hash is the oracle's CRC-32C
over the concatenated fields, big-endian in the header slot.  The two tests at
the non-temporal threshold (512 MiB) build and compare their images on the
device and take only the hashes from the host."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLIB = os.path.join(ROOT, "build", "libmchecksum_qfault.so")
GUARD, SENT = 0xA5, 0x5A
LENS = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 1000, 4103]
K = 256 << 10


class Case:
    """Segments in an arena (segment i at residue i mod 16, guard bytes
    between), objects over them, and a message table: message j is pay + N_j +
    delta[j] bytes long, the first one starts at an odd byte."""

    def __init__(self, rng, objs, pay, hoff, delta=None, lead=0, trail=0):
        # objs: per object the list of segment capacities; lead / trail: segments outside every object
        caps = [5] * lead + [c for o in objs for c in o] + [7] * trail
        self.cap = np.asarray(caps, dtype=np.int64)
        self.nseg, self.nobj = len(caps), len(objs)
        self.first = np.concatenate([[lead], lead + np.cumsum([len(o) for o in objs])]).astype(np.int64)
        at, pos = [], 64
        for i, c in enumerate(caps):
            pos = (pos + 15) // 16 * 16 + i % 16
            at.append(pos)
            pos += c + 1 + int(rng.integers(0, 20))
        self.at = np.asarray(at, dtype=np.int64)
        self.arena_size = pos + 64
        self.pay, self.hoff = pay, hoff
        self.delta = np.zeros(self.nobj, dtype=np.int64) if delta is None else np.asarray(delta, dtype=np.int64)
        self.lens = self.cap.copy()
        self.start = 64 + 2 * int(rng.integers(0, 40)) + 1
        self.table()

    def n(self, j):
        return int(self.lens[self.first[j]:self.first[j + 1]].sum())

    def table(self, sizes=None):
        """(Re)build the message table from the current lengths and deltas, or from explicit sizes."""
        if sizes is None:
            sizes = [max(0, self.pay + self.n(j) + int(self.delta[j])) for j in range(self.nobj)]
        self.off = np.concatenate([[self.start], self.start + np.cumsum(sizes)]).astype(np.int64)
        self.buf_size = int(self.off[-1]) + 64
        self.fits = np.asarray([int(self.off[j + 1] - self.off[j]) == self.pay + self.n(j) for j in range(self.nobj)])
        return self.off

    def segs(self, arena):
        return [arena[int(a):int(a) + int(c)] for a, c in zip(self.at, self.cap)]

    def fields(self, arena_h, j):
        return np.concatenate([arena_h[self.at[s]:self.at[s] + int(self.lens[s])]
                               for s in range(self.first[j], self.first[j + 1])] + [np.zeros(0, dtype=np.uint8)])

    def packed(self, arena_h, crc, buf_size=None):
        """The buffer a pack must leave: guards everywhere but the payload and hash bytes of fitting messages."""
        exp = np.full(buf_size or self.buf_size, GUARD, dtype=np.uint8)
        for j in np.nonzero(self.fits)[0]:
            b, m0 = self.fields(arena_h, j), int(self.off[j])
            exp[m0 + self.pay:m0 + self.pay + len(b)] = b
            exp[m0 + self.hoff:m0 + self.hoff + 4] = np.frombuffer(int(crc(b)).to_bytes(4, "big"), dtype=np.uint8)
        return exp

    def wire(self, rng, crc):
        """A received buffer: random bytes throughout, the right hash in every fitting message."""
        img = rng.integers(0, 256, size=self.buf_size, dtype=np.uint8)
        for j in np.nonzero(self.fits)[0]:
            m0 = int(self.off[j])
            v = crc(img[m0 + self.pay:int(self.off[j + 1])])
            img[m0 + self.hoff:m0 + self.hoff + 4] = np.frombuffer(int(v).to_bytes(4, "big"), dtype=np.uint8)
        return img

    def unpacked(self, img):
        """The arena an unpack must leave: sentinels everywhere but the segments of fitting messages."""
        exp = np.full(self.arena_size, SENT, dtype=np.uint8)
        for j in np.nonzero(self.fits)[0]:
            pos = int(self.off[j]) + self.pay
            for s in range(self.first[j], self.first[j + 1]):
                exp[self.at[s]:self.at[s] + int(self.lens[s])] = img[pos:pos + int(self.lens[s])]
                pos += int(self.lens[s])
        return exp


@pytest.fixture(scope="module")
def crc(oracle_mod):
    return lambda b: oracle_mod.crc("crc32c", np.ascontiguousarray(b, dtype=np.uint8))


@pytest.fixture(scope="module", autouse=True)
def _prepared(gpu):
    gpu.prepare("crc32c")


def _same(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[:5]}: got {got[bad[:5]]}, want {exp[bad[:5]]}"


def check_pack(gpu, c, rng, crc, batch_of=None, **kw):
    import torch
    arena_h = rng.integers(0, 256, size=c.arena_size, dtype=np.uint8)
    arena = torch.from_numpy(arena_h).cuda()
    buf = torch.full((c.buf_size,), GUARD, dtype=torch.uint8, device="cuda")
    batch = gpu.SegmentBatch(c.segs(arena), c.first)
    status = batch.pack_messages(buf, c.off, c.pay, c.hoff, **kw)
    torch.cuda.synchronize()
    _same(buf.cpu().numpy(), c.packed(arena_h, crc), "message buffer")
    _same(arena.cpu().numpy(), arena_h, "segment memory")
    if status is not False:
        assert status.cpu().numpy().tolist() == (~c.fits).astype(np.uint8).tolist()
    return arena, buf, batch


def check_unpack(gpu, c, rng, crc, corrupt=None, **kw):
    """corrupt: img -> set of messages it damaged (applied to the wire image)."""
    import torch
    img = c.wire(rng, crc)
    damaged = corrupt(img) if corrupt else set()
    buf = torch.from_numpy(img).cuda()
    arena = torch.full((c.arena_size,), SENT, dtype=torch.uint8, device="cuda")
    batch = gpu.SegmentBatch(c.segs(arena), c.first)
    status, mism = batch.unpack_messages(buf, c.off, c.pay, c.hoff, **kw)
    torch.cuda.synchronize()
    _same(arena.cpu().numpy(), c.unpacked(img), "segment arena")
    _same(buf.cpu().numpy(), img, "message buffer")
    want = [int(not c.fits[j] or j in damaged) for j in range(c.nobj)]
    if status is not False:
        assert status.cpu().numpy().tolist() == want
    if mism is not False:
        assert int(mism.item()) == sum(want)
    return img, arena, batch


def _ragged(rng, nobj=40):
    objs = [[int(rng.choice(LENS)) for _ in range(int(rng.integers(0, 7)))] for _ in range(nobj)]
    objs[3], objs[4] = [], [0, 0]  # no segments; only empty ones
    return objs


# 1 ------------------------------------------------------------------ ragged --
@pytest.mark.parametrize("pay,hoff", [(20, 16), (9, 3)])
@pytest.mark.parametrize("direction", ["pack", "unpack"])
def test_ragged_batch(gpu, crc, direction, pay, hoff):
    rng = np.random.default_rng(101 + pay)
    c = Case(rng, _ragged(rng), pay, hoff, lead=2, trail=1)
    assert c.nseg > 64 and set((c.at % 16).tolist()) == set(range(16))
    assert c.fits.all()
    (check_pack if direction == "pack" else check_unpack)(gpu, c, rng, crc)


# 2 ------------------------------------------------------------- chunk edges --
@pytest.mark.parametrize("direction", ["pack", "unpack"])
def test_chunk_edges(gpu, crc, direction):
    """A segment of one chunk + 5 bytes at an odd address, one of exactly two
    chunks, a 3-byte tail: the smallest sizes that give a segment more than
    one chunk, in one message."""
    rng = np.random.default_rng(202)
    c = Case(rng, [[3], [K + 5, 2 * K, 3], [17]], 20, 16, lead=2)
    assert c.cap[3] == K + 5 and c.at[3] % 2 == 1
    (check_pack if direction == "pack" else check_unpack)(gpu, c, rng, crc)


# 3 ------------------------------------------------- more than one scan block --
@pytest.mark.parametrize("direction", ["pack", "unpack"])
def test_more_than_one_scan_block(gpu, crc, direction):
    rng = np.random.default_rng(303)
    cuts = np.sort(rng.integers(0, 1031, size=199))
    caps = rng.integers(1, 49, size=1030)
    objs = [caps[a:b].tolist() for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [1030]]))]
    c = Case(rng, objs, 20, 16)
    assert c.nseg == 1030 and c.nobj == 200
    (check_pack if direction == "pack" else check_unpack)(gpu, c, rng, crc)


# 4 ----------------------------------------------------------------- misfits --
def _misfit_case(rng):
    objs = _ragged(rng, 24)
    objs[6], objs[9], objs[12], objs[15], objs[16] = [64, 5], [1000], [17, 16], [], []
    delta = np.zeros(24, dtype=np.int64)
    delta[6], delta[9] = 1, -1     # one byte long, one byte short
    delta[12] = -(17 + 16) - 7     # 13 bytes: shorter than payload_offset
    delta[16] = 2                  # no segments, longer than its headers
    delta[4] = -20                 # only empty segments, and no room for the headers: 0 bytes
    # (15: no segments and exactly payload_offset bytes -- fits, sealed with the empty message's CRC)
    return Case(rng, objs, 20, 16, delta=delta)


@pytest.mark.parametrize("direction", ["pack", "unpack"])
def test_misfits_among_fitting_messages(gpu, crc, direction):
    rng = np.random.default_rng(404)
    c = _misfit_case(rng)
    assert np.nonzero(~c.fits)[0].tolist() == [4, 6, 9, 12, 16] and c.fits[15] and c.fits[3]
    assert c.off[13] - c.off[12] == 13 and c.off[16] - c.off[15] == 20
    if direction == "pack":
        _, buf, _ = check_pack(gpu, c, rng, crc)
        m0 = int(c.off[15])
        assert bytes(buf[m0 + 16:m0 + 20].cpu().numpy()) == int(crc(np.zeros(0, dtype=np.uint8))).to_bytes(4, "big")
    else:
        check_unpack(gpu, c, rng, crc)


# 5 -------------------------------------------------------------- corruption --
def test_unpack_flags_exactly_the_corrupted_messages(gpu, crc):
    rng = np.random.default_rng(505)
    c = Case(rng, [o if sum(o) else [33] for o in _ragged(rng)], 20, 16)
    payload_hit, hash_hit = [2, 11, 29], [7, 30]

    def corrupt(img):
        for j in payload_hit:
            at = int(c.off[j]) + c.pay + int(rng.integers(0, c.n(j)))
            img[at] ^= 1 << int(rng.integers(0, 8))
        for j in hash_hit:
            img[int(c.off[j]) + c.hoff + int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
        return set(payload_hit + hash_hit)

    check_unpack(gpu, c, rng, crc, corrupt=corrupt)  # (the arena compare: flagged segments hold the bytes as received)


# 6 ------------------------------------------------ agreement with the others --
def test_agrees_with_the_existing_calls(gpu, crc):
    import torch
    rng = np.random.default_rng(606)
    c = Case(rng, _ragged(rng), 20, 16)
    arena, buf, batch = check_pack(gpu, c, rng, crc)
    off = torch.from_numpy(c.off).cuda()
    status, mism = gpu.verify_messages(buf, off)
    assert int(status.sum().item()) == 0 and int(mism.item()) == 0
    # gather_segments + seal_messages over the same tables
    two = torch.full((c.buf_size,), GUARD, dtype=torch.uint8, device="cuda")
    batch.gather("crc32c", two, (c.off[:-1] + c.pay).tolist())
    assert int(gpu.seal_messages(two, off).sum().item()) == 0
    assert torch.equal(two, buf)
    # the one-shot form
    one = torch.full((c.buf_size,), GUARD, dtype=torch.uint8, device="cuda")
    assert int(gpu.pack_segment_messages(c.segs(arena), c.first, one, c.off).sum().item()) == 0
    assert torch.equal(one, buf)
    # pack_messages (one contiguous source per message), then unpack_segment_messages
    src_off = np.concatenate([[0], np.cumsum([c.n(j) for j in range(c.nobj)])]).astype(np.int64)
    src_h = rng.integers(0, 256, size=int(src_off[-1]) + 16, dtype=np.uint8)
    src = torch.from_numpy(src_h).cuda()
    msgs = torch.full((c.buf_size,), GUARD, dtype=torch.uint8, device="cuda")
    assert int(gpu.pack_messages(src, torch.from_numpy(src_off).cuda(), msgs, off).sum().item()) == 0
    back = torch.full((c.arena_size,), SENT, dtype=torch.uint8, device="cuda")
    status, mism = gpu.unpack_segment_messages(msgs, c.off, c.segs(back), c.first)
    torch.cuda.synchronize()
    assert int(status.sum().item()) == 0 and int(mism.item()) == 0
    back_h = back.cpu().numpy()
    for j in range(c.nobj):
        assert bytes(c.fields(back_h, j)) == bytes(src_h[src_off[j]:src_off[j + 1]]), j


# 7 ------------------------------------------------------------ graph capture --
@pytest.mark.parametrize("direction", ["pack", "unpack"])
def test_graph_capture_with_new_tables(gpu, crc, direction):
    """One captured call, three replays; before each the segment lengths, the
    message table and the contents change, and in the second one message no
    longer fits.  Every replay is checked as the ragged batch is."""
    import torch
    rng = np.random.default_rng(707)
    c = Case(rng, _ragged(rng), 20, 16, lead=1)
    cap_buf = int(c.buf_size)  # the longest table: every later one is shorter
    arena = torch.empty(c.arena_size, dtype=torch.uint8, device="cuda")
    buf = torch.empty(cap_buf, dtype=torch.uint8, device="cuda")
    batch = gpu.SegmentBatch(c.segs(arena), c.first)
    off = torch.from_numpy(c.off).cuda()
    status = torch.ones(c.nobj, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        if direction == "pack":
            batch.pack_messages(buf, off, status=status)
        else:
            batch.unpack_messages(buf, off, status=status, mismatches=mism)
    steps = [c.cap, np.where(rng.integers(0, 3, size=c.nseg) == 0, c.cap // 2, c.cap),
             np.minimum(c.cap, rng.integers(0, 200, size=c.nseg))]
    for r, lens in enumerate(steps):
        c.lens = np.asarray(lens, dtype=np.int64)
        c.delta[:] = 0
        if r == 1:
            c.delta[5] = 1
        c.table()
        assert c.buf_size <= cap_buf and bool(c.fits.all()) == (r != 1)
        batch.set_lengths(c.lens, stream=s)
        status.fill_(7)
        mism.zero_()
        if direction == "pack":
            arena_h = rng.integers(0, 256, size=c.arena_size, dtype=np.uint8)
            arena.copy_(torch.from_numpy(arena_h))
            buf.fill_(GUARD)
        else:
            img = np.full(cap_buf, GUARD, dtype=np.uint8)
            img[:c.buf_size] = c.wire(rng, crc)
            buf.copy_(torch.from_numpy(img))
            arena.fill_(SENT)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            off.copy_(torch.from_numpy(c.off), non_blocking=False)
            g.replay()
        s.synchronize()
        want = (~c.fits).astype(np.uint8).tolist()
        assert status.cpu().numpy().tolist() == want, f"replay {r}"
        if direction == "pack":
            _same(buf.cpu().numpy(), c.packed(arena_h, crc, cap_buf), f"replay {r}: message buffer")
            _same(arena.cpu().numpy(), arena_h, f"replay {r}: segment memory")
        else:
            _same(arena.cpu().numpy(), c.unpacked(img), f"replay {r}: segment arena")
            _same(buf.cpu().numpy(), img, f"replay {r}: message buffer")
            assert int(mism.item()) == sum(want), f"replay {r}"
    torch.cuda.synchronize()


# 8 -------------------------------------------------------------- fail closed --
@pytest.fixture(scope="module")
def qlib(gpu):
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    L = ctypes.CDLL(QLIB)
    t = ctypes
    L.mchecksum_gpu_prepare.argtypes = [t.c_char_p]
    L.mchecksum_gpu_segment_messages_work_size.argtypes = [t.c_size_t, t.c_size_t]
    L.mchecksum_gpu_segment_messages_work_size.restype = t.c_size_t
    L.mchecksum_gpu_pack_segment_messages.argtypes = [t.c_char_p, t.c_void_p, t.c_void_p, t.c_size_t, t.c_void_p,
                                                      t.c_size_t, t.c_void_p, t.c_void_p, t.c_size_t, t.c_size_t,
                                                      t.c_void_p, t.c_size_t, t.c_void_p, t.c_void_p]
    L.mchecksum_gpu_unpack_segment_messages.argtypes = [t.c_char_p, t.c_void_p, t.c_void_p, t.c_size_t, t.c_size_t,
                                                        t.c_size_t, t.c_void_p, t.c_void_p, t.c_size_t, t.c_void_p,
                                                        t.c_void_p, t.c_size_t, t.c_void_p, t.c_void_p, t.c_void_p]
    L.mchecksum_gpu_set_error_word.argtypes = [t.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = t.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    return L


@pytest.mark.parametrize("direction", ["pack", "unpack"])
def test_a_scan_that_gave_up_writes_nothing(gpu, qlib, crc, monkeypatch, direction):
    """The test library's scan give-up setting (scan block 1 gives up its
    look-back at once; the list is padded with empty segments outside every
    object up to a third scan block): nothing is written on either side,
    every status is 1, the error word gets 1, unpack adds nobj."""
    import torch
    rng = np.random.default_rng(808)
    c = Case(rng, _ragged(rng, 12), 20, 16)
    fill = SENT if direction == "unpack" else 0x3C
    arena = torch.full((c.arena_size,), fill, dtype=torch.uint8, device="cuda")
    img = c.wire(rng, crc) if direction == "unpack" else np.full(c.buf_size, GUARD, dtype=np.uint8)
    buf = torch.from_numpy(img).cuda()
    batch = gpu.SegmentBatch(c.segs(arena) + [arena[0:0]] * (2060 - c.nseg), c.first)
    off = torch.from_numpy(c.off).cuda()
    status = torch.zeros(c.nobj, dtype=torch.uint8, device="cuda")
    mism = torch.full((1,), 3, dtype=torch.int32, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    n, base = batch.nseg, batch.meta.data_ptr()
    work = torch.zeros((qlib.mchecksum_gpu_segment_messages_work_size(n, c.nobj) + 7) // 8, dtype=torch.int64,
                       device="cuda")
    assert qlib.mchecksum_gpu_prepare(b"crc32c") == 0
    faults0 = qlib.mchecksum_gpu_queue_faults()
    monkeypatch.setenv("MCHECKSUM_GPU_QFAULT_SCAN", "1")
    qlib.mchecksum_gpu_reload_settings()
    qlib.mchecksum_gpu_set_error_word(word.data_ptr())
    h = torch.cuda.current_stream().cuda_stream
    try:
        if direction == "pack":
            rc = qlib.mchecksum_gpu_pack_segment_messages(b"crc32c", base, base + 8 * n, n, base + 16 * n, c.nobj,
                                                          buf.data_ptr(), off.data_ptr(), 20, 16, work.data_ptr(),
                                                          work.numel() * 8, status.data_ptr(), h)
        else:
            rc = qlib.mchecksum_gpu_unpack_segment_messages(b"crc32c", buf.data_ptr(), off.data_ptr(), c.nobj, 20, 16,
                                                            base, base + 8 * n, n, base + 16 * n, work.data_ptr(),
                                                            work.numel() * 8, status.data_ptr(), mism.data_ptr(), h)
        torch.cuda.synchronize()
    finally:
        qlib.mchecksum_gpu_set_error_word(None)
        monkeypatch.undo()
        qlib.mchecksum_gpu_reload_settings()
    assert rc == 0
    assert int(word.item()) == 1
    assert qlib.mchecksum_gpu_queue_faults() - faults0 == 1
    assert status.cpu().numpy().tolist() == [1] * c.nobj
    _same(buf.cpu().numpy(), img, "message buffer")
    assert bool((arena == fill).all()), "segment memory was written"
    if direction == "unpack":
        assert int(mism.item()) == 3 + c.nobj


# 9 ------------------------------------------ another stream, optional outputs --
def test_non_default_stream(gpu, crc):
    import torch
    rng = np.random.default_rng(909)
    c = Case(rng, _ragged(rng, 16), 20, 16)
    s = torch.cuda.Stream()
    check_pack(gpu, c, rng, crc, stream=s)
    check_unpack(gpu, c, rng, crc, stream=s)


def test_null_status_and_mismatches(gpu, crc):
    rng = np.random.default_rng(910)
    c = _misfit_case(rng)
    check_pack(gpu, c, rng, crc, status=False)
    check_unpack(gpu, c, rng, crc, status=False, mismatches=False)


# 10 --------------------------------------------- the non-temporal threshold --
# seg_msg_copy_kernel takes the non-temporal loads when the scan's total is
# kSegNtBytes = 512 MiB or more -- every segment counts, those of a message
# that does not fit too.  One list for both directions, 4099 bytes over: a
# segment of a chunk + 5 bytes (at an odd address in both tests), an empty
# segment, a message with no segments, and between fitting messages one whose
# slot is a byte too long -- the walk steps over its 64 MiB of chunks.
NT_BYTES = 512 << 20
M = 1 << 20
NT_PAY, NT_HOFF = 20, 16
NT_DELTA = [0, 0, 1, 0, 0]
# where segment s starts, mod 16: the source offset of a pack, the arena residue of an unpack
NT_RES = [1, 7, 0, 3, 0, 0, 9, 0, 0, 5, 11, 2]


def _nt_list():
    """(segment lengths, first, message table, bytes per message)."""
    objs = [[K + 5, 0, 60 * M], [], [40 * M + 3, 24 * M], [64 * M, 64 * M + 1, 64 * M], [64 * M, 17, 64 * M + 7, 0]]
    objs[4][3] = NT_BYTES + 4099 - sum(sum(o) for o in objs)
    lens = [n for o in objs for n in o]
    first = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.int64)
    N = [sum(o) for o in objs]
    off = (65 + np.concatenate([[0], np.cumsum([NT_PAY + n + d for n, d in zip(N, NT_DELTA)])])).astype(np.int64)
    assert sum(lens) == NT_BYTES + 4099 and len(lens) == len(NT_RES) and lens[0] == K + 5 and min(lens[2:]) > 0
    return lens, first, off, N


def _enough_memory(nbytes):
    import torch
    if torch.cuda.mem_get_info()[0] < nbytes:
        pytest.skip(f"not enough free device memory for the 512 MiB list ({nbytes >> 20} MiB wanted)")


def _same_on_device(got, exp, what):
    import torch
    if not torch.equal(got, exp):
        bad = torch.nonzero(got != exp).flatten()
        raise AssertionError(f"{what}: {bad.numel()} bytes differ, first at {bad[:5].tolist()}")


def _be32(v):
    import torch
    return torch.tensor(list(int(v).to_bytes(4, "big")), dtype=torch.uint8, device="cuda")


def test_pack_at_the_non_temporal_threshold(gpu, oracle_mod):
    """The segments are views into one 68 MiB source (reads may alias).  The
    expected buffer is built on the device -- torch.cat of the same views into
    a guard-filled buffer -- with the oracle's CRC-32C of each message's
    fields, computed over a host copy of the source; the whole buffer is
    compared, guards and the misfit's slot included."""
    import torch
    lens, first, off, N = _nt_list()
    size = int(off[-1]) + 64
    _enough_memory(4 * size)  # the buffer, the expected one, the compare's temporaries
    src = torch.empty(max(lens) + 4096, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(src, 0x5E65)
    host = src.cpu().numpy()
    assert src.data_ptr() % 16 == 0
    views = [src[r:r + n] for r, n in zip(NT_RES, lens)]
    buf = torch.full((size,), GUARD, dtype=torch.uint8, device="cuda")
    status = gpu.SegmentBatch(views, first).pack_messages(buf, off, NT_PAY, NT_HOFF)
    torch.cuda.synchronize()
    exp = torch.full((size,), GUARD, dtype=torch.uint8, device="cuda")
    for j in range(len(N)):
        if NT_DELTA[j]:
            continue
        m0, segs = int(off[j]), range(first[j], first[j + 1])
        if N[j]:
            exp[m0 + NT_PAY:m0 + NT_PAY + N[j]] = torch.cat([views[s] for s in segs])
        fields = np.concatenate([host[NT_RES[s]:NT_RES[s] + lens[s]] for s in segs] + [np.zeros(0, dtype=np.uint8)])
        exp[m0 + NT_HOFF:m0 + NT_HOFF + 4] = _be32(oracle_mod.crc("crc32c", fields, "sse42"))
    _same_on_device(buf, exp, "message buffer")
    assert status.tolist() == NT_DELTA
    assert np.array_equal(src.cpu().numpy(), host), "segment memory was written"


def test_unpack_at_the_non_temporal_threshold(gpu, oracle_mod):
    """The message buffer is generated on the device; the hashes come from
    the oracle over a host copy (batch_offsets over the table header, payload,
    header, ...: 8 threads).  The segments are distinct slices of one
    sentinel-filled arena, which is compared on the device with slices of the
    message buffer: the misfit's segments and every gap keep their sentinels.
    One fitting message is corrupted after its hash was stored."""
    import torch
    lens, first, off, N = _nt_list()
    size = int(off[-1]) + 64
    _enough_memory(6 * size)  # buffer and its copy, arena and the expected one, the compare's temporaries
    buf = torch.empty(size, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(buf, 0x5E66)
    table = np.stack([off[:-1], off[:-1] + NT_PAY], axis=1).ravel().tolist() + [int(off[-1])]
    crcs = oracle_mod.batch_offsets("crc32c", buf.cpu().numpy(), np.asarray(table), variant="sse42", nthreads=8)[1::2]
    assert int(crcs[1]) == oracle_mod.crc("crc32c", b"")  # (the message with no segments: exactly its headers)
    for j in range(len(N)):
        if not NT_DELTA[j]:
            buf[int(off[j]) + NT_HOFF:int(off[j]) + NT_HOFF + 4] = _be32(crcs[j])
    buf[int(off[3]) + NT_PAY + 100 * M + 3] ^= 0x10  # in message 3's second segment
    before = buf.clone()
    at, pos = [], 64
    for r, n in zip(NT_RES, lens):
        pos = (pos + 15) // 16 * 16 + r
        at.append(pos)
        pos += n + 14
    assert at[0] % 2 == 1
    arena = torch.full((pos + 64,), SENT, dtype=torch.uint8, device="cuda")
    status, mism = gpu.SegmentBatch([arena[a:a + n] for a, n in zip(at, lens)], first).unpack_messages(
        buf, off, NT_PAY, NT_HOFF)
    torch.cuda.synchronize()
    exp = torch.full((pos + 64,), SENT, dtype=torch.uint8, device="cuda")
    for j in range(len(N)):
        if NT_DELTA[j]:
            continue
        p = int(off[j]) + NT_PAY
        for s in range(first[j], first[j + 1]):
            exp[at[s]:at[s] + lens[s]] = buf[p:p + lens[s]]
            p += lens[s]
    _same_on_device(arena, exp, "segment arena")
    _same_on_device(buf, before, "message buffer")
    assert status.tolist() == [0, 0, 1, 1, 0] and int(mism.item()) == 2
