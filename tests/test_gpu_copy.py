"""Copy and checksum in one pass on the GPU (include/mchecksum_gpu.h:
mchecksum_gpu_copy_offsets, mchecksum_gpu_update_copy_offsets): every chunk is
stored at its own destination by the payload loop that hashes it.  The values
are the CPU streaming API's (mchecksum_update / get) or the oracle's; every
destination byte is compared with the source's, and every byte the calls must
not write -- before, between and after the destinations, and the source --
with its value before the call.  Every kernel of the family runs here.
"""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xEE
SEED = 19
# (source, destination) base shifts, as the receiver's: with byte-packed chunks and gaps of 0..40 bytes between
# the destinations every source residue and every (dst - src) mod 16 occurs
SHIFTS = ((0, 0), (1, 2), (2, 1), (3, 1))
SRC_LEAD, DST_LEAD, TAIL = 48, 80, 96
BIG = (65535, 65536, 65537, 70001, 66000, 67891, 69999, 68000)
METHODS = ("crc32c", "crc64", "crc64-ecma182")  # the last one MSB-first
# (method, MCHECKSUM_GPU_LIGHT, MCHECKSUM_GPU_NT): the light layout is CRC-32C's alone
LAYOUTS = [("crc32c", "0", None), ("crc32c", "1", None), ("crc32c", "0", "1"),
           ("crc64", "0", None), ("crc64", "0", "1"), ("crc64-ecma182", "0", None), ("crc64-ecma182", "0", "1")]


def _crcs(method, chunks):
    """The streaming API's value of every chunk."""
    from mercury_amd import Checksum
    ck = Checksum(method)
    out = []
    for c in chunks:
        ck.reset()
        ck.update(c.tobytes())
        out.append(ck.get())
    ck.close()
    return np.asarray(out, dtype=np.uint64)


def _scatter(rng, lens, max_gap=40):
    """Destination starts: the chunks in a random order, a 0..max_gap-byte gap
    before, between and after them.  Returns (starts, bytes of the view)."""
    order = rng.permutation(len(lens))
    gaps = rng.integers(0, max_gap + 1, len(lens) + 1)
    ds = np.zeros(len(lens), dtype=np.uint64)
    pos = int(gaps[0])
    for j, i in enumerate(order):
        ds[i] = pos
        pos += int(lens[i]) + int(gaps[j + 1])
    return ds, pos


def _expected_dst(buf, so, ds, ndst):
    want = np.full(ndst, CANARY, dtype=np.uint8)
    for a, b, d in zip(so[:-1].astype(np.int64), so[1:].astype(np.int64), ds.astype(np.int64)):
        want[d:d + b - a] = buf[a:b]
    return want


class Case:
    def __init__(self):
        rng = np.random.default_rng(SEED)
        lens = rng.integers(0, 2101, 4000)
        lens[4 + rng.choice(3990, 8, replace=False)] = BIG
        lens[:4] = (0, 1, 2100, 16)
        lens[-1] = 777
        self.lens = lens
        self.so = np.zeros(len(lens) + 1, dtype=np.uint64)
        self.so[1:] = np.cumsum(lens)
        self.so += np.uint64(37)  # packed back to back from a non-zero offset
        self.buf = rng.integers(0, 256, size=int(self.so[-1]) + 11, dtype=np.uint8)
        self.buf.setflags(write=False)
        self.ds, self.ndst = _scatter(rng, lens)
        assert not np.all(np.diff(self.ds.astype(np.int64)) > 0)  # not monotonic
        self.want = _expected_dst(self.buf, self.so, self.ds, self.ndst)
        self.want.setflags(write=False)
        # every source residue and every relative misalignment occurs (bases 16-byte aligned + shift)
        sres, rel = set(), set()
        live = lens > 0
        for ss, dsh in SHIFTS:
            s_at = self.so[:-1].astype(np.int64) + SRC_LEAD + ss
            d_at = self.ds.astype(np.int64) + DST_LEAD + dsh
            sres |= set((s_at[live] % 16).tolist())
            rel |= set(((d_at[live] - s_at[live]) % 16).tolist())
        assert sres == set(range(16)) and rel == set(range(16)), (sorted(sres), sorted(rel))
        self._crc = {}

    def chunks(self):
        return [self.buf[int(a):int(b)] for a, b in zip(self.so[:-1], self.so[1:])]

    def crcs(self, method):
        if method not in self._crc:
            self._crc[method] = _crcs(method, self.chunks())
        return self._crc[method]


@pytest.fixture(scope="module")
def case():
    return Case()


@pytest.fixture(scope="module", autouse=True)
def report(gpu):
    """The error word every call of this file reports to, and the fault count before the first."""
    import torch
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    faults0 = gpu.queue_faults()
    gpu.set_error_word(word)
    yield word, faults0
    gpu.set_error_word(None)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).cuda()


def _device(torch, buf, ss, dsh, ndst):
    """(source base, source view, destination base, destination view) on 16-byte-aligned bases."""
    sbase = torch.full((SRC_LEAD + 4 + buf.size + TAIL,), 0x11, dtype=torch.uint8, device="cuda")
    dbase = torch.full((DST_LEAD + 4 + ndst + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
    assert sbase.data_ptr() % 16 == 0 and dbase.data_ptr() % 16 == 0
    sview = sbase[SRC_LEAD + ss:SRC_LEAD + ss + buf.size]
    dview = dbase[DST_LEAD + dsh:DST_LEAD + dsh + ndst]
    sview.copy_(torch.from_numpy(np.array(buf)))
    return sbase, sview, dbase, dview


def _check_dst(dbase, dsh, want, what=""):
    """The destination view holds the scattered chunks, and every other byte of its base is canary still."""
    got = dbase.cpu().numpy()
    lo, hi = DST_LEAD + dsh, DST_LEAD + dsh + want.size
    diff = np.nonzero(got[lo:hi] != want)[0]
    assert diff.size == 0, f"{what}: {diff.size} destination bytes differ, first at {diff[:4]}"
    assert np.all(got[:lo] == CANARY) and np.all(got[hi:] == CANARY), f"{what}: a byte outside the destination view was written"


def _get(G, method, state):
    return G.as_unsigned(G.state_get(method, state)).astype(np.uint64)


def _set_layout(monkeypatch, light, nt):
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", light)
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)


@pytest.mark.parametrize("method,light,nt", LAYOUTS)
def test_copy_offsets(gpu, case, method, light, nt, monkeypatch):
    import torch
    _set_layout(monkeypatch, light, nt)
    sod, dsd = _dev(torch, case.so), _dev(torch, case.ds)
    want_crc = case.crcs(method)
    for ss, dsh in SHIFTS:
        sbase, sview, dbase, dview = _device(torch, case.buf, ss, dsh, case.ndst)
        sbefore = sbase.cpu().numpy()
        out = gpu.copy_offsets(method, sview, sod, dview, dsd, offsets_host=case.so, dst_starts_host=case.ds)
        got = gpu.as_unsigned(out).astype(np.uint64)
        bad = np.nonzero(got != want_crc)[0]
        assert bad.size == 0, (method, "shifts", ss, dsh, "chunks", bad[:8], case.lens[bad[:8]])
        _check_dst(dbase, dsh, case.want, f"{method} shifts {ss}/{dsh}")
        assert np.array_equal(sbase.cpu().numpy(), sbefore), "the source changed"


@pytest.mark.parametrize("method,light,nt", LAYOUTS)
def test_update_copy_offsets_in_rounds(gpu, case, method, light, nt, monkeypatch):
    """state_init, three update_copy_offsets over the chunks cut in three, state_get:
    the CRC of each whole chunk, and the destination of test_copy_offsets.
    A second state gets its middle round from update_offsets (no copy): the
    same values."""
    import torch
    _set_layout(monkeypatch, light, nt)
    rng = np.random.default_rng(3)
    lens = case.lens.astype(np.int64)
    n = len(lens)
    cuts = np.sort(rng.integers(0, lens + 1, (2, n)), axis=0)
    cuts[0][rng.random(n) < 0.15] = 0                      # an empty first round
    late = rng.random(n) < 0.15
    cuts[0][late], cuts[1][late] = lens[late], lens[late]  # empty second and third rounds
    mid = rng.random(n) < 0.15
    cuts[1][mid] = cuts[0][mid]                            # an empty second round
    bounds = np.vstack([np.zeros(n, dtype=np.int64), cuts, lens])
    start = case.so[:-1].astype(np.int64)
    dsh = SHIFTS[1][1]
    dbase = torch.full((DST_LEAD + 4 + case.ndst + TAIL,), CANARY, dtype=torch.uint8, device="cuda")
    dview = dbase[DST_LEAD + dsh:DST_LEAD + dsh + case.ndst]
    state = gpu.state_init(method, n)
    mixed = gpu.state_init(method, n)
    scratch = torch.empty(case.ndst, dtype=torch.uint8, device="cuda")
    for r in range(3):
        rl = bounds[r + 1] - bounds[r]
        assert np.any(rl == 0) and np.any(rl > 0)
        base = (5 + 7 * r) % 16  # each round's staging buffer packs its pieces from another residue
        ro = base + np.concatenate([[0], np.cumsum(rl)])
        parts = [case.buf[a:a + k] for a, k in zip(start + bounds[r], rl)]
        stage = np.concatenate([np.zeros(base, dtype=np.uint8)] + parts + [np.zeros(64, dtype=np.uint8)])
        rds = case.ds.astype(np.int64) + bounds[r]
        sdev, rod, rdsd = torch.from_numpy(stage).cuda(), _dev(torch, ro), _dev(torch, rds)
        raw = state.clone()
        assert gpu.update_copy_offsets(method, sdev, rod, dview, rdsd, state, offsets_host=ro, dst_starts_host=rds) is state
        same = (state == raw).cpu().numpy()
        assert np.all(same[rl == 0]), "an empty chunk changed its state"
        if r == 1:
            gpu.update_offsets(method, sdev, rod, mixed, offsets_host=ro)
        else:
            gpu.update_copy_offsets(method, sdev, rod, scratch, rdsd, mixed)
        assert np.array_equal(sdev.cpu().numpy(), stage), "the staging buffer changed"
    want = case.crcs(method)
    got = _get(gpu, method, state)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (method, "chunks", bad[:8], lens[bad[:8]])
    assert np.array_equal(_get(gpu, method, mixed), want), "update_offsets and update_copy_offsets rounds do not mix"
    _check_dst(dbase, dsh, case.want, f"{method} in rounds")


@pytest.mark.parametrize("count", [1, 1024, 1025, 8192])
@pytest.mark.parametrize("method", ["crc32c", "crc64"])
def test_every_kernel_of_the_family(gpu, oracle_mod, method, count):
    """Where the offsets plan changes kernels -- 1 and 1024 chunks (the light
    CRC-32C layout and its boundary), 1025 (the full layout, with a work-queue
    slot), 8192 (non-temporal) -- both operations, 300-byte chunks: with the
    layouts of the tests above, all 10 kernels run."""
    import torch
    G, O = gpu, oracle_mod
    n = 300
    rng = np.random.default_rng(count)
    host = O.splitmix_bytes(9 + n * count + 64, 0xC09 + count)
    so = 9 + n * np.arange(count + 1, dtype=np.int64)
    ds = 3 + (n + 5) * rng.permutation(count).astype(np.int64)
    ndst = 3 + (n + 5) * count
    want_crc = np.asarray(O.batch_fixed(method, host[9:], n, n, count), dtype=np.uint64)
    want = _expected_dst(host, so, ds, ndst)
    src, sod, dsd = torch.from_numpy(host).cuda(), _dev(torch, so), _dev(torch, ds)
    before = G.queue_stats()
    dst = torch.full((ndst,), CANARY, dtype=torch.uint8, device="cuda")
    out = G.copy_offsets(method, src, sod, dst, dsd)
    assert np.array_equal(G.as_unsigned(out).astype(np.uint64), want_crc)
    assert np.array_equal(dst.cpu().numpy(), want)
    dst.fill_(CANARY)
    state = G.state_init(method, count)
    G.update_copy_offsets(method, src, sod, dst, dsd, state)
    assert np.array_equal(_get(G, method, state), want_crc)
    assert np.array_equal(dst.cpu().numpy(), want)
    assert np.array_equal(src.cpu().numpy(), host)
    if count == 1025:
        torch.cuda.synchronize()
        assert G.queue_stats()["slot"] - before["slot"] >= 2, "the 1025-chunk calls took no work-queue slot"


def _ring_off64():
    text = open(os.path.join(ROOT, "mercury_amd", "csrc", "crc_gpu_shape.h")).read()
    return int(re.search(r"constexpr int kRingOff64 = (\d+);", text).group(1))


@pytest.mark.parametrize("nt", [None, "1"])
def test_crc64_step_and_ring_boundaries(gpu, nt, monkeypatch):
    """Chunk lengths around one 1 KiB step, one ring of steps and two rings of
    the CRC-64 loop, at source residues 0, 1, 8, 15 and destination residues
    0, 3, 15.  Filler chunks between them (copied and checked too) put every
    chunk at its residue."""
    import torch
    if nt is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_NT", nt)
    R = _ring_off64()
    sizes = [1023, 1024, 1025, 1024 * R - 1, 1024 * R + 1, 2048 * R - 1, 2048 * R + 1]
    rng = np.random.default_rng(64)
    lens, ds, want_sres, want_dres = [], [], [], []
    spos, dpos = 16, 0
    for sr in (0, 1, 8, 15):
        for dr in (0, 3, 15):
            for n in sizes:
                fill = (sr - spos) % 16  # a filler chunk up to the wanted source residue
                lens.append(fill)
                ds.append(dpos)
                dpos += fill + int(rng.integers(0, 9))
                spos += fill
                dpos += (dr - dpos) % 16
                lens.append(n)
                ds.append(dpos)
                want_sres.append(sr)
                want_dres.append(dr)
                dpos += n + int(rng.integers(0, 9))
                spos += n
    lens, ds = np.asarray(lens, dtype=np.int64), np.asarray(ds, dtype=np.int64)
    so = 16 + np.concatenate([[0], np.cumsum(lens)])
    assert (so[:-1][1::2] % 16).tolist() == want_sres and (ds[1::2] % 16).tolist() == want_dres
    buf = rng.integers(0, 256, size=int(so[-1]) + 7, dtype=np.uint8)
    ndst = dpos
    want = _expected_dst(buf, so, ds, ndst)
    want_crc = _crcs("crc64", [buf[a:b] for a, b in zip(so[:-1], so[1:])])
    sod, dsd = _dev(torch, so), _dev(torch, ds)
    sbase, sview, dbase, dview = _device(torch, buf, 0, 0, ndst)  # 16-byte-aligned views: the residues are the tables'
    out = gpu.copy_offsets("crc64", sview, sod, dview, dsd, offsets_host=so, dst_starts_host=ds)
    assert np.array_equal(gpu.as_unsigned(out).astype(np.uint64), want_crc)
    _check_dst(dbase, 0, want, "copy_offsets")
    dbase.fill_(CANARY)
    state = gpu.state_init("crc64", len(lens))
    gpu.update_copy_offsets("crc64", sview, sod, dview, dsd, state, offsets_host=so, dst_starts_host=ds)
    assert np.array_equal(_get(gpu, "crc64", state), want_crc)
    _check_dst(dbase, 0, want, "update_copy_offsets")


@pytest.mark.parametrize("count", [64, 2000])
@pytest.mark.parametrize("method", ["crc32c", "crc64"])
def test_graph_replay(gpu, report, method, count):
    """prepare, then one update_copy_offsets and one copy_offsets captured on a
    side stream and replayed twice: the state has advanced twice, the outputs
    and both destinations are the same after either replay, the error word is
    0 (count 64: the light CRC-32C kernel; 2000: the full kernels' static
    split, a capture gets no queue slot)."""
    import torch
    G = gpu
    rng = np.random.default_rng(5 + count)
    lens = rng.integers(0, 400, count)
    lens[[1, count // 3]] = 0
    so = 9 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ds, ndst = _scatter(rng, lens, 9)
    buf = rng.integers(0, 256, size=int(so[-1]) + 64, dtype=np.uint8)
    chunks = [buf[a:b] for a, b in zip(so[:-1], so[1:])]
    want_crc, want_twice = _crcs(method, chunks), _crcs(method, [np.concatenate([c, c]) for c in chunks])
    want = _expected_dst(buf, so, ds, ndst)
    G.prepare(method)
    src, sod, dsd = torch.from_numpy(buf).cuda(), _dev(torch, so), _dev(torch, ds)
    dst_u = torch.full((ndst,), CANARY, dtype=torch.uint8, device="cuda")
    dst_c = torch.full((ndst,), CANARY, dtype=torch.uint8, device="cuda")
    out = torch.zeros(count, dtype=G.out_dtype(method), device="cuda")
    state = G.state_init(method, count)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        G.update_copy_offsets(method, src, sod, dst_u, dsd, state)
        G.copy_offsets(method, src, sod, dst_c, dsd, out=out)
    torch.cuda.synchronize()
    assert bool((dst_u == CANARY).all()) and bool((dst_c == CANARY).all())  # the capture itself ran nothing
    for r in range(2):
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        assert np.array_equal(G.as_unsigned(out).astype(np.uint64), want_crc), ("replay", r)
        assert np.array_equal(dst_u.cpu().numpy(), want) and np.array_equal(dst_c.cpu().numpy(), want), ("replay", r)
        assert np.array_equal(_get(G, method, state), want_twice if r else want_crc), ("replay", r)
    assert int(report[0].item()) == 0


def test_chunk_past_2_gib_crc64(gpu):
    """A chunk of more than 2^31 bytes takes the 64-bit-length loop
    (payload64_generic), which stores by the same rule; between two small
    neighbours, source and destination misaligned by an odd number of bytes.
    The values are the streaming API's over the host copy of the source."""
    import torch

    from mercury_amd import _lib
    big = (1 << 31) + 4096 * 3 + 5
    lens = np.array([100, big, 4097])
    total = int(lens.sum())
    if torch.cuda.mem_get_info()[0] < 2 * total + (1 << 30):
        pytest.skip("not enough free device memory for a 2 GiB source and destination")
    so = 16 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ds = np.array([7, 7 + 100 + 9 + 4097 + 12, 7 + 100 + 9], dtype=np.int64)  # the big chunk last in the destination
    assert int(so[1] - ds[1]) % 2 == 1
    src = torch.empty(int(so[-1]) + 64, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(src, 0xB64)
    host = src.cpu().numpy()
    L = _lib.load_library()
    want = []
    for i in range(3):
        obj, val = ctypes.c_void_p(), ctypes.c_uint64(0)
        assert L.mchecksum_init(b"crc64", ctypes.byref(obj)) == 0
        assert L.mchecksum_update(obj, host.ctypes.data + int(so[i]), int(lens[i])) == 0
        assert L.mchecksum_get(obj, ctypes.byref(val), 8, 1) == 0
        L.mchecksum_destroy(obj)
        want.append(val.value)
    del host
    ndst = int(ds[1]) + big
    dst = torch.full((ndst,), CANARY, dtype=torch.uint8, device="cuda")
    out = gpu.copy_offsets("crc64", src, _dev(torch, so), dst, _dev(torch, ds), offsets_host=so, dst_starts_host=ds)
    assert gpu.as_unsigned(out).astype(np.uint64).tolist() == want
    for i in range(3):  # compared on the device, in slices
        a, d, n = int(so[i]), int(ds[i]), int(lens[i])
        for at in range(0, n, 1 << 28):
            k = min(1 << 28, n - at)
            assert torch.equal(dst[d + at:d + at + k], src[a + at:a + at + k]), (i, at)
    # the gaps: before the first chunk, between the two small ones, between them and the big one
    for lo, hi in ((0, 7), (107, 116), (116 + 4097, int(ds[1]))):
        assert bool((dst[lo:hi] == CANARY).all()), (lo, hi)


def test_no_fault_and_no_error_word_after_all_of_the_above(gpu, report):
    import torch
    word, faults0 = report
    torch.cuda.synchronize()
    assert int(word.item()) == 0
    assert gpu.queue_faults() == faults0
