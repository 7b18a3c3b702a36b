"""mchecksum_gpu_combine_runs on the GPU (include/mchecksum_gpu.h): the CRCs
of each run's chunks, joined in order, are the CRC of the run's bytes.  The
reference is the oracle's CRC of those bytes; where the lengths are too large
to have bytes, the pairwise mchecksum_gpu_combine chain.  The CPU half of the
algebra is tests/test_join_runs.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ("crc32c", "crc32", "crc64", "crc64-ecma182")
EMETHOD, EINVAL = -3, -1
POOL = np.asarray([0, 1, 15, 16, 17, 255, 4096, 4097])
# an empty run first, in the middle and last; 5000 is past the 4096 chunks a single wave takes
RUN_SIZES = (0, 1, 2, 3, 63, 64, 0, 65, 255, 256, 257, 1000, 5000, 0)
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u64(G, t):
    return G.as_unsigned(t).astype(np.uint64)


def _lens(rng, n, pool_share=0.08, top=512):
    lens = rng.integers(0, top + 1, n)
    pick = rng.random(n) < pool_share
    lens[pick] = rng.choice(POOL, int(pick.sum()))
    return lens.astype(np.int64)


def _first(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


class _Batch:
    """Chunks of real bytes: host data, chunk lengths and byte offsets, run
    table; per method the chunk CRCs (checksum_offsets, on the device) and
    the oracle's CRC of every run's bytes, computed once."""

    def __init__(self, O, sizes, seed, rng, **lens_kw):
        self.O = O
        self.first = _first(sizes)
        self.lens = _lens(rng, int(self.first[-1]), **lens_kw)
        self.offs = _first(self.lens)
        self.host = O.splitmix_bytes(int(self.offs[-1]) + 64, seed)
        self.run_offs = self.offs[self.first]
        self.run_bytes = (self.run_offs[1:] - self.run_offs[:-1]).astype(np.int64)
        self._cache = {}

    def on_device(self, G, torch, method):
        """(chunk CRCs, lens, run_first) device tensors and the wanted values."""
        if method not in self._cache:
            data = _dev(torch, self.host)
            crc = G.checksum_offsets(method, data, _dev(torch, self.offs), offsets_host=self.offs)
            want = np.asarray(self.O.batch_offsets(method, self.host, self.run_offs.astype(np.uint64)), dtype=np.uint64)
            self._cache[method] = (crc, _dev(torch, self.lens), _dev(torch, self.first), want)
        return self._cache[method]


@pytest.fixture(scope="module")
def batch(oracle_mod):
    b = _Batch(oracle_mod, RUN_SIZES, 0xC0B1, np.random.default_rng(0xC0B1))
    assert 1.5e6 < b.offs[-1] < 3e6 and set(POOL.tolist()) <= set(b.lens.tolist())
    return b


def _check(G, got, got_len, want, want_len, what):
    bad = np.nonzero(_u64(G, got) != want)[0]
    assert bad.size == 0, (what, "runs", bad[:8])
    if got_len is not None:
        assert np.array_equal(got_len.cpu().numpy(), want_len), what


@pytest.mark.parametrize("method", METHODS)
def test_parity_with_the_oracle(gpu, batch, method):
    """Runs of 0 .. 5000 chunks in one call: every out[j] is the oracle's CRC
    of the run's bytes, every out_len[j] its byte total."""
    import torch
    crc, lens, first, want = batch.on_device(gpu, torch, method)
    out, out_len = gpu.combine_runs(method, crc, lens, first, out_len=True, run_first_host=batch.first)
    _check(gpu, out, out_len, want, batch.run_bytes, method)
    # without out_len: the values alone
    assert np.array_equal(_u64(gpu, gpu.combine_runs(method, crc, lens, first)), want)


@pytest.mark.parametrize("method", METHODS)
def test_agrees_with_the_combine_fold_and_with_checksum_offsets(gpu, batch, method):
    """The same tables through the calls that existed before: K - 1 combine
    launches folding every run left to right, and checksum_offsets over the
    whole runs."""
    import torch
    G = gpu
    crc, lens, first, want = batch.on_device(G, torch, method)
    got = _u64(G, G.combine_runs(method, crc, lens, first))
    sizes = np.asarray(RUN_SIZES)
    start = first[:-1]
    acc = G.state_get(method, G.state_init(method, len(RUN_SIZES)))  # CRC of the empty message
    live = _dev(torch, np.nonzero(sizes > 0)[0])
    acc[live] = crc[start[live]]
    idx = live
    for k in range(1, max(RUN_SIZES)):
        if idx.numel() != int((sizes > k).sum()):  # the runs that have a chunk k
            idx = _dev(torch, np.nonzero(sizes > k)[0])
        at = start[idx] + k
        acc[idx] = G.combine(method, acc[idx], crc[at], lens[at])
    assert np.array_equal(_u64(G, acc), got)
    whole = G.checksum_offsets(method, _dev(torch, batch.host), _dev(torch, batch.run_offs))
    assert np.array_equal(_u64(G, whole), got)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("method", METHODS)
def test_every_path_boundary(gpu, oracle_mod, method):
    """Run sizes where the kernel changes path: one slice per lane and two
    (64, 65, 128, 129), the last run a wave takes and the first the workgroup
    takes (4096, 4097), a workgroup run that leaves lanes without a slice
    (4097 = 241 slices of 17), and a group of fewer than four runs at the end."""
    import torch
    sizes = (64, 65, 128, 129, 4095, 4096, 4097, 4353, 8191, 7)
    b = _Batch(oracle_mod, sizes, 0xB0DE, np.random.default_rng(7), pool_share=0.02, top=48)
    crc, lens, first, want = b.on_device(gpu, torch, method)
    out, out_len = gpu.combine_runs(method, crc, lens, first, out_len=True, run_first_host=b.first)
    _check(gpu, out, out_len, want, b.run_bytes, method)


@pytest.mark.parametrize("method", ["crc32c", "crc64"])
def test_more_runs_than_the_grid_holds(gpu, oracle_mod, method):
    """262144 + 4101 runs of 0 .. 3 chunks: workgroups stride past the grid's
    65536 groups of four runs."""
    import torch
    rng = np.random.default_rng(11)
    b = _Batch(oracle_mod, rng.integers(0, 4, 4 * 65536 + 4101), 0x6A1D, rng, pool_share=0.0, top=12)
    crc, lens, first, want = b.on_device(gpu, torch, method)
    out, out_len = gpu.combine_runs(method, crc, lens, first, out_len=True)
    _check(gpu, out, out_len, want, b.run_bytes, method)


@pytest.mark.parametrize("method", METHODS)
def test_lengths_that_cannot_be_materialised(gpu, method):
    """Chunks of up to 2^40 bytes with arbitrary CRC words, runs of 2 .. 9
    chunks: the reference is the pairwise combine chain."""
    import torch
    G = gpu
    rng = np.random.default_rng(40)
    sizes = np.concatenate([np.arange(2, 10), rng.integers(2, 10, 192)])
    first = _first(sizes)
    n = int(first[-1])
    lens = rng.integers(1, (1 << 40) + 1, n).astype(np.int64)
    lens[:6] = [1 << 40, (1 << 40) - 1, 0x0123456789, 1, 0xFFFFFFFFF, 1 << 36]
    words = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    dt = G.out_dtype(method)
    crc = _dev(torch, words.astype(np.uint32).view(np.int32) if dt == torch.int32 else words.view(np.int64))
    lens_d, first_d = _dev(torch, lens), _dev(torch, first)
    out, out_len = G.combine_runs(method, crc, lens_d, first_d, out_len=True, run_first_host=first)
    sizes_d, start = _dev(torch, sizes), first_d[:-1]
    acc = crc[start].clone()
    for k in range(1, 9):
        idx = torch.nonzero(sizes_d > k).flatten()
        at = start[idx] + k
        acc[idx] = G.combine(method, acc[idx], crc[at], lens_d[at])
    assert np.array_equal(_u64(G, out), _u64(G, acc))
    assert np.array_equal(out_len.cpu().numpy(), np.add.reduceat(lens, first[:-1]))


@pytest.mark.parametrize("method", METHODS)
def test_ignored_chunks(gpu, batch, method):
    """Zero-length chunks carrying poison words, and chunks outside
    [first[0], first[nruns]) carrying poison words and lengths, change no
    output."""
    import torch
    G = gpu
    crc, lens, first, want = batch.on_device(G, torch, method)
    pv = POISON.astype(np.uint32).view(np.int32) if crc.dtype == torch.int32 else POISON.view(np.int64)
    poison = torch.full((1,), int(pv), dtype=crc.dtype, device="cuda")
    assert int((lens == 0).sum()) > 10
    pcrc = torch.where(lens == 0, poison, crc)
    pad = 5
    pcrc = torch.cat([poison.expand(pad), pcrc, poison.expand(pad)]).contiguous()
    plens = torch.cat([torch.full((pad,), 0x2525252525, dtype=torch.int64, device="cuda"), lens,
                       torch.full((pad,), 0x2525252525, dtype=torch.int64, device="cuda")]).contiguous()
    out, out_len = G.combine_runs(method, pcrc, plens, first + pad, out_len=True)
    _check(G, out, out_len, want, batch.run_bytes, method)


@pytest.mark.parametrize("method", METHODS)
def test_two_level_join(gpu, batch, method):
    """All of the batch's chunks as one run: joined in one level (one
    workgroup), and in two -- runs of 64, then one run over their (out,
    out_len) -- the value is the oracle's CRC of all the bytes."""
    import torch
    G = gpu
    crc, lens, _, _ = batch.on_device(G, torch, method)
    n = crc.numel()
    assert n % 64 != 0 and n > 4096
    one, one_len = G.combine_runs(method, crc, lens, _dev(torch, np.asarray([0, n], dtype=np.int64)), out_len=True)
    first1 = np.append(np.arange(0, n, 64), n).astype(np.int64)
    mid, mid_len = G.combine_runs(method, crc, lens, _dev(torch, first1), out_len=True, run_first_host=first1)
    two, two_len = G.combine_runs(method, mid, mid_len, _dev(torch, np.asarray([0, len(first1) - 1], dtype=np.int64)),
                                  out_len=True)
    want = batch.O.crc(method, batch.host[:int(batch.offs[-1])])
    assert int(_u64(G, one)[0]) == want and int(_u64(G, two)[0]) == want
    assert int(one_len[0]) == int(two_len[0]) == int(batch.offs[-1])


@pytest.mark.parametrize("method", ["crc32c", "crc64-ecma182"])
def test_graph_replay_reads_the_tables_again(gpu, oracle_mod, method):
    """prepare, one call captured on a side stream, three replays with the
    CRCs, the lengths and the run boundaries rewritten in between: every
    replay gives the oracle's values for the tables it found.  And one eager
    call on a non-default stream."""
    import torch
    G, O = gpu, oracle_mod
    nruns, nchunks = 11, 6000
    variants = []
    for r in range(3):
        rng = np.random.default_rng(60 + r)
        cuts = np.sort(rng.integers(0, nchunks + 1, nruns - 1))
        if r == 1:
            cuts[:] = np.sort(rng.integers(0, 900, nruns - 1))  # the last run: 5100 chunks and more, the workgroup's
        sizes = np.diff(np.concatenate([[0], cuts, [nchunks]]))
        b = _Batch(O, sizes, 0x6A00 + r, rng, pool_share=0.02, top=64)
        variants.append((b,) + b.on_device(G, torch, method))
    G.prepare(method)
    crc = torch.zeros_like(variants[0][1])
    lens, first = torch.zeros_like(variants[0][2]), torch.zeros_like(variants[0][3])
    out = torch.zeros(nruns, dtype=G.out_dtype(method), device="cuda")
    out_len = torch.zeros(nruns, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        G.combine_runs(method, crc, lens, first, out=out, out_len=out_len)
    torch.cuda.synchronize()
    assert not bool(out.any()), "the capture itself ran the kernel"
    for r, (b, vcrc, vlens, vfirst, want) in enumerate(variants):
        with torch.cuda.stream(s):
            crc.copy_(vcrc)
            lens.copy_(vlens)
            first.copy_(vfirst)
            g.replay()
        s.synchronize()
        _check(G, out, out_len, want, b.run_bytes, (method, "replay", r))
    b, vcrc, vlens, vfirst, want = variants[1]
    with torch.cuda.stream(s):
        o2, l2 = G.combine_runs(method, vcrc, vlens, vfirst, out_len=True, stream=s)
    s.synchronize()
    _check(G, o2, l2, want, b.run_bytes, (method, "side stream"))


def test_arguments(gpu, oracle_mod):
    """Refusals before any GPU work, the empty calls, and the fault count."""
    import torch
    G, O = gpu, oracle_mod
    L = G._lib()
    faults = L.mchecksum_gpu_queue_faults()
    mark = 0x5A5A5A5A5A5A5A5A
    crc = torch.full((8,), mark, dtype=torch.int64, device="cuda")
    lens = torch.ones(8, dtype=torch.int64, device="cuda")
    first = _dev(torch, np.asarray([0, 3, 3, 8], dtype=np.int64))
    out = torch.full((8,), mark, dtype=torch.int64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    call = L.mchecksum_gpu_combine_runs
    # NULL tables
    assert call(b"crc64", None, p(lens), 8, p(first), 3, p(out), None, None) == EINVAL
    assert b"NULL" in L.mchecksum_gpu_last_error()
    assert call(b"crc64", p(crc), None, 8, p(first), 3, p(out), None, None) == EINVAL
    assert call(b"crc64", p(crc), p(lens), 8, None, 3, p(out), None, None) == EINVAL
    assert call(b"crc64", p(crc), p(lens), 8, p(first), 3, None, None, None) == EINVAL
    assert call(b"crc64", None, None, 8, None, 0, None, None, None) == EINVAL  # chunks need their tables
    # the caps
    big = (1 << 31) + 1
    assert call(b"crc64", p(crc), p(lens), 8, p(first), big, p(out), None, None) == EINVAL
    assert b"2^31" in L.mchecksum_gpu_last_error()
    assert call(b"crc64", p(crc), p(lens), big, p(first), 3, p(out), None, None) == EINVAL
    assert b"2^31" in L.mchecksum_gpu_last_error()
    # NULL comes before the method, the method after
    assert call(b"crc16", None, p(lens), 8, p(first), 3, p(out), None, None) == EINVAL
    assert call(b"crc16", p(crc), p(lens), 8, p(first), 3, p(out), None, None) == EMETHOD
    assert call(b"nope", p(crc), p(lens), 8, p(first), 3, p(out), None, None) == EMETHOD
    assert call(b"crc16", None, None, 0, None, 0, None, None, None) == EMETHOD
    # no runs: no buffers, no launch
    assert call(b"crc32c", None, None, 0, None, 0, None, None, None) == 0
    assert call(b"crc64", p(crc), p(lens), 8, p(first), 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == mark).all())
    # no chunks, three runs: three CRCs of the empty message, three zero lengths
    for method in ("crc32c", "crc64-ecma182"):
        o = torch.full((3,), -1, dtype=G.out_dtype(method), device="cuda")
        n = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        zeros = torch.zeros(4, dtype=torch.int64, device="cuda")
        assert call(method.encode(), None, None, 0, p(zeros), 3, p(o), p(n), None) == 0
        assert _u64(G, o).tolist() == [O.crc(method, b"")] * 3 and n.tolist() == [0, 0, 0]
    assert L.mchecksum_gpu_queue_faults() == faults
    # ... and the wrapper checks tensors and the host table
    ok32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc64", ok32, lens, first)  # wrong dtype for the method
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", ok32, lens[:4], first)  # fewer lengths than chunks
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", ok32, lens, first.to(torch.int32))
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", ok32, lens, first.cpu())
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", ok32, lens, first, out=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", ok32, lens, first, out_len=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", ok32, lens, first, run_first_host=[0, 5, 3, 8])  # decreasing
    with pytest.raises(G.GpuChecksumError):
        G.combine_runs("crc32c", ok32, lens, first, run_first_host=[0, 3, 3, 9])  # past the last chunk
