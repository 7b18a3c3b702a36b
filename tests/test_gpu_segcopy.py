"""GPU parity of mchecksum_gpu_gather_segments / _scatter_segments through the
Python wrappers: the values against the oracle (as tests/test_gpu_ext.py's
_want), the copied bytes against a host-side concatenation or split of the same
buffer, and every byte around them -- gaps, guards, segments outside every
object, the side that is read -- against what it held before.

Naming: the side that is read holds random bytes; the side that is written is
a tensor of its own filled with a sentinel.  gather reads segments at random,
possibly overlapping offsets of the 24 MiB `buf` and writes object ranges;
scatter reads object ranges and writes segments, and since the wrappers refuse
object ranges that overlap, its source is a tensor of its own with the ranges
placed like the written ones."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64
DIRS = ["gather", "scatter"]
METHODS = ["crc32c", "crc64", "crc64-ecma182"]
# test_gpu_ext._objects' length pool
POOL = [0, 1, 3, 7, 8, 15, 16, 17, 63, 64, 100, 1000, 4095, 4096, 4097, 65536, 100003, 262143, 262144, 262145, 600000,
        1 << 20, (1 << 20) + 5]
K = 256 << 10


@pytest.fixture(scope="module")
def buf(gpu):
    import torch
    t = torch.empty((24 << 20) + 64, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(t, 0x5E6C)
    return t


@pytest.fixture(scope="module")
def host(buf):
    return buf.cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _no_fault_in_this_file(gpu):
    """After all tests of the file: no queue fault was counted and no call
    reported on the error word."""
    import torch
    before = gpu.queue_faults()
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    gpu.set_error_word(word)
    yield
    torch.cuda.synchronize()
    gpu.set_error_word(None)
    assert int(word.item()) == 0, "a gather / scatter call reported on the error word"
    assert gpu.queue_faults() == before


def _place(rng, sizes, residues=None):
    """Ranges of the given sizes in a permuted order, 0..31 bytes apart (or at
    the given residues mod 16, at least a byte apart), GUARD bytes before the
    first and after the last: (offsets, total bytes)."""
    off = np.zeros(len(sizes), dtype=np.int64)
    at = GUARD
    for i in rng.permutation(len(sizes)):
        at += int(rng.integers(0, 32))
        if residues is not None:
            at += (int(residues[i]) - at) % 16
        off[i] = at
        at += int(sizes[i]) + (1 if residues is not None else 0)
    return off, at + 31 + GUARD


def _run(gpu, oracle_mod, method, direction, buf, host, lens, first, read_at, write_at, wsize):
    """One call and all its checks.  gather: read_at[s] = segment s's offset in
    buf, write_at[j] = object j's start in the written tensor; scatter:
    read_at[j] = object j's start in buf, write_at[s] = segment s's offset in
    the written tensor.  Returns the CRCs."""
    import torch
    lens, first = [int(x) for x in lens], [int(x) for x in first]
    w = torch.full((wsize,), SENT, dtype=torch.uint8, device="cuda")
    exp = np.full(wsize, SENT, dtype=np.uint8)
    want = []
    for j in range(len(first) - 1):
        ss = range(first[j], first[j + 1])
        if direction == "gather":
            b = np.concatenate([host[read_at[s]:read_at[s] + lens[s]] for s in ss] + [np.zeros(0, dtype=np.uint8)])
            exp[write_at[j]:write_at[j] + len(b)] = b
        else:
            b = host[read_at[j]:read_at[j] + sum(lens[s] for s in ss)]
            pos = 0
            for s in ss:
                exp[write_at[s]:write_at[s] + lens[s]] = b[pos:pos + lens[s]]
                pos += lens[s]
        want.append(oracle_mod.crc(method, np.ascontiguousarray(b)))
    if direction == "gather":
        views = [buf[int(o):int(o) + n] for o, n in zip(read_at, lens)]
        out = gpu.gather_segments(method, views, w, [int(x) for x in write_at], first)
    else:
        views = [w[int(o):int(o) + n] for o, n in zip(write_at, lens)]
        out = gpu.scatter_segments(method, buf, [int(x) for x in read_at], views, first)
    got = gpu.as_unsigned(out).tolist()
    assert got == want
    wh = w.cpu().numpy()
    bad = np.nonzero(wh != exp)[0]
    assert bad.size == 0, f"{bad.size} written-side bytes differ, first at {bad[:5]}"
    assert np.array_equal(buf.cpu().numpy(), host), "the side that is read changed"
    return got


def _layout(gpu, rng, direction, buf, host, lens, first, read_res=None, write_res=None, buf_len=24 << 20):
    """Both sides for _run: (the read tensor, its host copy, read_at, write_at,
    wsize).  gather: segments at random offsets of buf (or residues); scatter:
    object ranges placed by _place in a source of their own.  The written side
    is placed by _place."""
    import torch
    lens, first = np.asarray(lens, dtype=np.int64), np.asarray(first, dtype=np.int64)
    P = np.concatenate([[0], np.cumsum(lens)])
    N = P[first[1:]] - P[first[:-1]]
    if direction == "gather":
        read_at = np.array([int(rng.integers(0, buf_len - int(n))) for n in lens], dtype=np.int64)
        if read_res is not None:
            read_at = read_at - read_at % 16 + np.asarray(read_res)
        write_at, wsize = _place(rng, N, write_res)
        return buf, host, read_at, write_at, wsize
    read_at, rsize = _place(rng, N, read_res)
    src = torch.empty(rsize + 64, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(src, 0x5CA7)
    write_at, wsize = _place(rng, lens, write_res)
    return src, src.cpu().numpy(), read_at, write_at, wsize


def _objects(rng, nobj, max_seg=6, pool=POOL):
    lens, first = [], [0]
    for _ in range(nobj):
        for _ in range(int(rng.integers(0, max_seg + 1))):
            lens.append(int(pool[int(rng.integers(0, len(pool)))]))
        first.append(len(lens))
    return lens, first


# 1 ---------------------------------------------------------------- random --
@pytest.mark.parametrize("method,map_cap", [(m, None) for m in METHODS] + [("crc64", "0"), ("crc64", "40")])
@pytest.mark.parametrize("direction", DIRS)
def test_random_objects(gpu, buf, host, oracle_mod, direction, method, map_cap, monkeypatch):
    """120 objects of 0..6 segments from the segment tests' length pool,
    everything at random byte offsets, the written ranges permuted with 0..31
    byte gaps.  map_cap: the CRC-64 queue pass's chunk map forced off ("0") or
    too small ("40"), as in tests/test_gpu_ext.py."""
    if map_cap is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_SEG_MAP_CAP", map_cap)
    rng = np.random.default_rng(177 + METHODS.index(method) + 10 * DIRS.index(direction))
    lens, first = _objects(rng, 120)
    src, src_host, read_at, write_at, wsize = _layout(gpu, rng, direction, buf, host, lens, first)
    _run(gpu, oracle_mod, method, direction, src, src_host, lens, first, read_at, write_at, wsize)


# 2 -------------------------------------------------------------- residues --
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("direction", DIRS)
def test_residues(gpu, buf, host, oracle_mod, direction, method):
    """One segment per object: every load residue x store residue x length of
    the lists below in one call."""
    rng = np.random.default_rng(5)
    cases = [(lr, sr, n) for lr in (0, 1, 7, 15) for sr in (0, 3, 8, 15)
             for n in (0, 1, 3, 4, 7, 8, 15, 16, 17, 1023, 1024, 1025)]
    lens = [c[2] for c in cases]
    first = list(range(len(cases) + 1))
    src, src_host, read_at, write_at, wsize = _layout(gpu, rng, direction, buf, host, lens, first,
                                                      [c[0] for c in cases], [c[1] for c in cases])
    assert all(int(src.data_ptr() + r) % 16 == c[0] for r, c in zip(read_at, cases))
    assert all(int(w) % 16 == c[1] for w, c in zip(write_at, cases))  # (fresh tensors start on a 16-byte boundary)
    _run(gpu, oracle_mod, method, direction, src, src_host, lens, first, read_at, write_at, wsize)


# 3 ----------------------------------------------------------- chunk edges --
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("direction", DIRS)
def test_chunk_edges(gpu, buf, host, oracle_mod, direction, method):
    """Lengths on and around the 256 KiB chunk; one 20 MiB segment read at
    offset 3 and written at residue 5; one object of three segments whose joins
    fall inside a 16-byte piece."""
    rng = np.random.default_rng(9)
    lens = [K - 1, K, K + 1, 2 * K, 3 * K + 13, 0, 1, 5, 262139, 17]
    first = [0, 1, 2, 3, 4, 5, 6, 7, 10]
    src, src_host, read_at, write_at, wsize = _layout(gpu, rng, direction, buf, host, lens, first)
    _run(gpu, oracle_mod, method, direction, src, src_host, lens, first, read_at, write_at, wsize)
    big = 20 << 20
    _run(gpu, oracle_mod, method, direction, buf, host, [big], [0, 1], [3], [GUARD + 5], big + 2 * GUARD + 16)


# 4 ----------------------------------------------------------- scan blocks --
@pytest.mark.parametrize("nseg", [1, 1024, 1025])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("direction", DIRS)
def test_scan_blocks(gpu, buf, host, oracle_mod, direction, method, nseg):
    """Lists of one scan block, exactly one and one more: segments of 1..40
    bytes with runs of empty ones in front, a handful of objects over a
    sub-range of the list.  The segments outside it keep their sentinel on
    scatter (the whole written tensor is compared) and are not gathered."""
    rng = np.random.default_rng(40 + nseg)
    lens = rng.integers(1, 41, size=nseg)
    lens[:min(nseg // 3, 70)] = 0  # leading empty segments, some outside and some inside the first object
    if nseg == 1:
        lens[0] = 23
        first = [0, 0, 1, 1]
    else:
        cuts = np.sort(rng.integers(5, nseg - 3, size=6))
        cuts[3] = cuts[2]  # an empty object
        first = [5] + cuts.tolist() + [nseg - 3]
    src, src_host, read_at, write_at, wsize = _layout(gpu, rng, direction, buf, host, lens, first, buf_len=1 << 20)
    _run(gpu, oracle_mod, method, direction, src, src_host, lens, first, read_at, write_at, wsize)


# 5 ---------------------------------------------------------- empty inputs --
@pytest.mark.parametrize("direction", DIRS)
def test_empty_inputs_and_refusals(gpu, buf, host, oracle_mod, direction):
    import torch
    rng = np.random.default_rng(3)
    for method in METHODS:
        # empty objects only: nothing is written, every value the empty CRC
        lens, first = [0, 0, 9], [0, 0, 2, 2]
        src, src_host, read_at, write_at, wsize = _layout(gpu, rng, direction, buf, host, lens, first)
        got = _run(gpu, oracle_mod, method, direction, src, src_host, lens, first, read_at, write_at, wsize)
        assert got == [oracle_mod.crc(method, np.zeros(0, dtype=np.uint8))] * 3
        # no objects at all
        per_obj, per_seg = [], [100 if direction == "gather" else GUARD]
        _run(gpu, oracle_mod, method, direction, buf, host, [4], [1], *((per_seg, per_obj) if direction == "gather"
                                                                         else (per_obj, per_seg)), 2 * GUARD + 4)
        _run(gpu, oracle_mod, method, direction, buf, host, [], [0], [], [], 2 * GUARD)
    w = torch.full((256,), SENT, dtype=torch.uint8, device="cuda")

    def call(method, first, starts=(64,)):
        if direction == "gather":
            return gpu.gather_segments(method, [buf[:10]], w, list(starts), first)
        return gpu.scatter_segments(method, buf, list(starts), [w[64:74]], first)

    with pytest.raises(gpu.GpuChecksumError):
        call("crc16", [0, 1])  # no GPU segment kernel for 16-bit models
    with pytest.raises(gpu.GpuChecksumError):
        call("crc32c", [0, 2])  # first runs past nseg
    with pytest.raises(ValueError):
        call("crc32c", [0, 1], starts=(64, 80))
    torch.cuda.synchronize()
    assert bool((w == SENT).all()), "a refused call wrote"


# 6 ------------------------------------------------------------- graph capture --
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("direction", DIRS)
def test_graph_capture_with_new_lengths(gpu, buf, host, oracle_mod, direction, method):
    """One captured SegmentBatch.gather / .scatter, three replays, the lengths
    rewritten (set_lengths) before each: 1300 segments (two scan blocks) in 40
    objects.  Every replay must give the oracle's values and the bytes of
    THAT replay's lengths; what lies beyond them keeps the sentinel written
    before the replay."""
    import torch
    rng = np.random.default_rng(66)
    nseg, nobj = 1300, 40
    cap = rng.integers(0, 300, size=nseg)
    cap[rng.integers(0, nseg, size=8)] = rng.integers(K - 40, K + 300, size=8)
    first = np.sort(np.concatenate([[0, nseg], rng.integers(0, nseg + 1, size=nobj - 1)]))
    src, host, read_at, write_at, wsize = _layout(gpu, rng, direction, buf, host, cap, first)
    w = torch.empty(wsize, dtype=torch.uint8, device="cuda")
    if direction == "gather":
        batch = gpu.SegmentBatch([buf[int(o):int(o) + int(n)] for o, n in zip(read_at, cap)], first)
        starts_host = write_at
    else:
        batch = gpu.SegmentBatch([w[int(o):int(o) + int(n)] for o, n in zip(write_at, cap)], first)
        starts_host = read_at
    starts = torch.from_numpy(np.ascontiguousarray(starts_host)).cuda()
    out = torch.zeros(nobj, dtype=gpu.out_dtype(method), device="cuda")
    gpu.prepare(method)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        if direction == "gather":
            batch.gather(method, w, starts, out=out, dst_starts_host=starts_host)
        else:
            batch.scatter(method, src, starts, out=out, src_starts_host=starts_host)
    steps = [cap, np.where(rng.integers(0, 3, size=nseg) == 0, cap // 2, cap), np.minimum(cap, rng.integers(0, 200, size=nseg))]
    for r, lens in enumerate(steps):
        sent = SENT ^ (r + 1)
        w.fill_(sent)
        out.zero_()
        torch.cuda.synchronize()
        batch.set_lengths(lens, stream=s)
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        exp = np.full(wsize, sent, dtype=np.uint8)
        want = []
        for j in range(nobj):
            ss = range(int(first[j]), int(first[j + 1]))
            if direction == "gather":
                b = np.concatenate([host[read_at[t]:read_at[t] + int(lens[t])] for t in ss] + [np.zeros(0, dtype=np.uint8)])
                exp[write_at[j]:write_at[j] + len(b)] = b
            else:
                b = host[read_at[j]:read_at[j] + int(sum(int(lens[t]) for t in ss))]
                pos = 0
                for t in ss:
                    exp[write_at[t]:write_at[t] + int(lens[t])] = b[pos:pos + int(lens[t])]
                    pos += int(lens[t])
            want.append(oracle_mod.crc(method, np.ascontiguousarray(b)))
        assert gpu.as_unsigned(out).tolist() == want, f"replay {r}"
        bad = np.nonzero(w.cpu().numpy() != exp)[0]
        assert bad.size == 0, f"replay {r}: {bad.size} written-side bytes differ, first at {bad[:5]}"
    torch.cuda.synchronize()


# 7 -------------------------------------------------------- non-temporal path --
@pytest.mark.parametrize("method", ["crc32c", "crc64"])
@pytest.mark.parametrize("direction", DIRS)
def test_non_temporal_path(gpu, oracle_mod, direction, method):
    """A list of 512 MiB and more takes the non-temporal loads: the copied
    bytes compared on the device, the values against the oracle."""
    import torch
    M = 1 << 20
    lens = [100 * M + 3, 64 * M, 1, 150 * M + 17, 0, 120 * M, 78 * M + 5]
    first = [0, 2, 5, 7]
    total = sum(lens)
    assert total >= 512 * M
    data = torch.empty(total + 1024, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(data, 0x17E5)
    other = torch.full((total + 1024,), SENT, dtype=torch.uint8, device="cuda")
    # segments back to back from byte 5 of their tensor, objects back to back from byte 9 of theirs
    seg_at = 5 + np.concatenate([[0], np.cumsum(lens)[:-1]])
    N = [sum(lens[first[j]:first[j + 1]]) for j in range(3)]
    obj_at = (9 + np.concatenate([[0], np.cumsum(N)[:-1]])).tolist()
    seg_t, obj_t = (data, other) if direction == "gather" else (other, data)
    views = [seg_t[int(o):int(o) + n] for o, n in zip(seg_at, lens)]
    if direction == "gather":
        out = gpu.gather_segments(method, views, obj_t, obj_at, first)
    else:
        out = gpu.scatter_segments(method, obj_t, obj_at, views, first)
    # both sides hold the same bytes at a constant shift of 4
    assert torch.equal(other[(5 if direction == "scatter" else 9):][:total], data[(9 if direction == "scatter" else 5):][:total])
    lo = 5 if direction == "scatter" else 9
    assert bool((other[:lo] == SENT).all()) and bool((other[lo + total:] == SENT).all())
    hd = data.cpu().numpy()
    at = 5 if direction == "gather" else 9
    want = []
    for n in N:
        want.append(oracle_mod.crc(method, hd[at:at + n]))
        at += n
    assert gpu.as_unsigned(out).tolist() == want


# 8 ---------------------------------------------------- cross-call consistency --
@pytest.mark.parametrize("method", METHODS)
def test_gather_equals_checksum_and_scatter_gather_round_trips(gpu, buf, host, method):
    import torch
    rng = np.random.default_rng(88)
    lens, first = _objects(rng, 40)
    _, _, read_at, write_at, wsize = _layout(gpu, rng, "gather", buf, host, lens, first)
    views = [buf[int(o):int(o) + n] for o, n in zip(read_at, lens)]
    batch = gpu.SegmentBatch(views, first)
    flat = torch.full((wsize,), SENT, dtype=torch.uint8, device="cuda")
    a = gpu.as_unsigned(batch.checksum(method)).tolist()
    b = gpu.as_unsigned(batch.gather(method, flat, write_at.tolist())).tolist()
    assert a == b
    # spread the gathered objects over fresh segments, gather those again
    seg_at, ssize = _place(rng, lens)
    segmem = torch.full((ssize,), SENT, dtype=torch.uint8, device="cuda")
    views2 = [segmem[int(o):int(o) + n] for o, n in zip(seg_at, lens)]
    batch2 = gpu.SegmentBatch(views2, first)
    c = gpu.as_unsigned(batch2.scatter(method, flat, write_at.tolist())).tolist()
    flat2 = torch.full((wsize,), SENT, dtype=torch.uint8, device="cuda")
    d = gpu.as_unsigned(batch2.gather(method, flat2, write_at.tolist())).tolist()
    assert c == a and d == a
    assert torch.equal(flat, flat2)
    for v, v2 in zip(views, views2):
        assert torch.equal(v, v2)
