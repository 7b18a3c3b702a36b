"""GPU tests of the streaming and verifying segment calls through the Python
wrappers: SegmentBatch.update / .update_gather / .update_scatter / .verify and
state_verify, against the oracle.

The list: 5 objects over about 12 segments, every segment at an odd address --
an object with no segments, one whose segments are all empty, a head segment
shorter than the register, an object of 256 KiB + 17 bytes in one segment (two
chunks) and one of three chunks split unevenly over two segments -- plus a
segment outside every object.  Three stages with different segmentations."""
import ctypes
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ["crc32c", "crc64", "crc64-ecma182"]
K = 256 << 10
NOBJ = 5
# per stage: each object's segment lengths; then one segment outside every object
STAGES = [
    [[], [0, 0], [3, 1001, 4097], [K + 17], [100000, 2 * K + 5000 - 100000]],
    [[7], [], [0, 5, 0, 70000], [1, K], [K + 1, 9]],
    [[K + 17, 0], [4], [8], [], [3, 300001]],
]
OUTSIDE = 501
SENT, GUARD = 0xA5, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QLIB = os.path.join(ROOT, "build", "libmchecksum_qfault.so")


class Stage:
    """One stage's tables: lens, odd offsets into the pool, first."""

    def __init__(self, per_obj, base):
        self.lens, self.first = [], [0]
        for segs in per_obj:
            self.lens += segs
            self.first.append(len(self.lens))
        self.lens.append(OUTSIDE)
        self.at, at = [], base | 1
        for n in self.lens:
            self.at.append(at)
            at = (at + n + 2) | 1
        self.end = at

    def obj_bytes(self, host, j):
        parts = [host[self.at[s]:self.at[s] + self.lens[s]] for s in range(self.first[j], self.first[j + 1])]
        return np.concatenate(parts + [np.zeros(0, dtype=np.uint8)])

    def batch(self, gpu, dev):
        return gpu.SegmentBatch([dev[a:a + n] for a, n in zip(self.at, self.lens)], self.first)


@pytest.fixture(scope="module")
def pool(gpu):
    import torch
    stages, base = [], 0
    for per_obj in STAGES:
        stages.append(Stage(per_obj, base))
        base = stages[-1].end
    dev = torch.empty(base + 64, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(dev, 0x57A6E)
    for m in METHODS:
        gpu.prepare(m)
    torch.cuda.synchronize()
    return stages, dev, dev.cpu().numpy()


@pytest.fixture(scope="module")
def want(pool, oracle_mod):
    """Per method: the oracle's CRC of every object after 1, 2 and 3 stages,
    and of each stage's bytes alone.  Computed once."""
    stages, _, host = pool
    res = {}
    for m in METHODS:
        run, alone = [], []
        for k in range(len(stages)):
            run.append([oracle_mod.crc(m, np.ascontiguousarray(np.concatenate(
                [st.obj_bytes(host, j) for st in stages[:k + 1]]))) for j in range(NOBJ)])
            alone.append([oracle_mod.crc(m, np.ascontiguousarray(stages[k].obj_bytes(host, j))) for j in range(NOBJ)])
        res[m] = (run, alone)
    return res


@pytest.fixture(autouse=True)
def _error_word_stays_zero(request, gpu):
    """No call of the product library in this file reports on the error word."""
    import torch
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    gpu.set_error_word(word)
    yield
    torch.cuda.synchronize()
    gpu.set_error_word(None)
    assert int(word.item()) == 0


def _vals(gpu, method, state):
    return gpu.as_unsigned(gpu.state_get(method, state)).tolist()


def _signed(gpu, method, vals):
    import torch
    dt = np.uint32 if gpu.out_dtype(method) == torch.int32 else np.uint64
    return torch.from_numpy(np.asarray(vals, dtype=dt).view(np.int32 if dt == np.uint32 else np.int64)).cuda()


# ------------------------------------------------------------------ updates --
@pytest.mark.parametrize("method", METHODS)
def test_three_stages_equal_the_oracle_over_the_concatenation(gpu, pool, want, method):
    stages, dev, _ = pool
    state = gpu.state_init(method, NOBJ)
    for k, st in enumerate(stages):
        before = state.clone()
        st.batch(gpu, dev).update(method, state)
        assert _vals(gpu, method, state) == want[method][0][k], f"after stage {k}"
        # an object without bytes in this stage keeps its state, bit for bit
        for j in range(NOBJ):
            if sum(st.lens[st.first[j]:st.first[j + 1]]) == 0:
                assert int(state[j]) == int(before[j])


@pytest.mark.parametrize("method", METHODS)
def test_an_offsets_stage_between_two_segments_stages(gpu, pool, want, method):
    """States do not remember which family advanced them: the middle stage's
    bytes, laid out contiguously, go through update_offsets."""
    import torch
    stages, dev, host = pool
    mid = [stages[1].obj_bytes(host, j) for j in range(NOBJ)]
    off = np.concatenate([[0], np.cumsum([len(b) for b in mid])]).astype(np.int64)
    data = torch.cat([torch.from_numpy(np.concatenate(mid)).cuda(), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    state = gpu.state_init(method, NOBJ)
    stages[0].batch(gpu, dev).update(method, state)
    gpu.update_offsets(method, data, torch.from_numpy(off).cuda(), state)
    stages[2].batch(gpu, dev).update(method, state)
    assert _vals(gpu, method, state) == want[method][0][2]


def _flat_layout(st):
    """Object ranges of the contiguous side: GUARD bytes around each."""
    P = np.concatenate([[0], np.cumsum(st.lens)])
    N = [int(P[st.first[j + 1]] - P[st.first[j]]) for j in range(NOBJ)]
    starts, at = [], GUARD + 1
    for n in N:
        starts.append(at)
        at += n + GUARD + 1
    return N, starts, at + GUARD


@pytest.mark.parametrize("method", METHODS)
def test_update_gather(gpu, pool, want, method):
    """The destination equals the one-shot call's and the expected bytes, the
    guards around every range are untouched, the states equal update's."""
    import torch
    stages, dev, host = pool
    st = stages[0]
    N, starts, size = _flat_layout(st)
    exp = np.full(size, SENT, dtype=np.uint8)
    for j in range(NOBJ):
        exp[starts[j]:starts[j] + N[j]] = st.obj_bytes(host, j)
    b = st.batch(gpu, dev)
    one, two = (torch.full((size,), SENT, dtype=torch.uint8, device="cuda") for _ in range(2))
    out = b.gather(method, one, starts)
    assert gpu.as_unsigned(out).tolist() == want[method][1][0]
    # from states a stage in, so that the seed term is not the trivial one
    ref = gpu.state_init(method, NOBJ)
    stages[1].batch(gpu, dev).update(method, ref)
    state = ref.clone()
    b.update(method, ref)
    b.update_gather(method, two, starts, state)
    assert np.array_equal(one.cpu().numpy(), exp)
    assert np.array_equal(two.cpu().numpy(), exp), "bytes or guards differ from the one-shot gather's"
    assert torch.equal(state, ref), "update_gather's states differ from update's"
    assert np.array_equal(dev.cpu().numpy(), host), "segment memory was written"


@pytest.mark.parametrize("method", METHODS)
def test_update_scatter(gpu, pool, want, method):
    import torch
    stages, dev, host = pool
    st = stages[0]
    N, starts, size = _flat_layout(st)
    # the contiguous source: the objects' bytes at their starts
    src_h = np.full(size + 64, 0x3C, dtype=np.uint8)
    for j in range(NOBJ):
        src_h[starts[j]:starts[j] + N[j]] = st.obj_bytes(host, j)
    src = torch.from_numpy(src_h).cuda()
    # the written side: the stage's own segment placement, in sentinel-filled tensors
    wsize = st.end + GUARD
    exp = np.full(wsize, SENT, dtype=np.uint8)
    for s in range(st.first[-1]):  # (the segment outside every object is not written)
        exp[st.at[s]:st.at[s] + st.lens[s]] = host[st.at[s]:st.at[s] + st.lens[s]]
    one, two = (torch.full((wsize,), SENT, dtype=torch.uint8, device="cuda") for _ in range(2))
    b1 = gpu.SegmentBatch([one[a:a + n] for a, n in zip(st.at, st.lens)], st.first)
    b2 = gpu.SegmentBatch([two[a:a + n] for a, n in zip(st.at, st.lens)], st.first)
    out = b1.scatter(method, src, starts)
    assert gpu.as_unsigned(out).tolist() == want[method][1][0]
    ref = gpu.state_init(method, NOBJ)
    stages[1].batch(gpu, dev).update(method, ref)
    state = ref.clone()
    st.batch(gpu, dev).update(method, ref)
    b2.update_scatter(method, src, starts, state)
    assert np.array_equal(one.cpu().numpy(), exp)
    assert np.array_equal(two.cpu().numpy(), exp), "bytes or guards differ from the one-shot scatter's"
    assert torch.equal(state, ref), "update_scatter's states differ from update's"
    assert np.array_equal(src.cpu().numpy(), src_h), "the source was written"


# ------------------------------------------------------------- graph replay --
@pytest.mark.parametrize("method", METHODS)
def test_captured_update_advances_on_every_replay_with_that_replays_lengths(gpu, pool, oracle_mod, method):
    import torch
    stages, dev, host = pool
    st = stages[0]
    b = st.batch(gpu, dev)
    state = gpu.state_init(method, NOBJ)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        b.update(method, state)
    full = np.asarray(st.lens, dtype=np.int64)
    short = full.copy()
    short[st.first[2]] = 0              # the short head segment goes: the next one heads the object
    short[st.first[3]] = K - 1          # two chunks become one
    short[st.first[4] + 1] = K - 5      # the tail segment: one chunk instead of two
    seq = [full, full, short, full]
    parts = [[] for _ in range(NOBJ)]
    for r, lens in enumerate(seq):
        b.set_lengths(lens, stream=s)
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        for j in range(NOBJ):
            for i in range(st.first[j], st.first[j + 1]):
                parts[j].append(host[st.at[i]:st.at[i] + int(lens[i])])
        wantv = [oracle_mod.crc(method, np.ascontiguousarray(np.concatenate(p + [np.zeros(0, dtype=np.uint8)])))
                 for p in parts]
        assert _vals(gpu, method, state) == wantv, f"replay {r}"


# ---------------------------------------------------------- verify_segments --
@pytest.mark.parametrize("method", METHODS)
def test_verify_segments(gpu, pool, want, method):
    import torch
    stages, dev, _ = pool
    st = stages[0]
    good = want[method][1][0]
    exp = _signed(gpu, method, good)
    b = st.batch(gpu, dev)
    # all good; the counter is added to, not set
    mism = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    status = torch.full((NOBJ,), 7, dtype=torch.uint8, device="cuda")
    b.verify(method, exp, status=status, mismatches=mism)
    assert status.tolist() == [0] * NOBJ and int(mism.item()) == 5
    # one bit flipped in the second chunk of the two-chunk object (3), and
    # object 1's expected value corrupted (its segments are all empty)
    data = dev.clone()
    data[st.at[st.first[3]] + K + 9] ^= 0x10
    bad_exp = list(good)
    bad_exp[1] ^= 1 << 5
    exp2 = _signed(gpu, method, bad_exp)
    b2 = st.batch(gpu, data)
    status, mism = b2.verify(method, exp2, mismatches=mism)
    assert status.tolist() == [0, 1, 0, 1, 0] and int(mism.item()) == 7
    # either output left out
    status, none = b2.verify(method, exp2, mismatches=False)
    assert none is False and status.tolist() == [0, 1, 0, 1, 0]
    none, mism = b2.verify(method, exp2, status=False)
    assert none is False and int(mism.item()) == 2
    b2.verify(method, exp2, status=False, mismatches=False)
    torch.cuda.synchronize()
    assert torch.equal(data[:st.at[st.first[3]] + K + 9], dev[:st.at[st.first[3]] + K + 9]), "segment memory was written"


def test_verify_segments_searches_the_scan_table_without_a_map(gpu, pool, want, monkeypatch):
    """CRC-64 with no chunk map left to the call (MCHECKSUM_GPU_SEG_MAP_CAP=0):
    the path a list with more chunks than the call's part of the map takes."""
    stages, dev, _ = pool
    monkeypatch.setenv("MCHECKSUM_GPU_SEG_MAP_CAP", "0")
    good = list(want["crc64"][1][2])
    good[4] ^= 1
    status, mism = stages[2].batch(gpu, dev).verify("crc64", _signed(gpu, "crc64", good))
    assert status.tolist() == [0, 0, 0, 0, 1] and int(mism.item()) == 1


# ------------------------------------------------------------- state_verify --
@pytest.mark.parametrize("method", METHODS)
def test_state_verify(gpu, pool, want, method):
    import torch
    stages, dev, _ = pool
    state = gpu.state_init(method, NOBJ)
    for st in stages:
        st.batch(gpu, dev).update(method, state)
    before = state.clone()
    vals = _vals(gpu, method, state)
    assert vals == want[method][0][2]
    expv = list(vals)
    expv[0] ^= 1
    expv[3] ^= 1 << 31
    exp = _signed(gpu, method, expv)
    status, mism = gpu.state_verify(method, state, exp)
    assert status.tolist() == [int(a != b) for a, b in zip(vals, expv)] == [1, 0, 0, 1, 0]
    assert int(mism.item()) == 2
    # adds to the counter; either output may be left out
    status2, mism = gpu.state_verify(method, state, _signed(gpu, method, vals), mismatches=mism)
    assert status2.tolist() == [0] * NOBJ and int(mism.item()) == 2
    assert gpu.state_verify(method, state, exp, status=False)[1].item() == 2
    assert gpu.state_verify(method, state, exp, mismatches=False)[0].tolist() == [1, 0, 0, 1, 0]
    # inside a captured graph
    status = torch.zeros(NOBJ, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        gpu.state_verify(method, state, exp, status=status, mismatches=mism)
    for r in range(2):
        with torch.cuda.stream(s):
            g.replay()
        s.synchronize()
        assert status.tolist() == [1, 0, 0, 1, 0] and int(mism.item()) == 2 * (r + 1)
    assert torch.equal(state, before), "state_verify modified the states"


# ----------------------------------------------- the non-temporal threshold --
# A list of kSegNtBytes = 512 MiB and more takes the non-temporal loads in
# seg_pass (decided on the device from the scan's total): 640 segments of 1 MiB,
# views that reuse the small pool at 16-B aligned offsets, 4 per object, three
# of them ragged (an odd start, a length that is no multiple of 1 KiB, a short
# one).  The oracle hashes a fixed sample of the 160 objects -- the first, the
# last and the three that hold a ragged segment; all 160 are compared with the
# same segments run as two lists of 320 MiB, which take the default loads.
MIB = 1 << 20
NT_NOBJ = 160
NT_SAMPLE = (0, 1, 80, 159, 17)


@pytest.fixture(scope="module")
def nt_list(pool):
    """(segments as (offset, length), first, per object a small segment of an earlier stage)."""
    _, dev, _ = pool
    assert dev.data_ptr() % 16 == 0
    rng = np.random.default_rng(93)
    segs = [(16 * int(rng.integers(0, (dev.numel() - 64 - MIB) // 16)), MIB) for _ in range(4 * NT_NOBJ)]
    segs[5] = (segs[5][0] + 3, MIB - 7)
    segs[322] = (segs[322][0] + 1, MIB - 1029)
    segs[639] = (segs[639][0] + 7, 5)
    assert sum(n for _, n in segs) >= 512 * MIB
    first = list(range(0, 4 * NT_NOBJ + 1, 4))
    small = [(1 + 37 * j, 3 + 11 * j) for j in range(NT_NOBJ)]  # 3 .. 1752 bytes at odd and even addresses
    return segs, first, small


def _views(dev, segs):
    return [dev[o:o + n] for o, n in segs]


def _in_two_lists(gpu, method, dev, segs, state):
    """Advance `state` over the objects of the 640-segment list as two calls
    of 320 MiB each: objects 0..79, then 80..159, the others without segments."""
    half = 2 * NT_NOBJ
    quarter = list(range(0, half + 1, 4))
    gpu.SegmentBatch(_views(dev, segs[:half]), quarter + [half] * (NT_NOBJ // 2)).update(method, state)
    gpu.SegmentBatch(_views(dev, segs[half:]), [0] * (NT_NOBJ // 2) + quarter).update(method, state)
    return state


def _sample_bytes(host, segs, first, j):
    return [host[o:o + n] for o, n in segs[first[j]:first[j + 1]]]


@pytest.mark.parametrize("method", METHODS)
def test_update_segments_at_the_non_temporal_threshold(gpu, pool, nt_list, oracle_mod, method):
    """The states come from a small stage, so the chunk pass's XORs land on
    seeded states (seg_pre_kernel<T, true>)."""
    import torch
    _, dev, host = pool
    segs, first, small = nt_list
    state = gpu.state_init(method, NT_NOBJ)
    gpu.SegmentBatch(_views(dev, small), list(range(NT_NOBJ + 1))).update(method, state)
    ref = _in_two_lists(gpu, method, dev, segs, state.clone())
    gpu.SegmentBatch(_views(dev, segs), first).update(method, state)
    got = _vals(gpu, method, state)
    for j in NT_SAMPLE:
        parts = [host[small[j][0]:small[j][0] + small[j][1]]] + _sample_bytes(host, segs, first, j)
        assert got[j] == oracle_mod.crc(method, np.concatenate(parts)), j
    assert torch.equal(state, ref), "the states differ from the same objects' in two lists under the threshold"


@pytest.mark.parametrize("method", METHODS)
def test_verify_segments_at_the_non_temporal_threshold(gpu, pool, nt_list, oracle_mod, method):
    import torch
    _, dev, host = pool
    segs, first, _ = nt_list
    good = _vals(gpu, method, _in_two_lists(gpu, method, dev, segs, gpu.state_init(method, NT_NOBJ)))
    for j in NT_SAMPLE:
        assert good[j] == oracle_mod.crc(method, np.concatenate(_sample_bytes(host, segs, first, j))), j
    planted = list(good)
    planted[17] ^= 1        # one of the sample, so a value the oracle gave
    planted[101] ^= 1 << 31
    b = gpu.SegmentBatch(_views(dev, segs), first)
    mism = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    status, mism = b.verify(method, _signed(gpu, method, planted), mismatches=mism)
    assert np.nonzero(status.cpu().numpy())[0].tolist() == [17, 101] and int(mism.item()) == 7
    status, mism = b.verify(method, _signed(gpu, method, good))
    assert int(status.sum().item()) == 0 and int(mism.item()) == 0


# -------------------------------------------------------------- fail closed --
# tests/test_gpu_fail_closed.py's bound: a call whose waits are never satisfied
# returns within about one deadline (1 s)
STALL_MAX_S = 1.5


@pytest.fixture(scope="module")
def qlib(gpu):
    assert os.path.exists(QLIB), "build/libmchecksum_qfault.so missing: run make"
    L = ctypes.CDLL(QLIB)
    c = ctypes
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    seg = [c.c_char_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t]
    L.mchecksum_gpu_update_segments.argtypes = seg + [c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_verify_segments.argtypes = seg + [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_segments_work_size.argtypes = [c.c_size_t]
    L.mchecksum_gpu_segments_work_size.restype = c.c_size_t
    L.mchecksum_gpu_set_error_word.argtypes = [c.c_void_p]
    L.mchecksum_gpu_queue_faults.restype = c.c_longlong
    L.mchecksum_gpu_reload_settings.restype = None
    return L


def _small_list_in_three_scan_blocks(gpu, pool):
    """The small list, followed by empty segments outside every object up to a
    third scan block (1024 segments each): the injected scan faults need a
    block behind block 1."""
    import torch
    stages, dev, _ = pool
    st = stages[0]
    segs = [dev[a:a + n] for a, n in zip(st.at, st.lens)] + [dev[0:0]] * (2060 - len(st.lens))
    b = gpu.SegmentBatch(segs, st.first)
    torch.cuda.synchronize()
    return b


def _qenv(monkeypatch, qlib, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    qlib.mchecksum_gpu_reload_settings()


def test_verify_segments_fails_closed_when_the_scan_stalls(gpu, qlib, pool, want, monkeypatch):
    """scanstall: scan block 1 never publishes, block 2 waits out its deadline.
    Every expected value is right and every status starts 0, so only the
    fail-closed sweep can have flagged them."""
    import torch
    b = _small_list_in_three_scan_blocks(gpu, pool)
    exp = _signed(gpu, "crc64", want["crc64"][1][0])
    status = torch.zeros(NOBJ, dtype=torch.uint8, device="cuda")
    mism = torch.full((1,), 3, dtype=torch.int32, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    n, base = b.nseg, b.meta.data_ptr()
    work = torch.zeros((qlib.mchecksum_gpu_segments_work_size(n) + 7) // 8, dtype=torch.int64, device="cuda")
    assert qlib.mchecksum_gpu_prepare(b"crc64") == 0
    _qenv(monkeypatch, qlib, MCHECKSUM_GPU_QFAULT_SCAN="1", MCHECKSUM_GPU_QFAULT_MODE="scanstall")
    qlib.mchecksum_gpu_set_error_word(word.data_ptr())
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = qlib.mchecksum_gpu_verify_segments(b"crc64", base, base + 8 * n, n, base + 16 * n, NOBJ, work.data_ptr(),
                                                work.numel() * 8, exp.data_ptr(), status.data_ptr(), mism.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        qlib.mchecksum_gpu_set_error_word(None)
        monkeypatch.undo()
        qlib.mchecksum_gpu_reload_settings()
    print(f"stalled verify_segments returned after {dt:.3f} s")
    assert rc == 0
    assert dt <= STALL_MAX_S, f"the call took {dt:.3f} s"
    assert int(word.item()) == 1, "one failed call, one increment"
    assert int(mism.item()) == 3 + NOBJ
    assert status.tolist() == [1] * NOBJ


def test_update_segments_reports_a_scan_that_gave_up(gpu, qlib, pool, monkeypatch):
    """The give-up mode: scan block 1 gives up its look-back at once.  The
    call reports once on the error word and the fault counter, and leaves the
    states as they were."""
    import torch
    b = _small_list_in_three_scan_blocks(gpu, pool)
    state = gpu.state_init("crc64", NOBJ)
    before = state.clone()
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    n, base = b.nseg, b.meta.data_ptr()
    work = torch.zeros((qlib.mchecksum_gpu_segments_work_size(n) + 7) // 8, dtype=torch.int64, device="cuda")
    assert qlib.mchecksum_gpu_prepare(b"crc64") == 0
    faults0 = qlib.mchecksum_gpu_queue_faults()
    _qenv(monkeypatch, qlib, MCHECKSUM_GPU_QFAULT_SCAN="1")
    qlib.mchecksum_gpu_set_error_word(word.data_ptr())
    try:
        rc = qlib.mchecksum_gpu_update_segments(b"crc64", base, base + 8 * n, n, base + 16 * n, NOBJ, work.data_ptr(),
                                                work.numel() * 8, state.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        qlib.mchecksum_gpu_set_error_word(None)
        monkeypatch.undo()
        qlib.mchecksum_gpu_reload_settings()
    assert rc == 0
    assert int(word.item()) == 1
    assert qlib.mchecksum_gpu_queue_faults() - faults0 == 1
    assert torch.equal(state, before), "a call whose scan gave up must leave the states alone"


def test_verify_segments_fails_closed_when_the_chunk_pass_drops_a_chunk(gpu, qlib):
    """The work queue's give-up (tests/test_gpu_fail_closed.py's
    test_segment_chunk_queue_fault shape: 2048 aligned chunks, workgroup 3
    drops one): the chunk pass leaves its claim in the workspace and the
    compare, reading it, flags every object although every expected value is
    right -- the dropped chunk's object must not read as verified, and the
    compare cannot tell which one it is."""
    import torch
    nobj, nseg_per, seg = 128, 4, 1 << 20
    data = torch.empty(nobj * nseg_per * seg + 64, dtype=torch.uint8, device="cuda")
    gpu.fill_splitmix(data, 0x5E70)
    b = gpu.SegmentBatch([data[i * seg:(i + 1) * seg] for i in range(nobj * nseg_per)],
                         np.arange(0, nobj * nseg_per + 1, nseg_per))
    exp = b.checksum("crc64").clone()
    status, mism = b.verify("crc64", exp)  # the product library: clean
    assert int(status.sum().item()) == 0 and int(mism.item()) == 0
    status = torch.zeros(nobj, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    n, base = b.nseg, b.meta.data_ptr()
    work = torch.zeros((qlib.mchecksum_gpu_segments_work_size(n) + 7) // 8, dtype=torch.int64, device="cuda")
    assert qlib.mchecksum_gpu_prepare(b"crc64") == 0
    faults0 = qlib.mchecksum_gpu_queue_faults()
    torch.cuda.synchronize()
    qlib.mchecksum_gpu_set_error_word(word.data_ptr())
    try:
        rc = qlib.mchecksum_gpu_verify_segments(b"crc64", base, base + 8 * n, n, base + 16 * n, nobj, work.data_ptr(),
                                                work.numel() * 8, exp.data_ptr(), status.data_ptr(), mism.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        qlib.mchecksum_gpu_set_error_word(None)
    assert rc == 0
    assert int(word.item()) == 1
    assert qlib.mchecksum_gpu_queue_faults() - faults0 == 1
    assert int(mism.item()) == nobj
    assert int(status.sum().item()) == nobj
