"""Streaming batch checksums on the GPU (include/mchecksum_gpu.h:
mchecksum_gpu_state_init / update_offsets / state_get / combine): the value
after any number of updates is the CRC of the bytes so far, for every kernel
variant a plan can pick (light, full with a queue slot, non-temporal, the
static split of a graph replay).  The reference is the oracle's CRC of the
concatenated bytes (or checksum_offsets for a single update); the CPU half of
the algebra is tests/test_seed_update.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ("crc32c", "crc64", "crc64-ecma182", "crc32")
EMETHOD, EINVAL = -3, -1


class _Streams:
    """`count` streams fed over `ncalls` calls: stream i's bytes are
    whole[start[i] : start[i] + total[i]], cut so that call k carries
    lens[k][i] of them.  Call k's device buffer packs its chunks back to back
    from a base offset that differs per call, so chunks start at every
    alignment."""

    def __init__(self, O, lens, seed):
        self.lens = [np.asarray(l, dtype=np.int64) for l in lens]
        self.count = len(self.lens[0])
        self.total = np.sum(self.lens, axis=0)
        self.start = np.concatenate([[0], np.cumsum(self.total)]).astype(np.int64)
        self.whole = O.splitmix_bytes(int(self.start[-1]) + 1, seed)
        self.done = np.zeros(self.count, dtype=np.int64)  # bytes of every stream fed so far

    def call(self, k):
        """(host buffer, offsets table) of call k; marks its chunks as fed."""
        base = (5 + 7 * k) % 16
        offs = base + np.concatenate([[0], np.cumsum(self.lens[k])])
        lo = self.start[:-1] + self.done
        parts = [self.whole[a:a + n] for a, n in zip(lo, self.lens[k])]
        buf = np.concatenate([np.zeros(base, dtype=np.uint8)] + parts + [np.zeros(64, dtype=np.uint8)])
        self.done = self.done + self.lens[k]
        return buf, offs.astype(np.int64)

    def want(self, O, method):
        """The oracle's CRC of every stream's bytes so far."""
        return np.asarray([O.crc(method, self.whole[a:a + n]) for a, n in zip(self.start[:-1], self.done)],
                          dtype=np.uint64)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _got(G, method, state):
    return G.as_unsigned(G.state_get(method, state)).astype(np.uint64)


def _feed(G, O, torch, method, st, check_each=True):
    """Run every call of `st` through update_offsets; after each, state_get
    must be the oracle's CRC of the bytes so far (which also pins that
    state_get leaves the state intact)."""
    state = G.state_init(method, st.count)
    assert np.array_equal(_got(G, method, state), np.full(st.count, O.crc(method, b""), dtype=np.uint64))
    for k in range(len(st.lens)):
        buf, offs = st.call(k)
        G.update_offsets(method, _dev(torch, buf), _dev(torch, offs), state, offsets_host=offs)
        if check_each or k + 1 == len(st.lens):
            got, want = _got(G, method, state), st.want(O, method)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (method, "call", k, "streams", bad[:8], st.lens[k][bad[:8]])
    return state


def _one_shot_lens():
    lens = (np.arange(300) * 2 + (np.arange(300) % 3 == 0)).astype(np.int64)  # 1, 2, 4, 7, ..., 598; 0 below
    lens[5] = 0
    lens[[17, 99, 150, 201, 250, 299]] = [4095, 4096, 4097, 65535, 65536, 65537]
    return lens


@pytest.mark.parametrize("method", METHODS)
def test_one_update_equals_one_shot(gpu, oracle_mod, method):
    """state_init, one update_offsets, state_get == checksum_offsets on the
    same batch: 300 payloads of 0..599 bytes at every start alignment mod 16,
    and lengths around 4096 and 65536."""
    import torch
    G, O = gpu, oracle_mod
    lens = _one_shot_lens()
    offs = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert set((offs[:-1][lens > 0] % 16).tolist()) == set(range(16))
    data = _dev(torch, O.splitmix_bytes(int(offs[-1]) + 64, 0x51))
    offs_d = _dev(torch, offs)
    want = G.as_unsigned(G.checksum_offsets(method, data, offs_d, offsets_host=offs)).astype(np.uint64)
    state = G.state_init(method, 300)
    G.update_offsets(method, data, offs_d, state)
    assert np.array_equal(_got(G, method, state), want)
    # ... and the values are the oracle's
    host = data.cpu().numpy()
    for i in (0, 1, 17, 150, 299):
        assert int(want[i]) == O.crc(method, host[offs[i]:offs[i + 1]])


def _cuts(rng, count, ncalls, small):
    """A different random cut per stream per call: empty chunks, chunks
    shorter than the register, chunks ending 1 byte before or after a multiple
    of 16 or 128."""
    pool = np.asarray([0, 0, 1, 2, 3, 5, 7, 15, 17, 127, 129, 255, 257, 1023, 1025])
    lens = []
    for _ in range(ncalls):
        l = rng.integers(0, 200 if small else 700, count)
        pick = rng.random(count) < 0.4
        l[pick] = rng.choice(pool[pool < 200] if small else pool, int(pick.sum()))
        lens.append(l)
    return lens


@pytest.mark.parametrize("method", METHODS)
def test_chunked_equals_oracle_of_concatenation(gpu, oracle_mod, method):
    """257 streams over 3 calls, each call cutting every stream elsewhere."""
    import torch
    rng = np.random.default_rng(257)
    st = _Streams(oracle_mod, _cuts(rng, 257, 3, False), 0x257)
    for l in st.lens:
        assert np.any(l == 0) and np.any((l > 0) & (l < 4)) and np.any(l % 16 == 15) and np.any(l % 128 == 1)
    _feed(gpu, oracle_mod, torch, method, st)


@pytest.mark.parametrize("count", [1, 1024, 1025, 8192])
@pytest.mark.parametrize("method", METHODS)
def test_every_kernel_variant(gpu, oracle_mod, method, count):
    """The same check where the offsets plan changes kernels: 1 and 1024 (the
    light CRC-32C layout and its boundary), 1025 (the full layout, with a
    work-queue slot), 8192 payloads under 200 bytes (the non-temporal kernels,
    under 2 MiB moved).  Whatever the plan picks, the values must hold; only
    the slot of the 1025 case is asserted."""
    import torch
    G, O = gpu, oracle_mod
    rng = np.random.default_rng(count)
    st = _Streams(O, _cuts(rng, count, 3, count == 8192), 0xC0 + count)
    before = G.queue_stats()
    _feed(G, O, torch, method, st, check_each=count < 8192)
    if count == 1025:
        torch.cuda.synchronize()
        assert G.queue_stats()["slot"] - before["slot"] >= 1, "the 1025-payload update took no work-queue slot"


@pytest.mark.parametrize("count", [300, 1100])
@pytest.mark.parametrize("method", ["crc32c", "crc64"])
def test_zero_length_chunk_is_a_no_op(gpu, oracle_mod, method, count):
    """In the middle of a batch and as the whole batch, an empty chunk leaves
    its state word as it was."""
    import torch
    G, O = gpu, oracle_mod
    rng = np.random.default_rng(4)
    first = rng.integers(1, 300, count)
    second = rng.integers(1, 300, count)
    empty = rng.random(count) < 0.3
    empty[[0, count // 2, count - 1]] = True
    second[empty] = 0
    st = _Streams(O, [first, second, np.zeros(count, dtype=np.int64)], 0x2E80)
    state = G.state_init(method, count)
    buf, offs = st.call(0)
    G.update_offsets(method, _dev(torch, buf), _dev(torch, offs), state)
    raw0 = state.clone()
    buf, offs = st.call(1)
    G.update_offsets(method, _dev(torch, buf), _dev(torch, offs), state)
    same = (state == raw0).cpu().numpy()
    assert np.all(same[empty]), "an empty chunk changed its state"
    assert not np.any(same[~empty]), "a non-empty chunk left its state unchanged"
    assert np.array_equal(_got(G, method, state), st.want(O, method))
    raw1 = state.clone()
    buf, offs = st.call(2)  # every chunk empty
    G.update_offsets(method, _dev(torch, buf), _dev(torch, offs), state)
    assert bool((state == raw1).all())
    assert np.array_equal(_got(G, method, state), st.want(O, method))


@pytest.mark.parametrize("count", [64, 2000])
@pytest.mark.parametrize("method", METHODS)
def test_graph_replay_advances_the_state(gpu, oracle_mod, method, count):
    """prepare, one update_offsets captured on a side stream, three replays
    with the data buffer refilled in between: the state is the oracle's CRC of
    the three fills concatenated (count 64: the light kernel; 2000: the full
    kernel's static split, a capture gets no queue slot).  A linear graph, one
    replay at a time."""
    import torch
    G, O = gpu, oracle_mod
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 400, count)
    lens[[1, count // 3]] = 0
    offs = 9 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nb = int(offs[-1]) + 64
    fills = [O.splitmix_bytes(nb, 0xF111 + r) for r in range(3)]
    G.prepare(method)
    data = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    offs_d = _dev(torch, offs)
    state = G.state_init(method, count)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        G.update_offsets(method, data, offs_d, state)
    torch.cuda.synchronize()
    # the capture itself ran nothing
    assert np.array_equal(_got(G, method, state), np.full(count, O.crc(method, b""), dtype=np.uint64))
    for r in range(3):
        with torch.cuda.stream(s):
            data.copy_(torch.from_numpy(fills[r]))
            g.replay()
        s.synchronize()
        want = np.asarray([O.crc(method, np.concatenate([f[a:b] for f in fills[:r + 1]]))
                           for a, b in zip(offs[:-1], offs[1:])], dtype=np.uint64)
        with torch.cuda.stream(s):
            got = _got(G, method, state)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (method, "replay", r, bad[:8])


@pytest.mark.parametrize("method", METHODS)
def test_combine(gpu, oracle_mod, method):
    """combine(checksum(A), checksum(B), len_b) == CRC(A || B), also with out
    aliasing a; folding 5 chunks left to right gives the object's CRC."""
    import torch
    G, O = gpu, oracle_mod
    rng = np.random.default_rng(6)
    len_b = np.asarray([0, 1, 15, 16, 4096, 65537] * 4, dtype=np.int64)
    len_a = rng.integers(0, 3000, len(len_b))
    len_a[:3] = [0, 1, 70000]
    lens = np.stack([len_a, len_b], axis=1).reshape(-1)
    offs = 1 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    host = O.splitmix_bytes(int(offs[-1]) + 64, 0xAB)
    vals = G.checksum_offsets(method, _dev(torch, host), _dev(torch, offs), offsets_host=offs)
    a, b = vals[0::2].contiguous(), vals[1::2].contiguous()
    want = np.asarray([O.crc(method, host[offs[2 * i]:offs[2 * i + 2]]) for i in range(len(len_b))], dtype=np.uint64)
    lb = _dev(torch, len_b)
    assert np.array_equal(G.as_unsigned(G.combine(method, a, b, lb)).astype(np.uint64), want)
    assert G.combine(method, a, b, lb, out=a) is a
    assert np.array_equal(G.as_unsigned(a).astype(np.uint64), want)
    # 8 objects of 5 chunks each (chunks may be empty), folded left to right
    nobj, clen = 8, rng.integers(0, 5000, (8, 5))
    clen[0] = [0, 0, 7, 0, 1]
    coffs = np.concatenate([[0], np.cumsum(clen.reshape(-1))]).astype(np.int64)
    chost = O.splitmix_bytes(int(coffs[-1]) + 64, 0xCD)
    c = G.checksum_offsets(method, _dev(torch, chost), _dev(torch, coffs)).reshape(nobj, 5)
    acc = c[:, 0].contiguous()
    for k in range(1, 5):
        G.combine(method, acc, c[:, k].contiguous(), _dev(torch, clen[:, k]), out=acc)
    want = np.asarray([O.crc(method, chost[coffs[5 * j]:coffs[5 * j + 5]]) for j in range(nobj)], dtype=np.uint64)
    assert np.array_equal(G.as_unsigned(acc).astype(np.uint64), want)


def test_argument_errors_launch_nothing(gpu):
    """Refusals before any GPU work: the state and outputs stay as they were."""
    import torch
    L = gpu._lib()
    st = torch.full((8,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    data = torch.zeros(256, dtype=torch.uint8, device="cuda")
    offs = _dev(torch, np.asarray([0, 64, 128], dtype=np.int64))
    p = lambda t: t.data_ptr()  # noqa: E731
    # 16-bit methods have no payload kernels
    assert L.mchecksum_gpu_state_init(b"crc16", p(st), 2, None) == EMETHOD
    assert L.mchecksum_gpu_update_offsets(b"crc16", p(data), p(offs), 2, p(st), None) == EMETHOD
    assert L.mchecksum_gpu_state_get(b"crc16", p(st), 2, p(st), None) == EMETHOD
    assert L.mchecksum_gpu_combine(b"crc16", p(st), p(st), p(offs), 2, p(st), None) == EMETHOD
    assert L.mchecksum_gpu_state_init(b"nope", p(st), 2, None) == EMETHOD
    # NULL pointers with count > 0
    assert L.mchecksum_gpu_state_init(b"crc64", None, 2, None) == EINVAL
    assert L.mchecksum_gpu_update_offsets(b"crc64", p(data), p(offs), 2, None, None) == EINVAL
    assert b"NULL" in L.mchecksum_gpu_last_error()
    assert L.mchecksum_gpu_update_offsets(b"crc64", None, p(offs), 2, p(st), None) == EINVAL
    assert L.mchecksum_gpu_state_get(b"crc64", None, 2, p(st), None) == EINVAL
    assert L.mchecksum_gpu_state_get(b"crc64", p(st), 2, None, None) == EINVAL
    assert L.mchecksum_gpu_combine(b"crc64", p(st), p(st), None, 2, p(st), None) == EINVAL
    # more than 2^31 payloads
    big = (1 << 31) + 1
    assert L.mchecksum_gpu_state_init(b"crc64", p(st), big, None) == EINVAL
    assert b"2^31" in L.mchecksum_gpu_last_error()
    assert L.mchecksum_gpu_update_offsets(b"crc64", p(data), p(offs), big, p(st), None) == EINVAL
    assert L.mchecksum_gpu_state_get(b"crc64", p(st), big, p(st), None) == EINVAL
    assert L.mchecksum_gpu_combine(b"crc64", p(st), p(st), p(offs), big, p(st), None) == EINVAL
    # an empty batch needs no buffers
    assert L.mchecksum_gpu_state_init(b"crc32c", None, 0, None) == 0
    assert L.mchecksum_gpu_update_offsets(b"crc32c", None, None, 0, None, None) == 0
    assert L.mchecksum_gpu_state_get(b"crc32c", None, 0, None, None) == 0
    assert L.mchecksum_gpu_combine(b"crc32c", None, None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert bool((st == 0x5A5A5A5A).all())
    # ... and the wrappers check tensors on the host
    with pytest.raises(gpu.GpuChecksumError):
        gpu.update_offsets("crc64", data, offs, torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(gpu.GpuChecksumError):
        gpu.update_offsets("crc64", data, offs, torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(gpu.GpuChecksumError):
        gpu.state_get("crc32c", torch.zeros(2, dtype=torch.int32))
    with pytest.raises(gpu.GpuChecksumError):
        gpu.combine("crc32c", torch.zeros(2, dtype=torch.int32, device="cuda"),
                    torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))


def test_error_word_stays_zero_on_a_healthy_sequence(gpu, oracle_mod):
    import torch
    G, O = gpu, oracle_mod
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    G.set_error_word(word)
    try:
        for method in ("crc32c", "crc64"):
            rng = np.random.default_rng(8)
            st = _Streams(O, _cuts(rng, 1500, 2, False), 0xE0)
            state = _feed(G, O, torch, method, st, check_each=False)
            v = G.state_get(method, state)
            G.combine(method, v, v, _dev(torch, np.zeros(1500, dtype=np.int64)), out=v)
        torch.cuda.synchronize()
        assert int(word.item()) == 0
    finally:
        G.set_error_word(None)
    assert G.queue_faults() == 0
