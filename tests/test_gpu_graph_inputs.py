"""Captured calls replayed after their DEVICE-SIDE inputs changed -- the real
use of capture: a receive buffer, an offsets table or a bulk handle's segment
table refilled with new messages, then the same graph replayed.  The other
graph tests replay the same bytes and tables every time, so a kernel that
keeps state in device memory from one replay to the next could be wrong with
them green.  The segment scan keeps such state (its look-back descriptors,
mchecksum_gpu_ext.hip; tests/test_scan_model.py is the protocol's CPU model):
with unchanged lengths a stale prefix is the right one.

Every comparison is with the oracle on the host copy of that replay's
inputs; every wait is bounded (a wedged replay ends the process instead of
hanging); every graph is linear, on one stream.
"""
import functools
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 256 << 10   # the segment pass's chunk
SCAN_BLK = 1024     # segments per scan block (kScanBlk)
NSEG, POOL, BIG_CAP = 8197, 12 << 20, 600000
BIG = (1023, 2048, 3500, 5119, 8195)  # five scan blocks; 1023 | 1024 and 2047 | 2048 are block boundaries
NSTEP = 8  # lengths of: the eager call, 6 replays (the 6th = the 2nd's), the closing eager call


def _wait(torch, tag, streams=(None,)):
    evs = []
    for st in streams:
        ev = torch.cuda.Event()
        ev.record(st)
        evs.append(ev)
    t0 = time.time()
    while not all(ev.query() for ev in evs):
        if time.time() - t0 > 20:
            print("HUNG", tag, flush=True)
            os._exit(3)
        time.sleep(0.002)


def _boundary_prefixes(lens):
    """Inclusive byte and chunk prefixes at the 8 scan-block boundaries."""
    at = np.arange(SCAN_BLK, NSEG, SCAN_BLK)
    return np.cumsum(lens)[at - 1], np.cumsum((lens + CHUNK - 1) // CHUNK)[at - 1]


class _Scene:
    """The segment layout (fixed) and the lengths of every step (host side)."""

    def __init__(self, O):
        rng = np.random.default_rng(20260)
        self.host = O.splitmix_bytes(POOL, 0x5E65)
        self.cap = np.full(NSEG, 2048, dtype=np.int64)
        self.cap[list(BIG)] = BIG_CAP
        # starts anywhere in the pool (segments may overlap: they are only read), mixed alignment
        self.start = rng.integers(0, POOL - self.cap) // 16 * 16 + rng.choice([0, 0, 0, 1, 5, 8], NSEG)
        self.start = np.minimum(self.start, POOL - self.cap)
        # about 1640 objects of 0..10 segments; a few segments before the first and after the last belong to none
        counts = rng.integers(0, 11, 1640)
        first = 3 + np.concatenate([[0], np.cumsum(counts)])
        self.first = first[first <= NSEG - 2].astype(np.int64)
        self.nobj = len(self.first) - 1
        self.steps = []
        while len(self.steps) < NSTEP:
            if len(self.steps) == 6:  # the 6th replay: the 2nd's lengths again
                self.steps.append(self.steps[2].copy())
                continue
            lens = np.where(rng.random(NSEG) < 0.3, 0, rng.integers(1, 2049, NSEG))
            lens[list(BIG)] = rng.permutation([BIG_CAP, 2 * CHUNK, CHUNK + 1024, int(rng.integers(CHUNK, BIG_CAP)),
                                               int(rng.integers(0, BIG_CAP))])
            # (redrawn until it differs from its neighbours at every block boundary:
            # a stale prefix must never be right by accident -- asserted in the test)
            if all(self._differ(lens, other) for other in self._neighbours(len(self.steps))):
                self.steps.append(lens.astype(np.int64))
        self._want = {}

    def _neighbours(self, n):
        out = [self.steps[n - 1]] if n else []
        if n == 5:
            out.append(self.steps[2])  # step 6 repeats step 2, right after step 5
        return out

    @staticmethod
    def _differ(a, b):
        (pa, ca), (pb, cb) = _boundary_prefixes(a), _boundary_prefixes(b)
        return bool(np.all(pa != pb) and np.all(ca != cb))

    def want(self, O, method, step):
        """The oracle's CRC of every object under that step's lengths (shared
        by the cases of one method)."""
        key = (method, 2 if step == 6 else step)
        if key not in self._want:
            lens, vals = self.steps[step], []
            for j in range(self.nobj):
                parts = [self.host[self.start[s]:self.start[s] + lens[s]] for s in range(self.first[j], self.first[j + 1])]
                vals.append(O.crc(method, np.concatenate(parts) if parts else self.host[:0]))
            self._want[key] = np.asarray(vals, dtype=np.uint64)
        return self._want[key]


@functools.lru_cache(maxsize=1)
def _scene(O):
    return _Scene(O)


def _assert_steps_differ(sc):
    """Between consecutive steps the inclusive byte prefix and the inclusive
    chunk prefix differ at each of the 8 scan-block boundaries."""
    assert len(sc.steps) == NSTEP
    for a, b in zip(sc.steps, sc.steps[1:]):
        assert np.all(a <= sc.cap) and np.all(b <= sc.cap)
        (pa, ca), (pb, cb) = _boundary_prefixes(a), _boundary_prefixes(b)
        assert len(pa) == 8 and np.all(pa != pb) and np.all(ca != cb), "a stale prefix could be right by accident"


def test_scene_is_the_shape_the_scan_can_get_wrong(oracle_mod):
    """Host-side preconditions of the replay test."""
    sc = _scene(oracle_mod)
    assert (NSEG + SCAN_BLK - 1) // SCAN_BLK == 9
    assert {b // SCAN_BLK for b in BIG} == {0, 2, 3, 4, 8} and 1023 in BIG and 2048 in BIG
    assert 1500 <= sc.nobj <= 1640 and sc.first[0] > 0 and sc.first[-1] < NSEG
    n = np.diff(sc.first)
    assert n.min() == 0 and n.max() == 10
    straddle = [k for k in range(SCAN_BLK, NSEG, SCAN_BLK)
                if sc.first[0] < k < sc.first[-1] and k not in set(sc.first.tolist())]
    assert len(straddle) >= 4, "objects must straddle scan-block boundaries"
    assert np.all(sc.start + sc.cap <= POOL) and len(set((sc.start % 16).tolist())) >= 4
    _assert_steps_differ(sc)
    assert np.array_equal(sc.steps[6], sc.steps[2])
    for lens in sc.steps:
        assert 0.25 < np.mean(lens == 0) < 0.35 and np.max((lens + CHUNK - 1) // CHUNK) == 3


@pytest.mark.parametrize("method,map_cap", [("crc32c", None), ("crc64", None), ("crc64", 0), ("crc64-ecma182", None)],
                         ids=["crc32c", "crc64", "crc64-nomap", "crc64-ecma182"])
def test_segments_replay_with_new_lengths(gpu, oracle_mod, monkeypatch, method, map_cap):
    """One captured SegmentBatch.checksum, 6 replays, the device length table
    rewritten (set_lengths) before each: 8197 segments = 9 scan blocks, so
    blocks 1..8 take their offsets from the look-back descriptors the replay
    before left behind under the same captured epoch.  Every object of every
    replay must be the oracle's value for THAT replay's lengths; the 6th
    replay repeats the 2nd's lengths and values; an eager call on the same
    workspace closes."""
    import torch
    G, O = gpu, oracle_mod
    sc = _scene(O)
    _assert_steps_differ(sc)
    if map_cap is not None:
        monkeypatch.setenv("MCHECKSUM_GPU_SEG_MAP_CAP", str(map_cap))
    dev = torch.cat([torch.from_numpy(sc.host).cuda(), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    segs = [dev[int(a):int(a) + int(c)] for a, c in zip(sc.start, sc.cap)]
    batch = G.SegmentBatch(segs, sc.first)
    assert batch.nobj == sc.nobj and batch.bytes == int(np.sum(sc.cap[sc.first[0]:sc.first[-1]]))
    G.prepare(method)
    out = torch.zeros(sc.nobj, dtype=G.out_dtype(method), device="cuda")
    bad = {}

    def check(step, tag):
        got = G.as_unsigned(out).astype(np.uint64)
        want = sc.want(O, method, step)
        nb = int(np.count_nonzero(got != want))
        print(f"{method} map_cap={map_cap} {tag}: {nb} of {sc.nobj} objects differ", flush=True)
        if nb:
            bad[tag] = nb

    # refusals first: nothing reaches the device
    with pytest.raises(G.GpuChecksumError):
        batch.set_lengths(sc.steps[0][:-1])
    over = sc.steps[0].copy()
    over[7] = sc.cap[7] + 1
    with pytest.raises(G.GpuChecksumError):
        batch.set_lengths(over)
    batch.set_lengths(sc.steps[0])
    assert batch.bytes == int(np.sum(sc.steps[0][sc.first[0]:sc.first[-1]]))
    batch.checksum(method, out=out)  # eager
    _wait(torch, (method, "eager"))
    check(0, "eager")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        with pytest.raises(G.GpuChecksumError):
            batch.set_lengths(sc.steps[1])  # refused while capturing: nothing enqueued
        batch.checksum(method, out=out)
    vals = {}
    for r in range(6):
        step = 1 + r
        out.zero_()
        torch.cuda.synchronize()
        batch.set_lengths(sc.steps[step], stream=s)
        with torch.cuda.stream(s):
            g.replay()
        _wait(torch, (method, "replay", r), (s,))
        check(step, f"replay {r}")
        vals[r] = G.as_unsigned(out).copy()
    assert np.array_equal(vals[5], vals[1]), "the same lengths again must give the same values again"
    torch.cuda.synchronize()
    out.zero_()
    batch.set_lengths(sc.steps[7])
    batch.checksum(method, out=out)  # eager again, same workspace
    _wait(torch, (method, "closing eager"))
    check(7, "closing eager")
    assert not bad, bad
    assert G.queue_faults() == 0


def test_offsets_family_replay_with_new_tables(gpu, oracle_mod, monkeypatch):
    """One graph of four calls -- checksum_offsets crc32c and crc64, a zeroed
    mismatch counter then verify_offsets, and a split CRC-64 fixed batch --
    replayed 4 times; before each replay the buffer is refilled, the offsets
    table rewritten in place (same count, new cut points, empty payloads too)
    and a new set of mismatches planted in the expected values."""
    import torch
    G, O = gpu, oracle_mod
    L = G._lib()
    monkeypatch.setenv("MCHECKSUM_GPU_LIGHT", "0")
    monkeypatch.setenv("MCHECKSUM_GPU_SPLIT", "1")
    NB, COUNT, PIECE, NFIX = 8 << 20, 3000, 512 << 10, 16
    rng = np.random.default_rng(404)
    dev = torch.zeros(NB + 64, dtype=torch.uint8, device="cuda")
    offs_d = torch.zeros(COUNT + 1, dtype=torch.int64, device="cuda")
    exp_d = torch.zeros(COUNT, dtype=torch.int32, device="cuda")
    out32 = torch.zeros(COUNT, dtype=torch.int32, device="cuda")
    out64 = torch.zeros(COUNT, dtype=torch.int64, device="cuda")
    out_sp = torch.zeros(NFIX, dtype=torch.int64, device="cuda")
    status = torch.zeros(COUNT, dtype=torch.uint8, device="cuda")
    mism = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (allocated and zeroed on the default stream, used on another)

    def refill(k, stream):
        """New bytes, table and expected values, enqueued on `stream`; returns
        what the oracle says the graph must produce."""
        host = O.splitmix_bytes(NB, 0xC0FFEE + 7919 * k)
        lens = rng.integers(1, 2700, COUNT)
        lens[rng.choice(COUNT, 150, replace=False)] = 0
        offs = np.zeros(COUNT + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens)
        offs += np.uint64(rng.integers(0, 16))
        assert int(offs[-1]) <= NB
        w32 = O.batch_offsets("crc32c", host, offs, nthreads=8)
        w64 = O.batch_offsets("crc64", host, offs, nthreads=8)
        wsp = O.batch_fixed("crc64", host, PIECE, PIECE, NFIX, nthreads=8)
        victims = np.sort(rng.choice(COUNT, 60, replace=False))
        exp = w32.astype(np.uint32)
        exp[victims] ^= np.uint32(1) << rng.integers(0, 32, 60).astype(np.uint32)
        with torch.cuda.stream(stream):
            dev[:NB].copy_(torch.from_numpy(host))
            offs_d.copy_(torch.from_numpy(offs.astype(np.int64)))
            exp_d.copy_(torch.from_numpy(exp.view(np.int32)))
        return offs, w32, w64, wsp, victims

    def calls(stream, offsets_host=None):
        G.checksum_offsets("crc32c", dev, offs_d, out=out32, offsets_host=offsets_host)
        G.checksum_offsets("crc64", dev, offs_d, out=out64)
        mism.zero_()
        status.fill_(1)  # as gpu.verify_offsets: only a hashed payload's verdict overwrites it
        rc = L.mchecksum_gpu_verify_offsets(b"crc32c", dev.data_ptr(), offs_d.data_ptr(), COUNT, exp_d.data_ptr(),
                                            status.data_ptr(), mism.data_ptr(), stream.cuda_stream)
        assert rc == 0
        G.checksum_fixed("crc64", dev, PIECE, count=NFIX, out=out_sp)

    def check(tag, want):
        _offs, w32, w64, wsp, victims = want
        assert np.array_equal(G.as_unsigned(out32).astype(np.uint64), w32), tag
        assert np.array_equal(G.as_unsigned(out64), w64), tag
        assert np.array_equal(G.as_unsigned(out_sp), wsp), tag
        assert np.nonzero(status.cpu().numpy())[0].tolist() == victims.tolist(), tag
        assert int(mism.item()) == 60, tag

    G.prepare("crc32c")
    G.prepare("crc64")
    s = torch.cuda.Stream()
    want = refill(0, s)
    with torch.cuda.stream(s):
        calls(s, offsets_host=want[0])  # eager, the table validated once
    _wait(torch, "eager", (s,))
    check("eager", want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(g, stream=s):
        calls(s)
    for r in range(4):
        for o in (out32, out64, out_sp, status):
            o.zero_()
        mism.fill_(12345)  # the captured zero_() must run on every replay
        torch.cuda.synchronize()
        want = refill(1 + r, s)
        with torch.cuda.stream(s):
            g.replay()
        _wait(torch, ("replay", r), (s,))
        check(f"replay {r}", want)
    assert G.queue_faults() == 0
