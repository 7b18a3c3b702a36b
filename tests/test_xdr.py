"""XDR-mode proc checksum (include/mchecksum_gpu.h,
mchecksum_gpu_checksum_xdr).

In a Mercury built with MERCURY_USE_XDR the proc buffer holds XDR (integers
big-endian in 4/8-byte slots, byte arrays zero-padded to 4) while the
checksum covers the host-order values (/root/reference/src/mercury_proc.h:
110-122,147-160).  CPU tests pin the oracle's restatement (oracle.xdr_*)
on test_proc's two payloads; GPU tests compare the batch kernel with
oracle.crc(method, xdr_hashed_stream(...)) on the fixtures and on random
messages of every field kind."""
import json
import os

import numpy as np
import pytest

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "test_proc.json")))


def test_xdr_images_hash_the_host_values(oracle_mod):
    """test_proc's struct and string in XDR: the hashed stream is exactly the
    non-XDR image, so the checksum value is the same in both builds."""
    O = oracle_mod
    for name, e in GOLD["payloads"].items():
        schema = [tuple(f) for f in e["xdr_schema"]]
        wire = bytes.fromhex(e["xdr_hex"])
        assert O.xdr_encode(schema, _values(O, name)) == wire
        assert O.xdr_hashed_stream(schema, wire) == bytes.fromhex(e["hex"])
        for m in ("crc32c", "crc64"):
            assert O.crc(m, O.xdr_hashed_stream(schema, wire)) == int(e[m], 16)
        assert O.xdr_hashed_stream(schema, wire[:-1]) is None  # truncated


def _values(O, name):
    return [1, 2, 3, 4] if name == "uint_struct" else [6, b"Hello\x00", 0, 0]


# ----------------------------------------------------------------- GPU ----

def _schemas(O):
    I, OP, OPL, RAW, RAWL, SKIP = (O.XDR_INT, O.XDR_OPAQUE, O.XDR_OPAQUE_LEN, O.XDR_RAW, O.XDR_RAW_LEN,
                                   O.XDR_SKIP_IF_ZERO)
    return {
        # hg_perf_proc_iovec (Testing/perf/hg/mercury_perf.c:897-923): u32 length, raw bytes
        "iovec": [(I, 4), (OPL, 0)],
        # a struct with every integer width, an hg_string_t, a bulk handle
        # (u64 serialize size + save_ptr region) and a fixed opaque
        "mixed": [(I, 1), (I, 2), (I, 4), (I, 8), (I, 8), (SKIP, 3), (OPL, 0), (I, 1), (I, 1),
                  (I, 8), (RAWL, 0), (OP, 7), (RAW, 5), (I, 2)],
    }


def _random_values(rng, schema, O, max_len):
    vals, last, f = [], None, 0
    while f < len(schema):
        kind, size = schema[f]
        if kind == O.XDR_SKIP_IF_ZERO:
            if last == 0:
                f += size
            f += 1
            continue
        nxt = schema[f + 1][0] if f + 1 < len(schema) else None
        if kind == O.XDR_INT:
            if nxt in (O.XDR_OPAQUE_LEN, O.XDR_RAW_LEN) or (nxt == O.XDR_SKIP_IF_ZERO):
                v = int(rng.choice([0, 1, 3, 4, 5, 63, 64, 65, 1000, int(rng.integers(0, max_len))]))
            else:
                v = int(rng.integers(-(1 << (8 * size - 1)), 1 << (8 * size - 1)))  # signed range, sign-extended
            vals.append(v)
            last = v & ((1 << (8 * size)) - 1)
        else:
            n = last if kind in (O.XDR_OPAQUE_LEN, O.XDR_RAW_LEN) else size
            vals.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        f += 1
    return vals


def _run(gpu, method, msgs, schema, status=False):
    import torch
    off = np.zeros(len(msgs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    blob = b"".join(msgs)
    data = torch.zeros(len(blob) + 64, dtype=torch.uint8, device="cuda")
    if blob:
        data[:len(blob)].copy_(torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()))
    r = gpu.checksum_xdr(method, data, torch.from_numpy(off).cuda(), schema, status=status, offsets_host=off)
    if status:
        return gpu.as_unsigned(r[0]), r[1].cpu().numpy()
    return gpu.as_unsigned(r)


# the kernels a call can take: "0" the latency layout (byte-table walk), "1"
# the throughput layout (payload step loop for fields >= 256 B, work queue) with
# default loads, "1-nt" the same with non-temporal loads (MCHECKSUM_GPU_NT=1:
# what a batch of 8192 messages and more takes by itself; the latency layout
# has no such variant)
LAYOUTS = ["0", "1", "1-nt"]
# every reflected 32- and 64-bit model ("crc64" is crc64-xz).  crc64-jones: zero
# initial value (the running register the step loop starts from is then 0 at
# the first field); crc32, crc64-go-iso: a second polynomial of either width
METHODS = ["crc32c", "crc32", "crc64", "crc64-go-iso", "crc64-jones"]


def _path(monkeypatch, layout):
    """Select the kernel of LAYOUTS' entry `layout` (the library re-reads its
    settings on every change made through this monkeypatch)."""
    monkeypatch.setenv("MCHECKSUM_GPU_XDR_FAST", layout[0])
    if layout.endswith("-nt"):
        monkeypatch.setenv("MCHECKSUM_GPU_NT", "1")
    else:
        monkeypatch.delenv("MCHECKSUM_GPU_NT", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", ["crc32c", "crc64"])
def test_gpu_xdr_test_proc_fixtures(gpu, method, layout, monkeypatch):
    _path(monkeypatch, layout)
    for name, e in GOLD["payloads"].items():
        schema = [tuple(f) for f in e["xdr_schema"]]
        got = _run(gpu, method, [bytes.fromhex(e["xdr_hex"])] * 3, schema)
        assert got.tolist() == [int(e[method], 16)] * 3, name


_shared = {}


def _once(key, make):
    """A batch and its oracle values are built once and shared by the cases that use them."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def _oracle_crcs(O, key, method, schema, msgs):
    return _once((key, method), lambda: [O.crc(method, O.xdr_hashed_stream(schema, m)) for m in msgs])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["iovec", "mixed"])
def test_gpu_xdr_random_messages(gpu, oracle_mod, method, kind, layout, monkeypatch):
    _path(monkeypatch, layout)
    O = oracle_mod
    schema = _schemas(O)[kind]

    def make():
        rng = np.random.default_rng(17 if kind == "iovec" else 18)
        return [O.xdr_encode(schema, _random_values(rng, schema, O, 70000 if i % 97 == 0 else 3000))
                for i in range(700)]

    msgs = _once(("random", kind), make)
    got = _run(gpu, method, msgs, schema)
    assert got.tolist() == _oracle_crcs(O, ("random", kind), method, schema, msgs)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_xdr_truncated_messages_are_flagged(gpu, oracle_mod, layout, monkeypatch):
    _path(monkeypatch, layout)
    O = oracle_mod
    schema = _schemas(O)["mixed"]
    rng = np.random.default_rng(5)
    msgs = [O.xdr_encode(schema, _random_values(rng, schema, O, 500)) for _ in range(40)]
    cut = {3: 1, 10: 5, 20: len(msgs[20]) // 2}
    msgs = [m[:len(m) - cut[i]] if i in cut else m for i, m in enumerate(msgs)]
    got, st = _run(gpu, "crc32c", msgs, schema, status=True)
    assert sorted(np.nonzero(st)[0].tolist()) == sorted(cut)
    for i, m in enumerate(msgs):
        if i not in cut:
            assert int(got[i]) == O.crc("crc32c", O.xdr_hashed_stream(schema, m))


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["crc32c", "crc64"])
def test_gpu_xdr_large_iovec_batch(gpu, oracle_mod, method):
    """A batch past 1024 messages takes the throughput layout by default:
    5000 hg_perf_proc_iovec messages of C4's length mix (u32 length, bytes,
    zero pad), every CRC equal to the oracle's over the hashed stream (the
    host-order length, then the bytes)."""
    import torch
    from mercury_amd.workload import varlen_lengths
    O = oracle_mod
    schema = _schemas(O)["iovec"]
    lens = varlen_lengths(0x4D43310000000004, 5000).astype(np.int64)
    rng = np.random.default_rng(23)
    msgs = [O.xdr_encode(schema, [int(n), rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()]) for n in lens]
    got = _run(gpu, method, msgs, schema)
    want = [O.crc(method, O.xdr_hashed_stream(schema, m)) for m in msgs]
    assert got.tolist() == want


BIG = 70001


def _rule_messages(O):
    """(schema, 8192 iovec messages): lengths under 64; about every 64th (every
    63rd) carries the next of LENS' lengths from 256 up, and one carries BIG."""
    schema = _schemas(O)["iovec"]
    rng = np.random.default_rng(41)
    large = [n for n in LENS if n >= 256]
    msgs = []
    for i in range(8192):
        n = BIG if i == 4100 else large[(i // 63) % len(large)] if i % 63 == 9 else (37 * i + 11) % 64
        msgs.append(O.xdr_encode(schema, [n, rng.integers(0, 256, n, dtype=np.uint8).tobytes()]))
    return schema, msgs


@pytest.mark.gpu
@pytest.mark.parametrize("count", [8191, 8192])
@pytest.mark.parametrize("method", ["crc32c", "crc64"])
def test_gpu_xdr_default_count_rule(gpu, oracle_mod, method, count, monkeypatch):
    """With no setting, a batch takes the throughput layout past 1024 messages
    and its non-temporal kernel from 8192 on (launch_plan.h: nt_by_count): 8192
    is the smallest count that runs xdr_fast_kernel<W, true> by itself, 8191 the
    largest that runs <W, false>.  Every CRC equal to the oracle's."""
    monkeypatch.delenv("MCHECKSUM_GPU_XDR_FAST", raising=False)
    monkeypatch.delenv("MCHECKSUM_GPU_NT", raising=False)
    O = oracle_mod
    schema, msgs = _once("rule", lambda: _rule_messages(O))
    got = _run(gpu, method, msgs[:count], schema)
    assert got.tolist() == _oracle_crcs(O, "rule", method, schema, msgs)[:count]


@pytest.mark.gpu
def test_gpu_xdr_rejects_bad_schemas(gpu):
    import torch
    data = torch.zeros(64, dtype=torch.uint8, device="cuda")
    offs = torch.tensor([0, 8], dtype=torch.int64, device="cuda")
    for bad in ([(0, 3)], [(9, 1)], [(5, 2), (0, 4)], [(0, 4)] * 65):
        with pytest.raises(gpu.GpuChecksumError):
            gpu.checksum_xdr("crc32c", data, offs, bad)
    with pytest.raises(gpu.GpuChecksumError):
        gpu.checksum_xdr("crc16", data, offs, [(0, 4)])


# Field lengths of the edge tests.  Up to 5: the 4-byte pad; 7..129: the 64
# lane ranges and the 128-B grid; 252..260: kXdrFastMin = 256, where the step
# loop takes over; 383, 384, 1151, 1152: the grid inside a step.  The step loop
# (payload32_g64 / payload64_g64) moves 1024 bytes a step through a ring of
# kRingOff = 8 (CRC-32) or kRingOff64 = 4 (CRC-64) steps: 1020..1025 and
# 2047..2049 are one and two steps, 4095..4099 the CRC-64 ring's fill, 8191..8193
# the CRC-32 ring's fill and two CRC-64 rings (the first length whose steady
# loop, which loads a step as it folds one, runs at all), 16383..16385 two
# CRC-32 rings.  The start alignment shifts the step count by one either way.
LENS = [0, 1, 3, 4, 5, 7, 8, 9, 127, 128, 129, 252, 255, 256, 257, 260, 383, 384, 1020, 1023, 1024, 1025,
        1151, 1152, 2047, 2048, 2049, 4095, 4096, 4097, 4099, 8191, 8192, 8193, 16383, 16384, 16385]


def _edge_messages(O):
    """(schema, messages): every length of LENS behind a raw lead-in of 0..15 bytes."""
    I, OPL, RAWL, OP = O.XDR_INT, O.XDR_OPAQUE_LEN, O.XDR_RAW_LEN, O.XDR_OPAQUE
    rng = np.random.default_rng(31)
    # lead-in length + bytes, the field under test, a fixed 300-B opaque, a raw tail
    schema = [(I, 4), (RAWL, 0), (I, 4), (OPL, 0), (OP, 300), (I, 8), (RAWL, 0)]
    msgs = []
    for a in range(16):
        for n in LENS:
            v = [a, rng.integers(0, 256, a, dtype=np.uint8).tobytes(), n,
                 rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
                 rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), 700 + a,
                 rng.integers(0, 256, 700 + a, dtype=np.uint8).tobytes()]
            msgs.append(O.xdr_encode(schema, v))
    return schema, msgs


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", METHODS)
def test_gpu_xdr_fast_field_edges(gpu, oracle_mod, method, layout, monkeypatch):
    """Field lengths around the throughput layout's step-loop threshold
    (kXdrFastMin = 256: shorter fields take the byte walk, longer ones the
    1 KiB step loop started from the running register), around the 1 KiB
    step, the 128-B grid and the loop's ring of loads (LENS), at every start
    alignment mod 16 (a raw lead-in of 0..15 bytes, so every odd address), and
    three large fields in one message (the register runs from one step loop
    into the next): every CRC equal to the oracle's over the hashed stream."""
    _path(monkeypatch, layout)
    O = oracle_mod
    schema, msgs = _once("edges", lambda: _edge_messages(O))
    got = _run(gpu, method, msgs, schema)
    assert got.tolist() == _oracle_crcs(O, "edges", method, schema, msgs)
