"""One-process A/B of the RPC message calls of an XDR build by address list
against the table calls, launches interleaved, each side timed by its own
event pair (the pattern of tools/ab_rpc_xdr.py).  Every side goes straight
through the C ABI with preallocated outputs.  Per operation (verify, seal,
unpack, pack):

  table       this commit's _rpc_xdr_messages call on the messages laid contiguously
  list        the _rpc_xdr_message_list call on the same bytes in the same places
              (addresses are base + offset)
  list_far    the list call with every message in an allocation of its own (counts
              up to 64), else spread over 64 allocations, the list in an order
              shuffled across them
  table_prev  the PARENT commit's table call, from its library loaded beside this
              one (make prev): the table kernels did not move

Shapes: COUNT request messages of 20 header bytes and the iovec schema (a u32
length, then LEN bytes), none deferred: 8192 x 64 KiB and 65536 x 4 KiB in the
throughput layout, 64 x 4 KiB in the latency layout.  One warm-up round, then
ROUNDS rounds of ITERS launches of every side; every round gives one median
per side.  The table shows the median over rounds, the rounds' spread (min..max
of the round medians), each list side's ratio to the table side and whether its
median lies inside, above or below the table's spread.

    python3 tools/ab_rpc_xdr_list.py --prev build/variants/libmchecksum_prev.so [--shapes ...] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x4D43310000000028
PAY, HASH = 20, 16
SHAPES = {"64x4k": (64, 4096), "64kx4k": (65536, 4096), "8kx64k": (8192, 65536)}
FAR_ALLOCS = 64


def ab(torch, sides, rounds, iters):
    stream = torch.cuda.current_stream()
    med = {n: [] for n in sides}
    for r in range(rounds + 1):
        evs = {n: [] for n in sides}
        for _ in range(iters):
            for n, call in sides.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                evs[n].append((a, b))
        torch.cuda.synchronize()
        if r > 0:  # round 0 = warm-up
            for n in sides:
                med[n].append(float(np.median([a.elapsed_time(b) for a, b in evs[n]])))
    res = {}
    for n in sides:
        t = np.asarray(med[n])
        res[n] = {"median_ms": float(np.median(t)), "round_min_ms": float(t.min()), "round_max_ms": float(t.max())}
    for n in ("list", "list_far", "table_prev"):
        m, ref = res[n]["median_ms"], res["table"]
        res[n]["against_table_spread"] = ("below" if m < ref["round_min_ms"] else
                                          "above" if m > ref["round_max_ms"] else "inside")
        res[n]["ratio_to_table"] = m / ref["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev", required=True, help="the parent commit's libmchecksum.so (make prev)")
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6, help="interleaved launches of every side per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from mercury_amd import gpu as G
    from mercury_amd._lib import XdrField, load_library
    L = load_library()
    P = ctypes.CDLL(os.path.abspath(args.prev))
    for n in ("verify_rpc_xdr_messages", "seal_rpc_xdr_messages", "unpack_rpc_xdr_messages", "pack_rpc_xdr_messages", "prepare"):
        f = getattr(P, "mchecksum_gpu_" + n)
        f.argtypes, f.restype = getattr(L, "mchecksum_gpu_" + n).argtypes, ctypes.c_int
    for lib in (L, P):
        assert lib.mchecksum_gpu_prepare(b"crc32c") == 0 and lib.mchecksum_gpu_prepare(b"crc16") == 0
    fields = (XdrField * 2)(XdrField(G.XDR_INT, 4), XdrField(G.XDR_OPAQUE_LEN, 0))
    rng = np.random.default_rng(20261021)
    results = {}

    for shape in args.shapes:
        count, length = SHAPES[shape]
        size, isize = PAY + 4 + length, 4 + length
        mo = torch.arange(count + 1, dtype=torch.int64, device="cuda") * size
        so = torch.arange(count + 1, dtype=torch.int64, device="cuda") * isize
        blank = torch.empty(count * size + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(blank, SEED)
        blank[mo[:-1] + 10] &= 0xFE  # none deferred
        src = torch.empty(count * isize + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(src, SEED + 1)
        le = torch.tensor(list(length.to_bytes(4, "little")), dtype=torch.uint8, device="cuda")
        src[:count * isize].view(count, isize)[:, :4] = le
        buf, dst = blank.clone(), torch.zeros_like(src)
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(7, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        b, o, st = buf.data_ptr(), mo.data_ptr(), status.data_ptr()
        sp, dp, tp, cp = src.data_ptr(), dst.data_ptr(), so.data_ptr(), counts.data_ptr()
        # the same places by list: base + offset
        lens = torch.full((count,), size, dtype=torch.int64, device="cuda")
        near = mo[:-1] + b
        # far: message i is slot pos[i] of allocation pos[i] // per -- shuffled across the allocations, 16 bytes
        # between neighbours, every allocation its own torch tensor
        nalloc = count if count <= FAR_ALLOCS else FAR_ALLOCS
        per, stride = count // nalloc, size + 16
        pos = rng.permutation(count)
        chunks = [torch.zeros(per * stride + 256, dtype=torch.uint8, device="cuda") for _ in range(nalloc)]
        assert len({c.data_ptr() for c in chunks}) == nalloc
        far_h = np.array([chunks[p // per].data_ptr() + (p % per) * stride for p in pos], dtype=np.uint64)
        far = torch.from_numpy(far_h.view(np.int64)).cuda()
        inv = torch.from_numpy(np.argsort(pos)).cuda()  # slot -> message

        def far_put(flat):
            rows = flat[:count * size].view(count, size)
            for j, c in enumerate(chunks):
                c[:per * stride].view(per, stride)[:, :size] = rows[inv[j * per:(j + 1) * per]]

        def far_get():
            out = torch.empty(count, size, dtype=torch.uint8, device="cuda")
            for j, c in enumerate(chunks):
                out[inv[j * per:(j + 1) * per]] = c[:per * stride].view(per, stride)[:, :size]
            return out.view(-1)

        def rc0(rc):
            assert rc == 0, rc

        rpc = (b"crc16", b"crc32c", 0, fields, 2)

        def table(lib):
            return {
                "verify": lambda: rc0(lib.mchecksum_gpu_verify_rpc_xdr_messages(*rpc, b, o, count, PAY, HASH, st, cp, s)),
                "seal": lambda: rc0(lib.mchecksum_gpu_seal_rpc_xdr_messages(*rpc, b, o, count, PAY, HASH, st, s)),
                "unpack": lambda: rc0(lib.mchecksum_gpu_unpack_rpc_xdr_messages(*rpc, b, o, count, PAY, HASH, dp, tp, st, cp, s)),
                "pack": lambda: rc0(lib.mchecksum_gpu_pack_rpc_xdr_messages(*rpc, sp, tp, b, o, count, PAY, HASH, st, s)),
            }

        def by_list(addr):
            a, n = addr.data_ptr(), lens.data_ptr()
            return {
                "verify": lambda: rc0(L.mchecksum_gpu_verify_rpc_xdr_message_list(*rpc, a, n, count, PAY, HASH, st, cp, s)),
                "seal": lambda: rc0(L.mchecksum_gpu_seal_rpc_xdr_message_list(*rpc, a, n, count, PAY, HASH, st, s)),
                "unpack": lambda: rc0(L.mchecksum_gpu_unpack_rpc_xdr_message_list(*rpc, a, n, count, PAY, HASH, dp, tp, st, cp, s)),
                "pack": lambda: rc0(L.mchecksum_gpu_pack_rpc_xdr_message_list(*rpc, sp, tp, a, n, count, PAY, HASH, st, s)),
            }
        cur, prev, lst, lfar = table(L), table(P), by_list(near), by_list(far)

        print(f"{shape}: {count} messages of {PAY} + 4 + {length} bytes, iovec schema; list_far over {nalloc} allocations",
              flush=True)
        # the list calls write what the table call writes, in both placements, and read it clean
        cur["pack"]()
        packed = buf.clone()
        buf.copy_(blank)
        lst["pack"]()
        far_put(blank)
        lfar["pack"]()
        torch.cuda.synchronize()
        assert torch.equal(buf, packed) and torch.equal(far_get(), packed[:count * size])
        for side in (lst, lfar):
            counts.zero_()
            dst.zero_()
            side["verify"]()
            side["unpack"]()
            side["seal"]()
            torch.cuda.synchronize()
            assert counts.tolist() == [2 * count, 0, 0, 0, 0, 0, 0], counts.tolist()
            assert torch.equal(dst[:count * isize], src[:count * isize])
        assert torch.equal(buf, packed) and torch.equal(far_get(), packed[:count * size])
        for op in ("verify", "seal", "unpack", "pack"):
            res = ab(torch, {"table": cur[op], "list": lst[op], "list_far": lfar[op], "table_prev": prev[op]}, args.rounds,
                     args.iters)
            for n, r in res.items():
                extra = f"  x{r['ratio_to_table']:.3f} of table ({r['against_table_spread']} its rounds)" if n != "table" else ""
                print(f"{shape + ' ' + op:15s} {n:10s} median {r['median_ms']:.4f} ms  rounds "
                      f"{r['round_min_ms']:.4f}..{r['round_max_ms']:.4f} ms{extra}", flush=True)
            results[f"{shape}/{op}"] = res
        torch.cuda.synchronize()
        assert torch.equal(buf, packed) and torch.equal(far_get(), packed[:count * size]) and G.queue_faults() == 0
        del buf, blank, packed, src, dst, chunks
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
