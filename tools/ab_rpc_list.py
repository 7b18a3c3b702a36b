"""One-process A/B of the RPC message calls by address list against the table
calls of the same library on the same messages, launches interleaved, each
timed by its own event pair (the pattern of tools/ab_rpc_copy.py).  Every side
goes straight through the C ABI with preallocated outputs.

  table:   mchecksum_gpu_verify_rpc_messages / _unpack_rpc_messages on COUNT
           messages laid back to back in one buffer (the yardstick: by
           profiles/rpc_list/batch_kernel_pairs.txt its kernels are the
           parent's, instruction for instruction).
  list:    mchecksum_gpu_verify_rpc_message_list / _unpack_rpc_message_list on
           those same bytes, addressed by (address, length): the cost of the
           second array alone.
  spread:  the list calls on the same messages copied into four separate
           buffers, the list in an order shuffled across them.

Shapes: COUNT messages of a 16-byte request header, a 4-byte HG header and a
payload of LEN bytes, none deferred: 64 x 4 KiB, 1024 x 4 KiB, 65536 x 4 KiB,
65536 x 64 KiB.  Every round gives one median per side; the table shows the
median over rounds, the rounds' spread (min..max of the round medians), and for
the two list sides whether their median lies outside the table side's spread.

    python3 tools/ab_rpc_list.py [--shapes 64x4k ...] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x4D43310000000019
PAY, HASH, FLAGS = 20, 16, 10
NBUF = 4
SHAPES = {"64x4k": (64, 4096), "1kx4k": (1024, 4096), "64kx4k": (65536, 4096), "64kx64k": (65536, 65536)}


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
    base = res["table"]
    for n in sides:
        if n != "table":
            m = res[n]["median_ms"]
            res[n]["against_table_spread"] = ("below" if m < base["round_min_ms"] else
                                              "above" if m > base["round_max_ms"] else "inside")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6, help="interleaved launches of every side per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from mercury_amd import gpu as G
    from mercury_amd._lib import load_library
    L = load_library()
    G.prepare("crc32c")
    G.prepare("crc16")
    results = {}

    def show(tag, res):
        for n in res:
            rel = "" if n == "table" else f"  x{res[n]['median_ms'] / res['table']['median_ms']:.3f} of table"
            where = res[n].get("against_table_spread")
            rel += f"  ({where} the table call's rounds)" if where else ""
            print(f"{tag:15s} {n:7s} median {res[n]['median_ms']:.4f} ms  rounds "
                  f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms{rel}", flush=True)

    for shape in args.shapes:
        count, length = SHAPES[shape]
        size = PAY + length
        mo = torch.arange(count + 1, dtype=torch.int64, device="cuda") * size
        to = torch.arange(count + 1, dtype=torch.int64, device="cuda") * length
        buf = torch.empty(count * size + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(buf, SEED)
        buf[mo[:-1] + FLAGS] &= 0xFE
        src = torch.empty(count * length + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(src, SEED + 1)
        dst = torch.zeros_like(src)
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(7, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        b, o, st, cn = buf.data_ptr(), mo.data_ptr(), status.data_ptr(), counts.data_ptr()
        dp, tp = dst.data_ptr(), to.data_ptr()

        def rc0(rc):
            assert rc == 0, rc

        # a correct sender's batch, made by the table call
        rc0(L.mchecksum_gpu_pack_rpc_messages(b"crc16", b"crc32c", 0, src.data_ptr(), tp, b, o, count, PAY, HASH, st, s))
        # the same bytes by list
        lens = torch.full((count,), size, dtype=torch.int64, device="cuda")
        addr = mo[:-1] + b
        # ... and spread over four buffers: memory position m holds message order[m]; list entry i names message i
        order = torch.randperm(count, generator=torch.Generator().manual_seed(19)).cuda()
        inv = torch.empty_like(order)
        inv[order] = torch.arange(count, device="cuda")
        q = count // NBUF
        rows = buf[:count * size].view(count, size)
        parts = [rows[order[k * q:(k + 1) * q]].contiguous() for k in range(NBUF)]
        bases = torch.tensor([p.data_ptr() for p in parts], dtype=torch.int64, device="cuda")
        saddr = bases[inv // q] + (inv % q) * size
        la, ll, sa = addr.data_ptr(), lens.data_ptr(), saddr.data_ptr()

        sides = {
            "verify": {
                "table": lambda: rc0(L.mchecksum_gpu_verify_rpc_messages(b"crc16", b"crc32c", 0, b, o, count, PAY, HASH, st, cn, s)),
                "list": lambda: rc0(L.mchecksum_gpu_verify_rpc_message_list(b"crc16", b"crc32c", 0, la, ll, count, PAY, HASH, st, cn, s)),
                "spread": lambda: rc0(L.mchecksum_gpu_verify_rpc_message_list(b"crc16", b"crc32c", 0, sa, ll, count, PAY, HASH, st, cn, s)),
            },
            "unpack": {
                "table": lambda: rc0(L.mchecksum_gpu_unpack_rpc_messages(b"crc16", b"crc32c", 0, b, o, count, PAY, HASH, dp, tp, st, cn, s)),
                "list": lambda: rc0(L.mchecksum_gpu_unpack_rpc_message_list(b"crc16", b"crc32c", 0, la, ll, count, PAY, HASH, dp, tp, st, cn, s)),
                "spread": lambda: rc0(L.mchecksum_gpu_unpack_rpc_message_list(b"crc16", b"crc32c", 0, sa, ll, count, PAY, HASH, dp, tp, st, cn, s)),
            },
        }
        print(f"{shape}: {count} messages of {PAY} + {length} bytes", flush=True)
        # every side gives all OK, and every unpack the payloads, before any is timed
        for tag in sides:
            for n, call in sides[tag].items():
                counts.zero_()
                status.fill_(5)
                dst.zero_()
                call()
                torch.cuda.synchronize()
                assert counts.tolist() == [count, 0, 0, 0, 0, 0, 0], (tag, n, counts.tolist())
                assert int(status.max().item()) == 0, (tag, n)
                assert tag != "unpack" or torch.equal(dst[:count * length], src[:count * length]), (tag, n)
        for tag in sides:
            res = ab(torch, sides[tag], args.rounds, args.iters)
            show(f"{shape} {tag}", res)
            results[f"{shape}/{tag}"] = res
        torch.cuda.synchronize()
        assert G.queue_faults() == 0
        del buf, src, dst, rows, parts
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
