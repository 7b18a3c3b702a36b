"""One-process A/B of the RPC message entry points against the parent commit's
route for the same job, launches interleaved, each timed by its own event pair
(the pattern of tools/ab_detached.py).  Every side goes straight through the C
ABI with preallocated outputs.

  verify:  mchecksum_gpu_verify_rpc_messages (fused) against
           mchecksum_gpu_verify_core_headers then mchecksum_gpu_verify_messages
           (route), and verify_messages alone (floor).
  seal:    mchecksum_gpu_seal_rpc_messages (fused) against seal_core_headers
           then seal_messages (route), and seal_messages alone (floor).

Shapes: COUNT messages of a 16-byte request header, a 4-byte HG header and a
payload of LEN bytes, none deferred: 64 x 4 KiB, 1024 x 4 KiB, 65536 x 4 KiB,
65536 x 64 KiB.  `mixed`: 65536 x 4 KiB with every eighth message deferred
(HG_CORE_MORE_DATA set), the fused calls alone -- the route would report those
messages as corrupt --, with the payload bytes the fused call does not read.
Every round gives one median per side; the table shows the median over rounds
and the rounds' spread (min..max of the round medians).

    python3 tools/ab_rpc_messages.py [--shapes 64x4k ...] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x4D43310000000016
PAY, HASH, FLAGS = 20, 16, 10
SHAPES = {"64x4k": (64, 4096, 0), "1kx4k": (1024, 4096, 0), "64kx4k": (65536, 4096, 0), "64kx64k": (65536, 65536, 0),
          "mixed": (65536, 4096, 8)}
OK, DEFERRED = 0, 4


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

    def show(tag, res, base):
        for n in res:
            rel = "" if n == base else f"  x{res[n]['median_ms'] / res[base]['median_ms']:.3f} of {base}"
            print(f"{tag:15s} {n:10s} median {res[n]['median_ms']:.4f} ms  rounds "
                  f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms{rel}", flush=True)

    for shape in args.shapes:
        count, length, every = SHAPES[shape]
        size = PAY + length
        mo = torch.arange(count + 1, dtype=torch.int64, device="cuda") * size
        buf = torch.empty(count * size + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(buf, SEED)
        flags = mo[:-1] + FLAGS
        buf[flags] &= 0xFE
        if every:
            buf[flags[::every]] |= 1
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(6, dtype=torch.int32, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        b, o, st = buf.data_ptr(), mo.data_ptr(), status.data_ptr()

        def rc0(rc):
            assert rc == 0, G.last_error() if hasattr(G, "last_error") else rc

        v_fused = lambda: rc0(L.mchecksum_gpu_verify_rpc_messages(b"crc16", b"crc32c", 0, b, o, count, PAY, HASH, st,
                                                                  counts.data_ptr(), s))
        s_fused = lambda: rc0(L.mchecksum_gpu_seal_rpc_messages(b"crc16", b"crc32c", 0, b, o, count, PAY, HASH, st, s))
        v_hdr = lambda: rc0(L.mchecksum_gpu_verify_core_headers(b"crc16", 0, b, o, count, st, mism.data_ptr(), s))
        v_msg = lambda: rc0(L.mchecksum_gpu_verify_messages(b"crc32c", b, o, count, PAY, HASH, st, mism.data_ptr(), s))
        s_hdr = lambda: rc0(L.mchecksum_gpu_seal_core_headers(b"crc16", 0, b, o, count, st, s))
        s_msg = lambda: rc0(L.mchecksum_gpu_seal_messages(b"crc32c", b, o, count, PAY, HASH, st, s))
        ndef = len(range(0, count, every)) if every else 0
        print(f"{shape}: {count} messages of {PAY} + {length} bytes, {ndef} deferred"
              + (f" ({ndef * length} payload bytes not read)" if every else ""), flush=True)
        # seal once with the new call, and check the routes agree before timing them
        s_fused()
        sealed = buf.clone()
        v_fused()
        torch.cuda.synchronize()
        assert counts.tolist() == [count - ndef, 0, 0, 0, ndef, 0], counts.tolist()
        if not every:
            s_hdr()
            s_msg()
            v_hdr()
            v_msg()
            torch.cuda.synchronize()
            assert torch.equal(buf, sealed) and int(mism.item()) == 0
        if every:
            vs, ss = {"fused": v_fused}, {"fused": s_fused}
        else:
            def v_route():
                v_hdr()
                v_msg()

            def s_route():
                s_hdr()
                s_msg()
            vs, ss = {"route": v_route, "floor": v_msg, "fused": v_fused}, {"route": s_route, "floor": s_msg, "fused": s_fused}
        for tag, sides in (("verify", vs), ("seal", ss)):
            res = ab(torch, sides, args.rounds, args.iters)
            show(f"{shape} {tag}", res, "fused" if every else "floor")
            results[f"{shape}/{tag}"] = res
        torch.cuda.synchronize()
        assert torch.equal(buf, sealed) and G.queue_faults() == 0
        del buf, sealed
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
