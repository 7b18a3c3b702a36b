"""One-process A/B of the copying RPC message entry points against the existing
calls of the same library for the same job, launches interleaved, each timed by
its own event pair (the pattern of tools/ab_rpc_messages.py).  Every side goes
straight through the C ABI with preallocated outputs.

  unpack:  mchecksum_gpu_unpack_rpc_messages (fused) against
           mchecksum_gpu_verify_rpc_messages then mchecksum_gpu_unpack_messages
           (route), and unpack_messages alone (floor).
  pack:    mchecksum_gpu_pack_rpc_messages (fused) against
           mchecksum_gpu_pack_messages then mchecksum_gpu_seal_core_headers
           (route), and pack_messages alone (floor).

Shapes: COUNT messages of a 16-byte request header, a 4-byte HG header and a
payload of LEN bytes, none deferred: 64 x 4 KiB, 1024 x 4 KiB, 65536 x 4 KiB,
65536 x 64 KiB; the other buffer holds the payloads back to back.  `mixed`:
65536 x 4 KiB with every eighth message deferred (HG_CORE_MORE_DATA set), the
fused calls alone -- the route would report those messages as corrupt.  Every
round gives one median per side; the table shows the median over rounds, the
rounds' spread (min..max of the round medians), and for the fused side whether
its median lies outside the route's spread, and on which side.

    python3 tools/ab_rpc_copy.py [--shapes 64x4k ...] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x4D43310000000017
PAY, HASH, FLAGS = 20, 16, 10
SHAPES = {"64x4k": (64, 4096, 0), "1kx4k": (1024, 4096, 0), "64kx4k": (65536, 4096, 0), "64kx64k": (65536, 65536, 0),
          "mixed": (65536, 4096, 8)}


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
    if "route" in res:
        f, r = res["fused"]["median_ms"], res["route"]
        res["fused"]["against_route_spread"] = ("below" if f < r["round_min_ms"] else
                                                "above" if f > r["round_max_ms"] else "inside")
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
            where = res[n].get("against_route_spread")
            rel += f"  ({where} the route's rounds)" if where else ""
            print(f"{tag:15s} {n:10s} median {res[n]['median_ms']:.4f} ms  rounds "
                  f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms{rel}", flush=True)

    for shape in args.shapes:
        count, length, every = SHAPES[shape]
        size = PAY + length
        mo = torch.arange(count + 1, dtype=torch.int64, device="cuda") * size
        to = torch.arange(count + 1, dtype=torch.int64, device="cuda") * length
        blank = torch.empty(count * size + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(blank, SEED)
        flags = mo[:-1] + FLAGS
        blank[flags] &= 0xFE
        if every:
            blank[flags[::every]] |= 1
        src = torch.empty(count * length + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(src, SEED + 1)
        buf = blank.clone()
        dst = torch.zeros_like(src)
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(7, dtype=torch.int32, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        b, o, st = buf.data_ptr(), mo.data_ptr(), status.data_ptr()
        sp, dp, tp = src.data_ptr(), dst.data_ptr(), to.data_ptr()

        def rc0(rc):
            assert rc == 0, rc

        u_fused = lambda: rc0(L.mchecksum_gpu_unpack_rpc_messages(b"crc16", b"crc32c", 0, b, o, count, PAY, HASH, dp, tp, st,
                                                                  counts.data_ptr(), s))
        p_fused = lambda: rc0(L.mchecksum_gpu_pack_rpc_messages(b"crc16", b"crc32c", 0, sp, tp, b, o, count, PAY, HASH, st, s))
        v_rpc = lambda: rc0(L.mchecksum_gpu_verify_rpc_messages(b"crc16", b"crc32c", 0, b, o, count, PAY, HASH, st,
                                                                counts.data_ptr(), s))
        u_msg = lambda: rc0(L.mchecksum_gpu_unpack_messages(b"crc32c", b, o, count, PAY, HASH, dp, tp, st, mism.data_ptr(), s))
        p_msg = lambda: rc0(L.mchecksum_gpu_pack_messages(b"crc32c", sp, tp, b, o, count, PAY, HASH, st, s))
        s_hdr = lambda: rc0(L.mchecksum_gpu_seal_core_headers(b"crc16", 0, b, o, count, st, s))
        ndef = len(range(0, count, every)) if every else 0
        print(f"{shape}: {count} messages of {PAY} + {length} bytes, {ndef} deferred"
              + (f" ({ndef * length} payload bytes not moved)" if every else ""), flush=True)
        # pack once with the new call, unpack it, and check the routes agree before timing them
        p_fused()
        packed = buf.clone()
        u_fused()
        torch.cuda.synchronize()
        assert counts.tolist() == [count - ndef, 0, 0, 0, ndef, 0, 0], counts.tolist()
        keep = torch.ones(count, dtype=torch.bool, device="cuda")
        if every:
            keep[::every] = False
        assert torch.equal(dst[:count * length].view(count, length)[keep], src[:count * length].view(count, length)[keep])
        assert not every or int(dst[:count * length].view(count, length)[~keep].max().item()) == 0
        unpacked = dst.clone()
        if not every:
            buf.copy_(blank)
            p_msg()
            s_hdr()
            dst.zero_()
            v_rpc()
            u_msg()
            torch.cuda.synchronize()
            assert torch.equal(buf, packed) and torch.equal(dst, unpacked) and int(mism.item()) == 0
        if every:
            us, ps = {"fused": u_fused}, {"fused": p_fused}
        else:
            def u_route():
                v_rpc()
                u_msg()

            def p_route():
                p_msg()
                s_hdr()
            us, ps = {"route": u_route, "floor": u_msg, "fused": u_fused}, {"route": p_route, "floor": p_msg, "fused": p_fused}
        for tag, sides in (("unpack", us), ("pack", ps)):
            res = ab(torch, sides, args.rounds, args.iters)
            show(f"{shape} {tag}", res, "fused" if every else "floor")
            results[f"{shape}/{tag}"] = res
        torch.cuda.synchronize()
        assert torch.equal(buf, packed) and torch.equal(dst, unpacked) and G.queue_faults() == 0
        del buf, blank, packed, src, dst, unpacked
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
