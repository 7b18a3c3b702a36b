"""One-process A/B of the RPC message calls of an XDR build against the two
launches each replaces, the route measured on the PARENT commit's library
loaded beside this one (make prev), launches interleaved, each side timed by
its own event pair (the pattern of tools/ab_rpc_copy.py).  Every side goes
straight through the C ABI with preallocated outputs.

  verify:  mchecksum_gpu_verify_rpc_xdr_messages (fused) against the parent's
           mchecksum_gpu_verify_core_headers then mchecksum_gpu_verify_xdr_messages
           (route); this commit's verify_xdr_messages against the parent's
           (twin / twin_prev: the existing kernel did not move).
  seal:    seal_rpc_xdr_messages against seal_xdr_messages then seal_core_headers.
  unpack:  unpack_rpc_xdr_messages against verify_core_headers then unpack_xdr_messages.
  pack:    pack_rpc_xdr_messages against pack_xdr_messages then seal_core_headers.

Shapes: COUNT request messages of 20 header bytes and the iovec schema (a u32
length, then LEN bytes), none deferred: 8192 x 64 KiB and 65536 x 4 KiB in the
throughput layout, 64 x 4 KiB in the latency layout.  Every round gives one
median per side; the table shows the median over rounds, the rounds' spread
(min..max of the round medians), and for the fused side whether its median
lies inside, above or below the route's spread.

    python3 tools/ab_rpc_xdr.py --prev build/variants/libmchecksum_prev.so [--shapes ...] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x4D43310000000027
PAY, HASH = 20, 16
SHAPES = {"64x4k": (64, 4096), "64kx4k": (65536, 4096), "8kx64k": (8192, 65536)}


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
    for f, r in (("fused", "route"), ("twin", "twin_prev")):
        if f in res and r in res:
            m = res[f]["median_ms"]
            res[f]["against_" + r + "_spread"] = ("below" if m < res[r]["round_min_ms"] else
                                                  "above" if m > res[r]["round_max_ms"] else "inside")
            res[f]["ratio_to_" + r] = m / res[r]["median_ms"]
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
    for n in ("verify_core_headers", "seal_core_headers", "verify_xdr_messages", "seal_xdr_messages", "unpack_xdr_messages",
              "pack_xdr_messages", "prepare"):
        f = getattr(P, "mchecksum_gpu_" + n)
        f.argtypes, f.restype = getattr(L, "mchecksum_gpu_" + n).argtypes, ctypes.c_int
    for lib in (L, P):
        assert lib.mchecksum_gpu_prepare(b"crc32c") == 0 and lib.mchecksum_gpu_prepare(b"crc16") == 0
    fields = (XdrField * 2)(XdrField(G.XDR_INT, 4), XdrField(G.XDR_OPAQUE_LEN, 0))
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
        hstatus = torch.ones(count, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(7, dtype=torch.int32, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        b, o, st, hst = buf.data_ptr(), mo.data_ptr(), status.data_ptr(), hstatus.data_ptr()
        sp, dp, tp, cp, mp = src.data_ptr(), dst.data_ptr(), so.data_ptr(), counts.data_ptr(), mism.data_ptr()

        def rc0(rc):
            assert rc == 0, rc

        rpc = (b"crc16", b"crc32c", 0, fields, 2)
        xdr = (b"crc32c", fields, 2)
        fused = {
            "verify": lambda: rc0(L.mchecksum_gpu_verify_rpc_xdr_messages(*rpc, b, o, count, PAY, HASH, st, cp, s)),
            "seal": lambda: rc0(L.mchecksum_gpu_seal_rpc_xdr_messages(*rpc, b, o, count, PAY, HASH, st, s)),
            "unpack": lambda: rc0(L.mchecksum_gpu_unpack_rpc_xdr_messages(*rpc, b, o, count, PAY, HASH, dp, tp, st, cp, s)),
            "pack": lambda: rc0(L.mchecksum_gpu_pack_rpc_xdr_messages(*rpc, sp, tp, b, o, count, PAY, HASH, st, s)),
        }

        def twin(lib):
            return {
                "verify": lambda: rc0(lib.mchecksum_gpu_verify_xdr_messages(*xdr, b, o, count, PAY, HASH, st, mp, s)),
                "seal": lambda: rc0(lib.mchecksum_gpu_seal_xdr_messages(*xdr, b, o, count, PAY, HASH, st, s)),
                "unpack": lambda: rc0(lib.mchecksum_gpu_unpack_xdr_messages(*xdr, b, o, count, PAY, HASH, dp, tp, st, mp, s)),
                "pack": lambda: rc0(lib.mchecksum_gpu_pack_xdr_messages(*xdr, sp, tp, b, o, count, PAY, HASH, st, s)),
            }
        cur, prev = twin(L), twin(P)
        v_hdr = lambda: rc0(P.mchecksum_gpu_verify_core_headers(b"crc16", 0, b, o, count, hst, mp, s))
        s_hdr = lambda: rc0(P.mchecksum_gpu_seal_core_headers(b"crc16", 0, b, o, count, hst, s))

        def route(op):
            if op in ("verify", "unpack"):
                return lambda: (v_hdr(), prev[op]())
            return lambda: (prev[op](), s_hdr())

        print(f"{shape}: {count} messages of {PAY} + 4 + {length} bytes, iovec schema", flush=True)
        # pack with the new call, check it against the route's bytes and that both receivers read it clean
        fused["pack"]()
        packed = buf.clone()
        buf.copy_(blank)
        route("pack")()
        torch.cuda.synchronize()
        assert torch.equal(buf, packed)
        fused["verify"]()
        fused["unpack"]()
        torch.cuda.synchronize()
        assert counts.tolist() == [2 * count, 0, 0, 0, 0, 0, 0], counts.tolist()
        assert torch.equal(dst[:count * isize], src[:count * isize])
        fused["seal"]()
        torch.cuda.synchronize()
        assert torch.equal(buf, packed)
        for op in ("verify", "seal", "unpack", "pack"):
            res = ab(torch, {"route": route(op), "twin_prev": prev[op], "twin": cur[op], "fused": fused[op]}, args.rounds,
                     args.iters)
            for n, r in res.items():
                extra = "".join(f"  x{r[k]:.3f} of {k[9:]}" for k in r if k.startswith("ratio_to_"))
                extra += "".join(f"  ({r[k]} the {k[8:-7]}'s rounds)" for k in r if k.startswith("against_"))
                print(f"{shape + ' ' + op:15s} {n:10s} median {r['median_ms']:.4f} ms  rounds "
                      f"{r['round_min_ms']:.4f}..{r['round_max_ms']:.4f} ms{extra}", flush=True)
            results[f"{shape}/{op}"] = res
        torch.cuda.synchronize()
        assert torch.equal(buf, packed) and int(mism.item()) == 0 and G.queue_faults() == 0
        del buf, blank, packed, src, dst
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
