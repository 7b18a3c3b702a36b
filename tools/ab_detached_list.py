"""One-process A/B of the detached calls with both sides by address list against
the table calls of the same library on the same bytes, launches interleaved,
each timed by its own event pair (the pattern of tools/ab_rpc_list.py).  Every
side goes straight through the C ABI with preallocated outputs.

  table:   mchecksum_gpu_verify_detached_messages / _seal_detached_messages on
           COUNT payloads laid back to back in one buffer and COUNT eager
           messages of 52 bytes in another (the yardstick: by
           profiles/detached_list/batch_kernel_pairs.txt its kernels are the
           parent's, instruction for instruction).
  list:    mchecksum_gpu_verify_detached_message_list / _seal_ on those same
           bytes, addressed by (address, length) on both sides: the cost of the
           two more arrays alone.
  spread:  the list calls with every payload in an allocation of its own and
           the eager messages in another buffer, both lists in an order
           shuffled against memory.

Shapes: 8192 x 1 MiB (DESIGN.md 4.21's), 1024 x 64 KiB, 64 x 1 MiB.  Every
round gives one median per side; the table shows the median over rounds, the
rounds' spread (min..max of the round medians), and for the two list sides
whether their median lies outside the table side's spread.

    python3 tools/ab_detached_list.py [--shapes 8kx1m ...] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x4D4331000000001A
HASH, MSG = 16, 52
SHAPES = {"8kx1m": (8192, 1 << 20), "1kx64k": (1024, 65536), "64x1m": (64, 1 << 20)}


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
    results = {}

    def show(tag, res):
        for n in res:
            rel = "" if n == "table" else f"  x{res[n]['median_ms'] / res['table']['median_ms']:.3f} of table"
            where = res[n].get("against_table_spread")
            rel += f"  ({where} the table call's rounds)" if where else ""
            print(f"{tag:15s} {n:7s} median {res[n]['median_ms']:.4f} ms  rounds "
                  f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms{rel}", flush=True)

    def rc0(rc):
        assert rc == 0, rc

    for shape in args.shapes:
        count, length = SHAPES[shape]
        po = torch.arange(count + 1, dtype=torch.int64, device="cuda") * length
        mo = torch.arange(count + 1, dtype=torch.int64, device="cuda") * MSG
        pay = torch.empty(count * length + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(pay, SEED)
        msgs = torch.empty(count * MSG + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(msgs, SEED + 1)
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        mb, mt, pb, pt, st, mm = msgs.data_ptr(), mo.data_ptr(), pay.data_ptr(), po.data_ptr(), status.data_ptr(), mism.data_ptr()
        # the same bytes by list
        maddr, mlen = mo[:-1] + mb, torch.full((count,), MSG, dtype=torch.int64, device="cuda")
        paddr, plen = po[:-1] + pb, torch.full((count,), length, dtype=torch.int64, device="cuda")
        # ... and spread: every payload in an allocation of its own, the messages in another buffer at shuffled places;
        # list entry i names payload i and message i
        extra = [torch.empty(length, dtype=torch.uint8, device="cuda") for _ in range(count)]
        order = torch.randperm(count, generator=torch.Generator().manual_seed(26)).tolist()
        for i in order:  # (allocated in one order, filled and listed in another)
            extra[i].copy_(pay[i * length:(i + 1) * length])
        spaddr = torch.tensor([t.data_ptr() for t in extra], dtype=torch.int64, device="cuda")
        smsgs = torch.empty_like(msgs)
        place = torch.tensor(order, dtype=torch.int64, device="cuda")   # message i lies at position place[i]
        smaddr = place * MSG + smsgs.data_ptr()
        la = (maddr.data_ptr(), mlen.data_ptr(), paddr.data_ptr(), plen.data_ptr())
        sa = (smaddr.data_ptr(), mlen.data_ptr(), spaddr.data_ptr(), plen.data_ptr())

        def verify_list(a):
            return lambda: rc0(L.mchecksum_gpu_verify_detached_message_list(b"crc32c", a[0], a[1], HASH, a[2], a[3], count, st, mm, s))

        def seal_list(a):
            return lambda: rc0(L.mchecksum_gpu_seal_detached_message_list(b"crc32c", a[0], a[1], HASH, a[2], a[3], count, st, s))

        sides = {
            "seal": {
                "table": lambda: rc0(L.mchecksum_gpu_seal_detached_messages(b"crc32c", mb, mt, HASH, pb, pt, count, st, s)),
                "list": seal_list(la),
                "spread": seal_list(sa),
            },
            "verify": {
                "table": lambda: rc0(L.mchecksum_gpu_verify_detached_messages(b"crc32c", mb, mt, HASH, pb, pt, count, st, mm, s)),
                "list": verify_list(la),
                "spread": verify_list(sa),
            },
        }
        print(f"{shape}: {count} payloads of {length} bytes, eager messages of {MSG}", flush=True)
        # a correct sender's batch made by the table call; the spread messages get the same bytes, so every side's
        # seal must reproduce them and every side's verify must pass, before any is timed
        sides["seal"]["table"]()
        smsgs[:count * MSG].view(count, MSG)[place] = msgs[:count * MSG].view(count, MSG)
        torch.cuda.synchronize()
        want, swant = msgs.clone(), smsgs.clone()
        for tag in ("verify", "seal"):
            for n, call in sides[tag].items():
                mism.zero_()
                status.fill_(1)
                if tag == "seal":   # (the slots cleared first: the seal has to write them)
                    msgs[:count * MSG].view(count, MSG)[:, HASH:HASH + 4] = 0
                    smsgs[:count * MSG].view(count, MSG)[:, HASH:HASH + 4] = 0
                call()
                torch.cuda.synchronize()
                assert int(status.max().item()) == 0 and int(mism.item()) == 0, (tag, n)
                if tag == "seal":
                    assert torch.equal(smsgs if n == "spread" else msgs, swant if n == "spread" else want), (tag, n)
                    msgs.copy_(want)
                    smsgs.copy_(swant)
        for tag in sides:
            res = ab(torch, sides[tag], args.rounds, args.iters)
            show(f"{shape} {tag}", res)
            results[f"{shape}/{tag}"] = res
        torch.cuda.synchronize()
        assert G.queue_faults() == 0
        del pay, msgs, smsgs, extra
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
