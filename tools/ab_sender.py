"""One-process A/B of the sender entry points against what the parent commit
offers for the same job, launches interleaved ABAB, each timed by its own
event pair (the pattern of tools/ab_stream_update.py).

  seal:  mchecksum_gpu_seal_messages (B) against mchecksum_gpu_verify_messages
         (A) on the same buffer -- the verify kernels are the parent's.
  pack:  mchecksum_gpu_pack_messages (B) against one contiguous device-to-
         device copy of the sum of the payload bytes followed by
         verify_messages over the packed buffer (A): the copy is an upper
         bound on what any separate gather of the payloads can do.

Shapes: "msgs" -- bench.py --config msgs' table (C4's 262144 packets of
64..65536 bytes as messages); "4k" -- 65536 messages of 20 + 4096 bytes, R
copies of source and destination used in rotation (--rotate R: cold lines).
--shift S moves the source base by S bytes: both tables are contiguous, so
(dst - src) mod 16 steps by 4 from one message to the next and only its
residue mod 4 can be chosen -- S = 0 gives {0, 4, 8, 12}, S = 1 the odd ones.
Every round gives one median per side; the table shows the median over rounds
and the rounds' spread (min..max of the round medians), the run-to-run band.

    python3 tools/ab_sender.py [--shapes msgs 4k] [--shift 0 1] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C4_COUNT, C4_SEED = 262144, 0x4D43310000000004
PAY, HASH = 20, 16


def ab(torch, sides, rounds, iters, ncopies):
    stream = torch.cuda.current_stream()
    med = {n: [] for n in sides}
    for r in range(rounds + 1):
        evs = {n: [] for n in sides}
        for k in range(iters):
            for j, (n, call) in enumerate(sides.items()):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call((2 * k + j) % ncopies)
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
    ap.add_argument("--shapes", nargs="+", default=["msgs", "4k"])
    ap.add_argument("--shift", nargs="+", type=int, default=[0, 1], help="source base shifts (bytes) for the pack A/B")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=12, help="A/B pairs per round")
    ap.add_argument("--rotate", type=int, default=4, help="copies of the 4k batch (>= 4: cold lines)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from mercury_amd import gpu as G
    from mercury_amd.workload import varlen_offsets
    G.prepare("crc32c")
    results = {}

    def show(tag, res, a, b):
        for n in (a, b):
            print(f"{tag:14s} {n:22s} median {res[n]['median_ms']:.4f} ms  rounds "
                  f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms", flush=True)
        print(f"{tag:14s} {b} vs {a}: {100 * (res[b]['median_ms'] / res[a]['median_ms'] - 1):+.2f}% in time", flush=True)

    for shape in args.shapes:
        if shape == "msgs":
            mo_h = varlen_offsets(C4_SEED, C4_COUNT).astype(np.uint64)
            ncopies = 1
        else:
            mo_h = np.arange(65536 + 1, dtype=np.uint64) * np.uint64(PAY + 4096)
            ncopies = max(1, args.rotate)
        count = len(mo_h) - 1
        lens = (mo_h[1:] - mo_h[:-1]).astype(np.int64) - PAY
        assert lens.min() >= 0
        so_h = np.zeros(count + 1, dtype=np.uint64)
        so_h[1:] = np.cumsum(lens)
        nsrc, ndst = int(so_h[-1]), int(mo_h[-1])
        mo, so = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo_h, so_h))
        srcs = [torch.empty(nsrc + 128, dtype=torch.uint8, device="cuda") for _ in range(ncopies)]
        dsts = [torch.full((ndst + 64,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(ncopies)]
        flat = torch.empty(nsrc + 64, dtype=torch.uint8, device="cuda")  # the contiguous copy's target
        for d in srcs:
            G.fill_splitmix(d, C4_SEED)
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        alg = nsrc + nsrc + 4 * count + 16 * (count + 1)
        print(f"{shape}: {count} messages, {nsrc} payload bytes; pack's algorithmic bytes {alg}", flush=True)

        # pack every destination once: sealed buffers for the verify side, and the check that they verify
        for s, d in zip(srcs, dsts):
            G.pack_messages(s[:nsrc], so, d, mo, status=status)
            G.verify_messages(d, mo, status=status, mismatches=mism)
        assert int(mism.item()) == 0 and int(status.sum().item()) == 0

        sides = {"verify_messages": lambda b: G.verify_messages(dsts[b], mo, status=status, mismatches=mism),
                 "seal_messages": lambda b: G.seal_messages(dsts[b], mo, status=status)}
        res = ab(torch, sides, args.rounds, args.iters, ncopies)
        show(f"{shape} seal", res, "verify_messages", "seal_messages")
        results[f"{shape}/seal"] = res

        for shift in args.shift:
            views = [s[shift:shift + nsrc] for s in srcs]

            def pair(b):
                flat[:nsrc].copy_(views[b])
                G.verify_messages(dsts[b], mo, status=status, mismatches=mism)

            sides = {"copy+verify_messages": pair,
                     "pack_messages": lambda b: G.pack_messages(views[b], so, dsts[b], mo, status=status)}
            res = ab(torch, sides, args.rounds, args.iters, ncopies)
            for n in res:
                res[n]["alg_GBs_median"] = alg / (res[n]["median_ms"] * 1e-3) / 1e9
            show(f"{shape} pack +{shift}", res, "copy+verify_messages", "pack_messages")
            results[f"{shape}/pack/shift{shift}"] = res
        torch.cuda.synchronize()
        assert int(mism.item()) == 0 and int(status.sum().item()) == 0
        assert G.queue_faults() == 0
        del srcs, dsts, flat
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
