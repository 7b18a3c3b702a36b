"""One-process A/B of the seed epilogue: mchecksum_gpu_checksum_offsets (A)
against mchecksum_gpu_update_offsets (B) on the same batch, launches
interleaved ABAB, each timed by its own event pair.

Shapes: "c4" -- bench.py's C4 offsets mix (262144 payloads of 64..65536
bytes); "4k" -- 65536 x 4 KiB as an offsets table, read on cold lines (launch
k reads copy k % R of R equal batches, --rotate R, as tools/ab_variants.py);
any other number N -- 65536 x N bytes packed, the same way (N = 4369 = 0x1111
takes four Z^n digit steps where 4096 takes one).
Every round gives one median per side; the table shows the median over rounds
and the rounds' spread (min..max of the round medians), which is the
run-to-run band a difference has to clear.

    python3 tools/ab_stream_update.py [--shapes c4 4k] [--methods crc32c crc64] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C4_COUNT, C4_SEED = 262144, 0x4D43310000000004


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["c4", "4k"])
    ap.add_argument("--methods", nargs="+", default=["crc32c", "crc64"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=12, help="A/B pairs per round")
    ap.add_argument("--rotate", type=int, default=4, help="copies of the 4k batch (>= 4: cold lines)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from mercury_amd import gpu as G
    from mercury_amd.workload import varlen_offsets
    results = {}
    for shape in args.shapes:
        if shape == "c4":
            off_h = varlen_offsets(C4_SEED, C4_COUNT)
            ncopies = 1
        else:
            # "4k": n = 0x1000, one Z^n digit step; "4369": n = 0x1111, four (the same
            # payload loop, so the difference of the two overheads is three digit steps)
            off_h = np.arange(65536 + 1, dtype=np.uint64) * np.uint64(4096 if shape == "4k" else int(shape))
            ncopies = max(1, args.rotate)
        count, nbytes = len(off_h) - 1, int(off_h[-1])
        offs = torch.from_numpy(off_h.astype(np.int64)).cuda()
        copies = [torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda") for _ in range(ncopies)]
        for d in copies:
            G.fill_splitmix(d, C4_SEED)
        for method in args.methods:
            G.prepare(method)
            out = torch.empty(count, dtype=G.out_dtype(method), device="cuda")
            state = G.state_init(method, count)
            # the seeded call computes what the one-shot call computes
            G.update_offsets(method, copies[0], offs, state)
            assert torch.equal(G.state_get(method, state), G.checksum_offsets(method, copies[0], offs))
            stream = torch.cuda.current_stream()
            sides = {"checksum_offsets": lambda d: G.checksum_offsets(method, d, offs, out=out),
                     "update_offsets": lambda d: G.update_offsets(method, d, offs, state)}
            med = {n: [] for n in sides}
            for r in range(args.rounds + 1):
                evs = {n: [] for n in sides}
                for k in range(args.iters):
                    for j, (n, call) in enumerate(sides.items()):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        call(copies[(2 * k + j) % ncopies])
                        b.record(stream)
                        evs[n].append((a, b))
                torch.cuda.synchronize()
                if r > 0:  # round 0 = warm-up
                    for n in sides:
                        med[n].append(float(np.median([a.elapsed_time(b) for a, b in evs[n]])))
            assert G.queue_faults() == 0
            res = {}
            for n in sides:
                t = np.asarray(med[n])
                res[n] = {"median_ms": float(np.median(t)), "round_min_ms": float(t.min()), "round_max_ms": float(t.max()),
                          "GBs_median": nbytes / (float(np.median(t)) * 1e-3) / 1e9}
                print(f"{shape:3s} {method:7s} {n:17s} median {res[n]['median_ms']:.4f} ms  rounds "
                      f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms  {res[n]['GBs_median']:.0f} GB/s",
                      flush=True)
            d = res["update_offsets"]["median_ms"] / res["checksum_offsets"]["median_ms"] - 1
            print(f"{shape:3s} {method:7s} update_offsets vs checksum_offsets: {100 * d:+.2f}% in time", flush=True)
            results[f"{shape}/{method}"] = res
        del copies
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
