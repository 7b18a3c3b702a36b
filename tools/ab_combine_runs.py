"""One-process A/B of mchecksum_gpu_combine_runs (B) against the route that
existed before it (A): K - 1 mchecksum_gpu_combine launches that fold every
run's K chunk CRCs left to right.  HIP events around each whole sequence, the
two sides alternating; every round gives one median per side, the table shows
the median over rounds and the rounds' min..max (the run-to-run band).

Side A gets its tables laid out for it beforehand, chunk-major ([K][runs]), so
every step's operands are contiguous and no host work but the launches is
timed; its calls go straight through ctypes.  Both sides are checked against
each other before timing.

Shapes: RUNSxK (e.g. 4096x16), and "two:N:U" -- one run of N chunks joined in
two levels through out_len: runs of U, then one run over the results -- beside
"1xN", the same run in one call.  Chunk lengths: "mix" = random 64..65536
bytes (up to four non-zero hex digits per Z^n), or a number = every chunk that
many bytes.

    python3 tools/ab_combine_runs.py [--shapes 4096x16 1024x1024 1x1048576 two:1048576:64]
                                     [--methods crc32c crc64] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x16", "1024x1024", "1x1048576", "two:1048576:64"])
    ap.add_argument("--methods", nargs="+", default=["crc32c", "crc64"])
    ap.add_argument("--lens", default="mix")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="A/B pairs per round")
    ap.add_argument("--fold-budget", type=int, default=60000,
                    help="side A launches per round above which a round is one pair (and rounds are 3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from mercury_amd import gpu as G
    L = G._lib()
    rng = np.random.default_rng(0xC0DE)
    results = {}
    for shape in args.shapes:
        two = shape.startswith("two:")
        if two:
            _, n, unit = shape.split(":")
            runs, k, unit = 1, int(n), int(unit)
        else:
            runs, k = (int(v) for v in shape.split("x"))
        nchunks = runs * k
        lens_h = (rng.integers(64, 65537, nchunks) if args.lens == "mix"
                  else np.full(nchunks, int(args.lens))).astype(np.int64)
        for method in args.methods:
            G.prepare(method)
            dt = G.out_dtype(method)
            words = rng.integers(-(1 << 31), 1 << 31, nchunks).astype(np.int32 if dt == torch.int32 else np.int64)
            if dt == torch.int64:
                words = words * np.int64(0x100000001)
            crc = torch.from_numpy(words).cuda()                       # run-major: run j's chunks adjacent
            lens = torch.from_numpy(lens_h).cuda()
            first = torch.arange(0, nchunks + 1, k, dtype=torch.int64, device="cuda")
            out = torch.empty(runs, dtype=dt, device="cuda")
            stream = torch.cuda.current_stream()
            h = stream.cuda_stream
            if two:
                first1 = torch.from_numpy(np.append(np.arange(0, k, unit), k).astype(np.int64)).cuda()
                n1 = first1.numel() - 1
                mid, mid_len = torch.empty(n1, dtype=dt, device="cuda"), torch.empty(n1, dtype=torch.int64, device="cuda")
                first2 = torch.tensor([0, n1], dtype=torch.int64, device="cuda")

                def side_b():
                    G.combine_runs(method, crc, lens, first1, out=mid, out_len=mid_len)
                    G.combine_runs(method, mid, mid_len, first2, out=out)
                side_a = None
            else:
                # side A's operands, chunk-major: step s joins acc with row s
                crc_t = crc.view(runs, k).t().contiguous()
                len_t = lens.view(runs, k).t().contiguous()
                acc = torch.empty(runs, dtype=dt, device="cuda")
                es = crc.element_size()
                m, pc, pl, pa = method.encode(), crc_t.data_ptr(), len_t.data_ptr(), acc.data_ptr()

                def side_a():
                    if k == 1:
                        acc.copy_(crc_t[0])
                    for s in range(1, k):  # the first step reads row 0 in place: K - 1 launches in all
                        rc = L.mchecksum_gpu_combine(m, pc if s == 1 else pa, pc + s * runs * es, pl + s * runs * 8,
                                                     runs, pa, h)
                        if rc:
                            raise RuntimeError(f"combine rc={rc}")

                def side_b():
                    G.combine_runs(method, crc, lens, first, out=out)
            sides = {"combine x (K-1)": side_a, "combine_runs": side_b}
            if side_a is None:
                del sides["combine x (K-1)"]
                one = G.combine_runs(method, crc, lens, torch.tensor([0, k], dtype=torch.int64, device="cuda"))
                side_b()
                assert torch.equal(out, one), "two levels differ from one"
            else:
                side_a()
                side_b()
                assert torch.equal(out, acc), "combine_runs differs from the combine fold"
            heavy = side_a is not None and k - 1 > args.fold_budget
            # a heavy side A runs once a round for three rounds, side B eight times a round between them
            rounds = 3 if heavy else args.rounds
            reps = {n: 1 if heavy and n != "combine_runs" else 8 if heavy else args.iters for n in sides}
            med = {n: [] for n in sides}
            for r in range(rounds + (0 if heavy else 1)):  # (the check above warmed both sides up)
                evs = {n: [] for n in sides}
                for i in range(max(reps.values())):
                    for n, call in sides.items():
                        if i >= reps[n]:
                            continue
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        call()
                        b.record(stream)
                        evs[n].append((a, b))
                torch.cuda.synchronize()
                if heavy or r > 0:
                    for n in sides:
                        med[n].append(float(np.median([a.elapsed_time(b) for a, b in evs[n]])))
            assert G.queue_faults() == 0
            res = {}
            for n in sides:
                t = np.asarray(med[n])
                res[n] = {"median_ms": float(np.median(t)), "round_min_ms": float(t.min()), "round_max_ms": float(t.max()),
                          "samples": int(rounds * reps[n]), "launches": (k - 1 if n != "combine_runs" else 2 if two else 1)}
                print(f"{shape:18s} {method:7s} {n:16s} median {res[n]['median_ms']:10.4f} ms  rounds "
                      f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms  ({rounds * reps[n]} samples)",
                      flush=True)
            results[f"{shape}/{method}"] = res
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
