"""One-process A/B of the streaming copy-and-checksum call against the two-pass
path it replaces, launches interleaved ABAB on the same buffers, each side
timed by its own event pair (the loop of tools/ab_sender.py).

  A: mchecksum_gpu_update_offsets followed by one contiguous device-to-device
     copy of the same bytes, both inside one event pair.  Both are the parent
     commit's code; the contiguous copy is the most favourable form of the
     second pass (a real one scatters the chunks).
  B: mchecksum_gpu_update_copy_offsets -- hash and scatter in one pass.

Shapes: "c4" -- the C4 mix (64..65536-byte chunks) at count 8192, the
destinations a random permutation of the chunks; "64k" -- 1024 chunks of
64 KiB, R copies of source and destination used in rotation (--rotate R: cold
lines).  Every round gives one median per side; the table shows the median over
rounds and the rounds' spread (min..max of the round medians), the run-to-run
band, and says whether the fused call wins by more than the larger band.

    python3 tools/ab_stream_copy.py [--shapes c4 64k] [--methods crc32c crc64] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ab_sender import C4_SEED, ab  # noqa: E402  (the same ABAB loop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["c4", "64k"])
    ap.add_argument("--methods", nargs="+", default=["crc32c", "crc64"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=12, help="A/B pairs per round")
    ap.add_argument("--rotate", type=int, default=4, help="copies of the 64k batch (>= 4: cold lines)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from mercury_amd import gpu as G
    from mercury_amd.workload import varlen_offsets
    results = {}
    rng = np.random.default_rng(0xC0)

    for shape in args.shapes:
        if shape == "c4":
            so_h = varlen_offsets(C4_SEED, 8192).astype(np.int64)
            ncopies = 1
        else:
            so_h = np.arange(1024 + 1, dtype=np.int64) * 65536
            ncopies = max(1, args.rotate)
        count = len(so_h) - 1
        lens = so_h[1:] - so_h[:-1]
        nbytes = int(so_h[-1] - so_h[0])
        order = rng.permutation(count)  # chunk order[j] is the j-th in the destination
        ds_h = np.zeros(count, dtype=np.int64)
        ds_h[order] = np.concatenate([[0], np.cumsum(lens[order])[:-1]])
        so, ds = (torch.from_numpy(x).cuda() for x in (so_h, ds_h))
        srcs = [torch.empty(int(so_h[-1]) + 128, dtype=torch.uint8, device="cuda") for _ in range(ncopies)]
        dsts = [torch.full((nbytes + 64,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(ncopies)]
        for s in srcs:
            G.fill_splitmix(s, C4_SEED)
        lo = int(so_h[0])
        print(f"{shape}: {count} chunks, {nbytes} bytes", flush=True)

        for method in args.methods:
            G.prepare(method)
            # the fused call computes what the two passes compute, and moves the bytes where the tables say
            want = G.state_get(method, G.update_offsets(method, srcs[0], so, G.state_init(method, count)))
            got = G.state_get(method, G.update_copy_offsets(method, srcs[0], so, dsts[0], ds, G.state_init(method, count),
                                                            offsets_host=so_h, dst_starts_host=ds_h))
            assert torch.equal(want, got)
            for i in (0, count // 2, count - 1):
                assert torch.equal(dsts[0][int(ds_h[i]):int(ds_h[i] + lens[i])], srcs[0][int(so_h[i]):int(so_h[i + 1])])
            assert bool((dsts[0][nbytes:] == 0xEE).all())
            st_a, st_b = G.state_init(method, count), G.state_init(method, count)

            def two_pass(b):
                G.update_offsets(method, srcs[b], so, st_a)
                dsts[b][:nbytes].copy_(srcs[b][lo:lo + nbytes])

            a, bn = "update_offsets+copy", "update_copy_offsets"
            sides = {a: two_pass, bn: lambda b: G.update_copy_offsets(method, srcs[b], so, dsts[b], ds, st_b)}
            res = ab(torch, sides, args.rounds, args.iters, ncopies)
            tag = f"{shape} {method}"
            for n in (a, bn):
                res[n]["GBs_of_chunk_bytes_median"] = nbytes / (res[n]["median_ms"] * 1e-3) / 1e9
                print(f"{tag:12s} {n:22s} median {res[n]['median_ms']:.4f} ms  rounds "
                      f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms", flush=True)
            band = max(res[n]["round_max_ms"] - res[n]["round_min_ms"] for n in (a, bn))
            gain = res[a]["median_ms"] - res[bn]["median_ms"]
            res["fused_vs_two_pass_pct"] = 100 * (res[bn]["median_ms"] / res[a]["median_ms"] - 1)
            res["fused_wins_beyond_spread"] = bool(gain > band)
            print(f"{tag:12s} {bn} vs {a}: {res['fused_vs_two_pass_pct']:+.2f}% in time; gain {gain:.4f} ms, larger "
                  f"spread {band:.4f} ms: {'wins' if gain > band else 'does not win'} beyond the spread", flush=True)
            results[f"{shape}/{method}"] = res
            torch.cuda.synchronize()
            assert torch.equal(st_a, st_b)  # both sides advanced their states over the same bytes, equally often
        assert G.queue_faults() == 0
        del srcs, dsts
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
