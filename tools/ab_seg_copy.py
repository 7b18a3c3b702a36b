"""One-process A/B of the gather / scatter calls against the two-pass paths they
replace, launches interleaved ABAB on the same buffers, each side timed by its
own event pair (the loop of tools/ab_sender.py).  The baselines are the parent
commit's code, never the code under test:

  gather   A: SegmentBatch.checksum, then torch.cat(segments of object j,
              out=view of dst) per object -- the most favourable second pass.
           B: SegmentBatch.gather.
  scatter  A: checksum_offsets over the contiguous objects, then one copy_ per
              segment.
           B: SegmentBatch.scatter.

Shapes: "seg" -- bench.py's seg layout (objects of 1 MiB in SEGS_PER_OBJECT
equal segments at the slots of workload.segment_slots), --count objects (the
bench runs 8192; the per-object and per-segment launches of side A make that
many a matter of minutes); "ragged" -- 120 objects of 0..6 segments from the
segment tests' length pool at random byte offsets.  Every round gives one
median per side; the table shows the median over rounds and the rounds' spread
(min..max of the round medians), and says whether the fused call wins by more
than the larger spread.

    python3 tools/ab_seg_copy.py [--shapes seg ragged] [--methods crc32c crc64] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ab_sender import ab  # noqa: E402  (the same ABAB loop)

POOL = [0, 1, 3, 7, 8, 15, 16, 17, 63, 64, 100, 1000, 4095, 4096, 4097, 65536, 100003, 262143, 262144, 262145, 600000,
        1 << 20, (1 << 20) + 5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["seg", "ragged"])
    ap.add_argument("--methods", nargs="+", default=["crc32c", "crc64"])
    ap.add_argument("--dirs", nargs="+", default=["gather", "scatter"])
    ap.add_argument("--count", type=int, default=1024, help="objects of the seg shape")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6, help="A/B pairs per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    from mercury_amd import gpu as G
    from mercury_amd.workload import segment_slots
    results = {}
    rng = np.random.default_rng(0x5E6)

    for shape in args.shapes:
        if shape == "seg":
            _, _, length, seed, _ = bench.CONFIGS["seg"]
            per = bench.SEGS_PER_OBJECT
            seg_len = length // per
            slots = segment_slots(seed, args.count * per)
            off = np.asarray(slots, dtype=np.int64) * seg_len
            lens = np.full(len(off), seg_len, dtype=np.int64)
            first = np.arange(0, args.count * per + 1, per)
            span = args.count * length
        else:
            lens, first = [], [0]
            for _ in range(120):
                lens += [POOL[int(rng.integers(0, len(POOL)))] for _ in range(int(rng.integers(0, 7)))]
                first.append(len(lens))
            lens, first = np.asarray(lens, dtype=np.int64), np.asarray(first)
            # disjoint segments (scatter writes them), a few bytes apart, in a shuffled order
            off = np.zeros(len(lens), dtype=np.int64)
            at = 0
            for i in rng.permutation(len(lens)):
                at += int(rng.integers(0, 32))
                off[i] = at
                at += int(lens[i])
            span = at
        nobj = len(first) - 1
        P = np.concatenate([[0], np.cumsum(lens)])
        N = P[first[1:]] - P[first[:-1]]
        nbytes = int(N.sum())
        starts_h = np.concatenate([[0], np.cumsum(N)[:-1]]).astype(np.int64)  # objects back to back
        offs_h = np.concatenate([starts_h, [nbytes]]).astype(np.int64)
        segmem = torch.empty(span + 128, dtype=torch.uint8, device="cuda")
        flat = torch.empty(nbytes + 128, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(segmem, 0x5E6)
        G.fill_splitmix(flat, 0x5E7)
        views = [segmem[int(o):int(o) + int(n)] for o, n in zip(off, lens)]
        batch = G.SegmentBatch(views, first)
        starts, offs = torch.from_numpy(starts_h).cuda(), torch.from_numpy(offs_h).cuda()
        obj_views = [flat[int(s):int(s) + int(n)] for s, n in zip(starts_h, N)]
        obj_segs = [[views[s] for s in range(int(first[j]), int(first[j + 1])) if lens[s]] for j in range(nobj)]
        flat_pieces = [flat[int(starts_h[j] + P[s] - P[first[j]]):][:int(lens[s])]
                       for j in range(nobj) for s in range(int(first[j]), int(first[j + 1]))]
        seg_in_obj = [views[s] for j in range(nobj) for s in range(int(first[j]), int(first[j + 1]))]
        print(f"{shape}: {nobj} objects, {len(lens)} segments, {nbytes} bytes", flush=True)

        for method in args.methods:
            G.prepare(method)
            out_a = torch.zeros(nobj, dtype=G.out_dtype(method), device="cuda")
            out_b = torch.zeros_like(out_a)
            for direction in args.dirs:
                if direction == "gather":
                    def two_pass(_):
                        batch.checksum(method, out=out_a)
                        for segs, dv in zip(obj_segs, obj_views):
                            if segs:
                                torch.cat(segs, out=dv)

                    def fused(_):
                        batch.gather(method, flat, starts, out=out_b)
                    a, bn = "checksum_segments+cat", "gather_segments"
                else:
                    def two_pass(_):
                        G.checksum_offsets(method, flat, offs, out=out_a)
                        for sv, fv in zip(seg_in_obj, flat_pieces):
                            sv.copy_(fv)

                    def fused(_):
                        batch.scatter(method, flat, starts, out=out_b)
                    a, bn = "checksum_offsets+copy", "scatter_segments"
                # the fused call computes what the two passes compute and moves the same bytes
                two_pass(0)
                keep = (flat if direction == "gather" else segmem).clone()
                (flat if direction == "gather" else segmem).fill_(0xEE)
                fused(0)
                torch.cuda.synchronize()
                assert torch.equal(out_a, out_b)
                moved = flat if direction == "gather" else segmem
                if direction == "gather":
                    assert torch.equal(moved[:nbytes], keep[:nbytes])
                else:
                    for v, o, n in zip(views, off, lens):
                        assert torch.equal(v, keep[int(o):int(o) + int(n)])
                del keep
                res = ab(torch, {a: two_pass, bn: fused}, args.rounds, args.iters, 1)
                tag = f"{shape} {method} {direction}"
                for n in (a, bn):
                    res[n]["GBs_of_object_bytes_median"] = nbytes / (res[n]["median_ms"] * 1e-3) / 1e9
                    print(f"{tag:22s} {n:24s} median {res[n]['median_ms']:.4f} ms  rounds "
                          f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms", flush=True)
                band = max(res[n]["round_max_ms"] - res[n]["round_min_ms"] for n in (a, bn))
                gain = res[a]["median_ms"] - res[bn]["median_ms"]
                res["fused_vs_two_pass_pct"] = 100 * (res[bn]["median_ms"] / res[a]["median_ms"] - 1)
                res["fused_wins_beyond_spread"] = bool(gain > band)
                print(f"{tag:22s} {bn} vs {a}: {res['fused_vs_two_pass_pct']:+.2f}% in time; gain {gain:.4f} ms, "
                      f"larger spread {band:.4f} ms: {'wins' if gain > band else 'does not win'} beyond the spread",
                      flush=True)
                results[f"{shape}/{method}/{direction}"] = res
                if direction == "scatter":  # scatter rewrote the segments with flat's bytes: both sides stay defined
                    torch.cuda.synchronize()
        assert G.queue_faults() == 0
        del views, batch, segmem, flat, obj_views, obj_segs, flat_pieces, seg_in_obj
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
