"""One-process A/B of the per-field message calls against the two calls each
replaces over the same tables, launches interleaved ABAB on the same buffers,
each side timed by its own event pair (the loop of tools/ab_sender.py, the
method of tools/ab_seg_copy.py).  The baselines are the parent commit's calls:

  pack     A: SegmentBatch.gather into the message buffer, then seal_messages.
           B: SegmentBatch.pack_messages.
  unpack   A: verify_messages, then SegmentBatch.scatter.
           B: SegmentBatch.unpack_messages.

Shapes: "64k" -- 8192 messages of 64 KiB in 4 equal segments at 16-byte aligned
addresses; "4k" -- 65536 messages of 4 KiB in 3 fields of unequal length (24,
1000 and 3072 bytes) at odd addresses.  Every round gives one median per side;
the table shows the median over rounds and the rounds' spread (min..max of the
round medians), and says whether the fused call wins by more than the larger
spread.

    python3 tools/ab_seg_messages.py [--shapes 64k 4k] [--dirs pack unpack] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ab_sender import ab  # noqa: E402  (the same ABAB loop)

PAY, HOFF = 20, 16
SHAPES = {"64k": (8192, [16384] * 4, 16), "4k": (65536, [24, 1000, 3072], 1)}  # messages, fields, address step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["64k", "4k"])
    ap.add_argument("--dirs", nargs="+", default=["pack", "unpack"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=6, help="A/B pairs per round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from mercury_amd import gpu as G
    G.prepare("crc32c")
    results = {}
    for shape in args.shapes:
        nobj, fields, step = SHAPES[shape]
        per = len(fields)
        lens = np.tile(np.asarray(fields, dtype=np.int64), nobj)
        first = np.arange(0, nobj * per + 1, per)
        # segments one after another; step 1: a gap that leaves every one at an odd address
        at, pos = np.zeros(len(lens), dtype=np.int64), 1 if step == 1 else 0
        for i, n in enumerate(lens):
            at[i] = pos
            pos += int(n)
            pos += (1 - pos % 2) if step == 1 else 0
        n_obj = int(sum(fields))
        off_h = (7 + np.arange(nobj + 1, dtype=np.int64) * (PAY + n_obj))
        nbytes = nobj * n_obj
        segmem = torch.empty(pos + 128, dtype=torch.uint8, device="cuda")
        buf = torch.empty(int(off_h[-1]) + 128, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(segmem, 0x5E8)
        buf.fill_(0xEE)
        views = [segmem[int(o):int(o) + int(n)] for o, n in zip(at, lens)]
        batch = G.SegmentBatch(views, first)
        off = torch.from_numpy(off_h).cuda()
        starts = torch.from_numpy(off_h[:-1] + PAY).cuda()
        out = torch.zeros(nobj, dtype=G.out_dtype("crc32c"), device="cuda")
        st_a = torch.ones(nobj, dtype=torch.uint8, device="cuda")
        st_b = torch.ones(nobj, dtype=torch.uint8, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        print(f"{shape}: {nobj} messages, {len(lens)} segments, {nbytes} payload bytes", flush=True)
        for direction in args.dirs:
            if direction == "pack":
                def two_calls(_):
                    batch.gather("crc32c", buf, starts, out=out)
                    G.seal_messages(buf, off, PAY, HOFF, status=st_a)

                def fused(_):
                    batch.pack_messages(buf, off, PAY, HOFF, status=st_b)
                a, bn = "gather_segments+seal_messages", "pack_segment_messages"
            else:
                def two_calls(_):
                    G.verify_messages(buf, off, PAY, HOFF, status=st_a, mismatches=mism)
                    batch.scatter("crc32c", buf, starts, out=out)

                def fused(_):
                    batch.unpack_messages(buf, off, PAY, HOFF, status=st_b, mismatches=mism)
                a, bn = "verify_messages+scatter_segments", "unpack_segment_messages"
            # both routes leave the same bytes and verdicts (unpack runs on what pack sealed)
            moved = buf if direction == "pack" else segmem
            if direction == "unpack":
                batch.pack_messages(buf, off, PAY, HOFF, status=st_b)
                ref = segmem.clone()
            two_calls(0)
            keep = moved.clone()
            moved.fill_(0xEE) if direction == "pack" else moved.zero_()
            fused(0)
            torch.cuda.synchronize()
            assert torch.equal(moved, keep) if direction == "pack" else all(
                torch.equal(v, ref[int(o):int(o) + int(n)]) for v, o, n in list(zip(views, at, lens))[:4096])
            assert int(st_a.sum().item()) == 0 and int(st_b.sum().item()) == 0
            del keep
            mism.zero_()
            res = ab(torch, {a: two_calls, bn: fused}, args.rounds, args.iters, 1)
            assert int(mism.item()) == 0
            tag = f"{shape} {direction}"
            for n in (a, bn):
                res[n]["GBs_of_payload_bytes_median"] = nbytes / (res[n]["median_ms"] * 1e-3) / 1e9
                print(f"{tag:12s} {n:34s} median {res[n]['median_ms']:.4f} ms  rounds "
                      f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms", flush=True)
            band = max(res[n]["round_max_ms"] - res[n]["round_min_ms"] for n in (a, bn))
            gain = res[a]["median_ms"] - res[bn]["median_ms"]
            res["fused_vs_two_calls_pct"] = 100 * (res[bn]["median_ms"] / res[a]["median_ms"] - 1)
            res["fused_wins_beyond_spread"] = bool(gain > band)
            print(f"{tag:12s} {bn} vs {a}: {res['fused_vs_two_calls_pct']:+.2f}% in time; gain {gain:.4f} ms, "
                  f"larger spread {band:.4f} ms: {'wins' if gain > band else 'does not win'} beyond the spread",
                  flush=True)
            results[f"{shape}/{direction}"] = res
        assert G.queue_faults() == 0
        del views, batch, segmem, buf
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
