"""One-process A/B of the receiver's copying entry point against what the parent
commit offers for the same job, launches interleaved ABAB on the same
buffers, each timed by its own event pair (the pattern of tools/ab_sender.py).

  A: mchecksum_gpu_unpack_messages -- verify and copy out in one pass.
  B: mchecksum_gpu_verify_messages followed by one contiguous device-to-device
     copy of the sum of the payload bytes, both inside one event pair: the
     copy is an upper bound on what any separate scatter of the payloads to
     where they are consumed can do.

Shapes: "msgs" -- bench.py --config msgs' table (C4's 262144 packets of
64..65536 bytes as messages); "4k" -- 65536 messages of 20 + 4096 bytes, R
copies of message buffer and destination used in rotation (--rotate R: cold
lines).  --shift S moves the message buffer's base by S bytes: both tables are
contiguous, so (dst - src) mod 16 steps by 4 from one message to the next and
only its residue mod 4 can be chosen -- S = 0 gives {0, 4, 8, 12} (the
destination payloads start 16-byte aligned + 4k), S = 1 the odd ones.
Every round gives one median per side; the table shows the median over rounds
and the rounds' spread (min..max of the round medians), the run-to-run band.

    python3 tools/ab_receiver.py [--shapes msgs 4k] [--shift 0 1] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ab_sender import C4_COUNT, C4_SEED, PAY, ab  # noqa: E402  (the same ABAB loop and shapes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["msgs", "4k"])
    ap.add_argument("--shift", nargs="+", type=int, default=[0, 1], help="message-buffer base shifts (bytes)")
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
        do_h = np.zeros(count + 1, dtype=np.uint64)
        do_h[1:] = np.cumsum(lens)
        npay, nmsg = int(do_h[-1]), int(mo_h[-1])
        mo, do = (torch.from_numpy(x.astype(np.int64)).cuda() for x in (mo_h, do_h))
        src = torch.empty(npay + 128, dtype=torch.uint8, device="cuda")  # the payloads the messages are packed from
        G.fill_splitmix(src, C4_SEED)
        bufs = [torch.empty(nmsg + 128, dtype=torch.uint8, device="cuda") for _ in range(ncopies)]
        dsts = [torch.full((npay + 64,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(ncopies)]
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        alg = npay + npay + 4 * count + 16 * (count + 1)
        print(f"{shape}: {count} messages, {npay} payload bytes; unpack's algorithmic bytes {alg}", flush=True)

        for shift in args.shift:
            views = [b[shift:shift + nmsg] for b in bufs]
            # sealed messages at this shift, and the check that they unpack to the source's bytes
            for v, d in zip(views, dsts):
                G.pack_messages(src[:npay], do, v, mo, status=status)
                d.fill_(0xEE)
                G.unpack_messages(v, mo, d, do, status=status, mismatches=mism)
                assert torch.equal(d[:npay], src[:npay]) and bool((d[npay:] == 0xEE).all())
            assert int(mism.item()) == 0 and int(status.sum().item()) == 0

            def pair(b):
                G.verify_messages(views[b], mo, status=status, mismatches=mism)
                # (a contiguous stand-in of the same size for the scattered payloads: the message bytes from
                # the first payload on)
                dsts[b][:npay].copy_(views[b][PAY:PAY + npay])

            sides = {"verify_messages+copy": pair,
                     "unpack_messages": lambda b: G.unpack_messages(views[b], mo, dsts[b], do, status=status,
                                                                    mismatches=mism)}
            res = ab(torch, sides, args.rounds, args.iters, ncopies)
            for n in res:
                res[n]["alg_GBs_median"] = alg / (res[n]["median_ms"] * 1e-3) / 1e9
            a, b = "verify_messages+copy", "unpack_messages"
            tag = f"{shape} +{shift}"
            for n in (a, b):
                print(f"{tag:10s} {n:22s} median {res[n]['median_ms']:.4f} ms  rounds "
                      f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms", flush=True)
            print(f"{tag:10s} {b} vs {a}: {100 * (res[b]['median_ms'] / res[a]['median_ms'] - 1):+.2f}% in time", flush=True)
            results[f"{shape}/unpack/shift{shift}"] = res
            torch.cuda.synchronize()
            assert int(mism.item()) == 0 and int(status.sum().item()) == 0
        assert G.queue_faults() == 0
        del src, bufs, dsts
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
