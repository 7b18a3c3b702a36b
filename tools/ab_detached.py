"""One-process A/B of the overflow-RPC entry points against what the parent
commit offers for the same job, launches interleaved, each timed by its own
event pair (the pattern of tools/ab_sender.py).

  verify:  mchecksum_gpu_verify_detached_messages (B) against a device gather +
           byte swap of the header slots into an `expected` table (torch ops on
           the same stream) followed by mchecksum_gpu_verify_offsets (A); and
           verify_offsets alone on a ready table (A0), the floor the fused call
           is held to.
  seal:    mchecksum_gpu_seal_detached_messages (B) against
           mchecksum_gpu_checksum_offsets + a scatter of the swapped values
           into the slots (A); checksum_offsets alone (A0).
  stream:  mchecksum_gpu_state_verify_messages (B) against state_get + the
           gather + a compare and count in torch (A).

Shapes: 8192 x 1 MiB and 65536 x 64 KiB payloads, 52-byte eager messages with
the hash slot at 16.  Every round gives one median per side; the table shows
the median over rounds and the rounds' spread (min..max of the round medians).

    python3 tools/ab_detached.py [--shapes 1m 64k] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x4D43310000000015
MSG, HASH = 52, 16
SHAPES = {"1m": (8192, 1 << 20), "64k": (65536, 64 << 10)}


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
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1m", "64k"], choices=sorted(SHAPES))
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

    def show(tag, res, base):
        for n in res:
            rel = "" if n == base else f"  {100 * (res[n]['median_ms'] / res[base]['median_ms'] - 1):+.2f}% vs {base}"
            print(f"{tag:12s} {n:34s} median {res[n]['median_ms']:.4f} ms  rounds "
                  f"{res[n]['round_min_ms']:.4f}..{res[n]['round_max_ms']:.4f} ms{rel}", flush=True)

    for shape in args.shapes:
        count, length = SHAPES[shape]
        po = torch.arange(count + 1, dtype=torch.int64, device="cuda") * length
        mo = torch.arange(count + 1, dtype=torch.int64, device="cuda") * MSG
        pay = torch.empty(count * length + 64, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(pay, SEED)
        msgs = torch.empty(count * MSG, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(msgs, SEED + 1)
        idx = (mo[:-1, None] + HASH + torch.arange(4, device="cuda")[None, :]).contiguous()  # the slots' bytes
        status = torch.ones(count, dtype=torch.uint8, device="cuda")
        mism = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.empty(count, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        print(f"{shape}: {count} payloads of {length} bytes, {MSG}-byte eager messages", flush=True)

        def gather():  # the slots, network order, as the host-order table verify_offsets wants
            w = msgs[idx].to(torch.int32)
            return (w[:, 0] << 24) | (w[:, 1] << 16) | (w[:, 2] << 8) | w[:, 3]

        def scatter():  # checksum_offsets' values into the slots, network order (the host is little-endian)
            msgs[idx] = out.view(torch.uint8).view(count, 4).flip(1)

        def verify_offsets(expected):
            rc = L.mchecksum_gpu_verify_offsets(b"crc32c", pay.data_ptr(), po.data_ptr(), count, expected.data_ptr(),
                                                status.data_ptr(), mism.data_ptr(), s)
            assert rc == 0

        # seal once, and check the two routes agree before timing them
        G.seal_detached_messages(msgs, mo, pay, po, hash_offset=HASH, status=status)
        sealed = msgs.clone()
        ready = gather().contiguous()
        verify_offsets(ready)
        G.verify_detached_messages(msgs, mo, pay, po, hash_offset=HASH, status=status, mismatches=mism)
        G.checksum_offsets("crc32c", pay, po, out=out)
        scatter()
        torch.cuda.synchronize()
        assert int(mism.item()) == 0 and int(status.sum().item()) == 0 and torch.equal(msgs, sealed)

        sides = {"gather+swap+verify_offsets": lambda: verify_offsets(gather().contiguous()),
                 "verify_offsets alone": lambda: verify_offsets(ready),
                 "verify_detached_messages": lambda: G.verify_detached_messages(msgs, mo, pay, po, hash_offset=HASH,
                                                                                 status=status, mismatches=mism)}
        res = ab(torch, sides, args.rounds, args.iters)
        show(f"{shape} verify", res, "verify_offsets alone")
        results[f"{shape}/verify"] = res

        def two_call_seal():
            G.checksum_offsets("crc32c", pay, po, out=out)
            scatter()

        sides = {"checksum_offsets+swap+scatter": two_call_seal,
                 "checksum_offsets alone": lambda: G.checksum_offsets("crc32c", pay, po, out=out),
                 "seal_detached_messages": lambda: G.seal_detached_messages(msgs, mo, pay, po, hash_offset=HASH,
                                                                             status=status)}
        res = ab(torch, sides, args.rounds, args.iters)
        show(f"{shape} seal", res, "checksum_offsets alone")
        results[f"{shape}/seal"] = res

        # the streaming end: states that have seen every payload
        state = G.state_init("crc32c", count)
        G.update_offsets("crc32c", pay, po, state)
        bad = torch.empty(count, dtype=torch.bool, device="cuda")

        def get_gather_compare():
            G.state_get("crc32c", state, out=out)
            torch.ne(out, gather(), out=bad)
            return bad.sum()

        sides = {"state_get+gather+compare": get_gather_compare,
                 "state_verify_messages": lambda: G.state_verify_messages(state, msgs, mo, hash_offset=HASH, status=status,
                                                                          mismatches=mism)}
        assert int(get_gather_compare().item()) == 0
        res = ab(torch, sides, args.rounds, args.iters)
        show(f"{shape} stream", res, "state_get+gather+compare")
        results[f"{shape}/stream"] = res
        torch.cuda.synchronize()
        assert int(mism.item()) == 0 and int(status.sum().item()) == 0 and torch.equal(msgs, sealed)
        assert G.queue_faults() == 0
        del pay, msgs, sealed
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
