#!/usr/bin/env python3
"""A/B of the streaming and verifying segment calls against the parent's calls
they extend, both libraries in ONE process, interleaved round by round
(`make prev` builds build/variants/libmchecksum_prev.so and _cur.so):

  hash      prev checksum_segments | cur checksum_segments, update_segments, verify_segments
  gather    prev gather_segments   | cur gather_segments, update_gather_segments
  scatter   prev scatter_segments  | cur scatter_segments, update_scatter_segments
  pipeline  a three-stage transfer (the same list three times):
            prev: three checksum_segments into stage-major value arrays, then
                  two mchecksum_gpu_combine calls (combine_runs wants each
                  object's values side by side, which per-stage calls do not
                  write; the length table is prepared outside the timed part)
            cur:  three update_segments, then one state_verify

Shapes: bench.py's seg layout (--count objects of 1 MiB in 4 segments) and the
ragged list of tools/ab_seg_copy.py.  Each round gives one median per side;
the table shows the median over rounds and the rounds' spread, and says
whether a side lies inside the parent's own min..max range.

    python3 tools/ab_seg_stream.py [--shapes seg ragged] [--methods crc32c crc64] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_variants import ragged_segments  # noqa: E402
from mercury_amd import gpu as G  # noqa: E402


def load(name):
    L = ctypes.CDLL(os.path.join(ROOT, "build", "variants", f"libmchecksum_{name}.so"))
    c = ctypes
    seg = [c.c_char_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t]
    tail = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    L.mchecksum_gpu_prepare.argtypes = [c.c_char_p]
    for n, a in (("checksum_segments", seg + tail), ("update_segments", seg + tail),
                 ("gather_segments", seg + [c.c_void_p, c.c_void_p] + tail),
                 ("update_gather_segments", seg + [c.c_void_p, c.c_void_p] + tail),
                 ("scatter_segments", [c.c_char_p, c.c_void_p, c.c_void_p] + seg[1:] + tail),
                 ("update_scatter_segments", [c.c_char_p, c.c_void_p, c.c_void_p] + seg[1:] + tail),
                 ("verify_segments", seg + [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]),
                 ("state_verify", [c.c_char_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]),
                 ("state_init", [c.c_char_p, c.c_void_p, c.c_size_t, c.c_void_p]),
                 ("combine", [c.c_char_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p])):
        f = getattr(L, "mchecksum_gpu_" + n, None)
        if f is not None:
            f.argtypes = a
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["seg", "ragged"])
    ap.add_argument("--methods", nargs="+", default=["crc32c", "crc64"])
    ap.add_argument("--count", type=int, default=8192, help="objects of the seg shape")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    prev, cur = load("prev"), load("cur")
    results = {}
    for shape in args.shapes:
        if shape == "seg":
            from mercury_amd.workload import segment_slots
            seed, slen = 0x4D43310000000003, (1 << 20) // 4
            data = torch.empty((args.count << 20) + 64, dtype=torch.uint8, device="cuda")
            slots = segment_slots(seed, args.count * 4)
            views = [data[int(q) * slen:(int(q) + 1) * slen] for q in slots]
            first = np.arange(0, args.count * 4 + 1, 4)
            sizes = np.full(args.count, 1 << 20, dtype=np.int64)
        else:
            seed = 0x5E6
            lens, off, first, span = ragged_segments(seed)
            data = torch.empty(span + 128, dtype=torch.uint8, device="cuda")
            views = [data[int(o):int(o) + int(n)] for o, n in zip(off, lens)]
            P = np.concatenate([[0], np.cumsum(lens)])
            sizes = P[first[1:]] - P[first[:-1]]
        G.fill_splitmix(data, seed)
        nbytes = int(sizes.sum())
        seg = G.SegmentBatch(views, first)
        nobj, ns, mb = seg.nobj, seg.nseg, seg.meta.data_ptr()
        flat = torch.empty(nbytes + 128, dtype=torch.uint8, device="cuda")
        G.fill_splitmix(flat, seed + 1)
        starts = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)).cuda()
        sizes_d = torch.from_numpy(sizes.astype(np.int64)).cuda()
        stream = torch.cuda.current_stream()
        h = stream.cuda_stream
        tables = (mb, mb + 8 * ns, ns, mb + 16 * ns, nobj)
        work = (seg.work.data_ptr(), seg.work.numel() * 8)
        print(f"{shape}: {nobj} objects, {ns} segments, {nbytes} bytes", flush=True)
        for method in args.methods:
            m = method.encode()
            assert prev.mchecksum_gpu_prepare(m) == 0 and cur.mchecksum_gpu_prepare(m) == 0
            dt = G.out_dtype(method)
            out = torch.zeros(3 * nobj, dtype=dt, device="cuda")
            state = torch.zeros(nobj, dtype=dt, device="cuda")
            status = torch.zeros(nobj, dtype=torch.uint8, device="cuda")
            mism = torch.zeros(1, dtype=torch.int32, device="cuda")
            expect = seg.checksum(method).clone()
            flat_expect = G.checksum_offsets(method, flat, torch.cat([starts, starts[-1:] + sizes_d[-1:]])).clone()
            three = G.state_init(method, nobj)
            for _ in range(3):
                seg.update(method, three)
            expect3 = G.state_get(method, three).clone()
            torch.cuda.synchronize()
            o, st = out.data_ptr(), state.data_ptr()
            es = out.element_size()
            fl, sp = flat.data_ptr(), starts.data_ptr()

            def ok(rc):
                assert rc == 0

            sides = {
                "hash": {
                    "prev checksum": lambda: ok(prev.mchecksum_gpu_checksum_segments(m, *tables, *work, o, h)),
                    "cur checksum": lambda: ok(cur.mchecksum_gpu_checksum_segments(m, *tables, *work, o, h)),
                    "cur update": lambda: ok(cur.mchecksum_gpu_update_segments(m, *tables, *work, st, h)),
                    "cur verify": lambda: ok(cur.mchecksum_gpu_verify_segments(m, *tables, *work, expect.data_ptr(),
                                                                               status.data_ptr(), mism.data_ptr(), h)),
                },
                "gather": {
                    "prev gather": lambda: ok(prev.mchecksum_gpu_gather_segments(m, *tables, fl, sp, *work, o, h)),
                    "cur gather": lambda: ok(cur.mchecksum_gpu_gather_segments(m, *tables, fl, sp, *work, o, h)),
                    "cur update_gather": lambda: ok(cur.mchecksum_gpu_update_gather_segments(m, *tables, fl, sp, *work,
                                                                                             st, h)),
                },
                "scatter": {
                    "prev scatter": lambda: ok(prev.mchecksum_gpu_scatter_segments(m, fl, sp, *tables, *work, o, h)),
                    "cur scatter": lambda: ok(cur.mchecksum_gpu_scatter_segments(m, fl, sp, *tables, *work, o, h)),
                    "cur update_scatter": lambda: ok(cur.mchecksum_gpu_update_scatter_segments(m, fl, sp, *tables,
                                                                                               *work, st, h)),
                },
            }

            def pipe_prev():
                for k in range(3):
                    ok(prev.mchecksum_gpu_checksum_segments(m, *tables, *work, o + k * nobj * es, h))
                ok(prev.mchecksum_gpu_combine(m, o, o + nobj * es, sizes_d.data_ptr(), nobj, o, h))
                ok(prev.mchecksum_gpu_combine(m, o, o + 2 * nobj * es, sizes_d.data_ptr(), nobj, o, h))

            def pipe_cur():
                ok(cur.mchecksum_gpu_state_init(m, st, nobj, h))
                for _ in range(3):
                    ok(cur.mchecksum_gpu_update_segments(m, *tables, *work, st, h))
                ok(cur.mchecksum_gpu_state_verify(m, st, nobj, expect3.data_ptr(), status.data_ptr(), mism.data_ptr(), h))

            sides["pipeline"] = {"prev 3 checksum + 2 combine": pipe_prev,
                                 "cur state_init + 3 update + state_verify": pipe_cur}
            # what each side computes, once, before anything is timed
            pipe_prev()
            torch.cuda.synchronize()
            assert torch.equal(out[:nobj], expect3), "the parent's pipeline and the streamed one differ"
            mism.zero_()
            pipe_cur()
            sides["hash"]["cur verify"]()
            torch.cuda.synchronize()
            assert int(mism.item()) == 0 and int(status.sum().item()) == 0
            sides["scatter"]["cur scatter"]()  # the segments now hold flat's bytes: both copy directions stay defined
            torch.cuda.synchronize()
            assert torch.equal(out[:nobj], flat_expect)
            expect = seg.checksum(method).clone()
            torch.cuda.synchronize()

            for group, fns in sides.items():
                times = {n: [] for n in fns}
                for r in range(args.rounds + 1):
                    for n, fn in fns.items():
                        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                               for _ in range(args.iters)]
                        for a, b in evs:
                            a.record(stream)
                            fn()
                            b.record(stream)
                        torch.cuda.synchronize()
                        if r > 0:  # round 0 = warm-up
                            times[n].append(float(np.median([a.elapsed_time(b) for a, b in evs])))
                res = {n: {"median_of_rounds_ms": float(np.median(t)), "round_min_ms": min(t), "round_max_ms": max(t)}
                       for n, t in times.items()}
                base = next(iter(res.values()))  # the parent's side comes first
                for n, v in res.items():
                    v["inside_parent_range"] = bool(base["round_min_ms"] <= v["median_of_rounds_ms"] <= base["round_max_ms"])
                    print(f"{shape:6s} {method:7s} {group:8s} {n:42s} {v['median_of_rounds_ms']:.4f} ms  rounds "
                          f"{v['round_min_ms']:.4f}..{v['round_max_ms']:.4f}  "
                          f"{'inside' if v['inside_parent_range'] else 'OUTSIDE'} the parent's range", flush=True)
                results[f"{shape}/{method}/{group}"] = res
            assert G.queue_faults() == 0
        del views, seg, data, flat
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
