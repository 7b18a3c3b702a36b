// mchecksum_gpu_ext.hip -- MI355X batch entry points next to the payload CRC
// (declared in include/mchecksum_gpu.h):
//
//  * mchecksum_gpu_checksum_segments -- the CRC of scatter-gather objects: a
//    bulk handle's segments (HG_Bulk_create(count, buf_ptrs, buf_sizes),
//    src/mercury_bulk.h:55,79) registered as device memory (hg_bulk_attr
//    mem_type HG_MEM_TYPE_ROCM, src/mercury_types.h:38,44-47), hashed as the
//    concatenation of its segments in order.  Mercury never checksums bulk
//    data today (src/mercury_core_types.h:68-69); this is what a receiver
//    would call to check a device-resident bulk transfer in one launch.
//  * mchecksum_gpu_verify_core_headers -- the CRC16 check of Mercury core
//    headers (hg_core_header_request_proc / _response_proc,
//    src/mercury_core_header.c:175-289) for a batch of received messages that
//    already sit in device memory.
//  * mchecksum_gpu_checksum_xdr -- the proc checksum of messages serialized in
//    XDR mode (HG_HAS_XDR, src/mercury_proc.h:110-122,147-160), where the
//    buffer holds big-endian, 4-byte-rounded XDR but the checksum covers the
//    host-order field values: a per-field schema says how to undo the XDR.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <type_traits>

#include "crc_gpu_device.h"
#include "gpu_host.h"
#include "launch_plan.h"
#include "mchecksum_gpu.h"
#include "mchecksum_models.h"
#include "seg_plan.h"

namespace {

// ------------------------------------------------------------ segments ----
//
// Object j = the concatenation of segments [first[j], first[j+1]).  By
// linearity (register form, crc_gpu_layout.h):
//   CRC(object) = Z^N(init) ^ XOR_c Z^(after_c)(L(chunk_c)) ^ xorout
// where chunks of at most kSegChunk bytes (seg_plan.h) tile every segment, L is the CRC with
// zero init and no finalisation, N is the object's byte count and after_c the
// number of object bytes that follow chunk c.  Short scan launches write the
// segment lengths' byte and chunk prefix sums (caller's workspace) and preset
// out[j] = init ^ xorout (the CRC of an empty object); then persistent waves
// take chunks, compute L on 64 lanes with the payload kernels' step loop,
// shift it by after_c (at most 12 table-operator applications, base-16
// digits) and XOR it into out[j] with an atomic -- XOR commutes, so the value
// is deterministic.  The chunk that starts its object (object offset 0) runs
// its step loop from the register `init` instead of 0 (R(init, M) =
// R(0, M ^ init): init rides in its first W/8 bytes, or Z^n(init) is added
// for a chunk shorter than that) and XORs init once more, cancelling the
// preset's: Z^after(Z^n(init)) = Z^N(init), so the object term costs nothing
// (round 3 added it in a launch of its own: ~6 us per call, plus a kernel
// boundary).
//
// 256 KiB chunks: enough of them to fill the chip from a single GiB-sized
// segment, while the shift (a few us of dependent scalar loads) stays a few
// percent of a chunk's scan time.  A chunk that ends its object needs no shift.
//
// seg_plan.h is the one home of the passes' arithmetic: the chunk size, the
// workspace's layout (seg_work_layout; the host fills SegWork from it, and
// both kernels' arguments carry that one struct), and the chunk record
// (SegChunk) with every rule and guard that fills it.  This file keeps the
// loads, the payload loops and the launches.
using mck::kDescWords;
using mck::kNoObj;
using mck::kScanBlk;
using mck::kScanPer;
using mck::kScanThreads;
using mck::kSegChunk;
using mck::seg_chunk_count;
using mck::SegChunk;
using mck::SegWork;

struct SegArgs {
    const uint64_t *addr, *len;
    uint64_t nseg;
    const uint64_t *first;
    uint64_t nobj;
    // the workspace (seg_plan.h).  Per segment s its object record is {its
    // object j (kNoObj outside [first[0], first[nobj])), first[j], first[j +
    // 1], the object's head segment (its first non-empty one; kNoObj when the
    // scan block could not tell)}: 4 words, one scalar load in the queue pass.
    // map_cap: the part of the map this call uses (0: the pass searches C).
    SegWork w;
    void *out;
    const void *pack, *shift;
    // work-queue slot of the chunk passes (crc_gpu_queue.h, WgQueue; nullptr:
    // static split) and the caller's fail-closed word
    unsigned long long *queue;
    uint32_t *err_word;
    // the call's look-back epoch (scan_key; scan_gave_up)
    uint64_t epoch;
};

// Exclusive prefix sums of segment bytes (P) and chunk counts (C), each
// segment's object, the chunk -> segment map and the ragged flag, in ONE
// launch over scan blocks of kScanBlk segments (round 4; one workgroup
// streams only ~20 GB/s, so a single-workgroup scan of 32768 segments took
// 48 us).  A block scans its own segments, publishes its aggregate, and finds
// its offset by a decoupled look-back over the blocks before it: one wave
// reads 64 predecessors' descriptors at once and sums aggregates back to the
// nearest published inclusive prefix, then publishes its own inclusive prefix.
// Descriptors carry the call's tag: its key -- scan_key(epoch, gen), the epoch
// a process-wide counter from a random seed, gen the workspace's count of
// scans -- above the 2 state bits.  A workspace left by an earlier call needs
// no clearing, and neither does one left by an earlier replay of the same
// captured call: a graph replays the epoch it captured, so the epoch alone
// would let block b take block b - 1's inclusive prefix of the LAST replay
// (state 2, same epoch) for this one's whenever b looks back before b - 1 has
// published -- right only while the lengths never change.  gen differs: every
// block reads it before its first flag store (the release orders the read
// first), and the last block bumps it only after its look-back, which ends at
// an inclusive prefix carrying this call's tag and so, by induction down to
// block 0, after every block of the call has published -- hence read gen.
// All blocks of a call therefore read the same gen, calls on one workspace
// are serialized (header), so each call's gen is its predecessor's + 1, and
// two tags of one epoch are equal only 2^62 scans apart.  The wait
// depends only on blocks dispatched before this one (a kernel's workgroups
// are dispatched in order and run to completion), and is bounded: a give-up
// is counted as a queue fault and reported on the caller's error word.
// The totals also flag segments whose chunks cannot all take the aligned loop
// (start not 16-B aligned or length not a multiple of 1 KiB).  The same
// launch presets out[j] = init ^ xorout.  Round 3 ran this as a block-reduce
// launch and a block-offset launch (4.8 + 8.5 us at 32768 segments, beside a
// kernel boundary), round 2 as three.  (1 or 2 segments per scan thread --
// 4x / 2x the scan blocks -- measured +-0.1% on the bench's 32768-segment
// lists, profiles/r05/scan_per/.)
// (kScanThreads, kScanPer, kScanBlk and the descriptors' kDescWords: seg_plan.h)

// Block-wide inclusive scan of (p, c) over the first 256 threads (a wider
// block's other threads only take part in the barrier); returns the block
// totals through *tp, *tc.
__device__ __forceinline__ void block_scan2(uint64_t &p, uint64_t &c, uint64_t *tp, uint64_t *tc) {
    __shared__ uint64_t wp[4], wc[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (w < kScanThreads / 64) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t op = __shfl_up(p, d, 64), oc = __shfl_up(c, d, 64);
            if (lane >= (uint32_t)d) {
                p += op;
                c += oc;
            }
        }
        if (lane == 63) {
            wp[w] = p;
            wc[w] = c;
        }
    }
    __syncthreads();
    if (w >= kScanThreads / 64) return;
    uint64_t bp = 0, bc = 0, sp = 0, sc = 0;
#pragma unroll
    for (uint32_t v = 0; v < kScanThreads / 64; v++) {
        if (v < w) {
            bp += wp[v];
            bc += wc[v];
        }
        sp += wp[v];
        sc += wc[v];
    }
    p += bp;
    c += bc;
    *tp = sp;
    *tc = sc;
}

// One wave: the largest index j < n with a[j] <= key (a sorted ascending,
// a[0] <= key), by 64-ary narrowing: each round probes 64 evenly spaced
// entries at once (3 rounds of loads for n = 8193 instead of 13 dependent ones).
__device__ __forceinline__ uint64_t wave_last_le(const uint64_t *a, uint64_t n, uint64_t key, uint32_t lane) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t idx = lo + (uint64_t)lane * step;
        const unsigned long long m = __ballot(idx < hi && a[idx] <= key);
        const uint64_t L = 63u - (uint32_t)__builtin_clzll(m);  // lane 0 (a[lo] <= key) is always set
        lo += L * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return lo;
}

// (readfirstlane returns int: cast through uint32_t so nothing sign-extends)
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform(uint64_t v) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t ld_relaxed(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(uint64_t *p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Wave 0 of block b: publish (tp, tc, tr), look back, publish the inclusive
// prefix; returns the exclusive prefix (bytes, chunks, ragged) in every lane.
// tag: the call's key above the two state bits (scan_block).  false: the
// bounded wait gave up (fault counted).
__device__ __forceinline__ bool seg_lookback(uint64_t *desc, uint64_t b, uint64_t tag, uint64_t tp, uint64_t tc,
                                             uint64_t tr, uint32_t lane, uint64_t *ep, uint64_t *ec, uint64_t *er,
                                             uint64_t fault_block) {
    uint64_t *me = desc + kDescWords * b;
#if MCK_QFAULT_TEST
    // injected stall (MCHECKSUM_GPU_QFAULT_MODE=scanstall): this block never
    // publishes, so every later block waits out its deadline
    const bool mute = (g_mck_qfault_mode & 2u) && b == fault_block;
#else
    constexpr bool mute = false;
#endif
    if (lane == 0 && !mute) {
        st_relaxed(me + 1, tp);
        st_relaxed(me + 2, tc);
        st_relaxed(me + 3, tr);
        if (b == 0) {
            st_relaxed(me + 4, tp);
            st_relaxed(me + 5, tc);
            st_relaxed(me + 6, tr);
        }
        __hip_atomic_store(me, tag | (b == 0 ? 2u : 1u), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint64_t sp = 0, sc = 0, sr = 0;
    bool ok = true;
    if (b > 0) {
        int64_t k = (int64_t)b - 1;  // window: blocks k, k - 1, ..., k - 63 (lane order)
        Deadline dl;  // 1 s of real time (crc_gpu_queue.h)
        for (;;) {
#if MCK_QFAULT_TEST
            if (b == fault_block && g_mck_qfault_mode == 0u) {  // injected give-up (test builds, MCHECKSUM_GPU_QFAULT_SCAN)
                if (lane == 0) queue_fault(11, b, 0);
                ok = false;
                break;
            }
#else
            (void)fault_block;
#endif
            const int64_t idx = k - (int64_t)lane;
            // (the lanes past block 0 present this call's own tag: an inclusive prefix of 0)
            const uint64_t f = idx >= 0 ? ld_relaxed(desc + kDescWords * (uint64_t)idx) : tag | 2u;
            const uint32_t state = (f & ~3ull) == tag ? (uint32_t)(f & 3u) : 0u;
            const unsigned long long incl = __ballot(state == 2), none = __ballot(state == 0);
            const uint32_t S = incl ? (uint32_t)__builtin_ctzll(incl) : 64u;  // nearest inclusive prefix
            const unsigned long long below = S >= 64 ? ~0ull : ((1ull << S) - 1);
            if (none & below) {  // a nearer block has not published yet
                __builtin_amdgcn_s_sleep(1);
                if (dl.passed()) {
                    if (lane == 0) queue_fault(10, b, (uint64_t)k);
                    ok = false;
                    break;
                }
                continue;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            uint64_t vp = 0, vc = 0, vr = 0;
            if (idx >= 0 && lane <= S) {
                const uint64_t *d = desc + kDescWords * (uint64_t)idx + (lane == S ? 4 : 1);
                vp = ld_relaxed(d);
                vc = ld_relaxed(d + 1);
                vr = ld_relaxed(d + 2);
            }
            sp += wave_sum(vp);
            sc += wave_sum(vc);
            sr |= wave_sum(vr);
            if (S < 64) break;
            k -= 64;
        }
        if (lane == 0 && !mute) {
            st_relaxed(me + 4, sp + tp);
            st_relaxed(me + 5, sc + tc);
            st_relaxed(me + 6, sr | tr);
            __hip_atomic_store(me, tag | 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    *ep = sp;
    *ec = sc;
    *er = sr ? 1u : 0u;
    return ok;
}

// Each segment's object (obj, the queue pass's map) without a per-segment
// search: waves 1 and 2 find the objects of the block's first and last
// segments (wave_last_le over first[]); a thread per object in between writes
// the object's index and bounds over its segments in LDS rows of the block
// (empty objects write nothing, so a segment gets the last object whose range
// starts at or before it), and every thread then reads its own segments'
// entries.  Round 3 ran a binary search over all of first[] in global memory
// per segment: ~14 dependent loads, 15 of the pass's 17 us at 32768 segments.
// The scan's arguments.
struct ScanArgs {
    const uint64_t *len, *addr;
    uint64_t nseg;
    uint64_t epoch;
    const uint64_t *first;
    uint64_t nobj;
    SegWork w;  // the workspace, as the chunk pass gets it; obj nullptr: no object records (CRC-32C)
    void *out;
    uint32_t width;
    uint64_t preset;
    uint32_t *err_word;
    uint64_t fault_block;
};
// The scan is the workspace's one writer: its view of the same regions, and
// the one place where they become writable.
using ScanWork = mck::SegWorkT<uint64_t, uint32_t>;
__device__ __forceinline__ ScanWork scan_work(const SegWork &w) { return __builtin_bit_cast(ScanWork, w); }
// A call's key: its epoch and the workspace's call count.  A graph replays
// its captured epoch, so the epoch alone cannot tell two replays apart
// (ADVICE r5); the count moves on every scan, captured or not.
__device__ __forceinline__ uint64_t scan_key(uint64_t epoch, uint64_t gen) {
    return epoch ^ (gen * 0x9E3779B97F4A7C15ull) ^ 0xD1B54A32D192ED03ull;
}
// A call's scan-side give-ups (a look-back in any scan block) add 1 to the
// error word between them, as the header promises per call: the first to
// swap the call's key into the claim word reports, the rest see it already
// there -- and the chunk pass, seeing it, hashes nothing (fail closed, and
// no second deadline in the same call).
__device__ __forceinline__ void report_scan_fault(const ScanArgs &sa, const ScanWork &ws, uint64_t gen) {
    const uint64_t key = scan_key(sa.epoch, gen);
    const uint64_t was = __hip_atomic_exchange(ws.fault_claim, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (was != key && sa.err_word) atomicAdd(sa.err_word, 1u);
}
// LDS scratch of one scan block: the object rows of its segments (4 x u64 +
// u32 each) and a few broadcast words
constexpr uint32_t kScanScratch = kScanBlk * (4 * 8 + 4) + 64;

// Scan block b of nb (kScanThreads threads).
__device__ __forceinline__ void scan_block(const ScanArgs &sa, uint64_t b, uint64_t nb, uint8_t *scratch) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const bool act = tid < kScanThreads;
    const uint64_t nseg = sa.nseg, nobj = sa.nobj;
    const ScanWork ws = scan_work(sa.w);
    const uint64_t s0 = b * kScanBlk, s1 = s0 + kScanBlk < nseg ? s0 + kScanBlk : nseg;
    uint64_t *row = reinterpret_cast<uint64_t *>(scratch);
    uint64_t *row_f0 = row + kScanBlk, *row_f1 = row_f0 + kScanBlk;  // the object's first[j], first[j + 1]
    uint64_t *row_hs = row_f1 + kScanBlk;                             // the object's head segment
    uint32_t *row_ne = reinterpret_cast<uint32_t *>(row_hs + kScanBlk);  // 1: the segment is not empty
    uint64_t *bc = reinterpret_cast<uint64_t *>(row_ne + kScanBlk);     // jb, je, ex[3]
    uint32_t *rag = reinterpret_cast<uint32_t *>(bc + 5);
    // every object starts as the CRC of the empty message (the chunk passes XOR
    // into it); an update or verify call (no out here) presets its words after
    // the scan, when the objects' byte totals are known (seg_pre_kernel)
    if (act && sa.out)
        for (uint64_t j = b * kScanThreads + tid; j < nobj; j += nb * kScanThreads) {
            if (sa.width == 64) reinterpret_cast<uint64_t *>(sa.out)[j] = sa.preset;
            else reinterpret_cast<uint32_t *>(sa.out)[j] = (uint32_t)sa.preset;
        }
    uint64_t l[kScanPer], p = 0, c = 0, r = 0;
#pragma unroll
    for (uint32_t e = 0; e < kScanPer; e++) {
        const uint64_t i = s0 + tid * kScanPer + e;
        l[e] = act && i < nseg ? sa.len[i] : 0;
        p += l[e];
        c += seg_chunk_count(l[e]);
        r |= act && i < nseg && l[e] && (l[e] % 1024 != 0 || sa.addr[i] % 16 != 0);
    }
    // the objects touching this block (queue pass only)
    const uint64_t f0 = sa.first[0], f1 = sa.first[nobj];
    const uint64_t lo_s = s0 > f0 ? s0 : f0, hi_s = s1 < f1 ? s1 : f1;
    if (ws.obj && lo_s < hi_s) {
        if (w == 1) {
            const uint64_t jb = wave_last_le(sa.first, nobj + 1, lo_s, lane);
            if (lane == 0) bc[0] = jb;
        } else if (w == 2) {
            const uint64_t je = wave_last_le(sa.first, nobj + 1, hi_s - 1, lane);
            if (lane == 0) bc[1] = je;
        }
    }
    const uint64_t p0 = p, c0 = c;
    uint64_t tp = 0, tc = 0;
    block_scan2(p, c, &tp, &tc);
    if (tid == 0) *rag = 0;
    __syncthreads();
    if (act && __any(r != 0) && lane == 0) atomicOr(rag, 1u);
    __syncthreads();
    uint64_t *ex = bc + 2;
    if (w == 0) {
        // the workspace's call count, read before this block publishes: the
        // last block bumps it only after its look-back saw every block's
        // descriptor, so all blocks of the call read the same count -- and
        // tag their descriptors with it: the key's low 62 bits above the state
        const uint64_t gen = uniform(ld_relaxed(ws.gen));
        uint64_t ep, ec, er;
        const bool ok = seg_lookback(ws.desc, b, scan_key(sa.epoch, gen) << 2, tp, tc, *rag, lane, &ep, &ec, &er,
                                     sa.fault_block);
        if (lane == 0) {
            ex[0] = ep;
            ex[1] = ec;
            ex[2] = er;
            if (!ok) report_scan_fault(sa, ws, gen);  // fail closed: the scan is not trustworthy
            if (b + 1 == nb) st_relaxed(ws.gen, gen + 1);
        }
    }
    __syncthreads();
    if (b + 1 == nb && tid == 0) {
        ws.P[nseg] = ex[0] + tp;
        ws.C[nseg] = ex[1] + tc;
        *ws.ragged = ex[2] | *rag;
    }
    uint64_t ep = ex[0] + p - p0, ec = ex[1] + c - c0;
    if (ws.obj) {
        if (act) {
            for (uint32_t t = tid; t < kScanBlk; t += kScanThreads) row[t] = kNoObj;
#pragma unroll
            for (uint32_t e = 0; e < kScanPer; e++) row_ne[tid * kScanPer + e] = l[e] != 0;
        }
        __syncthreads();
        if (act && lo_s < hi_s) {
            const uint64_t jb = bc[0], je = bc[1];
            for (uint64_t k = jb + tid; k <= je; k += kScanThreads) {
                const uint64_t a0 = sa.first[k], a1 = sa.first[k + 1];
                const uint64_t lo = a0 > lo_s ? a0 : lo_s, hi = a1 < hi_s ? a1 : hi_s;
                // the head segment is known here when the object starts in this
                // block and one of its segments here is not empty; otherwise
                // (kNoObj) the chunk pass compares byte offsets instead
                uint64_t hs = kNoObj;
                if (a0 >= s0)
                    for (uint64_t i = lo; i < hi; i++)
                        if (row_ne[i - s0]) {
                            hs = i;
                            break;
                        }
                for (uint64_t i = lo; i < hi; i++) {
                    row[i - s0] = k;
                    row_f0[i - s0] = a0;
                    row_f1[i - s0] = a1;
                    row_hs[i - s0] = hs;
                }
            }
        }
        __syncthreads();
    }
    if (!act) return;
#pragma unroll
    for (uint32_t e = 0; e < kScanPer; e++) {
        const uint64_t i = s0 + tid * kScanPer + e;
        if (i < nseg) {
            ws.P[i] = ep;
            ws.C[i] = ec;
            if (ws.obj) {
                const uint64_t t = i - s0;
                ws.obj[4 * i] = row[t];
                if (row[t] != kNoObj) {
                    ws.obj[4 * i + 1] = row_f0[t];
                    ws.obj[4 * i + 2] = row_f1[t];
                    ws.obj[4 * i + 3] = row_hs[t];
                }
            }
            // chunk -> segment map, while it fits (the chunk passes check the
            // total against map_cap and search C otherwise)
            const uint64_t ce = ec + seg_chunk_count(l[e]);
            if (ce <= ws.map_cap)
                for (uint64_t k = ec; k < ce; k++) ws.map[k] = (uint32_t)i;
        }
        ep += l[e];
        ec += seg_chunk_count(l[e]);
    }
}

__global__ __launch_bounds__(kScanThreads) void seg_scan(ScanArgs sa) {
    __shared__ __attribute__((aligned(16))) uint8_t scratch[kScanScratch];
    scan_block(sa, blockIdx.x, gridDim.x, scratch);
}


// Chunk c of segment s, as a pass found s: the chunk's bytes (k->addr, k->n)
// and its offset in the segment, or false.  (A scan whose look-back gave up --
// reported on the error word -- leaves tables that may not fit the list: such
// a chunk is skipped, never read out of bounds.  The rules: seg_plan.h.)
__device__ __forceinline__ bool seg_chunk_of(const SegArgs &a, uint64_t s, uint64_t c, uint64_t *off, SegChunk *k) {
    const bool ok = mck::seg_segment_ok(s, a.nseg);
    const uint64_t cs = ok ? a.w.C[s] : ~0ull, L = ok ? a.len[s] : 0;
    k->in = false;
    if (!mck::seg_chunk_bytes(c, cs, L, off, &k->n)) return false;
    k->addr = a.addr[s] + *off;
    return true;
}

// A wave's contiguous range of chunks [c, c1), walked in order.  The segment
// and object indices only advance, so a chunk costs a few cached scalar loads
// instead of two binary searches (~30 dependent loads); chunks are at most
// 256 KiB, so equal chunk counts are near-equal bytes.
struct ChunkWalk {
    const SegArgs *a;
    uint64_t c, c1, s, j;

    __device__ __forceinline__ ChunkWalk(const SegArgs &args, uint32_t wave, uint32_t nw, uint64_t nchunks) : a(&args) {
        c = nchunks * wave / nw;
        c1 = nchunks * (wave + 1) / nw;
        s = c < c1 ? lower_bound_u64(a->w.C, a->nseg + 1, c + 1) - 1 : 0;
        j = c < c1 && s >= a->first[0] ? lower_bound_u64(a->first, a->nobj + 1, s + 1) - 1 : 0;
    }

    // Next chunk, placed in its object (k->in: hash it).
    __device__ __forceinline__ bool next(SegChunk *k) {
        if (c >= c1) return false;
        while (s < a->nseg && a->w.C[s + 1] <= c) s++;  // skips empty segments
        uint64_t off;
        if (seg_chunk_of(*a, s, c, &off, k) && s >= a->first[0] && s < a->first[a->nobj]) {
            while (j + 1 < a->nobj && a->first[j + 1] <= s) j++;
            k->obj = j;
            k->at = a->w.P[s] + off;
            k->obj_at = a->w.P[a->first[j]];
            k->end = a->w.P[a->first[j + 1]];
            k->head = mck::seg_chunk_head(kNoObj, s, off, k->at, k->obj_at);
            k->in = mck::seg_chunk_place(k);
        }
        c++;
        return true;
    }
};

// Work-queue chunk pass (CRC-64).  Chunks are the queue's units, so a wave
// holds chunks from anywhere in the list and needs each one's segment and
// object without walking: the scan writes both maps (SegArgs::obj, ::map), so
// a chunk costs three dependent scalar loads.  A list with more chunks than
// the map holds (segments far above 1 MiB on average) searches C instead.
// The first build searched C and first[] for every chunk (a guess plus a
// gallop): its search loops pushed the 64-VGPR CRC-64 pass into 54 SGPR / 10
// VGPR spills and it measured 5% slower than the static ranges
// (profiles/r02/ab_seg_queue.log).
//
// Chunk c (< nchunks): its bytes and, when its segment belongs to an object
// (k->in), the object, its byte offsets and whether it starts the object.  c
// is wave-uniform, so every load is scalar: the map, then the segment's words
// and its 4-word object record.  The object's end offset (k->end) is a third
// dependent load, but the payload loop does not wait for it: without PLACE
// the caller applies seg_chunk_after only after the loop (round 4: the head
// test from the record's head segment instead of the object's start offset, a
// second third-round load).  Only a chunk whose object's head the scan block
// could not place compares byte offsets -- or, PLACE, a copying pass, which
// needs the object's start offset for the chunk's place anyway and has the
// chunk placed here.  Locate latency is not what limits the pass: two rounds instead
// of three measured within noise, and so did a one-round locate of bench.py's
// seg layout from the chunk index alone; the same layout with a constant
// chunk length measured +1.6-2.5% -- the compile-time trip count gave the
// payload loop whole-ring code (payload64_even, crc_gpu_crc64.h), now taken
// for every chunk of whole rings (profiles/r04/ab_seg_locate_bound.log,
// ab_seg_cheats.log, ab_seg_full.log, ab_seg_head.log, ab_seg_even.log).
template <bool PLACE>
__device__ __forceinline__ void seg_locate(const SegArgs &a, uint64_t c, uint64_t nchunks, SegChunk *k) {
    const uint64_t s = nchunks <= a.w.map_cap ? (uint64_t)a.w.map[c] : lower_bound_u64(a.w.C, a.nseg + 1, c + 1) - 1;
    uint64_t off;
    if (!seg_chunk_of(a, s, c, &off, k)) return;
    const uint64_t *o4 = a.w.obj + 4 * s;  // {j, first[j], first[j + 1], head segment}
    const uint64_t j = o4[0], fs = o4[1], ls = o4[2], hs = o4[3];
    if (!mck::seg_record_ok(j, a.nobj, fs, ls, a.nseg)) return;
    k->obj = j;
    k->at = a.w.P[s] + off;
    k->end = a.w.P[ls];
    k->obj_at = PLACE || !mck::seg_head_known(hs) ? a.w.P[fs] : 0;
    k->head = mck::seg_chunk_head(hs, s, off, k->at, k->obj_at);
    k->in = PLACE ? mck::seg_chunk_place(k) : true;
}

// The scan of this call gave up (reported on the error word, report_scan_fault):
// the chunk pass hashes nothing and writes nothing.
__device__ __forceinline__ bool scan_gave_up(const SegArgs &a) {
    return uniform(ld_relaxed(a.w.fault_claim)) == scan_key(a.epoch, uniform(ld_relaxed(a.w.gen)) - 1);
}

// A hashed chunk's epilogue: x, the chunk's register on the wave's lanes, is
// made uniform, completed for a head chunk shorter than the register (the
// init it could not carry in its first W/8 bytes comes in as Z^n(init)),
// shifted over the object bytes after the chunk and XORed into the object's
// output -- with init once more for a head chunk, cancelling the preset's.
template <int W, class Pack, class Shift, class Reg>
__device__ __forceinline__ void seg_emit(const Pack *pk, const Shift *sp, void *out, Reg init, Reg x, const SegChunk &k,
                                         uint32_t lane) {
    x = uniform(x);
    if (k.head && k.n < W / 8) x ^= pk->zinit[k.n];
    if constexpr (W == 32) {
        x = shift32(sp, x, k.after);
        if (lane == 0) atomicXor(reinterpret_cast<uint32_t *>(out) + k.obj, k.head ? x ^ init : x);
    } else {
        x = shift64(sp, x, k.after);
        if (lane == 0)
            atomicXor(reinterpret_cast<unsigned long long *>(out) + k.obj, (unsigned long long)(k.head ? x ^ init : x));
    }
}

// The chunk passes, one launch after the scan: one 1024-thread workgroup per
// CU either way.  CRC-32C (140 KiB of LDS tables): each wave walks a static
// contiguous range of chunks (ChunkWalk).  CRC-64 (round 4, "merged"): every
// chunk from the work queue, the ragged loop beside the aligned one in 128
// VGPRs and every operator in LDS.  (Round 3 split the CRC-64 chunks by
// shape: the aligned ones at two workgroups per CU, the ragged ones in a
// launch of their own -- ~7 us per call even when it found none.  Round 5
// tried scanning inside the chunk pass for lists of one scan block: one
// launch per call, but slower per call -- the other workgroups wait on block
// 0's scan with an agent-scope acquire -- and not kept: HISTORY.md.)
constexpr uint64_t kSegNtBytes = 512ull << 20;

// verify_segments' pass (BYSEG) has no output array: the object's word lies
// in the workspace, indexed by the object's first segment (seg_plan.h,
// seg_verify_layout).  false: no such segment -- skip the chunk.
__device__ __forceinline__ bool seg_by_first(const SegArgs &a, SegChunk *k) {
    const uint64_t fs = a.first[k->obj];
    k->obj = fs;
    return mck::seg_segment_ok(fs, a.nseg);
}

// The pass itself; BYSEG also leaves the call's key in *chunk_claim when a
// wait of the work queue gave up, for the compare that follows.
template <int W, bool BYSEG>
__device__ __forceinline__ void seg_pass(const SegArgs &a, uint64_t *chunk_claim) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_tab[W == 32 ? kL32Bytes : kL64Bytes];
    constexpr int kWPB = 1024 / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWPB + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * kWPB;
    const uint64_t nchunks = uniform(a.w.C[a.nseg]);
    // the CRC-64 pass takes chunks from the work queue (the host passes a
    // slot; without one, for_each_unit strides statically)
    constexpr bool kQueue = W == 64;
    __shared__ WgQueue wgq;
    if (kQueue && threadIdx.x == 0) wg_queue_init(&wgq, a.queue, nchunks);
    // hash nothing -- after the queue's init, which readies the slot's other bank
    if (scan_gave_up(a)) return;
    if constexpr (W == 32) {
        uint8_t *lds_raw = lds_tab;
        const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
        const crc32_shift_pack_t *sp = reinterpret_cast<const crc32_shift_pack_t *>(a.shift);
        fill_lds32<false, 1024>(lds_raw, pk);
        __syncthreads();
        const Tab32<false> lds{lds_raw};
        const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
        const bool nt = uniform(a.w.P[a.nseg]) >= kSegNtBytes;  // as for CRC-64 below
        const uint32_t init = pk->init;
        // every chunk of this wave's static range that belongs to an object
        ChunkWalk walk(a, wave, nw, nchunks);
        SegChunk k;
        while (walk.next(&k)) {
            if (!k.in) continue;
            if constexpr (BYSEG)
                if (!seg_by_first(a, &k)) continue;
            const uint8_t *q = reinterpret_cast<const uint8_t *>(k.addr);
            const uint64_t n = k.n;
            // whole rings of 1 KiB steps from a 16-B aligned start (the usual
            // bulk segment) take the aligned loop: no edge masks, no pad operator
            const bool aligned = k.addr % 16 == 0 && n % (1024u * kRing) == 0 && n != 0;
            // the object's first chunk starts from the register init (in its
            // first 4 bytes; Z^n(init) for a shorter chunk: seg_emit)
            const uint32_t reg = k.head && n >= 4 ? init : 0u;
            const uint32_t x = aligned && nt ? payload32_aligned<6, true>(lds, q, n >> 10, lane, lc0, lc1, reg)
                               : aligned     ? payload32_aligned<6, false>(lds, q, n >> 10, lane, lc0, lc1, reg)
                                             : payload32_g64<false, Tab32<false>, true>(lds, pk, q, n, lane, lc0, lc1, reg);
            seg_emit<32>(pk, sp, a.out, init, x, k, lane);
        }
    } else {
        uint8_t *lds = lds_tab;
        const crc64_gpu_pack_t *pk = reinterpret_cast<const crc64_gpu_pack_t *>(a.pack);
        const crc64_shift_pack_t *sp = reinterpret_cast<const crc64_shift_pack_t *>(a.shift);
        fill_lds64<1024, kOpsLds>(lds, pk);
        __syncthreads();
        const uint32_t lc = (lane & 31u) << 3;
        // Non-temporal payload loads once the batch is far larger than the
        // Infinity Cache, as for fixed batches.  Here the size is only known on
        // the device (the segment scan's total), so the choice is a uniform
        // branch per chunk: +3% on `seg` (duplicating the whole walk under one
        // branch measured the same and spills more).
        const bool nt = uniform(a.w.P[a.nseg]) >= kSegNtBytes;
        const uint64_t init = pk->init;
        // Pipelined (round 6, as the split CRC-64 pieces): a chunk of whole
        // rings from an aligned start (every chunk of a list of 16-B aligned
        // KiB-multiple segments) runs from a ring its predecessor loaded --
        // the wave takes the next chunk and issues its first loads as soon as
        // the current step loop ends, before the current chunk's lane combine,
        // Z^n shift and output XOR.  Other chunks run on their own.
        struct Chunk : SegChunk {
            bool even = false;
        };
        auto locate = [&](uint64_t c, Chunk *k) {
            seg_locate<false>(a, c, nchunks, k);
            if constexpr (BYSEG)
                if (k->in) k->in = seg_by_first(a, k);
            k->even = k->in && k->addr % 16 == 0 && k->n % (1024u * kRing64) == 0 && k->n >= 2048u * kRing64;
        };
        auto issue = [&](uint4 (&ring)[kRing64], const Chunk &k) {
            if (nt) ring64_load<true>(ring, reinterpret_cast<const uint8_t *>(k.addr), lane);
            else ring64_load<false>(ring, reinterpret_cast<const uint8_t *>(k.addr), lane);
        };
        UnitTaker<ChunkPlan> tk(&wgq, a.queue, nchunks, wave, nw, false, ChunkPlan(nchunks, gridDim.x));
        Lane64 ln = lane64(lc);
        uint4 ring[kRing64];
        uint64_t c = 0;
        Chunk cur;
        bool have = tk.take_unit(&c);
        if (have) locate(c, &cur);
        if (have && cur.even) issue(ring, cur);
        while (have) {
            // an untrusted scan (seg_plan.h): prefixes that put the chunk past
            // its object's end would shift by a wrapped count (shift64 indexes
            // its operators by that count's hex digits, 12 of them held) --
            // skipped as the others.  Tested here, not in locate(): the next
            // chunk's first loads do not wait for its object's end offset.
            if (cur.in && !mck::seg_chunk_after(&cur)) cur.in = cur.even = false;
            const uint8_t *q = reinterpret_cast<const uint8_t *>(cur.addr);
            // the object's first chunk starts from the register init (in its
            // first 8 bytes; Z^n(init) for a shorter, ragged chunk: seg_emit)
            const uint64_t reg = cur.head && cur.n >= 8 ? init : 0ull;
            uint64_t x = 0, x0 = 0, x1 = 0;
            const bool aligned = cur.addr % 16 == 0 && cur.n % 1024 == 0;
            if (cur.even) {
                if (nt) fold64_ring<true>(lds, ring, q, (uint32_t)(cur.n >> 10), lane, ln, reg, &x0, &x1);
                else fold64_ring<false>(lds, ring, q, (uint32_t)(cur.n >> 10), lane, ln, reg, &x0, &x1);
            } else if (cur.in && aligned) {
                x = payload64_aligned<6, false, kOpsLds>(lds, pk, q, (uint32_t)(cur.n >> 10), lane, lc, reg);
            } else if (cur.in) {
                x = payload64_g64<false, true>(lds, pk, q, cur.n, lane, lc, reg);
            }
            uint64_t cn = 0;
            Chunk nxt;
            const bool next = tk.take_unit(&cn);
            if (next) locate(cn, &nxt);
            if (next && nxt.even) issue(ring, nxt);  // in flight during the combine below
            if (cur.in) {
                if (cur.even) x = combine64<6, kOpsLds>(lds, pk, x0, x1, lane);
                seg_emit<64>(pk, sp, a.out, init, x, cur, lane);
            }
            cur = nxt;
            have = next;
        }
        const bool faulted = tk.finish(wave);
        if (faulted && lane == 0 && a.err_word) atomicAdd(a.err_word, 1u);
        if constexpr (BYSEG)
            if (faulted && lane == 0) st_relaxed(chunk_claim, scan_key(a.epoch, ld_relaxed(a.w.gen) - 1));
    }
}

template <int W>
__global__ __launch_bounds__(1024, 1) void seg_kernel(SegArgs a) {
    seg_pass<W, false>(a, nullptr);
}

// verify_segments: the chunk pass into the workspace's words, then the compare.
struct SegVerifyArgs {
    SegArgs s;  // s.out: the accumulator words (seg_verify_layout)
    uint64_t *chunk_claim;
    const void *expected;
    uint8_t *status;
    uint32_t *mism;
    uint64_t init, xorout;
    int msb;
};

template <int W>
__global__ __launch_bounds__(1024, 1) void seg_verify_pass_kernel(SegVerifyArgs va) {
    seg_pass<W, true>(va.s, va.chunk_claim);
}

// Between the scan and the chunk pass of an update or verify call, a thread
// per object.  Update: the state becomes the seed term of the object's byte
// total (crc_gpu_seed.h, mck_seg_seed), so that the chunk pass's XORs end it
// as R(s, M); an object without bytes is not written, and after a scan that
// gave up neither is any (the chunk pass then hashes nothing: the states
// stay as they were).  Verify (SEED false): the object's word starts at 0.
struct SegPreArgs {
    const uint64_t *first;
    uint64_t nobj, nseg, epoch;
    SegWork w;
    void *word;  // the states, or verify's accumulator words
    const void *shift;
    uint64_t init;
};

template <typename T, bool SEED>
__global__ __launch_bounds__(256) void seg_pre_kernel(SegPreArgs a) {
    if constexpr (SEED)
        if (ld_relaxed(a.w.fault_claim) == scan_key(a.epoch, ld_relaxed(a.w.gen) - 1)) return;
    T *word = reinterpret_cast<T *>(a.word);
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < a.nobj; j += (uint64_t)gridDim.x * 256) {
        const uint64_t f0 = a.first[j], f1 = a.first[j + 1];
        if (!(f0 < f1 && f1 <= a.nseg)) continue;
        if constexpr (!SEED) {
            word[f0] = 0;
        } else {
            const uint64_t n = a.w.P[f1] - a.w.P[f0];
            if (n == 0) continue;
            if constexpr (sizeof(T) == 8)
                word[j] = mck_seg_seed64(reinterpret_cast<const crc64_shift_pack_t *>(a.shift), word[j], a.init, n);
            else
                word[j] = mck_seg_seed32(reinterpret_cast<const crc32_shift_pack_t *>(a.shift), word[j],
                                         (uint32_t)a.init, n);
        }
    }
}

// verify_segments' compare, after the chunk pass: the call's fault state
// first, then a thread per object (seg_plan.h: seg_call_faulted,
// seg_verify_decide).  An object without segments has no word: its value is
// the CRC of the empty message, as is that of one whose segments are empty.
template <typename T>
__global__ __launch_bounds__(256) void seg_verify_kernel(SegVerifyArgs va) {
    const SegArgs &a = va.s;
    const bool faulted = mck::seg_call_faulted(ld_relaxed(a.w.fault_claim), ld_relaxed(va.chunk_claim),
                                               scan_key(a.epoch, ld_relaxed(a.w.gen) - 1));
    const T *acc = reinterpret_cast<const T *>(a.out);
    uint32_t nbad = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < a.nobj; j += (uint64_t)gridDim.x * 256) {
        const uint64_t f0 = a.first[j], f1 = a.first[j + 1];
        const T x = !faulted && f0 < f1 && f1 <= a.nseg ? acc[f0] : (T)0;
        uint64_t v;
        if constexpr (sizeof(T) == 8) v = mck_seg_value64(x, va.init, va.xorout, va.msb);
        else v = mck_seg_value32(x, (uint32_t)va.init, (uint32_t)va.xorout, va.msb);
        nbad += mck::seg_verify_decide(faulted, v, reinterpret_cast<const T *>(va.expected)[j], va.status, j);
    }
    add_mismatches(va.mism, nbad);  // once per workgroup (crc_gpu_common.h); no counter: nothing added
}

// The copying chunk passes (mchecksum_gpu_gather_segments, _scatter_segments):
// seg_kernel's walk, head-chunk rule, shift and output XOR, with every chunk
// also stored on the other side by the payload loop that hashes it, so each
// byte is read once.  DIR (seg_plan.h): gather loads the chunk from its
// segment and stores it at its place in the object's contiguous range,
// scatter the reverse; the hashed bytes are the loaded ones either way.  The
// chunk's place in its object is P[s] + off - P[first[j]]: one more scalar
// load than seg_kernel per chunk (the queue pass has first[j] in the
// segment's record).  Every chunk takes the one-payload-per-wave loop in its
// RAW, COPY form (chunks are at most 256 KiB): right for every alignment of
// either side, and the store rule (crc_gpu_pack_store.h) writes only the
// chunk's own bytes -- whole 16-byte pieces unaligned, edge pieces byte by
// byte -- so the waves that store neighbouring chunks of one object never
// touch the same byte and nothing is read back from the destination.  The
// aligned loops have no COPY form, and the CRC-64 pass is not pipelined
// across chunks.
struct SegCopyArgs {
    SegArgs s;
    uint8_t *flat;           // the contiguous side: gather's destination, scatter's source
    const uint64_t *starts;  // nobj byte offsets into it
};

template <int W, int DIR>
__global__ __launch_bounds__(1024, 1) void seg_copy_kernel(SegCopyArgs ca) {
    static_assert(DIR == mck::kSegGather || DIR == mck::kSegScatter, "no such direction");
    const SegArgs &a = ca.s;
    __shared__ __attribute__((aligned(16))) uint8_t lds_tab[W == 32 ? kL32Bytes : kL64Bytes];
    constexpr int kWPB = 1024 / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWPB + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * kWPB;
    const uint64_t nchunks = uniform(a.w.C[a.nseg]);
    __shared__ WgQueue wgq;
    if (W == 64 && threadIdx.x == 0) wg_queue_init(&wgq, a.queue, nchunks);
    // hash nothing and, ahead of the first store below, write nothing
    if (scan_gave_up(a)) return;
    const bool nt = uniform(a.w.P[a.nseg]) >= kSegNtBytes;  // as seg_kernel
    const uint64_t flat = reinterpret_cast<uint64_t>(ca.flat);
    // a placed chunk's addresses: where the payload loop loads and stores it
    auto sides = [&](const SegChunk &k, const uint8_t **q, uint8_t **d) {
        const mck::SegCopyAddr ad = mck::seg_copy_addr(DIR, k.addr, flat, ca.starts[k.obj], k.obj_off);
        *q = reinterpret_cast<const uint8_t *>(ad.load);
        *d = reinterpret_cast<uint8_t *>(ad.store);
    };
    if constexpr (W == 32) {
        uint8_t *lds_raw = lds_tab;
        const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
        const crc32_shift_pack_t *sp = reinterpret_cast<const crc32_shift_pack_t *>(a.shift);
        [[clang::always_inline]] fill_lds32<false, 1024>(lds_raw, pk);  // (as it is in seg_kernel)
        __syncthreads();
        const Tab32<false> lds{lds_raw};
        const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
        const uint32_t init = pk->init;
        ChunkWalk walk(a, wave, nw, nchunks);
        SegChunk k;
        while (walk.next(&k)) {
            if (!k.in) continue;  // (a chunk the walk could not place is stored nowhere)
            const uint8_t *q;
            uint8_t *d;
            sides(k, &q, &d);
            const uint64_t n = k.n;
            const uint32_t reg = k.head && n >= 4 ? init : 0u;
            const uint32_t x = nt ? payload32_g64<true, Tab32<false>, true, true>(lds, pk, q, n, lane, lc0, lc1, reg, d)
                                  : payload32_g64<false, Tab32<false>, true, true>(lds, pk, q, n, lane, lc0, lc1, reg, d);
            seg_emit<32>(pk, sp, a.out, init, x, k, lane);
        }
    } else {
        uint8_t *lds = lds_tab;
        const crc64_gpu_pack_t *pk = reinterpret_cast<const crc64_gpu_pack_t *>(a.pack);
        const crc64_shift_pack_t *sp = reinterpret_cast<const crc64_shift_pack_t *>(a.shift);
        fill_lds64<1024, kOpsLds>(lds, pk);
        __syncthreads();
        const uint32_t lc = (lane & 31u) << 3;
        const uint64_t init = pk->init;
        auto one = [&](uint64_t c) {
            SegChunk k;
            seg_locate<true>(a, c, nchunks, &k);
            if (!k.in) return;
            const uint8_t *q;
            uint8_t *d;
            sides(k, &q, &d);
            const uint64_t n = k.n;
            const uint64_t reg = k.head && n >= 8 ? init : 0ull;
            const uint64_t x = nt ? payload64_g64<true, true, kOpsLds, true>(lds, pk, q, n, lane, lc, reg, d)
                                  : payload64_g64<false, true, kOpsLds, true>(lds, pk, q, n, lane, lc, reg, d);
            seg_emit<64>(pk, sp, a.out, init, x, k, lane);
        };
        const bool faulted = for_each_unit<true>(&wgq, a.queue, nchunks, wave, nw, one);
        if (faulted && lane == 0 && a.err_word) atomicAdd(a.err_word, 1u);
    }
}

// The message calls (mchecksum_gpu_pack_segment_messages, _unpack_segment_
// messages; CRC-32C): object j's segments are the fields of message j, the
// per-field form of pack_messages / unpack_messages (HG_PROC_TYPE copies a
// field and feeds the same bytes to mchecksum_update, src/mercury_proc.h:
// 124-143,162-181).  The copying pass above with the messages' payloads as
// the contiguous side -- c.flat = dev_buf + payload_offset, c.starts = the
// message table -- in a kernel of its own (the plain copying kernels keep
// their code) between two thread-per-object launches:
//   before: the fit of message j (seg_plan.h, seg_msg_gate: from the scan's P
//           and the message table) into gate[j], and the object's accumulator
//           word (c.s.out, a word per object behind the scan's workspace:
//           seg_msg_layout) zeroed;
//   the pass: seg_copy_kernel<32, DIR>'s walk and loop; no chunk of a message
//           that does not fit is loaded or stored;
//   after:  the call's fault state first, as verify_segments' compare; then
//           pack stores the finalised value big-endian in the header's hash
//           slot (byte by byte: the slot has no alignment), unpack compares it
//           with the word there and counts.  A gated message gets status 1
//           and, on unpack, one mismatch.
// The CRC-32C pass walks static ranges: only the scan can give up.
struct SegMsgArgs {
    SegCopyArgs c;
    uint8_t *gate;          // nobj bytes of the workspace
    uint8_t *buf;           // the messages (unpack only reads them)
    const uint64_t *off;    // nobj + 1 message offsets
    uint64_t pay_off, hash_off;
    uint8_t *status;
    uint32_t *mism;
    uint32_t init, xorout;
};

__global__ __launch_bounds__(256) void seg_msg_pre_kernel(SegMsgArgs ma) {
    const SegArgs &a = ma.c.s;
    uint32_t *acc = reinterpret_cast<uint32_t *>(a.out);
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < a.nobj; j += (uint64_t)gridDim.x * 256) {
        const uint64_t f0 = a.first[j], f1 = a.first[j + 1];
        const bool ok = mck::seg_msg_range_ok(f0, f1, a.nseg);
        const uint64_t p0 = ok ? a.w.P[f0] : 0, p1 = ok ? a.w.P[f1] : 0;
        acc[j] = 0;
        ma.gate[j] = mck::seg_msg_gate(ok, p0, p1, ma.off[j], ma.off[j + 1], ma.pay_off);
    }
}

template <int DIR>
__global__ __launch_bounds__(1024, 1) void seg_msg_copy_kernel(SegMsgArgs ma) {
    static_assert(DIR == mck::kSegGather || DIR == mck::kSegScatter, "no such direction");
    const SegArgs &a = ma.c.s;
    __shared__ __attribute__((aligned(16))) uint8_t lds_raw[kL32Bytes];
    constexpr int kWPB = 1024 / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWPB + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * kWPB;
    const uint64_t nchunks = uniform(a.w.C[a.nseg]);
    // hash nothing and, ahead of the first store below, write nothing
    if (scan_gave_up(a)) return;
    const bool nt = uniform(a.w.P[a.nseg]) >= kSegNtBytes;  // as seg_kernel
    const uint64_t flat = reinterpret_cast<uint64_t>(ma.c.flat);
    const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
    const crc32_shift_pack_t *sp = reinterpret_cast<const crc32_shift_pack_t *>(a.shift);
    [[clang::always_inline]] fill_lds32<false, 1024>(lds_raw, pk);  // (as in seg_copy_kernel)
    __syncthreads();
    const Tab32<false> lds{lds_raw};
    const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
    const uint32_t init = pk->init;
    ChunkWalk walk(a, wave, nw, nchunks);
    SegChunk k;
    while (walk.next(&k)) {
        if (!k.in) continue;           // (a chunk the walk could not place is stored nowhere)
        if (ma.gate[k.obj]) continue;  // the message does not fit: none of its bytes moves
        const mck::SegCopyAddr ad = mck::seg_copy_addr(DIR, k.addr, flat, ma.c.starts[k.obj], k.obj_off);
        const uint8_t *q = reinterpret_cast<const uint8_t *>(ad.load);
        uint8_t *d = reinterpret_cast<uint8_t *>(ad.store);
        const uint64_t n = k.n;
        const uint32_t reg = k.head && n >= 4 ? init : 0u;
        const uint32_t x = nt ? payload32_g64<true, Tab32<false>, true, true>(lds, pk, q, n, lane, lc0, lc1, reg, d)
                              : payload32_g64<false, Tab32<false>, true, true>(lds, pk, q, n, lane, lc0, lc1, reg, d);
        seg_emit<32>(pk, sp, a.out, init, x, k, lane);
    }
}

// DIR: kSegGather = pack (seal), kSegScatter = unpack (compare)
template <int DIR>
__global__ __launch_bounds__(256) void seg_msg_post_kernel(SegMsgArgs ma) {
    const SegArgs &a = ma.c.s;
    const uint64_t claim = ld_relaxed(a.w.fault_claim);
    const bool faulted = mck::seg_call_faulted(claim, claim, scan_key(a.epoch, ld_relaxed(a.w.gen) - 1));
    const uint32_t *acc = reinterpret_cast<const uint32_t *>(a.out);
    uint32_t nbad = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < a.nobj; j += (uint64_t)gridDim.x * 256) {
        const uint8_t gate = ma.gate[j];
        const uint32_t v = mck_seg_value32(faulted ? 0u : acc[j], ma.init, ma.xorout, 0);
        if constexpr (DIR == mck::kSegGather) {
            if (mck::seg_msg_seal_decide(faulted, gate, ma.status, j)) {
                uint8_t *h = ma.buf + ma.off[j] + ma.hash_off;
                h[0] = (uint8_t)(v >> 24);
                h[1] = (uint8_t)(v >> 16);
                h[2] = (uint8_t)(v >> 8);
                h[3] = (uint8_t)v;
            }
        } else {
            uint32_t want = 0;
            if (mck::seg_msg_compares(faulted, gate)) {
                const uint8_t *h = ma.buf + ma.off[j] + ma.hash_off;
                want = (uint32_t)h[0] << 24 | (uint32_t)h[1] << 16 | (uint32_t)h[2] << 8 | h[3];
            }
            nbad += mck::seg_msg_open_decide(faulted, gate, v, want, ma.status, j);
        }
    }
    if constexpr (DIR == mck::kSegScatter) add_mismatches(ma.mism, nbad);  // once per workgroup; no counter: nothing added
}

// --------------------------------------------------------- core headers ----
//
// Wire layout (hg_core_header_*_proc, src/mercury_core_header.c:175-289; the
// structs are 16 bytes, src/mercury_core_header.h:23-40, and a buffer shorter
// than that is rejected, :183-184 / :240-242):
//   request : hg u8 | protocol u8 | id u64 big-endian | flags u8 | cookie u8 | hash u16 BE at 12
//   response: ret_code i8 | flags u8 | cookie u16 BE | hash u16 BE at 4
// The CRC runs over the HOST-order field values as the proc code feeds them to
// mchecksum_update (HG_CORE_HEADER_CHECKSUM_UPDATE, :48-55): request
// hg, protocol, id (8 little-endian bytes), flags, cookie = 12 bytes; response
// ret_code, flags, cookie (2 little-endian bytes) = 4 bytes.
constexpr uint32_t kHdrSize = 16;

struct HdrArgs {
    const uint8_t *buf;
    const uint64_t *off;
    uint64_t count;
    uint8_t *status;
    uint32_t *mism;
    const uint16_t *table;  // byte table of the 16-bit model
    uint32_t kind, reflected, init, xorout;
};

// One body for the receiver's check and the sender's seal (SEAL: the value is
// stored big-endian in the header's hash field instead of compared with it --
// two byte stores, a message starts at any byte -- and a message shorter than
// a header is not written; status 1).  No wait on the device in either, so
// nothing to fail closed on.
template <bool SEAL>
__device__ __forceinline__ void core_header_body(const HdrArgs &a) {
    __shared__ uint16_t T[256];
    T[threadIdx.x] = a.table[threadIdx.x];
    __syncthreads();
    uint32_t nbad = 0;
    for (uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x; m < a.count; m += (uint64_t)gridDim.x * 256) {
        const uint64_t o = a.off[m];
        const bool whole = a.off[m + 1] - o >= kHdrSize;
        const uint8_t *h = a.buf + o;
        uint8_t img[12];
        uint32_t n, wire = 0;
        if (!whole) {
            n = 0;
        } else if (a.kind == MCHECKSUM_GPU_CORE_HEADER_REQUEST) {
            img[0] = h[0];
            img[1] = h[1];
#pragma unroll
            for (int b = 0; b < 8; b++) img[2 + b] = h[9 - b];  // big-endian on the wire, host LE image
            img[10] = h[10];
            img[11] = h[11];
            if constexpr (!SEAL) wire = (uint32_t)h[12] << 8 | h[13];
            n = 12;
        } else {
            img[0] = h[0];
            img[1] = h[1];
            img[2] = h[3];
            img[3] = h[2];
            if constexpr (!SEAL) wire = (uint32_t)h[4] << 8 | h[5];
            n = 4;
        }
        uint32_t r = a.init;
        if (a.reflected) {
            for (uint32_t i = 0; i < n; i++) r = (r >> 8) ^ T[(r ^ img[i]) & 0xFFu];
        } else {
            for (uint32_t i = 0; i < n; i++) r = ((r << 8) ^ T[((r >> 8) ^ img[i]) & 0xFFu]) & 0xFFFFu;
        }
        if constexpr (SEAL) {
            if (whole) {
                uint8_t *q = const_cast<uint8_t *>(h) + (a.kind == MCHECKSUM_GPU_CORE_HEADER_REQUEST ? 12 : 4);
                q[0] = (uint8_t)((r ^ a.xorout) >> 8);
                q[1] = (uint8_t)(r ^ a.xorout);
            }
            if (a.status) a.status[m] = whole ? 0 : 1;
        } else {
            const bool bad = !whole || ((r ^ a.xorout) & 0xFFFFu) != wire;
            if (a.status) a.status[m] = bad ? 1 : 0;
            nbad += bad;
        }
    }
    if constexpr (!SEAL) add_mismatches(a.mism, nbad);  // once per workgroup (crc_gpu_common.h)
}

__global__ __launch_bounds__(256) void core_header_kernel(HdrArgs a) { core_header_body<false>(a); }
__global__ __launch_bounds__(256) void core_header_seal_kernel(HdrArgs a) { core_header_body<true>(a); }

// ------------------------------------------------------------------ XDR ----
//
// Under HG_HAS_XDR every typed field goes through xdr_<type>: RNDUP(sizeof)
// bytes on the wire -- a 1-, 2- or 4-byte integer as one big-endian 32-bit
// word (sign-extended for the signed types), an 8-byte integer as two
// big-endian words, high first -- while HG_PROC_CHECKSUM_UPDATE hashes the
// sizeof(type) bytes of the HOST variable (src/mercury_proc.h:110-122).  Byte
// arrays go through xdr_opaque: the bytes, then zero pad to a multiple of 4,
// with only the bytes hashed (:147-160).  hg_proc_save_ptr/restore_ptr regions
// (bulk handles, src/mercury_proc_bulk.c:91-125) are raw at their exact size
// (src/mercury_proc.c:277-335).  So a whole-buffer CRC is wrong in XDR mode;
// this kernel walks a per-message field schema instead.  The hashed stream of
// a little-endian host is, per field: the low `size` bytes of the decoded
// integer in little-endian order, or the raw bytes of an opaque/raw field.
//
// One wave per message, the schema walk wave-uniform (the schema rides in the
// kernel arguments).  The register L of the hashed stream starts at the
// model's initial value and is built field by field: an integer updates it
// byte by byte from an LDS byte table; an opaque or raw field of n bytes is
// cut into 64 lane ranges hashed byte by byte, each shifted past the bytes
// after it (Z^k from the base-16 digit tables) and XOR-reduced over the
// wave, then L <- Z^n(L) ^ that.  CRC = L ^ xorout.
//
// Large batches (the throughput layout, round 3) run the same walk in
// persistent 1024-thread workgroups that also hold the payload kernels' LDS
// tables: an opaque or raw field of >= kXdrFastMin bytes is hashed by the
// payload step loop (coalesced 1 KiB steps, payload32_g64 / payload64_g64 in
// RAW form: zero init, no finalisation) instead of 64 byte-serial lane
// ranges, and messages come from the work queue (crc_gpu_queue.h).  The
// step loop starts from the running register itself (it rides in the field's
// first bytes, R(L, M) = R(0, M ^ L)), so such a field needs no Z^n shift:
// an iovec message (hg_perf_proc_iovec, Testing/perf/hg/mercury_perf.c:897-923:
// a u32 length, then the bytes) costs its 4-byte table walk plus what the
// same payload costs through the offsets kernel -- no dependent chain of
// digit-table loads per message (round 3: two Z^n shifts per message before).
constexpr uint32_t kXdrMaxFields = 64;
constexpr uint64_t kXdrFastMin = 256;

struct XdrArgs {
    const uint8_t *buf;
    const uint64_t *off;
    uint64_t count;
    void *out;
    uint8_t *status;
    const void *shift;
    const void *pack;                // throughput kernel: the model's G = 64 table pack
    unsigned long long *queue;       // throughput kernel: work-queue slot (nullptr: static split)
    uint32_t *err_word;              // throughput kernel: fail-closed report
    uint64_t rpoly, init, xorout;
    uint32_t nf;
    uint32_t kind[kXdrMaxFields], size[kXdrMaxFields];
};

template <int W>
using xdr_reg_t = typename std::conditional<W == 32, uint32_t, uint64_t>::type;

template <int W>
__device__ __forceinline__ xdr_reg_t<W> xdr_shift(const void *sp, xdr_reg_t<W> x, uint64_t n) {
    if constexpr (W == 32) return shift32(reinterpret_cast<const crc32_shift_pack_t *>(sp), x, n);
    else return shift64(reinterpret_cast<const crc64_shift_pack_t *>(sp), x, n);
}

// Byte table of the register form (Z^1 of the low byte) for entry t < 256.
template <int W>
__device__ __forceinline__ xdr_reg_t<W> xdr_tab_entry(uint64_t rpoly, uint32_t t) {
    using R = xdr_reg_t<W>;
    R r = (R)t;
    for (int k = 0; k < 8; k++) r = (r & 1u) ? (r >> 1) ^ (R)rpoly : r >> 1;
    return r;
}

// What an XDR call does with each message's value x (as launch_plan.h's
// BatchOp names the offsets kernels' operations: the one name an entry point
// gives its call, carried into the kernels' OP template argument, from which
// the walk derives its compile-time variants -- so checksum_xdr's kernels are
// the code they were).  The three message operations take whole messages:
// the walk starts XdrMsg::pay_off bytes into message m and the header hash is
// the network-order u32 at XdrMsg::hash_off; a message shorter than pay_off
// fails like one the schema runs past.
enum XdrOp : int {
    // out[m] = x, status[m] = 1 when the schema runs past the message.
    kXdrChecksum,
    // mchecksum_gpu_verify_xdr_messages: x is compared with the header hash:
    // status[m], and the launch's count in *mism.
    kXdrVerify,
    // mchecksum_gpu_seal_xdr_messages: x is stored big-endian in the hash
    // slot; a failed message gets status 1 and is not written.
    kXdrSeal,
    // mchecksum_gpu_unpack_xdr_messages: verify, and the hashed stream -- the
    // little-endian image of every INT, the bytes of every opaque or raw
    // field -- is also stored at dst[dst_off[m], dst_off[m + 1]) by the walk
    // that hashes it.  The decoded length depends on the data, so the INT
    // fields are walked once for it first (xdr_decoded_len): a message whose
    // decoded length is not its slot's gets status 1, one mismatch and no
    // byte written.
    kXdrUnpack,
    // mchecksum_gpu_pack_xdr_messages: the sender's mirror of unpack -- the
    // walk reads the non-XDR image, stores its XDR encoding into the message
    // and seals it (xdr_pack_message, a sibling walker with arguments and
    // kernels of its own: XdrPackArgs).
    kXdrPack,
    // The four message operations in the RPC frame (launch_plan.h, "whole RPC
    // messages in XDR mode"): mchecksum_gpu_verify_rpc_xdr_messages, _seal_,
    // _unpack_, _pack_.  The same walks between a prologue -- sixteen lanes
    // load the core header and look up its CRC-16 terms; the flags byte and
    // the length decide for the whole wave whether the walk starts -- and an
    // epilogue that gives the message its class (xdr_rpc_header, _hdr_crc).
    // Kernels of their own (xdr_rpc_kernel, xdr_rpc_fast_kernel): the five
    // operations above keep theirs, instantiated as they were.
    kXdrRpcVerify,
    kXdrRpcSeal,
    kXdrRpcUnpack,
    kXdrRpcPack,
};
constexpr bool xdr_op_rpc(int op) { return op >= kXdrRpcVerify; }
// What the walk does between the frame's two ends: the operation without its frame.
constexpr int xdr_op_walk(int op) { return xdr_op_rpc(op) ? op - kXdrRpcVerify + kXdrVerify : op; }
static_assert(xdr_op_walk(kXdrRpcVerify) == kXdrVerify && xdr_op_walk(kXdrRpcSeal) == kXdrSeal &&
                  xdr_op_walk(kXdrRpcUnpack) == kXdrUnpack && xdr_op_walk(kXdrRpcPack) == kXdrPack,
              "the RPC operations name the message operations in their order");

// The message operations' arguments beside XdrArgs (whose `out` they leave unused).
struct XdrMsg {
    uint64_t pay_off, hash_off;
    uint8_t *dst;             // unpack
    const uint64_t *dst_off;  // unpack: count + 1 entries
    uint32_t *mism;           // verify, unpack (the RPC frame: the 6 or 7 class counts)
};
struct XdrMsgArgs {
    XdrArgs a;
    XdrMsg x;
};

// ---- the RPC frame around a walk ----
// The header model's pack as a kernel reads it once, at entry (scalar loads).
struct XdrRpcFront {
    rpc_tab_t tab = nullptr;  // RpcHdrPack::row, in global memory: one 2-byte load per header byte and message
    uint32_t kind = 0, c = 0;
};
__device__ __forceinline__ XdrRpcFront xdr_rpc_front(const void *hdr_pack) {
    const mck::RpcHdrPack *hp = reinterpret_cast<const mck::RpcHdrPack *>(hdr_pack);
    XdrRpcFront r;
    r.tab = (rpc_tab_t)uniform64(reinterpret_cast<uint64_t>(&hp->row[0][0]));
    r.kind = hp->kind;
    r.c = hp->c;
    return r;
}
// Prologue, the whole wave, ahead of every load behind the core header: lanes
// 0..15 load a header byte each (none of a message without a whole header),
// the flags byte is read from its lane, and each lane's term of the CRC-16 is
// looked up -- that load is in flight under the walk and joined in the epilogue
// (xdr_rpc_hdr_crc), as the plain RPC kernels do it (crc_gpu_crc32.h).
struct XdrRpcHdr {
    bool more = false;
    uint32_t term = 0;
};
__device__ __forceinline__ XdrRpcHdr xdr_rpc_header(const XdrRpcFront &r, const uint8_t *msg, uint64_t L, uint32_t lane) {
    const bool whole = L >= mck::kRpcHdrBytes;
    uint32_t hb = 0;
    XdrRpcHdr h;
    if (whole && lane < mck::kRpcHdrBytes) hb = global_ptr(msg, true)[lane];
    h.more = whole && (__builtin_amdgcn_readlane(hb, mck::rpc_flags_at(r.kind)) & 1u);
    if (whole && lane < mck::kRpcHdrBytes) h.term = r.tab[mck::rpc_hdr_term_index(r.kind, lane, hb)];
    return h;
}
// Epilogue, the whole wave: the image's terms XOR over the lanes that hold them; the wire hash is two identity terms.
__device__ __forceinline__ void xdr_rpc_hdr_crc(const XdrRpcFront &r, uint32_t term, uint32_t lane, uint32_t *crc16,
                                                uint32_t *wire) {
    uint32_t t = lane < mck::rpc_img_bytes(r.kind) ? term : 0u;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) t ^= __shfl_xor(t, d, 64);
    *crc16 = mck::rpc_hdr_crc(r.c, __builtin_amdgcn_readfirstlane(t));
    const uint32_t hat = mck::rpc_hash_at(r.kind);
    *wire = __builtin_amdgcn_readlane(term, hat) << 8 | __builtin_amdgcn_readlane(term, hat + 1);
}
// (byte stores: the two bytes share their granule with other header fields)
__device__ __forceinline__ void xdr_rpc_store_crc16(uint8_t *msg, uint32_t kind, uint32_t crc16) {
    const uint32_t hat = mck::rpc_hash_at(kind);
    msg[hat] = (uint8_t)(crc16 >> 8);
    msg[hat + 1] = (uint8_t)crc16;
}

// Where message m lies: [pos, end) from a.buf.  The table form reads two
// offsets.  LIST (the _rpc_xdr_message_list calls, the RPC frame's kernels
// only): a.off holds the `count` addresses, `len` the lengths, a.buf is NULL
// and the frame is launch_plan.h's -- pos is the address itself, or 0 for a
// message without a whole core header, whose entry so forms no pointer.
struct XdrMsgAt {
    uint64_t pos, end, L;  // (L: the RPC frame's; the table form takes it from pos and end where it always did)
};
template <bool LIST>
__device__ __forceinline__ XdrMsgAt xdr_msg_at(const XdrArgs &a, [[maybe_unused]] const uint64_t *len, uint64_t m) {
    if constexpr (LIST) {
        const uint64_t addr = a.off[m], n = len[m];
        const uint64_t at = mck::rpc_xdr_list_at(addr, n), L = mck::rpc_xdr_list_len(addr, n);
        return XdrMsgAt{at, at + L, L};
    } else {
        return XdrMsgAt{a.off[m], a.off[m + 1], 0};
    }
}

// The length of the hashed stream of the message at [pos, end): the main
// walk's steps and bounds tests, reading the INT fields only.  false: the
// schema runs past the message.
__device__ __forceinline__ bool xdr_decoded_len(const XdrArgs &a, uint64_t pos, uint64_t end, uint64_t *n,
                                                uint64_t *wire = nullptr) {
    uint64_t last = 0, total = 0;
    const uint64_t pos0 = pos;
    for (uint32_t f = 0; f < a.nf; f++) {
        const uint32_t kind = a.kind[f], sz = a.size[f];
        if (kind == MCHECKSUM_XDR_SKIP_IF_ZERO) {
            if (last == 0) f += sz;
            continue;
        }
        if (kind == MCHECKSUM_XDR_INT) {
            const uint32_t slot = sz <= 4 ? 4u : 8u;
            if (end - pos < slot) return false;
            uint64_t v = 0;
            for (uint32_t b = 0; b < slot; b++) v = v << 8 | a.buf[pos + b];
            last = sz == 8 ? v : v & ((1ull << (8 * sz)) - 1);
            total += sz;
            pos += slot;
            continue;
        }
        const bool raw = kind == MCHECKSUM_XDR_RAW || kind == MCHECKSUM_XDR_RAW_LEN;
        const uint64_t len = (kind == MCHECKSUM_XDR_OPAQUE_LEN || kind == MCHECKSUM_XDR_RAW_LEN) ? last : sz;
        if (len > end - pos || (!raw && ((len + 3) & ~3ull) > end - pos)) return false;
        total += len;  // (every field lies inside the message: no overflow)
        pos += raw ? len : (len + 3) & ~3ull;
    }
    *n = total;
    if (wire) *wire = pos - pos0;  // (the size calls: the XDR bytes the schema consumed)
    return true;
}

// One message (one wave, wave-uniform walk): the checksum writes out[m] and
// status[m]; the message operations (XdrOp) end in their own epilogues and
// count failures in lane 0's nbad (add_mismatches).
// fast(p, len, &L, d) may hash an opaque/raw field of len bytes at p itself,
// continuing the running register L (returning true) and, unpack, storing the
// bytes at d; otherwise 64 lane ranges are hashed -- and copied -- byte by
// byte and combined into L.
template <int W, int OP = kXdrChecksum, bool LIST = false, class Fast>
__device__ __forceinline__ void xdr_message(const XdrArgs &a, const XdrMsg &x, uint64_t m, const xdr_reg_t<W> *tab,
                                            uint32_t lane, Fast &&fast, uint32_t &nbad,
                                            const XdrRpcFront &rf = XdrRpcFront{}, const uint64_t *len = nullptr) {
    using R = xdr_reg_t<W>;
    enum : int { WALK = xdr_op_walk(OP) };
    enum : bool {
        RPC = xdr_op_rpc(OP),
        MSG = WALK != kXdrChecksum,
        VERIFY = WALK == kXdrVerify || WALK == kXdrUnpack,
        COPY = WALK == kXdrUnpack
    };
    static_assert(!MSG || W == 32, "the header's hash slot is 32 bits");
    static_assert(WALK != kXdrPack, "the sender's walk is xdr_pack_message");
    static_assert(!LIST || RPC, "the list form: of the RPC frame's calls only");
    const XdrMsgAt at = xdr_msg_at<LIST>(a, len, m);
    uint64_t pos = at.pos;
    const uint64_t end = at.end;
    [[maybe_unused]] const uint64_t m0 = pos;
    R acc = (R)a.init;
    uint64_t last = 0;
    bool bad = end < pos;
    // RPC: the frame's facts for the class.  `bad` is "the walk does not run"
    // until the walk, and "it ran past the message" from then on.
    [[maybe_unused]] uint64_t L = 0, decoded = 0, range = 0;
    [[maybe_unused]] XdrRpcHdr h;
    [[maybe_unused]] bool fits = false;
    if constexpr (RPC) {
        L = LIST ? at.L : mck::rpc_len(pos, end);
        h = xdr_rpc_header(rf, a.buf + pos, L, lane);
        bad = !mck::rpc_xdr_walks(L, h.more, x.pay_off);  // SHORT or DEFERRED: no byte behind the core header is read
        pos += x.pay_off;
    } else if constexpr (MSG) {
        bad = bad || end - pos < x.pay_off;
        pos += x.pay_off;
    }
    // unpack: where the next decoded byte goes.  A message that does not fit
    // its slot is not walked at all: nothing of it is hashed or stored.
    [[maybe_unused]] uint8_t *d = nullptr;
    if constexpr (COPY && RPC) {
        const uint64_t d0 = x.dst_off[m];
        range = mck::rpc_len(d0, x.dst_off[m + 1]);
        fits = !bad && xdr_decoded_len(a, pos, end, &decoded);
        bad = !mck::rpc_xdr_unpacks(L, h.more, x.pay_off, fits, decoded, range);
        d = x.dst + d0;
    } else if constexpr (COPY) {
        const uint64_t d0 = x.dst_off[m], d1 = x.dst_off[m + 1];
        uint64_t n = 0;
        bad = bad || d1 < d0 || !xdr_decoded_len(a, pos, end, &n) || n != d1 - d0;
        d = x.dst + d0;
    }
    [[maybe_unused]] const bool walked = !bad;
    for (uint32_t f = 0; f < a.nf && !bad; f++) {
        const uint32_t kind = a.kind[f], sz = a.size[f];
        if (kind == MCHECKSUM_XDR_SKIP_IF_ZERO) {
            if (last == 0) f += sz;
            continue;
        }
        if (kind == MCHECKSUM_XDR_INT) {
            const uint32_t slot = sz <= 4 ? 4u : 8u;
            if (end - pos < slot) {
                bad = true;
                break;
            }
            uint64_t v = 0;
            for (uint32_t b = 0; b < slot; b++) v = v << 8 | a.buf[pos + b];
            for (uint32_t b = 0; b < sz; b++) acc = (acc >> 8) ^ tab[(uint32_t)(acc ^ (R)(v >> (8 * b))) & 0xFFu];
            if constexpr (COPY) {
                // the host-order image, at any byte address: byte stores from lane 0
                if (lane == 0)
                    for (uint32_t b = 0; b < sz; b++) d[b] = (uint8_t)(v >> (8 * b));
                d += sz;
            }
            last = sz == 8 ? v : v & ((1ull << (8 * sz)) - 1);
            pos += slot;
            continue;
        }
        const bool raw = kind == MCHECKSUM_XDR_RAW || kind == MCHECKSUM_XDR_RAW_LEN;
        const uint64_t len = (kind == MCHECKSUM_XDR_OPAQUE_LEN || kind == MCHECKSUM_XDR_RAW_LEN) ? last : sz;
        if (len > end - pos || (!raw && ((len + 3) & ~3ull) > end - pos)) {
            bad = true;
            break;
        }
        if (!fast(a.buf + pos, len, &acc, d)) {
            R p = 0;
            const uint64_t chunk = (len + 63) / 64;
            const uint64_t lo = lane * chunk < len ? lane * chunk : len, hi = lo + chunk < len ? lo + chunk : len;
            for (uint64_t i = lo; i < hi; i++) {
                const uint8_t byte = a.buf[pos + i];
                if constexpr (COPY) d[i] = byte;  // the lane's own range of the field: no byte outside it
                p = (p >> 8) ^ tab[(uint32_t)(p ^ byte) & 0xFFu];
            }
            p = xdr_shift<W>(a.shift, p, len - hi);
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) p ^= __shfl_xor(p, k, 64);
            acc = xdr_shift<W>(a.shift, acc, len) ^ p;
        }
        if constexpr (COPY) d += len;
        pos += raw ? len : (len + 3) & ~3ull;
    }
    if constexpr (RPC) {
        // The frame's epilogue: the class from launch_plan.h's ladders, the
        // status byte, byte stores for the two hashes; a verifying workgroup
        // counts its classes in LDS (rpc_wg_counts, added once per workgroup).
        uint32_t crc16, wire;
        xdr_rpc_hdr_crc(rf, h.term, lane, &crc16, &wire);
        if (lane == 0) {
            const uint32_t crc = (uint32_t)acc ^ (uint32_t)a.xorout;
            uint32_t cls;
            if constexpr (WALK == kXdrSeal) {
                // (`bad`: the walk did not run, or ran past the message)
                cls = mck::rpc_xdr_seal_class(L, h.more, x.pay_off, !bad);
                uint8_t *msg = const_cast<uint8_t *>(a.buf) + m0;
                if (cls == mck::kRpcOk) store_be32(msg + x.hash_off, crc);
                if (cls != mck::kRpcShort) xdr_rpc_store_crc16(msg, rf.kind, crc16);
            } else {
                // (unpack: the bytes are stored as decoded; both verdicts are known only after them.  A pre-walk
                // that fitted and a walk that then ran past -- the buffer changed under the call -- is SHORT.)
                if constexpr (COPY) fits = fits && !(walked && bad);
                else fits = !bad;
                const bool pay_ok = !bad && load_be32(a.buf + m0 + x.hash_off) == crc;
                if constexpr (COPY)
                    cls = mck::rpc_xdr_unpack_class(L, crc16 == wire, h.more, x.pay_off, fits, decoded, range, pay_ok);
                else cls = mck::rpc_xdr_verify_class(L, crc16 == wire, h.more, x.pay_off, fits, pay_ok);
                atomicAdd(&rpc_wg_counts<COPY ? mck::kRpcCopyClasses : mck::kRpcClasses>()[cls], 1u);
            }
            if (a.status) a.status[m] = (uint8_t)cls;
        }
        return;
    }
    if (lane == 0) {
        const R crc = bad ? (R)0 : acc ^ (R)a.xorout;
        if constexpr (!MSG) {
            reinterpret_cast<R *>(a.out)[m] = crc;
        } else if constexpr (OP == kXdrSeal) {
            // In place: the slot lies in the message's headers, outside every
            // hashed byte, so no value depends on whether another wave's
            // 16-byte loads around a field see its old or its new bytes.
            if (!bad) store_be32(const_cast<uint8_t *>(a.buf) + m0 + x.hash_off, (uint32_t)crc);
        } else {
            // (unpack: the bytes are stored as decoded; the value is known only after them)
            bad = bad || load_be32(a.buf + m0 + x.hash_off) != (uint32_t)crc;
            nbad += bad;
        }
        if (a.status) a.status[m] = bad ? 1 : 0;
    }
}

// Latency layout (small batches): 256-thread workgroups, a byte table only.
template <int W>
__global__ __launch_bounds__(256) void xdr_kernel(XdrArgs a) {
    using R = xdr_reg_t<W>;
    __shared__ R tab[256];
    tab[threadIdx.x] = xdr_tab_entry<W>(a.rpoly, threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    uint32_t nbad = 0;  // (the message operations' count: unused here)
    for (uint64_t m = uniform((uint32_t)(blockIdx.x * 4 + (threadIdx.x >> 6))); m < a.count; m += nw)
        xdr_message<W>(a, XdrMsg{}, m, tab, lane, [](const uint8_t *, uint64_t, R *, uint8_t *) { return false; }, nbad);
}

// The message operations in the latency layout (32-bit models): no wait on
// the device, so nothing to fail closed on.
template <int OP>
__global__ __launch_bounds__(256) void xdr_msg_kernel(XdrMsgArgs ma) {
    const XdrArgs &a = ma.a;
    const XdrMsg &x = ma.x;
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = xdr_tab_entry<32>(a.rpoly, threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    uint32_t nbad = 0;
    for (uint64_t m = uniform((uint32_t)(blockIdx.x * 4 + (threadIdx.x >> 6))); m < a.count; m += nw)
        xdr_message<32, OP>(a, x, m, tab, lane, [](const uint8_t *, uint64_t, uint32_t *, uint8_t *) { return false; },
                            nbad);
    if constexpr (OP != kXdrSeal) add_mismatches(x.mism, nbad);  // once per workgroup (crc_gpu_common.h)
}

// Throughput layout (large batches): persistent 1024-thread workgroups with the
// payload step loop's LDS tables (CRC-32C: the replicated byte tables, one
// workgroup per CU; CRC-64: the 12-lookup tables with combine operators in
// global memory) and the byte table after them; messages from the work queue.
template <int W>
constexpr uint32_t kXdrMainLds = W == 32 ? kL32Bytes : kL64Main;

template <int W, bool NT>
__global__ __launch_bounds__(1024, 1) void xdr_fast_kernel(XdrArgs a) {
    using R = xdr_reg_t<W>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXdrMainLds<W> + 256 * sizeof(R)];
    __shared__ WgQueue wgq;
    R *tab = reinterpret_cast<R *>(lds + kXdrMainLds<W>);
    if (threadIdx.x == 0) wg_queue_init(&wgq, a.queue, a.count);
    if constexpr (W == 32) fill_lds32<false, 1024>(lds, reinterpret_cast<const crc32_gpu_pack_t *>(a.pack));
    else fill_lds64<1024, kOpsGlobal>(lds, reinterpret_cast<const crc64_gpu_pack_t *>(a.pack));
    if (threadIdx.x < 256) tab[threadIdx.x] = xdr_tab_entry<W>(a.rpoly, threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 16u + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * 16u;
    const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u, lc64 = (lane & 31u) << 3;
    auto fast = [&](const uint8_t *p, uint64_t len, R *reg, uint8_t *) -> bool {
        if (len < kXdrFastMin || len >= (1ull << 31)) return false;
        if constexpr (W == 32)
            *reg = payload32_g64<NT, Tab32<false>, true>(Tab32<false>{lds}, reinterpret_cast<const crc32_gpu_pack_t *>(a.pack),
                                                         p, len, lane, lc0, lc1, *reg);
        else
            *reg = payload64_g64<NT, true, kOpsGlobal>(lds, reinterpret_cast<const crc64_gpu_pack_t *>(a.pack), p, len,
                                                       lane, lc64, *reg);
        return true;
    };
    uint32_t nbad = 0;  // (the message operations' count: unused here)
    const bool faulted = for_each_unit<true>(&wgq, a.queue, a.count, wave, nw,
                                             [&](uint64_t m) { xdr_message<W>(a, XdrMsg{}, m, tab, lane, fast, nbad); });
    if (faulted) {  // fail closed: the caller's error word, and every status flagged
        if (lane == 0 && a.err_word) atomicAdd(a.err_word, 1u);
        if (a.status)
            for (uint64_t m = lane; m < a.count; m += 64) a.status[m] = 1;
    }
}

// The message operations in the throughput layout: xdr_fast_kernel's
// workgroups, tables and work queue for the 32-bit models; unpack hashes a
// field of >= kXdrFastMin bytes with the step loop's copying twin, which
// stores it at its place in the destination -- whole 16-byte pieces
// unaligned, edge pieces byte by byte (crc_gpu_pack_store.h).
// Fail closed: a launch whose wait gave up adds 1 to the error word and, where
// there is a counter, `count` to it; its statuses are flagged after the
// launch, once no wave can overwrite them (xdr_flag_kernel).
// (The copying step loop is instantiated for a table type of this kernel's
// own: the segment copy kernels' instance of it -- its inlined fold -- then
// compiles as it did before this kernel called the same template.)
struct XdrTab32 : Tab32<false> {};
template <int OP, bool NT>
__global__ __launch_bounds__(1024, 1) void xdr_msg_fast_kernel(XdrMsgArgs ma) {
    const XdrArgs &a = ma.a;
    const XdrMsg &x = ma.x;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXdrMainLds<32> + 256 * sizeof(uint32_t)];
    __shared__ WgQueue wgq;
    uint32_t *tab = reinterpret_cast<uint32_t *>(lds + kXdrMainLds<32>);
    if (threadIdx.x == 0) wg_queue_init(&wgq, a.queue, a.count);
    const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
    fill_lds32<false, 1024>(lds, pk);
    if (threadIdx.x < 256) tab[threadIdx.x] = xdr_tab_entry<32>(a.rpoly, threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 16u + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * 16u;
    const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
    auto fast = [&](const uint8_t *p, uint64_t len, uint32_t *reg, [[maybe_unused]] uint8_t *d) -> bool {
        if (len < kXdrFastMin || len >= (1ull << 31)) return false;
        if constexpr (OP == kXdrUnpack)
            *reg = payload32_g64<NT, XdrTab32, true, true>(XdrTab32{{lds}}, pk, p, len, lane, lc0, lc1, *reg, d);
        else
            *reg = payload32_g64<NT, Tab32<false>, true>(Tab32<false>{lds}, pk, p, len, lane, lc0, lc1, *reg);
        return true;
    };
    uint32_t nbad = 0;
    const bool faulted = for_each_unit<true>(&wgq, a.queue, a.count, wave, nw,
                                             [&](uint64_t m) { xdr_message<32, OP>(a, x, m, tab, lane, fast, nbad); });
    if (faulted && lane == 0) {
        if (a.err_word) atomicAdd(a.err_word, 1u);
        if (OP != kXdrSeal && x.mism) atomicAdd(x.mism, (uint32_t)a.count);
    }
    if constexpr (OP != kXdrSeal) add_mismatches(x.mism, nbad);  // once per workgroup (crc_gpu_common.h)
}

// After a message operation's throughput launch that held a work-queue slot
// (this launch holds the slot in its place, so the bank is still the call's):
// if a wait of that launch gave up -- its fault flag is claimed -- every
// status becomes 1.  The launch's own waves write verdicts until its end, so
// only a launch after it can leave all of them flagged.  value: what a flagged
// status reads -- 1, or MCHECKSUM_GPU_RPC_FAULT from the calls in the RPC frame.
struct XdrFlagArgs {
    const unsigned long long *queue;
    uint8_t *status;
    uint64_t count;
    uint8_t value;
};
__global__ __launch_bounds__(256) void xdr_flag_kernel(XdrFlagArgs f) {
    if (!__hip_atomic_load(f.queue + kQFault * kQStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    for (uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x; m < f.count; m += (uint64_t)gridDim.x * 256)
        f.status[m] = f.value;
}

// -------------------------------------------------------- XDR encoder ----
//
// mchecksum_gpu_pack_xdr_messages (kXdrPack): unpack's walk with the two
// counters' roles swapped.  The wave reads message m's non-XDR image --
// what unpack writes: every integer's little-endian `size` bytes, every
// opaque or raw field's unpadded bytes -- from src[src_off[m], src_off[m+1]),
// advancing by image strides; it hashes those bytes (they are the hashed
// stream) and stores their XDR encoding from pay_off bytes into message m of
// a.buf on, advancing by XDR strides.  The stores are unpack's: an integer's
// big-endian slot by byte stores from lane 0, a field on the lane-range path
// byte by byte by the lane that hashes it, a field of >= kXdrFastMin bytes in
// the throughput layout by the copying step loop; one lane writes the zero
// pad behind an opaque field.  The encoded length depends on the data, so the
// image's integers are walked once first (xdr_encoded_len): a message whose
// image the schema does not consume exactly, or whose slot is not pay_off +
// the encoded length, is not walked at all -- status 1, no byte written.
// A sibling of xdr_message, not a fifth variant of it: the existing kernels
// keep their source.
struct XdrPack {
    const uint8_t *src;       // the images
    const uint64_t *src_off;  // count + 1 entries
    uint64_t sint;            // bit f: schema entry f is an INT of a signed type (MCHECKSUM_XDR_SINT)
};
struct XdrPackArgs {
    XdrArgs a;
    XdrMsg x;
    XdrPack p;
};

// The little-endian image of an INT of sz bytes at p.
__device__ __forceinline__ uint64_t xdr_image_int(const uint8_t *p, uint32_t sz) {
    uint64_t v = 0;
    for (uint32_t b = 0; b < sz; b++) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

// The XDR length of the image img[0, end): xdr_decoded_len's twin, reading
// the image's INT fields only.  false: the schema runs past the image or
// stops short of its end.
__device__ __forceinline__ bool xdr_encoded_len(const XdrArgs &a, const uint8_t *img, uint64_t end, uint64_t *n) {
    uint64_t last = 0, total = 0, pos = 0;
    for (uint32_t f = 0; f < a.nf; f++) {
        const uint32_t kind = a.kind[f], sz = a.size[f];
        if (kind == MCHECKSUM_XDR_SKIP_IF_ZERO) {
            if (last == 0) f += sz;
            continue;
        }
        if (kind == MCHECKSUM_XDR_INT) {
            if (end - pos < sz) return false;
            last = xdr_image_int(img + pos, sz);
            total += sz <= 4 ? 4u : 8u;
            pos += sz;
            continue;
        }
        const bool raw = kind == MCHECKSUM_XDR_RAW || kind == MCHECKSUM_XDR_RAW_LEN;
        const uint64_t len = (kind == MCHECKSUM_XDR_OPAQUE_LEN || kind == MCHECKSUM_XDR_RAW_LEN) ? last : sz;
        if (len > end - pos) return false;
        total += raw ? len : (len + 3) & ~3ull;  // (len <= the image's length: no overflow)
        pos += len;
    }
    *n = total;
    return pos == end;
}

// One message (one wave, wave-uniform walk).  fast(s, len, &L, d) as in
// xdr_message: it may hash the field of len bytes at s itself, continuing L,
// and store it at d.
// OP: kXdrPack, or kXdrRpcPack -- the RPC frame around the same walk: the
// message's own core header (the caller filled it but for the two hashes) is
// read first, and an image is read only for a message that is eager and whole.
template <int OP = kXdrPack, bool LIST = false, class Fast>
__device__ __forceinline__ void xdr_pack_message(const XdrArgs &a, const XdrMsg &x, const XdrPack &p, uint64_t m,
                                                 const uint32_t *tab, uint32_t lane, Fast &&fast,
                                                 const XdrRpcFront &rf = XdrRpcFront{}, const uint64_t *len = nullptr) {
    static_assert(xdr_op_walk(OP) == kXdrPack, "the sender's walk");
    enum : bool { RPC = xdr_op_rpc(OP) };
    static_assert(!LIST || RPC, "the list form: of the RPC frame's calls only");
    const XdrMsgAt at = xdr_msg_at<LIST>(a, len, m);
    const uint64_t m0 = at.pos, end = at.end;
    const uint64_t s0 = p.src_off[m], s1 = p.src_off[m + 1];
    uint64_t n = 0;
    bool bad;
    [[maybe_unused]] uint64_t L = 0;
    [[maybe_unused]] XdrRpcHdr h;
    [[maybe_unused]] bool exact = false;
    if constexpr (RPC) {
        L = LIST ? at.L : mck::rpc_len(m0, end);
        h = xdr_rpc_header(rf, a.buf + m0, L, lane);
        // (a DEFERRED or SHORT message's source range is not read; a table that runs backwards is an empty image)
        exact = mck::rpc_hashes_payload(L, h.more, x.pay_off) && xdr_encoded_len(a, p.src + s0, mck::rpc_len(s0, s1), &n);
        bad = !mck::rpc_xdr_packs(L, h.more, x.pay_off, exact, n);
    } else {
        bad = end < m0 || s1 < s0 || end - m0 < x.pay_off;
        bad = bad || !xdr_encoded_len(a, p.src + s0, s1 - s0, &n) || n != end - m0 - x.pay_off;
    }
    [[maybe_unused]] const bool packed = !bad;
    const uint8_t *s = p.src + s0;                                // the next image byte
    const uint8_t *const s_end = p.src + (RPC ? s0 + mck::rpc_len(s0, s1) : s1);
    uint8_t *d = const_cast<uint8_t *>(a.buf) + m0 + x.pay_off;  // where the next XDR byte goes
    uint8_t *const d_end = const_cast<uint8_t *>(a.buf) + end;
    uint32_t acc = (uint32_t)a.init;
    uint64_t last = 0;
    for (uint32_t f = 0; f < a.nf && !bad; f++) {
        const uint32_t kind = a.kind[f], sz = a.size[f];
        if (kind == MCHECKSUM_XDR_SKIP_IF_ZERO) {
            if (last == 0) f += sz;
            continue;
        }
        // (the bounds tests again, on both sides: an image changed under the call moves no store out of the slot)
        if (kind == MCHECKSUM_XDR_INT) {
            const uint32_t slot = sz <= 4 ? 4u : 8u;
            if ((uint64_t)(s_end - s) < sz || (uint64_t)(d_end - d) < slot) {
                bad = true;
                break;
            }
            const uint64_t v = xdr_image_int(s, sz);
            for (uint32_t b = 0; b < sz; b++) acc = (acc >> 8) ^ tab[(acc ^ (uint32_t)(v >> (8 * b))) & 0xFFu];
            // xdr_<type>: a signed type's value is sign-extended into its 32-bit word, an unsigned one's zero-extended
            uint64_t w = v;
            if (sz < 8 && ((p.sint >> f) & 1u) && ((v >> (8 * sz - 1)) & 1u)) w |= ~0ull << (8 * sz);
            if (lane == 0)
                for (uint32_t b = 0; b < slot; b++) d[b] = (uint8_t)(w >> (8 * (slot - 1 - b)));
            last = v;
            s += sz;
            d += slot;
            continue;
        }
        const bool raw = kind == MCHECKSUM_XDR_RAW || kind == MCHECKSUM_XDR_RAW_LEN;
        const uint64_t len = (kind == MCHECKSUM_XDR_OPAQUE_LEN || kind == MCHECKSUM_XDR_RAW_LEN) ? last : sz;
        const uint64_t wire = raw ? len : (len + 3) & ~3ull;
        if (len > (uint64_t)(s_end - s) || wire < len || wire > (uint64_t)(d_end - d)) {
            bad = true;
            break;
        }
        if (!fast(s, len, &acc, d)) {
            uint32_t q = 0;
            const uint64_t chunk = (len + 63) / 64;
            const uint64_t lo = lane * chunk < len ? lane * chunk : len, hi = lo + chunk < len ? lo + chunk : len;
            for (uint64_t i = lo; i < hi; i++) {
                const uint8_t byte = s[i];
                d[i] = byte;  // the lane's own range of the field: no byte outside it
                q = (q >> 8) ^ tab[(q ^ byte) & 0xFFu];
            }
            q = xdr_shift<32>(a.shift, q, len - hi);
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) q ^= __shfl_xor(q, k, 64);
            acc = xdr_shift<32>(a.shift, acc, len) ^ q;
        }
        if (lane == 0)
            for (uint64_t i = len; i < wire; i++) d[i] = 0;  // xdr_opaque's pad
        s += len;
        d += wire;
    }
    if constexpr (RPC) {
        uint32_t crc16, wire_hash;
        xdr_rpc_hdr_crc(rf, h.term, lane, &crc16, &wire_hash);
        if (lane == 0) {
            // (an image that changed under the call so that the walk ran past it: MISFIT, its bytes unspecified)
            const uint32_t cls = mck::rpc_xdr_pack_class(L, h.more, x.pay_off, exact && !(packed && bad), n);
            uint8_t *msg = const_cast<uint8_t *>(a.buf) + m0;
            // (the XDR bytes are in place by now: they, the 4 hash bytes and the 2 CRC-16 bytes, no others)
            if (cls == mck::kRpcOk) store_be32(msg + x.hash_off, acc ^ (uint32_t)a.xorout);
            if (cls == mck::kRpcOk || cls == mck::kRpcDeferred) xdr_rpc_store_crc16(msg, rf.kind, crc16);
            if (a.status) a.status[m] = (uint8_t)cls;
        }
        return;
    }
    if (lane == 0) {
        // (the slot lies in the message's headers, outside every XDR byte)
        if (!bad) store_be32(const_cast<uint8_t *>(a.buf) + m0 + x.hash_off, acc ^ (uint32_t)a.xorout);
        if (a.status) a.status[m] = bad ? 1 : 0;
    }
}

// Latency layout: xdr_msg_kernel's workgroups.
__global__ __launch_bounds__(256) void xdr_pack_kernel(XdrPackArgs pa) {
    const XdrArgs &a = pa.a;
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = xdr_tab_entry<32>(a.rpoly, threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t m = uniform((uint32_t)(blockIdx.x * 4 + (threadIdx.x >> 6))); m < a.count; m += nw)
        xdr_pack_message(a, pa.x, pa.p, m, tab, lane, [](const uint8_t *, uint64_t, uint32_t *, uint8_t *) { return false; });
}

// Throughput layout: xdr_msg_fast_kernel's workgroups, tables and work queue;
// fails closed as seal does (the error word here, the statuses by
// xdr_flag_kernel after the launch).  The copying step loop is instantiated
// for a table type of this kernel's own, as for unpack (XdrTab32).
struct XdrPackTab32 : Tab32<false> {};
template <bool NT>
__global__ __launch_bounds__(1024, 1) void xdr_pack_fast_kernel(XdrPackArgs pa) {
    const XdrArgs &a = pa.a;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXdrMainLds<32> + 256 * sizeof(uint32_t)];
    __shared__ WgQueue wgq;
    uint32_t *tab = reinterpret_cast<uint32_t *>(lds + kXdrMainLds<32>);
    if (threadIdx.x == 0) wg_queue_init(&wgq, a.queue, a.count);
    const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
    fill_lds32<false, 1024>(lds, pk);
    if (threadIdx.x < 256) tab[threadIdx.x] = xdr_tab_entry<32>(a.rpoly, threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 16u + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * 16u;
    const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
    auto fast = [&](const uint8_t *s, uint64_t len, uint32_t *reg, uint8_t *d) -> bool {
        if (len < kXdrFastMin || len >= (1ull << 31)) return false;
        *reg = payload32_g64<NT, XdrPackTab32, true, true>(XdrPackTab32{{lds}}, pk, s, len, lane, lc0, lc1, *reg, d);
        return true;
    };
    const bool faulted = for_each_unit<true>(&wgq, a.queue, a.count, wave, nw,
                                             [&](uint64_t m) { xdr_pack_message(a, pa.x, pa.p, m, tab, lane, fast); });
    if (faulted && lane == 0 && a.err_word) atomicAdd(a.err_word, 1u);
}

// ------------------------------------------- XDR walks in the RPC frame ----
//
// mchecksum_gpu_verify_rpc_xdr_messages, _seal_, _unpack_, _pack_: the kernels
// above with the frame's prologue and epilogue around each message's walk
// (xdr_message / xdr_pack_message with an RPC operation), one latency and one
// throughput kernel for the four operations.  Beside their twins' LDS they
// hold the verifying calls' 6 or 7 class counts (rpc_wg_counts, 24 or 28
// bytes); the header pack stays in global memory, as in the plain RPC kernels:
// 6.5 KiB of rows for sixteen 2-byte loads a message do not earn a fill per
// workgroup, and those loads are in flight under the walk.
struct XdrRpcArgs : XdrMsgArgs {
    const void *hdr_pack;  // launch_plan.h, RpcHdrPack: the header model's, of the call's kind
};
struct XdrRpcPackArgs : XdrPackArgs {
    const void *hdr_pack;
};
// The message side by address list (the _rpc_xdr_message_list calls): a.off
// holds the addresses, a.buf is NULL (xdr_msg_at).  Arguments of the list
// kernels' own: the table kernels keep theirs, byte for byte.
struct XdrRpcListArgs : XdrRpcArgs {
    const uint64_t *len;  // count entries
};
struct XdrRpcPackListArgs : XdrRpcPackArgs {
    const uint64_t *len;
};
template <int OP, bool LIST = false>
using xdr_rpc_args_t =
    typename std::conditional<OP == kXdrRpcPack, typename std::conditional<LIST, XdrRpcPackListArgs, XdrRpcPackArgs>::type,
                              typename std::conditional<LIST, XdrRpcListArgs, XdrRpcArgs>::type>::type;
template <bool LIST, class Args>
__device__ __forceinline__ const uint64_t *xdr_rpc_lens([[maybe_unused]] const Args &ra) {
    if constexpr (LIST) return ra.len;
    else return nullptr;
}
template <int OP>
constexpr bool kXdrRpcCounts = OP == kXdrRpcVerify || OP == kXdrRpcUnpack;
template <int OP>
constexpr uint32_t kXdrRpcClasses = OP == kXdrRpcUnpack ? mck::kRpcCopyClasses : mck::kRpcClasses;

template <int OP, bool LIST = false, class Fast>
__device__ __forceinline__ void xdr_rpc_one(const xdr_rpc_args_t<OP, LIST> &ra, const XdrRpcFront &rf, uint64_t m,
                                            const uint32_t *tab, uint32_t lane, Fast &&fast) {
    if constexpr (OP == kXdrRpcPack) {
        xdr_pack_message<OP, LIST>(ra.a, ra.x, ra.p, m, tab, lane, fast, rf, xdr_rpc_lens<LIST>(ra));
    } else {
        uint32_t nbad = 0;  // (the plain frame's count: the classes are counted in LDS)
        xdr_message<32, OP, LIST>(ra.a, ra.x, m, tab, lane, fast, nbad, rf, xdr_rpc_lens<LIST>(ra));
    }
}

// Latency layout: xdr_msg_kernel's workgroups.
template <int OP, bool LIST = false>
__global__ __launch_bounds__(256) void xdr_rpc_kernel(xdr_rpc_args_t<OP, LIST> ra) {
    static_assert(xdr_op_rpc(OP), "the RPC frame's operations");
    const XdrArgs &a = ra.a;
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = xdr_tab_entry<32>(a.rpoly, threadIdx.x);
    const XdrRpcFront rf = xdr_rpc_front(ra.hdr_pack);
    if (kXdrRpcCounts<OP> && threadIdx.x < kXdrRpcClasses<OP>) rpc_wg_counts<kXdrRpcClasses<OP>>()[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t m = uniform((uint32_t)(blockIdx.x * 4 + (threadIdx.x >> 6))); m < a.count; m += nw)
        xdr_rpc_one<OP, LIST>(ra, rf, m, tab, lane, [](const uint8_t *, uint64_t, uint32_t *, uint8_t *) { return false; });
    if constexpr (kXdrRpcCounts<OP>) rpc_add_counts<kXdrRpcClasses<OP>>(ra.x.mism);  // once per workgroup and class
}

// Throughput layout: xdr_msg_fast_kernel's / xdr_pack_fast_kernel's workgroups,
// tables and work queue.  Fail closed: the error word, a verifying call's
// FAULT count, and the statuses after the launch (xdr_flag_kernel with
// MCHECKSUM_GPU_RPC_FAULT).  The copying step loop: a table type of these
// kernels' own, as above.
struct XdrRpcTab32 : Tab32<false> {};
template <int OP, bool NT, bool LIST = false>
__global__ __launch_bounds__(1024, 1) void xdr_rpc_fast_kernel(xdr_rpc_args_t<OP, LIST> ra) {
    static_assert(xdr_op_rpc(OP), "the RPC frame's operations");
    const XdrArgs &a = ra.a;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXdrMainLds<32> + 256 * sizeof(uint32_t)];
    __shared__ WgQueue wgq;
    uint32_t *tab = reinterpret_cast<uint32_t *>(lds + kXdrMainLds<32>);
    if (threadIdx.x == 0) wg_queue_init(&wgq, a.queue, a.count);
    const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
    const XdrRpcFront rf = xdr_rpc_front(ra.hdr_pack);
    fill_lds32<false, 1024>(lds, pk);
    if (threadIdx.x < 256) tab[threadIdx.x] = xdr_tab_entry<32>(a.rpoly, threadIdx.x);
    if (kXdrRpcCounts<OP> && threadIdx.x < kXdrRpcClasses<OP>) rpc_wg_counts<kXdrRpcClasses<OP>>()[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 16u + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * 16u;
    const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
    auto fast = [&](const uint8_t *p, uint64_t len, uint32_t *reg, [[maybe_unused]] uint8_t *d) -> bool {
        if (len < kXdrFastMin || len >= (1ull << 31)) return false;
        if constexpr (OP == kXdrRpcUnpack || OP == kXdrRpcPack)
            *reg = payload32_g64<NT, XdrRpcTab32, true, true>(XdrRpcTab32{{lds}}, pk, p, len, lane, lc0, lc1, *reg, d);
        else
            *reg = payload32_g64<NT, Tab32<false>, true>(Tab32<false>{lds}, pk, p, len, lane, lc0, lc1, *reg);
        return true;
    };
    const bool faulted = for_each_unit<true>(&wgq, a.queue, a.count, wave, nw,
                                             [&](uint64_t m) { xdr_rpc_one<OP, LIST>(ra, rf, m, tab, lane, fast); });
    if (faulted && lane == 0) {
        if (a.err_word) atomicAdd(a.err_word, 1u);
        if (kXdrRpcCounts<OP> && ra.x.mism) atomicAdd(&ra.x.mism[mck::kRpcFault], (uint32_t)a.count);
    }
    if constexpr (kXdrRpcCounts<OP>) rpc_add_counts<kXdrRpcClasses<OP>>(ra.x.mism);
}

// mchecksum_gpu_xdr_encoded_sizes / _decoded_sizes: the pre-walks alone, one
// thread per message -- the INT fields only, with the walks' bounds tests; no
// tables, no queue, no wait.  a.buf / a.off: the images (ENC) or the messages.
struct XdrSizeArgs {
    XdrArgs a;
    uint64_t pay_off;
    uint64_t *sizes, *wire;
};
template <bool ENC>
__global__ __launch_bounds__(256) void xdr_sizes_kernel(XdrSizeArgs s) {
    const XdrArgs &a = s.a;
    for (uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x; m < a.count; m += (uint64_t)gridDim.x * 256) {
        const uint64_t pos = a.off[m], end = a.off[m + 1];
        uint64_t n = 0, w = 0;
        bool ok = end >= pos;
        if constexpr (ENC) ok = ok && xdr_encoded_len(a, a.buf + pos, end - pos, &n);
        else ok = ok && end - pos >= s.pay_off && xdr_decoded_len(a, pos + s.pay_off, end, &n, &w);
        s.sizes[m] = ok ? n : 0;
        if (!ENC && s.wire) s.wire[m] = ok ? w : 0;
        if (a.status) a.status[m] = ok ? 0 : 1;
    }
}

}  // namespace

// ------------------------------------------------------------ host side ----

namespace mck {

// Per-device, per-model extension tables (shift pack for 32/64-bit models,
// byte table for 16-bit ones), built and uploaded once (under g_mu), then
// read without a lock.
int get_ext(DevCtx *c, int idx, const void **out) {
    if (void *p = c->ext[idx].load(std::memory_order_acquire)) {
        *out = p;
        return 0;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (void *p = c->ext[idx].load(std::memory_order_relaxed)) {
        *out = p;
        return 0;
    }
    const mck_model_t &m = mck_models[idx];
    size_t bytes = 0;
    void *host = nullptr;
    int rc = -1;
    if (m.width == 16) {
        bytes = 256 * sizeof(uint16_t);
        uint16_t *t = (uint16_t *)calloc(256, sizeof(uint16_t));
        host = t;
        if (t) {
            const uint32_t rp = (uint32_t)mck_reflect(m.poly, 16);
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t r;
                if (m.reflected) {
                    r = i;
                    for (int k = 0; k < 8; k++) r = r & 1u ? (r >> 1) ^ rp : r >> 1;
                } else {
                    r = i << 8;
                    for (int k = 0; k < 8; k++) r = (r & 0x8000u ? (r << 1) ^ (uint32_t)m.poly : r << 1) & 0xFFFFu;
                }
                t[i] = (uint16_t)r;
            }
            rc = 0;
        }
    } else {
        const crc_rmodel_t rm = gpu_rmodel(idx);
        bytes = m.width == 32 ? sizeof(crc32_shift_pack_t) : sizeof(crc64_shift_pack_t);
        host = calloc(1, bytes);
        if (host)
            rc = m.width == 32 ? crc32_shift_pack_build(&rm, (crc32_shift_pack_t *)host)
                               : crc64_shift_pack_build(&rm, (crc64_shift_pack_t *)host);
    }
    if (rc != 0) {
        free(host);
        return set_err(MCHECKSUM_GPU_EINVAL, "table build failed for %s", m.name);
    }
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess) e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return hip_err(e, "table upload");
    }
    c->ext[idx].store(d, std::memory_order_release);
    *out = d;
    return 0;
}

long long ext_queue_faults() {
    unsigned int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_mck_queue_faults), sizeof(n), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return n;
}

}  // namespace mck

using namespace mck;

extern "C" {

// Test builds (MCK_QFAULT_TEST): MCHECKSUM_GPU_QFAULT_SCAN=b makes scan block
// b give up its look-back -- or, with MCHECKSUM_GPU_QFAULT_MODE=scanstall,
// never publish its descriptor (tests/test_gpu_fail_closed.py); ~0 = none.
uint64_t scan_fault_block() {
    return MCK_QFAULT_TEST ? mck_settings()->qfault_scan : ~0ull;
}
// The scan's look-back epochs: a process-wide counter from a random seed, so a
// workspace's descriptors from any earlier call (this process or, through
// reused memory, another) never match the current call's.
uint64_t scan_epoch() {
    static std::atomic<uint64_t> ctr{[] {
        uint64_t seed = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count() * 0x9E3779B97F4A7C15ull;
        try {
            std::random_device rd;
            seed ^= (uint64_t)rd() << 32 ^ rd();
        } catch (...) {  // no entropy source: the clock alone (never throw through the C ABI)
        }
        return (seed & ((1ull << 60) - 1)) | 1ull;
    }()};
    return ctr.fetch_add(1, std::memory_order_relaxed) & ((1ull << 61) - 1);
}
// (the workspace's layout: seg_work_layout, seg_plan.h)
size_t mchecksum_gpu_segments_work_size(size_t nseg) { return seg_work_bytes(nseg); }

// grid of the per-object launches of an update or verify call (256 threads)
static unsigned seg_elem_grid(uint64_t n) {
    const uint64_t blocks = (n + 255) / 256;
    return blocks > 1024 ? 1024u : (unsigned)blocks;
}

// One segment call: checksum_segments, or with a direction (mck::kSegGather /
// kSegScatter), the contiguous side and its starts table, a copying call.
constexpr int kSegHashOnly = -1;
struct SegCall {
    const char *method;
    const uint64_t *seg_addr, *seg_len;
    size_t nseg;
    const uint64_t *obj_first;
    size_t nobj;
    void *work;
    size_t work_size;
    void *out;
    void *stream;
    int dir = kSegHashOnly;
    void *flat = nullptr;              // gather: the destination; scatter: the source
    const uint64_t *starts = nullptr;  // nobj byte offsets into it
    // what becomes of the objects' registers: values in out; running states in
    // out advanced in place (the update calls); or compared on the device with
    // expected (verify_segments: no out)
    enum Mode { kValues, kUpdate, kVerify } mode = kValues;
    const void *expected = nullptr;
    uint8_t *status = nullptr;
    uint32_t *mism = nullptr;
    // a message call (pack / unpack_segment_messages): flat holds the
    // messages, starts is their nobj + 1 offsets, no out
    bool msg = false;
    size_t pay_off = 0, hash_off = 0;
};

// A message call: its own argument order (the method is an argument, checked
// ahead of the device, as pack_messages does), then the scan, the fit launch,
// the gated copying pass and the seal / compare launch.
static int seg_msg_call(const SegCall &sc) {
    const size_t nseg = sc.nseg, nobj = sc.nobj;
    // an empty batch needs no buffers, the workspace included
    if (nobj && (!sc.obj_first || !sc.work || !sc.flat || !sc.starts || (nseg && (!sc.seg_addr || !sc.seg_len))))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if (sc.hash_off + 4 > sc.pay_off || sc.pay_off > (1u << 30))
        return set_err(MCHECKSUM_GPU_EINVAL, "hash_offset + 4 must not exceed payload_offset");
    if ((uint64_t)nobj > mck::kMaxMsgObjs) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 messages in one call");
    if ((uint64_t)nseg > mck::kMaxVerifySegs)
        return set_err(MCHECKSUM_GPU_EINVAL, "the message calls take fewer than 2^32 segments in one call");
    mck::SegMsgLayout ml{};
    (void)mck::seg_msg_layout(nseg, nobj, &ml);  // (within both caps)
    if (nobj && (sc.work_size < ml.bytes || (uintptr_t)sc.work % 8))
        return set_err(MCHECKSUM_GPU_EINVAL,
                       "workspace smaller than mchecksum_gpu_segment_messages_work_size() or unaligned");
    Model m;
    int rc = resolve_model(sc.method, &m);
    if (rc) return rc;
    if (strcmp(mck_models[m.idx].name, "crc32c") != 0)
        return set_err(MCHECKSUM_GPU_EMETHOD, "the message calls on segment lists take crc32c only");
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    DevCtx *c = nullptr;
    const void *pack = nullptr, *shift = nullptr;
    rc = device_ctx(&c);
    if (!rc) rc = get_pack(c, m.idx, CRC_GPU_MAX_LOG2G, &pack);
    if (!rc) rc = get_ext(c, m.idx, &shift);
    if (rc) return rc;
    if (nobj == 0) return MCHECKSUM_GPU_OK;
    uint64_t *const work = static_cast<uint64_t *>(sc.work);
    SegArgs a{};
    a.addr = sc.seg_addr;
    a.len = sc.seg_len;
    a.nseg = nseg;
    a.first = sc.obj_first;
    a.nobj = nobj;
    a.w = seg_work(sc.work, nseg);
    a.w.map_cap = 0;  // (only the CRC-64 queue pass reads the map)
    a.out = work + ml.acc;
    a.pack = pack;
    a.shift = shift;
    a.err_word = error_word();
    a.epoch = scan_epoch();
    const crc_rmodel_t rm = gpu_rmodel(m.idx);
    ScanArgs sa{};
    sa.len = sc.seg_len;
    sa.addr = sc.seg_addr;
    sa.nseg = nseg;
    sa.epoch = a.epoch;
    sa.first = sc.obj_first;
    sa.nobj = nobj;
    sa.w = a.w;
    sa.w.obj = nullptr;  // (CRC-32C: no object records)
    sa.out = nullptr;    // (the fit launch zeroes the accumulator words)
    sa.width = 32;
    sa.preset = rm.rinit ^ rm.xorout;
    sa.err_word = a.err_word;
    sa.fault_block = scan_fault_block();
    const hipStream_t st = (hipStream_t)sc.stream;
    hipError_t e = launch_kernel(seg_scan, dim3((unsigned)seg_scan_blocks(nseg)), dim3(kScanThreads), st, nullptr, sa);
    if (e != hipSuccess) return hip_err(e, "segment scan launch");
    uint8_t *const buf = static_cast<uint8_t *>(sc.flat);
    const SegMsgArgs ma{{a, buf + sc.pay_off, sc.starts},
                        reinterpret_cast<uint8_t *>(work + ml.gate),
                        buf,
                        sc.starts,
                        sc.pay_off,
                        sc.hash_off,
                        sc.status,
                        sc.mism,
                        (uint32_t)rm.rinit,
                        (uint32_t)rm.xorout};
    e = launch_kernel(seg_msg_pre_kernel, dim3(seg_elem_grid(nobj)), dim3(256), st, nullptr, ma);
    if (e != hipSuccess) return hip_err(e, "segment message fit launch");
    const bool gather = sc.dir == mck::kSegGather;
    SlotRef sr;  // (no work queue: the CRC-32C pass walks static ranges)
    rc = launch_slot(c, sr, gather ? seg_msg_copy_kernel<mck::kSegGather> : seg_msg_copy_kernel<mck::kSegScatter>,
                     (unsigned)c->cus, 1024, sc.stream, ma, "segment message kernel launch");
    if (rc != MCHECKSUM_GPU_OK) return rc;
    e = launch_kernel(gather ? seg_msg_post_kernel<mck::kSegGather> : seg_msg_post_kernel<mck::kSegScatter>,
                      dim3(seg_elem_grid(nobj)), dim3(256), st, nullptr, ma);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, gather ? "segment message seal launch" : "segment message compare launch");
}

// The front of the segment entry points: the argument checks, the scan launch
// and the chunk pass -- seg_kernel, or for a copying call seg_copy_kernel
// under the same launch policy.  An update call seeds the states between the
// two (seg_pre_kernel) and has the same chunk pass XOR into them; verify runs
// the chunk pass on words of the workspace and the compare after it.  (The
// message calls: seg_msg_call.)
static int seg_call(const SegCall &sc) {
    if (sc.msg) return seg_msg_call(sc);
    const bool copy = sc.dir != kSegHashOnly, verify = sc.mode == SegCall::kVerify;
    const size_t nseg = sc.nseg, nobj = sc.nobj;
    if (!sc.obj_first || (nobj && !(verify ? sc.expected : sc.out)) || (nseg && (!sc.seg_addr || !sc.seg_len)) ||
        !sc.work || (copy && nobj && (!sc.flat || !sc.starts)))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if ((uint64_t)nseg > kMaxSegs) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^40 segments in one call");
    mck::SegVerifyLayout vl{};
    if (verify && !mck::seg_verify_layout(nseg, &vl))
        return set_err(MCHECKSUM_GPU_EINVAL, "verify_segments takes fewer than 2^32 segments in one call");
    if (sc.work_size < mchecksum_gpu_segments_work_size(nseg) || (uintptr_t)sc.work % 8)
        return set_err(MCHECKSUM_GPU_EINVAL, "workspace smaller than mchecksum_gpu_segments_work_size() or unaligned");
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    Model m;
    DevCtx *c = nullptr;
    const void *pack = nullptr, *shift = nullptr;
    int rc = resolve_model(sc.method, &m);
    if (!rc) rc = device_ctx(&c);
    if (!rc) rc = get_pack(c, m.idx, CRC_GPU_MAX_LOG2G, &pack);
    if (!rc) rc = get_ext(c, m.idx, &shift);
    if (rc) return rc;
    const int width = m.width;
    if (nobj == 0) return MCHECKSUM_GPU_OK;
    SegArgs a{};
    a.addr = sc.seg_addr;
    a.len = sc.seg_len;
    a.nseg = nseg;
    a.first = sc.obj_first;
    a.nobj = nobj;
    a.w = seg_work(sc.work, nseg);
    // only the CRC-64 queue pass reads the map; MCHECKSUM_GPU_SEG_MAP_CAP caps
    // the part of it used (tests: 0 forces the search over C)
    // (verify keeps its words in the map's tail: seg_verify_layout)
    const uint64_t cap = width == 64 ? (verify ? vl.map_cap : a.w.map_cap) : 0, v = mck_settings()->gpu_seg_map_cap;
    a.w.map_cap = v < cap ? v : cap;
    uint64_t *const work = static_cast<uint64_t *>(sc.work);
    a.out = verify ? static_cast<void *>(work + vl.acc) : sc.out;
    a.pack = pack;
    a.shift = shift;
    a.err_word = error_word();
    a.epoch = scan_epoch();
    // every object starts as the CRC of the empty message, init ^ xorout in
    // the kernels' register form (MSB-first models: byte-reversed, swapped
    // back with the outputs below)
    const crc_rmodel_t rm = gpu_rmodel(m.idx);
    ScanArgs sa{};
    sa.len = sc.seg_len;
    sa.addr = sc.seg_addr;
    sa.nseg = nseg;
    sa.epoch = a.epoch;
    sa.first = sc.obj_first;
    sa.nobj = nobj;
    sa.w = a.w;
    if (width != 64) sa.w.obj = nullptr;  // only the queue pass reads the object records
    sa.out = sc.mode == SegCall::kValues ? sc.out : nullptr;  // (the others: seg_pre_kernel, after the scan)
    sa.width = (uint32_t)width;
    sa.preset = rm.rinit ^ rm.xorout;
    sa.err_word = a.err_word;
    sa.fault_block = scan_fault_block();
    hipError_t e = launch_kernel(seg_scan, dim3((unsigned)seg_scan_blocks(nseg)), dim3(kScanThreads),
                                 (hipStream_t)sc.stream, nullptr, sa);
    if (e != hipSuccess) return hip_err(e, "segment scan launch");
    if (sc.mode != SegCall::kValues) {
        const SegPreArgs pa{sc.obj_first, nobj, nseg, a.epoch, a.w, a.out, shift, rm.rinit};
        auto k = verify ? (width == 32 ? seg_pre_kernel<uint32_t, false> : seg_pre_kernel<uint64_t, false>)
                        : (width == 32 ? seg_pre_kernel<uint32_t, true> : seg_pre_kernel<uint64_t, true>);
        e = launch_kernel(k, dim3(seg_elem_grid(nobj)), dim3(256), (hipStream_t)sc.stream, nullptr, pa);
        if (e != hipSuccess) return hip_err(e, "segment seed launch");
    }
    SlotRef sr;  // only the CRC-64 pass takes chunks from a work queue
    if (width == 64) sr = queue_slot(c, sc.stream);
    a.queue = sr.q;
    if (verify) {
        const SegVerifyArgs va{a, work + vl.chunk_claim, sc.expected, sc.status, sc.mism, rm.rinit, rm.xorout, rm.msb};
        rc = launch_slot(c, sr, width == 32 ? seg_verify_pass_kernel<32> : seg_verify_pass_kernel<64>, (unsigned)c->cus,
                         1024, sc.stream, va, "segment kernel launch");
        if (rc != MCHECKSUM_GPU_OK) return rc;
        e = launch_kernel(width == 32 ? seg_verify_kernel<uint32_t> : seg_verify_kernel<uint64_t>,
                          dim3(seg_elem_grid(nobj)), dim3(256), (hipStream_t)sc.stream, nullptr, va);
        return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "segment verify launch");
    }
    if (!copy) {
        rc = launch_slot(c, sr, width == 32 ? seg_kernel<32> : seg_kernel<64>, (unsigned)c->cus, 1024, sc.stream, a,
                         "segment kernel launch");
    } else {
        const SegCopyArgs ca{a, (uint8_t *)sc.flat, sc.starts};
        const bool gather = sc.dir == mck::kSegGather;
        auto k = width == 32 ? (gather ? seg_copy_kernel<32, mck::kSegGather> : seg_copy_kernel<32, mck::kSegScatter>)
                             : (gather ? seg_copy_kernel<64, mck::kSegGather> : seg_copy_kernel<64, mck::kSegScatter>);
        rc = launch_slot(c, sr, k, (unsigned)c->cus, 1024, sc.stream, ca, "segment copy kernel launch");
    }
    // MSB-first model: the kernels' values are the CRCs byte-swapped
    // (crc_gpu_layout.h); running registers stay in the kernels' form
    if (rc == MCHECKSUM_GPU_OK && m.msb && sc.mode == SegCall::kValues) rc = swap_outputs(sc.out, nobj, width, sc.stream);
    return rc;
}

int mchecksum_gpu_checksum_segments(const char *hash_method, const uint64_t *dev_seg_addr,
                                    const uint64_t *dev_seg_len, size_t nseg, const uint64_t *dev_obj_first,
                                    size_t nobj, void *dev_work, size_t work_size, void *dev_out, void *stream) {
    return seg_call({hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, dev_out,
                     stream});
}

int mchecksum_gpu_gather_segments(const char *hash_method, const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len,
                                  size_t nseg, const uint64_t *dev_obj_first, size_t nobj, void *dev_dst,
                                  const uint64_t *dev_dst_starts, void *dev_work, size_t work_size, void *dev_out,
                                  void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, dev_out, stream};
    sc.dir = mck::kSegGather;
    sc.flat = dev_dst;
    sc.starts = dev_dst_starts;
    return seg_call(sc);
}

int mchecksum_gpu_scatter_segments(const char *hash_method, const void *dev_src, const uint64_t *dev_src_starts,
                                   const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
                                   const uint64_t *dev_obj_first, size_t nobj, void *dev_work, size_t work_size,
                                   void *dev_out, void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, dev_out, stream};
    sc.dir = mck::kSegScatter;
    sc.flat = const_cast<void *>(dev_src);
    sc.starts = dev_src_starts;
    return seg_call(sc);
}

int mchecksum_gpu_update_segments(const char *hash_method, const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len,
                                  size_t nseg, const uint64_t *dev_obj_first, size_t nobj, void *dev_work,
                                  size_t work_size, void *dev_state, void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, dev_state, stream};
    sc.mode = SegCall::kUpdate;
    return seg_call(sc);
}

int mchecksum_gpu_update_gather_segments(const char *hash_method, const uint64_t *dev_seg_addr,
                                         const uint64_t *dev_seg_len, size_t nseg, const uint64_t *dev_obj_first,
                                         size_t nobj, void *dev_dst, const uint64_t *dev_dst_starts, void *dev_work,
                                         size_t work_size, void *dev_state, void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, dev_state, stream};
    sc.dir = mck::kSegGather;
    sc.flat = dev_dst;
    sc.starts = dev_dst_starts;
    sc.mode = SegCall::kUpdate;
    return seg_call(sc);
}

int mchecksum_gpu_update_scatter_segments(const char *hash_method, const void *dev_src, const uint64_t *dev_src_starts,
                                          const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
                                          const uint64_t *dev_obj_first, size_t nobj, void *dev_work, size_t work_size,
                                          void *dev_state, void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, dev_state, stream};
    sc.dir = mck::kSegScatter;
    sc.flat = const_cast<void *>(dev_src);
    sc.starts = dev_src_starts;
    sc.mode = SegCall::kUpdate;
    return seg_call(sc);
}

int mchecksum_gpu_verify_segments(const char *hash_method, const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len,
                                  size_t nseg, const uint64_t *dev_obj_first, size_t nobj, void *dev_work,
                                  size_t work_size, const void *dev_expected, uint8_t *dev_status,
                                  uint32_t *dev_mismatches, void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, nullptr, stream};
    sc.mode = SegCall::kVerify;
    sc.expected = dev_expected;
    sc.status = dev_status;
    sc.mism = dev_mismatches;
    return seg_call(sc);
}

size_t mchecksum_gpu_segment_messages_work_size(size_t nseg, size_t nobj) { return seg_msg_work_bytes(nseg, nobj); }

int mchecksum_gpu_pack_segment_messages(const char *hash_method, const uint64_t *dev_seg_addr,
                                        const uint64_t *dev_seg_len, size_t nseg, const uint64_t *dev_obj_first,
                                        size_t nobj, void *dev_buf, const uint64_t *dev_msg_offsets,
                                        size_t payload_offset, size_t hash_offset, void *dev_work, size_t work_size,
                                        uint8_t *dev_status, void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, nullptr, stream};
    sc.dir = mck::kSegGather;
    sc.flat = dev_buf;
    sc.starts = dev_msg_offsets;
    sc.status = dev_status;
    sc.msg = true;
    sc.pay_off = payload_offset;
    sc.hash_off = hash_offset;
    return seg_call(sc);
}

int mchecksum_gpu_unpack_segment_messages(const char *hash_method, const void *dev_buf,
                                          const uint64_t *dev_msg_offsets, size_t nobj, size_t payload_offset,
                                          size_t hash_offset, const uint64_t *dev_seg_addr,
                                          const uint64_t *dev_seg_len, size_t nseg, const uint64_t *dev_obj_first,
                                          void *dev_work, size_t work_size, uint8_t *dev_status,
                                          uint32_t *dev_mismatches, void *stream) {
    SegCall sc{hash_method, dev_seg_addr, dev_seg_len, nseg, dev_obj_first, nobj, dev_work, work_size, nullptr, stream};
    sc.dir = mck::kSegScatter;
    sc.flat = const_cast<void *>(dev_buf);
    sc.starts = dev_msg_offsets;
    sc.status = dev_status;
    sc.mism = dev_mismatches;
    sc.msg = true;
    sc.pay_off = payload_offset;
    sc.hash_off = hash_offset;
    return seg_call(sc);
}

// verify_core_headers and seal_core_headers: the argument checks, the 16-bit
// model's table and the launch.
static int core_headers_call(const char *hash_method, int kind, const void *dev_buf, const uint64_t *dev_msg_offsets,
                             size_t count, uint8_t *dev_status, uint32_t *dev_mismatches, void *stream, bool seal) {
    if ((count && !dev_buf) || !dev_msg_offsets) return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if (kind != MCHECKSUM_GPU_CORE_HEADER_REQUEST && kind != MCHECKSUM_GPU_CORE_HEADER_RESPONSE)
        return set_err(MCHECKSUM_GPU_EINVAL, "unknown core header kind %d", kind);
    const int idx = mck_model_index(hash_method);
    if (idx < 0)
        return set_err(MCHECKSUM_GPU_EMETHOD, "unknown hash method \"%s\"", hash_method ? hash_method : "(null)");
    const mck_model_t &m = mck_models[idx];
    if (m.width != 16)
        return set_err(MCHECKSUM_GPU_EMETHOD, "core headers carry a 16-bit hash: \"%s\" is not a crc16 model",
                       hash_method);
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    DevCtx *c = nullptr;
    const void *table = nullptr;
    if (int rc = device_ctx(&c)) return rc;
    if (int rc = get_ext(c, idx, &table)) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    HdrArgs a{};
    a.buf = (const uint8_t *)dev_buf;
    a.off = dev_msg_offsets;
    a.count = count;
    a.status = dev_status;
    a.mism = dev_mismatches;
    a.table = (const uint16_t *)table;
    a.kind = (uint32_t)kind;
    a.reflected = (uint32_t)m.reflected;
    a.init = (uint32_t)(m.reflected ? mck_reflect(m.init, 16) : m.init);
    a.xorout = (uint32_t)m.xorout;
    uint64_t blocks = (count + 255) / 256;
    if (blocks > (uint64_t)c->cus * 8) blocks = (uint64_t)c->cus * 8;
    const hipError_t e = launch_kernel(seal ? core_header_seal_kernel : core_header_kernel, dim3((unsigned)blocks),
                                       dim3(256), (hipStream_t)stream, nullptr, a);
    if (e != hipSuccess) return hip_err(e, "core header kernel launch");
    return MCHECKSUM_GPU_OK;
}

int mchecksum_gpu_verify_core_headers(const char *hash_method, int kind, const void *dev_buf,
                                      const uint64_t *dev_msg_offsets, size_t count, uint8_t *dev_status,
                                      uint32_t *dev_mismatches, void *stream) {
    return core_headers_call(hash_method, kind, dev_buf, dev_msg_offsets, count, dev_status, dev_mismatches, stream,
                             false);
}

int mchecksum_gpu_seal_core_headers(const char *hash_method, int kind, void *dev_buf, const uint64_t *dev_msg_offsets,
                                    size_t count, uint8_t *dev_status, void *stream) {
    return core_headers_call(hash_method, kind, dev_buf, dev_msg_offsets, count, dev_status, nullptr, stream, true);
}

// The XDR entry points' schema check; the fields go into the kernel arguments.
// MCHECKSUM_XDR_SINT differs from INT only in the slot the encoder writes: the
// kernels see INT, and the pack call gets the signed fields as a mask (*sint,
// one bit per schema entry: kXdrMaxFields is 64).
static int xdr_schema(const mchecksum_xdr_field_t *fields, size_t nfields, XdrArgs *a, uint64_t *sint = nullptr) {
    if (nfields > kXdrMaxFields) return set_err(MCHECKSUM_GPU_EINVAL, "more than %u schema fields", kXdrMaxFields);
    static_assert(kXdrMaxFields <= 64, "the signed fields ride in a 64-bit mask");
    for (size_t f = 0; f < nfields; f++) {
        uint32_t k = fields[f].kind;
        const uint32_t z = fields[f].size;
        if (k == MCHECKSUM_XDR_SINT) {
            k = MCHECKSUM_XDR_INT;
            if (sint) *sint |= 1ull << f;
        }
        const bool ok = (k == MCHECKSUM_XDR_INT && (z == 1 || z == 2 || z == 4 || z == 8)) ||
                        k == MCHECKSUM_XDR_OPAQUE || k == MCHECKSUM_XDR_RAW || k == MCHECKSUM_XDR_OPAQUE_LEN ||
                        k == MCHECKSUM_XDR_RAW_LEN || (k == MCHECKSUM_XDR_SKIP_IF_ZERO && z <= nfields - f - 1);
        if (!ok) return set_err(MCHECKSUM_GPU_EINVAL, "schema field %zu: bad kind %u / size %u", f, fields[f].kind, z);
        a->kind[f] = k;
        a->size[f] = z;
    }
    a->nf = (uint32_t)nfields;
    return MCHECKSUM_GPU_OK;
}

// The model's words of the walk (register form).
static void xdr_model(int idx, const void *shift, XdrArgs *a) {
    const mck_model_t &m = mck_models[idx];
    a->shift = shift;
    a->rpoly = mck_reflect(m.poly, m.width);
    a->init = mck_reflect(m.init, m.width);
    a->xorout = m.xorout;
}

// throughput layout for batches past a receive queue's worth of RPCs
// (MCHECKSUM_GPU_XDR_FAST=0/1 overrides)
static bool xdr_fast_layout(const mck_settings_t &s, size_t count) {
    return s.gpu_xdr_fast >= 0 ? s.gpu_xdr_fast == 1 : count > kRecvQueueBatch;
}

int mchecksum_gpu_checksum_xdr(const char *hash_method, const mchecksum_xdr_field_t *fields, size_t nfields,
                               const void *dev_buf, const uint64_t *dev_msg_offsets, size_t count, void *dev_out,
                               uint8_t *dev_status, void *stream) {
    if ((nfields && !fields) || !dev_msg_offsets || (count && (!dev_buf || !dev_out)))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    XdrArgs a{};
    if (int rc = xdr_schema(fields, nfields, &a)) return rc;
    Model model;
    const int found = gpu_model(hash_method, &model);
    if (found == -1) return set_err(MCHECKSUM_GPU_EMETHOD, "unknown hash method \"%s\"", hash_method ? hash_method : "(null)");
    if (found < 0 || model.msb)
        return set_err(MCHECKSUM_GPU_EMETHOD, "method \"%s\" has no XDR kernel (reflected 32/64-bit only)", hash_method);
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    const int idx = model.idx, width = model.width;
    DevCtx *c = nullptr;
    const void *shift = nullptr;
    if (int rc = device_ctx(&c)) return rc;
    if (int rc = get_ext(c, idx, &shift)) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    const mck_settings_t &s = *mck_settings();
    const bool fast = xdr_fast_layout(s, count);
    if (fast) {
        const void *pack = nullptr;
        if (int rc = get_pack(c, idx, CRC_GPU_MAX_LOG2G, &pack)) return rc;
        a.pack = pack;
    }
    a.buf = (const uint8_t *)dev_buf;
    a.off = dev_msg_offsets;
    a.count = count;
    a.out = dev_out;
    a.status = dev_status;
    xdr_model(idx, shift, &a);
    if (fast) {
        // non-temporal loads for batches far past the Infinity Cache, sized
        // by count as for offsets batches (MCHECKSUM_GPU_NT=0/1 overrides)
        const bool nt = nt_by_count(s, count);
        a.err_word = error_word();
        uint64_t blocks = (count + 15) / 16;
        if (blocks > (uint64_t)c->cus) blocks = (uint64_t)c->cus;
        SlotRef sr = queue_slot(c, stream);
        a.queue = sr.q;
        auto k = width == 32 ? (nt ? xdr_fast_kernel<32, true> : xdr_fast_kernel<32, false>)
                             : (nt ? xdr_fast_kernel<64, true> : xdr_fast_kernel<64, false>);
        return launch_slot(c, sr, k, (unsigned)blocks, 1024, stream, a, "XDR kernel launch");
    }
    uint64_t blocks = (count + 3) / 4;
    if (blocks > (uint64_t)c->cus * 8) blocks = (uint64_t)c->cus * 8;
    const hipError_t e = launch_kernel(width == 32 ? xdr_kernel<32> : xdr_kernel<64>, dim3((unsigned)blocks), dim3(256),
                                       (hipStream_t)stream, nullptr, a);
    if (e != hipSuccess) return hip_err(e, "XDR kernel launch");
    return MCHECKSUM_GPU_OK;
}

}  // extern "C"

// The kernels of one message operation: the latency layout's, and the
// throughput layout's with default and non-temporal loads.
template <class Args>
struct XdrMsgKernels {
    void (*lat)(Args);
    void (*fast)(Args);
    void (*fast_nt)(Args);
};
#define MCK_XDR_MSG_KERNELS(OP) \
    XdrMsgKernels<XdrMsgArgs> { xdr_msg_kernel<OP>, xdr_msg_fast_kernel<OP, false>, xdr_msg_fast_kernel<OP, true> }

// One message call (verify_xdr_messages, seal_xdr_messages,
// unpack_xdr_messages, pack_xdr_messages, and the four in the RPC frame): the
// argument checks in the header's order, then checksum_xdr's choice of layout,
// slot and loads.
// Args: the operation's kernel arguments (XdrMsgArgs; pack: XdrPackArgs; the
// RPC frame's: XdrRpcArgs, XdrRpcPackArgs, and by address list XdrRpcListArgs,
// XdrRpcPackListArgs).
struct XdrMsgCall {
    XdrOp op;
    const char *method;
    const mchecksum_xdr_field_t *fields;
    size_t nfields;
    const void *buf;
    const uint64_t *off;
    size_t count, pay_off, hash_off;
    uint8_t *status;
    void *stream;
    void *dst = nullptr;
    const uint64_t *dst_off = nullptr;
    uint32_t *mism = nullptr;
    const void *src = nullptr;  // pack: the images and their table
    const uint64_t *src_off = nullptr;
    // the RPC frame (xdr_op_rpc(op)): the core header's layout and its 16-bit model
    int kind = 0;
    const char *hdr_method = nullptr;
    // the message side by address list (the RPC frame's _list calls, told by their Args): `off` holds the count
    // addresses, `len` the lengths, `buf` is unused -- the kernels run from base 0 (xdr_msg_at)
    const uint64_t *len = nullptr;
};
template <class Args>
constexpr bool kXdrListArgs = std::is_base_of_v<XdrRpcListArgs, Args> || std::is_base_of_v<XdrRpcPackListArgs, Args>;

template <class Args>
static int xdr_msg_call(const XdrMsgCall &mc, const XdrMsgKernels<Args> &ks) {
    const size_t count = mc.count;
    const bool rpc = xdr_op_rpc(mc.op);
    const bool unpack = xdr_op_walk(mc.op) == kXdrUnpack, pack = xdr_op_walk(mc.op) == kXdrPack;
    constexpr bool list = kXdrListArgs<Args>;
    const bool no_msgs = list ? !mc.off || !mc.len : !mc.buf || !mc.off;
    if ((mc.nfields && !mc.fields) ||
        (count && (no_msgs || (unpack && (!mc.dst || !mc.dst_off)) || (pack && (!mc.src || !mc.src_off)))))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if (rpc && mc.kind != MCHECKSUM_GPU_CORE_HEADER_REQUEST && mc.kind != MCHECKSUM_GPU_CORE_HEADER_RESPONSE)
        return set_err(MCHECKSUM_GPU_EINVAL, "unknown core header kind %d", mc.kind);
    if (rpc && (mc.hash_off < mck::kRpcHdrBytes || mc.hash_off > mck::kMaxHashOff))
        return set_err(MCHECKSUM_GPU_EINVAL, "hash_offset must lie behind the core header and be at most 2^30");
    if (mc.hash_off > mc.pay_off || mc.pay_off - mc.hash_off < 4)
        return set_err(MCHECKSUM_GPU_EINVAL, "hash_offset + 4 must not exceed payload_offset");
    if ((uint64_t)count > (1ull << 31)) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 messages in one call");
    Args ma{};
    XdrArgs &a = ma.a;
    uint64_t sint = 0;
    if (int rc = xdr_schema(mc.fields, mc.nfields, &a, &sint)) return rc;
    Model model;
    const int found = gpu_model(mc.method, &model);
    if (found == -1)
        return set_err(MCHECKSUM_GPU_EMETHOD, "unknown hash method \"%s\"", mc.method ? mc.method : "(null)");
    if (found < 0 || model.msb || model.width != 32)
        return set_err(MCHECKSUM_GPU_EMETHOD,
                       "the message header carries a 32-bit hash: \"%s\" is not a reflected 32-bit method", mc.method);
    int hdr_idx = -1;
    if (rpc) {
        hdr_idx = mck_model_index(mc.hdr_method);
        if (hdr_idx < 0)
            return set_err(MCHECKSUM_GPU_EMETHOD, "unknown hash method \"%s\"", mc.hdr_method ? mc.hdr_method : "(null)");
        if (mck_models[hdr_idx].width != 16)
            return set_err(MCHECKSUM_GPU_EMETHOD, "core headers carry a 16-bit hash: \"%s\" is not a crc16 model", mc.hdr_method);
    }
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    DevCtx *c = nullptr;
    const void *shift = nullptr;
    if (int rc = device_ctx(&c)) return rc;
    if (int rc = get_ext(c, model.idx, &shift)) return rc;
    if constexpr (std::is_base_of_v<XdrRpcArgs, Args> || std::is_base_of_v<XdrRpcPackArgs, Args>) {
        // (an empty batch too builds its tables: the plain RPC calls' pack, shared with them)
        if (int rc = get_rpc_pack(c, hdr_idx, mc.kind, &ma.hdr_pack)) return rc;
    }
    if (count == 0) return MCHECKSUM_GPU_OK;
    const mck_settings_t &s = *mck_settings();
    const bool fast = xdr_fast_layout(s, count);
    if (fast) {
        const void *pack = nullptr;
        if (int rc = get_pack(c, model.idx, CRC_GPU_MAX_LOG2G, &pack)) return rc;
        a.pack = pack;
    }
    a.buf = list ? nullptr : (const uint8_t *)mc.buf;
    a.off = mc.off;
    if constexpr (list) ma.len = mc.len;
    a.count = count;
    a.status = mc.status;
    xdr_model(model.idx, shift, &a);
    ma.x = XdrMsg{mc.pay_off, mc.hash_off, (uint8_t *)mc.dst, mc.dst_off, mc.mism};
    if constexpr (std::is_base_of_v<XdrPackArgs, Args>) ma.p = XdrPack{(const uint8_t *)mc.src, mc.src_off, sint};
    if (!fast) {
        uint64_t blocks = (count + 3) / 4;
        if (blocks > (uint64_t)c->cus * 8) blocks = (uint64_t)c->cus * 8;
        const hipError_t e = launch_kernel(ks.lat, dim3((unsigned)blocks), dim3(256), (hipStream_t)mc.stream, nullptr, ma);
        return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "XDR message kernel launch");
    }
    a.err_word = error_word();
    uint64_t blocks = (count + 15) / 16;
    if (blocks > (uint64_t)c->cus) blocks = (uint64_t)c->cus;
    SlotRef sr = queue_slot(c, mc.stream);
    a.queue = sr.q;
    const auto k = nt_by_count(s, count) ? ks.fast_nt : ks.fast;
    // Without a slot (a captured call: static split, no wait on the device)
    // or without statuses there is nothing to flag after the launch.
    if (!sr.q || !mc.status) return launch_slot(c, sr, k, (unsigned)blocks, 1024, mc.stream, ma, "XDR message kernel launch");
    // Fail closed: the flagging launch takes over the slot -- its completion
    // frees it -- so the bank it reads is still this call's.
    const hipError_t e = launch_kernel(k, dim3((unsigned)blocks), dim3(1024), (hipStream_t)mc.stream, nullptr, ma);
    if (e != hipSuccess) {
        slot_unissue(c, sr);
        return hip_err(e, "XDR message kernel launch");
    }
    uint64_t fb = (count + 4095) / 4096;
    if (fb > (uint64_t)c->cus * 4) fb = (uint64_t)c->cus * 4;
    const uint8_t flag = rpc ? (uint8_t)MCHECKSUM_GPU_RPC_FAULT : (uint8_t)1;
    return launch_slot(c, sr, xdr_flag_kernel, (unsigned)fb, 256, mc.stream, XdrFlagArgs{sr.q, mc.status, count, flag},
                       "XDR status launch");
}

extern "C" {

int mchecksum_gpu_verify_xdr_messages(const char *hash_method, const mchecksum_xdr_field_t *fields, size_t nfields,
                                      const void *dev_buf, const uint64_t *dev_msg_offsets, size_t count,
                                      size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
                                      uint32_t *dev_mismatches, void *stream) {
    XdrMsgCall mc{kXdrVerify, hash_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset, hash_offset,
                  dev_status, stream};
    mc.mism = dev_mismatches;
    return xdr_msg_call(mc, MCK_XDR_MSG_KERNELS(kXdrVerify));
}

int mchecksum_gpu_seal_xdr_messages(const char *hash_method, const mchecksum_xdr_field_t *fields, size_t nfields,
                                    void *dev_buf, const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                    size_t hash_offset, uint8_t *dev_status, void *stream) {
    return xdr_msg_call({kXdrSeal, hash_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset,
                         hash_offset, dev_status, stream},
                        MCK_XDR_MSG_KERNELS(kXdrSeal));
}

int mchecksum_gpu_unpack_xdr_messages(const char *hash_method, const mchecksum_xdr_field_t *fields, size_t nfields,
                                      const void *dev_buf, const uint64_t *dev_msg_offsets, size_t count,
                                      size_t payload_offset, size_t hash_offset, void *dev_dst,
                                      const uint64_t *dev_dst_offsets, uint8_t *dev_status, uint32_t *dev_mismatches,
                                      void *stream) {
    XdrMsgCall mc{kXdrUnpack, hash_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset, hash_offset,
                  dev_status, stream};
    mc.dst = dev_dst;
    mc.dst_off = dev_dst_offsets;
    mc.mism = dev_mismatches;
    return xdr_msg_call(mc, MCK_XDR_MSG_KERNELS(kXdrUnpack));
}

int mchecksum_gpu_pack_xdr_messages(const char *hash_method, const mchecksum_xdr_field_t *fields, size_t nfields,
                                    const void *dev_src, const uint64_t *dev_src_offsets, void *dev_buf,
                                    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                    size_t hash_offset, uint8_t *dev_status, void *stream) {
    XdrMsgCall mc{kXdrPack, hash_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset, hash_offset,
                  dev_status, stream};
    mc.src = dev_src;
    mc.src_off = dev_src_offsets;
    return xdr_msg_call(mc, XdrMsgKernels<XdrPackArgs>{xdr_pack_kernel, xdr_pack_fast_kernel<false>,
                                                       xdr_pack_fast_kernel<true>});
}

// The size calls: one launch of the pre-walk, nothing of the device context
// (no tables, no slot), so they can be captured without prepare().
static int xdr_sizes_call(bool enc, const mchecksum_xdr_field_t *fields, size_t nfields, const void *buf,
                          const uint64_t *off, size_t count, size_t pay_off, uint64_t *sizes, uint64_t *wire,
                          uint8_t *status, void *stream) {
    if ((nfields && !fields) || (count && (!buf || !off || !sizes)))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if ((uint64_t)count > (1ull << 31)) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 messages in one call");
    XdrSizeArgs s{};
    if (int rc = xdr_schema(fields, nfields, &s.a)) return rc;
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    if (count == 0) return MCHECKSUM_GPU_OK;
    s.a.buf = (const uint8_t *)buf;
    s.a.off = off;
    s.a.count = count;
    s.a.status = status;
    s.pay_off = pay_off;
    s.sizes = sizes;
    s.wire = wire;
    uint64_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const hipError_t e = launch_kernel(enc ? xdr_sizes_kernel<true> : xdr_sizes_kernel<false>, dim3((unsigned)blocks),
                                       dim3(256), (hipStream_t)stream, nullptr, s);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "XDR sizes kernel launch");
}

int mchecksum_gpu_xdr_encoded_sizes(const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_src,
                                    const uint64_t *dev_src_offsets, size_t count, uint64_t *dev_sizes,
                                    uint8_t *dev_status, void *stream) {
    return xdr_sizes_call(true, fields, nfields, dev_src, dev_src_offsets, count, 0, dev_sizes, nullptr, dev_status,
                          stream);
}

int mchecksum_gpu_xdr_decoded_sizes(const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_buf,
                                    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                    uint64_t *dev_sizes, uint64_t *dev_wire_sizes, uint8_t *dev_status, void *stream) {
    return xdr_sizes_call(false, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset, dev_sizes,
                          dev_wire_sizes, dev_status, stream);
}

// The four calls in the RPC frame: whole RPC messages of an XDR build.
#define MCK_XDR_RPC_KERNELS(OP) \
    XdrMsgKernels<xdr_rpc_args_t<OP>> { xdr_rpc_kernel<OP>, xdr_rpc_fast_kernel<OP, false>, xdr_rpc_fast_kernel<OP, true> }

int mchecksum_gpu_verify_rpc_xdr_messages(const char *header_method, const char *payload_method, int kind,
                                          const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_buf,
                                          const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                          size_t hash_offset, uint8_t *dev_status, uint32_t *dev_counts, void *stream) {
    XdrMsgCall mc{kXdrRpcVerify, payload_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset,
                  hash_offset, dev_status, stream};
    mc.mism = dev_counts;
    mc.kind = kind;
    mc.hdr_method = header_method;
    return xdr_msg_call(mc, MCK_XDR_RPC_KERNELS(kXdrRpcVerify));
}

int mchecksum_gpu_seal_rpc_xdr_messages(const char *header_method, const char *payload_method, int kind,
                                        const mchecksum_xdr_field_t *fields, size_t nfields, void *dev_buf,
                                        const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                        size_t hash_offset, uint8_t *dev_status, void *stream) {
    XdrMsgCall mc{kXdrRpcSeal, payload_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset,
                  hash_offset, dev_status, stream};
    mc.kind = kind;
    mc.hdr_method = header_method;
    return xdr_msg_call(mc, MCK_XDR_RPC_KERNELS(kXdrRpcSeal));
}

int mchecksum_gpu_unpack_rpc_xdr_messages(const char *header_method, const char *payload_method, int kind,
                                          const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_buf,
                                          const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                          size_t hash_offset, void *dev_dst, const uint64_t *dev_dst_offsets,
                                          uint8_t *dev_status, uint32_t *dev_counts, void *stream) {
    XdrMsgCall mc{kXdrRpcUnpack, payload_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset,
                  hash_offset, dev_status, stream};
    mc.dst = dev_dst;
    mc.dst_off = dev_dst_offsets;
    mc.mism = dev_counts;
    mc.kind = kind;
    mc.hdr_method = header_method;
    return xdr_msg_call(mc, MCK_XDR_RPC_KERNELS(kXdrRpcUnpack));
}

int mchecksum_gpu_pack_rpc_xdr_messages(const char *header_method, const char *payload_method, int kind,
                                        const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_src,
                                        const uint64_t *dev_src_offsets, void *dev_buf, const uint64_t *dev_msg_offsets,
                                        size_t count, size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
                                        void *stream) {
    XdrMsgCall mc{kXdrRpcPack, payload_method, fields, nfields, dev_buf, dev_msg_offsets, count, payload_offset,
                  hash_offset, dev_status, stream};
    mc.src = dev_src;
    mc.src_off = dev_src_offsets;
    mc.kind = kind;
    mc.hdr_method = header_method;
    return xdr_msg_call(mc, MCK_XDR_RPC_KERNELS(kXdrRpcPack));
}

}  // extern "C"

// The four calls above with the message side by address list: the same call
// (checks, layout, slot, flag launch), the kernels' LIST twins.
#define MCK_XDR_RPC_LIST_KERNELS(OP)                                                                         \
    XdrMsgKernels<xdr_rpc_args_t<OP, true>> {                                                                \
        xdr_rpc_kernel<OP, true>, xdr_rpc_fast_kernel<OP, false, true>, xdr_rpc_fast_kernel<OP, true, true> \
    }

static XdrMsgCall xdr_rpc_list_call(XdrOp op, const char *header_method, const char *payload_method, int kind,
                                    const mchecksum_xdr_field_t *fields, size_t nfields, const uint64_t *addr,
                                    const uint64_t *len, size_t count, size_t pay_off, size_t hash_off, uint8_t *status,
                                    void *stream) {
    XdrMsgCall mc{op, payload_method, fields, nfields, nullptr, addr, count, pay_off, hash_off, status, stream};
    mc.kind = kind;
    mc.hdr_method = header_method;
    mc.len = len;
    return mc;
}

extern "C" {

int mchecksum_gpu_verify_rpc_xdr_message_list(const char *header_method, const char *payload_method, int kind,
                                              const mchecksum_xdr_field_t *fields, size_t nfields,
                                              const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
                                              size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
                                              uint32_t *dev_counts, void *stream) {
    XdrMsgCall mc = xdr_rpc_list_call(kXdrRpcVerify, header_method, payload_method, kind, fields, nfields, dev_msg_addr,
                                      dev_msg_len, count, payload_offset, hash_offset, dev_status, stream);
    mc.mism = dev_counts;
    return xdr_msg_call(mc, MCK_XDR_RPC_LIST_KERNELS(kXdrRpcVerify));
}

int mchecksum_gpu_seal_rpc_xdr_message_list(const char *header_method, const char *payload_method, int kind,
                                            const mchecksum_xdr_field_t *fields, size_t nfields,
                                            const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
                                            size_t payload_offset, size_t hash_offset, uint8_t *dev_status, void *stream) {
    const XdrMsgCall mc = xdr_rpc_list_call(kXdrRpcSeal, header_method, payload_method, kind, fields, nfields,
                                            dev_msg_addr, dev_msg_len, count, payload_offset, hash_offset, dev_status,
                                            stream);
    return xdr_msg_call(mc, MCK_XDR_RPC_LIST_KERNELS(kXdrRpcSeal));
}

int mchecksum_gpu_unpack_rpc_xdr_message_list(const char *header_method, const char *payload_method, int kind,
                                              const mchecksum_xdr_field_t *fields, size_t nfields,
                                              const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
                                              size_t payload_offset, size_t hash_offset, void *dev_dst,
                                              const uint64_t *dev_dst_offsets, uint8_t *dev_status, uint32_t *dev_counts,
                                              void *stream) {
    XdrMsgCall mc = xdr_rpc_list_call(kXdrRpcUnpack, header_method, payload_method, kind, fields, nfields, dev_msg_addr,
                                      dev_msg_len, count, payload_offset, hash_offset, dev_status, stream);
    mc.dst = dev_dst;
    mc.dst_off = dev_dst_offsets;
    mc.mism = dev_counts;
    return xdr_msg_call(mc, MCK_XDR_RPC_LIST_KERNELS(kXdrRpcUnpack));
}

int mchecksum_gpu_pack_rpc_xdr_message_list(const char *header_method, const char *payload_method, int kind,
                                            const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_src,
                                            const uint64_t *dev_src_offsets, const uint64_t *dev_msg_addr,
                                            const uint64_t *dev_msg_len, size_t count, size_t payload_offset,
                                            size_t hash_offset, uint8_t *dev_status, void *stream) {
    XdrMsgCall mc = xdr_rpc_list_call(kXdrRpcPack, header_method, payload_method, kind, fields, nfields, dev_msg_addr,
                                      dev_msg_len, count, payload_offset, hash_offset, dev_status, stream);
    mc.src = dev_src;
    mc.src_off = dev_src_offsets;
    return xdr_msg_call(mc, MCK_XDR_RPC_LIST_KERNELS(kXdrRpcPack));
}

}  // extern "C"
