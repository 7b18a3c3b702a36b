// crc_gpu_queue.h -- the batch kernels' work queue, device side: the
// per-workgroup LDS state, chunk fetch and publish, the bounded waits with
// their fault and trace globals, and the loops that hand a wave its units
// (UnitTaker, for_each_unit).  Layout constants: crc_gpu_shape.h; the chunk
// plan: crc_gpu_plan.h.
#ifndef CRC_GPU_QUEUE_H
#define CRC_GPU_QUEUE_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "crc_gpu_plan.h"
#include "crc_gpu_shape.h"

#ifndef MCK_TRACE
#define MCK_TRACE 0
#endif

namespace {

// ------------------------------------------------------------ work queue --
// Dynamic distribution of payloads over waves.  With a static assignment the
// waves of one 4 GiB launch finish between 566 and 642 us (p10..max; the XCDs
// stream at different rates, profiles/r01/tail_trace.json), so the slowest
// wave sets the launch time.  Per-wave tickets from global counters do not
// work: device-scope atomics on one address retire ~1 per 45 ns on MI355X,
// so 8 per-XCD counters fed one ticket per payload group throttled C2 2.6x.
//
// Two levels instead.  Units [0, n) form chunks (ChunkPlan, crc_gpu_plan.h); the chunk
// ids are dealt round-robin to 8 sub-queues (one per XCD by blockIdx % 8, the
// dispatch order), each a global counter on its own 256-B line.  A workgroup
// takes whole chunks (one device-scope atomic per chunk, stealing from the
// next sub-queue once its own is drained) and its waves take the chunk's
// units one at a time through an LDS counter.  The wave that takes the slot a
// quarter chunk before the end fetches the NEXT chunk -- after reading its own
// chunk id, so fetches run in chunk order and the first "no more chunks" is
// final -- and the fetch's latency hides under the rest of the chunk.  Chunk
// ids pass through a small LDS ring whose entries are recycled only after all
// readers of the previous occupant have read it (the host hands each launch a
// slot of its stream's own, mchecksum_gpu.hip).  tests/test_queue_model.py
// runs the same protocol on the CPU under random interleavings.
//
// Two banks per slot (round 3).  Launch s on a slot counts in bank s & 1 (the
// host passes that bank) and, from its first workgroup at entry, zeroes the
// protocol lines of the OTHER bank, which the slot's next launch will use --
// launches on a slot never overlap, so nobody is using that bank.  Round 2
// instead had the launch's last group zero its own bank at exit, behind a
// hierarchical exit count (LDS per workgroup, a line per group, one per
// slot): three dependent device-scope atomics, the zeroing and a wait after
// the last wave's last payload, on every launch's critical path.  Round 3
// kept one non-returning add per workgroup on a completion line, summed by the
// host (a device round trip) before it gave a slot to another stream; round 4
// records a HIP event at each slot launch's completion instead
// (hipExtLaunchKernel's stop event, queried without blocking, queue_slot), so
// a workgroup's exit touches no slot line.
// Bank layout (one counter per 256-B line, 8 KiB per bank, 16 KiB-aligned
// slots): [0, 8) sub-queue tickets, [8] fault flag of the launch (claimed by
// its first faulting wave, which reports), [9] abort flag (set by any wave
// whose bounded wait gave up; every later wait of the launch then gives up at
// once, so one call spends at most one deadline however many stalls it meets)
// -- all zeroed by the previous launch on the slot.
//
// Exclusivity.  A slot serves one launch at a time: the host hands the queue
// only to eager launches, each on a slot of its stream's own (launches on one
// stream never overlap).  Launches it cannot give an exclusive slot -- graph
// captures (every replay reuses the captured arguments, and two execs of one
// capture may replay at once) and streams past the per-stream table -- get
// no slot and take the static split (units wave, wave + #waves, ...).  (Round
// 2 had such launches claim a shared slot with a tag; a launch whose early
// workgroups found the slot busy and later ones found it free never released
// it, and its next replay -- same tag -- ran on stale counters and skipped
// units: one wrong batch in 400 concurrent replays.  The XOR-accumulating
// kernels (split CRC-64 pieces, scatter-gather chunks) also cannot tolerate
// the units such mixed launches hashed twice.)

struct WgQueue {
    unsigned int slot;     // next (chunk, unit) slot of this workgroup
    unsigned int drained;  // sub-queues (counted from home) found empty
    unsigned int busy;     // 1: no slot for this launch -> static split
    unsigned int reads[kWgRing];
    unsigned long long entry[kWgRing];  // (chunk seq << 32) | global chunk id
};

// (readfirstlane returns int: widen each half as uint32_t, or a low half with
// bit 31 set would sign-extend over the high half)
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    return (uint64_t)hi << 32 | lo;
}

template <class T>
__device__ __forceinline__ T lds_ld(T *p) {
    return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <class T>
__device__ __forceinline__ void lds_st(T *p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Every wait in the queue protocol is bounded in time: a wait still unmet
// after kWaitTicks of the constant 100 MHz real-time counter (1 s; or a wave
// that takes more slots than the launch has) counts a fault in
// g_mck_queue_faults (read by mchecksum_gpu_queue_faults()) and leaves the
// loop, so a protocol failure shows up as a fault count and a failed call
// instead of a wedged GPU.  Diagnostic builds (-DMCK_TRACE=1) also record
// where (g_mck_qdiag).
__device__ unsigned int g_mck_queue_faults;
#if MCK_TRACE
__device__ unsigned long long g_mck_qdiag[4 * 64];
__device__ unsigned int g_mck_qdiag_n;
// per wave: fetches, fetch ticks (sum), fetch ticks (max), entry-wait ticks
__device__ unsigned long long g_mck_qwave[6 * 16384];
// per unit (u < 2^17): completion time | (blockIdx % 8) << 60 (tools/unit_timeline.py)
__device__ unsigned long long g_mck_unit_end[1u << 17];
#endif
__device__ __noinline__ void queue_fault(uint32_t kind, uint64_t a, uint64_t b) {
    atomicAdd(&g_mck_queue_faults, 1u);
#if MCK_TRACE
    const unsigned int i = atomicAdd(&g_mck_qdiag_n, 1u);
    if (i < 64) {
        g_mck_qdiag[4 * i] = kind;
        g_mck_qdiag[4 * i + 1] = blockIdx.x * 64ull + (threadIdx.x >> 6);
        g_mck_qdiag[4 * i + 2] = a;
        g_mck_qdiag[4 * i + 3] = b;
    }
#else
    (void)kind;
    (void)a;
    (void)b;
#endif
}
// A wait's deadline, on wall_clock64() -- the 100 MHz real-time counter,
// independent of the shader clock and of how slow each poll gets under
// contention (round 4's reverted in-kernel zeroing hung with 8192 waves
// polling one line: an iteration count had bounded nothing).  The counter is
// read on every 16th poll only (the polls stay tight: the ring-entry wait sits
// on the path of every unit taken) and the first read starts the clock.
//  * Preemption: a gap of more than kGapTicks between two reads (16 polls
//    take microseconds) means the wave was switched out -- CWSR, when other
//    processes share the GPU -- and that time does not count, so a healthy
//    launch resumed after a long preemption does not fail closed at once.
//  * Abort: the launch's abort flag (kQAbort; nullptr for waits outside the
//    queue) is read with the counter; once any wait of the launch has given
//    up, every other one gives up at its next read, so a call meets at most
//    one deadline however many stalls it has.
#ifndef MCK_WAIT_TICKS
#define MCK_WAIT_TICKS 100000000ull  // 1 s at 100 MHz
#endif
constexpr uint64_t kWaitTicks = MCK_WAIT_TICKS;
constexpr uint64_t kGapTicks = 5000000ull;  // 50 ms
struct Deadline {
    const unsigned long long *abort = nullptr;
    uint64_t t0 = 0, last = 0;
    uint32_t polls = 0;
    __device__ explicit Deadline(const unsigned long long *abort_word = nullptr) : abort(abort_word) {}
    // true once this wait has lasted kWaitTicks, or the launch aborted (call once per poll)
    __device__ __forceinline__ bool passed() {
        if ((++polls & 15u) != 1u) return false;
        const uint64_t now = wall_clock64();
        if (polls == 1u) {
            t0 = last = now;
            return abort && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (now - last > kGapTicks) t0 += now - last;  // switched out: not waiting time
        last = now;
        return now - t0 > kWaitTicks || (abort && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
};
// The launch's abort flag in its bank (queue non-null), set by a wave whose wait gave up.
__device__ __forceinline__ unsigned long long *abort_word(unsigned long long *q) { return q + kQAbort * kQStride; }
__device__ __forceinline__ void raise_abort(unsigned long long *q) {
    if (q) __hip_atomic_store(abort_word(q), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#define MCK_WAIT_GUARD(dl, kind, A_, B_) \
    if ((dl).passed()) {                 \
        queue_fault(kind, A_, B_);       \
        break;                           \
    }

#if MCK_QFAULT_TEST
// Test builds: which failure the qfault library injects (set from
// MCHECKSUM_GPU_QFAULT_MODE before every launch, gpu_host.h): 0 = a wave gives
// up one unit without waiting (workgroup 3, the first unit of its second
// chunk; in the segment scan, block MCHECKSUM_GPU_QFAULT_SCAN gives up its
// look-back); 1 = "stall": workgroup 3 never publishes its third chunk, so its
// waves wait out the deadline; 2 = "scanstall": segment-scan block
// MCHECKSUM_GPU_QFAULT_SCAN never publishes its look-back descriptor, so its
// successors wait out theirs; 3 = "stall+scanstall": both in one call.
__device__ unsigned int g_mck_qfault_mode;
#endif

// Steal order: thieves of one home start at different victims.  On since
// round 3: never slower in four one-process A/Bs over rounds 3-4 (headline
// +0.1 to +0.2%, C4 +0.14 to +0.55%; profiles/r03/ab_steal_rot*.log,
// profiles/r04/ab_qmask.log) -- gains inside the run-to-run band, kept because
// the rotation is free (one index formula, a bijection over the other seven
// sub-queues, run by the CPU model in tests/test_queue_model.py).  A drained-
// state mask read before stealing (one load per fetch instead of an atomic on
// each drained sub-queue) measured -0.1% / -0.5% and is gone.
// One lane: the next global chunk id for this workgroup, or kNoChunk.
__device__ uint64_t wg_fetch(WgQueue *L, unsigned long long *q, uint64_t nch) {
    const uint32_t home = blockIdx.x % kQSub;
    uint32_t d = lds_ld(&L->drained);
    while (d < kQSub) {
        // thieves of one home start at different victims (a rotation of the
        // other seven by workgroup), so a drained XCD's 32 workgroups do not
        // all queue on the next sub-queue's counter at the end of the batch
        const uint32_t k = d == 0 ? home : (home + 1 + (d - 1 + (blockIdx.x / kQSub) % (kQSub - 1)) % (kQSub - 1)) % kQSub;
        // sub-queue k owns chunks k, k + 8, k + 16, ...: every XCD streams
        // from the same moving window of the batch (contiguous per-XCD ranges
        // -- 8 windows far apart -- measured 8% slower on the headline batch)
        const uint64_t t = atomicAdd(q + k * kQStride, 1ull);
        if (k + t * kQSub < nch) return k + t * kQSub;
        atomicMax(&L->drained, d + 1);
        const uint32_t seen = lds_ld(&L->drained);
        d = seen > d + 1 ? seen : d + 1;
    }
    return kNoChunk;
}

// One lane: make chunk `seq` of this workgroup known in the ring.  Returns
// false when the wait for the ring entry's readers gave up (fault counted,
// the launch's abort flag raised).
__device__ bool wg_publish(WgQueue *L, unsigned long long *q, uint32_t seq, uint64_t id, uint32_t cl) {
    const uint32_t r = seq % kWgRing;
    bool ok = true;
    Deadline dl(abort_word(q));
    if (seq >= kWgRing)
        while (lds_ld(&L->reads[r]) != (1u << cl)) {
            __builtin_amdgcn_s_sleep(1);
            if (dl.passed()) {
                queue_fault(1, seq, lds_ld(&L->reads[r]));
                raise_abort(q);
                ok = false;
                break;
            }
        }
    lds_st(&L->reads[r], 0u);
    lds_st(&L->entry[r], (unsigned long long)seq << 32 | id);
    return ok;
}

// Thread 0, before the kernel's first barrier: reset the LDS state and
// publish the first chunk (its fetch overlaps the LDS table fill); workgroup
// 0 first zeroes the other bank's protocol lines for the slot's next launch
// (the fetch's returning atomic waits for those adds to be performed: vmcnt
// also counts non-returning atomics on gfx9-family parts).  Without a slot
// (see "Exclusivity") the workgroup takes the static split (busy = 1).
//
// Split in two for kernels whose waves start on a static first unit
// (for_each_unit<DYN, true>): wg_queue_reset (LDS only) before the barrier,
// wg_queue_start after it -- the fetch's round trip then no longer sits in
// front of thread 0's wave's table fill (waves look for a chunk only after
// their first unit; until the publish they wait on the ring entry).
__device__ __attribute__((unused)) void wg_queue_reset(WgQueue *L, unsigned long long *q) {
    L->slot = 0;
    L->drained = 0;
    L->busy = q == nullptr;
    for (uint32_t r = 0; r < kWgRing; r++) {
        L->reads[r] = 0;
        L->entry[r] = ~0ull;
    }
}
template <class Plan>
__device__ __attribute__((unused)) void wg_queue_start_plan(WgQueue *L, unsigned long long *q, const Plan &plan) {
    if (!q) return;
    if (blockIdx.x == 0) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(reinterpret_cast<uintptr_t>(q) ^ kQBankBytes);
#pragma unroll
        for (uint32_t j = 0; j < kQBankLines; j++) atomicExch(o + j * kQStride, 0ull);
    }
    (void)wg_publish(L, q, 0, wg_fetch(L, q, plan.nch), plan.cl);
}
__device__ __attribute__((unused)) void wg_queue_start(WgQueue *L, unsigned long long *q, uint64_t n) {
    if (!q) return;
    wg_queue_start_plan(L, q, ChunkPlan(n, gridDim.x));
}
__device__ __attribute__((unused)) void wg_queue_init(WgQueue *L, unsigned long long *q, uint64_t n) {
    wg_queue_reset(L, q);
    wg_queue_start(L, q, n);
}
template <class Plan>
__device__ __attribute__((unused)) void wg_queue_init_plan(WgQueue *L, unsigned long long *q, const Plan &plan) {
    wg_queue_reset(L, q);
    wg_queue_start_plan(L, q, plan);
}


template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const T o = __shfl_xor(v, k, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Calls body(u) for this wave's units: through the work queue (DYN: the
// throughput kernels, wg_queue_init has run) or u = wave, wave + nw, ... (the
// light layout's small batches, and DYN launches without a slot).
//
// Fail closed.  Every wait of the queue protocol is bounded; a wave whose wait
// gives up leaves the loop, and the units it would still have taken may then
// never be hashed.  for_each_unit returns true in the FIRST such wave of the
// launch (one fault flag per slot), which must then run fail_closed(): it
// reports the launch as failed, so unhashed bytes never read as verified.
// -DMCK_QFAULT_TEST=1 (test builds only) forces one give-up per launch.
#ifndef MCK_QFAULT_TEST
#define MCK_QFAULT_TEST 0
#endif
//
// FIRST: the caller has already run each wave's first unit, `wave` itself
// (known at kernel entry, so its loads can go out before the LDS fill); the
// static cursor starts at wave + nw and the queue deals units [q0, n),
// q0 = min(n, nw) -- wg_queue_init gets n - q0 (first_static_units).
__device__ __forceinline__ uint64_t first_static_units(uint64_t n, uint32_t nw) { return n < nw ? n : nw; }

// One wave's side of the queue protocol: take() takes the wave's next slot
// (LDS counter), waits for its chunk in the ring, does the slot's fetch duty
// and names the unit.  Without a slot (busy) it walks the static split.
template <class Plan>
struct UnitTaker {
    WgQueue *L;
    unsigned long long *queue;
    uint64_t n, q0, su, nch, max_iters, iters = 0;
    uint32_t nw, cl, cu, lead, flt = 0;  // flt (lane 0): a wait of this wave gave up
    uint32_t seq = 0;                     // the workgroup's chunk sequence number of the last slot taken
    bool l0;
    Plan plan;
#if MCK_TRACE
    unsigned long long qs_n = 0, qs_sum = 0, qs_max = 0, qs_wait = 0, qs_busy = 0, qs_units = 0;
#endif
    __device__ __forceinline__ UnitTaker(WgQueue *L_, unsigned long long *q, uint64_t n_, uint32_t wave, uint32_t nw_,
                                         bool first, const Plan &p)
        : L(L_), queue(q), n(n_), q0(first ? first_static_units(n_, nw_) : 0),
          su(first ? (uint64_t)wave + nw_ : wave), nch(p.nch), nw(nw_), cl(p.cl), cu(1u << p.cl),
          lead(cu > 4 ? cu / 4 : 1), l0((threadIdx.x & 63u) == 0), plan(p) {
        max_iters = (uint64_t)cu * nch + 4ull * cu + 64;
    }
    // The wave's next slot: false when the wave is done (the queue ran dry,
    // or a wait gave up); else *u = its unit, or n for a tail chunk's slot
    // past the chunk's size.  (busy is re-read from LDS every call -- an
    // atomic load the compiler cannot hoist: one call site of the payload loop
    // for both splits; a second inlined copy made the offsets kernels spill.)
    __device__ __forceinline__ bool take(uint64_t *u) {
        if (__builtin_amdgcn_readfirstlane(lds_ld(&L->busy))) {
            if (su >= n) return false;
            *u = su;
            su += nw;
            return true;
        }
        uint64_t e = 0;
        uint32_t t = 0;
        if (++iters > max_iters) {  // more slots than the launch has: protocol fault
            if (l0) {
                queue_fault(3, iters, 0);
                flt = 1;
            }
            return false;
        }
        if (l0) {
            t = atomicAdd(&L->slot, 1u);
            const uint32_t seq = t >> cl, r = seq % kWgRing;
            Deadline dl(abort_word(queue));
#if MCK_TRACE
            const unsigned long long w0 = wall_clock64();
            unsigned long long f0 = 0;
#endif
            while (((e = lds_ld(&L->entry[r])) >> 32) != seq) {
                __builtin_amdgcn_s_sleep(1);
                MCK_WAIT_GUARD(dl, 2, seq, e)
            }
#if MCK_TRACE
            qs_wait += wall_clock64() - w0;
#endif
            if ((e >> 32) != seq) {  // gave up (fault counted)
                raise_abort(queue);
                e = kNoChunk;
                flt = 1;
            }
            atomicAdd(&L->reads[r], 1u);
            // One taker per chunk (slot cu - lead) fetches the next chunk --
            // after its own chunk is known, so fetches run in chunk order and
            // the first kNoChunk is final.
            if ((t & (cu - 1)) == cu - lead) {
#if MCK_TRACE
                f0 = wall_clock64();
#endif
#if MCK_QFAULT_TEST
                // injected stall: workgroup 3 neither fetches nor publishes
                // its third chunk (no chunk is lost: the other workgroups take
                // every unit), so each of its waves waits out the deadline on
                // that ring entry
                const bool stall = (g_mck_qfault_mode & 1u) && blockIdx.x == 3 && seq == 1;
#else
                constexpr bool stall = false;
#endif
                const uint64_t nid = (e & 0xFFFFFFFFull) == kNoChunk || stall ? kNoChunk : wg_fetch(L, queue, nch);
#if MCK_TRACE
                const unsigned long long df = wall_clock64() - f0;
                qs_n++;
                qs_sum += df;
                qs_max = df > qs_max ? df : qs_max;
#endif
                if (!stall && !wg_publish(L, queue, seq + 1, nid, cl)) flt = 1;
            }
#if MCK_QFAULT_TEST
            // injected give-up: workgroup 3 drops the first unit of its second
            // chunk (after its reads/publish duties, so the rest of the launch
            // runs on)
            if (g_mck_qfault_mode == 0u && blockIdx.x == 3 && seq == 1 && (t & (cu - 1)) == 0 && !flt) {
                queue_fault(9, seq, t);
                e = kNoChunk;
                flt = 1;
            }
#endif
        }
        t = __builtin_amdgcn_readfirstlane(t);
        seq = t >> cl;
        const uint64_t id = uniform64(e) & 0xFFFFFFFFull;
        if (id == kNoChunk) return false;
        // every chunk spans cu slots; a tail chunk's slots past its size are skipped
        const uint32_t k = t & (cu - 1);
        *u = k < plan.size(id) ? q0 + plan.start(id) + k : n;
        return true;
    }
    // The wave's next unit, past any empty slots: false when it is done.
    __device__ __forceinline__ bool take_unit(uint64_t *u) {
        while (take(u))
            if (*u < n) return true;
        return false;
    }
    // After the wave's last take: true in the FIRST wave of the launch whose
    // wait gave up (it claims the bank's fault flag and must run fail_closed).
    __device__ __forceinline__ bool finish(uint32_t wave) {
#if MCK_TRACE
        if (l0 && wave < 16384u) {
            g_mck_qwave[4 * wave] = qs_n;
            g_mck_qwave[4 * wave + 1] = qs_sum;
            g_mck_qwave[4 * wave + 2] = qs_max;
            g_mck_qwave[4 * wave + 3] = qs_wait;
            g_mck_qwave[4 * 16384 + 2 * wave] = qs_units;
            g_mck_qwave[4 * 16384 + 2 * wave + 1] = qs_busy;
        }
#else
        (void)wave;
#endif
        if (__builtin_amdgcn_readfirstlane(lds_ld(&L->busy))) return false;  // no slot
        uint32_t first = 0;
        if (l0 && flt) first = atomicCAS(queue + kQFault * kQStride, 0ull, 1ull) == 0ull;
        return __builtin_amdgcn_readfirstlane(first) != 0;
    }
};

template <bool DYN, bool FIRST = false, class Plan = ChunkPlan, class F>
__device__ __forceinline__ bool for_each_unit(WgQueue *L, unsigned long long *queue, uint64_t n, uint32_t wave,
                                              uint32_t nw, F &&body, const Plan *given = nullptr) {
    if constexpr (DYN) {
        const Plan plan = [&] {
            if constexpr (std::is_same_v<Plan, ChunkPlan>) return given ? *given : ChunkPlan(n - (FIRST ? first_static_units(n, nw) : 0), gridDim.x);
            else return *given;
        }();
        UnitTaker<Plan> tk(L, queue, n, wave, nw, FIRST, plan);
        uint64_t u;
        while (tk.take(&u)) {
#if MCK_TRACE
            const unsigned long long b0 = wall_clock64();
#endif
            if (u < n) body(u);
#if MCK_TRACE
            tk.qs_busy += wall_clock64() - b0;
            tk.qs_units += u < n;
            if (tk.l0 && u < n && u < (1ull << 17)) g_mck_unit_end[u] = wall_clock64() | (unsigned long long)(blockIdx.x % kQSub) << 60;
#endif
        }
        return tk.finish(wave);
    } else {
        for (uint64_t u = FIRST ? (uint64_t)wave + nw : wave; u < n; u += nw) body(u);
        return false;
    }
}

// Run by the wave for_each_unit picked after a give-up (wave-uniform): the
// launch did not hash every payload, so it must not read as clean.  The
// caller's error word (if set) gets +1; a verify launch adds `count` to the
// mismatch counter and marks every payload's status 1 -- payloads that are
// hashed after this sweep overwrite theirs with the true result, so each
// status ends as the correct value or 1 ("flagged"), never a stale 0.
template <bool VERIFY>
__device__ __forceinline__ void fail_closed(const BatchArgs &a) {
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0) {
        if (a.err_word) atomicAdd(a.err_word, 1u);
        if (VERIFY && a.mismatches) atomicAdd(a.mismatches, (uint32_t)a.count);
    }
    if (VERIFY && a.status)
        for (uint64_t p = lane; p < a.count; p += 64) a.status[p] = 1;
}

// Diagnostic build (-DMCK_TRACE=1, tools/tail_trace.py): per-wave clock
// stamps (kernel entry, after the LDS fill, exit) of the last launch.
#if MCK_TRACE
constexpr int kTraceWaves = 16384;
__device__ unsigned long long g_mck_trace[3 * kTraceWaves];
// the XCD each wave ran on (hardware register XCC_ID), stamped at entry
__device__ unsigned int g_mck_trace_xcc[kTraceWaves];
// the shader-clock counter (clock64) at entry and exit: with the wall stamps
// the clock each XCD ran at over the wave's life (tools/xcd_clock.py)
__device__ unsigned long long g_mck_trace_clk[2 * kTraceWaves];
__device__ __forceinline__ unsigned int xcc_id() {
    unsigned int r;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(r));
    return r & 15u;
}
#define MCK_STAMP(w, k)                                                                   \
    do {                                                                                  \
        if ((threadIdx.x & 63u) == 0 && (w) < kTraceWaves) {                              \
            g_mck_trace[3 * (w) + (k)] = wall_clock64();                                  \
            if ((k) == 0) g_mck_trace_xcc[(w)] = xcc_id();                                \
            if ((k) != 1) g_mck_trace_clk[2 * (w) + ((k) >> 1)] = clock64();              \
        }                                                                                 \
    } while (0)
#else
#define MCK_STAMP(w, k) do { } while (0)
#endif

}  // namespace

#endif  // CRC_GPU_QUEUE_H
