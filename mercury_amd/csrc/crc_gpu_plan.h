// crc_gpu_plan.h -- the work queue's chunk plan: how the units [0, n) of a
// launch are cut into chunks for a grid of workgroups.  One piece of
// arithmetic for the kernels (which pass gridDim.x), the host's launch plan
// and the CPU tests (tests/native/split_plan.cpp; tests/test_queue_model.py
// checks its Python model against it).  Plain C++ compiles it.
#ifndef CRC_GPU_PLAN_H
#define CRC_GPU_PLAN_H

#include <cstdint>

#include "crc_gpu_shape.h"

namespace {

// Chunk plan: ids [0, nbig) are full chunks of 2^cl units; the last
// (about one full chunk per workgroup of) units go out as eighth chunks, ids
// [nbig, nch), so a workgroup that fetches late holds little unstarted work
// when the queue runs dry.  The highest ids are handed out last (every
// sub-queue counts up), so the small chunks form the tail.
// (kWgChunkMaxLog2, kQTailShift: crc_gpu_shape.h.)
struct ChunkPlan {
    uint32_t cl, sl;    // log2 of the full / tail chunk size
    uint64_t nbig, nch, big_end;
    // log2 of the full chunk size: about a quarter of a workgroup's fair share
    MCK_HOST_DEVICE_INLINE static uint32_t full_log2(uint64_t n, uint32_t grid) {
        const uint64_t share = n / (4ull * grid);
        uint32_t l = 0;
        while (l < kWgChunkMaxLog2 && (2ull << l) <= share) l++;
        return l;
    }
    MCK_HOST_DEVICE_INLINE ChunkPlan(uint64_t n, uint32_t grid) {
        cl = full_log2(n, grid);
        sl = cl >= kQTailShift ? cl - kQTailShift : cl;
        const uint64_t tail = (uint64_t)grid << cl;
        nbig = n > tail ? (n - tail) >> cl : 0;
        big_end = nbig << cl;
        nch = nbig + ((n - big_end + (1ull << sl) - 1) >> sl);
    }
    // first unit and size of chunk id
    MCK_HOST_DEVICE_INLINE uint64_t start(uint64_t id) const { return id < nbig ? id << cl : big_end + ((id - nbig) << sl); }
    MCK_HOST_DEVICE_INLINE uint32_t size(uint64_t id) const { return id < nbig ? 1u << cl : 1u << sl; }
};
// Split CRC-64: the queue plan of a split launch -- ChunkPlan's layout over
// count << psl units, unit u = piece (u & (2^psl - 1)) of payload u >> psl.
// (Late round 5 also tried the tail's payloads in 2-4x finer pieces: the
// per-wave end spread fell from 111 to 42 us, but every piece pays its own
// combine and Z^n shift, and C3 lost 0.5%: HISTORY.md.)
struct SplitPlan : ChunkPlan {
    uint32_t psl;  // log2 pieces per payload
    uint64_t n;    // units
    MCK_HOST_DEVICE SplitPlan(uint64_t count, uint32_t psl_, uint32_t grid)
        : ChunkPlan(count << psl_, grid), psl(psl_), n(count << psl_) {}
    // unit u: piece *q of payload *p
    MCK_HOST_DEVICE void unit(uint64_t u, uint64_t *p, uint32_t *q) const {
        *p = u >> psl;
        *q = (uint32_t)u & ((1u << psl) - 1u);
    }
    // every chunk holds whole payloads, at most kSplitAcc of them (the
    // in-workgroup combine, split_lds)
    MCK_HOST_DEVICE bool whole() const {
        return psl >= 1 && (1u << psl) <= (1u << sl) && (1u << cl) / (1u << psl) <= kSplitAcc;
    }
};

}  // namespace

#endif  // CRC_GPU_PLAN_H
