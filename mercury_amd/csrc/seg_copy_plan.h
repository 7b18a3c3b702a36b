// seg_copy_plan.h -- where a chunk of a scatter-gather object lies on both
// sides of mchecksum_gpu_gather_segments / mchecksum_gpu_scatter_segments
// (seg_copy_kernel, mchecksum_gpu_ext.hip): how a segment is cut into chunks
// and the two addresses of each chunk.  Pure arithmetic, like launch_plan.h and
// copy_plan.h: the kernels include it, and the host compiler walks it on the
// CPU (tests/native/seg_copy_plan.cpp) together with the store rule
// (crc_gpu_pack_store.h).  Plain C++ compiles it.
//
// Object j = segments [first[j], first[j + 1]) in order; P is the exclusive
// prefix sum of the segment lengths (the scan's).  A chunk is bytes [off, off +
// n) of segment s, off a multiple of the chunk size.  It starts at
//   segment side:    addr[s] + off
//   contiguous side: base + starts[j] + (P[s] + off - P[first[j]])
// and the direction says which of the two is loaded and which is stored.
#ifndef MCK_SEG_COPY_PLAN_H
#define MCK_SEG_COPY_PLAN_H

#include <cstdint>

#include "crc_gpu_shape.h"

namespace mck {

// gather: segments -> contiguous; scatter: contiguous -> segments
enum SegCopyDir : int { kSegGather, kSegScatter };

// The segment passes' chunk size (mchecksum_gpu_ext.hip, kChunk).  CH is a
// parameter so that a test can make chunk edges dense.
constexpr uint64_t kSegChunk = 256u << 10;

template <uint64_t CH = kSegChunk>
MCK_HOST_DEVICE_INLINE uint64_t seg_chunk_count(uint64_t len) {
    return (len + CH - 1) / CH;
}
// bytes of the chunk at offset off (< len) of a segment of len bytes
template <uint64_t CH = kSegChunk>
MCK_HOST_DEVICE_INLINE uint64_t seg_chunk_len(uint64_t len, uint64_t off) {
    return len - off < CH ? len - off : CH;
}

struct SegCopyAddr {
    uint64_t load, store;
};

// seg_at = addr[s] + off; at = P[s] + off (the chunk's first byte in the
// list's byte order); obj_at = P[first[j]]; start = starts[j].
MCK_HOST_DEVICE_INLINE SegCopyAddr seg_copy_addr(int dir, uint64_t seg_at, uint64_t base, uint64_t start, uint64_t at,
                                                 uint64_t obj_at) {
    const uint64_t flat = base + start + (at - obj_at);
    return dir == kSegGather ? SegCopyAddr{seg_at, flat} : SegCopyAddr{flat, seg_at};
}

}  // namespace mck

#endif  // MCK_SEG_COPY_PLAN_H
