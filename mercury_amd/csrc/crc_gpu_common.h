// crc_gpu_common.h -- what the CRC-32C and CRC-64 batch kernels share: payload
// and LDS loads, the three-input XOR, the copying loops' store of a piece,
// result emission and mismatch counting, and the byte-balanced static
// partition of an offsets batch.
#ifndef CRC_GPU_COMMON_H
#define CRC_GPU_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc_gpu_pack_store.h"
#include "crc_gpu_queue.h"
#include "crc_gpu_shape.h"

namespace {

// Network-order u32 at an arbitrary byte address (the HG header's payload
// hash, src/mercury_header.c:111-112 writes it with htonl).
__device__ __forceinline__ uint32_t load_be32(const uint8_t *q) {
    return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3];
}

// ... and its store (hg_set_struct's, src/mercury.c:699-707): four byte
// stores, since the slot sits at any byte address.
__device__ __forceinline__ void store_be32(uint8_t *q, uint32_t v) {
    q[0] = (uint8_t)(v >> 24);
    q[1] = (uint8_t)(v >> 16);
    q[2] = (uint8_t)(v >> 8);
    q[3] = (uint8_t)v;
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// Payload bytes are read exactly once.  Non-temporal loads keep a batch far
// larger than the 256 MiB Infinity Cache from churning the caches: +13% on the
// 4 GiB headline batch (profiles/r01/ab1.log); a small batch replayed
// back to back is faster with the default policy (it partly hits the cache).
template <bool NT>
__device__ __forceinline__ uint4 ld16(const uint4 *p) {
    if constexpr (NT) {
        const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}

__device__ __forceinline__ uint32_t lds32(const uint8_t *lds, uint32_t a) {
    return *reinterpret_cast<const uint32_t *>(lds + a);
}
__device__ __forceinline__ uint64_t lds64(const uint8_t *lds, uint32_t a) {
    return *reinterpret_cast<const uint64_t *>(lds + a);
}

// a ^ b ^ c in one VALU op: gfx950's v_bitop3_b32 with truth table 0x96
// (there is no v_xor3_b32 on CDNA; hipcc does not form bitop3 from ^ chains).
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// Global-address-space views: loads through them are global_load (never
// flat_load, which would also count against lgkmcnt and make every LDS wait
// wait for HBM), and a wave-uniform base in SGPRs gives the saddr form.
typedef const __attribute__((address_space(1))) uint8_t *gbyte_t;
typedef const __attribute__((address_space(1))) u32x4_t *gvec_t;
__device__ __forceinline__ gbyte_t global_ptr(const uint8_t *p, bool uniform) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    return (gbyte_t)(uniform ? uniform64(v) : v);
}
template <bool NT>
__device__ __forceinline__ uint4 ldg16(gbyte_t p) {
    const gvec_t q = (gvec_t)p;
    u32x4_t v;
    if constexpr (NT) v = __builtin_nontemporal_load(q);
    else v = *q;
    return make_uint4(v.x, v.y, v.z, v.w);
}

// The copying payload loops (COPY: mchecksum_gpu_pack_messages,
// mchecksum_gpu_unpack_messages, and the copy kernels of crc_gpu_copy.h, both
// widths): the lane that
// folds a piece stores the bytes crc_gpu_pack_store.h names at dst + their
// payload position.  A whole piece is one 16-byte store through an align-1
// type (source and destination residues differ in general; one
// global_store_dwordx4), an edge piece goes byte by byte.
typedef u32x4_t piece16_t __attribute__((aligned(1)));
typedef __attribute__((address_space(1))) uint8_t *gwbyte_t;
__device__ __forceinline__ void store_piece(gwbyte_t dst, const PieceStore &s, const uint4 &v) {
    if (s.whole()) {
        *(__attribute__((address_space(1))) piece16_t *)(dst + s.lo) = u32x4_t{v.x, v.y, v.z, v.w};
    } else {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t b = 0; b < 16; b++)
            if (b >= s.b0 && b < s.b1) dst[s.lo + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3u)));
    }
}

// Byte-balanced static partition of an offsets batch: wave w owns payloads
// whose start offset lies in [off0 + total*w/nw, off0 + total*(w+1)/nw).
__device__ __forceinline__ uint64_t lower_bound_u64(const uint64_t *a, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void wave_range(const uint64_t *off, uint64_t count, uint32_t wave, uint32_t nw,
                                           uint64_t *first, uint64_t *last) {
    const uint64_t o0 = off[0], total = off[count] - o0;
    const uint64_t q = total / nw, r = total % nw;
    const uint64_t lo = o0 + q * wave + (r * wave) / nw;
    const uint64_t hi = o0 + q * (wave + 1) + (r * (wave + 1)) / nw;
    *first = wave == 0 ? 0 : lower_bound_u64(off, count, lo);
    *last = wave + 1 == nw ? count : lower_bound_u64(off, count, hi);
}

// A verify launch counts its mismatches per lane (nbad) and adds them to the
// caller's counter once per WORKGROUP at its end.  Device-scope atomics on one
// word serialize: one per bad payload (or per wave) made 4096 bad 4 KiB
// messages a 58 us kernel against 19 us when they all matched
// (tools/lat_offsets.py), so a corrupted buffer cost three times a good one.
// Every thread of the workgroup calls this, once.
__device__ __forceinline__ void add_mismatches(uint32_t *ctr, uint32_t nbad) {
    __shared__ uint32_t wg_bad;
    if (threadIdx.x == 0) wg_bad = 0;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) nbad += __shfl_xor(nbad, d, 64);
    if ((threadIdx.x & 63u) == 0 && nbad) atomicAdd(&wg_bad, nbad);
    __syncthreads();
    if (threadIdx.x == 0 && wg_bad && ctr) atomicAdd(ctr, wg_bad);
}

template <typename T, bool VERIFY>
__device__ __forceinline__ void emit(const BatchArgs &a, uint64_t p, T v, uint32_t &nbad) {
    if (VERIFY) {
        if (a.bswap) {
            if constexpr (sizeof(T) == 8) v = (T)__builtin_bswap64((uint64_t)v);
            else v = (T)__builtin_bswap32((uint32_t)v);
        }
        const bool bad = reinterpret_cast<const T *>(a.expected)[p] != v;
        if (a.status) a.status[p] = bad ? 1 : 0;
        nbad += bad;
    } else {
        reinterpret_cast<T *>(a.out)[p] = v;
    }
}

}  // namespace

#endif  // CRC_GPU_COMMON_H
