// crc_gpu_copy.h -- the copy kernels: mchecksum_gpu_copy_offsets and
// mchecksum_gpu_update_copy_offsets.  Chunk p = base[offsets[p], offsets[p+1])
// is stored at dst[dst_starts[p], ...) by the payload loop that hashes it, so
// the chunk is read once for the copy and the CRC.  A third kernel family
// beside the batch kernels (crc_gpu_crc32.h, crc_gpu_crc64.h), as the segment
// and XDR kernels are: offsets mode only, one chunk per wave (G = 64), keyed by
// copy_plan.h's CopyKey.  Everything but the kernels' own few lines is the
// batch kernels': the LDS fill, the work queue and its fail-closed report
// (for_each_unit, fail_closed), the light layout's static ranges (wave_range),
// the copying payload loops (payload32_g64 / payload32_generic and payload64_g64
// / payload64_generic with COPY) and the owning lane's epilogues (emit,
// mck_seed32, mck_seed64).
//
// Unlike pack and unpack the destinations are independent: dst_starts holds
// one start per chunk, in any order, and the length comes from the source
// table, so there is no fit rule and no status.
#ifndef CRC_GPU_COPY_H
#define CRC_GPU_COPY_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "copy_plan.h"
#include "crc_gpu_common.h"
#include "crc_gpu_crc32.h"
#include "crc_gpu_crc64.h"

namespace {

// A batch call's arguments (base, offsets, count, out = the CRCs or the
// running registers, pack, queue, err_word, shift) and where the chunks go.
struct CopyArgs {
    BatchArgs b;
    uint8_t *dst;
    const uint64_t *dst_starts;  // count byte offsets into dst
};
MCK_AT(CopyArgs, b, 0);
MCK_AT(CopyArgs, dst, 136);
MCK_AT(CopyArgs, dst_starts, 144);
static_assert(sizeof(CopyArgs) == 152, "CopyArgs changed size");

// OP (copy_plan.h, CopyOp): what the owning lane does with a chunk's CRC.
template <int OP, bool NT, bool LIGHT>
__global__ __launch_bounds__(kBlk32<LIGHT>, 1) void crc32c_copy_kernel(CopyArgs c) {
    static_assert(mck::copy_key_valid(mck::CopyKey{32, OP, NT, LIGHT}), "no such copy kernel");
    enum : bool { SEED = OP == mck::kCopyUpdate };
    const BatchArgs &a = c.b;
    constexpr int kWavesPerBlock = kBlk32<LIGHT> / 64;
    __shared__ __attribute__((aligned(16))) uint8_t lds_raw[LIGHT ? kL32LightBytes : kL32Bytes];
    const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
    const uint64_t units = a.count;
    __shared__ WgQueue wgq;
    const uint32_t gl = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    // (model words read once, ahead of any store: see crc32c_batch_kernel)
    const uint32_t init = pk->init, xorout = pk->xorout;
    if (!LIGHT && threadIdx.x == 0) wg_queue_init(&wgq, a.queue, units);
    fill_lds32<LIGHT, kBlk32<LIGHT>>(lds_raw, pk);
    __syncthreads();
    const Tab32<LIGHT> lds{lds_raw};
    const uint32_t lc0 = (gl & 31u) << 2, lc1 = lc0 | 0x10000u;

    auto one = [&](uint64_t p) {
        const uint64_t o = a.offsets[p], n = a.offsets[p + 1] - o;
        uint8_t *dst = c.dst + c.dst_starts[p];
        const uint32_t x =
            n < (1ull << 31) ? payload32_g64<NT, Tab32<LIGHT>, false, true>(lds, pk, a.base + o, n, gl, lc0, lc1, 0u, dst)
                             : payload32_generic<6, NT, Tab32<LIGHT>, true>(lds, pk, a.base + o, n, gl, lc0, lc1, dst);
        if (gl == 0) {
            if constexpr (SEED) {
                uint32_t *st = reinterpret_cast<uint32_t *>(a.out) + p;
                *st = mck_seed32(reinterpret_cast<const crc32_shift_pack_t *>(a.shift), x, *st, init, n);
            } else {
                uint32_t nbad = 0;
                emit<uint32_t, false>(a, p, x ^ xorout, nbad);
            }
        }
    };
    if constexpr (!LIGHT) {
        if (for_each_unit<true>(&wgq, a.queue, units, wave, nw, one)) fail_closed<false>(a);
    } else {  // static: a byte-balanced contiguous range per wave
        uint64_t first, last;
        wave_range(a.offsets, a.count, wave, nw, &first, &last);
        for (uint64_t p = first; p < last; p++) one(p);
    }
}

// The CRC-64 offsets kernels' shape: two workgroups per CU, the mixed operator
// placement, a 4-deep ring (crc_gpu_shape.h, Shape<64, kOffsets>).
template <int OP, bool NT>
__global__ __launch_bounds__(kBlk64<kOffsets * 16 + 6>, kWpe64<kOffsets * 16 + 6>) void crc64_copy_kernel(CopyArgs c) {
    static_assert(mck::copy_key_valid(mck::CopyKey{64, OP, NT, false}), "no such copy kernel");
    enum : bool { SEED = OP == mck::kCopyUpdate };
    using S = Shape<64, kOffsets, false, 6>;
    constexpr int kWPB = S::block / 64;
    const BatchArgs &a = c.b;
    __shared__ __attribute__((aligned(16))) uint8_t lds[S::lds64_bytes];
    const crc64_gpu_pack_t *pk = reinterpret_cast<const crc64_gpu_pack_t *>(a.pack);
    const uint64_t units = a.count;
    __shared__ WgQueue wgq;
    if (threadIdx.x == 0) wg_queue_init(&wgq, a.queue, units);
    fill_lds64<S::block, S::ops_mode>(lds, pk);
    __syncthreads();

    const uint32_t gl = threadIdx.x & 63u;
    const uint32_t lc = (gl & 31u) << 3;
    const uint64_t xorout = pk->xorout;
    const uint32_t nw = gridDim.x * kWPB;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWPB + (threadIdx.x >> 6));

    auto one = [&](uint64_t p) {
        const uint64_t o = a.offsets[p], n = a.offsets[p + 1] - o;
        uint8_t *dst = c.dst + c.dst_starts[p];
        const uint64_t x =
            n < (1ull << 31) ? payload64_g64<NT, false, S::ops_mode, true>(lds, pk, a.base + o, n, gl, lc, 0ull, dst)
                             : payload64_generic<6, NT, S::ops_mode, true>(lds, pk, a.base + o, n, gl, lc, dst);
        if (gl == 0) {
            if constexpr (SEED) {
                uint64_t *st = reinterpret_cast<uint64_t *>(a.out) + p;
                *st = mck_seed64(reinterpret_cast<const crc64_shift_pack_t *>(a.shift), x, *st, pk->init, n);
            } else {
                uint32_t nbad = 0;
                emit<uint64_t, false>(a, p, x ^ xorout, nbad);
            }
        }
    };
    if (for_each_unit<true>(&wgq, a.queue, units, wave, nw, one)) fail_closed<false>(a);
}

}  // namespace

#endif  // CRC_GPU_COPY_H
