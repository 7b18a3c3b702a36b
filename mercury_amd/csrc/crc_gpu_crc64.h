// crc_gpu_crc64.h -- CRC-64 on the device: the 12-lookup step fold, the
// operator placements and combines, the LDS fill, the payload loops, the Z^n
// register shift and the persistent batch kernel (with its split pieces).
// Algebra: crc_gpu_layout.h.
#ifndef CRC_GPU_CRC64_H
#define CRC_GPU_CRC64_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "crc_gpu_common.h"
#include "crc_gpu_layout.h"
#include "crc_gpu_mask.h"
#include "crc_gpu_plan.h"
#include "crc_gpu_queue.h"
#include "crc_gpu_seed.h"
#include "crc_gpu_shape.h"
#include "crc_gpu_window.h"
#include "launch_plan.h"

namespace {

__device__ __forceinline__ uint64_t xor3_64(uint64_t a, uint64_t b, uint64_t c) {
    return (uint64_t)xor3((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32)) << 32 |
           xor3((uint32_t)a, (uint32_t)b, (uint32_t)c);
}

// XOR of 16 table words and one more value: 8 bitop3 per 32-bit half.
__device__ __forceinline__ uint64_t xor17(const uint64_t *r, uint64_t extra) {
    const uint64_t a = xor3_64(r[0], r[1], r[2]), b = xor3_64(r[3], r[4], r[5]), c = xor3_64(r[6], r[7], r[8]);
    const uint64_t d = xor3_64(r[9], r[10], r[11]), e = xor3_64(r[12], r[13], r[14]);
    return xor3_64(xor3_64(r[15], extra, a), xor3_64(b, c, d), e);
}

// Per-lane lookup address registers of f64x: the lane-copy offset in byte 0
// of four persistent registers, whose byte 1 the pair index is written into
// by one v_and_b32_sdwa each (dst_unused:UNUSED_PRESERVE keeps byte 0), so a
// replicated lookup costs one VALU op and no separate masking.
struct Lane64 {
    uint32_t lc;
    uint32_t al[4];
};
__device__ __forceinline__ Lane64 lane64(uint32_t lc) { return Lane64{lc, {lc, lc, lc, lc}}; }

// (byte B of x) & 0xF8: a 5-bit field scaled by 8, its own f5 address;
// (byte B of t) & 0x3F into byte 1 of the lane-copy register a.
#define MCK_SDWA_P6(B)                                                                              \
    __device__ __forceinline__ uint32_t sdwa_f8_##B(uint32_t x) {                                   \
        uint32_t r;                                                                                 \
        asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD "         \
            "src1_sel:BYTE_" #B : "=v"(r) : "s"(0xF8u), "v"(x));                                    \
        return r;                                                                                   \
    }                                                                                               \
    __device__ __forceinline__ void sdwa_p6_##B(uint32_t &a, uint32_t t) {                          \
        asm("v_and_b32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD "   \
            "src1_sel:BYTE_" #B : "+v"(a) : "s"(0x3Fu), "v"(t));                                    \
    }
MCK_SDWA_P6(0)
MCK_SDWA_P6(1)
MCK_SDWA_P6(2)
MCK_SDWA_P6(3)
#undef MCK_SDWA_P6
// Byte i of the result: bits 0..2 of byte i of the low half xl and, above
// them, bits 0..4 of byte i of the high half xh -- the 6-bit index of pair
// table i (bytes i and i + 4 of the word; sdwa_p6 keeps 6 bits).  One shift
// and one v_bfi_b32 (mask in an SGPR; VOP3 takes no literal on gfx9) for all
// four pair indexes: round 1 paired bytes (2i, 2i+1) within a half, which took
// a shift and a bit-select per half (28 -> 26 VALU ops per 8-byte word on a
// VALU-bound loop).  The C form (x & m) | (y & ~m) compiled to v_and +
// v_and_or: one op more.  (Round 5: the bit-select as a v_bitop3 with its mask
// in a VGPR, which the probe issues faster, measured +-0 in the loop.)
__device__ __forceinline__ uint32_t gather6(uint32_t xl, uint32_t xh) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "s"(0x07070707u), "v"(xl), "v"(xh << 3));
    return r;
}
__device__ __forceinline__ uint64_t xor13(const uint64_t *r, uint64_t extra) {
    const uint64_t a = xor3_64(r[0], r[1], r[2]), b = xor3_64(r[3], r[4], r[5]), c = xor3_64(r[6], r[7], r[8]);
    return xor3_64(a, b, xor3_64(c, xor3_64(r[9], r[10], r[11]), extra));
}
// Z^(16G)(x) ^ next from the 12 tables f5/f6 (LDS map: crc_gpu_shape.h): 12 address
// ops, 2 for the gather, 12 v_bitop3 for the XOR tree (the next data word
// rides in its 13th input).
__device__ __forceinline__ uint64_t f64x(const uint8_t *lds, uint64_t x, uint64_t next, Lane64 &ln) {
    const uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
    // byte i of t: bits 0..2 of bytes i and i + 4 of the word (bit-select)
    const uint32_t t = gather6(xl, xh);
    uint64_t r[12];
    r[0] = lds64(lds, sdwa_f8_0(xl) + kL64P5 + 0 * 256);
    r[1] = lds64(lds, sdwa_f8_1(xl) + kL64P5 + 1 * 256);
    r[2] = lds64(lds, sdwa_f8_2(xl) + kL64P5 + 2 * 256);
    r[3] = lds64(lds, sdwa_f8_3(xl) + kL64P5 + 3 * 256);
    r[4] = lds64(lds, sdwa_f8_0(xh) + kL64P5 + 4 * 256);
    r[5] = lds64(lds, sdwa_f8_1(xh) + kL64P5 + 5 * 256);
    r[6] = lds64(lds, sdwa_f8_2(xh) + kL64P5 + 6 * 256);
    r[7] = lds64(lds, sdwa_f8_3(xh) + kL64P5 + 7 * 256);
    sdwa_p6_0(ln.al[0], t);
    r[8] = lds64(lds, ln.al[0] + kL64P6 + 0 * 16384);
    sdwa_p6_1(ln.al[1], t);
    r[9] = lds64(lds, ln.al[1] + kL64P6 + 1 * 16384);
    sdwa_p6_2(ln.al[2], t);
    r[10] = lds64(lds, ln.al[2] + kL64P6 + 2 * 16384);
    sdwa_p6_3(ln.al[3], t);
    r[11] = lds64(lds, ln.al[3] + kL64P6 + 3 * 16384);
    return xor13(r, next);
}

template <bool OG>
__device__ __forceinline__ uint64_t op64(const uint8_t *lds, const crc64_gpu_pack_t *pk, uint32_t o, uint64_t x) {
    uint64_t r[16];
    if constexpr (OG) {
        const uint64_t *t = &pk->ops[o][0][0];
#pragma unroll
        for (int h = 0; h < 16; h++) r[h] = t[h * 16 + ((x >> (4 * h)) & 15u)];
    } else {
        const uint32_t base = kL64Main + o * 2048;
#pragma unroll
        for (int h = 0; h < 16; h++) r[h] = lds64(lds, base + h * 128 + (uint32_t)(((x >> (4 * h)) & 15u) << 3));
    }
    return xor17(r, 0);
}

template <int OM>
__device__ __forceinline__ uint64_t opm64(const uint8_t *lds, const crc64_gpu_pack_t *pk, uint32_t o, uint64_t x) {
    if constexpr (OM == kOpsMix) {
        if (o >= 1 && o <= 6) return op64<false>(lds, pk, o - 1, x);  // butterflies at kL64Main
        return op64<true>(lds, pk, o, x);
    } else {
        return op64<OM == kOpsGlobal>(lds, pk, o, x);
    }
}

template <int LOG2G, int OM>
__device__ __forceinline__ uint64_t combine64(const uint8_t *lds, const crc64_gpu_pack_t *pk, uint64_t s0, uint64_t s1,
                                              uint32_t gl) {
    uint64_t x = s0 ^ opm64<OM>(lds, pk, 0, s1);
#pragma unroll
    for (int k = 0; k < LOG2G; k++) {
        const uint64_t other = __shfl_xor(x, 1 << k, 64);
        const bool bit = (gl >> k) & 1u;
        const uint64_t lo = bit ? other : x, hi = bit ? x : other;
        x = lo ^ opm64<OM>(lds, pk, 1 + k, hi);
    }
    return x;
}

// The same sum as a halving reduction (lane 0 of each group of G lanes): at
// distance d = G/2, ..., 2, 1 the lanes below d add Z^-(16d) of the state d
// lanes up, so level d's lookups run on d lanes where the butterfly's ran on
// all G, and lane 0 ends with the sum (payload64_g64 then runs its tail
// operators on lane 0 alone).  C4-layout CRC-64 +3.1% / +2.4%
// (profiles/r06/ab_c4_64_combine.log, ab_lane0.log: the combine and tail were
// 14% of that kernel's time; running the tail on the wave-uniform value
// through the scalar cache instead cost 9%).  The C3 split pieces and the
// segment chunk pass measured +-0 / -0.9% with it and keep the butterfly;
// payload64_g64 uses it only in the offsets kernels (kOpsMix).
template <int LOG2G, int OM>
__device__ __forceinline__ uint64_t combine64_lane0(const uint8_t *lds, const crc64_gpu_pack_t *pk, uint64_t s0,
                                                    uint64_t s1, uint32_t gl) {
    uint64_t x = s0 ^ opm64<OM>(lds, pk, 0, s1);
#pragma unroll
    for (int k = LOG2G - 1; k >= 0; k--) {
        const uint32_t d = 1u << k;
        const uint64_t hi = __shfl_down(x, d, 64);
        if (gl < d) x ^= opm64<OM>(lds, pk, 1 + k, hi);
    }
    return x;
}

template <int BLOCK, int OM>
__device__ void fill_lds64(uint8_t *lds, const crc64_gpu_pack_t *pk) {
    uint64_t *l = reinterpret_cast<uint64_t *>(lds);
    uint4 *l4 = reinterpret_cast<uint4 *>(lds);
    // f6: entry v of table i at i*16 KiB + v*256 B, 32 copies (two per 16-B write)
    for (uint32_t q = threadIdx.x; q < 4096u; q += BLOCK) {
        const uint64_t v = pk->f6[q >> 10][(q >> 4) & 63u];
        l4[kL64P6 / 16 + q] = make_uint4((uint32_t)v, (uint32_t)(v >> 32), (uint32_t)v, (uint32_t)(v >> 32));
    }
    for (uint32_t d = threadIdx.x; d < 256u; d += BLOCK) l[kL64P5 / 8 + d] = pk->f5[d >> 5][d & 31u];
    if constexpr (OM == kOpsLds) {
        const uint4 *ops = reinterpret_cast<const uint4 *>(&pk->ops[0][0][0]);
        const uint32_t nops = pk->nops * 128u;
        for (uint32_t q = threadIdx.x; q < nops; q += BLOCK) l4[kL64Main / 16 + q] = ops[q];
    } else if constexpr (OM == kOpsMix) {  // ops 1..6 (needs G = 64: nops >= 7)
        const uint4 *ops = reinterpret_cast<const uint4 *>(&pk->ops[1][0][0]);
        for (uint32_t q = threadIdx.x; q < 6u * 128u; q += BLOCK) l4[kL64Main / 16 + q] = ops[q];
    }
}

__device__ __forceinline__ uint64_t lo64(uint4 v) { return (uint64_t)v.y << 32 | v.x; }
__device__ __forceinline__ uint64_t hi64(uint4 v) { return (uint64_t)v.w << 32 | v.z; }

// Aligned CRC-64 loop: a 4-deep ring of dwordx4 loads per lane, two 64-bit
// sub-streams per lane.  Whole rings (K a multiple of the ring, K >= 2
// rings) take payload64_even: no load or step is conditional, so the waitcnt
// pass sees one load per step and waits vmcnt(R - 1) throughout.  In the
// merged segment kernel the general loop -- conditional ring fill and tail --
// kept only one or two loads in flight (vmcnt(1) in its steady loop,
// vmcnt(0) after the fill): +2.5% on seg for the even form
// (profiles/r04/ab_seg_even.log).
constexpr int kRing64 = 4;
template <int LOG2G, bool NT, int OM>
__device__ __forceinline__ uint64_t payload64_even(const uint8_t *lds, const crc64_gpu_pack_t *pk, const uint8_t *p,
                                                   uint32_t K, uint32_t gl, uint32_t lc, uint64_t init) {
    constexpr int G = 1 << LOG2G;
    constexpr int R = kRing64;
    Lane64 ln = lane64(lc);
    gbyte_t src = global_ptr(p, LOG2G == 6) + 16u * gl;
    uint4 ring[R];
#pragma unroll
    for (int u = 0; u < R; u++) ring[u] = ldg16<NT>(src + u * (16u * G));
    // x holds state ^ (the data word of the step about to run)
    uint64_t x0 = (gl == 0 ? init : 0ull) ^ lo64(ring[0]), x1 = hi64(ring[0]);
    for (uint32_t k = R; k < K; k += R) {
        src += R * (16u * G);
#pragma unroll
        for (int u = 0; u < R; u++) {
            ring[u] = ldg16<NT>(src + u * (16u * G));
            const uint4 nx = ring[(u + 1) % R];
            x0 = f64x(lds, x0, lo64(nx), ln);
            x1 = f64x(lds, x1, hi64(nx), ln);
        }
    }
#pragma unroll
    for (int u = 0; u < R; u++) {
        const uint4 nx = u + 1 < R ? ring[u + 1] : make_uint4(0, 0, 0, 0);
        x0 = f64x(lds, x0, lo64(nx), ln);
        x1 = f64x(lds, x1, hi64(nx), ln);
    }
    return combine64<LOG2G, OM>(lds, pk, x0, x1, gl);
}

// The split pieces' loop (G = 64, K a multiple of the ring and >= 2 rings):
// ring64_load issues a piece's first kRing64 steps -- early, while the
// previous piece still combines -- and fold64_ring runs the piece from them,
// leaving the two sub-stream registers uncombined.
template <bool NT>
__device__ __forceinline__ void ring64_load(uint4 (&ring)[kRing64], const uint8_t *p, uint32_t gl) {
    const gbyte_t src = global_ptr(p, true) + 16u * gl;
#pragma unroll
    for (int u = 0; u < kRing64; u++) ring[u] = ldg16<NT>(src + u * 1024u);
}
template <bool NT>
__device__ __forceinline__ void fold64_ring(const uint8_t *lds, uint4 (&ring)[kRing64], const uint8_t *p, uint32_t K,
                                            uint32_t gl, Lane64 &ln, uint64_t init, uint64_t *s0, uint64_t *s1) {
    constexpr int R = kRing64;
    gbyte_t src = global_ptr(p, true) + 16u * gl;
    uint64_t x0 = (gl == 0 ? init : 0ull) ^ lo64(ring[0]), x1 = hi64(ring[0]);
    for (uint32_t k = R; k < K; k += R) {
        src += R * 1024u;
#pragma unroll
        for (int u = 0; u < R; u++) {
            ring[u] = ldg16<NT>(src + u * 1024u);
            const uint4 nx = ring[(u + 1) % R];
            x0 = f64x(lds, x0, lo64(nx), ln);
            x1 = f64x(lds, x1, hi64(nx), ln);
        }
    }
#pragma unroll
    for (int u = 0; u < R; u++) {
        const uint4 nx = u + 1 < R ? ring[u + 1] : make_uint4(0, 0, 0, 0);
        x0 = f64x(lds, x0, lo64(nx), ln);
        x1 = f64x(lds, x1, hi64(nx), ln);
    }
    *s0 = x0;
    *s1 = x1;
}

template <int LOG2G, bool NT, int OM>
__device__ __forceinline__ uint64_t payload64_aligned(const uint8_t *lds, const crc64_gpu_pack_t *pk, const uint8_t *p,
                                                      uint32_t K, uint32_t gl, uint32_t lc, uint64_t init) {
    constexpr int G = 1 << LOG2G;
    constexpr int R = kRing64;
    if (K % R == 0 && K >= 2 * R) return payload64_even<LOG2G, NT, OM>(lds, pk, p, K, gl, lc, init);
    Lane64 ln = lane64(lc);
    // global (address-space 1) loads: a flat load would also hold up every LDS wait
    const gbyte_t src = global_ptr(p, LOG2G == 6) + 16u * gl;
    auto ldk = [&](uint32_t k) { return ldg16<NT>(src + (uint64_t)k * (16u * G)); };
    uint4 ring[R];
#pragma unroll
    for (int u = 0; u < R; u++) ring[u] = (uint32_t)u < K ? ldk(u) : make_uint4(0, 0, 0, 0);
    // x holds state ^ (the data word of the step about to run)
    uint64_t x0 = (gl == 0 ? init : 0ull) ^ lo64(ring[0]), x1 = hi64(ring[0]);
    uint32_t k = 0;
    for (; k + 2 * R <= K; k += R) {  // every load and look-ahead in range
#pragma unroll
        for (int u = 0; u < R; u++) {
            ring[u] = ldk(k + u + R);
            const uint4 nx = ring[(u + 1) % R];
            x0 = f64x(lds, x0, lo64(nx), ln);
            x1 = f64x(lds, x1, hi64(nx), ln);
        }
    }
    for (; k < K; k += R) {
#pragma unroll
        for (int u = 0; u < R; u++) {
            if (k + u + R < K) ring[u] = ldk(k + u + R);
            if (k + u < K) {
                const uint4 nx = k + u + 1 < K ? ring[(u + 1) % R] : make_uint4(0, 0, 0, 0);
                x0 = f64x(lds, x0, lo64(nx), ln);
                x1 = f64x(lds, x1, hi64(nx), ln);
            }
        }
    }
    return combine64<LOG2G, OM>(lds, pk, x0, x1, gl);
}

// COPY: the payload is also stored at dst (crc_gpu_pack_store.h), as in
// payload32_generic.
template <int LOG2G, bool NT, int OM = kOpsLds, bool COPY = false>
__device__ __forceinline__ uint64_t payload64_generic(const uint8_t *lds, const crc64_gpu_pack_t *pk,
                                                      const uint8_t *p, uint64_t len, uint32_t gl, uint32_t lc,
                                                      uint8_t *dst = nullptr) {
    const uint64_t init = pk->init;
    const LaneWindow win(reinterpret_cast<uint64_t>(p), len, 8, LOG2G);
    const int64_t K = win.K, r0 = win.r0, step = win.step, hs = win.hs, he = win.he;
    const int64_t ilen = (int64_t)len;
    const int64_t kmax = LOG2G == 6 ? K : wave_max(K);
    const int64_t lane_off = 16 * (int64_t)gl;

    const gbyte_t g0 = global_ptr(reinterpret_cast<const uint8_t *>(win.a0), false);
    auto fetch = [&](int64_t k) -> uint4 {
        const int64_t pc = r0 + k * step + lane_off;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < K && pc >= 0) v = ldg16<NT>(g0 + (uint64_t)pc);
        return v;
    };
    // edge handling (crc_gpu_mask.h) for the piece of step k < K
    auto prep = [&](int64_t k, uint4 v, uint64_t *w0, uint64_t *w1) {
        const int64_t pc = r0 + k * step + lane_off;
        *w0 = lo64(v);
        *w1 = hi64(v);
        if (!mck_piece_clean(pc, hs, he, 8)) {
            const int64_t lo = pc - hs;
            *w0 = mck_mask64(*w0, lo, ilen, init);
            *w1 = mck_mask64(*w1, lo + 8, ilen, init);
        }
    };

    uint4 ring[kRing];
#pragma unroll
    for (int u = 0; u < kRing; u++) ring[u] = fetch(u);
    uint64_t x0 = 0, x1 = 0;
    Lane64 ln = lane64(lc);
    for (int64_t k = 0; k < kmax; k += kRing) {
#pragma unroll
        for (int u = 0; u < kRing; u++) {
            const int64_t j = k + u;
            const uint4 raw = ring[u];
            ring[u] = fetch(j + kRing);
            if (j < K) {
                if constexpr (COPY) store_piece((gwbyte_t)dst, mck_lane_piece_store(win, j, win.piece(j, lane_off)), raw);
                uint64_t w0, w1;
                prep(j, raw, &w0, &w1);
                x0 = f64x(lds, x0 ^ w0, 0, ln);
                x1 = f64x(lds, x1 ^ w1, 0, ln);
            }
        }
    }
    uint64_t x = combine64<LOG2G, OM>(lds, pk, x0, x1, gl);
    x = opm64<OM>(lds, pk, 1 + LOG2G + win.pad(), x);
    if (len < 8) x ^= pk->zinit[len];
    return x;
}

template <int OM>
__device__ __forceinline__ uint64_t tail64(const uint8_t *lds, const crc64_gpu_pack_t *pk, uint32_t t, uint64_t x) {
    x = opm64<OM>(lds, pk, 1 + 6 + (t & 15u), x);
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
        if ((t >> (4 + k)) & 1u) x = opm64<OM>(lds, pk, 1 + k, x);
    return x;
}

// CRC-64 counterpart of payload32_g64 (a non-zero RAW `reg` needs len >= 8).
// COPY: as there -- the lane that folds a piece also stores it at dst + (the
// piece's position in the payload); dst is wave-uniform, at any alignment.
template <bool NT, bool RAW = false, int OM = kOpsLds, bool COPY = false>
__device__ __forceinline__ uint64_t payload64_g64(const uint8_t *lds, const crc64_gpu_pack_t *pk, const uint8_t *p,
                                                  uint64_t len, uint32_t gl, uint32_t lc, uint64_t reg = 0ull,
                                                  uint8_t *dst = nullptr) {
    const uint64_t init = RAW ? reg : pk->init;
    const GridWindow win(reinterpret_cast<uint64_t>(p), len, 8);
    const uint32_t K = win.K, lead = win.lead;
    const gbyte_t wb = global_ptr(reinterpret_cast<const uint8_t *>(win.origin), true);
    const int32_t ilen = (int32_t)len;
    const uint32_t lo_lane = 16u * gl;
    const uint32_t qs = win.qs, kc0 = win.kc0, kc1 = win.kc1;  // steps [kc0, kc1) are clean for every lane
    constexpr uint32_t R = kRingOff64;

    uint64_t x0 = 0, x1 = 0;
    Lane64 ln = lane64(lc);
    [[maybe_unused]] gwbyte_t db = nullptr;
    if constexpr (COPY) db = (gwbyte_t)uniform64(reinterpret_cast<uint64_t>(dst));
    auto fold = [&](uint32_t kk, uint4 v) {
        // (the raw piece: the masking below XORs the initial register into it)
        if constexpr (COPY) store_piece(db, mck_grid_piece_store(win, kk, gl), v);
        uint64_t w0 = lo64(v), w1 = hi64(v);
        if (kk < kc0 || kk >= kc1) {  // wave-uniform: an edge step
            const int32_t lo = (int32_t)(kk * 1024u + lo_lane) - (int32_t)qs;
            w0 = mck_mask64(w0, lo, ilen, init);
            w1 = mck_mask64(w1, lo + 8, ilen, init);
        }
        x0 = f64x(lds, x0 ^ w0, 0, ln);
        x1 = f64x(lds, x1 ^ w1, 0, ln);
    };
    uint4 ring[R];
    ring[0] = K > 0 && lo_lane >= lead ? ldg16<NT>(wb + lo_lane) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (uint32_t u = 1; u < R; u++) ring[u] = u < K ? ldg16<NT>(wb + (u * 1024u + lo_lane)) : make_uint4(0, 0, 0, 0);
    uint32_t k = 0;
    for (; k + 2 * R <= K; k += R) {
#pragma unroll
        for (uint32_t u = 0; u < R; u++) {
            const uint4 v = ring[u];
            ring[u] = ldg16<NT>(wb + ((k + u + R) * 1024u + lo_lane));
            fold(k + u, v);
        }
    }
    for (; k < K; k += R) {
#pragma unroll
        for (uint32_t u = 0; u < R; u++) {
            const uint4 v = ring[u];
            if (k + u + R < K) ring[u] = ldg16<NT>(wb + ((k + u + R) * 1024u + lo_lane));
            if (k + u < K) fold(k + u, v);
        }
    }
    uint64_t x;
    if constexpr (OM == kOpsMix) {  // the offsets batches (see combine64_lane0)
        x = combine64_lane0<6, OM>(lds, pk, x0, x1, gl);
        if (gl == 0) x = tail64<OM>(lds, pk, win.pad(), x);
        x = uniform64(x);
    } else {  // the segment and XDR kernels: the halving form there cost the
              // segment chunk pass 6.8% (register allocation of its other paths,
              // profiles/r06/ab_seg_lane0.log)
        x = combine64<6, OM>(lds, pk, x0, x1, gl);
        x = tail64<OM>(lds, pk, win.pad(), x);
    }
    if (!RAW && len < 8) x ^= pk->zinit[len];
    return x;
}

__device__ __forceinline__ uint64_t shift64(const crc64_shift_pack_t *sp, uint64_t x, uint64_t n) {
    for (int k = 0; n; k++, n >>= 4) {
        const uint32_t d = (uint32_t)(n & 15u);
        if (d) {
            const uint64_t *t = &sp->op[k][d - 1][0][0];
            uint64_t r = 0;
#pragma unroll
            for (int h = 0; h < 16; h++) r ^= t[h * 16 + ((x >> (4 * h)) & 15u)];
            x = r;
        }
    }
    return x;
}

// SPLIT (aligned batches of large payloads, G = 64): a unit is one
// kSplitBytes piece q of payload p, so the work queue balances pieces instead
// of whole 1 MiB payloads (one per wave at C3's shape: the slowest XCD set the
// launch time).  By linearity the payload's register is the XOR over pieces of
// Z^(bytes after piece q)(L_q), L_0 carrying the initial value; each piece
// adds its term (and piece 0 the final XOR) to out[p] with a 64-bit atomic
// XOR, into an output the host zeroed before the launch.
// OP: as in crc32c_batch_kernel (checksum, verify and update only).
template <int LOG2G, int MODE, int OP, bool NT, bool SPLIT = false>
__global__ __launch_bounds__(kBlk64<MODE * 16 + LOG2G>, kWpe64<MODE * 16 + LOG2G>) void crc64_batch_kernel(BatchArgs a) {
    static_assert(mck::kernel_key_valid(mck::KernelKey{64, LOG2G, MODE, OP, NT, false, SPLIT}), "no such batch kernel");
    enum : bool { VERIFY = OP == mck::kOpVerify, SEED = OP == mck::kOpUpdate };  // (enumerators: see crc32c_batch_kernel)
    using S = Shape<64, MODE, false, LOG2G>;
    constexpr int kWPB = S::block / 64;
    __shared__ __attribute__((aligned(16))) uint8_t lds[S::lds64_bytes];
    const crc64_gpu_pack_t *pk = reinterpret_cast<const crc64_gpu_pack_t *>(a.pack);
    constexpr int PPW = 64 >> LOG2G;
    // split launches: the plan with the finer tail pieces (SplitPlan)
    const SplitPlan splan(SPLIT ? a.count : 0, SPLIT ? a.split_log2 : 1u, gridDim.x);
    const uint64_t units = MODE == kOffsets ? a.count : SPLIT ? splan.n : (a.count + PPW - 1) / PPW;
    __shared__ WgQueue wgq;
    constexpr bool DYN = dyn_policy(64, MODE, NT, false) || SPLIT;
    MCK_STAMP(blockIdx.x * kWPB + (threadIdx.x >> 6), 0);
    if (DYN && threadIdx.x == 0) {
        if constexpr (SPLIT) wg_queue_init_plan(&wgq, a.queue, splan);
        else wg_queue_init(&wgq, a.queue, units);
    }
    // split pieces combined in the workgroup (SPLIT, split_lds): per set
    // (chunk sequence number % kAccSets) and payload (% kSplitAcc) the XOR of
    // the pieces' terms, their count and the owning chunk (sequence + 1; 0 free)
    __shared__ unsigned long long sacc[SPLIT ? kAccSets * kSplitAcc : 1];
    __shared__ unsigned int scnt[SPLIT ? kAccSets * kSplitAcc : 1];
    __shared__ unsigned int stag[SPLIT ? kAccSets * kSplitAcc : 1];
    if (SPLIT && threadIdx.x < kAccSets * kSplitAcc) {
        sacc[threadIdx.x] = 0;
        scnt[threadIdx.x] = 0;
        stag[threadIdx.x] = 0;
    }
    fill_lds64<S::block, S::ops_mode>(lds, pk);
    __syncthreads();
    MCK_STAMP(blockIdx.x * kWPB + (threadIdx.x >> 6), 1);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = lane & ((1u << LOG2G) - 1u), grp = lane >> LOG2G;
    const uint32_t lc = (lane & 31u) << 3;
    const uint64_t xorout = pk->xorout;
    const uint32_t nw = gridDim.x * kWPB;
    uint32_t nbad = 0;  // verify: this lane's mismatches (add_mismatches)
    // A static split with fewer units than waves numbers the waves across
    // workgroups first, so a small batch spreads over CUs (the host then
    // launches one workgroup per unit) instead of filling one CU's LDS
    // pipe: 64 x 4 KiB took 18.4 us packed into one workgroup.
    const bool spread = !DYN && units < nw;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(spread ? (threadIdx.x >> 6) * gridDim.x + blockIdx.x
                                                                : blockIdx.x * kWPB + (threadIdx.x >> 6));

    if (MODE == kOffsets) {
        auto one = [&](uint64_t p) {
            const uint64_t o = a.offsets[p];
            const uint64_t n = a.offsets[p + 1] - o;
            const uint64_t x = n < (1ull << 31) ? payload64_g64<NT, false, S::ops_mode>(lds, pk, a.base + o, n, gl, lc)
                                                : payload64_generic<LOG2G, NT, S::ops_mode>(lds, pk, a.base + o, n, gl, lc);
            if constexpr (SEED) {
                if (gl == 0) {
                    uint64_t *st = reinterpret_cast<uint64_t *>(a.out) + p;
                    *st = mck_seed64(reinterpret_cast<const crc64_shift_pack_t *>(a.shift), x, *st, pk->init, n);
                }
            } else {
                if (gl == 0) emit<uint64_t, VERIFY>(a, p, x ^ xorout, nbad);
            }
        };
        if (for_each_unit<true>(&wgq, a.queue, units, wave, nw, one)) fail_closed<VERIFY>(a);
        if constexpr (VERIFY) add_mismatches(a.mismatches, nbad);
        return;
    }
    if constexpr (SPLIT) {  // (kernel_key_valid: aligned G = 64 checksums)
        const crc64_shift_pack_t *sp = reinterpret_cast<const crc64_shift_pack_t *>(a.shift);
        unsigned long long *out = reinterpret_cast<unsigned long long *>(a.out);
        // In-workgroup combine (split_lds, a slot launch whose queue chunks hold
        // whole payloads): per ring entry and payload, the XOR of the pieces'
        // terms and their count; the last piece stores the CRC -- no zeroing
        // launch and no global atomics.  Otherwise (graph captures: static
        // split) each piece XORs its term into the out[] the host zeroed.
        // (The host's check is repeated here: a mismatch is a fault, never a
        // silently wrong value.)
        const bool in_wg = a.split_lds && a.queue && splan.whole();
        if (a.split_lds && !in_wg) {  // host and device disagree: fail closed, reported once per launch
            if (blockIdx.x == 0 && threadIdx.x < 64) {
                if (threadIdx.x == 0) queue_fault(13, units, a.split_log2);
                fail_closed<false>(a);
            }
            return;
        }
        // Pipelined (round 6): a wave takes its NEXT piece as soon as the
        // current one's step loop ends and issues that piece's first loads,
        // so their HBM round trip overlaps the current piece's lane combine,
        // Z^n shift and accumulation (before, each 256 KiB piece waited one
        // HBM latency at its start, after its predecessor's combine).  A
        // taken piece's ring read counts at once (no deferred reader), so the
        // accumulators are keyed by the chunk's sequence number instead of
        // its ring entry: set seq % kAccSets, owner tag seq + 1.  A piece
        // whose entry an older chunk still holds waits for it (bounded; the
        // older chunk's pieces are all taken and never wait on this one); a
        // newer owner means one wave held every taken piece of its chunk while
        // the workgroup's other waves finished kAccSets - 1 whole chunks (most
        // of a launch at a 256 KiB piece per wave and chunk) -- a fault, never
        // a value.
        const uint32_t pieces = 1u << splan.psl;
        const uint64_t bytes = a.len >> splan.psl;  // kSplitBytes
        const uint32_t K = (uint32_t)(bytes >> 10);
        auto src_of = [&](uint64_t u, uint64_t *p, uint32_t *q) {
            splan.unit(u, p, q);
            return a.base + *p * a.stride + (uint64_t)*q * bytes;
        };
        UnitTaker<SplitPlan> tk(&wgq, a.queue, units, wave, nw, false, splan);
        Lane64 ln = lane64(lc);
        uint4 ring[kRing64];
        uint64_t u, p = 0;
        uint32_t q = 0;
        bool have = tk.take_unit(&u);
        uint32_t seq = tk.seq;
        const uint8_t *src = have ? src_of(u, &p, &q) : a.base;
        if (have) ring64_load<NT>(ring, src, gl);
        while (have) {
            uint64_t x0, x1;
            fold64_ring<NT>(lds, ring, src, K, gl, ln, q == 0 ? pk->init : 0ull, &x0, &x1);
            uint64_t un = 0, pn = 0;
            uint32_t qn = 0;
            const bool next = tk.take_unit(&un);
            const uint32_t seqn = tk.seq;
            const uint8_t *srcn = next ? src_of(un, &pn, &qn) : src;
            if (next) ring64_load<NT>(ring, srcn, gl);  // in flight during the combine below
            const uint64_t x = combine64<6, kOpsLds>(lds, pk, x0, x1, gl);
            if (gl == 0) {
                const uint64_t t = shift64(sp, x, (uint64_t)(pieces - 1 - q) * bytes) ^ (q == 0 ? xorout : 0ull);
                if (in_wg) {
                    const uint32_t ai = (seq % kAccSets) * kSplitAcc + (uint32_t)(p & (kSplitAcc - 1));
                    const uint32_t me = seq + 1;
                    Deadline dl(abort_word(a.queue));
                    bool own = false;
                    for (;;) {
                        const uint32_t tg = lds_ld(&stag[ai]);
                        if (tg == me) {
                            own = true;
                            break;
                        }
                        if (tg == 0u) {
                            unsigned int expect = 0u;
                            if (__hip_atomic_compare_exchange_strong(&stag[ai], &expect, me, __ATOMIC_ACQ_REL,
                                                                     __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                                own = true;
                                break;
                            }
                            continue;
                        }
                        if (tg > me) {  // a newer chunk on this entry: fail closed
                            queue_fault(16, seq, tg);
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                        if (dl.passed()) {  // the older chunk never finished
                            queue_fault(17, seq, tg);
                            raise_abort(a.queue);
                            break;
                        }
                    }
                    if (own) {
                        // (one wave's LDS atomics are performed in order: a
                        // piece's XOR lands before its count, the last piece's
                        // reset before the entry's release)
                        __hip_atomic_fetch_xor(&sacc[ai], (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        const uint32_t seen = __hip_atomic_fetch_add(&scnt[ai], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (seen == pieces - 1) {
                            out[p] = __hip_atomic_exchange(&sacc[ai], 0ull, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_store(&scnt[ai], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_store(&stag[ai], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    } else {
                        tk.flt = 1;
                    }
                } else {
                    atomicXor(out + p, (unsigned long long)t);
                }
            }
            have = next;
            u = un;
            p = pn;
            q = qn;
            seq = seqn;
            src = srcn;
        }
        const bool faulted = tk.finish(wave);
        if (faulted) fail_closed<false>(a);
        MCK_STAMP(blockIdx.x * kWPB + (threadIdx.x >> 6), 2);
        return;
    }
    const bool faulted = for_each_unit<DYN>(&wgq, a.queue, units, wave, nw, [&](uint64_t u) {
        const uint64_t p = u * PPW + grp;
        const bool act = p < a.count;
        const uint64_t pc = act ? p : a.count - 1;
        uint64_t x;
        if constexpr (MODE == kFixedAligned)
            x = payload64_aligned<LOG2G, NT, S::ops_mode>(lds, pk, a.base + pc * a.stride, (uint32_t)(a.len >> (4 + LOG2G)), gl, lc, pk->init);
        else
            x = payload64_generic<LOG2G, NT>(lds, pk, a.base + pc * a.stride, a.len, gl, lc);
        if (act && gl == 0) emit<uint64_t, VERIFY>(a, p, x ^ xorout, nbad);
    });
    if (faulted) fail_closed<VERIFY>(a);
    if constexpr (VERIFY) add_mismatches(a.mismatches, nbad);
    MCK_STAMP(blockIdx.x * kWPB + (threadIdx.x >> 6), 2);
}

}  // namespace

#endif  // CRC_GPU_CRC64_H
