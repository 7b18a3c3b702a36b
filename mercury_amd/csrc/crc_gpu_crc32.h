// crc_gpu_crc32.h -- CRC-32C on the device: LDS table access, the step fold,
// the sub-stream combine, the LDS fill, the payload loops, the Z^n register
// shift and the persistent batch kernel.  Algebra: crc_gpu_layout.h.
#ifndef CRC_GPU_CRC32_H
#define CRC_GPU_CRC32_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "crc_gpu_common.h"
#include "crc_gpu_layout.h"
#include "crc_gpu_mask.h"
#include "crc_gpu_queue.h"
#include "crc_gpu_seed.h"
#include "crc_gpu_shape.h"
#include "crc_gpu_window.h"
#include "launch_plan.h"

namespace {

// CRC-32C table access policy: Tab32<false> = 32x-replicated conflict-free
// layout (throughput), Tab32<true> = light layout (latency of small batches).
template <bool LIGHT>
struct Tab32 {
    const uint8_t *lds;
};

// Z^(16G)(x): main[p][byte_p(x)], tables p=0,1 in LDS region 0 (lc0), p=2,3
// in region 1 (lc1 has +64 KiB in its byte 2); odd p at +128 B.  One step of
// a sub-stream costs 4 v_perm + 2 v_bitop3 (+1 XOR with the data word) per
// 4 bytes.  (Folding the next word into this XOR tree instead -- a look-ahead
// pipeline -- measured 7% slower on the headline batch, profiles/r01/ab3.log.)
__device__ __forceinline__ uint32_t f32s(Tab32<false> t, uint32_t x, uint32_t lc0, uint32_t lc1) {
    const uint32_t a0 = __builtin_amdgcn_perm(x, lc0, 0x0C020400u);
    const uint32_t a1 = __builtin_amdgcn_perm(x, lc0, 0x0C020500u);
    const uint32_t a2 = __builtin_amdgcn_perm(x, lc1, 0x0C020600u);
    const uint32_t a3 = __builtin_amdgcn_perm(x, lc1, 0x0C020700u);
    return xor3(lds32(t.lds, a0), lds32(t.lds, a1 + 128), lds32(t.lds, a2)) ^ lds32(t.lds, a3 + 128);
}

__device__ __forceinline__ uint32_t f32s(Tab32<true> t, uint32_t x, uint32_t, uint32_t) {
    const uint32_t a0 = (x << 2) & 0x3FCu, a1 = (x >> 6) & 0x3FCu, a2 = (x >> 14) & 0x3FCu, a3 = (x >> 22) & 0x3FCu;
    return xor3(lds32(t.lds, a0), lds32(t.lds, a1 + 1024), lds32(t.lds, a2 + 2048)) ^ lds32(t.lds, a3 + 3072);
}

// Z^(16G)(x) ^ extra: the fourth lookup and the next data word share one bitop3.
__device__ __forceinline__ uint32_t f32sx(Tab32<false> t, uint32_t x, uint32_t extra, uint32_t lc0, uint32_t lc1) {
    const uint32_t a0 = __builtin_amdgcn_perm(x, lc0, 0x0C020400u);
    const uint32_t a1 = __builtin_amdgcn_perm(x, lc0, 0x0C020500u);
    const uint32_t a2 = __builtin_amdgcn_perm(x, lc1, 0x0C020600u);
    const uint32_t a3 = __builtin_amdgcn_perm(x, lc1, 0x0C020700u);
    return xor3(xor3(lds32(t.lds, a0), lds32(t.lds, a1 + 128), lds32(t.lds, a2)), lds32(t.lds, a3 + 128), extra);
}
__device__ __forceinline__ uint32_t f32sx(Tab32<true> t, uint32_t x, uint32_t extra, uint32_t lc0, uint32_t lc1) {
    return f32s(t, x, lc0, lc1) ^ extra;
}

template <bool LIGHT>
__device__ __forceinline__ uint32_t op32(Tab32<LIGHT> tab, uint32_t o, uint32_t x) {
    const uint32_t base = (LIGHT ? kL32LightMain : kL32Main) + o * 512;
    uint32_t t[8];
#pragma unroll
    for (int h = 0; h < 8; h++) t[h] = lds32(tab.lds, base + h * 64 + (((x >> (4 * h)) & 15u) << 2));
    return xor3(xor3(t[0], t[1], t[2]), xor3(t[3], t[4], t[5]), t[6] ^ t[7]);
}

// Lane-dependent operator i of level l of the two-level combine (LDS map:
// crc_gpu_shape.h; interleaved so that lanes with different i hit different banks).
__device__ __forceinline__ uint32_t oplv32(Tab32<false> tab, uint32_t l, uint32_t i, uint32_t x) {
    const uint32_t base = kL32Lv + l * 4096 + i * 4;
    uint32_t t[8];
#pragma unroll
    for (int h = 0; h < 8; h++) t[h] = lds32(tab.lds, base + h * 512 + (((x >> (4 * h)) & 15u) << 5));
    return xor3(xor3(t[0], t[1], t[2]), xor3(t[3], t[4], t[5]), t[6] ^ t[7]);
}

// XOR_q Z^(-4q)(S_q) in the lane, then over the G lanes of the group.  For
// G = 64 on the throughput layout: lane l = 8a + b applies
// Z^(-16b), the 8 lanes of each a XOR-reduce (shuffles only), the groups
// apply Z^(-128a) and XOR-reduce -- two table operators on the lane's path
// instead of six butterfly levels of one each.
template <int LOG2G, class TAB>
__device__ __forceinline__ uint32_t combine32(TAB lds, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3,
                                              uint32_t gl) {
    uint32_t x = s0 ^ op32(lds, 0, s1);
    const uint32_t y = s2 ^ op32(lds, 0, s3);
    x ^= op32(lds, 1, y);
    if constexpr (LOG2G == 6 && std::is_same<TAB, Tab32<false>>::value) {
        x = oplv32(lds, 0, gl & 7u, x);
        x ^= __shfl_xor(x, 1, 64);
        x ^= __shfl_xor(x, 2, 64);
        x ^= __shfl_xor(x, 4, 64);
        x = oplv32(lds, 1, gl >> 3, x);
        x ^= __shfl_xor(x, 8, 64);
        x ^= __shfl_xor(x, 16, 64);
        x ^= __shfl_xor(x, 32, 64);
        return x;
    }
#pragma unroll
    for (int k = 0; k < LOG2G; k++) {
        const uint32_t other = __shfl_xor(x, 1 << k, 64);
        const bool bit = (gl >> k) & 1u;
        const uint32_t lo = bit ? other : x, hi = bit ? x : other;
        x = lo ^ op32(lds, 2 + k, hi);
    }
    return x;
}

// LDS fill in 16-byte granules: a replicated entry's 4 neighbouring copies are
// one ds_write_b128 of the same value (8 per thread at 1024 threads instead of
// 32 dword loads + writes); the operator tables are copied as uint4.  The
// throughput layout issues every load of the fill (8 table entries, one
// operator granule, one combine-operator granule per thread) before its first
// write, so the fill costs one global round trip instead of three (round 2 ran
// the three copies one after another, each behind its own wait).
// `issue` runs between the fill's loads and its LDS writes (the kernel's
// first-payload prefetch: issued after the table loads, it does not delay
// their writes).
struct NoIssue {
    __device__ void operator()() const {}
};
template <bool LIGHT, int BLOCK, class F = NoIssue>
__device__ void fill_lds32(uint8_t *lds, const crc32_gpu_pack_t *pk, F &&issue = F{}) {
    uint4 *l4 = reinterpret_cast<uint4 *>(lds);
    const uint4 *ops = reinterpret_cast<const uint4 *>(&pk->ops[0][0][0]);
    const uint32_t nops = pk->nops * 32u;
    if constexpr (LIGHT) {
        // all loads (one main-table granule, up to three operator granules per
        // thread) before the first write: one global round trip, not two
        static_assert(BLOCK == 256 && CRC32_NOPS_MAX * 32 <= 3 * BLOCK, "fill granules per thread");
        issue();
        const uint4 *m = reinterpret_cast<const uint4 *>(&pk->main[0][0]);
        const uint32_t t = threadIdx.x;
        const uint4 mv = m[t];
        auto op_at = [&](uint32_t q) { return ops[q < CRC32_NOPS_MAX * 32u ? q : 0u]; };
        uint4 o0 = op_at(t), o1 = op_at(t + BLOCK), o2 = op_at(t + 2 * BLOCK);
        // (pinned after all four loads are out: the compiler sank each
        // operator load into its predicated store, one round trip apiece)
        asm volatile("" : "+v"(o0.x), "+v"(o0.y), "+v"(o0.z), "+v"(o0.w), "+v"(o1.x), "+v"(o1.y), "+v"(o1.z),
                     "+v"(o1.w), "+v"(o2.x), "+v"(o2.y), "+v"(o2.z), "+v"(o2.w));
        l4[t] = mv;
        if (t < nops) l4[kL32LightMain / 16 + t] = o0;
        if (t + BLOCK < nops) l4[kL32LightMain / 16 + t + BLOCK] = o1;
        if (t + 2 * BLOCK < nops) l4[kL32LightMain / 16 + t + 2 * BLOCK] = o2;
    } else {
        static_assert(BLOCK == 1024 && CRC32_NOPS_MAX * 32 <= BLOCK, "one operator granule per thread");
        const uint32_t t = threadIdx.x;
        const uint4 *lv = reinterpret_cast<const uint4 *>(&pk->lv[0][0][0][0]);  // two-level combine operators
        // loads in range of the pack's arrays whatever nops is (so none waits
        // for the scalar load of nops), stores predicated
        const uint32_t tc = t < CRC32_NOPS_MAX * 32u ? t : 0u, tl = t & 511u;
        uint4 o = ops[tc];
        const uint4 w = lv[tl];
        uint32_t v[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) {
            const uint32_t d = (t + i * BLOCK) << 2;
            const uint32_t region = d >> 14, e = (d >> 6) & 255u, half = (d >> 5) & 1u;
            v[i] = pk->main[2 * region + half][e];
        }
        // keep the operator load up here with the others (the compiler would
        // sink it into the predicated store below, behind a second round trip)
        asm volatile("" : "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(o.w));
        issue();
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) l4[t + i * BLOCK] = make_uint4(v[i], v[i], v[i], v[i]);
        if (t < nops) l4[kL32Main / 16 + t] = o;
        if (t < 512u) l4[kL32Lv / 16 + t] = w;
    }
}

// (The copying payload loops' store of a piece, store_piece: crc_gpu_common.h.)
//
// Ring slot j % kRing holds the piece of step j, loaded kRing steps ahead.
//
// Aligned fixed-size payload: base 16-B aligned, len = K * 16G, no masking,
// no pad bytes (tail op is the identity and is skipped).
// Aligned step loop without per-step tests: K is a multiple of kRing and
// >= kRing (launch_fixed's aligned test), so every load of the steady loop is
// in range and the last kRing steps run without loads.  The load pointer
// advances by kRing steps per iteration (for G = 64 a wave-uniform SGPR pair:
// saddr loads with the lane offset in one VGPR and the slot in the immediate).
// Each slot's data word is folded into the state before the slot is reloaded,
// so the ring needs no register copies.
// The first kRing steps of a payload (every one in range: K >= kRing).
template <int LOG2G, bool NT>
__device__ __forceinline__ void ring32_load(uint4 (&ring)[kRing], const uint8_t *p, uint32_t gl) {
    constexpr uint32_t S = 16u << LOG2G;
    const gbyte_t lb = global_ptr(p, LOG2G == 6);
#pragma unroll
    for (uint32_t u = 0; u < kRing; u++) ring[u] = ldg16<NT>(lb + (16u * gl + u * S));
}

// loaded: ring already holds the payload's first kRing steps (ring32_load,
// issued by the kernel before its LDS fill for the wave's first payload).
template <int LOG2G, bool NT, class TAB>
__device__ __forceinline__ uint32_t payload32_aligned(TAB lds, const uint8_t *p, uint64_t K64, uint32_t gl,
                                                      uint32_t lc0, uint32_t lc1, uint32_t init,
                                                      uint4 (&ring)[kRing], bool loaded) {
    constexpr uint32_t G = 1u << LOG2G;
    constexpr uint32_t R = kRing;
    constexpr uint32_t S = 16u * G;  // bytes per step
    const uint32_t K = (uint32_t)K64;
    gbyte_t lb = global_ptr(p, LOG2G == 6);
    const uint32_t lo = 16u * gl;
    if (!loaded) ring32_load<LOG2G, NT>(ring, p, gl);
    lb += R * S;
    uint32_t x0 = gl == 0 ? init : 0u, x1 = 0, x2 = 0, x3 = 0;
    // look-ahead: y holds state ^ (data of the step about to run), and the
    // next step's data word rides in the table-XOR tree (2 v_bitop3, no XOR)
    uint32_t y0 = x0 ^ ring[0].x, y1 = ring[0].y, y2 = ring[0].z, y3 = ring[0].w;
    for (uint32_t k = R; k < K; k += R) {
#pragma unroll
        for (uint32_t u = 0; u < R; u++) {
            ring[u] = ldg16<NT>(lb + (lo + u * S));
            const uint4 nx = ring[(u + 1) % R];
            y0 = f32sx(lds, y0, nx.x, lc0, lc1);
            y1 = f32sx(lds, y1, nx.y, lc0, lc1);
            y2 = f32sx(lds, y2, nx.z, lc0, lc1);
            y3 = f32sx(lds, y3, nx.w, lc0, lc1);
        }
        lb += R * S;
    }
#pragma unroll
    for (uint32_t u = 0; u + 1 < R; u++) {
        const uint4 nx = ring[u + 1];
        y0 = f32sx(lds, y0, nx.x, lc0, lc1);
        y1 = f32sx(lds, y1, nx.y, lc0, lc1);
        y2 = f32sx(lds, y2, nx.z, lc0, lc1);
        y3 = f32sx(lds, y3, nx.w, lc0, lc1);
    }
    x0 = f32s(lds, y0, lc0, lc1);
    x1 = f32s(lds, y1, lc0, lc1);
    x2 = f32s(lds, y2, lc0, lc1);
    x3 = f32s(lds, y3, lc0, lc1);
    return combine32<LOG2G>(lds, x0, x1, x2, x3, gl);
}
template <int LOG2G, bool NT, class TAB>
__device__ __forceinline__ uint32_t payload32_aligned(TAB lds, const uint8_t *p, uint64_t K, uint32_t gl,
                                                      uint32_t lc0, uint32_t lc1, uint32_t init) {
    uint4 ring[kRing];
    return payload32_aligned<LOG2G, NT>(lds, p, K, gl, lc0, lc1, init, ring, false);
}

// Any alignment, any length (0 included).  Per-lane window; the wave loops to
// the largest step count of its groups.  COPY: the payload is also stored at
// dst (crc_gpu_pack_store.h).
template <int LOG2G, bool NT, class TAB, bool COPY = false>
__device__ __forceinline__ uint32_t payload32_generic(TAB lds, const crc32_gpu_pack_t *pk,
                                                      const uint8_t *p, uint64_t len, uint32_t gl, uint32_t lc0,
                                                      uint32_t lc1, uint8_t *dst = nullptr) {
    const uint32_t init = pk->init;
    const LaneWindow win(reinterpret_cast<uint64_t>(p), len, 4, LOG2G);
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
    auto prep = [&](int64_t k, uint4 v) -> uint4 {
        const int64_t pc = r0 + k * step + lane_off;
        if (!mck_piece_clean(pc, hs, he, 4)) {
            const int64_t lo = pc - hs;
            v.x = mck_mask32(v.x, lo, ilen, init);
            v.y = mck_mask32(v.y, lo + 4, ilen, init);
            v.z = mck_mask32(v.z, lo + 8, ilen, init);
            v.w = mck_mask32(v.w, lo + 12, ilen, init);
        }
        return v;
    };

    uint4 ring[kRing];
#pragma unroll
    for (int u = 0; u < kRing; u++) ring[u] = fetch(u);
    uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
    for (int64_t k = 0; k < kmax; k += kRing) {
#pragma unroll
        for (int u = 0; u < kRing; u++) {
            const int64_t j = k + u;
            const uint4 raw = ring[u];
            ring[u] = fetch(j + kRing);
            if (j < K) {
                if constexpr (COPY) store_piece((gwbyte_t)dst, mck_lane_piece_store(win, j, win.piece(j, lane_off)), raw);
                const uint4 w = prep(j, raw);
                x0 = f32s(lds, x0 ^ w.x, lc0, lc1);
                x1 = f32s(lds, x1 ^ w.y, lc0, lc1);
                x2 = f32s(lds, x2 ^ w.z, lc0, lc1);
                x3 = f32s(lds, x3 ^ w.w, lc0, lc1);
            }
        }
    }
    uint32_t x = combine32<LOG2G>(lds, x0, x1, x2, x3, gl);
    x = op32(lds, 2 + LOG2G + win.pad(), x);
    if (len < 4) x ^= pk->zinit[len];
    return x;
}

template <class TAB>
__device__ __forceinline__ uint32_t tail32(TAB lds, uint32_t t, uint32_t x) {
    x = op32(lds, 2 + 6 + (t & 15u), x);
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
        if ((t >> (4 + k)) & 1u) x = op32(lds, 2 + k, x);
    return x;
}

// One payload per wave (G = 64): the window geometry is wave-uniform, so the
// payload base stays in SGPRs, each lane carries a 32-bit offset (saddr-form
// global loads), and "does this step touch an edge?" is a scalar test -- only
// the first/last steps pay for per-lane masking.  Payloads < 2 GiB.
// RAW: no finalisation and the register starts at `reg` (default 0: the
// linear part L(M) of the CRC, used to combine the pieces of a scatter-gather
// object, mchecksum_gpu_ext.hip); a non-zero `reg` continues a running
// register (the XDR walker's fields) and needs len >= 4, since it rides in
// the first four payload bytes (R(reg, M) = R(0, M ^ reg)).
// COPY: the lane that folds a piece also stores it at dst + (the piece's
// position in the payload), crc_gpu_pack_store.h: the payload is read once for
// the copy and the CRC.  dst is wave-uniform, at any alignment.
template <bool NT, class TAB, bool RAW = false, bool COPY = false>
__device__ __forceinline__ uint32_t payload32_g64(TAB lds, const crc32_gpu_pack_t *pk, const uint8_t *p,
                                                  uint64_t len, uint32_t gl, uint32_t lc0, uint32_t lc1,
                                                  uint32_t reg = 0u, uint8_t *dst = nullptr) {
    const uint32_t init = RAW ? reg : pk->init;
    const GridWindow win(reinterpret_cast<uint64_t>(p), len, 4);
    const uint32_t K = win.K, lead = win.lead;  // the window starts `lead` bytes into step 0
    const gbyte_t wb = global_ptr(reinterpret_cast<const uint8_t *>(win.origin), true);  // step grid origin
    const int32_t ilen = (int32_t)len;
    const uint32_t lo_lane = 16u * gl;
    const uint32_t qs = win.qs, kc0 = win.kc0, kc1 = win.kc1;  // steps [kc0, kc1) are clean for every lane
    constexpr uint32_t R = kRingOff;

    uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
    [[maybe_unused]] gwbyte_t db = nullptr;
    if constexpr (COPY) db = (gwbyte_t)uniform64(reinterpret_cast<uint64_t>(dst));
    auto fold = [&](uint32_t kk, uint4 v) {
        // (the raw piece: the masking below XORs the initial register into it)
        if constexpr (COPY) store_piece(db, mck_grid_piece_store(win, kk, gl), v);
        if (kk < kc0 || kk >= kc1) {  // wave-uniform: an edge step
            const int32_t lo = (int32_t)(kk * 1024u + lo_lane) - (int32_t)qs;
            v.x = mck_mask32(v.x, lo, ilen, init);
            v.y = mck_mask32(v.y, lo + 4, ilen, init);
            v.z = mck_mask32(v.z, lo + 8, ilen, init);
            v.w = mck_mask32(v.w, lo + 12, ilen, init);
        }
        x0 = f32s(lds, x0 ^ v.x, lc0, lc1);
        x1 = f32s(lds, x1 ^ v.y, lc0, lc1);
        x2 = f32s(lds, x2 ^ v.z, lc0, lc1);
        x3 = f32s(lds, x3 ^ v.w, lc0, lc1);
    };
    // Loads go through global (address-space 1) pointers -- flat loads would
    // also count against lgkmcnt, so every LDS wait of the fold would wait for
    // the ring's HBM loads too -- and only step 0 tests lanes (the ones before
    // the window start read nothing); the steady loop loads unconditionally.
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
    uint32_t x = combine32<6>(lds, x0, x1, x2, x3, gl);
    x = tail32(lds, win.pad(), x);
    if (!RAW && len < 4) x ^= pk->zinit[len];
    return x;
}

template <bool LIGHT>
constexpr int kBlk32 = LIGHT ? kLightBlock : kBlock;

// ---- whole RPC messages (kFrameRpc) ----
// The header pack's rows through a global pointer (a flat load would also count against the LDS waits).
typedef const __attribute__((address_space(1))) uint16_t *rpc_tab_t;

// A verifying workgroup's per-class counts: LDS atomics by the owning lanes
// (none returns a value or leaves the CU), added to the caller's six words
// once per WORKGROUP at its end, as add_mismatches adds its one.  The batch
// kernels' LDS has room for these 24 bytes, not for a table.  N: the classes
// of the call -- the unpack twin's seven words are its own, so the verify
// twin's LDS is what it was.
template <uint32_t N>
__device__ __forceinline__ uint32_t *rpc_wg_counts() {
    __shared__ uint32_t wg_cls[N];
    return wg_cls;
}
// Every thread of the workgroup calls this, once (counters zeroed ahead of the fill's barrier).
template <uint32_t N>
__device__ __forceinline__ void rpc_add_counts(uint32_t *ctr) {
    __syncthreads();
    if (threadIdx.x < N && ctr) {
        const uint32_t v = rpc_wg_counts<N>()[threadIdx.x];
        if (v) atomicAdd(&ctr[threadIdx.x], v);
    }
}
// fail_closed's sibling for the RPC twins: the caller's error word gets +1, a
// verify adds `count` to the FAULT class, and every status becomes FAULT --
// verify's and seal's, so a stale OK or DEFERRED in the caller's buffer never
// survives; messages hashed after the sweep overwrite theirs with the truth.
// The copying twins' too: an unpack is a verify here (its FAULT word is the
// same one of its seven), a pack a seal.
template <bool VERIFY>
__device__ __forceinline__ void rpc_fail_closed(const BatchArgs &a) {
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0) {
        if (a.err_word) atomicAdd(a.err_word, 1u);
        if (VERIFY && a.mismatches) atomicAdd(&a.mismatches[mck::kRpcFault], (uint32_t)a.count);
    }
    if (a.status)
        for (uint64_t p = lane; p < a.count; p += 64) a.status[p] = (uint8_t)mck::kRpcFault;
}

// OP (launch_plan.h, BatchOp): what the owning lane does with a payload's CRC.
// FRAME (launch_plan.h, MsgFrame): what surrounds a payload and where its hash
// slot is.  kFrameDetached: a verify's or a seal's slots lie in the eager
// messages, a buffer and table of their own.  kFrameRpc: whole RPC messages --
// the core header's CRC-16 and its flags decide with the payload's CRC what a
// message is (launch_plan.h: rpc_verify_class, rpc_seal_class); with a copying
// OP the payload is also stored by the payload loop, and the other range's
// length enters the rules (rpc_copies_payload, rpc_unpack_class,
// rpc_pack_class).  In place is the payloads frame's kernels (BatchArgs::msg).
// LIST (launch_plan.h, KernelKey::list; kFrameRpc only): the message side is an
// address list -- its table entry p is the message's absolute address, used with
// a null buffer pointer, and its end that address + len[p] from a second array
// (BatchArgs::rpc_list_len) where the table form reads entry p + 1.  Nothing
// else differs but what follows from messages that lie anywhere: a message
// whose payload is not hashed runs the empty payload at address 0 -- no load,
// where the table form's may read on in the line of the message's end --, and
// the light layout deals messages by count, there being no table to balance by.
// BOTH (KernelKey::both_lists; kFrameDetached only): both sides are address
// lists -- the payloads' as above, and the slots' table entry p is the eager
// message's address, used with a null `msgs`, its length from a third array
// (BatchArgs::slot_list_len).  The rules of entries that lie anywhere are
// launch_plan.h's (list_msg_len, list_payload_ok, _len, _at).
template <int LOG2G, int MODE, int OP, bool NT, bool LIGHT = false, mck::MsgFrame FRAME = mck::kFramePayloads, bool LIST = false,
          bool BOTH = false>
__global__ __launch_bounds__(kBlk32<LIGHT>, 1) void crc32c_batch_kernel(BatchArgs a) {
    static_assert(mck::kernel_key_valid(mck::KernelKey{32, LOG2G, MODE, OP, NT, LIGHT, false, FRAME, LIST, BOTH}),
                  "no such batch kernel");
    // (enumerators: as constexpr locals, their debug records moved instructions in a -g build of one kernel)
    enum : bool {
        VERIFY = OP == mck::kOpVerify || OP == mck::kOpUnpack,
        SEED = OP == mck::kOpUpdate,
        SEAL = OP == mck::kOpSeal || OP == mck::kOpPack,
        COPY = OP == mck::kOpPack || OP == mck::kOpUnpack,
        RPC = FRAME == mck::kFrameRpc,
        LIST_BATCH = (LIST && !(COPY && SEAL)) || BOTH  // the list is the batch's own side (a pack's is the written side)
    };
    constexpr int kWavesPerBlock = kBlk32<LIGHT> / 64;
    __shared__ __attribute__((aligned(16))) uint8_t lds_raw[LIGHT ? kL32LightBytes : kL32Bytes];
    const crc32_gpu_pack_t *pk = reinterpret_cast<const crc32_gpu_pack_t *>(a.pack);
    MCK_STAMP(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), 0);
    constexpr int PPW = 64 >> LOG2G;
    const uint64_t units = MODE == kOffsets ? a.count : (a.count + PPW - 1) / PPW;
    __shared__ WgQueue wgq;
    constexpr bool DYN = dyn_policy(32, MODE, NT, LIGHT);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gl = lane & ((1u << LOG2G) - 1u), grp = lane >> LOG2G;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    // Aligned batches on the static split (C2): the loads of the wave's first
    // payload go out inside the LDS table fill, so their HBM round trip
    // overlaps the fill's.  The queue path (the headline) keeps its first unit
    // dynamic: a static first unit there measured 1% slower (round 3); the
    // light layout gained nothing from it.
    constexpr bool PRE = MODE == kFixedAligned && !LIGHT && !DYN;
    // model words read once, ahead of any store (scalar loads; read after the
    // barrier they became a vector load per payload whose wait, merged with
    // the ring's at the prefetch branch, cost a vmcnt(0) per payload)
    const uint32_t init = pk->init, xorout = pk->xorout;
    // RPC: the header model's pack (two scalar loads, here for the reason above)
    [[maybe_unused]] rpc_tab_t rpc_tab = nullptr;
    [[maybe_unused]] uint32_t rpc_kind = 0, rpc_c = 0;
    constexpr uint32_t kCounts = COPY ? mck::kRpcCopyClasses : mck::kRpcClasses;  // (RPC && VERIFY: the words of LDS counts)
    if constexpr (RPC) {
        const mck::RpcHdrPack *hp = reinterpret_cast<const mck::RpcHdrPack *>(COPY ? a.rpc_copy_hdr_pack : a.rpc_hdr_pack);
        rpc_tab = (rpc_tab_t)uniform64(reinterpret_cast<uint64_t>(&hp->row[0][0]));
        rpc_kind = hp->kind;
        rpc_c = hp->c;
        if (VERIFY && threadIdx.x < kCounts) rpc_wg_counts<kCounts>()[threadIdx.x] = 0;  // (ahead of the fill's barrier)
    }
    uint4 ring0[kRing];
    const bool pre = PRE && wave < units;
    if (DYN && threadIdx.x == 0) wg_queue_init(&wgq, a.queue, units);
    fill_lds32<LIGHT, kBlk32<LIGHT>>(lds_raw, pk, [&] {
        // Throughput layout: unconditional (a wave without a first unit reads
        // the last payload's first steps) -- loads under a branch leave the
        // waitcnt pass a merge point, where it falls back to vmcnt(0) for the
        // fill's writes.  Light layout (small batches: most of its 8192 waves
        // may have no unit): only waves with a first unit load, and before the
        // fill's loads (fill_lds32 runs `issue` first there), so the fill's
        // waits count the same on both paths.
        if constexpr (PRE) {
            const uint64_t p = (uint64_t)wave * PPW + grp;
            if (!LIGHT || pre) ring32_load<LOG2G, NT>(ring0, a.base + (p < a.count ? p : a.count - 1) * a.stride, gl);
        }
    });
    __syncthreads();
    MCK_STAMP(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), 1);
    const Tab32<LIGHT> lds{lds_raw};

    const uint32_t lc0 = (lane & 31u) << 2, lc1 = lc0 | 0x10000u;
    uint32_t nbad = 0;  // verify: this lane's mismatches (add_mismatches)

    if (MODE == kOffsets) {
        auto one = [&](uint64_t p) {
            // (LIST: entry p is an address and the array has no entry `count`; an end that wraps is an empty message)
            const uint64_t m0 = a.offsets[p], m1 = LIST_BATCH ? m0 + a.rpc_list_len()[p] : a.offsets[p + 1];
            if constexpr (RPC) {
                // A whole RPC message.  Lanes 0..15 load a header byte each and
                // look up its term of the CRC-16 (launch_plan.h, RpcHdrPack:
                // one load, no chain, and in flight under the payload loop).
                // The flags byte, from its lane, and the length decide for the
                // whole wave whether the payload is hashed -- ahead of the first
                // payload load; otherwise the wave hashes an empty payload.
                //
                // The copying twins: the message is [g0, g0 + L) of `mbuf`, and
                // R the length of the other range.  An unpack's message is the
                // batch's own (base, offsets) and its destination copy_dst by
                // dst_offsets; a pack's message is the WRITTEN side (msgs,
                // dst_offsets: the caller filled its header, and no byte the
                // sixteen lanes use is stored by this launch), its payload the
                // batch's.  rpc_copies_payload decides, as above, ahead of the
                // first payload load or store: a message that is not copied
                // runs the empty payload, and R is not looked at with MORE_DATA.
                const uint64_t pay = a.rpc_pay_off();
                uint64_t g0 = m0, g1 = m1;
                const uint8_t *mbuf = a.base;
                if constexpr (COPY && SEAL) {
                    g0 = a.dst_offsets[p], g1 = LIST ? g0 + a.rpc_list_len()[p] : a.dst_offsets[p + 1];
                    mbuf = a.msgs;
                }
                const uint64_t L = mck::rpc_len(g0, g1);
                const bool whole = L >= mck::kRpcHdrBytes;
                uint32_t hb = 0, term = 0;
                if (whole && lane < mck::kRpcHdrBytes) hb = global_ptr(mbuf + g0, true)[lane];
                const bool more = whole && (__builtin_amdgcn_readlane(hb, mck::rpc_flags_at(rpc_kind)) & 1u);
                if (whole && lane < mck::kRpcHdrBytes) term = rpc_tab[mck::rpc_hdr_term_index(rpc_kind, lane, hb)];
                [[maybe_unused]] uint64_t R = 0;
                if constexpr (COPY && SEAL) R = mck::rpc_len(m0, m1);
                else if constexpr (COPY) R = mck::rpc_len(a.dst_offsets[p], a.dst_offsets[p + 1]);
                bool hashed;
                if constexpr (COPY) hashed = mck::rpc_copies_payload(L, more, pay, R);
                else hashed = mck::rpc_hashes_payload(L, more, pay);
                uint32_t x;
                if constexpr (COPY) {
                    // (an unpack reads [m0 + pay, m0 + L), a pack [m0, m0 + R): R bytes either way)
                    // (LIST_BATCH: a message that is not copied may lie anywhere, or nowhere: its empty payload is
                    // address 0's, a grid window of no step)
                    uint64_t o = SEAL ? m0 : m0 + pay;
                    const uint64_t n = hashed ? R : 0;
                    if constexpr (LIST_BATCH) o = hashed ? o : 0;
                    uint8_t *dst = a.copy_dst + (SEAL ? g0 + pay : a.dst_offsets[p]);
                    x = n < (1ull << 31)
                            ? payload32_g64<NT, Tab32<LIGHT>, false, true>(lds, pk, a.base + o, n, gl, lc0, lc1, 0u, dst)
                            : payload32_generic<LOG2G, NT, Tab32<LIGHT>, true>(lds, pk, a.base + o, n, gl, lc0, lc1, dst);
                } else {
                    uint64_t o = hashed ? m0 + pay : m0 + L;
                    const uint64_t n = m0 + L - o;
                    if constexpr (LIST) o = hashed ? o : 0;  // (as above: address 0's empty payload)
                    x = n < (1ull << 31) ? payload32_g64<NT>(lds, pk, a.base + o, n, gl, lc0, lc1)
                                         : payload32_generic<LOG2G, NT>(lds, pk, a.base + o, n, gl, lc0, lc1);
                }
                // the image's terms XOR over the lanes that hold them; the wire hash is two identity terms
                uint32_t t = lane < mck::rpc_img_bytes(rpc_kind) ? term : 0u;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) t ^= __shfl_xor(t, d, 64);
                const uint32_t crc16 = mck::rpc_hdr_crc(rpc_c, __builtin_amdgcn_readfirstlane(t));
                const uint32_t hat = mck::rpc_hash_at(rpc_kind);
                const uint32_t wire = __builtin_amdgcn_readlane(term, hat) << 8 | __builtin_amdgcn_readlane(term, hat + 1);
                if (gl == 0) {
                    if constexpr (SEAL) {
                        // (byte stores: the 2 or 6 bytes share their granules with other fields and messages)
                        // (a pack's payload bytes are in place by now: R + 6 or 2 bytes of a message, no others)
                        uint8_t *msg = a.msgs + g0;
                        uint32_t cls;
                        if constexpr (COPY) cls = mck::rpc_pack_class(L, more, pay, R);
                        else cls = mck::rpc_seal_class(L, more, pay);
                        if (cls == mck::kRpcOk) store_be32(msg + a.hash_off, x ^ xorout);
                        if (COPY ? cls == mck::kRpcOk || cls == mck::kRpcDeferred : cls != mck::kRpcShort) {
                            msg[hat] = (uint8_t)(crc16 >> 8);
                            msg[hat + 1] = (uint8_t)crc16;
                        }
                        if (a.status) a.status[p] = (uint8_t)cls;
                    } else {
                        // (an unpack's bytes are stored as received: both verdicts are known only after the copy)
                        const bool pay_ok = hashed && load_be32(a.base + m0 + a.hash_off) == (x ^ xorout);
                        uint32_t cls;
                        if constexpr (COPY) cls = mck::rpc_unpack_class(L, crc16 == wire, more, pay, R, pay_ok);
                        else cls = mck::rpc_verify_class(L, crc16 == wire, more, pay, pay_ok);
                        if (a.status) a.status[p] = (uint8_t)cls;
                        atomicAdd(&rpc_wg_counts<kCounts>()[cls], 1u);  // LDS; the device's counters once per workgroup
                    }
                }
            } else if constexpr (FRAME == mck::kFrameDetached) {
                // The payload is the whole of [m0, m1); its hash slot is in eager
                // message p of another buffer (msgs, by the table dst_offsets),
                // four bytes at any alignment -- the in-place epilogues below at
                // another address (launch_plan.h: msg_slot_ok, msg_slot_at).  A
                // verify reads msgs only.
                // BOTH: m1 - m0 is the payload's length whether its end wraps or not; a
                // wrapped payload is hashed as an empty one and fails its entry with the
                // slotless messages, and every empty payload runs at address 0.
                const uint64_t h0 = a.dst_offsets[p];
                uint64_t h1, n = m1 - m0, o = m0;
                [[maybe_unused]] bool wrapped = false;
                if constexpr (BOTH) {
                    h1 = h0 + mck::list_msg_len(h0, a.slot_list_len()[p]);
                    wrapped = !mck::list_payload_ok(m0, n);
                    o = mck::list_payload_at(m0, n);
                    n = mck::list_payload_len(m0, n);
                } else {
                    h1 = a.dst_offsets[p + 1];
                }
                const uint32_t x = n < (1ull << 31) ? payload32_g64<NT>(lds, pk, a.base + o, n, gl, lc0, lc1)
                                                    : payload32_generic<LOG2G, NT>(lds, pk, a.base + o, n, gl, lc0, lc1);
                if (gl == 0) {
                    const bool short_msg = !mck::msg_slot_ok(h0, h1, a.hash_off) || (BOTH && wrapped);
                    uint8_t *slot = a.msgs + mck::msg_slot_at(h0, a.hash_off);
                    if constexpr (SEAL) {
                        if (!short_msg) store_be32(slot, x ^ xorout);
                        if (a.status) a.status[p] = short_msg ? 1 : 0;
                    } else {
                        const bool bad = short_msg || load_be32(slot) != (x ^ xorout);
                        if (a.status) a.status[p] = bad ? 1 : 0;
                        nbad += bad;
                    }
                }
            } else if constexpr (COPY) {
                // In place, the payload moved.  The message is the side with the
                // headers -- an unpack's source, a pack's destination --, L bytes,
                // and R the other range's.  A pair that does not fit (a message
                // shorter than its headers never does) is hashed and copied as an
                // empty payload: status 1, no byte written, and an unpack's mismatch.
                const uint64_t d0 = a.dst_offsets[p], d1 = a.dst_offsets[p + 1];
                const uint64_t L = SEAL ? d1 - d0 : m1 - m0, R = SEAL ? m1 - m0 : d1 - d0;
                const bool misfit = L != a.pay_off + R;
                const uint64_t o = misfit ? m1 : SEAL ? m0 : m0 + a.pay_off, n = m1 - o;
                uint8_t *dst = a.copy_dst + d0;  // (a pack's is its message: the payload goes behind the headers)
                const uint32_t x =
                    n < (1ull << 31)
                        ? payload32_g64<NT, Tab32<LIGHT>, false, true>(lds, pk, a.base + o, n, gl, lc0, lc1, 0u, SEAL ? dst + a.pay_off : dst)
                        : payload32_generic<LOG2G, NT, Tab32<LIGHT>, true>(lds, pk, a.base + o, n, gl, lc0, lc1, SEAL ? dst + a.pay_off : dst);
                if (gl == 0) {
                    if constexpr (SEAL) {
                        // (the hash slot's neighbours in its 16-byte granule are
                        // other messages' payload and header bytes: byte stores
                        // here, and whole-piece stores only inside a payload)
                        if (!misfit) store_be32(dst + a.hash_off, x ^ xorout);
                        if (a.status) a.status[p] = misfit ? 1 : 0;
                    } else {
                        // (the bytes are stored as received: the value is known only after the copy)
                        const bool bad = misfit || load_be32(a.base + m0 + a.hash_off) != (x ^ xorout);
                        if (a.status) a.status[p] = bad ? 1 : 0;
                        nbad += bad;
                    }
                }
            } else {
                // bare payloads, or in place (a.msg): a message shorter than its headers fails verification
                const bool short_msg = a.msg && m1 - m0 < a.pay_off;
                const uint64_t o = a.msg ? (short_msg ? m1 : m0 + a.pay_off) : m0;
                const uint64_t n = m1 - o;
                const uint32_t x = n < (1ull << 31) ? payload32_g64<NT>(lds, pk, a.base + o, n, gl, lc0, lc1)
                                                    : payload32_generic<LOG2G, NT>(lds, pk, a.base + o, n, gl, lc0, lc1);
                if constexpr (SEED) {
                    if (gl == 0) {
                        uint32_t *st = reinterpret_cast<uint32_t *>(a.out) + p;
                        *st = mck_seed32(reinterpret_cast<const crc32_shift_pack_t *>(a.shift), x, *st, init, n);
                    }
                } else if constexpr (SEAL) {
                    // The hash slot shares a 16-byte granule with the payload's
                    // first bytes (slot at 16..19, payload from 20), may share one
                    // with the previous message's tail, and lies in the pad bytes
                    // the previous message's last step reads: payload loads of this
                    // or another wave see its old or its new bytes.  Those bytes
                    // are outside every payload, so mck_mask32 clears them before
                    // the fold and no value depends on which.
                    if (gl == 0) {
                        if (!short_msg) store_be32(a.msgs + m0 + a.hash_off, x ^ xorout);
                        if (a.status) a.status[p] = short_msg ? 1 : 0;
                    }
                } else if (gl == 0) {
                    if (VERIFY && a.msg) {
                        const bool bad = short_msg || load_be32(a.base + m0 + a.hash_off) != (x ^ xorout);
                        if (a.status) a.status[p] = bad ? 1 : 0;
                        nbad += bad;
                    } else {
                        emit<uint32_t, VERIFY>(a, p, x ^ xorout, nbad);
                    }
                }
            }
        };
        if constexpr (!LIGHT) {
            // (a sealing launch sweeps its statuses as a verify does, with no counter to add to)
            if (for_each_unit<true>(&wgq, a.queue, units, wave, nw, one)) {
                if constexpr (RPC) rpc_fail_closed<VERIFY>(a);
                else fail_closed<VERIFY || SEAL>(a);
            }
        } else {  // static: a byte-balanced contiguous range per wave
            uint64_t first, last;
            if constexpr (LIST_BATCH) {  // addresses are no table to balance bytes by: a contiguous range by count
                const uint64_t q = a.count / nw, r = a.count % nw;
                first = q * wave + (r * wave) / nw;
                last = q * (wave + 1) + (r * (wave + 1)) / nw;
            } else {
                wave_range(a.offsets, a.count, wave, nw, &first, &last);
            }
            for (uint64_t p = first; p < last; p++) one(p);
        }
        if constexpr (RPC && VERIFY) rpc_add_counts<kCounts>(a.mismatches);
        else if constexpr (VERIFY) add_mismatches(a.mismatches, nbad);
        MCK_STAMP(wave, 2);
        return;
    }
    auto unit = [&](uint64_t u, bool loaded) {
        const uint64_t p = u * PPW + grp;
        const bool act = p < a.count;
        const uint64_t pc = act ? p : a.count - 1;
        uint32_t x;
        if (MODE == kFixedAligned)
            x = payload32_aligned<LOG2G, NT>(lds, a.base + pc * a.stride, a.len >> (4 + LOG2G), gl, lc0, lc1, init, ring0,
                                             loaded);
        else
            x = payload32_generic<LOG2G, NT>(lds, pk, a.base + pc * a.stride, a.len, gl, lc0, lc1);
        if (act && gl == 0) emit<uint32_t, VERIFY>(a, p, x ^ xorout, nbad);
    };
    // The prefetched first unit runs in a copy of the payload loop of its own:
    // one copy behind a loaded/not-loaded branch leaves the prefetch loads
    // pending at the loop head in the waitcnt pass's view, and it then waited
    // vmcnt(0) -- the previous payload's CRC store included -- at every payload.
    if (PRE && pre) unit(wave, true);
    const bool faulted = for_each_unit<DYN, PRE>(&wgq, a.queue, units, wave, nw, [&](uint64_t u) { unit(u, false); });
    if (faulted) fail_closed<VERIFY>(a);
    if constexpr (VERIFY) add_mismatches(a.mismatches, nbad);
    MCK_STAMP(wave, 2);
}

// Z^n(x) from the base-16 digit tables; n and x are wave-uniform on the chunk
// paths (mchecksum_gpu_ext.hip) and the split CRC-64 pieces (crc_gpu_crc64.h), so the table words come through the scalar cache.
// Not so in the seeded offsets kernels and the combine kernel, which run
// mck_zshift32/64 (crc_gpu_seed.h, the same loop bounded by the pack's digit
// count) with a per-lane n: there the table words come through vector loads --
// at most 12 digit steps per payload, on one lane.
__device__ __forceinline__ uint32_t shift32(const crc32_shift_pack_t *sp, uint32_t x, uint64_t n) {
    for (int k = 0; n; k++, n >>= 4) {
        const uint32_t d = (uint32_t)(n & 15u);
        if (d) {
            const uint32_t *t = &sp->op[k][d - 1][0][0];
            uint32_t r = 0;
#pragma unroll
            for (int h = 0; h < 8; h++) r ^= t[h * 16 + ((x >> (4 * h)) & 15u)];
            x = r;
        }
    }
    return x;
}

}  // namespace

#endif  // CRC_GPU_CRC32_H
