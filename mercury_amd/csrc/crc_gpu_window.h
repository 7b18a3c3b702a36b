// crc_gpu_window.h -- where a payload's 16-byte pieces lie: the two window
// geometries of the payload loops, built from (address, length, word bytes).
// Shared by the HIP kernels and the CPU emulator
// (tests/native/kernel_emulator.cpp), like the edge handling they feed
// (crc_gpu_mask.h), so the emulator checks the geometry the GPU runs.  Plain
// C++ compiles it.
#ifndef CRC_GPU_WINDOW_H
#define CRC_GPU_WINDOW_H

#include <cstdint>

#include "crc_gpu_mask.h"
#include "crc_gpu_shape.h"

namespace {

// Per-lane window of the generic loops (payload32_generic / payload64_generic):
// any alignment, any length (0 included), 2^log2g lanes per payload.  The
// window [a0, a1) is the payload widened to 16-B boundaries; its K steps of
// 16 * 2^log2g bytes END at a1, so step 0 starts r0 <= 0 bytes into the window
// and pieces at a negative offset are not read.  The payload is [hs, he) in
// window offsets; the pad bytes [he, a1 - a0) are undone by the tail operator.
struct LaneWindow {
    uint64_t a0;              // window start (16-B aligned address)
    int64_t step, K, r0, hs, he;
    uint64_t ea, a1;          // payload end, window end
    int wbytes;
    MCK_HOST_DEVICE_INLINE LaneWindow(uint64_t sa, uint64_t len, int wbytes_, int log2g) : wbytes(wbytes_) {
        ea = sa + len;
        a0 = sa & ~15ull;
        a1 = (ea + 15) & ~15ull;
        step = (int64_t)16 << log2g;
        const int64_t W = (int64_t)(a1 - a0);
        K = (W + step - 1) >> (4 + log2g);
        r0 = W - K * step;
        hs = (int64_t)(sa - a0);
        he = (int64_t)(ea - a0);
    }
    // pad bytes behind the payload: 0..15
    MCK_HOST_DEVICE_INLINE uint32_t pad() const { return (uint32_t)(a1 - ea); }
    // window offset of a lane's piece of step k (lane_off = 16 * lane in group)
    MCK_HOST_DEVICE_INLINE int64_t piece(int64_t k, int64_t lane_off) const { return r0 + k * step + lane_off; }
    // the piece at window offset pc needs no edge handling
    MCK_HOST_DEVICE_INLINE bool clean(int64_t pc) const { return mck_piece_clean(pc, hs, he, wbytes) != 0; }
};

// Step grid of the one-payload-per-wave loops (payload32_g64 / payload64_g64):
// the window of 1 KiB steps ENDS on a 128-B line boundary past the payload
// (16 B before round 3), so every step reads exactly 8 whole
// lines.  With non-temporal loads a line that two steps straddle is fetched
// twice: on C4's byte-packed payloads that was 1.7% of extra HBM requests
// (TCC_EA0_RDREQ: 6.83e7 vs 6.74e7 with NT off, profiles/r03/tcc_c4_nt*.txt;
// NT off costs 11%).  Reads stay inside the last byte's 128-B line, hence
// its page.  The up-to-127 pad bytes are removed by Z^-t, t = 16q + r: the
// tail table Z^-r and the butterfly operators Z^-(16*2^k) for the bits of q.
constexpr uint64_t kGridAlign = 128;

// Offsets are relative to the grid origin (step 0, lane 0); lane l's piece of
// step k is at k * 1024 + 16 * l.  The window starts `lead` bytes into step 0
// (lanes with 16 * l < lead read nothing there) and the payload is [qs, qe).
// Steps [kc0, kc1) are clean for every lane -- wholly inside the payload and
// past the wbytes init bytes --, so only the others need masking: a
// wave-uniform test.  Payloads < 2 GiB.
struct GridWindow {
    uint64_t origin;  // address of the grid origin (16-B aligned)
    uint64_t ea, a1;  // payload end, grid end
    uint32_t K, lead, qs, qe, kc0, kc1;
    MCK_HOST_DEVICE_INLINE GridWindow(uint64_t sa, uint64_t len, uint32_t wbytes) {
        ea = sa + len;
        const uint64_t a0 = sa & ~15ull;
        a1 = (ea + kGridAlign - 1) & ~(kGridAlign - 1);
        const uint32_t W = (uint32_t)(a1 - a0);
        K = (W + 1023u) >> 10;
        lead = K * 1024u - W;
        origin = a0 - lead;
        qs = lead + (uint32_t)(sa - a0);
        qe = lead + (uint32_t)(ea - a0);
        kc0 = (qs + wbytes + 1023u) >> 10;
        kc1 = qe >= 1024u ? (qe - 1024u) / 1024u + 1u : 0u;
    }
    // pad bytes behind the payload: 0..127
    MCK_HOST_DEVICE_INLINE uint32_t pad() const { return (uint32_t)(a1 - ea); }
    // step k touches an edge of the payload in some lane
    MCK_HOST_DEVICE_INLINE bool edge(uint32_t k) const { return k < kc0 || k >= kc1; }
};

}  // namespace

#endif  // CRC_GPU_WINDOW_H
