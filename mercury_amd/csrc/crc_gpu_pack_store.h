// crc_gpu_pack_store.h -- which bytes of a 16-byte piece the copying payload
// loops store, and where: the COPY twins of the CRC-32C offsets kernels
// (mchecksum_gpu_pack_messages, mchecksum_gpu_unpack_messages) and the copy
// kernels of both widths (crc_gpu_copy.h: mchecksum_gpu_copy_offsets,
// mchecksum_gpu_update_copy_offsets).  The word size -- 4 bytes for CRC-32C, 8
// for CRC-64 -- enters only through the window geometry the caller built
// (GridWindow(sa, len, 4 or 8), LaneWindow(sa, len, 4 or 8, log2g)): it decides
// which pieces the loop calls clean, never which bytes are stored.  Shared by
// the HIP kernels and two CPU tests (tests/native/test_pack_store.c for 4-byte
// words, tests/native/test_copy_store64.cpp for 8-byte words), like the edge
// handling (crc_gpu_mask.h) and the window geometry (crc_gpu_window.h) it sits
// on.  Plain C++ compiles it.
//
// A payload loop reads whole 16-byte pieces of the window around the payload;
// the lane that folds a piece also stores it.  For a piece whose first byte is
// payload byte `lo` (negative before the payload, >= len past it), payload
// byte lo + b goes to dst[lo + b] for every b with 0 <= lo + b < len -- the
// bounds mck_mask32 / mck_mask64 clear bytes by -- and nothing else is stored: each payload
// byte lies in exactly one piece, so it is written exactly once, and no byte
// outside [dst, dst + len) is written.  A piece the loop calls clean lies
// wholly inside the payload and is stored whole; source and destination
// residues differ in general, so that store is unaligned.
#ifndef CRC_GPU_PACK_STORE_H
#define CRC_GPU_PACK_STORE_H

#include <cstdint>

#include "crc_gpu_shape.h"
#include "crc_gpu_window.h"

namespace {

// Bytes [b0, b1) of the piece go to dst[lo + b0, lo + b1); b0 >= b1: none.
struct PieceStore {
    int64_t lo;
    uint32_t b0, b1;
    MCK_HOST_DEVICE_INLINE bool whole() const { return b0 == 0 && b1 == 16; }
    MCK_HOST_DEVICE_INLINE bool none() const { return b0 >= b1; }
};

// clean: the loop's own test (wave-uniform in the G = 64 loop) said the piece
// needs no edge handling, so its bounds are not looked at.
MCK_HOST_DEVICE_INLINE PieceStore mck_piece_store(int64_t lo, int64_t len, bool clean) {
    PieceStore s{lo, 0u, 16u};
    if (clean) return s;
    if (lo >= len || lo <= -16) {
        s.b1 = 0;
        return s;
    }
    s.b0 = lo < 0 ? (uint32_t)(-lo) : 0u;
    s.b1 = len - lo < 16 ? (uint32_t)(len - lo) : 16u;
    return s;
}

// Lane `lane`'s piece of step k of the one-payload-per-wave loop
// (payload32_g64): at k * 1024 + 16 * lane from the grid origin, the payload
// at [qs, qe).  Lanes before the window start in step 0 read nothing and
// store nothing (their piece ends at or before qs).
MCK_HOST_DEVICE_INLINE PieceStore mck_grid_piece_store(const GridWindow &w, uint32_t k, uint32_t lane) {
    const int64_t lo = (int64_t)k * 1024 + 16 * (int64_t)lane - (int64_t)w.qs;
    return mck_piece_store(lo, (int64_t)w.qe - (int64_t)w.qs, !w.edge(k));
}

// The piece at window offset pc = w.piece(k, lane_off) of the generic loop
// (payload32_generic: payloads of 2 GiB and more): the payload at [hs, he).
// Pieces of steps >= K or at a negative window offset are not read.
MCK_HOST_DEVICE_INLINE PieceStore mck_lane_piece_store(const LaneWindow &w, int64_t k, int64_t pc) {
    if (k >= w.K || pc < 0) return PieceStore{0, 0u, 0u};
    return mck_piece_store(pc - w.hs, w.he - w.hs, w.clean(pc));
}

}  // namespace

#endif  // CRC_GPU_PACK_STORE_H
