/*
 * test_copy_store64.cpp -- which bytes the CRC-64 copy kernels' payload loops
 * store (payload64_g64 and payload64_generic with COPY, crc_gpu_crc64.h),
 * replayed on the CPU with the rule the kernels compile
 * (mercury_amd/csrc/crc_gpu_pack_store.h) over the window geometry they build
 * for 8-byte words: GridWindow(sa, len, 8) and LaneWindow(sa, len, 8, 6).  The
 * 8-byte-word counterpart of tests/native/test_pack_store.c.
 *
 * For every source residue 0..15 x destination residue 0..15 x length
 * 0..2100, and the lengths 65535, 65536 and 65537, every step of every lane
 * of both loops is walked as the kernels walk them, against a destination
 * surrounded by canaries:
 *   - each byte of [dst, dst + len) is written exactly once, with the source
 *     byte of the same payload position;
 *   - no other byte is written;
 *   - a piece the geometry calls clean -- stored whole, its bounds not looked
 *     at -- lies wholly inside the payload;
 *   - a piece is read only inside [src & ~15, the 128-byte line end past the
 *     payload) -- the memory rule of the offsets layout.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "crc_gpu_pack_store.h"

/* kNear canary bytes on either side are looked at after every case, all of them at the end */
enum { kMaxLen = 65537, kCanary = 256, kNear = 32, kSrcPad = 16 + 1024 + 128 };

static uint8_t *src_mem, *dst_mem, *dst_cnt;
static unsigned long long n_cases, n_pieces, n_whole, n_clean, n_bytes;
static int failures;

static void fail(const char *what, uint32_t sr, uint32_t dr, uint32_t len, long long at) {
    if (failures++ < 10) printf("FAIL %s: src residue %u, dst residue %u, len %u, at %lld\n", what, sr, dr, len, at);
}

/* One piece, as store_piece (crc_gpu_common.h) executes a PieceStore: the 16
 * bytes read at `piece` (nullptr: the lane read nothing), stored at dst + lo + b. */
static void replay(const PieceStore &s, const uint8_t *piece, uint8_t *dst, uint8_t *cnt) {
    n_pieces++;
    if (s.none()) return;
    if (!piece) {
        failures++;
        printf("FAIL: a piece that was not read is stored\n");
        return;
    }
    n_whole += s.whole();
    for (uint32_t b = s.b0; b < s.b1; b++) {
        dst[s.lo + (int64_t)b] = piece[b];
        cnt[s.lo + (int64_t)b]++;
        n_bytes++;
    }
}

static void check(uint32_t sr, uint32_t dr, uint32_t len, const char *loop) {
    const uint8_t *src = src_mem + 1024 + 16 + sr;
    const size_t d0 = kCanary + 16 + dr;
    for (size_t i = 0; i < kNear; i++) {
        if (dst_cnt[d0 - 1 - i] || dst_mem[d0 - 1 - i] != 0xC3) fail(loop, sr, dr, len, -1 - (long long)i);
        if (dst_cnt[d0 + len + i] || dst_mem[d0 + len + i] != 0xC3) fail(loop, sr, dr, len, (long long)len + (long long)i);
    }
    for (size_t i = 0; i < len; i++)
        if (dst_cnt[d0 + i] != 1 || dst_mem[d0 + i] != src[i]) {
            fail(loop, sr, dr, len, (long long)i);
            break;
        }
    memset(dst_mem + d0, 0xC3, len);
    memset(dst_cnt + d0, 0, len);
}

static void one_case(uint32_t sr, uint32_t dr, uint32_t len) {
    const uint8_t *src = src_mem + 1024 + 16 + sr;
    uint8_t *dst = dst_mem + kCanary + 16 + dr, *cnt = dst_cnt + kCanary + 16 + dr;
    const uint64_t sa = (uint64_t)(uintptr_t)src;
    const uint64_t lo_ok = sa & ~15ull, hi_ok = (sa + len + 127) & ~127ull;
    n_cases++;

    /* payload64_g64: lanes before the window start in step 0 read nothing; a
     * step is clean for every lane or an edge step (the fold's wave-uniform test) */
    const GridWindow g(sa, len, 8);
    for (uint32_t k = 0; k < g.K; k++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t at = g.origin + (uint64_t)k * 1024 + 16 * lane;
            const bool read = k > 0 || 16 * lane >= g.lead;
            if (read && (at < lo_ok || at + 16 > hi_ok)) fail("g64 read out of range", sr, dr, len, (long long)(at - sa));
            if (!g.edge(k)) {
                n_clean++;
                const int64_t lo = (int64_t)at - (int64_t)sa;
                if (!read || lo < 0 || lo + 16 > (int64_t)len) fail("g64 clean piece outside the payload", sr, dr, len, lo);
            }
            replay(mck_grid_piece_store(g, k, lane), read ? (const uint8_t *)(uintptr_t)at : nullptr, dst, cnt);
        }
    check(sr, dr, len, "g64");

    /* payload64_generic at 64 lanes: pieces at a negative window offset are not read */
    const LaneWindow w(sa, len, 8, 6);
    for (int64_t k = 0; k < w.K; k++)
        for (int64_t lane = 0; lane < 64; lane++) {
            const int64_t pc = w.piece(k, 16 * lane);
            const bool read = pc >= 0;
            const uint64_t at = w.a0 + (uint64_t)pc;
            if (read && (at < lo_ok || at + 16 > hi_ok)) fail("generic read out of range", sr, dr, len, pc);
            if (read && w.clean(pc)) {
                n_clean++;
                const int64_t lo = (int64_t)at - (int64_t)sa;
                if (lo < 0 || lo + 16 > (int64_t)len) fail("generic clean piece outside the payload", sr, dr, len, lo);
            }
            replay(mck_lane_piece_store(w, k, pc), read ? (const uint8_t *)(uintptr_t)at : nullptr, dst, cnt);
        }
    check(sr, dr, len, "generic");
}

int main() {
    const size_t src_bytes = kMaxLen + 2 * kSrcPad, dst_bytes = kMaxLen + 2 * kCanary + 64;
    uint8_t *src_raw = (uint8_t *)malloc(src_bytes + 1024), *dst_raw = (uint8_t *)malloc(dst_bytes + 16);
    uint8_t *cnt_raw = (uint8_t *)calloc(dst_bytes + 16, 1);
    if (!src_raw || !dst_raw || !cnt_raw) return 2;
    /* residue 0 of both arrays is a 1024- / 16-byte boundary */
    src_mem = (uint8_t *)(((uintptr_t)src_raw + 1023) & ~(uintptr_t)1023);
    const size_t shift = (size_t)((16 - ((uintptr_t)dst_raw & 15)) & 15);
    dst_mem = dst_raw + shift;
    dst_cnt = cnt_raw + shift;
    uint32_t x = 0x85EBCA6Bu;
    for (size_t i = 0; i < src_bytes; i++) {
        x = x * 1664525u + 1013904223u;
        src_mem[i] = (uint8_t)(x >> 24);
    }
    memset(dst_mem, 0xC3, dst_bytes);

    for (uint32_t sr = 0; sr < 16; sr++)
        for (uint32_t dr = 0; dr < 16; dr++) {
            for (uint32_t len = 0; len <= 2100; len++) one_case(sr, dr, len);
            for (uint32_t len = 65535; len <= 65537; len++) one_case(sr, dr, len);
        }
    for (size_t i = 0; i < dst_bytes; i++)
        if (dst_cnt[i] || dst_mem[i] != 0xC3) fail("stray write", 0, 0, 0, (long long)i);
    printf("%llu cases, %llu pieces replayed, %llu stored whole, %llu called clean, %llu bytes stored\n", n_cases, n_pieces,
           n_whole, n_clean, n_bytes);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    if (!n_clean) {
        printf("no clean piece seen\n");
        return 1;
    }
    printf("all checks passed\n");
    free(src_raw);
    free(dst_raw);
    free(cnt_raw);
    return 0;
}
