// Host check of the work queue's chunk plans (crc_gpu_plan.h).  ChunkPlan:
// for many unit counts and grids the chunks tile the units exactly once, no
// chunk is larger than 2^cl and tail chunks are 2^sl.  SplitPlan (split
// CRC-64): the same, the units tile every payload's bytes exactly once
// (pieces of len / 2^psl), and whenever whole() is true every
// chunk holds whole payloads -- at most kSplitAcc, distinct mod kSplitAcc --
// which the in-workgroup combine needs.  Also prints "plan n grid cl sl nbig
// big_end nch" for a fixed list of shapes, which tests/test_queue_model.py
// compares with its Python model's plan.  Plain C++: no HIP header.
#include "crc_gpu_plan.h"

#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c, ...)                       \
    do {                                    \
        if (!(c)) {                         \
            if (fails++ < 10) {             \
                printf("FAIL: " __VA_ARGS__); \
                printf("\n");               \
            }                               \
        }                                   \
    } while (0)

// Chunks 0 .. nch - 1 of P tile [0, n): each starts where the last one ended,
// full chunks have 2^cl units, tail chunks 2^sl (the last may run past n).
template <class Plan>
static void check_tiling(const Plan &P, uint64_t n, uint32_t grid) {
    CHECK(P.sl <= P.cl && P.cl <= kWgChunkMaxLog2, "chunk sizes: cl %u sl %u", P.cl, P.sl);
    CHECK(P.big_end == P.nbig << P.cl && P.big_end <= n, "full chunks end at %llu of %llu units",
          (unsigned long long)P.big_end, (unsigned long long)n);
    uint64_t next = 0;
    for (uint64_t id = 0; id < P.nch; id++) {
        const uint64_t st = P.start(id), sz = P.size(id);
        CHECK(st == next, "chunk %llu starts at %llu, expected %llu", (unsigned long long)id, (unsigned long long)st,
              (unsigned long long)next);
        CHECK(st < n, "chunk %llu starts past the units", (unsigned long long)id);
        CHECK(sz <= (1u << P.cl), "chunk larger than its slots");
        CHECK(sz == (id < P.nbig ? 1u << P.cl : 1u << P.sl), "chunk %llu has %llu units", (unsigned long long)id,
              (unsigned long long)sz);
        next = st + sz < n ? st + sz : n;
    }
    CHECK(next == n, "chunks end at %llu of %llu units (grid %u)", (unsigned long long)next, (unsigned long long)n, grid);
}

// (n, grid) of every launch tests/test_queue_model.py runs through its model
static const uint64_t kModelShapes[][2] = {
    {1, 1}, {2, 3}, {17, 1}, {67, 2}, {67, 5}, {100, 3}, {257, 8}, {1000, 9}, {4096, 1}, {4096, 16}, {20000, 8},
    {5000, 4}, {4096, 8}, {700, 4}, {500, 3}, {2000, 4}, {5000, 8}, {300, 2}, {900, 4}, {900, 6}, {700, 5},
    {1300, 9}, {40, 3}, {3000, 3}, {256, 2}, {800, 3}, {2048, 4}, {600, 4}, {512, 1}, {160, 1},
    {262144, 256}, {8192, 512}, {100, 256}};

static void print_plan(uint64_t n, uint32_t grid) {
    const ChunkPlan P(n, grid);
    printf("plan %llu %u %u %u %llu %llu %llu\n", (unsigned long long)n, grid, P.cl, P.sl, (unsigned long long)P.nbig,
           (unsigned long long)P.big_end, (unsigned long long)P.nch);
}

int main() {
    const uint32_t grids[] = {1, 3, 8, 64, 255, 256, 512};
    const uint64_t unit_counts[] = {0, 1, 2, 5, 63, 100, 1000, 8192, 262144};
    int plain = 0;
    for (uint32_t grid : grids)
        for (uint64_t n : unit_counts) {
            check_tiling(ChunkPlan(n, grid), n, grid);
            print_plan(n, grid);
            plain++;
        }
    for (const auto &s : kModelShapes) {
        check_tiling(ChunkPlan(s[0], (uint32_t)s[1]), s[0], (uint32_t)s[1]);
        print_plan(s[0], (uint32_t)s[1]);
        plain++;
    }
    // the chunk sizes of C4, a C3-sized fixed batch at 512 workgroups, a small batch
    CHECK(1u << ChunkPlan(262144, 256).cl == 32 && 1u << ChunkPlan(8192, 512).cl == 4 && 1u << ChunkPlan(100, 256).cl == 1,
          "chunk size rule");
    const uint64_t counts[] = {1, 2, 5, 63, 100, 1000, 2048, 8192, 20000};
    const uint32_t psls[] = {1, 2, 3, 4, 6};
    int shapes = 0, whole = 0;
    for (uint32_t grid : grids)
        for (uint64_t count : counts)
            for (uint32_t psl : psls) {
                const SplitPlan P(count, psl, grid);
                shapes++;
                // chunks tile [0, n)
                CHECK(P.n == count << psl, "split plan over %llu units", (unsigned long long)P.n);
                check_tiling(P, P.n, grid);
                // units tile every payload in pieces of len / 2^psl
                const uint32_t gran = 1u << P.psl;
                std::vector<uint8_t> cover(count * gran, 0);
                for (uint64_t u = 0; u < P.n; u++) {
                    uint64_t p;
                    uint32_t q;
                    P.unit(u, &p, &q);
                    CHECK(p < count && q < gran, "unit %llu out of range", (unsigned long long)u);
                    if (p >= count) continue;
                    cover[p * gran + q]++;
                }
                for (uint64_t i = 0; i < cover.size(); i++)
                    CHECK(cover[i] == 1, "granule %llu covered %d times (grid %u count %llu psl %u)",
                          (unsigned long long)i, cover[i], grid, (unsigned long long)count, psl);
                if (!P.whole()) continue;
                whole++;
                for (uint64_t id = 0; id < P.nch; id++) {
                    const uint64_t st = P.start(id), en = st + P.size(id) < P.n ? st + P.size(id) : P.n;
                    std::vector<uint64_t> pays;
                    std::vector<uint32_t> seen;
                    for (uint64_t u = st; u < en; u++) {
                        uint64_t p;
                        uint32_t q;
                        P.unit(u, &p, &q);
                        if (pays.empty() || pays.back() != p) {
                            pays.push_back(p);
                            seen.push_back(0);
                        }
                        seen.back()++;
                        CHECK(q + 1 == seen.back(), "pieces of a payload out of order in a chunk");
                    }
                    CHECK(pays.size() <= kSplitAcc, "chunk with %zu payloads", pays.size());
                    for (size_t k = 0; k < pays.size(); k++) {
                        CHECK(seen[k] == gran, "payload %llu split over chunks (%u of %u pieces)",
                              (unsigned long long)pays[k], seen[k], gran);
                        for (size_t j = 0; j < k; j++)
                            CHECK((pays[j] & (kSplitAcc - 1)) != (pays[k] & (kSplitAcc - 1)),
                                  "two payloads of a chunk share an accumulator");
                    }
                }
            }
    // C3's shape: 4 pieces per payload, whole-payload chunks
    const SplitPlan c3(8192, 2, 256);
    CHECK(c3.whole() && c3.n == 8192 * 4 && c3.cl == 5 && c3.sl == 2, "C3 plan: n %llu cl %u sl %u",
          (unsigned long long)c3.n, c3.cl, c3.sl);
    printf("chunk plan: %d shapes; split plan: %d shapes (%d whole-chunk), %d failures\n", plain, shapes, whole, fails);
    return fails ? 1 : 0;
}
