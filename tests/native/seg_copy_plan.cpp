/*
 * seg_copy_plan.cpp -- the chunk arithmetic of mchecksum_gpu_gather_segments /
 * mchecksum_gpu_scatter_segments walked on the CPU: the header the kernels
 * include (mercury_amd/csrc/seg_copy_plan.h) cuts every segment of a random
 * list into chunks and gives each chunk its two addresses, and every chunk is
 * copied as seg_copy_kernel's payload loops copy it -- piece by piece through
 * mck_grid_piece_store (crc_gpu_pack_store.h) over GridWindow(load address,
 * chunk length, 4) and (.., 8), the CRC-32C and CRC-64 geometries.
 *
 * Layouts: runs of empty segments, empty objects, segments outside every
 * object (first[0] > 0, first[nobj] < nseg), objects that straddle the scan's
 * blocks of 1024 segments, lengths on and around the chunk size; segments at
 * random byte addresses, objects' contiguous ranges permuted with 0..31-byte
 * gaps.  The chunk size is a template parameter: 256 KiB as the kernels cut,
 * and 48 bytes so that chunk edges are dense.
 *
 * Checked, for gather and for scatter: every destination byte is written
 * exactly once and equals the reference concatenation (or split); no guard
 * byte -- before, after, in a gap, in a segment outside every object, in the
 * side that is read -- is touched; pieces are read only from the 16-byte
 * boundary below a chunk to the 128-byte line end past it.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crc_gpu_pack_store.h"
#include "seg_copy_plan.h"

static unsigned long long n_layouts, n_chunks, n_pieces, n_bytes;
static int failures;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

static void fail(const char *what, long long a, long long b) {
    if (failures++ < 10) printf("FAIL %s (%lld, %lld)\n", what, a, b);
}

/* Memory with a byte-wise write count; reads outside [0, size) are a failure. */
struct Mem {
    std::vector<uint8_t> v, cnt;
    explicit Mem(size_t n) : v(n + 256, 0xC3), cnt(n + 256, 0) {}
    uint8_t *base() { return v.data() + 128; }  /* 128 guard bytes on either side */
    size_t size() const { return v.size() - 256; }
};

/* One chunk: n bytes at `load` (an index into from) go to `store` (into to),
 * as payload32_g64 / payload64_g64 with COPY walk their window. */
static void copy_chunk(Mem &from, Mem &to, uint64_t load, uint64_t store, uint64_t n, uint32_t wbytes) {
    /* the kernels see addresses: give the window the load side's real one */
    const uint64_t la = (uint64_t)(uintptr_t)from.base() + load;
    const GridWindow g(la, n, wbytes);
    const uint64_t lo_ok = la & ~15ull, hi_ok = (la + n + 127) & ~127ull;
    n_chunks++;
    for (uint32_t k = 0; k < g.K; k++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t at = g.origin + (uint64_t)k * 1024 + 16 * lane;
            const bool read = k > 0 || 16 * lane >= g.lead;
            if (read && (at < lo_ok || at + 16 > hi_ok)) fail("piece read out of range", (long long)load, (long long)n);
            const PieceStore s = mck_grid_piece_store(g, k, lane);
            n_pieces++;
            if (s.none()) continue;
            if (!read) {
                fail("a piece that was not read is stored", (long long)load, (long long)n);
                continue;
            }
            for (uint32_t b = s.b0; b < s.b1; b++) {
                const int64_t src_i = (int64_t)(at - (uint64_t)(uintptr_t)from.base()) + b;
                const int64_t dst_i = (int64_t)store + s.lo + b;
                if (src_i < -128 || src_i >= (int64_t)from.size() + 128 || dst_i < -128 || dst_i >= (int64_t)to.size() + 128) {
                    fail("stored byte outside the arrays", src_i, dst_i);
                    continue;
                }
                to.base()[dst_i] = from.base()[src_i];
                to.cnt[128 + dst_i]++;
                n_bytes++;
            }
        }
}

struct Layout {
    std::vector<uint64_t> addr, len, first, starts;  /* addr / starts: byte indices into seg / flat memory */
    uint64_t seg_bytes = 0, flat_bytes = 0;
};

/* pool: lengths to draw from */
static Layout make_layout(uint64_t nseg, uint64_t nobj, const std::vector<uint64_t> &pool, bool subrange) {
    Layout L;
    L.len.resize(nseg);
    for (uint64_t s = 0; s < nseg;) {
        if (below(6) == 0) {  /* a run of empty segments */
            for (uint64_t r = 1 + below(5); r && s < nseg; r--) L.len[s++] = 0;
        } else {
            L.len[s++] = pool[below(pool.size())];
        }
    }
    /* segments at random addresses, in a shuffled order, 0..40 bytes apart */
    std::vector<uint64_t> order(nseg);
    for (uint64_t s = 0; s < nseg; s++) order[s] = s;
    for (uint64_t s = nseg; s > 1; s--) {
        const uint64_t t = below(s);
        const uint64_t x = order[s - 1];
        order[s - 1] = order[t];
        order[t] = x;
    }
    L.addr.resize(nseg);
    uint64_t at = below(16);
    for (uint64_t i = 0; i < nseg; i++) {
        L.addr[order[i]] = at;
        at += L.len[order[i]] + below(41);
    }
    L.seg_bytes = at + 16;
    /* objects: sorted cut points with repeats (empty objects) */
    const uint64_t lo = subrange && nseg > 2 ? 1 + below(nseg / 3) : 0;
    const uint64_t hi = subrange && nseg > 2 ? nseg - 1 - below(nseg / 3) : nseg;
    L.first.resize(nobj + 1);
    for (auto &f : L.first) f = lo + below(hi - lo + 1);
    for (uint64_t i = 1; i < L.first.size(); i++)  /* insertion sort: nobj is small */
        for (uint64_t k = i; k > 0 && L.first[k - 1] > L.first[k]; k--) {
            const uint64_t x = L.first[k];
            L.first[k] = L.first[k - 1];
            L.first[k - 1] = x;
        }
    if (nobj) {
        L.first[0] = lo;
        L.first[nobj] = hi;
    }
    /* contiguous ranges: the objects permuted, 0..31-byte gaps */
    std::vector<uint64_t> P(nseg + 1, 0);
    for (uint64_t s = 0; s < nseg; s++) P[s + 1] = P[s] + L.len[s];
    std::vector<uint64_t> perm(nobj);
    for (uint64_t j = 0; j < nobj; j++) perm[j] = j;
    for (uint64_t j = nobj; j > 1; j--) {
        const uint64_t t = below(j);
        const uint64_t x = perm[j - 1];
        perm[j - 1] = perm[t];
        perm[t] = x;
    }
    L.starts.assign(nobj, 0);
    at = below(32);
    for (uint64_t i = 0; i < nobj; i++) {
        const uint64_t j = perm[i];
        L.starts[j] = at;
        at += P[L.first[j + 1]] - P[L.first[j]] + below(32);
    }
    L.flat_bytes = at + 16;
    return L;
}

template <uint64_t CH>
static void run_layout(const Layout &L, int dir, uint32_t wbytes) {
    const uint64_t nseg = L.len.size(), nobj = L.first.size() - 1;
    Mem seg(L.seg_bytes), flat(L.flat_bytes);
    std::vector<uint64_t> P(nseg + 1, 0);
    for (uint64_t s = 0; s < nseg; s++) P[s + 1] = P[s] + L.len[s];
    /* the side that is read holds data, the other keeps its 0xC3 */
    Mem &from = dir == mck::kSegGather ? seg : flat, &to = dir == mck::kSegGather ? flat : seg;
    for (size_t i = 0; i < from.v.size(); i++) from.v[i] = (uint8_t)(rnd() >> 56);
    const std::vector<uint8_t> from_before = from.v;
    n_layouts++;
    /* the reference: what each destination byte must hold (-1: untouched) */
    std::vector<int> want(to.size(), -1);
    for (uint64_t j = 0; j < nobj; j++) {
        uint64_t pos = 0;
        for (uint64_t s = L.first[j]; s < L.first[j + 1]; s++)
            for (uint64_t i = 0; i < L.len[s]; i++, pos++) {
                const uint64_t si = L.addr[s] + i, fi = L.starts[j] + pos;
                if (dir == mck::kSegGather) want[fi] = seg.base()[si];
                else want[si] = flat.base()[fi];
            }
    }
    /* the walk: every chunk of every segment inside an object, as the chunk passes find them */
    uint64_t j = 0;
    for (uint64_t s = 0; s < nseg; s++) {
        if (!nobj || s < L.first[0] || s >= L.first[nobj]) continue;  /* outside every object */
        while (j + 1 < nobj && L.first[j + 1] <= s) j++;
        const uint64_t nch = mck::seg_chunk_count<CH>(L.len[s]);
        uint64_t covered = 0;
        for (uint64_t c = 0; c < nch; c++) {
            const uint64_t off = c * CH, n = mck::seg_chunk_len<CH>(L.len[s], off);
            if (n == 0 || n > CH) fail("chunk length", (long long)s, (long long)c);
            covered += n;
            const mck::SegCopyAddr ad = mck::seg_copy_addr(dir, L.addr[s] + off, 0, L.starts[j], P[s] + off, P[L.first[j]]);
            copy_chunk(from, to, ad.load, ad.store, n, wbytes);
        }
        if (covered != L.len[s]) fail("chunks do not tile the segment", (long long)s, (long long)covered);
    }
    for (size_t i = 0; i < to.v.size(); i++) {
        const int64_t at = (int64_t)i - 128;
        const int w = at >= 0 && at < (int64_t)to.size() ? want[at] : -1;
        if (w < 0 ? (to.cnt[i] != 0 || to.v[i] != 0xC3) : (to.cnt[i] != 1 || to.v[i] != (uint8_t)w)) {
            fail(w < 0 ? "guard byte touched" : "destination byte wrong or not written once", (long long)at, to.cnt[i]);
            break;
        }
    }
    if (from.v != from_before) fail("the side that is read was written", dir, 0);
    for (size_t i = 0; i < from.cnt.size(); i++)
        if (from.cnt[i]) {
            fail("the side that is read was written", dir, (long long)i);
            break;
        }
}

template <uint64_t CH>
static void run_all(const std::vector<uint64_t> &pool, const uint64_t (*shapes)[2], size_t nshapes) {
    for (size_t k = 0; k < nshapes; k++)
        for (int sub = 0; sub < 2; sub++) {
            const Layout L = make_layout(shapes[k][0], shapes[k][1], pool, sub != 0);
            for (int dir : {(int)mck::kSegGather, (int)mck::kSegScatter})
                for (uint32_t wbytes : {4u, 8u}) run_layout<CH>(L, dir, wbytes);
        }
}

int main() {
    /* the kernels' cut: lengths on and around 256 KiB, few segments */
    const uint64_t k = mck::kSegChunk;
    static_assert(mck::kSegChunk == 262144, "the segment passes cut 256 KiB chunks");
    const std::vector<uint64_t> big = {0, 1, 5, 17, 1000, 4097, k - 1, k, k + 1, 2 * k, 3 * k + 13, 262139};
    const uint64_t big_shapes[][2] = {{1, 1}, {7, 3}, {12, 5}, {20, 0}};
    run_all<mck::kSegChunk>(big, big_shapes, 4);
    /* dense chunk edges: 48-byte chunks, lists past one and two scan blocks of
     * 1024 segments with objects that straddle them */
    const std::vector<uint64_t> small = {0, 1, 3, 4, 7, 8, 15, 16, 17, 40, 47, 48, 49, 95, 96, 97, 150, 1023, 1024, 1025};
    const uint64_t small_shapes[][2] = {{1, 1}, {3, 1}, {40, 7}, {1024, 5}, {1025, 3}, {2300, 9}, {2300, 1}, {64, 64}};
    for (int rep = 0; rep < 3; rep++) run_all<48>(small, small_shapes, 8);
    printf("%llu layouts, %llu chunks, %llu pieces replayed, %llu bytes stored\n", n_layouts, n_chunks, n_pieces, n_bytes);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    if (!n_chunks || !n_bytes) {
        printf("nothing walked\n");
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
