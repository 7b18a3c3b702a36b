/*
 * seg_plan.cpp -- the arithmetic of the segment passes (checksum_segments,
 * gather_segments, scatter_segments) walked on the CPU: the header the kernels
 * include (mercury_amd/csrc/seg_plan.h) cuts every segment of a random
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
 *
 * Then the rest of the header.  The workspace layout (seg_work_layout): its
 * regions in order, disjoint and inside the total, the total equal to the
 * closed form the ABI has always returned, fault_claim and gen -- which live
 * across calls -- where they have always been.  And the chunk record
 * (SegChunk) through this file's copies of the kernels' loaders, which do each
 * load the kernels do, bounds-checked:
 *  - on a trusted scan's tables, the in-order walk (cut into 1, 7 and 64 wave
 *    ranges) and the random-access locate (shuffled; map and search; head
 *    segment known and not; placed or only shifted) give for every chunk the
 *    record of a brute-force reference, skip none, and tile every object once
 *    with one head;
 *  - on tables that cannot be trusted -- another valid list's, which is what a
 *    scan that gave up leaves, and random words -- every record that is not
 *    skipped lies inside the caller's own segment, shifts by a count that did
 *    not wrap and is below 2^48, sits at no negative offset in its object and
 *    names an object of the call, and no load leaves its table.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "crc_gpu_pack_store.h"
#include "seg_plan.h"

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
            const mck::SegCopyAddr ad = mck::seg_copy_addr(dir, L.addr[s] + off, 0, L.starts[j], P[s] + off - P[L.first[j]]);
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

/* ------------------------------------------------- the workspace layout ---- */

static void check_layout() {
    const uint64_t ns[] = {0, 1, 2, 1023, 1024, 1025, 4096, (1ull << 20) + 3, (1ull << 32) - 1, 1ull << 32, 1ull << 40};
    for (uint64_t nseg : ns) {
        const mck::SegWorkLayout w = mck::seg_work_layout(nseg);
        const uint64_t blocks = nseg ? (nseg + 1023) / 1024 : 1;
        const uint64_t map_cap = nseg < (1ull << 32) ? 4 * nseg + 65536 : 0;
        /* regions in order with their sizes in words; the map follows in bytes */
        const uint64_t at[] = {w.P, w.C, w.ragged, w.fault_claim, w.gen, w.spare, w.desc, w.obj, w.map};
        const uint64_t words[] = {nseg + 1, nseg + 1, 1, 1, 1, 1, mck::kDescWords * blocks, 4 * nseg};
        if (w.P != 0) fail("layout: P is not first", (long long)nseg, (long long)w.P);
        for (int r = 0; r < 8; r++)  /* in order, disjoint, nothing between them (so 8-byte aligned) */
            if (at[r] + words[r] != at[r + 1]) fail("layout: region does not end where the next begins", (long long)nseg, r);
        if (w.desc + mck::kDescWords * mck::seg_scan_blocks(nseg) != w.obj || mck::seg_scan_blocks(nseg) != blocks)
            fail("layout: descriptors", (long long)nseg, (long long)blocks);
        if (w.map_cap != map_cap) fail("layout: map_cap", (long long)nseg, (long long)w.map_cap);
        if (8 * w.map + 4 * w.map_cap != w.bytes || w.bytes % 4) fail("layout: the map does not end at the total", (long long)nseg, 0);
        if (w.bytes != 8 * (2 * (nseg + 1) + 4 + 8 * blocks + 4 * nseg) + 4 * map_cap)
            fail("layout: total differs from the closed form", (long long)nseg, (long long)w.bytes);
        if (w.fault_claim != 2 * (nseg + 1) + 1 || w.gen != 2 * (nseg + 1) + 2)
            fail("layout: fault_claim / gen moved", (long long)nseg, (long long)w.gen);
        if (mck::seg_work_bytes(nseg) != w.bytes) fail("layout: work size", (long long)nseg, 0);
        /* the pointers the kernels get are these offsets */
        alignas(8) static const unsigned char base[8] = {};
        const mck::SegWork p = mck::seg_work(base, nseg > 4096 ? 0 : nseg);  /* (pointer arithmetic: small lists only) */
        const mck::SegWorkLayout q = mck::seg_work_layout(nseg > 4096 ? 0 : nseg);
        const uint64_t *b = reinterpret_cast<const uint64_t *>(base);
        if (p.P != b + q.P || p.C != b + q.C || p.ragged != b + q.ragged || p.fault_claim != b + q.fault_claim ||
            p.gen != b + q.gen || p.desc != b + q.desc || p.obj != b + q.obj ||
            p.map != reinterpret_cast<const uint32_t *>(b + q.map) || p.map_cap != q.map_cap)
            fail("layout: seg_work pointers", (long long)nseg, 0);
    }
    if (mck::seg_work_bytes((1ull << 40) + 1) != SIZE_MAX) fail("layout: past 2^40 segments", 0, 0);
}

/* ---------------------------------------------------- the chunk record ---- */

/* What the scan leaves in the workspace for a list, as seg_scan defines it:
 * the prefix sums, per segment its object record {object, first[j], first[j +
 * 1], head segment -- known only when the object starts in the segment's scan
 * block and has a non-empty segment there}, and the chunk -> segment map. */
struct Tables {
    std::vector<uint64_t> P, C, obj;
    std::vector<uint32_t> map;
};

template <uint64_t CH>
static Tables scan_tables(const Layout &L) {
    const uint64_t nseg = L.len.size(), nobj = L.first.size() - 1;
    Tables t;
    t.P.assign(nseg + 1, 0);
    t.C.assign(nseg + 1, 0);
    for (uint64_t s = 0; s < nseg; s++) {
        t.P[s + 1] = t.P[s] + L.len[s];
        t.C[s + 1] = t.C[s] + mck::seg_chunk_count<CH>(L.len[s]);
    }
    t.obj.assign(4 * nseg, mck::kNoObj);
    for (uint64_t j = 0; j < nobj; j++)
        for (uint64_t s = L.first[j]; s < L.first[j + 1]; s++) {
            const uint64_t s0 = s / mck::kScanBlk * mck::kScanBlk, s1 = s0 + mck::kScanBlk;
            uint64_t hs = mck::kNoObj;
            if (L.first[j] >= s0)
                for (uint64_t i = L.first[j]; i < L.first[j + 1] && i < s1 && hs == mck::kNoObj; i++)
                    if (L.len[i]) hs = i;
            t.obj[4 * s] = j;
            t.obj[4 * s + 1] = L.first[j];
            t.obj[4 * s + 2] = L.first[j + 1];
            t.obj[4 * s + 3] = hs;
        }
    t.map.assign(mck::seg_work_layout(nseg).map_cap, 0);
    if (t.C[nseg] <= t.map.size())
        for (uint64_t s = 0; s < nseg; s++)
            for (uint64_t c = t.C[s]; c < t.C[s + 1]; c++) t.map[c] = (uint32_t)s;
    return t;
}

/* What a chunk pass sees: the caller's own list (trusted) and a workspace. */
struct Pass {
    const Layout *L;
    const Tables *t;
    uint64_t nseg, nobj, map_cap;
};

/* a load, as the kernels' loads: inside its table or a failure */
template <class T>
static T ld(const std::vector<T> &v, uint64_t i) {
    if (i >= v.size()) {
        fail("load outside its table", (long long)i, (long long)v.size());
        return 0;
    }
    return v[i];
}
static uint64_t lower_bound_u64(const std::vector<uint64_t> &a, uint64_t n, uint64_t key) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (ld(a, mid) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* The kernels' loaders (mchecksum_gpu_ext.hip: seg_chunk_of, ChunkWalk,
 * seg_locate), load for load, around the header's rules. */
template <uint64_t CH>
static bool chunk_of(const Pass &a, uint64_t s, uint64_t c, uint64_t *off, mck::SegChunk *k) {
    const bool ok = mck::seg_segment_ok(s, a.nseg);
    const uint64_t cs = ok ? ld(a.t->C, s) : ~0ull, len = ok ? ld(a.L->len, s) : 0;
    k->in = false;
    if (!mck::seg_chunk_bytes<CH>(c, cs, len, off, &k->n)) return false;
    k->addr = ld(a.L->addr, s) + *off;
    return true;
}

template <uint64_t CH>
struct Walk {
    const Pass *a;
    uint64_t c, c1, s, j;
    Walk(const Pass &p, uint32_t wave, uint32_t nw, uint64_t nchunks) : a(&p) {
        c = nchunks * wave / nw;
        c1 = nchunks * (wave + 1) / nw;
        s = c < c1 ? lower_bound_u64(a->t->C, a->nseg + 1, c + 1) - 1 : 0;
        j = c < c1 && s >= ld(a->L->first, 0) ? lower_bound_u64(a->L->first, a->nobj + 1, s + 1) - 1 : 0;
    }
    bool next(mck::SegChunk *k, uint64_t *seg) {
        if (c >= c1) return false;
        while (s < a->nseg && ld(a->t->C, s + 1) <= c) s++;
        uint64_t off;
        if (chunk_of<CH>(*a, s, c, &off, k) && s >= ld(a->L->first, 0) && s < ld(a->L->first, a->nobj)) {
            while (j + 1 < a->nobj && ld(a->L->first, j + 1) <= s) j++;
            k->obj = j;
            k->at = ld(a->t->P, s) + off;
            k->obj_at = ld(a->t->P, ld(a->L->first, j));
            k->end = ld(a->t->P, ld(a->L->first, j + 1));
            k->head = mck::seg_chunk_head(mck::kNoObj, s, off, k->at, k->obj_at);
            k->in = mck::seg_chunk_place(k);
        }
        *seg = s;
        c++;
        return true;
    }
};

/* no_head: the record's head segment read as kNoObj (the scan block could not tell) */
template <uint64_t CH, bool PLACE>
static void locate(const Pass &a, uint64_t c, uint64_t nchunks, bool no_head, mck::SegChunk *k, uint64_t *seg) {
    const uint64_t s = nchunks <= a.map_cap ? (uint64_t)ld(a.t->map, c) : lower_bound_u64(a.t->C, a.nseg + 1, c + 1) - 1;
    *seg = s;
    uint64_t off;
    if (!chunk_of<CH>(a, s, c, &off, k)) return;
    const uint64_t j = ld(a.t->obj, 4 * s), fs = ld(a.t->obj, 4 * s + 1), ls = ld(a.t->obj, 4 * s + 2);
    const uint64_t hs = no_head ? mck::kNoObj : ld(a.t->obj, 4 * s + 3);
    if (!mck::seg_record_ok(j, a.nobj, fs, ls, a.nseg)) return;
    k->obj = j;
    k->at = ld(a.t->P, s) + off;
    k->end = ld(a.t->P, ls);
    k->obj_at = PLACE || !mck::seg_head_known(hs) ? ld(a.t->P, fs) : 0;
    k->head = mck::seg_chunk_head(hs, s, off, k->at, k->obj_at);
    k->in = PLACE ? mck::seg_chunk_place(k) : mck::seg_chunk_after(k);  /* (seg_kernel<64>: after its payload loop) */
}

/* The brute-force reference: chunk c of the list, from the lengths alone. */
struct Ref {
    uint64_t s = 0, addr = 0, n = 0, obj = 0, obj_off = 0, after = 0;
    bool in = false, head = false;
};
template <uint64_t CH>
static std::vector<Ref> reference(const Layout &L) {
    const uint64_t nseg = L.len.size(), nobj = L.first.size() - 1;
    std::vector<uint64_t> owner(nseg, mck::kNoObj), pos(nseg, 0), size(nobj, 0);
    for (uint64_t j = 0; j < nobj; j++)
        for (uint64_t s = L.first[j]; s < L.first[j + 1]; s++) {
            owner[s] = j;
            pos[s] = size[j];
            size[j] += L.len[s];
        }
    std::vector<Ref> ref;
    for (uint64_t s = 0; s < nseg; s++)
        for (uint64_t off = 0; off < L.len[s]; off += CH) {
            Ref r;
            r.s = s;
            r.addr = L.addr[s] + off;
            r.n = L.len[s] - off < CH ? L.len[s] - off : CH;
            r.in = owner[s] != mck::kNoObj;
            if (r.in) {
                r.obj = owner[s];
                r.obj_off = pos[s] + off;
                r.after = size[r.obj] - r.obj_off - r.n;
                r.head = r.obj_off == 0;
            }
            ref.push_back(r);
        }
    return ref;
}

static unsigned long long n_trusted, n_yielded[2], n_skipped[2];  /* [0]: stale tables, [1]: random words */

/* One pass over a trusted scan: every chunk's record equals the reference's,
 * none is skipped, and the chunks of each object tile it once with one head. */
struct Tiling {
    std::vector<std::vector<uint8_t>> cover;
    std::vector<uint32_t> heads;
    explicit Tiling(const Layout &L) : heads(L.first.size() - 1, 0) {
        for (uint64_t j = 0; j + 1 < L.first.size(); j++) {
            uint64_t n = 0;
            for (uint64_t s = L.first[j]; s < L.first[j + 1]; s++) n += L.len[s];
            cover.emplace_back(n, 0);
        }
    }
    void done(const char *what) {
        for (size_t j = 0; j < cover.size(); j++) {
            for (uint8_t b : cover[j])
                if (b != 1) {
                    fail(what, (long long)j, b);
                    break;
                }
            if (heads[j] != (cover[j].empty() ? 0u : 1u)) fail("heads of an object", (long long)j, heads[j]);
        }
    }
};
static void check_trusted(const mck::SegChunk &k, uint64_t seg, const Ref &r, bool place, Tiling *t, uint64_t c) {
    n_trusted++;
    if (seg != r.s) fail("trusted: segment of the chunk", (long long)c, (long long)seg);
    if (k.in != r.in) {  /* zero skips */
        fail("trusted: a chunk inside an object skipped, or one outside hashed", (long long)c, k.in);
        return;
    }
    if (!k.in) return;
    if (k.addr != r.addr || k.n != r.n || k.obj != r.obj || k.after != r.after || k.head != r.head ||
        (place && k.obj_off != r.obj_off))
        fail("trusted: record differs from the reference", (long long)c, (long long)k.obj);
    for (uint64_t b = 0; b < r.n; b++) t->cover[r.obj][r.obj_off + b]++;
    t->heads[r.obj] += k.head;
}

template <uint64_t CH>
static void run_trusted(const Layout &L) {
    const uint64_t nseg = L.len.size(), nobj = L.first.size() - 1;
    if (!nobj) return;  /* (no launch) */
    const Tables t = scan_tables<CH>(L);
    const std::vector<Ref> ref = reference<CH>(L);
    const uint64_t nchunks = t.C[nseg];
    if (nchunks != ref.size()) fail("trusted: chunk count", (long long)nchunks, (long long)ref.size());
    const Pass a{&L, &t, nseg, nobj, t.map.size()};
    for (uint32_t nw : {1u, 7u, 64u}) {  /* the in-order walk, cut into wave ranges */
        Tiling tile(L);
        uint64_t seen = 0;
        for (uint32_t wave = 0; wave < nw; wave++) {
            Walk<CH> w(a, wave, nw, nchunks);
            mck::SegChunk k;
            uint64_t seg;
            for (uint64_t c = w.c; w.next(&k, &seg); c++, seen++) check_trusted(k, seg, ref[c], true, &tile, c);
        }
        if (seen != nchunks) fail("trusted: the ranges do not cover the chunks", (long long)seen, nw);
        tile.done("trusted walk: object byte not covered once");
    }
    std::vector<uint64_t> order(nchunks);  /* the random-access locate, in a shuffled order */
    for (uint64_t c = 0; c < nchunks; c++) order[c] = c;
    for (uint64_t c = nchunks; c > 1; c--) std::swap(order[c - 1], order[below(c)]);
    for (int variant = 0; variant < 8; variant++) {
        const bool place = variant & 1, no_head = variant & 2, search = variant & 4;
        Pass b = a;
        if (search) b.map_cap = 0;  /* (MCHECKSUM_GPU_SEG_MAP_CAP=0: the search over C) */
        Tiling tile(L);
        for (uint64_t c : order) {
            mck::SegChunk k;
            uint64_t seg;
            if (place) locate<CH, true>(b, c, nchunks, no_head, &k, &seg);
            else locate<CH, false>(b, c, nchunks, no_head, &k, &seg);
            check_trusted(k, seg, ref[c], place, &tile, c);
        }
        tile.done("trusted locate: object byte not covered once");
    }
}

/* A record a pass would hash (and copy) from tables it cannot trust. */
static void check_untrusted(const Pass &a, const mck::SegChunk &k, uint64_t seg, bool place, int kind) {
    if (!k.in) {
        n_skipped[kind]++;
        return;
    }
    n_yielded[kind]++;
    typedef unsigned __int128 u128;
    if (seg >= a.nseg || k.addr < a.L->addr[seg] || (u128)k.addr + k.n > (u128)a.L->addr[seg] + a.L->len[seg] || !k.n)
        fail("untrusted: bytes outside the caller's segment", (long long)seg, (long long)k.n);
    if (k.after >= (1ull << 48) || (u128)k.at + k.n + k.after != k.end)
        fail("untrusted: shift count wrapped or past 2^48", (long long)seg, (long long)k.after);
    if (place && (u128)k.obj_at + k.obj_off != k.at) fail("untrusted: negative offset in the object", (long long)seg, 0);
    if (k.obj >= a.nobj) fail("untrusted: no such object", (long long)seg, (long long)k.obj);
}

template <uint64_t CH>
static void run_untrusted(const Layout &L, Tables t, int kind) {
    const uint64_t nseg = L.len.size(), nobj = L.first.size() - 1;
    if (!nobj || !nseg) return;
    /* the workspace is the caller's, sized for this list: what the other list
     * did not fill holds whatever it held */
    auto word = [&]() -> uint64_t {  /* small, table-sized and arbitrary words alike */
        const uint64_t r = rnd();
        switch (r >> 62) {
        case 0: return (r >> 8) % (2 * nseg + 2);
        case 1: return (r >> 8) % (CH * (nseg + 1));
        case 2: return mck::kNoObj;
        default: return r * 0x9E3779B97F4A7C15ull;
        }
    };
    const size_t cap = mck::seg_work_layout(nseg).map_cap;
    while (t.P.size() < nseg + 1) t.P.push_back(word());
    while (t.C.size() < nseg + 1) t.C.push_back(word());
    while (t.obj.size() < 4 * nseg) t.obj.push_back(word());
    while (t.map.size() < cap) t.map.push_back((uint32_t)word());
    t.P.resize(nseg + 1);
    t.C.resize(nseg + 1);
    t.obj.resize(4 * nseg);
    t.map.resize(cap);
    if (kind == 1) {  /* random words: one word in eight of every table (all of them would yield nothing to check) */
        for (auto &x : t.P) x = below(8) ? x : word();
        for (auto &x : t.C) x = below(8) ? x : word();
        for (auto &x : t.obj) x = below(8) ? x : word();
        for (auto &x : t.map) x = below(8) ? x : (uint32_t)word();
    }
    const uint64_t nchunks = t.C[nseg] % (8 * (nseg + 1) + 64);  /* (the walk here stays short; the kernels' is only long) */
    t.C[nseg] = nchunks;
    const Pass a{&L, &t, nseg, nobj, cap};
    for (uint32_t wave = 0; wave < 7; wave++) {
        Walk<CH> w(a, wave, 7, nchunks);
        mck::SegChunk k;
        uint64_t seg;
        while (w.next(&k, &seg)) check_untrusted(a, k, seg, true, kind);
    }
    for (int variant = 0; variant < 4; variant++) {
        const bool place = variant & 1, search = variant & 2;
        Pass b = a;
        if (search) b.map_cap = 0;
        for (uint64_t c = 0; c < nchunks; c++) {
            mck::SegChunk k;
            uint64_t seg;
            if (place) locate<CH, true>(b, c, nchunks, false, &k, &seg);
            else locate<CH, false>(b, c, nchunks, false, &k, &seg);
            check_untrusted(b, k, seg, place, kind);
        }
    }
}

template <uint64_t CH>
static void run_records(const std::vector<uint64_t> &pool, const uint64_t (*shapes)[2], size_t nshapes, int seeds) {
    for (size_t k = 0; k < nshapes; k++)
        for (int sub = 0; sub < 2; sub++) run_trusted<CH>(make_layout(shapes[k][0], shapes[k][1], pool, sub != 0));
    for (int seed = 0; seed < seeds; seed++) {  /* this list's pass on the workspace another list's scan left */
        const uint64_t *mine = shapes[below(nshapes)], *other = shapes[below(nshapes)];
        const Layout L = make_layout(mine[0], mine[1], pool, below(2) != 0);
        const Layout stale = make_layout(other[0], other[1], pool, below(2) != 0);
        run_untrusted<CH>(L, scan_tables<CH>(stale), 0);
        run_untrusted<CH>(L, scan_tables<CH>(stale), 1);
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
    /* the workspace layout, and the chunk record over the same kinds of list:
     * a trusted scan's tables, then tables that cannot be trusted */
    check_layout();
    run_records<mck::kSegChunk>(big, big_shapes, 4, 16);
    run_records<48>(small, small_shapes, 8, 64);
    printf("%llu records of trusted scans; stale tables: %llu records yielded, %llu skipped; random words: %llu yielded, "
           "%llu skipped\n", n_trusted, n_yielded[0], n_skipped[0], n_yielded[1], n_skipped[1]);
    if (!n_trusted || !n_yielded[0] || !n_skipped[0] || !n_yielded[1]) {
        printf("the record checks are vacuous\n");
        return 1;
    }
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
