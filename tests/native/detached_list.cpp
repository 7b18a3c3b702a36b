// The detached calls with both sides by address list (include/mchecksum_gpu.h:
// mchecksum_gpu_verify_detached_message_list, _seal_, and the two
// _state_*_message_list calls): the rules the kernels run
// (mercury_amd/csrc/launch_plan.h: list_msg_len, list_payload_ok, _len, _at,
// msg_slot_ok) and a plain emulation of what a wave reads and writes per entry
// (crc_gpu_crc32.h, BOTH; state_message_list_kernel), against a model written
// here from the header text alone.  `wave_*` below index the four arrays as the
// kernel does -- entry p of each, never entry `count` -- and take every byte
// through its address with no buffer under it.  hash_offset 16 and 13; L = 0 ..
// hash_offset + 8; payloads of 0 .. 1025 bytes; each of payload and slot right
// and wrong; both wrap cases.  Every message and every payload sits alone in an
// exactly sized heap allocation, the allocations are handed over in shuffled
// order, all arrays hold exactly `count` entries, and every slotless message
// and every empty payload has a NULL address: a byte read between, before or
// behind entries, a dereferenced NULL or a read of entry `count` is the
// sanitizer's.  Then the key space: the both_lists field names six kernels, no
// others, and leaves every count tests/native/launch_plan.cpp and
// rpc_list_msg.cpp pin as it was; and the host front's call shape
// (offsets_call.h).  Stand-alone: plain and under the sanitizers
// (tests/test_detached_list.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "crc_gpu_window.h"
#include "launch_plan.h"
#include "offsets_call.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (g_fail++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                               \
    } while (0)

enum Verdict : int { GOOD = 0, PAYLOAD_DIFFERS, SLOT_DIFFERS, NO_SLOT, EMPTY_PAYLOAD, WRAPPED, VERDICTS };

// ---- the model: nothing from launch_plan.h below this line ----
uint32_t naive_crc32c(const uint8_t *p, size_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        r ^= p[i];
        for (int k = 0; k < 8; k++) r = r & 1u ? (r >> 1) ^ 0x82F63B78u : r >> 1;
    }
    return ~r;
}
uint32_t be32(const uint8_t *q) { return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3]; }

// `n` bytes alone in an allocation of exactly n bytes, or none behind a NULL address
struct Blob {
    std::unique_ptr<uint8_t[]> bytes;
    size_t n = 0;
    uint8_t *p() const { return bytes.get(); }
};
// "Its slot exists iff L >= hash_offset + 4"; "a verify counts it as a mismatch with status 1"
uint32_t naive_verify(const Blob &msg, const Blob &pay, size_t hash) {
    if (msg.n < hash + 4) return 1;
    return naive_crc32c(pay.p(), pay.n) == be32(msg.p() + hash) ? 0 : 1;
}
// "a seal gives status 1 and makes no store"; "exactly those 4 bytes per entry and nothing else"
uint32_t naive_seal(Blob &msg, const Blob &pay, size_t hash) {
    if (msg.n < hash + 4) return 1;
    const uint32_t x = naive_crc32c(pay.p(), pay.n);
    for (int b = 0; b < 4; b++) msg.p()[hash + b] = (uint8_t)(x >> (24 - 8 * b));
    return 0;
}

// ---- what a wave does with entry p of the lists, with launch_plan.h's functions ----
// The kernel's `base + offset` with a null base: an address is all there is.
uint8_t *at_addr(uint64_t a) { return reinterpret_cast<uint8_t *>((uintptr_t)a); }

// the payload loop: n bytes at address o.  An empty payload runs at address 0: a window of no step
// (crc_gpu_window.h), checked in main.
uint32_t payload(uint64_t o, uint64_t n) {
    if (n == 0) {
        CHECK(o == 0);
        return naive_crc32c(nullptr, 0);
    }
    return naive_crc32c(at_addr(o), n);
}
struct Lists {
    const uint64_t *msg_addr, *msg_len, *pay_addr, *pay_len;  // `count` entries each
};
// the owning lane's epilogue: the slot by address and length (the batch kernels' and state_message_list_kernel's)
uint32_t slot_epilogue(bool seal, uint64_t h0, uint64_t len, uint64_t hash, uint32_t x, bool failed) {
    const uint64_t h1 = h0 + mck::list_msg_len(h0, len);
    const bool short_msg = !mck::msg_slot_ok(h0, h1, hash) || failed;
    if (seal) {
        if (!short_msg)
            for (int b = 0; b < 4; b++) at_addr(mck::msg_slot_at(h0, hash))[b] = (uint8_t)(x >> (24 - 8 * b));
        return short_msg ? 1 : 0;
    }
    return short_msg || be32(at_addr(mck::msg_slot_at(h0, hash))) != x ? 1 : 0;
}
uint32_t wave(bool seal, const Lists &l, uint64_t p, uint64_t hash) {
    const uint64_t m0 = l.pay_addr[p], m1 = m0 + l.pay_len[p], n = m1 - m0;  // (the kernel's: the length whether m1 wraps or not)
    const bool wrapped = !mck::list_payload_ok(m0, n);
    const uint32_t x = payload(mck::list_payload_at(m0, n), mck::list_payload_len(m0, n));
    return slot_epilogue(seal, l.msg_addr[p], l.msg_len[p], hash, x, wrapped);
}
// the streamed ending: the value comes from a state, the slot as above
uint32_t element_state(bool seal, const Lists &l, uint64_t p, uint64_t hash, uint32_t value) {
    return slot_epilogue(seal, l.msg_addr[p], l.msg_len[p], hash, value, false);
}

uint32_t g_rng = 20261021;
uint32_t next() { return g_rng = g_rng * 1664525u + 1013904223u; }

Blob make_blob(size_t n, bool null_if) {
    Blob b;
    b.n = n;
    if (!null_if && n) {
        b.bytes.reset(new uint8_t[n]);
        for (size_t i = 0; i < n; i++) b.bytes[i] = (uint8_t)(next() >> 24);
    }
    return b;
}
Blob clone(const Blob &a) {
    Blob b;
    b.n = a.n;
    if (a.bytes) {
        b.bytes.reset(new uint8_t[a.n]);
        std::memcpy(b.p(), a.p(), a.n);
    }
    return b;
}
bool same(const Blob &a, const Blob &b) { return a.n == b.n && (!a.bytes || std::memcmp(a.p(), b.p(), a.n) == 0); }

struct Case {
    size_t L, N;
    int variant;  // 0: as sealed, 1: one payload bit flipped, 2: one slot bit flipped
};

}  // namespace

int main() {
    unsigned long long seen[VERDICTS] = {0}, entries = 0;
    const size_t payload_sizes[] = {0, 1, 3, 15, 16, 17, 100, 1023, 1025};
    for (const uint64_t hash : {16u, 13u}) {
        std::vector<Case> cases;
        for (size_t L = 0; L <= hash + 8; L++)
            for (size_t N : payload_sizes)
                for (int variant = 0; variant < 3; variant++) cases.push_back({L, N, variant});
        // the lists' order is not the allocations': a shuffle (allocation i is made i-th, handed over perm[i]-th)
        const size_t count = cases.size();
        std::vector<size_t> perm(count);
        for (size_t i = 0; i < count; i++) perm[i] = i;
        for (size_t i = count - 1; i > 0; i--) std::swap(perm[i], perm[next() % (i + 1)]);
        std::vector<Case> by_slot(count);
        std::vector<Blob> msg0(count), pay0(count);
        for (size_t i = 0; i < count; i++) {
            by_slot[perm[i]] = cases[i];
            msg0[perm[i]] = make_blob(cases[i].L, cases[i].L < hash + 4);  // a slotless message: NULL
            pay0[perm[i]] = make_blob(cases[i].N, false);                 // an empty payload: NULL
        }
        std::vector<uint64_t> ma, ml, pa, pl;
        auto lists_of = [&](const std::vector<Blob> &m, const std::vector<Blob> &p) {
            for (auto *v : {&ma, &ml, &pa, &pl}) v->assign(count, 0), v->shrink_to_fit();  // entry `count` is the sanitizer's
            for (size_t i = 0; i < count; i++) {
                ma[i] = (uint64_t)(uintptr_t)m[i].p(), ml[i] = m[i].n;
                pa[i] = (uint64_t)(uintptr_t)p[i].p(), pl[i] = p[i].n;
            }
            return Lists{ma.data(), ml.data(), pa.data(), pl.data()};
        };
        // ---- seal: the wave against the model, entry by entry ----
        std::vector<Blob> a(count), b(count), st(count);
        for (size_t i = 0; i < count; i++) a[i] = clone(msg0[i]), b[i] = clone(msg0[i]), st[i] = clone(msg0[i]);
        Lists l = lists_of(a, pay0);
        for (size_t p = 0; p < count; p++) {
            CHECK((ma[p] == 0) == (by_slot[p].L < hash + 4) && (pa[p] == 0) == (by_slot[p].N == 0));
            const Blob pay_before = clone(pay0[p]);
            const uint32_t sa = wave(true, l, p, hash), sb = naive_seal(b[p], pay0[p], hash);
            CHECK(sa == sb && same(a[p], b[p]) && same(pay0[p], pay_before));
            CHECK(sa == (by_slot[p].L < hash + 4 ? 1u : 0u));
            for (size_t i = 0; a[p].bytes && i < a[p].n; i++)
                if (sa || i < hash || i >= hash + 4) CHECK(a[p].p()[i] == msg0[p].p()[i]);  // those 4 bytes, no others
        }
        // the streamed seal: the same slots from a value per entry
        {
            Lists ls = lists_of(st, pay0);
            for (size_t p = 0; p < count; p++) {
                CHECK(element_state(true, ls, p, hash, naive_crc32c(pay0[p].p(), pay0[p].n)) == (by_slot[p].L < hash + 4 ? 1u : 0u));
                CHECK(same(st[p], a[p]));
            }
        }
        // ---- verify: the sealed messages and their payloads, one bit flipped by the case's variant ----
        std::vector<Blob> rm(count), rp(count);
        for (size_t p = 0; p < count; p++) {
            rm[p] = clone(a[p]), rp[p] = clone(pay0[p]);
            const Case &c = by_slot[p];
            if (c.variant == 1 && c.N) rp[p].p()[(c.L * 7) % c.N] ^= (uint8_t)(1u << (c.L % 8));
            if (c.variant == 2 && c.L >= hash + 4) rm[p].p()[hash + c.L % 4] ^= (uint8_t)(1u << (c.N % 8));
        }
        std::vector<Blob> rm0(count), rp0(count);
        for (size_t p = 0; p < count; p++) rm0[p] = clone(rm[p]), rp0[p] = clone(rp[p]);
        l = lists_of(rm, rp);
        for (size_t p = 0; p < count; p++) {
            const Case &c = by_slot[p];
            const uint32_t va = wave(false, l, p, hash);
            CHECK(va == naive_verify(rm0[p], rp0[p], hash));
            CHECK(same(rm[p], rm0[p]) && same(rp[p], rp0[p]));  // a verify writes nothing
            CHECK(element_state(false, l, p, hash, naive_crc32c(rp0[p].p(), rp0[p].n)) == va);
            const bool slot = c.L >= hash + 4, flipped = slot && ((c.variant == 1 && c.N) || c.variant == 2);
            CHECK(va == (!slot || flipped ? 1u : 0u));
            seen[!slot ? NO_SLOT : c.variant == 1 && c.N ? PAYLOAD_DIFFERS : c.variant == 2 ? SLOT_DIFFERS : c.N == 0 ? EMPTY_PAYLOAD : GOOD]++;
            entries++;
        }
        // ---- both wrap cases: an end past the address space ----
        for (uint64_t back = 1; back <= 32; back++) {
            // a message whose end wraps holds no bytes: no slot, never dereferenced -- whatever the payload
            Blob pay = make_blob(17, false);
            const uint64_t wa[1] = {~0ull - back + 1}, wl[1] = {back + hash + 8}, pa1[1] = {(uint64_t)(uintptr_t)pay.p()}, pl1[1] = {17};
            CHECK(mck::list_msg_len(wa[0], wl[0]) == 0 && mck::list_msg_len(wa[0], back - 1) == back - 1);
            CHECK(wave(false, Lists{wa, wl, pa1, pl1}, 0, hash) == 1 && wave(true, Lists{wa, wl, pa1, pl1}, 0, hash) == 1);
            CHECK(element_state(false, Lists{wa, wl, pa1, pl1}, 0, hash, 0) == 1 && element_state(true, Lists{wa, wl, pa1, pl1}, 0, hash, 0) == 1);
            // a payload whose end wraps fails the entry, and nothing of it is read: its message holds the empty
            // payload's CRC in a good slot, and still the verdict is 1 and a seal stores nothing
            Blob msg = make_blob(hash + 4, false);
            const uint32_t x0 = naive_crc32c(nullptr, 0);
            for (int k = 0; k < 4; k++) msg.p()[hash + k] = (uint8_t)(x0 >> (24 - 8 * k));
            const Blob before = clone(msg);
            const uint64_t ma1[1] = {(uint64_t)(uintptr_t)msg.p()}, ml1[1] = {hash + 4}, wp[1] = {~0ull - back + 1}, wn[1] = {back + 1024};
            CHECK(!mck::list_payload_ok(wp[0], wn[0]) && mck::list_payload_ok(wp[0], back - 1));
            CHECK(mck::list_payload_len(wp[0], wn[0]) == 0 && mck::list_payload_at(wp[0], wn[0]) == 0);
            CHECK(wave(false, Lists{ma1, ml1, wp, wn}, 0, hash) == 1);
            CHECK(wave(true, Lists{ma1, ml1, wp, wn}, 0, hash) == 1 && same(msg, before));
            // ... where a legitimate empty payload at that slot passes, from a NULL address
            const uint64_t zp[1] = {0}, zn[1] = {0};
            CHECK(wave(false, Lists{ma1, ml1, zp, zn}, 0, hash) == 0);
            seen[WRAPPED] += 2;
            entries += 2;
        }
    }
    for (int k = 0; k < VERDICTS; k++) CHECK(seen[k] > 0);

    // the rules at their edges
    CHECK(mck::list_payload_at(0x1000, 0) == 0 && mck::list_payload_at(0x1000, 1) == 0x1000 && mck::list_payload_len(0x1000, 5) == 5);
    CHECK(mck::list_payload_ok(~0ull, 0) && !mck::list_payload_ok(~0ull, 1) && mck::list_payload_ok(0, ~0ull));
    CHECK(mck::list_msg_len(~0ull, 1) == 0 && mck::list_msg_len(~0ull - 1, 1) == 1 && mck::list_msg_len(0, 0) == 0);
    // the empty payload: at address 0 the payload loop's window has no step -- no load --, where at its own address
    // it may have one
    {
        const GridWindow w(0, 0, 4);
        CHECK(w.K == 0 && w.pad() == 0);
        CHECK(GridWindow(0x1000 + 37, 0, 4).K == 1);
    }

    // ---- the key space ----
    // Six keys carry both_lists: the detached frame's (light, full, non-temporal) x (verify, seal).  With the field
    // clear every pinned count is what it was: in the payloads frame 35 fixed CRC-32C, 21 fixed CRC-64, 2 split, 15
    // offsets checksum / verify / update and 9 seal / pack / unpack; 0 in place, 6 detached, 12 RPC, none past the
    // last frame; 12 keys with `list`, all RPC.
    int n_both = 0, n_list = 0, n[5] = {0, 0, 0, 0, 0}, nf[mck::kFrameRpc + 2] = {0, 0, 0, 0, 0};
    for (int both = 0; both < 2; both++)
        for (int list = 0; list < 2; list++)
            for (int frame = -1; frame <= mck::kFrameRpc + 1; frame++)
                for (int width : {16, 32, 64})
                    for (int lg = -1; lg <= CRC_GPU_MAX_LOG2G + 1; lg++)
                        for (int mode = -1; mode <= kOffsets + 1; mode++)
                            for (int op = -1; op <= mck::kOpUnpack + 1; op++)
                                for (int f = 0; f < 8; f++) {
                                    const mck::KernelKey k{width, lg, mode, op, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0,
                                                           (mck::MsgFrame)frame, list != 0, both != 0};
                                    if (!mck::kernel_key_valid(k)) continue;
                                    CHECK(frame >= 0 && frame <= mck::kFrameRpc && mode >= 0 && mode <= kOffsets);
                                    if (both) {
                                        n_both++;
                                        CHECK(frame == mck::kFrameDetached && !list && width == 32 && mode == kOffsets && lg == CRC_GPU_MAX_LOG2G);
                                        CHECK(op == mck::kOpVerify || op == mck::kOpSeal);
                                        CHECK(!k.split && !(k.nt && k.light));
                                        mck::KernelKey table = k;
                                        table.both_lists = false;
                                        CHECK(mck::kernel_key_valid(table) && !(table == k));  // a twin of a table kernel, and another key
                                    } else if (list) {
                                        n_list++;
                                        CHECK(frame == mck::kFrameRpc);
                                    } else if (frame == mck::kFramePayloads) {
                                        n[k.split ? 2 : mode != kOffsets ? (width == 64) : op <= mck::kOpUpdate ? 3 : 4]++;
                                    } else {
                                        nf[frame]++;
                                    }
                                }
    CHECK(n_both == 6 && n_list == 12);
    CHECK(n[0] == 35 && n[1] == 21 && n[2] == 2 && n[3] == 15 && n[4] == 9);
    CHECK(nf[mck::kFrameInPlace] == 0 && nf[mck::kFrameDetached] == 6 && nf[mck::kFrameRpc] == 12 && nf[mck::kFrameRpc + 1] == 0);
    CHECK((!mck::KernelKey{32, 6, kOffsets, mck::kOpVerify, false, false, false, mck::kFrameDetached}.both_lists));  // the default: tables
    const mck_settings_t s = [] {
        mck_settings_t v{};
        v.gpu_light = v.gpu_nt = v.gpu_log2g = v.gpu_split = v.gpu_xdr_fast = -1;  // nothing set: the library decides
        v.gpu_split_lds = 1;
        return v;
    }();
    for (size_t count : {1u, 1024u, 1025u, 8191u, 8192u}) {
        const mck::LaunchPlan p = mck::plan_offsets(s, 256, 32, count);  // the table form's plan for the same count
        for (int op : {mck::kOpVerify, mck::kOpSeal}) {
            const mck::KernelKey t = mck::kernel_key(p, (mck::BatchOp)op, mck::kFrameDetached);
            const mck::KernelKey l = mck::kernel_key(p, (mck::BatchOp)op, mck::kFrameDetached, false, true);
            CHECK(!t.both_lists && l.both_lists && !l.list && mck::kernel_key_valid(l));
            mck::KernelKey u = l;
            u.both_lists = false;
            CHECK(u == t);
            CHECK(l.light == (count <= 1024) && l.nt == (count >= 8192));
        }
        CHECK(p.dyn == (count > 1024));  // the queue from 1,025 entries on: what tests/test_gpu_detached_list.py relies on
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpVerify, mck::kFrameDetached, true)));  // still no {detached, list}
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpVerify, mck::kFrameDetached, true, true)));
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpVerify, mck::kFrameRpc, false, true)));
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpVerify, mck::kFramePayloads, false, true)));
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpVerify, mck::kFrameInPlace, false, true)));
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpChecksum, mck::kFrameDetached, false, true)));
    }

    // ---- the host front's call shape (offsets_call.h) ----
    {
        uint64_t maddr[1] = {0}, mlen[1] = {0}, paddr[1] = {0}, plen[1] = {0};
        uint8_t buf[1] = {0};
        for (int op : {mck::kOpVerify, mck::kOpSeal}) {
            mck::OffsetsCall c{(mck::BatchOp)op, "crc32c", nullptr, paddr, 1};
            c.frame = mck::kFrameDetached;
            c.both_lists = true;
            c.payload_len = plen;
            c.hdr_off = maddr;
            c.msg_len = mlen;
            CHECK(!mck::offsets_lacks_pointer(c));  // no buffer under either list, no `out` of a seal
            mck::OffsetsCall d = c;
            d.src_off = nullptr;
            CHECK(mck::offsets_lacks_pointer(d));
            d = c;
            d.payload_len = nullptr;
            CHECK(mck::offsets_lacks_pointer(d));
            d = c;
            d.hdr_off = nullptr;
            CHECK(mck::offsets_lacks_pointer(d));
            d = c;
            d.msg_len = nullptr;
            CHECK(mck::offsets_lacks_pointer(d));
            d = c;
            d.count = 0, d.src_off = nullptr, d.payload_len = nullptr, d.hdr_off = nullptr, d.msg_len = nullptr;
            CHECK(!mck::offsets_lacks_pointer(d));
            // the kernels' argument: both buffers null whatever the call holds, and a length array behind each accessor
            c.src = buf, c.hdr = buf;
            const BatchArgs a = mck::batch_args_of(c, nullptr, nullptr, nullptr, false, nullptr);
            CHECK(a.base == nullptr && a.msgs == nullptr && a.offsets == paddr && a.dst_offsets == maddr);
            CHECK(a.rpc_list_len() == plen && a.stride == (uint64_t)(uintptr_t)plen);
            CHECK(a.slot_list_len() == mlen && a.len == (uint64_t)(uintptr_t)mlen);
            CHECK(a.count == 1 && a.shift == nullptr);
            // the table form is what it was
            uint64_t tab[2] = {0, 0};
            mck::OffsetsCall t{(mck::BatchOp)op, "crc32c", buf, tab, 1};
            t.frame = mck::kFrameDetached;
            t.hdr = buf, t.hdr_off = tab;
            CHECK(!mck::offsets_lacks_pointer(t));
            const BatchArgs ta = mck::batch_args_of(t, nullptr, nullptr, nullptr, false, nullptr);
            CHECK(ta.stride == 0 && ta.len == 0 && ta.base == buf && ta.msgs == buf);
            t.hdr = nullptr;
            CHECK(mck::offsets_lacks_pointer(t));
            const mck::OffsetsNeeds tn = mck::offsets_needs((mck::BatchOp)op, mck::kFrameDetached);
            CHECK(tn.src_buf && tn.hdr_buf && !tn.msg_len && !tn.payload_len && tn.hdr && tn.method_first);
            const mck::OffsetsNeeds ln = mck::offsets_needs((mck::BatchOp)op, mck::kFrameDetached, false, true);
            CHECK(!ln.src_buf && !ln.hdr_buf && ln.msg_len && ln.payload_len && ln.hdr && ln.method_first && !ln.out);
        }
    }

    std::printf("%llu entries: good %llu payload %llu slot %llu noslot %llu empty %llu wrapped %llu\n", entries, seen[GOOD],
                seen[PAYLOAD_DIFFERS], seen[SLOT_DIFFERS], seen[NO_SLOT], seen[EMPTY_PAYLOAD], seen[WRAPPED]);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
