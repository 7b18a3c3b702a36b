// The RPC message calls by address list (include/mchecksum_gpu.h:
// mchecksum_gpu_verify_rpc_message_list, _seal_, _unpack_, _pack_): the rules
// the kernels run (mercury_amd/csrc/launch_plan.h) and a plain emulation of
// what each call's wave reads and writes of a LIST (crc_gpu_crc32.h, LIST),
// against a model written here from the header text alone.  `wave_*` below
// index the two arrays as the kernel does -- entry p of each, never entry
// `count` -- and take a message's bytes through its address with no buffer
// under it.  Both kinds; L = 0 .. payload_offset + 8; R = L - payload_offset
// - 1 .. + 1; MORE_DATA set and clear; each hash right and wrong.  Every
// message sits alone in an exactly sized heap allocation, the allocations are
// handed over in shuffled order, both arrays hold exactly `count` entries, and
// a message with L < 16 has a NULL address: a byte read between, before or
// behind messages, a dereferenced SHORT address or a read of entry `count` is
// the sanitizer's.  Then the key space: the list field names twelve kernels,
// no others, and leaves every count tests/native/launch_plan.cpp pins as it
// was; and the host front's call shape (offsets_call.h).  Stand-alone: plain
// and under the sanitizers (tests/test_rpc_list_msg.py).
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

struct Model16 {
    const char *name;
    uint32_t poly;
    bool reflected;
    uint32_t init, xorout;
};
const Model16 kModels[] = {
    {"crc16-kermit", 0x1021, true, 0x0000, 0x0000},
    {"crc16-genibus", 0x1021, false, 0xFFFF, 0xFFFF},
};
enum : uint32_t { OK = 0, PAYLOAD, HEADER, SHORT, DEFERRED, FAULT, MISFIT, CLASSES };
const uint8_t kSentinel = 0xA5;

// ---- the model: nothing from launch_plan.h below this line ----
uint32_t naive_crc16(const Model16 &m, const uint8_t *p, size_t n) {
    uint32_t r = m.init;
    for (size_t i = 0; i < n; i++) {
        uint32_t b = p[i];
        if (m.reflected) {
            uint32_t v = 0;
            for (int k = 0; k < 8; k++) v |= ((b >> k) & 1u) << (7 - k);
            b = v;
        }
        r ^= b << 8;
        for (int k = 0; k < 8; k++) r = (r & 0x8000u ? (r << 1) ^ m.poly : r << 1) & 0xFFFFu;
    }
    if (m.reflected) {
        uint32_t v = 0;
        for (int k = 0; k < 16; k++) v |= ((r >> k) & 1u) << (15 - k);
        r = v;
    }
    return (r ^ m.xorout) & 0xFFFFu;
}
uint32_t naive_crc32c(const uint8_t *p, size_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        r ^= p[i];
        for (int k = 0; k < 8; k++) r = r & 1u ? (r >> 1) ^ 0x82F63B78u : r >> 1;
    }
    return ~r;
}
// the core header's CRC-16 over the host-order image, field by field
uint32_t naive_hdr_crc(const Model16 &m, int kind, const uint8_t *h) {
    uint8_t img[12];
    if (kind == 0) {
        img[0] = h[0];  // hg
        img[1] = h[1];  // protocol
        uint64_t id = 0;
        for (int b = 0; b < 8; b++) id = id << 8 | h[2 + b];  // big-endian on the wire
        std::memcpy(img + 2, &id, 8);                         // a little-endian host's uint64_t
        img[10] = h[10];  // flags
        img[11] = h[11];  // cookie
        return naive_crc16(m, img, 12);
    }
    img[0] = h[0];  // ret_code
    img[1] = h[1];  // flags
    const uint16_t cookie = (uint16_t)(h[2] << 8 | h[3]);
    std::memcpy(img + 2, &cookie, 2);
    return naive_crc16(m, img, 4);
}
size_t flags_at(int kind) { return kind == 0 ? 10 : 1; }
size_t hdr_hash_at(int kind) { return kind == 0 ? 12 : 4; }
uint32_t be32(const uint8_t *q) { return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3]; }

// A message of the model: its bytes, or none behind a NULL address when it is shorter than a core header.
struct Msg {
    std::unique_ptr<uint8_t[]> bytes;  // exactly L bytes of heap (new uint8_t[L]), or null
    size_t L = 0;
    uint8_t *p() const { return bytes.get(); }
};

uint32_t naive_verify(const Model16 &m, int kind, const Msg &g, size_t pay, size_t hash) {
    if (g.L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (naive_hdr_crc(m, kind, g.p()) != (uint32_t)(g.p()[at] << 8 | g.p()[at + 1])) return HEADER;
    if (g.p()[flags_at(kind)] & 1) return DEFERRED;
    if (g.L < pay) return SHORT;
    return naive_crc32c(g.p() + pay, g.L - pay) == be32(g.p() + hash) ? OK : PAYLOAD;
}
uint32_t naive_seal(const Model16 &m, int kind, Msg &g, size_t pay, size_t hash) {
    if (g.L < 16) return SHORT;
    const bool more = g.p()[flags_at(kind)] & 1;
    if (!more && g.L < pay) return SHORT;
    if (!more) {
        const uint32_t x = naive_crc32c(g.p() + pay, g.L - pay);
        for (int b = 0; b < 4; b++) g.p()[hash + b] = (uint8_t)(x >> (24 - 8 * b));
    }
    const uint32_t c = naive_hdr_crc(m, kind, g.p());
    g.p()[hdr_hash_at(kind)] = (uint8_t)(c >> 8);
    g.p()[hdr_hash_at(kind) + 1] = (uint8_t)c;
    return more ? DEFERRED : OK;
}
uint32_t naive_unpack(const Model16 &m, int kind, const Msg &g, size_t pay, size_t hash, uint8_t *dst, size_t R) {
    const size_t L = g.L;
    const bool more = L >= 16 && (g.p()[flags_at(kind)] & 1);
    if (L >= 16 && !more && L >= pay && L == pay + R)
        for (size_t i = 0; i < R; i++) dst[i] = g.p()[pay + i];
    if (L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (naive_hdr_crc(m, kind, g.p()) != (uint32_t)(g.p()[at] << 8 | g.p()[at + 1])) return HEADER;
    if (more) return DEFERRED;
    if (L < pay) return SHORT;
    if (L != pay + R) return MISFIT;
    return naive_crc32c(g.p() + pay, R) == be32(g.p() + hash) ? OK : PAYLOAD;
}
uint32_t naive_pack(const Model16 &m, int kind, Msg &g, size_t pay, size_t hash, const uint8_t *src, size_t R) {
    const size_t L = g.L;
    if (L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (g.p()[flags_at(kind)] & 1) {
        const uint32_t c = naive_hdr_crc(m, kind, g.p());
        g.p()[at] = (uint8_t)(c >> 8);
        g.p()[at + 1] = (uint8_t)c;
        return DEFERRED;
    }
    if (L < pay) return SHORT;
    if (L != pay + R) return MISFIT;
    for (size_t i = 0; i < R; i++) g.p()[pay + i] = src[i];
    const uint32_t x = naive_crc32c(src, R);
    for (int b = 0; b < 4; b++) g.p()[hash + b] = (uint8_t)(x >> (24 - 8 * b));
    const uint32_t c = naive_hdr_crc(m, kind, g.p());
    g.p()[at] = (uint8_t)(c >> 8);
    g.p()[at + 1] = (uint8_t)c;
    return OK;
}

// ---- what a wave does with entry p of a list, with launch_plan.h's functions ----
// The kernel's `base + offset` with a null base: an address is all there is.
uint8_t *at_addr(uint64_t a) { return reinterpret_cast<uint8_t *>((uintptr_t)a); }

struct Front {
    bool more = false;
    uint32_t crc16 = 0, wire = 0;
};
// sixteen lanes: a header byte each, the flags from its lane, a term each (only of a whole header)
Front lanes_front(const mck::RpcHdrPack &pk, uint32_t kind, uint64_t g0, uint64_t L) {
    Front r;
    const bool whole = L >= mck::kRpcHdrBytes;
    uint32_t hb[16] = {0}, term[16] = {0};
    for (uint32_t lane = 0; lane < 16; lane++)
        if (whole) hb[lane] = at_addr(g0)[lane];
    r.more = whole && (hb[mck::rpc_flags_at(kind)] & 1u);
    for (uint32_t lane = 0; lane < 16; lane++)
        if (whole) term[lane] = mck::rpc_hdr_term(&pk, kind, lane, hb[lane]);
    uint32_t t = 0;
    for (uint32_t lane = 0; lane < mck::rpc_img_bytes(kind); lane++) t ^= term[lane];
    r.crc16 = mck::rpc_hdr_crc(pk.c, t);
    const uint32_t hat = mck::rpc_hash_at(kind);
    r.wire = term[hat] << 8 | term[hat + 1];
    return r;
}
// the payload loop: n bytes at address o are hashed and, with a dst, stored.  The LIST kernels run a payload that is
// not hashed at address 0 with n = 0: a window of no step (crc_gpu_window.h), checked in main.
uint32_t payload(uint64_t o, uint64_t n, uint8_t *dst) {
    if (n == 0) return naive_crc32c(nullptr, 0);
    for (uint64_t i = 0; dst && i < n; i++) dst[i] = at_addr(o)[i];
    return naive_crc32c(at_addr(o), n);
}
struct List {
    const uint64_t *addr, *len;  // `count` entries each
};
uint32_t wave_verify(const mck::RpcHdrPack &pk, uint32_t kind, const List &l, uint64_t p, uint64_t pay, uint64_t hash) {
    const uint64_t m0 = l.addr[p], m1 = m0 + l.len[p], L = mck::rpc_len(m0, m1);
    const Front f = lanes_front(pk, kind, m0, L);
    const bool hashed = mck::rpc_hashes_payload(L, f.more, pay);
    uint64_t o = hashed ? m0 + pay : m0 + L;
    const uint64_t n = m0 + L - o;
    o = hashed ? o : 0;
    const uint32_t x = payload(o, n, nullptr);
    const bool pay_ok = hashed && be32(at_addr(m0 + hash)) == x;
    return mck::rpc_verify_class(L, f.crc16 == f.wire, f.more, pay, pay_ok);
}
uint32_t wave_seal(const mck::RpcHdrPack &pk, uint32_t kind, const List &l, uint64_t p, uint64_t pay, uint64_t hash) {
    const uint64_t m0 = l.addr[p], m1 = m0 + l.len[p], L = mck::rpc_len(m0, m1);
    const Front f = lanes_front(pk, kind, m0, L);
    const bool hashed = mck::rpc_hashes_payload(L, f.more, pay);
    uint64_t o = hashed ? m0 + pay : m0 + L;
    const uint64_t n = m0 + L - o;
    o = hashed ? o : 0;
    const uint32_t x = payload(o, n, nullptr);
    const uint32_t cls = mck::rpc_seal_class(L, f.more, pay);
    if (cls == mck::kRpcOk)
        for (int b = 0; b < 4; b++) at_addr(m0 + hash)[b] = (uint8_t)(x >> (24 - 8 * b));
    if (cls != mck::kRpcShort) {
        const uint32_t hat = mck::rpc_hash_at(kind);
        at_addr(m0)[hat] = (uint8_t)(f.crc16 >> 8);
        at_addr(m0)[hat + 1] = (uint8_t)f.crc16;
    }
    return cls;
}
uint32_t wave_unpack(const mck::RpcHdrPack &pk, uint32_t kind, const List &l, uint64_t p, uint64_t pay, uint64_t hash,
                     uint8_t *dst, const uint64_t *dst_off) {
    const uint64_t m0 = l.addr[p], m1 = m0 + l.len[p], L = mck::rpc_len(m0, m1);
    const Front f = lanes_front(pk, kind, m0, L);
    const uint64_t R = mck::rpc_len(dst_off[p], dst_off[p + 1]);
    const bool copied = mck::rpc_copies_payload(L, f.more, pay, R);
    const uint32_t x = payload(copied ? m0 + pay : 0, copied ? R : 0, dst + dst_off[p]);
    const bool pay_ok = copied && be32(at_addr(m0 + hash)) == x;
    return mck::rpc_unpack_class(L, f.crc16 == f.wire, f.more, pay, R, pay_ok);
}
uint32_t wave_pack(const mck::RpcHdrPack &pk, uint32_t kind, const List &l, uint64_t p, uint64_t pay, uint64_t hash,
                   const uint8_t *src, const uint64_t *src_off) {
    const uint64_t g0 = l.addr[p], g1 = g0 + l.len[p], L = mck::rpc_len(g0, g1);  // the list is the written side
    const Front f = lanes_front(pk, kind, g0, L);
    const uint64_t m0 = src_off[p], R = mck::rpc_len(m0, src_off[p + 1]);
    const bool copied = mck::rpc_copies_payload(L, f.more, pay, R);
    const uint32_t x = payload((uint64_t)(uintptr_t)(src + m0), copied ? R : 0, copied ? at_addr(g0 + pay) : nullptr);
    const uint32_t cls = mck::rpc_pack_class(L, f.more, pay, R);
    if (cls == mck::kRpcOk)
        for (int b = 0; b < 4; b++) at_addr(g0 + hash)[b] = (uint8_t)(x >> (24 - 8 * b));
    if (cls == mck::kRpcOk || cls == mck::kRpcDeferred) {
        const uint32_t hat = mck::rpc_hash_at(kind);
        at_addr(g0)[hat] = (uint8_t)(f.crc16 >> 8);
        at_addr(g0)[hat + 1] = (uint8_t)f.crc16;
    }
    return cls;
}

uint32_t g_rng = 20251021;
uint32_t next() { return g_rng = g_rng * 1664525u + 1013904223u; }

Msg make_msg(size_t L) {
    Msg g;
    g.L = L;
    if (L >= 16) {  // (a SHORT message has no bytes at all: its address is NULL)
        g.bytes.reset(new uint8_t[L]);
        for (size_t i = 0; i < L; i++) g.bytes[i] = (uint8_t)(next() >> 24);
    }
    return g;
}
Msg clone(const Msg &a) {
    Msg g;
    g.L = a.L;
    if (a.bytes) {
        g.bytes.reset(new uint8_t[a.L]);
        std::memcpy(g.p(), a.p(), a.L);
    }
    return g;
}
bool same(const Msg &a, const Msg &b) { return a.L == b.L && (!a.bytes || std::memcmp(a.p(), b.p(), a.L) == 0); }

struct Case {
    size_t L, R;
    int more, variant;
};

}  // namespace

int main() {
    const uint64_t shapes[][2] = {{20, 16}, {24, 16}, {21, 17}};  // payload_offset, hash_offset
    unsigned long long seen[CLASSES] = {0}, unpacked[CLASSES] = {0}, sealed[CLASSES] = {0}, packed[CLASSES] = {0}, msgs = 0;
    for (const Model16 &m : kModels)
        for (uint32_t kind = 0; kind < 2; kind++) {
            mck::RpcHdrPack pk;
            mck::rpc_hdr_pack_build(m.poly, m.reflected, m.init, m.xorout, kind, &pk);
            for (const auto &sh : shapes) {
                const uint64_t pay = sh[0], hash = sh[1];
                std::vector<Case> cases;
                for (uint64_t L = 0; L <= pay + 8; L++)
                    for (int d = -1; d <= 1; d++)
                        for (int more = 0; more < 2; more++)
                            for (int variant = 0; variant < 4; variant++)  // bit 0: header hash wrong, bit 1: payload hash wrong
                                cases.push_back({(size_t)L, (size_t)(L >= pay + (d < 0) ? L - pay + d : (uint64_t)(d + 1)), more, variant});
                // the list's order is not the allocations': a shuffle (allocation i is made i-th, handed over perm[i]-th)
                const size_t count = cases.size();
                std::vector<size_t> perm(count);
                for (size_t i = 0; i < count; i++) perm[i] = i;
                for (size_t i = count - 1; i > 0; i--) std::swap(perm[i], perm[next() % (i + 1)]);
                std::vector<Msg> blank(count);
                for (size_t i = 0; i < count; i++) {
                    const Case &c = cases[i];
                    blank[perm[i]] = make_msg(c.L);
                    Msg &g = blank[perm[i]];
                    if (g.bytes) g.p()[flags_at(kind)] = (uint8_t)((g.p()[flags_at(kind)] & ~1u) | (unsigned)c.more);
                }
                std::vector<Case> by_slot(count);
                for (size_t i = 0; i < count; i++) by_slot[perm[i]] = cases[i];
                auto list_of = [&](const std::vector<Msg> &v, std::vector<uint64_t> &addr, std::vector<uint64_t> &len) {
                    addr.assign(count, 0), len.assign(count, 0);  // exactly `count` entries: entry `count` is the sanitizer's
                    addr.shrink_to_fit(), len.shrink_to_fit();
                    for (size_t i = 0; i < count; i++) addr[i] = (uint64_t)(uintptr_t)v[i].p(), len[i] = v[i].L;
                };
                std::vector<uint64_t> addr, len;
                // ---- seal: the wave against the model, message by message ----
                std::vector<Msg> a(count), b(count);
                for (size_t i = 0; i < count; i++) a[i] = clone(blank[i]), b[i] = clone(blank[i]);
                list_of(a, addr, len);
                for (size_t p = 0; p < count; p++) {
                    const uint32_t sa = wave_seal(pk, kind, List{addr.data(), len.data()}, p, pay, hash);
                    const uint32_t sb = naive_seal(m, (int)kind, b[p], pay, hash);
                    CHECK(sa == sb);
                    CHECK(same(a[p], b[p]));
                    CHECK((addr[p] == 0) == (sa == SHORT && len[p] < 16));
                    size_t changed = 0;
                    for (size_t i = 0; a[p].bytes && i < a[p].L; i++) {
                        const size_t at = hdr_hash_at(kind);
                        const bool hdr = i == at || i == at + 1, slot = i >= hash && i < hash + 4;
                        if (!(sa == OK ? hdr || slot : sa == DEFERRED ? hdr : false)) CHECK(a[p].p()[i] == blank[p].p()[i]);
                        changed += a[p].p()[i] != blank[p].p()[i];
                    }
                    CHECK(changed <= (sa == OK ? 6u : sa == DEFERRED ? 2u : 0u));
                    sealed[sa]++;
                }
                // ---- verify: the sealed messages, hashes flipped by the case's variant ----
                std::vector<Msg> recv(count);
                for (size_t p = 0; p < count; p++) {
                    recv[p] = clone(a[p]);
                    const Case &c = by_slot[p];
                    if (c.L >= 16) {
                        if (c.variant & 1) recv[p].p()[hdr_hash_at(kind) + (c.L & 1)] ^= (uint8_t)(1u << (c.L % 8));
                        if ((c.variant & 2) && c.L >= hash + 4) recv[p].p()[hash + c.L % 4] ^= 0x40;
                    }
                }
                std::vector<Msg> recv0(count);
                for (size_t p = 0; p < count; p++) recv0[p] = clone(recv[p]);
                list_of(recv, addr, len);
                for (size_t p = 0; p < count; p++) {
                    const uint32_t va = wave_verify(pk, kind, List{addr.data(), len.data()}, p, pay, hash);
                    CHECK(va == naive_verify(m, (int)kind, recv0[p], pay, hash));
                    CHECK(same(recv[p], recv0[p]));
                    CHECK(va < MISFIT && va != FAULT);
                    const Case &c = by_slot[p];
                    if (!(c.variant & 1) && c.L >= 16) {
                        if (c.more) CHECK(va == DEFERRED);
                        else if (c.L >= pay) CHECK(va == ((c.variant & 2) ? PAYLOAD : OK));
                        // (an eager message shorter than payload_offset was not sealed: its header hash is as it came)
                    }
                    seen[va]++;
                }
                // ---- unpack: the same messages, the destination a table of ranges of R bytes between guards ----
                {
                    std::vector<uint64_t> doff(count + 1);
                    uint64_t at = 3;
                    for (size_t p = 0; p < count; p++) doff[p] = at, at += by_slot[p].R;
                    doff[count] = at;
                    std::vector<uint8_t> da(at + 3, kSentinel), db(at + 3, kSentinel);
                    for (size_t p = 0; p < count; p++) {
                        const uint32_t va = wave_unpack(pk, kind, List{addr.data(), len.data()}, p, pay, hash, da.data(), doff.data());
                        const uint32_t vb = naive_unpack(m, (int)kind, recv0[p], pay, hash, db.data() + doff[p], by_slot[p].R);
                        CHECK(va == vb);
                        CHECK(same(recv[p], recv0[p]));
                        unpacked[va]++;
                        msgs++;
                    }
                    CHECK(da == db);
                }
                // ---- pack: blank messages by list, the sources a table; then the wave's verify reads what it made ----
                {
                    std::vector<uint64_t> soff(count + 1);
                    uint64_t at = 5;
                    for (size_t p = 0; p < count; p++) soff[p] = at, at += by_slot[p].R;
                    soff[count] = at;
                    std::vector<uint8_t> src(at);
                    for (auto &x : src) x = (uint8_t)(next() >> 24);
                    const std::vector<uint8_t> src0 = src;
                    std::vector<Msg> pa(count), pb(count);
                    for (size_t i = 0; i < count; i++) pa[i] = clone(blank[i]), pb[i] = clone(blank[i]);
                    list_of(pa, addr, len);
                    for (size_t p = 0; p < count; p++) {
                        const uint32_t sa = wave_pack(pk, kind, List{addr.data(), len.data()}, p, pay, hash, src.data(), soff.data());
                        const uint32_t sb = naive_pack(m, (int)kind, pb[p], pay, hash, src.data() + soff[p], by_slot[p].R);
                        CHECK(sa == sb);
                        CHECK(same(pa[p], pb[p]));
                        packed[sa]++;
                        if (sa == OK || sa == DEFERRED) CHECK(wave_verify(pk, kind, List{addr.data(), len.data()}, p, pay, hash) == sa);
                    }
                    CHECK(src == src0);
                }
            }
        }
    for (uint32_t k = 0; k < CLASSES; k++) {
        CHECK((seen[k] > 0) == (k != FAULT && k != MISFIT));
        CHECK((unpacked[k] > 0) == (k != FAULT));
    }
    CHECK(sealed[OK] && sealed[DEFERRED] && sealed[SHORT] && !sealed[PAYLOAD] && !sealed[HEADER] && !sealed[FAULT] && !sealed[MISFIT]);
    CHECK(packed[OK] && packed[DEFERRED] && packed[SHORT] && packed[MISFIT] && !packed[PAYLOAD] && !packed[HEADER] && !packed[FAULT]);

    // the empty payload of a message that is not hashed: at address 0 the payload loop's window has no step -- no load
    {
        const GridWindow w(0, 0, 4);
        CHECK(w.K == 0 && w.pad() == 0);
        // ... where the table form's, at the message's end, may have one (why the list form does not run it there)
        CHECK(GridWindow(0x1000 + 37, 0, 4).K == 1);
    }
    // a length that carries a message past the end of the address space is an empty message: SHORT, never read
    {
        mck::RpcHdrPack pk;
        mck::rpc_hdr_pack_build(0x1021, true, 0, 0, 0, &pk);
        const uint64_t addr[1] = {~0ull - 7}, len[1] = {64};
        CHECK(wave_verify(pk, 0, List{addr, len}, 0, 20, 16) == mck::kRpcShort);
        CHECK(wave_seal(pk, 0, List{addr, len}, 0, 20, 16) == mck::kRpcShort);
    }

    // ---- the key space ----
    // Twelve keys carry the list field: the RPC frame's (light, full, non-temporal) x (verify, seal, pack, unpack).
    // With the field clear every count tests/native/launch_plan.cpp pins is what it was: in the payloads frame 35
    // fixed CRC-32C, 21 fixed CRC-64, 2 split, 15 offsets checksum / verify / update and 9 seal / pack / unpack;
    // 0 in place, 6 detached, 12 RPC; none with mode 3 or a frame past the last.
    int n_list = 0, n[5] = {0, 0, 0, 0, 0}, nf[mck::kFrameRpc + 2] = {0, 0, 0, 0, 0};
    for (int list = 0; list < 2; list++)
        for (int frame = -1; frame <= mck::kFrameRpc + 1; frame++)
            for (int width : {16, 32, 64})
                for (int lg = -1; lg <= CRC_GPU_MAX_LOG2G + 1; lg++)
                    for (int mode = -1; mode <= kOffsets + 1; mode++)
                        for (int op = -1; op <= mck::kOpUnpack + 1; op++)
                            for (int f = 0; f < 8; f++) {
                                const mck::KernelKey k{width, lg, mode, op, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (mck::MsgFrame)frame, list != 0};
                                if (!mck::kernel_key_valid(k)) continue;
                                CHECK(frame >= 0 && frame <= mck::kFrameRpc && mode >= 0 && mode <= kOffsets);
                                if (!list) {
                                    if (frame == mck::kFramePayloads)
                                        n[k.split ? 2 : mode != kOffsets ? (width == 64) : op <= mck::kOpUpdate ? 3 : 4]++;
                                    else
                                        nf[frame]++;
                                    continue;
                                }
                                n_list++;
                                CHECK(frame == mck::kFrameRpc && width == 32 && mode == kOffsets && lg == CRC_GPU_MAX_LOG2G);
                                CHECK(op == mck::kOpVerify || op == mck::kOpSeal || op == mck::kOpPack || op == mck::kOpUnpack);
                                CHECK(!k.split && !(k.nt && k.light));
                                mck::KernelKey table = k;
                                table.list = false;
                                CHECK(mck::kernel_key_valid(table) && !(table == k));  // a twin of a table kernel, and another key
                            }
    CHECK(n_list == 12);
    CHECK(n[0] == 35 && n[1] == 21 && n[2] == 2 && n[3] == 15 && n[4] == 9);
    CHECK(nf[mck::kFrameInPlace] == 0 && nf[mck::kFrameDetached] == 6 && nf[mck::kFrameRpc] == 12 && nf[mck::kFrameRpc + 1] == 0);
    CHECK((!mck::KernelKey{32, 6, kOffsets, mck::kOpVerify, false, false, false, mck::kFrameRpc}.list));  // the default: a table
    // the plan is the table form's for the same count, and kernel_key carries the field
    const mck_settings_t s = [] {
        mck_settings_t v{};
        v.gpu_light = v.gpu_nt = v.gpu_log2g = v.gpu_split = v.gpu_xdr_fast = -1;  // nothing set: the library decides
        v.gpu_split_lds = 1;
        return v;
    }();
    for (size_t count : {1u, 1024u, 1025u, 8191u, 8192u}) {
        const mck::LaunchPlan p = mck::plan_offsets(s, 256, 32, count);
        for (int op : {mck::kOpVerify, mck::kOpSeal, mck::kOpPack, mck::kOpUnpack}) {
            const mck::KernelKey t = mck::kernel_key(p, (mck::BatchOp)op, mck::kFrameRpc);
            const mck::KernelKey l = mck::kernel_key(p, (mck::BatchOp)op, mck::kFrameRpc, true);
            CHECK(!t.list && l.list && mck::kernel_key_valid(l));
            mck::KernelKey u = l;
            u.list = false;
            CHECK(u == t);
            CHECK(l.light == (count <= 1024) && l.nt == (count >= 8192));
        }
        CHECK(p.dyn == (count > 1024));  // the queue from 1,025 messages on: what tests/test_gpu_rpc_list.py relies on
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpChecksum, mck::kFramePayloads, true)));
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpVerify, mck::kFrameDetached, true)));
        CHECK(!mck::kernel_key_valid(mck::kernel_key(p, mck::kOpVerify, mck::kFrameInPlace, true)));
    }

    // ---- the host front's call shape (offsets_call.h) ----
    {
        uint64_t tab[2] = {0, 0}, lens[1] = {0};
        uint8_t buf[1] = {0};
        for (int op : {mck::kOpVerify, mck::kOpSeal, mck::kOpUnpack, mck::kOpPack}) {
            const bool pack = op == mck::kOpPack, copy = pack || op == mck::kOpUnpack;
            mck::OffsetsCall c{(mck::BatchOp)op, "crc32c", pack ? buf : nullptr, tab, 1};
            c.frame = mck::kFrameRpc;
            c.list = true;
            c.msg_len = lens;
            if (copy) c.dst_off = tab;
            if (op == mck::kOpUnpack) c.dst = buf;
            CHECK(!mck::offsets_lacks_pointer(c));  // no buffer under the list, no `out` of a seal
            mck::OffsetsCall d = c;
            d.msg_len = nullptr;
            CHECK(mck::offsets_lacks_pointer(d));
            d = c;
            (pack ? d.dst_off : d.src_off) = nullptr;
            CHECK(mck::offsets_lacks_pointer(d));
            if (copy) {
                d = c;
                (pack ? d.src_off : d.dst_off) = nullptr;
                CHECK(mck::offsets_lacks_pointer(d));
                d = c;
                if (pack) d.src = nullptr;
                else d.dst = nullptr;
                CHECK(mck::offsets_lacks_pointer(d));
            }
            d = c;
            d.count = 0, d.src = nullptr, d.src_off = nullptr, d.dst = nullptr, d.dst_off = nullptr, d.msg_len = nullptr;
            CHECK(!mck::offsets_lacks_pointer(d));
            // the kernels' argument: the lengths ride in `stride`, and the list's side has a null buffer whatever the call holds
            c.src = pack ? (const void *)buf : (const void *)buf, c.dst = buf, c.out = buf;
            const BatchArgs a = mck::batch_args_of(c, nullptr, nullptr, nullptr, false, nullptr);
            CHECK(a.rpc_list_len() == lens && a.stride == (uint64_t)(uintptr_t)lens);
            if (pack) CHECK(a.copy_dst == nullptr && a.base == buf && a.dst_offsets == tab);
            else CHECK(a.base == nullptr && a.offsets == tab);
            if (op == mck::kOpSeal) CHECK(a.msgs == nullptr);
            if (op == mck::kOpUnpack) CHECK(a.copy_dst == buf);
            // the table form is what it was
            mck::OffsetsCall t{(mck::BatchOp)op, "crc32c", buf, tab, 1};
            t.frame = mck::kFrameRpc;
            CHECK(mck::batch_args_of(t, nullptr, nullptr, nullptr, false, nullptr).stride == 0);
            CHECK(mck::offsets_needs((mck::BatchOp)op, mck::kFrameRpc).src_buf && mck::offsets_needs((mck::BatchOp)op, mck::kFrameRpc).dst_buf &&
                  !mck::offsets_needs((mck::BatchOp)op, mck::kFrameRpc).msg_len);
        }
    }

    std::printf("%llu messages: ok %llu payload %llu header %llu short %llu deferred %llu misfit %llu\n", msgs, unpacked[OK],
                unpacked[PAYLOAD], unpacked[HEADER], unpacked[SHORT], unpacked[DEFERRED], unpacked[MISFIT]);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
