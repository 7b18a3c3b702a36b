// The frame of the RPC message calls of an XDR build by address list
// (mercury_amd/csrc/launch_plan.h: rpc_xdr_list_len, rpc_xdr_list_at, around
// the table form's ladders and gates rpc_xdr_walks, rpc_xdr_*_class,
// rpc_xdr_unpacks, rpc_xdr_packs) against a model written here from the
// contract alone (include/mchecksum_gpu.h: mchecksum_gpu_verify_rpc_xdr_message_list
// and its three siblings).  `lanes_*` do what a wave does (mchecksum_gpu_ext.hip:
// xdr_message / xdr_pack_message with an RPC operation and LIST) with the same
// functions in the kernel's order: the entry, its frame, the header's sixteen
// bytes, the gate, the pre-walk, the walk, the class.
//
// Every byte of a message goes through a checked accessor (Space): list entry
// (addr, len) names bytes of a simulated address space, and before the lanes
// run the MODEL says which of them the contract lets this call read and which
// write for the class the model found --
//   L < 16, an end past the address space among them:  none; the address forms
//                                                      no pointer, it may be 0
//   DEFERRED, or eager and shorter than payload_offset: the 16 header bytes
//   pack, rejected before the walk (MISFIT):            the 16 header bytes
//   else:                                               the message's L bytes
//   written: the 2 CRC-16 bytes (DEFERRED); they and the 4 hash bytes (seal
//   OK); they and everything from payload_offset on (pack OK); else nothing
// -- and a read or a write outside them aborts the program.  (This form's
// reads beyond the message, in the throughput layout's 16-byte pieces behind a
// field of >= 256 bytes, enter no verdict and are not modelled here.)
//
// Schema and cases as in rpc_xdr_msg.cpp: INT 4 (n) then OPAQUE_LEN; both
// kinds; L = 0, 15, 16, payload_offset - 1, payload_offset .. + 20; n = 0, 1,
// 3, 4, 5, 8; MORE_DATA set and clear; each hash right and wrong; the other
// range one byte short, exact, one long, alone in an exactly sized allocation.
// Entries lie at odd addresses, at NULL (L < 16), and with addr + len past
// the end of the address space (a message of no bytes, whatever len says).
// Stand-alone: plain and under the sanitizers (tests/test_rpc_xdr_list_msg.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "launch_plan.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (g_fail++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                               \
    } while (0)

struct Model16 {
    uint32_t poly;
    bool reflected;
    uint32_t init, xorout;
};
const Model16 kModels[] = {{0x1021, true, 0x0000, 0x0000}, {0x1021, false, 0xFFFF, 0xFFFF}};
enum : uint32_t { OK = 0, PAYLOAD, HEADER, SHORT, DEFERRED, FAULT, MISFIT, CLASSES };
const uint8_t kSentinel = 0xA5;
typedef std::vector<uint8_t> Bytes;

// ---- the simulated address space: one message, and what of it may be touched ----
struct Space {
    uint64_t base = 0;  // address of bytes[0]
    Bytes bytes;
    uint64_t read_lo = 0, read_hi = 0;                    // [lo, hi): what the contract lets the call read
    std::vector<std::pair<uint64_t, uint64_t>> writes;    // and write
    unsigned long long reads = 0;
    bool inside(uint64_t a) const { return a >= base && a - base < bytes.size(); }
    uint8_t rd(uint64_t a) {
        if (!(a >= read_lo && a < read_hi && inside(a))) {
            std::printf("ABORT: read of address %#llx outside [%#llx, %#llx)\n", (unsigned long long)a,
                        (unsigned long long)read_lo, (unsigned long long)read_hi);
            std::abort();
        }
        reads++;
        return bytes[a - base];
    }
    void wr(uint64_t a, uint8_t v) {
        bool ok = false;
        for (const auto &w : writes) ok = ok || (a >= w.first && a < w.second);
        if (!ok || !inside(a)) {
            std::printf("ABORT: write of address %#llx outside the bytes the call may write\n", (unsigned long long)a);
            std::abort();
        }
        bytes[a - base] = v;
    }
};

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
        img[0] = h[0];
        img[1] = h[1];
        for (int b = 0; b < 8; b++) img[2 + b] = h[9 - b];  // the id: big-endian on the wire, a little-endian host's value
        img[10] = h[10];
        img[11] = h[11];
        return naive_crc16(m, img, 12);
    }
    img[0] = h[0];
    img[1] = h[1];
    img[2] = h[3];  // the cookie
    img[3] = h[2];
    return naive_crc16(m, img, 4);
}
size_t flags_at(int kind) { return kind == 0 ? 10 : 1; }
size_t hdr_hash_at(int kind) { return kind == 0 ? 12 : 4; }
void put_hdr_crc(const Model16 &m, int kind, Bytes &msg) {
    const uint32_t c = naive_hdr_crc(m, kind, msg.data());
    msg[hdr_hash_at(kind)] = (uint8_t)(c >> 8);
    msg[hdr_hash_at(kind) + 1] = (uint8_t)c;
}
uint32_t get_be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
void put_be32(uint8_t *p, uint32_t v) {
    for (int b = 0; b < 4; b++) p[b] = (uint8_t)(v >> (24 - 8 * b));
}
// The list entry's message: `len` bytes at `addr`, none when the end would pass the end of the address space.
// (the end, addr + len, is an address: a message may end at ~0 at the latest)
uint64_t naive_len(uint64_t addr, uint64_t len) { return len > ~0ull - addr ? 0 : len; }
bool naive_decode(const uint8_t *x, size_t avail, Bytes *image) {
    image->clear();
    if (avail < 4) return false;
    const uint32_t n = get_be32(x);
    if ((uint64_t)((n + 3ull) & ~3ull) > avail - 4) return false;
    for (int b = 0; b < 4; b++) image->push_back((uint8_t)(n >> (8 * b)));
    for (uint32_t i = 0; i < n; i++) image->push_back(x[4 + i]);
    return true;
}
bool naive_encode(const Bytes &image, Bytes *x) {
    x->clear();
    if (image.size() < 4) return false;
    const uint32_t n = (uint32_t)image[0] | (uint32_t)image[1] << 8 | (uint32_t)image[2] << 16 | (uint32_t)image[3] << 24;
    if (image.size() - 4 != n) return false;
    for (int b = 0; b < 4; b++) x->push_back((uint8_t)(n >> (24 - 8 * b)));
    for (uint32_t i = 0; i < n; i++) x->push_back(image[4 + i]);
    while (x->size() % 4) x->push_back(0);
    return true;
}
// The four ladders over the message's bytes (msg.size() is L), as the header words them.
uint32_t naive_verify(const Model16 &m, int kind, const Bytes &msg, size_t pay, size_t hash, const size_t *R = nullptr,
                      Bytes *dst = nullptr) {
    const size_t L = msg.size();
    const bool more = L >= 16 && (msg[flags_at(kind)] & 1);
    Bytes image;
    const bool fits = L >= 16 && !more && L >= pay && naive_decode(msg.data() + pay, L - pay, &image);
    if (R && fits && image.size() == *R) *dst = image;  // what is written does not wait for the verdicts
    if (L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (naive_hdr_crc(m, kind, msg.data()) != (uint32_t)(msg[at] << 8 | msg[at + 1])) return HEADER;
    if (more) return DEFERRED;
    if (L < pay || !fits) return SHORT;
    if (R && image.size() != *R) return MISFIT;
    return naive_crc32c(image.data(), image.size()) == get_be32(msg.data() + hash) ? OK : PAYLOAD;
}
uint32_t naive_seal(const Model16 &m, int kind, Bytes &msg, size_t pay, size_t hash) {
    const size_t L = msg.size();
    if (L < 16) return SHORT;
    if (msg[flags_at(kind)] & 1) {
        put_hdr_crc(m, kind, msg);
        return DEFERRED;
    }
    Bytes image;
    if (L < pay || !naive_decode(msg.data() + pay, L - pay, &image)) return SHORT;
    put_be32(msg.data() + hash, naive_crc32c(image.data(), image.size()));
    put_hdr_crc(m, kind, msg);
    return OK;
}
uint32_t naive_pack(const Model16 &m, int kind, Bytes &msg, size_t pay, size_t hash, const Bytes &image) {
    const size_t L = msg.size();
    if (L < 16) return SHORT;
    if (msg[flags_at(kind)] & 1) {
        put_hdr_crc(m, kind, msg);
        return DEFERRED;
    }
    if (L < pay) return SHORT;
    Bytes x;
    if (!naive_encode(image, &x) || L != pay + x.size()) return MISFIT;
    std::memcpy(msg.data() + pay, x.data(), x.size());
    put_be32(msg.data() + hash, naive_crc32c(image.data(), image.size()));
    put_hdr_crc(m, kind, msg);
    return OK;
}
// What the contract lets a call read of the message at addr whose bytes are `msg` (L = msg.size()): the "Reads"
// paragraph.  header_only: pack's message rejected before the walk.
void allow_reads(Space &sp, uint64_t addr, const Bytes &msg, int kind, size_t pay, bool header_only = false) {
    const size_t L = msg.size();
    sp.read_lo = sp.read_hi = 0;
    sp.writes.clear();
    sp.reads = 0;
    if (L < 16) return;  // never dereferenced
    const bool more = msg[flags_at(kind)] & 1;
    sp.read_lo = addr;
    sp.read_hi = addr + (more || L < pay || header_only ? 16 : L);
}

// ---- what a wave does, with launch_plan.h's functions, every message byte through the accessor ----
struct Frame {
    uint64_t at, L;
};
Frame lanes_frame(uint64_t addr, uint64_t len) { return Frame{mck::rpc_xdr_list_at(addr, len), mck::rpc_xdr_list_len(addr, len)}; }
struct Front {
    bool more = false;
    uint32_t crc16 = 0, wire = 0;
};
Front lanes_front(Space &sp, const mck::RpcHdrPack &pk, uint32_t kind, uint64_t at, uint64_t L) {
    Front r;
    const bool whole = L >= mck::kRpcHdrBytes;
    uint32_t hb[16] = {0}, term[16] = {0};
    for (uint32_t lane = 0; lane < 16; lane++)
        if (whole) hb[lane] = sp.rd(at + lane);
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
uint32_t rd_be32(Space &sp, uint64_t a) {
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) v = v << 8 | sp.rd(a + b);
    return v;
}
void wr_be32(Space &sp, uint64_t a, uint32_t v) {
    for (int b = 0; b < 4; b++) sp.wr(a + b, (uint8_t)(v >> (24 - 8 * b)));
}
void store_crc16(Space &sp, uint64_t at, uint32_t kind, uint32_t crc16) {
    sp.wr(at + mck::rpc_hash_at(kind), (uint8_t)(crc16 >> 8));
    sp.wr(at + mck::rpc_hash_at(kind) + 1, (uint8_t)crc16);
}
// xdr_decoded_len of the schema over [pos, end): the INT field only, with the walk's bounds tests
bool pre_decoded_len(Space &sp, uint64_t pos, uint64_t end, uint64_t *n) {
    if (end - pos < 4) return false;
    const uint64_t len = rd_be32(sp, pos);
    if (len > end - pos - 4 || ((len + 3) & ~3ull) > end - pos - 4) return false;
    *n = 4 + len;
    return true;
}
// the walk over [pos, end): hashes the decoded stream, stores it at d when d is not null; false: it ran past the message
bool walk(Space &sp, uint64_t pos, uint64_t end, uint8_t *d, uint32_t *crc) {
    if (end - pos < 4) return false;
    const uint32_t len = rd_be32(sp, pos);
    if (len > end - pos - 4 || (((uint64_t)len + 3) & ~3ull) > end - pos - 4) return false;
    Bytes stream;
    for (int b = 0; b < 4; b++) stream.push_back((uint8_t)(len >> (8 * b)));
    for (uint32_t i = 0; i < len; i++) stream.push_back(sp.rd(pos + 4 + i));
    if (d) std::memcpy(d, stream.data(), stream.size());
    *crc = naive_crc32c(stream.data(), stream.size());
    return true;
}
uint32_t lanes_verify(Space &sp, const mck::RpcHdrPack &pk, uint32_t kind, uint64_t addr, uint64_t len, uint64_t pay, uint64_t hash) {
    const Frame fr = lanes_frame(addr, len);
    const uint64_t pos = fr.at, end = fr.at + fr.L, L = fr.L;
    const Front f = lanes_front(sp, pk, kind, pos, L);
    bool bad = !mck::rpc_xdr_walks(L, f.more, pay);
    uint32_t crc = 0;
    if (!bad) bad = !walk(sp, pos + pay, end, nullptr, &crc);
    const bool pay_ok = !bad && rd_be32(sp, pos + hash) == crc;
    return mck::rpc_xdr_verify_class(L, f.crc16 == f.wire, f.more, pay, !bad, pay_ok);
}
uint32_t lanes_seal(Space &sp, const mck::RpcHdrPack &pk, uint32_t kind, uint64_t addr, uint64_t len, uint64_t pay, uint64_t hash) {
    const Frame fr = lanes_frame(addr, len);
    const uint64_t pos = fr.at, end = fr.at + fr.L, L = fr.L;
    const Front f = lanes_front(sp, pk, kind, pos, L);
    bool bad = !mck::rpc_xdr_walks(L, f.more, pay);
    uint32_t crc = 0;
    if (!bad) bad = !walk(sp, pos + pay, end, nullptr, &crc);
    const uint32_t cls = mck::rpc_xdr_seal_class(L, f.more, pay, !bad);
    if (cls == mck::kRpcOk) wr_be32(sp, pos + hash, crc);
    if (cls != mck::kRpcShort) store_crc16(sp, pos, kind, f.crc16);
    return cls;
}
uint32_t lanes_unpack(Space &sp, const mck::RpcHdrPack &pk, uint32_t kind, uint64_t addr, uint64_t len, uint64_t pay, uint64_t hash,
                      uint8_t *dst, uint64_t d0, uint64_t d1) {
    const Frame fr = lanes_frame(addr, len);
    const uint64_t pos = fr.at, end = fr.at + fr.L, L = fr.L, R = mck::rpc_len(d0, d1);
    const Front f = lanes_front(sp, pk, kind, pos, L);
    bool bad = !mck::rpc_xdr_walks(L, f.more, pay);
    uint64_t decoded = 0;
    bool fits = !bad && pre_decoded_len(sp, pos + pay, end, &decoded);
    bad = !mck::rpc_xdr_unpacks(L, f.more, pay, fits, decoded, R);
    const bool walked = !bad;
    uint32_t crc = 0;
    if (!bad) bad = !walk(sp, pos + pay, end, dst, &crc);
    fits = fits && !(walked && bad);
    const bool pay_ok = !bad && rd_be32(sp, pos + hash) == crc;
    return mck::rpc_xdr_unpack_class(L, f.crc16 == f.wire, f.more, pay, fits, decoded, R, pay_ok);
}
uint32_t lanes_pack(Space &sp, const mck::RpcHdrPack &pk, uint32_t kind, uint64_t addr, uint64_t len, uint64_t pay, uint64_t hash,
                    const uint8_t *src, uint64_t s0, uint64_t s1) {
    const Frame fr = lanes_frame(addr, len);
    const uint64_t pos = fr.at, L = fr.L, R = mck::rpc_len(s0, s1);
    const Front f = lanes_front(sp, pk, kind, pos, L);
    uint64_t encoded = 0;
    bool exact = false;
    if (mck::rpc_hashes_payload(L, f.more, pay) && R >= 4) {  // xdr_encoded_len: the image's INT field only
        const uint64_t n = (uint64_t)src[0] | (uint64_t)src[1] << 8 | (uint64_t)src[2] << 16 | (uint64_t)src[3] << 24;
        exact = n == R - 4;
        encoded = 4 + ((n + 3) & ~3ull);
    }
    uint32_t crc = 0;
    if (mck::rpc_xdr_packs(L, f.more, pay, exact, encoded)) {
        const uint64_t n = R - 4;
        wr_be32(sp, pos + pay, (uint32_t)n);
        for (uint64_t i = 0; i < n; i++) sp.wr(pos + pay + 4 + i, src[4 + i]);
        for (uint64_t i = 4 + n; i < encoded; i++) sp.wr(pos + pay + i, 0);
        crc = naive_crc32c(src, R);
    }
    const uint32_t cls = mck::rpc_xdr_pack_class(L, f.more, pay, exact, encoded);
    if (cls == mck::kRpcOk) wr_be32(sp, pos + hash, crc);
    if (cls == mck::kRpcOk || cls == mck::kRpcDeferred) store_crc16(sp, pos, kind, f.crc16);
    return cls;
}

}  // namespace

int main() {
    static_assert(mck::kRpcMisfit == MISFIT && mck::kRpcCopyClasses == CLASSES && mck::kRpcClasses == 6, "the classes");
    const uint64_t shapes[][2] = {{20, 16}, {23, 17}};  // payload_offset, hash_offset
    const uint32_t lens[] = {0, 1, 3, 4, 5, 8};
    unsigned long long seen[CLASSES] = {0}, unpacked[CLASSES] = {0}, sealed[CLASSES] = {0}, packed[CLASSES] = {0}, msgs = 0;
    unsigned long long nulls = 0, wraps = 0, at_zero = 0, hdr_only = 0;
    uint32_t rng = 20261021;
    auto next = [&] { return rng = rng * 1664525u + 1013904223u; };
    for (const Model16 &m : kModels)
        for (uint32_t kind = 0; kind < 2; kind++) {
            mck::RpcHdrPack pk;
            mck::rpc_hdr_pack_build(m.poly, m.reflected, m.init, m.xorout, kind, &pk);
            for (const auto &sh : shapes) {
                const uint64_t pay = sh[0], hash = sh[1];
                std::vector<uint64_t> Ls = {0, 15, 16, pay - 1};
                for (uint64_t L = pay; L <= pay + 20; L++) Ls.push_back(L);
                for (uint64_t L0 : Ls)
                    for (uint32_t n : lens)
                        for (int more = 0; more < 2; more++)
                            for (int variant = 0; variant < 4; variant++)   // bit 0: header hash wrong, bit 1: payload hash wrong
                                for (int place = 0; place < 3; place++) {  // 0: an odd address, 1: NULL, 2: the end wraps
                                    if (place == 1 && L0 >= 16) continue;  // (only a message without a header may be NULL)
                                    Bytes blank(L0);
                                    for (auto &b : blank) b = (uint8_t)(next() >> 24);
                                    if (L0 > flags_at(kind)) blank[flags_at(kind)] = (uint8_t)((blank[flags_at(kind)] & ~1u) | (unsigned)more);
                                    if (L0 >= pay + 4) put_be32(blank.data() + pay, n);
                                    // the entry: `len` bytes at `addr`; the bytes the model sees are what the entry holds
                                    uint64_t addr = 0x7F3A00001003ull + (next() >> 28), len = L0;
                                    if (place == 1) addr = 0;
                                    if (place == 2) addr = ~0ull - L0 / 2, len = L0 + 2;  // the end would pass ~0
                                    const uint64_t Lm = naive_len(addr, len);
                                    if (place == 2) {
                                        CHECK(Lm == 0);
                                        blank.clear();
                                    } else {
                                        CHECK(Lm == L0);
                                    }
                                    nulls += place == 1;
                                    wraps += place == 2;
                                    // the frame: L by the list rule, and an address of 0 exactly when no byte is read
                                    CHECK(mck::rpc_xdr_list_len(addr, len) == Lm);
                                    CHECK((mck::rpc_xdr_list_at(addr, len) == 0) == (Lm < 16 || addr == 0));
                                    if (Lm >= 16) CHECK(mck::rpc_xdr_list_at(addr, len) == addr);
                                    at_zero += mck::rpc_xdr_list_at(addr, len) == 0;
                                    const uint64_t need = 4 + ((n + 3ull) & ~3ull);
                                    Space sp;
                                    sp.base = addr;
                                    // ---- seal ----
                                    Bytes b = blank;
                                    const uint32_t sb = naive_seal(m, (int)kind, b, pay, hash);
                                    sp.bytes = blank;
                                    allow_reads(sp, addr, blank, (int)kind, pay);
                                    const uint64_t hat = addr + hdr_hash_at(kind);
                                    if (sb != SHORT) sp.writes.push_back({hat, hat + 2});
                                    if (sb == OK) sp.writes.push_back({addr + hash, addr + hash + 4});
                                    const uint32_t sa = lanes_seal(sp, pk, kind, addr, len, pay, hash);
                                    CHECK(sa == sb && sp.bytes == b);
                                    if (Lm < 16) CHECK(sp.reads == 0);
                                    sealed[sa]++;
                                    // ---- verify: a message sealed by the model, then corrupted by the variant ----
                                    Bytes msg = b;
                                    if (Lm >= 16) {
                                        if (sb == SHORT) put_hdr_crc(m, (int)kind, msg);  // (a short eager message with a good header)
                                        if (variant & 1) msg[hdr_hash_at(kind) + (Lm & 1)] ^= (uint8_t)(1u << (Lm % 8));
                                        if ((variant & 2) && Lm >= hash + 4) msg[hash + Lm % 4] ^= 0x40;
                                    }
                                    sp.bytes = msg;
                                    allow_reads(sp, addr, msg, (int)kind, pay);
                                    hdr_only += sp.read_hi - sp.read_lo == 16 && Lm > 16;
                                    const uint32_t va = lanes_verify(sp, pk, kind, addr, len, pay, hash);
                                    CHECK(va == naive_verify(m, (int)kind, msg, pay, hash));
                                    CHECK(sp.bytes == msg && va < mck::kRpcClasses && va != FAULT);
                                    if (Lm < 16) CHECK(sp.reads == 0 && va == SHORT);
                                    seen[va]++;
                                    msgs++;
                                    // ---- unpack: R = decoded - 1, decoded, decoded + 1 ----
                                    for (int d = -1; d <= 1; d++) {
                                        const size_t R = 4 + n + d;
                                        Bytes da(R, kSentinel), db(R, kSentinel);
                                        allow_reads(sp, addr, msg, (int)kind, pay);
                                        const uint32_t ua = lanes_unpack(sp, pk, kind, addr, len, pay, hash, da.data(), 11, 11 + R);
                                        CHECK(ua == naive_verify(m, (int)kind, msg, pay, hash, &R, &db));
                                        CHECK(da == db && sp.bytes == msg);
                                        if (va != OK && va != PAYLOAD) CHECK(ua == va && (ua == HEADER || da == Bytes(R, kSentinel)));
                                        else CHECK(ua == (d ? (uint32_t)MISFIT : va));
                                        unpacked[ua]++;
                                    }
                                    // ---- pack: image one byte short, exact, one long ----
                                    for (int d = -1; d <= 1; d++) {
                                        Bytes image(4 + n + d);
                                        for (auto &q : image) q = (uint8_t)(next() >> 24);
                                        for (size_t q = 0; q < 4 && q < image.size(); q++) image[q] = (uint8_t)(n >> (8 * q));
                                        const Bytes image0 = image;
                                        Bytes pb = blank;
                                        const uint32_t qb = naive_pack(m, (int)kind, pb, pay, hash, image);
                                        sp.bytes = blank;
                                        allow_reads(sp, addr, blank, (int)kind, pay, true);  // a pack reads the header alone
                                        if (qb == OK || qb == DEFERRED) sp.writes.push_back({hat, hat + 2});
                                        if (qb == OK) {
                                            sp.writes.push_back({addr + hash, addr + hash + 4});
                                            sp.writes.push_back({addr + pay, addr + Lm});
                                        }
                                        const uint32_t qa = lanes_pack(sp, pk, kind, addr, len, pay, hash, image.data(), 3, 3 + image.size());
                                        CHECK(qa == qb && sp.bytes == pb && image == image0);
                                        if (Lm >= 16 && !more && Lm >= pay) CHECK((qa == OK) == (d == 0 && Lm == pay + need));
                                        packed[qa]++;
                                    }
                                }
            }
        }
    for (uint32_t k = 0; k < mck::kRpcClasses; k++) CHECK((seen[k] >= 100) == (k != FAULT));  // every verdict, not vacuously
    for (uint32_t k = 0; k < CLASSES; k++) CHECK((unpacked[k] >= 100) == (k != FAULT));
    CHECK(sealed[OK] && sealed[DEFERRED] && sealed[SHORT] && !sealed[PAYLOAD] && !sealed[HEADER] && !sealed[FAULT] && !sealed[MISFIT]);
    CHECK(packed[OK] && packed[DEFERRED] && packed[SHORT] && packed[MISFIT] && !packed[PAYLOAD] && !packed[HEADER] && !packed[FAULT]);
    CHECK(nulls >= 100 && wraps >= 100 && at_zero >= nulls + wraps && hdr_only >= 100);
    // the frame's edges, one by one
    CHECK(mck::rpc_xdr_list_len(0x1000, 15) == 15 && mck::rpc_xdr_list_at(0x1000, 15) == 0);
    CHECK(mck::rpc_xdr_list_len(0x1000, 16) == 16 && mck::rpc_xdr_list_at(0x1000, 16) == 0x1000);
    CHECK(mck::rpc_xdr_list_len(0, 0) == 0 && mck::rpc_xdr_list_at(0, 0) == 0 && mck::rpc_xdr_list_at(0, 15) == 0);
    CHECK(mck::rpc_xdr_list_len(~0ull - 15, 16) == 0 && mck::rpc_xdr_list_at(~0ull - 15, 16) == 0);  // the end would be 2^64
    CHECK(mck::rpc_xdr_list_len(~0ull - 16, 16) == 16 && mck::rpc_xdr_list_at(~0ull - 16, 16) == ~0ull - 16);
    CHECK(mck::rpc_xdr_list_len(0x1000, ~0ull) == 0 && mck::rpc_xdr_list_at(0x1000, ~0ull) == 0);
    CHECK(mck::rpc_xdr_list_len(0x1000, (1ull << 33) + 20) == (1ull << 33) + 20);  // sizes past 2^32 are not truncated
    // the FAULT value is no rule's verdict: only a launch that gave up a wait writes it (xdr_flag_kernel)
    std::printf("%llu messages: ok %llu payload %llu header %llu short %llu deferred %llu; unpack misfit %llu; "
                "null %llu wrapped %llu header-only %llu\n",
                msgs, seen[OK], seen[PAYLOAD], seen[HEADER], seen[SHORT], seen[DEFERRED], unpacked[MISFIT], nulls, wraps, hdr_only);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
