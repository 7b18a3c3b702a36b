// The rules of the RPC message calls of an XDR build (mercury_amd/csrc/
// launch_plan.h: rpc_xdr_walks, rpc_xdr_verify_class, rpc_xdr_seal_class,
// rpc_xdr_unpacks, rpc_xdr_unpack_class, rpc_xdr_packs, rpc_xdr_pack_class,
// with the header pack's per-byte terms) against a model written here from
// the contract alone (include/mchecksum_gpu.h: mchecksum_gpu_verify_rpc_xdr_messages
// and its three siblings): the field image assembled field by field, both CRCs
// bit by bit, the four ladders as the header words them, and what each call
// writes.  `lanes_*` below do what a wave does (mchecksum_gpu_ext.hip:
// xdr_message / xdr_pack_message with an RPC operation) with the same
// functions, on host memory, in the kernel's order: the header's sixteen
// bytes, the frame's test, the pre-walk, the walk, the class.
//
// The schema is hg_string_t's shape without its flags: INT 4 (n), then
// OPAQUE_LEN -- on the wire 4 big-endian bytes, n bytes and a zero pad to a
// multiple of 4; decoded, 4 little-endian bytes and the n bytes.  Both kinds;
// L = 0 .. payload_offset + 20 with n = 0, 1, 3, 4, 5, 8 (so the schema ends
// one byte past the message, at its end, and with slack); R = decoded - 1, =,
// + 1; image one byte short, exact, one byte long; (payload_offset,
// hash_offset) = (20, 16), (24, 16), (21, 17); MORE_DATA set and clear;
// header hash and payload hash right and wrong.  Every message, destination
// and image sits alone in an exactly sized allocation, so a byte read or
// written past an end -- behind the core header of a message that must not be
// walked, in the range of a message that must not be copied -- is the
// sanitizer's.  Stand-alone: plain and under the sanitizers
// (tests/test_rpc_xdr_msg.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    const char *name;
    uint32_t poly;
    bool reflected;
    uint32_t init, xorout;
};
const Model16 kModels[] = {
    {"crc16-kermit", 0x1021, true, 0x0000, 0x0000},
    {"crc16-ibm-3740", 0x1021, false, 0xFFFF, 0x0000},
    {"crc16-genibus", 0x1021, false, 0xFFFF, 0xFFFF},
};
enum : uint32_t { OK = 0, PAYLOAD, HEADER, SHORT, DEFERRED, FAULT, MISFIT, CLASSES };
const uint8_t kSentinel = 0xA5;
typedef std::vector<uint8_t> Bytes;

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
void put_hdr_crc(const Model16 &m, int kind, Bytes &msg) {
    const uint32_t c = naive_hdr_crc(m, kind, msg.data());
    msg[hdr_hash_at(kind)] = (uint8_t)(c >> 8);
    msg[hdr_hash_at(kind) + 1] = (uint8_t)c;
}
uint32_t get_be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
void put_be32(uint8_t *p, uint32_t v) {
    for (int b = 0; b < 4; b++) p[b] = (uint8_t)(v >> (24 - 8 * b));
}

// The XDR bytes [0, avail) decoded by the schema: false when it runs past them; bytes behind its end are ignored.
bool naive_decode(const uint8_t *x, size_t avail, Bytes *image) {
    image->clear();
    if (avail < 4) return false;
    const uint32_t n = get_be32(x);
    if ((uint64_t)((n + 3ull) & ~3ull) > avail - 4) return false;
    for (int b = 0; b < 4; b++) image->push_back((uint8_t)(n >> (8 * b)));
    for (uint32_t i = 0; i < n; i++) image->push_back(x[4 + i]);
    return true;
}
// The image encoded: false when the schema does not consume it exactly.
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

uint32_t naive_verify(const Model16 &m, int kind, const Bytes &msg, size_t pay, size_t hash) {
    const size_t L = msg.size();
    if (L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (naive_hdr_crc(m, kind, msg.data()) != (uint32_t)(msg[at] << 8 | msg[at + 1])) return HEADER;
    if (msg[flags_at(kind)] & 1) return DEFERRED;
    if (L < pay) return SHORT;
    Bytes image;
    if (!naive_decode(msg.data() + pay, L - pay, &image)) return SHORT;
    return naive_crc32c(image.data(), image.size()) == get_be32(msg.data() + hash) ? OK : PAYLOAD;
}
uint32_t naive_unpack(const Model16 &m, int kind, const Bytes &msg, size_t pay, size_t hash, Bytes &dst) {
    const size_t L = msg.size(), R = dst.size();
    const bool more = L >= 16 && (msg[flags_at(kind)] & 1);
    Bytes image;
    const bool fits = L >= 16 && !more && L >= pay && naive_decode(msg.data() + pay, L - pay, &image);
    if (fits && image.size() == R) dst = image;  // what is written does not wait for the verdicts
    if (L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (naive_hdr_crc(m, kind, msg.data()) != (uint32_t)(msg[at] << 8 | msg[at + 1])) return HEADER;
    if (more) return DEFERRED;
    if (L < pay || !fits) return SHORT;
    if (image.size() != R) return MISFIT;
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

// ---- what a wave does, with launch_plan.h's functions ----
struct Front {
    bool more = false;
    uint32_t crc16 = 0, wire = 0;
};
// sixteen lanes: a header byte each, the flags from its lane, a term each (only of a whole header)
Front lanes_front(const mck::RpcHdrPack &pk, uint32_t kind, const uint8_t *msg, uint64_t L) {
    Front r;
    const bool whole = L >= mck::kRpcHdrBytes;
    uint32_t hb[16] = {0}, term[16] = {0};
    for (uint32_t lane = 0; lane < 16; lane++)
        if (whole) hb[lane] = msg[lane];
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
void store_crc16(uint8_t *msg, uint32_t kind, uint32_t crc16) {
    msg[mck::rpc_hash_at(kind)] = (uint8_t)(crc16 >> 8);
    msg[mck::rpc_hash_at(kind) + 1] = (uint8_t)crc16;
}
// xdr_decoded_len of the schema: the INT field only, with the walk's bounds tests
bool pre_decoded_len(const uint8_t *x, uint64_t avail, uint64_t *n) {
    if (avail < 4) return false;
    const uint64_t len = get_be32(x);
    if (len > avail - 4 || ((len + 3) & ~3ull) > avail - 4) return false;
    *n = 4 + len;
    return true;
}
// the walk: hashes the decoded stream, stores it at d when d is not null; false: it ran past the message
bool walk(const uint8_t *x, uint64_t avail, uint8_t *d, uint32_t *crc) {
    if (avail < 4) return false;
    const uint32_t len = get_be32(x);
    uint8_t le[4];
    for (int b = 0; b < 4; b++) le[b] = (uint8_t)(len >> (8 * b));
    if (len > avail - 4 || (((uint64_t)len + 3) & ~3ull) > avail - 4) return false;
    Bytes stream(le, le + 4);
    for (uint32_t i = 0; i < len; i++) stream.push_back(x[4 + i]);
    if (d) std::memcpy(d, stream.data(), stream.size());
    *crc = naive_crc32c(stream.data(), stream.size());
    return true;
}
uint32_t lanes_verify(const mck::RpcHdrPack &pk, uint32_t kind, const uint8_t *msg, uint64_t m0, uint64_t m1, uint64_t pay,
                      uint64_t hash) {
    const uint64_t L = mck::rpc_len(m0, m1);
    const Front f = lanes_front(pk, kind, msg, L);
    bool bad = !mck::rpc_xdr_walks(L, f.more, pay);
    uint32_t crc = 0;
    if (!bad) bad = !walk(msg + pay, L - pay, nullptr, &crc);
    const bool pay_ok = !bad && get_be32(msg + hash) == crc;
    return mck::rpc_xdr_verify_class(L, f.crc16 == f.wire, f.more, pay, !bad, pay_ok);
}
uint32_t lanes_seal(const mck::RpcHdrPack &pk, uint32_t kind, uint8_t *msg, uint64_t m0, uint64_t m1, uint64_t pay,
                    uint64_t hash) {
    const uint64_t L = mck::rpc_len(m0, m1);
    const Front f = lanes_front(pk, kind, msg, L);
    bool bad = !mck::rpc_xdr_walks(L, f.more, pay);
    uint32_t crc = 0;
    if (!bad) bad = !walk(msg + pay, L - pay, nullptr, &crc);
    const uint32_t cls = mck::rpc_xdr_seal_class(L, f.more, pay, !bad);
    if (cls == mck::kRpcOk) put_be32(msg + hash, crc);
    if (cls != mck::kRpcShort) store_crc16(msg, kind, f.crc16);
    return cls;
}
uint32_t lanes_unpack(const mck::RpcHdrPack &pk, uint32_t kind, const uint8_t *msg, uint64_t m0, uint64_t m1, uint64_t pay,
                      uint64_t hash, uint8_t *dst, uint64_t d0, uint64_t d1) {
    const uint64_t L = mck::rpc_len(m0, m1), R = mck::rpc_len(d0, d1);
    const Front f = lanes_front(pk, kind, msg, L);
    bool bad = !mck::rpc_xdr_walks(L, f.more, pay);
    uint64_t decoded = 0;
    bool fits = !bad && pre_decoded_len(msg + pay, L - pay, &decoded);
    bad = !mck::rpc_xdr_unpacks(L, f.more, pay, fits, decoded, R);
    const bool walked = !bad;
    uint32_t crc = 0;
    if (!bad) bad = !walk(msg + pay, L - pay, dst, &crc);
    fits = fits && !(walked && bad);
    const bool pay_ok = !bad && get_be32(msg + hash) == crc;
    return mck::rpc_xdr_unpack_class(L, f.crc16 == f.wire, f.more, pay, fits, decoded, R, pay_ok);
}
uint32_t lanes_pack(const mck::RpcHdrPack &pk, uint32_t kind, uint8_t *msg, uint64_t m0, uint64_t m1, uint64_t pay, uint64_t hash,
                    const uint8_t *src, uint64_t s0, uint64_t s1) {
    const uint64_t L = mck::rpc_len(m0, m1), R = mck::rpc_len(s0, s1);
    const Front f = lanes_front(pk, kind, msg, L);
    uint64_t encoded = 0;
    bool exact = false;
    if (mck::rpc_hashes_payload(L, f.more, pay)) {  // xdr_encoded_len: the image's INT field only
        if (R >= 4) {
            const uint64_t n = (uint64_t)src[0] | (uint64_t)src[1] << 8 | (uint64_t)src[2] << 16 | (uint64_t)src[3] << 24;
            exact = n == R - 4;
            encoded = 4 + ((n + 3) & ~3ull);
        }
    }
    const bool packs = mck::rpc_xdr_packs(L, f.more, pay, exact, encoded);
    uint32_t crc = 0;
    if (packs) {
        const uint64_t n = R - 4;
        put_be32(msg + pay, (uint32_t)n);
        for (uint64_t i = 0; i < n; i++) msg[pay + 4 + i] = src[4 + i];
        for (uint64_t i = 4 + n; i < encoded; i++) msg[pay + i] = 0;
        crc = naive_crc32c(src, R);
    }
    const uint32_t cls = mck::rpc_xdr_pack_class(L, f.more, pay, exact, encoded);
    if (cls == mck::kRpcOk) put_be32(msg + hash, crc);
    if (cls == mck::kRpcOk || cls == mck::kRpcDeferred) store_crc16(msg, kind, f.crc16);
    return cls;
}

}  // namespace

int main() {
    static_assert(mck::kRpcMisfit == MISFIT && mck::kRpcCopyClasses == CLASSES && mck::kRpcClasses == 6, "the classes");
    const uint64_t shapes[][2] = {{20, 16}, {24, 16}, {21, 17}};  // payload_offset, hash_offset
    const uint32_t lens[] = {0, 1, 3, 4, 5, 8};
    unsigned long long seen[CLASSES] = {0}, unpacked[CLASSES] = {0}, sealed[CLASSES] = {0}, packed[CLASSES] = {0}, msgs = 0;
    unsigned long long copied_bad_header = 0, past_by_one = 0, exact_end = 0, slack = 0;
    uint32_t rng = 20240607;
    auto next = [&] { return rng = rng * 1664525u + 1013904223u; };
    for (const Model16 &m : kModels)
        for (uint32_t kind = 0; kind < 2; kind++) {
            mck::RpcHdrPack pk;
            mck::rpc_hdr_pack_build(m.poly, m.reflected, m.init, m.xorout, kind, &pk);
            for (const auto &sh : shapes)
                for (uint64_t L = 0; L <= sh[0] + 20; L++)
                    for (uint32_t n : lens)
                        for (int more = 0; more < 2; more++)
                            for (int variant = 0; variant < 4; variant++) {  // bit 0: header hash wrong, bit 1: payload hash wrong
                                const uint64_t pay = sh[0], hash = sh[1];
                                Bytes blank(L);  // exactly sized: one past is the sanitizer's
                                for (auto &b : blank) b = (uint8_t)(next() >> 24);
                                if (L > flags_at(kind)) blank[flags_at(kind)] = (uint8_t)((blank[flags_at(kind)] & ~1u) | (unsigned)more);
                                if (L >= pay + 4) put_be32(blank.data() + pay, n);
                                const uint64_t need = 4 + ((n + 3ull) & ~3ull);
                                if (L >= pay + 4) {
                                    past_by_one += L - pay + 1 == need;
                                    exact_end += L - pay == need;
                                    slack += L - pay == need + 1;
                                }
                                // ---- seal: the lanes against the model, and exactly 0, 2 or 6 bytes change ----
                                Bytes a = blank, b = blank;
                                const uint32_t sa = lanes_seal(pk, kind, a.data(), 7, 7 + L, pay, hash);
                                CHECK(sa == naive_seal(m, (int)kind, b, pay, hash));
                                CHECK(a == b);
                                sealed[sa]++;
                                for (uint64_t i = 0; i < L; i++) {
                                    const size_t at = hdr_hash_at(kind);
                                    const bool hdr = i == at || i == at + 1, slot = i >= hash && i < hash + 4;
                                    if (!(sa == OK ? hdr || slot : sa == DEFERRED && hdr)) CHECK(a[i] == blank[i]);
                                }
                                // ---- verify: a message sealed by the model, then corrupted by the variant ----
                                Bytes msg = b;
                                if (L >= 16) {
                                    if (sa == SHORT) put_hdr_crc(m, (int)kind, msg);  // (a short eager message with a good header)
                                    if (variant & 1) msg[hdr_hash_at(kind) + (L & 1)] ^= (uint8_t)(1u << (L % 8));
                                    if ((variant & 2) && L >= hash + 4) msg[hash + L % 4] ^= 0x40;
                                }
                                const Bytes msg0 = msg;
                                const uint32_t va = lanes_verify(pk, kind, msg.data(), 5, 5 + L, pay, hash);
                                CHECK(va == naive_verify(m, (int)kind, msg, pay, hash));
                                CHECK(msg == msg0 && va < mck::kRpcClasses && va != FAULT);
                                if (!(variant & 1) && L >= 16) {  // header good: the verdict follows the sender's
                                    if (more) CHECK(va == DEFERRED);
                                    else if (sa == SHORT) CHECK(va == SHORT);
                                    else CHECK(va == ((variant & 2) ? PAYLOAD : OK));
                                }
                                if ((variant & 1) && L >= 16) CHECK(va == HEADER);  // also with MORE_DATA: not DEFERRED
                                seen[va]++;
                                msgs++;
                                // ---- unpack: R = decoded - 1, decoded, decoded + 1 (4 + n where nothing is decoded) ----
                                for (int d = -1; d <= 1; d++) {
                                    const uint64_t R = 4 + n + d;
                                    Bytes da(R, kSentinel), db(R, kSentinel);
                                    const uint32_t ua = lanes_unpack(pk, kind, msg.data(), 5, 5 + L, pay, hash, da.data(), 11, 11 + R);
                                    CHECK(ua == naive_unpack(m, (int)kind, msg, pay, hash, db));
                                    CHECK(da == db && msg == msg0);
                                    const bool fits = L >= 16 && !more && L >= pay + need;
                                    const bool written = fits && d == 0;
                                    if (!written) CHECK(da == Bytes(R, kSentinel));
                                    else CHECK(da[0] == n && std::memcmp(da.data() + 4, msg.data() + pay + 4, n) == 0);
                                    CHECK(written == (ua == OK || ua == PAYLOAD) || ua == HEADER);
                                    if (va != OK && va != PAYLOAD) CHECK(ua == va);  // rules 1-5 are verify's
                                    else CHECK(ua == (d ? (uint32_t)MISFIT : va));
                                    copied_bad_header += written && ua == HEADER;
                                    unpacked[ua]++;
                                }
                                // ---- pack: image one byte short, exact, one long; the message exact or one off ----
                                for (int d = -1; d <= 1; d++) {
                                    Bytes image(4 + n + d);
                                    for (auto &q : image) q = (uint8_t)(next() >> 24);
                                    for (size_t q = 0; q < 4 && q < image.size(); q++) image[q] = (uint8_t)(n >> (8 * q));
                                    const Bytes image0 = image;
                                    Bytes pa = blank, pb = blank;
                                    const uint32_t qa = lanes_pack(pk, kind, pa.data(), 7, 7 + L, pay, hash, image.data(), 3, 3 + image.size());
                                    CHECK(qa == naive_pack(m, (int)kind, pb, pay, hash, image));
                                    CHECK(pa == pb && image == image0);
                                    packed[qa]++;
                                    if (L >= 16 && !more && L >= pay) CHECK((qa == OK) == (d == 0 && L == pay + need));
                                    size_t changed_ok = 0;
                                    for (uint64_t i = 0; i < L; i++) {
                                        const size_t at = hdr_hash_at(kind);
                                        const bool hdr = i == at || i == at + 1, slot = i >= hash && i < hash + 4, body = i >= pay;
                                        const bool may = qa == OK ? hdr || slot || body : qa == DEFERRED && hdr;
                                        if (!may) CHECK(pa[i] == blank[i]);
                                        changed_ok += may;
                                    }
                                    CHECK(changed_ok == (qa == OK ? need + 6 : qa == DEFERRED ? 2u : 0u));
                                    // round trip: what pack made, verify reads so, and unpack returns the image
                                    if (qa == OK || qa == DEFERRED) {
                                        CHECK(lanes_verify(pk, kind, pa.data(), 0, L, pay, hash) == qa);
                                        Bytes back(image.size(), kSentinel);
                                        CHECK(lanes_unpack(pk, kind, pa.data(), 0, L, pay, hash, back.data(), 0, back.size()) == qa);
                                        CHECK(qa == OK ? back == image : back == Bytes(image.size(), kSentinel));
                                    }
                                }
                            }
        }
    for (uint32_t k = 0; k < mck::kRpcClasses; k++) CHECK((seen[k] >= 100) == (k != FAULT));  // every verdict, not vacuously
    for (uint32_t k = 0; k < CLASSES; k++) CHECK((unpacked[k] >= 100) == (k != FAULT));
    CHECK(sealed[OK] && sealed[DEFERRED] && sealed[SHORT] && !sealed[PAYLOAD] && !sealed[HEADER] && !sealed[FAULT] && !sealed[MISFIT]);
    CHECK(packed[OK] && packed[DEFERRED] && packed[SHORT] && packed[MISFIT] && !packed[PAYLOAD] && !packed[HEADER] && !packed[FAULT]);
    CHECK(copied_bad_header > 0);                           // a HEADER message that fits is decoded
    CHECK(past_by_one > 0 && exact_end > 0 && slack > 0);  // the schema's end on both sides of the message's
    // the boundaries, one by one: L = 15 / 16, payload_offset - 1 / payload_offset, fits or not, lengths off by one
    CHECK(mck::rpc_xdr_verify_class(15, true, false, 20, true, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_verify_class(16, true, true, 20, false, false) == mck::kRpcDeferred);
    CHECK(mck::rpc_xdr_verify_class(16, false, true, 20, false, false) == mck::kRpcHeader);  // not DEFERRED
    CHECK(mck::rpc_xdr_verify_class(19, true, false, 20, true, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_verify_class(20, true, false, 20, true, true) == mck::kRpcOk);
    CHECK(mck::rpc_xdr_verify_class(20, true, false, 20, false, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_verify_class(20, true, false, 20, true, false) == mck::kRpcPayload);
    CHECK(!mck::rpc_xdr_walks(15, false, 20) && !mck::rpc_xdr_walks(19, false, 20) && mck::rpc_xdr_walks(20, false, 20));
    CHECK(!mck::rpc_xdr_walks(1ull << 40, true, 20));
    CHECK(mck::rpc_xdr_seal_class(15, false, 20, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_seal_class(16, true, 20, false) == mck::kRpcDeferred);
    CHECK(mck::rpc_xdr_seal_class(19, false, 20, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_seal_class(20, false, 20, false) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_seal_class(20, false, 20, true) == mck::kRpcOk);
    for (uint64_t R : {7ull, 9ull}) {
        CHECK(mck::rpc_xdr_unpack_class(28, true, false, 20, true, 8, R, true) == mck::kRpcMisfit);
        CHECK(!mck::rpc_xdr_unpacks(28, false, 20, true, 8, R));
    }
    CHECK(mck::rpc_xdr_unpack_class(28, true, false, 20, true, 8, 8, true) == mck::kRpcOk);
    CHECK(mck::rpc_xdr_unpack_class(28, false, false, 20, true, 8, 8, true) == mck::kRpcHeader);
    CHECK(mck::rpc_xdr_unpacks(28, false, 20, true, 8, 8));  // the header's verdict does not enter
    CHECK(mck::rpc_xdr_unpack_class(28, true, false, 20, false, 8, 8, true) == mck::kRpcShort);
    CHECK(!mck::rpc_xdr_unpacks(28, false, 20, false, 8, 8) && !mck::rpc_xdr_unpacks(28, true, 20, true, 8, 8));
    CHECK(mck::rpc_xdr_unpack_class(15, true, false, 20, true, 8, 8, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_unpack_class(19, true, false, 20, true, 8, 8, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_unpack_class(16, true, true, 20, false, 0, 5, false) == mck::kRpcDeferred);
    CHECK(mck::rpc_xdr_pack_class(15, false, 20, true, 0) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_pack_class(16, true, 20, false, 0) == mck::kRpcDeferred);
    CHECK(mck::rpc_xdr_pack_class(19, false, 20, true, 0) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_pack_class(28, false, 20, true, 8) == mck::kRpcOk);
    CHECK(mck::rpc_xdr_pack_class(28, false, 20, false, 8) == mck::kRpcMisfit);
    CHECK(mck::rpc_xdr_pack_class(27, false, 20, true, 8) == mck::kRpcMisfit);
    CHECK(mck::rpc_xdr_pack_class(29, false, 20, true, 8) == mck::kRpcMisfit);
    CHECK(mck::rpc_xdr_packs(28, false, 20, true, 8) && !mck::rpc_xdr_packs(29, false, 20, true, 8));
    CHECK(!mck::rpc_xdr_packs(28, true, 20, true, 8) && !mck::rpc_xdr_packs(28, false, 20, false, 8));
    // a table that runs backwards is an empty message; sizes past 2^32 are not truncated
    CHECK(mck::rpc_xdr_verify_class(mck::rpc_len(9, 3), true, false, 20, true, true) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_pack_class(mck::rpc_len(9, 3), false, 20, true, 0) == mck::kRpcShort);
    CHECK(mck::rpc_xdr_unpack_class((1ull << 33) + 20, true, false, 20, true, 1ull << 33, 1ull << 33, true) == mck::kRpcOk);
    CHECK(mck::rpc_xdr_unpack_class((1ull << 33) + 20, true, false, 20, true, 1ull << 33, 0, true) == mck::kRpcMisfit);
    CHECK(mck::rpc_xdr_pack_class((1ull << 33) + 20, false, 20, true, 0) == mck::kRpcMisfit);
    // the FAULT value is no rule's verdict: only a launch that gave up a wait writes it
    std::printf("%llu messages: ok %llu payload %llu header %llu short %llu deferred %llu; unpack misfit %llu\n", msgs, seen[OK],
                seen[PAYLOAD], seen[HEADER], seen[SHORT], seen[DEFERRED], unpacked[MISFIT]);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
