// The rules of the copying RPC message calls (mercury_amd/csrc/launch_plan.h:
// rpc_copies_payload, rpc_unpack_class, rpc_pack_class, with the header pack's
// per-byte terms) against a model written here from the contract alone
// (include/mchecksum_gpu.h: mchecksum_gpu_unpack_rpc_messages,
// mchecksum_gpu_pack_rpc_messages): the field image assembled field by field,
// both CRCs bit by bit, the rule tables as the header words them, and what each
// call writes.  `lanes_*` below do what the kernel's lanes do (crc_gpu_crc32.h,
// RPC with a copying OP) with the same functions, on host memory.  Both kinds;
// L = 0 .. payload_offset + 8; R = L - payload_offset - 1 .. + 1 (where that is
// negative: 0, 1, 2); (payload_offset, hash_offset) = (20, 16), (24, 16),
// (21, 17); MORE_DATA set and clear; header hash and payload hash right and
// wrong; a table that runs backwards.  Every message, destination and source
// sits alone in an exactly sized allocation, so a byte read or written past an
// end -- the bytes behind the core header of a message that must not be read,
// the range of a message that must not be copied -- is the sanitizer's.
// Stand-alone: plain and under the sanitizers (tests/test_rpc_copy_msg.py).
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

// The receiver: the rule table, then -- by the rule of its own -- what is written.
uint32_t naive_unpack(const Model16 &m, int kind, const std::vector<uint8_t> &msg, size_t pay, size_t hash,
                      std::vector<uint8_t> &dst) {
    const size_t L = msg.size(), R = dst.size();
    const bool more = L >= 16 && (msg[flags_at(kind)] & 1);
    if (L >= 16 && !more && L >= pay && L == pay + R)
        for (size_t i = 0; i < R; i++) dst[i] = msg[pay + i];
    if (L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (naive_hdr_crc(m, kind, msg.data()) != (uint32_t)(msg[at] << 8 | msg[at + 1])) return HEADER;
    if (more) return DEFERRED;
    if (L < pay) return SHORT;
    if (L != pay + R) return MISFIT;
    const uint32_t wire = (uint32_t)msg[hash] << 24 | (uint32_t)msg[hash + 1] << 16 | (uint32_t)msg[hash + 2] << 8 | msg[hash + 3];
    return naive_crc32c(msg.data() + pay, R) == wire ? OK : PAYLOAD;
}
// The sender: the rule table with its effects.
uint32_t naive_pack(const Model16 &m, int kind, std::vector<uint8_t> &msg, size_t pay, size_t hash,
                    const std::vector<uint8_t> &src) {
    const size_t L = msg.size(), R = src.size();
    if (L < 16) return SHORT;
    const size_t at = hdr_hash_at(kind);
    if (msg[flags_at(kind)] & 1) {
        const uint32_t c = naive_hdr_crc(m, kind, msg.data());
        msg[at] = (uint8_t)(c >> 8);
        msg[at + 1] = (uint8_t)c;
        return DEFERRED;
    }
    if (L < pay) return SHORT;
    if (L != pay + R) return MISFIT;
    for (size_t i = 0; i < R; i++) msg[pay + i] = src[i];
    const uint32_t x = naive_crc32c(src.data(), R);
    for (int b = 0; b < 4; b++) msg[hash + b] = (uint8_t)(x >> (24 - 8 * b));
    const uint32_t c = naive_hdr_crc(m, kind, msg.data());
    msg[at] = (uint8_t)(c >> 8);
    msg[at + 1] = (uint8_t)c;
    return OK;
}

// ---- what the kernel's lanes do, with launch_plan.h's functions ----
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
// the payload loop with COPY: n bytes from p are stored at dst and hashed (n = 0: nothing is touched)
uint32_t copy_and_hash(const uint8_t *p, uint64_t n, uint8_t *dst) {
    for (uint64_t i = 0; i < n; i++) dst[i] = p[i];
    return n ? naive_crc32c(p, n) : naive_crc32c(nullptr, 0);
}
uint32_t lanes_unpack(const mck::RpcHdrPack &pk, uint32_t kind, const uint8_t *msg, uint64_t m0, uint64_t m1, uint64_t pay,
                      uint64_t hash, uint8_t *dst, uint64_t d0, uint64_t d1) {
    const uint64_t L = mck::rpc_len(m0, m1);
    const Front f = lanes_front(pk, kind, msg, L);
    const uint64_t R = mck::rpc_len(d0, d1);
    const bool copied = mck::rpc_copies_payload(L, f.more, pay, R);
    const uint32_t x = copy_and_hash(msg + (copied ? pay : 0), copied ? R : 0, dst);
    bool pay_ok = false;
    if (copied) {
        const uint8_t *q = msg + hash;
        pay_ok = ((uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3]) == x;
    }
    return mck::rpc_unpack_class(L, f.crc16 == f.wire, f.more, pay, R, pay_ok);
}
uint32_t lanes_pack(const mck::RpcHdrPack &pk, uint32_t kind, uint8_t *msg, uint64_t m0, uint64_t m1, uint64_t pay, uint64_t hash,
                    const uint8_t *src, uint64_t s0, uint64_t s1) {
    const uint64_t L = mck::rpc_len(m0, m1);
    const Front f = lanes_front(pk, kind, msg, L);
    const uint64_t R = mck::rpc_len(s0, s1);
    const bool copied = mck::rpc_copies_payload(L, f.more, pay, R);
    const uint32_t x = copy_and_hash(src, copied ? R : 0, msg + (copied ? pay : 0));
    const uint32_t cls = mck::rpc_pack_class(L, f.more, pay, R);
    if (cls == mck::kRpcOk)
        for (int b = 0; b < 4; b++) msg[hash + b] = (uint8_t)(x >> (24 - 8 * b));
    if (cls == mck::kRpcOk || cls == mck::kRpcDeferred) {
        const uint32_t hat = mck::rpc_hash_at(kind);
        msg[hat] = (uint8_t)(f.crc16 >> 8);
        msg[hat + 1] = (uint8_t)f.crc16;
    }
    return cls;
}

}  // namespace

int main() {
    static_assert(mck::kRpcMisfit == MISFIT && mck::kRpcCopyClasses == CLASSES && mck::kRpcClasses == 6, "the classes");
    const uint64_t shapes[][2] = {{20, 16}, {24, 16}, {21, 17}};  // payload_offset, hash_offset
    unsigned long long seen[CLASSES] = {0}, packed[CLASSES] = {0}, msgs = 0, copied_bad_header = 0;
    uint32_t rng = 424242;
    auto next = [&] { return rng = rng * 1664525u + 1013904223u; };
    for (const Model16 &m : kModels)
        for (uint32_t kind = 0; kind < 2; kind++) {
            mck::RpcHdrPack pk;
            mck::rpc_hdr_pack_build(m.poly, m.reflected, m.init, m.xorout, kind, &pk);
            for (const auto &sh : shapes)
                for (uint64_t L = 0; L <= sh[0] + 8; L++)
                    for (int d = -1; d <= 1; d++)
                        for (int more = 0; more < 2; more++)
                            for (int variant = 0; variant < 4; variant++) {  // bit 0: header hash wrong, bit 1: payload hash wrong
                                const uint64_t pay = sh[0], hash = sh[1];
                                const uint64_t R = L >= pay + (d < 0) ? L - pay + d : (uint64_t)(d + 1);
                                // ---- pack: blank headers, both hashes random; the lanes against the model ----
                                std::vector<uint8_t> blank(L), src(R);  // exactly sized: one past is the sanitizer's
                                for (auto &b : blank) b = (uint8_t)(next() >> 24);
                                for (auto &b : src) b = (uint8_t)(next() >> 24);
                                if (L > flags_at(kind)) blank[flags_at(kind)] = (uint8_t)((blank[flags_at(kind)] & ~1u) | (unsigned)more);
                                std::vector<uint8_t> a = blank, b = blank;
                                const std::vector<uint8_t> src0 = src;
                                // (tables that do not start at 0: the lanes see offsets, not sizes)
                                const uint32_t sa = lanes_pack(pk, kind, a.data(), 7, 7 + L, pay, hash, src.data(), 3, 3 + R);
                                const uint32_t sb = naive_pack(m, (int)kind, b, pay, hash, src);
                                CHECK(sa == sb);
                                CHECK(a == b);
                                CHECK(src == src0);
                                packed[sa]++;
                                size_t may_n = 0;
                                for (uint64_t i = 0; i < L; i++) {
                                    const size_t at = hdr_hash_at(kind);
                                    const bool hdr = i == at || i == at + 1, slot = i >= hash && i < hash + 4, body = i >= pay;
                                    const bool may = sa == OK ? hdr || slot || body : sa == DEFERRED ? hdr : false;
                                    if (!may) CHECK(a[i] == blank[i]);
                                    may_n += may;
                                }
                                CHECK(may_n == (sa == OK ? R + 6 : sa == DEFERRED ? 2u : 0u));
                                if (sa == OK) CHECK(R == L - pay && (R == 0 || std::memcmp(a.data() + pay, src.data(), R) == 0));
                                // ---- unpack: a message sealed by the model, whatever pack said of this R ----
                                std::vector<uint8_t> msg = blank;
                                if (L >= 16) {
                                    if (!more && L >= pay) {
                                        const uint32_t x = naive_crc32c(msg.data() + pay, L - pay);
                                        for (int q = 0; q < 4; q++) msg[hash + q] = (uint8_t)(x >> (24 - 8 * q));
                                    }
                                    const uint32_t c = naive_hdr_crc(m, (int)kind, msg.data());
                                    msg[hdr_hash_at(kind)] = (uint8_t)(c >> 8);
                                    msg[hdr_hash_at(kind) + 1] = (uint8_t)c;
                                    if (variant & 1) msg[hdr_hash_at(kind) + (L & 1)] ^= (uint8_t)(1u << (L % 8));
                                    if ((variant & 2) && L >= hash + 4) msg[hash + L % 4] ^= 0x40;
                                }
                                const std::vector<uint8_t> msg0 = msg;
                                std::vector<uint8_t> da(R, kSentinel), db(R, kSentinel);
                                const uint32_t va = lanes_unpack(pk, kind, msg.data(), 5, 5 + L, pay, hash, da.data(), 11, 11 + R);
                                const uint32_t vb = naive_unpack(m, (int)kind, msg, pay, hash, db);
                                CHECK(va == vb);
                                CHECK(da == db);
                                CHECK(msg == msg0);
                                CHECK(va < CLASSES && va != FAULT);
                                const bool written = L >= 16 && !more && L >= pay && L == pay + R;
                                if (written) CHECK(R == 0 || std::memcmp(da.data(), msg.data() + pay, R) == 0);
                                else CHECK(da == std::vector<uint8_t>(R, kSentinel));
                                CHECK(written == (va == OK || va == PAYLOAD) || va == HEADER);
                                copied_bad_header += written && va == HEADER && R > 0;
                                if (!(variant & 1) && L >= 16) {  // header good: the verdict follows the sender's
                                    if (more) CHECK(va == DEFERRED);
                                    else if (L >= pay) CHECK(va == (L != pay + R ? MISFIT : (variant & 2) ? PAYLOAD : OK));
                                }
                                seen[va]++;
                                msgs++;
                                // ---- round trip: what pack made OK or DEFERRED, unpack reads so, and the bytes come back ----
                                if (sa == OK || sa == DEFERRED) {
                                    std::vector<uint8_t> back(R, kSentinel);
                                    CHECK(lanes_unpack(pk, kind, a.data(), 0, L, pay, hash, back.data(), 0, R) == sa);
                                    CHECK(sa == OK ? back == src : back == std::vector<uint8_t>(R, kSentinel));
                                }
                            }
        }
    for (uint32_t k = 0; k < CLASSES; k++) CHECK((seen[k] > 0) == (k != FAULT));  // every verdict was reached
    CHECK(packed[OK] && packed[DEFERRED] && packed[SHORT] && packed[MISFIT] && !packed[PAYLOAD] && !packed[HEADER] && !packed[FAULT]);
    CHECK(copied_bad_header > 0);  // a HEADER message that fits is copied
    // a table that runs backwards is an empty range: of the message (SHORT) and of the other side (R = 0)
    CHECK(mck::rpc_unpack_class(mck::rpc_len(9, 3), true, false, 20, 0, true) == mck::kRpcShort);
    CHECK(mck::rpc_pack_class(mck::rpc_len(9, 3), false, 20, 0) == mck::kRpcShort);
    CHECK(!mck::rpc_copies_payload(mck::rpc_len(9, 3), false, 20, 0));
    CHECK(mck::rpc_unpack_class(25, true, false, 20, mck::rpc_len(40, 35), true) == mck::kRpcMisfit);
    CHECK(mck::rpc_pack_class(25, false, 20, mck::rpc_len(40, 35)) == mck::kRpcMisfit);
    CHECK(!mck::rpc_copies_payload(25, false, 20, mck::rpc_len(40, 35)));
    CHECK(mck::rpc_copies_payload(20, false, 20, mck::rpc_len(40, 35)));  // an empty payload fits an empty range
    CHECK(mck::rpc_unpack_class(20, true, false, 20, mck::rpc_len(40, 35), true) == mck::kRpcOk);
    {
        // ... and through the lanes: nothing behind either table's start is touched (both allocations are empty)
        mck::RpcHdrPack pk;
        mck::rpc_hdr_pack_build(0x1021, true, 0, 0, 0, &pk);
        std::vector<uint8_t> none;
        CHECK(lanes_unpack(pk, 0, none.data(), 90, 60, 20, 16, none.data(), 8, 2) == mck::kRpcShort);
        CHECK(lanes_pack(pk, 0, none.data(), 90, 60, 20, 16, none.data(), 8, 2) == mck::kRpcShort);
    }
    // sizes past 2^32 are not truncated, and payload_offset + R does not wrap
    CHECK(mck::rpc_unpack_class(1ull << 33, true, false, 1ull << 40, 0, true) == mck::kRpcShort);
    CHECK(mck::rpc_unpack_class((1ull << 33) + 20, true, false, 20, 1ull << 33, true) == mck::kRpcOk);
    CHECK(mck::rpc_unpack_class((1ull << 33) + 20, true, false, 20, 0, true) == mck::kRpcMisfit);
    CHECK(mck::rpc_pack_class(24, false, 20, ~0ull - 15) == mck::kRpcMisfit);  // 20 + R wraps to 4
    CHECK(!mck::rpc_copies_payload(24, false, 20, ~0ull - 15));
    // with MORE_DATA, R does not enter
    for (uint64_t R : {0ull, 1ull, 5ull, ~0ull}) {
        CHECK(mck::rpc_unpack_class(16, true, true, 20, R, false) == mck::kRpcDeferred);
        CHECK(mck::rpc_pack_class(16, true, 20, R) == mck::kRpcDeferred);
        CHECK(!mck::rpc_copies_payload(16 + R, true, 20, R));
    }
    // the kernels there are for the copying calls: light, full, non-temporal, pack and unpack -- the RPC frame's
    // keys with a copying operation (its six others: verify and seal, rpc_msg.cpp); no other frame but the
    // payloads' has a copying key, and kernel_key names them from the call's operation and frame
    int n = 0, n_check = 0;
    for (int op = -1; op <= mck::kOpUnpack + 1; op++)
        for (int width : {32, 64})
            for (int mode = 0; mode <= kOffsets; mode++)
                for (int f = 0; f < 8; f++)
                    for (int frame = -1; frame <= mck::kFrameRpc + 1; frame++) {
                        const mck::KernelKey k{width, CRC_GPU_MAX_LOG2G, mode, op, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (mck::MsgFrame)frame};
                        const bool copy = op == mck::kOpPack || op == mck::kOpUnpack;
                        if (!mck::kernel_key_valid(k) || frame == mck::kFramePayloads) continue;
                        CHECK(frame == mck::kFrameRpc || (frame == mck::kFrameDetached && !copy));
                        if (frame != mck::kFrameRpc) continue;
                        (copy ? n : n_check)++;
                        CHECK(width == 32 && mode == kOffsets && !k.split && !(k.nt && k.light));
                        CHECK(copy || op == mck::kOpVerify || op == mck::kOpSeal);
                        mck::KernelKey plain = k;
                        plain.frame = mck::kFramePayloads;
                        CHECK(mck::kernel_key_valid(plain) && !(plain == k));
                    }
    CHECK(n == 6 && n_check == 6);
    mck::LaunchPlan p;
    p.width = 32, p.lg = CRC_GPU_MAX_LOG2G, p.mode = kOffsets;
    for (int op : {mck::kOpVerify, mck::kOpSeal, mck::kOpPack, mck::kOpUnpack}) {
        const mck::KernelKey k = mck::kernel_key(p, (mck::BatchOp)op, mck::kFrameRpc);
        CHECK(mck::kernel_key_valid(k) && k.frame == mck::kFrameRpc && k.op == op);
        CHECK(mck::kernel_key(p, (mck::BatchOp)op).frame == mck::kFramePayloads);
        // in place is a run-time field of the payloads frame's kernels: folded by kernel_key, and no key says it
        CHECK(mck::kernel_key(p, (mck::BatchOp)op, mck::kFrameInPlace) == mck::kernel_key(p, (mck::BatchOp)op));
        mck::KernelKey in_place = k;
        in_place.frame = mck::kFrameInPlace;
        CHECK(!mck::kernel_key_valid(in_place));
    }
    std::printf("%llu messages: ok %llu payload %llu header %llu short %llu deferred %llu misfit %llu\n", msgs, seen[OK],
                seen[PAYLOAD], seen[HEADER], seen[SHORT], seen[DEFERRED], seen[MISFIT]);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
