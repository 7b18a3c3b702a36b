// The rules of the RPC message calls (mercury_amd/csrc/launch_plan.h:
// rpc_verify_class, rpc_seal_class, rpc_hashes_payload, the header pack and its
// per-byte terms) against a model written here from the contract alone: the
// field image assembled field by field, both CRCs bit by bit, the rules as the
// header words them.  `lanes_*` below do what the kernel's lanes do
// (crc_gpu_crc32.h, RPC) with the same functions, on host memory.  Both kinds;
// L = 0 .. payload_offset + 8; (payload_offset, hash_offset) = (20, 16),
// (24, 16), (21, 17); MORE_DATA set and clear; header hash and payload hash
// right and wrong; four 16-bit models of both bit orders.  Every message sits
// alone in an exactly sized allocation, so a byte read or written past its end
// is the sanitizer's.  Stand-alone: plain and under the sanitizers
// (tests/test_rpc_msg.py).
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
    {"crc16-arc", 0x8005, true, 0x0000, 0x0000},
    {"crc16-genibus", 0x1021, false, 0xFFFF, 0xFFFF},
};

// ---- the model: nothing from launch_plan.h below this line ----
uint32_t naive_crc16(const Model16 &m, const uint8_t *p, size_t n) {
    uint32_t r = m.init;
    for (size_t i = 0; i < n; i++) {
        uint32_t b = p[i];
        if (m.reflected) {  // refin: the byte's bits enter low bit first = the byte bit-reversed, MSB first
            uint32_t v = 0;
            for (int k = 0; k < 8; k++) v |= ((b >> k) & 1u) << (7 - k);
            b = v;
        }
        r ^= b << 8;
        for (int k = 0; k < 8; k++) r = (r & 0x8000u ? (r << 1) ^ m.poly : r << 1) & 0xFFFFu;
    }
    if (m.reflected) {  // refout
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
// the host-order image hg_core_header_*_proc hashes, from the wire bytes, field by field
size_t naive_image(int kind, const uint8_t *h, uint8_t *img) {
    if (kind == 0) {
        img[0] = h[0];  // hg
        img[1] = h[1];  // protocol
        uint64_t id = 0;
        for (int b = 0; b < 8; b++) id = id << 8 | h[2 + b];  // big-endian on the wire
        std::memcpy(img + 2, &id, 8);                         // a little-endian host's uint64_t
        img[10] = h[10];  // flags
        img[11] = h[11];  // cookie
        return 12;
    }
    img[0] = h[0];  // ret_code
    img[1] = h[1];  // flags
    const uint16_t cookie = (uint16_t)(h[2] << 8 | h[3]);
    std::memcpy(img + 2, &cookie, 2);
    return 4;
}
uint32_t naive_verify(const Model16 &m, int kind, const std::vector<uint8_t> &msg, size_t pay, size_t hash) {
    const size_t L = msg.size();
    if (L < 16) return 3;
    uint8_t img[12];
    const size_t n = naive_image(kind, msg.data(), img);
    const size_t at = kind == 0 ? 12 : 4;
    if (naive_crc16(m, img, n) != (uint32_t)(msg[at] << 8 | msg[at + 1])) return 2;
    if (msg[kind == 0 ? 10 : 1] & 1) return 4;
    if (L < pay) return 3;
    const uint32_t wire = (uint32_t)msg[hash] << 24 | (uint32_t)msg[hash + 1] << 16 | (uint32_t)msg[hash + 2] << 8 | msg[hash + 3];
    return naive_crc32c(msg.data() + pay, L - pay) == wire ? 0 : 1;
}
// the sealed message and its status
uint32_t naive_seal(const Model16 &m, int kind, std::vector<uint8_t> &msg, size_t pay, size_t hash) {
    const size_t L = msg.size();
    if (L < 16) return 3;
    const bool more = msg[kind == 0 ? 10 : 1] & 1;
    if (!more && L < pay) return 3;
    uint8_t img[12];
    const size_t n = naive_image(kind, msg.data(), img);
    const uint32_t c = naive_crc16(m, img, n);
    const size_t at = kind == 0 ? 12 : 4;
    msg[at] = (uint8_t)(c >> 8);
    msg[at + 1] = (uint8_t)c;
    if (more) return 4;
    const uint32_t x = naive_crc32c(msg.data() + pay, L - pay);
    for (int b = 0; b < 4; b++) msg[hash + b] = (uint8_t)(x >> (24 - 8 * b));
    return 0;
}

// ---- what the kernel's lanes do, with launch_plan.h's functions ----
struct Lanes {
    bool more = false, hashed = false;
    uint32_t crc16 = 0, wire = 0, x = 0;
};
Lanes lanes_front(const mck::RpcHdrPack &pk, uint32_t kind, const uint8_t *msg, uint64_t L, uint64_t pay) {
    Lanes r;
    const bool whole = L >= mck::kRpcHdrBytes;
    uint32_t hb[16] = {0}, term[16] = {0};
    for (uint32_t lane = 0; lane < 16; lane++)
        if (whole) hb[lane] = msg[lane];
    r.more = whole && (hb[mck::rpc_flags_at(kind)] & 1u);
    for (uint32_t lane = 0; lane < 16; lane++)
        if (whole) term[lane] = mck::rpc_hdr_term(&pk, kind, lane, hb[lane]);
    r.hashed = mck::rpc_hashes_payload(L, r.more, pay);
    // (the payload loops themselves are the kernels' and the emulator's; here the value they return)
    r.x = r.hashed ? naive_crc32c(msg + pay, L - pay) : naive_crc32c(nullptr, 0);
    uint32_t t = 0;
    for (uint32_t lane = 0; lane < mck::rpc_img_bytes(kind); lane++) t ^= term[lane];
    r.crc16 = mck::rpc_hdr_crc(pk.c, t);
    const uint32_t hat = mck::rpc_hash_at(kind);
    r.wire = term[hat] << 8 | term[hat + 1];
    return r;
}
uint32_t lanes_verify(const mck::RpcHdrPack &pk, uint32_t kind, const uint8_t *msg, uint64_t L, uint64_t pay, uint64_t hash) {
    const Lanes r = lanes_front(pk, kind, msg, L, pay);
    bool pay_ok = false;
    if (r.hashed) {
        const uint8_t *q = msg + hash;
        pay_ok = ((uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3]) == r.x;
    }
    return mck::rpc_verify_class(L, r.crc16 == r.wire, r.more, pay, pay_ok);
}
uint32_t lanes_seal(const mck::RpcHdrPack &pk, uint32_t kind, uint8_t *msg, uint64_t L, uint64_t pay, uint64_t hash) {
    const Lanes r = lanes_front(pk, kind, msg, L, pay);
    const uint32_t cls = mck::rpc_seal_class(L, r.more, pay);
    if (cls == mck::kRpcOk)
        for (int b = 0; b < 4; b++) msg[hash + b] = (uint8_t)(r.x >> (24 - 8 * b));
    if (cls != mck::kRpcShort) {
        const uint32_t hat = mck::rpc_hash_at(kind);
        msg[hat] = (uint8_t)(r.crc16 >> 8);
        msg[hat + 1] = (uint8_t)r.crc16;
    }
    return cls;
}

}  // namespace

int main() {
    const uint64_t shapes[][2] = {{20, 16}, {24, 16}, {21, 17}};  // payload_offset, hash_offset
    unsigned long long seen[mck::kRpcClasses] = {0}, sealed[mck::kRpcClasses] = {0}, msgs = 0;
    uint32_t rng = 12345;
    auto next = [&] { return rng = rng * 1664525u + 1013904223u; };
    for (const Model16 &m : kModels)
        for (uint32_t kind = 0; kind < 2; kind++) {
            mck::RpcHdrPack pk;
            mck::rpc_hdr_pack_build(m.poly, m.reflected, m.init, m.xorout, kind, &pk);
            CHECK(pk.kind == kind);
            for (const auto &sh : shapes)
                for (uint64_t L = 0; L <= sh[0] + 8; L++)
                    for (int more = 0; more < 2; more++)
                        for (int variant = 0; variant < 4; variant++) {  // bit 0: header hash wrong, bit 1: payload hash wrong
                            const uint64_t pay = sh[0], hash = sh[1];
                            std::vector<uint8_t> blank(L);  // exactly L bytes: one past is the sanitizer's
                            for (auto &b : blank) b = (uint8_t)(next() >> 24);
                            const size_t fl = kind == 0 ? 10 : 1;
                            if (L > fl) blank[fl] = (uint8_t)((blank[fl] & ~1u) | (unsigned)more);
                            // seal: the lanes against the model, byte for byte
                            std::vector<uint8_t> a = blank, b = blank;
                            const uint32_t sa = lanes_seal(pk, kind, a.data(), L, pay, hash);
                            const uint32_t sb = naive_seal(m, (int)kind, b, pay, hash);
                            CHECK(sa == sb);
                            CHECK(a == b);
                            sealed[sa]++;
                            size_t changed = 0;
                            for (uint64_t i = 0; i < L; i++) {
                                const size_t at = kind == 0 ? 12 : 4;
                                const bool hdr = i == at || i == at + 1, slot = i >= hash && i < hash + 4;
                                const bool may = sa == mck::kRpcOk ? hdr || slot : sa == mck::kRpcDeferred ? hdr : false;
                                if (!may) CHECK(a[i] == blank[i]);
                                changed += may;
                            }
                            CHECK(changed == (sa == mck::kRpcOk ? 6u : sa == mck::kRpcDeferred ? 2u : 0u));
                            // a sealed message verifies: OK or DEFERRED
                            if (sa != mck::kRpcShort) CHECK(lanes_verify(pk, kind, a.data(), L, pay, hash) == sa);
                            // verify, with the hashes right or wrong as the variant says
                            if ((variant & 1) && L >= 16) a[(kind == 0 ? 12 : 4) + (L & 1)] ^= (uint8_t)(1u << (L % 8));
                            if ((variant & 2) && L >= hash + 4) a[hash + L % 4] ^= 0x40;
                            const uint32_t va = lanes_verify(pk, kind, a.data(), L, pay, hash);
                            const uint32_t vb = naive_verify(m, (int)kind, a, pay, hash);
                            CHECK(va == vb);
                            CHECK(va < mck::kRpcFault);
                            seen[va]++;
                            msgs++;
                        }
            // every covered header byte, bit by bit: HEADER; an uncovered one: still OK
            std::vector<uint8_t> good(20 + 33);
            for (auto &b : good) b = (uint8_t)(next() >> 24);
            good[kind == 0 ? 10 : 1] &= 0xFE;
            CHECK(lanes_seal(pk, kind, good.data(), good.size(), 20, 16) == mck::kRpcOk);
            for (size_t i = 0; i < 16; i++)
                for (int bit = 0; bit < 8; bit++) {
                    std::vector<uint8_t> c = good;
                    c[i] ^= (uint8_t)(1u << bit);
                    const bool covered = i < (kind == 0 ? 14u : 6u);  // the image and the hash itself
                    const uint32_t v = lanes_verify(pk, kind, c.data(), c.size(), 20, 16);
                    CHECK(v == (covered ? mck::kRpcHeader : mck::kRpcOk));
                    CHECK(v == naive_verify(m, (int)kind, c, 20, 16));
                }
        }
    for (uint32_t k = 0; k < mck::kRpcFault; k++) CHECK(seen[k] > 0);  // every verdict was reached
    CHECK(seen[mck::kRpcFault] == 0 && sealed[mck::kRpcOk] && sealed[mck::kRpcDeferred] && sealed[mck::kRpcShort]);
    // a table that runs backwards is an empty message
    CHECK(mck::rpc_len(100, 99) == 0 && mck::rpc_len(~0ull, 3) == 0 && mck::rpc_len(5, 25) == 20);
    CHECK(mck::rpc_verify_class(mck::rpc_len(9, 3), true, false, 20, true) == mck::kRpcShort);
    CHECK(!mck::rpc_hashes_payload(mck::rpc_len(9, 3), false, 20));
    // a payload_offset past 2^32 is not truncated
    CHECK(mck::rpc_verify_class(1ull << 33, true, false, (1ull << 40), true) == mck::kRpcShort);
    CHECK(mck::rpc_seal_class(1ull << 33, false, (1ull << 40)) == mck::kRpcShort);
    // the kernels there are for the RPC calls: light, full, non-temporal, verify and seal -- six keys of the RPC
    // frame; its other six are the copying twins' (rpc_copy_msg.cpp), and a key has one frame: never detached
    int n = 0, n_copy = 0;
    for (int op = -1; op <= mck::kOpUnpack + 1; op++)
        for (int width : {32, 64})
            for (int mode = 0; mode <= kOffsets; mode++)
                for (int f = 0; f < 8; f++) {
                    const mck::KernelKey k{width, CRC_GPU_MAX_LOG2G, mode, op, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, mck::kFrameRpc};
                    if (!mck::kernel_key_valid(k)) continue;
                    const bool copy = op == mck::kOpPack || op == mck::kOpUnpack;
                    (copy ? n_copy : n)++;
                    CHECK(width == 32 && mode == kOffsets && !k.split && k.frame != mck::kFrameDetached && !(k.nt && k.light));
                    CHECK(copy || op == mck::kOpVerify || op == mck::kOpSeal);
                    mck::KernelKey plain = k;
                    plain.frame = mck::kFramePayloads;
                    CHECK(mck::kernel_key_valid(plain) && !(plain == k));
                }
    CHECK(n == 6 && n_copy == 6);
    {
        // kernel_key(plan, op, frame) yields them, and kernel_key(plan, op) does not
        mck::LaunchPlan p;
        p.width = 32, p.lg = CRC_GPU_MAX_LOG2G, p.mode = kOffsets;
        for (mck::BatchOp op : {mck::kOpVerify, mck::kOpSeal}) {
            const mck::KernelKey k = mck::kernel_key(p, op, mck::kFrameRpc);
            CHECK(mck::kernel_key_valid(k) && k.frame == mck::kFrameRpc && k.op == op);
            CHECK(mck::kernel_key(p, op).frame == mck::kFramePayloads);
        }
    }
    {
        // kernel_key(plan, op, frame) yields them, and kernel_key(plan, op) does not
        mck::LaunchPlan p;
        p.width = 32, p.lg = CRC_GPU_MAX_LOG2G, p.mode = kOffsets;
        for (mck::BatchOp op : {mck::kOpVerify, mck::kOpSeal}) {
            CHECK(mck::kernel_key_valid(mck::kernel_key(p, op, mck::kFrameRpc)) && mck::kernel_key(p, op, mck::kFrameRpc).frame == mck::kFrameRpc);
            CHECK(mck::kernel_key(p, op).frame == mck::kFramePayloads);
        }
    }
    std::printf("%llu messages: ok %llu payload %llu header %llu short %llu deferred %llu\n", msgs, seen[0], seen[1], seen[2], seen[3],
                seen[4]);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
