// The call shape of every offsets-shaped entry point (mercury_amd/csrc/
// offsets_call.h: OffsetsCall, offsets_needs, offsets_lacks_pointer,
// batch_args_of) against a table written out by hand from what
// mchecksum_gpu.hip's offsets_call did with its `msg`, `detached` and `rpc`
// booleans before the frame had a name: for each of the thirteen entry points,
// which pointers a non-empty call must supply, whether its method is checked
// ahead of the device, and where everything lands in the kernels' argument --
// base, offsets, the three unions by each member's name, msg / pay_off /
// hash_off, the 64-bit RPC payload offset, bswap only for an MSB-first verify.
// The pointers are made-up addresses, never followed.  Stand-alone: plain and
// under the sanitizers (tests/test_offsets_call.py).
#include <cstdint>
#include <cstdio>

#include "offsets_call.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                                                    \
    do {                                                                                            \
        if (!(c)) {                                                                                 \
            if (g_fail++ < 40) std::printf("FAIL %s:%d [%s] %s\n", __FILE__, __LINE__, g_row, #c);  \
        }                                                                                           \
    } while (0)
const char *g_row = "";

template <class T = void>
T *fake(uintptr_t v) {
    return reinterpret_cast<T *>(v << 8);
}
// what the entry points are given
void *const SRC = fake(1), *const OUT = fake(3), *const DST = fake(4), *const EXPECTED = fake(6), *const HDR = fake(9);
uint64_t *const SRC_OFF = fake<uint64_t>(2), *const DST_OFF = fake<uint64_t>(5), *const HDR_OFF = fake<uint64_t>(10);
uint8_t *const STATUS = fake<uint8_t>(7);
uint32_t *const MISM = fake<uint32_t>(8), *const ERR = fake<uint32_t>(14);
// what offsets_call looks up
void *const PACK = fake(11), *const SHIFT = fake(12), *const HDR_PACK = fake(13);
const size_t kCount = 77, kPay = 20, kHash = 16;

enum Given : unsigned { gOut = 1, gDst = 2, gExpected = 4, gStatus = 8, gMism = 16, gHdr = 32, gOffs = 64, gRpc = 128 };

struct Row {
    const char *entry;  // mchecksum_gpu_<entry>
    mck::BatchOp op;
    mck::MsgFrame frame;
    unsigned given;  // what the entry point sets beside op, method, src, src_off, count, stream
    // offsets_needs
    bool need_out, need_dst, need_hdr, need_expected, method_first;
    // BatchArgs: the pointer at offset 40 (out / msgs / copy_dst), at 48 (expected / dst_offsets / rpc_hdr_pack),
    // at 112 (shift / rpc_copy_hdr_pack), then msg, pay_off, hash_off and the word at 24 (len / rpc_pay_off)
    const void *at40, *at48, *at112;
    uint32_t msg, pay_off, hash_off;
    uint64_t at24;
};
const Row kRows[] = {
    {"checksum_offsets", mck::kOpChecksum, mck::kFramePayloads, gOut, 1, 0, 0, 0, 0, OUT, nullptr, nullptr, 0, 0, 0, 0},
    {"verify_offsets", mck::kOpVerify, mck::kFramePayloads, gExpected | gStatus | gMism, 0, 0, 0, 1, 0, nullptr, EXPECTED, nullptr, 0,
     0, 0, 0},
    {"update_offsets", mck::kOpUpdate, mck::kFramePayloads, gOut, 1, 0, 0, 0, 0, OUT, nullptr, SHIFT, 0, 0, 0, 0},
    {"verify_messages", mck::kOpVerify, mck::kFrameInPlace, gOffs | gStatus | gMism, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, 1,
     kPay, kHash, 0},
    {"seal_messages", mck::kOpSeal, mck::kFrameInPlace, gOut | gOffs | gStatus, 1, 0, 0, 0, 1, OUT, nullptr, nullptr, 1, kPay, kHash, 0},
    {"pack_messages", mck::kOpPack, mck::kFrameInPlace, gDst | gOffs | gStatus, 0, 1, 0, 0, 1, DST, DST_OFF, nullptr, 1, kPay, kHash, 0},
    {"unpack_messages", mck::kOpUnpack, mck::kFrameInPlace, gDst | gOffs | gStatus | gMism, 0, 1, 0, 0, 1, DST, DST_OFF, nullptr, 1,
     kPay, kHash, 0},
    {"verify_detached_messages", mck::kOpVerify, mck::kFrameDetached, gHdr | gOffs | gStatus | gMism, 0, 0, 1, 0, 1, HDR, HDR_OFF,
     nullptr, 0, 0, kHash, 0},
    {"seal_detached_messages", mck::kOpSeal, mck::kFrameDetached, gHdr | gOffs | gStatus, 0, 0, 1, 0, 1, HDR, HDR_OFF, nullptr, 0, 0,
     kHash, 0},
    {"verify_rpc_messages", mck::kOpVerify, mck::kFrameRpc, gRpc | gOffs | gStatus | gMism, 0, 0, 0, 0, 1, nullptr, HDR_PACK, nullptr,
     0, kPay, kHash, kPay},
    {"seal_rpc_messages", mck::kOpSeal, mck::kFrameRpc, gRpc | gOut | gOffs | gStatus, 1, 0, 0, 0, 1, OUT, HDR_PACK, nullptr, 0, kPay,
     kHash, kPay},
    {"unpack_rpc_messages", mck::kOpUnpack, mck::kFrameRpc, gRpc | gDst | gOffs | gStatus | gMism, 0, 1, 0, 0, 1, DST, DST_OFF,
     HDR_PACK, 0, kPay, kHash, kPay},
    {"pack_rpc_messages", mck::kOpPack, mck::kFrameRpc, gRpc | gDst | gOffs | gStatus, 0, 1, 0, 0, 1, DST, DST_OFF, HDR_PACK, 0, kPay,
     kHash, kPay},
};

// the call as the entry point builds it (detached calls take no payload_offset)
mck::OffsetsCall call_of(const Row &r) {
    mck::OffsetsCall c{r.op, "crc32c", SRC, SRC_OFF, kCount};
    c.frame = r.frame;
    if (r.given & gOut) c.out = OUT;
    if (r.given & gDst) c.dst = DST, c.dst_off = DST_OFF;
    if (r.given & gExpected) c.expected = EXPECTED;
    if (r.given & gStatus) c.status = STATUS;
    if (r.given & gMism) c.mismatches = MISM;
    if (r.given & gHdr) c.hdr = HDR, c.hdr_off = HDR_OFF;
    if (r.given & gOffs) c.pay_off = r.frame == mck::kFrameDetached ? 0 : kPay, c.hash_off = kHash;
    if (r.given & gRpc) c.kind = 1, c.hdr_method = "crc16";
    return c;
}

}  // namespace

int main() {
    int frames[mck::kFrameRpc + 1] = {};
    for (const Row &r : kRows) {
        g_row = r.entry;
        frames[r.frame]++;
        const mck::OffsetsNeeds need = mck::offsets_needs(r.op, r.frame);
        CHECK(need.out == r.need_out && need.dst == r.need_dst && need.hdr == r.need_hdr && need.expected == r.need_expected);
        CHECK(need.method_first == r.method_first);
        const mck::OffsetsCall c = call_of(r);
        // the entry point's own call is complete; without any pointer it must supply it is not, without one it
        // need not supply it still is; an empty batch needs none
        CHECK(!mck::offsets_lacks_pointer(c));
        auto lacks = [&](auto &&drop) {
            mck::OffsetsCall d = c;
            drop(d);
            return mck::offsets_lacks_pointer(d);
        };
        CHECK(lacks([](mck::OffsetsCall &d) { d.src = nullptr; }));
        CHECK(lacks([](mck::OffsetsCall &d) { d.src_off = nullptr; }));
        CHECK(lacks([](mck::OffsetsCall &d) { d.out = nullptr; }) == r.need_out);
        CHECK(lacks([](mck::OffsetsCall &d) { d.dst = nullptr; }) == r.need_dst);
        CHECK(lacks([](mck::OffsetsCall &d) { d.dst_off = nullptr; }) == r.need_dst);
        CHECK(lacks([](mck::OffsetsCall &d) { d.hdr = nullptr; }) == r.need_hdr);
        CHECK(lacks([](mck::OffsetsCall &d) { d.hdr_off = nullptr; }) == r.need_hdr);
        CHECK(lacks([](mck::OffsetsCall &d) { d.expected = nullptr; }) == r.need_expected);
        CHECK(!lacks([](mck::OffsetsCall &d) { d.status = nullptr, d.mismatches = nullptr, d.stream = nullptr; }));
        CHECK(!lacks([](mck::OffsetsCall &d) { d = mck::OffsetsCall{d.op, d.method, nullptr, nullptr, 0, d.frame}; }));

        for (int msb = 0; msb < 2; msb++) {
            // (offsets_call fetches the shift pack for an update and the header pack for an RPC call, else null)
            const void *shift = r.op == mck::kOpUpdate ? SHIFT : nullptr, *hdr_pack = r.frame == mck::kFrameRpc ? HDR_PACK : nullptr;
            const BatchArgs a = mck::batch_args_of(c, PACK, shift, hdr_pack, msb != 0, ERR);
            CHECK(a.base == (const uint8_t *)SRC && a.offsets == SRC_OFF && a.count == kCount && a.stride == 0);
            CHECK(a.out == r.at40 && a.msgs == r.at40 && a.copy_dst == r.at40);
            CHECK(a.expected == r.at48 && a.dst_offsets == r.at48 && a.rpc_hdr_pack == r.at48);
            CHECK(a.shift == r.at112 && a.rpc_copy_hdr_pack == r.at112);
            CHECK(a.len == r.at24 && a.rpc_pay_off() == r.at24);
            CHECK(a.msg == r.msg && a.pay_off == r.pay_off && a.hash_off == r.hash_off);
            CHECK(a.status == ((r.given & gStatus) ? STATUS : nullptr) && a.mismatches == ((r.given & gMism) ? MISM : nullptr));
            CHECK(a.pack == PACK && a.err_word == ERR && a.queue == nullptr);
            CHECK(a.split_log2 == 0 && a.split_lds == 0);
            CHECK(a.bswap == (msb && r.op == mck::kOpVerify ? 1u : 0u));
        }
        // a payload_offset past 2^32 survives in the RPC calls' 64-bit member (the 32-bit one is the other frames')
        mck::OffsetsCall big = c;
        big.pay_off = (size_t)((1ull << 33) + kPay);
        const BatchArgs a = mck::batch_args_of(big, PACK, nullptr, HDR_PACK, false, ERR);
        CHECK(a.rpc_pay_off() == (r.frame == mck::kFrameRpc ? (1ull << 33) + kPay : 0));
        // the kernel each call's frame leads to: its own frame's, in place the payloads frame's
        mck::LaunchPlan p;
        p.width = 32, p.lg = CRC_GPU_MAX_LOG2G, p.mode = kOffsets;
        const mck::KernelKey k = mck::kernel_key(p, r.op, r.frame);
        CHECK(mck::kernel_key_valid(k) && k.op == r.op);
        CHECK(k.frame == (r.frame == mck::kFrameInPlace ? mck::kFramePayloads : r.frame));
    }
    g_row = "";
    CHECK(sizeof(kRows) / sizeof(kRows[0]) == 13);
    CHECK(frames[mck::kFramePayloads] == 3 && frames[mck::kFrameInPlace] == 4 && frames[mck::kFrameDetached] == 2 &&
          frames[mck::kFrameRpc] == 4);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("%zu call shapes: all checks passed\n", sizeof(kRows) / sizeof(kRows[0]));
    return 0;
}
