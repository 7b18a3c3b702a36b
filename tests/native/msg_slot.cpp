// The slot rule of the detached message calls (mercury_amd/csrc/launch_plan.h:
// msg_slot_ok, msg_slot_at) against a naive model that walks the message byte
// by byte: which messages carry their four hash bytes, where those bytes are,
// and that a sealing or verifying lane that follows the rule touches exactly
// them -- never a byte past a short message's end.  Message lengths 0 ..
// hash_offset + 8, hash_offset in {0, 1, 16, 17}, every start residue mod 16,
// and tables that run backwards.  Stand-alone: plain and under the sanitizers
// (tests/test_msg_slot.py).
#include <cstdint>
#include <cstdio>
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

// the rule as the contract words it: the slot is the bytes hash_off .. hash_off + 3
// of the message, and each of them must be one of the message's bytes
bool naive_ok(uint64_t len, uint64_t hash_off) {
    for (uint64_t b = hash_off; b < hash_off + 4; b++)
        if (b >= len) return false;
    return true;
}

// what the owning lane does (crc_gpu_common.h: load_be32, store_be32), on host memory
uint32_t load_be32(const uint8_t *q) {
    return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3];
}
void store_be32(uint8_t *q, uint32_t v) {
    q[0] = (uint8_t)(v >> 24);
    q[1] = (uint8_t)(v >> 16);
    q[2] = (uint8_t)(v >> 8);
    q[3] = (uint8_t)v;
}

}  // namespace

int main() {
    const uint64_t hash_offs[] = {0, 1, 16, 17};
    unsigned long long msgs = 0, with_slot = 0, without = 0;
    for (uint64_t ho : hash_offs)
        for (uint64_t len = 0; len <= ho + 8; len++)
            for (uint64_t start = 0; start < 16; start++) {
                // the message alone in an exactly sized allocation after `start`
                // bytes of another message: a byte past its end is the sanitizer's
                std::vector<uint8_t> buf(start + len);
                for (size_t i = 0; i < buf.size(); i++) buf[i] = (uint8_t)(0x40 + i);
                const std::vector<uint8_t> before = buf;
                const uint64_t m0 = start, m1 = start + len;
                const bool ok = mck::msg_slot_ok(m0, m1, ho);
                CHECK(ok == naive_ok(len, ho));
                CHECK(ok == (len >= ho + 4));
                msgs++;
                (ok ? with_slot : without)++;
                if (!ok) continue;  // no byte of a message without a slot is touched
                const uint64_t at = mck::msg_slot_at(m0, ho);
                CHECK(at == start + ho && at + 4 <= m1);
                const uint32_t v = 0xA1B2C3D4u ^ (uint32_t)(len * 16 + start);
                store_be32(buf.data() + at, v);
                CHECK(load_be32(buf.data() + at) == v);
                CHECK(buf[at] == (uint8_t)(v >> 24) && buf[at + 3] == (uint8_t)v);  // network order
                for (uint64_t i = 0; i < buf.size(); i++)
                    if (i < at || i >= at + 4) CHECK(buf[i] == before[i]);
            }
    // a table that runs backwards carries no slot, whatever the distance
    CHECK(!mck::msg_slot_ok(100, 99, 0));
    CHECK(!mck::msg_slot_ok(~0ull, 3, 0));  // m1 - m0 wraps to 4
    CHECK(!mck::msg_slot_ok(10, 5, 16));
    // the largest hash_offset a call admits, and lengths around it
    CHECK(mck::kMaxHashOff == 1ull << 30);
    CHECK(mck::msg_slot_ok(7, 7 + mck::kMaxHashOff + 4, mck::kMaxHashOff));
    CHECK(!mck::msg_slot_ok(7, 7 + mck::kMaxHashOff + 3, mck::kMaxHashOff));
    CHECK(mck::msg_slot_at(7, mck::kMaxHashOff) == 7 + mck::kMaxHashOff);
    // messages high in the address space: no wrap in the rule
    CHECK(mck::msg_slot_ok(~0ull - 20, ~0ull, 16));
    CHECK(!mck::msg_slot_ok(~0ull - 19, ~0ull, 16));
    // the kernels there are for the detached calls: light, full, non-temporal, verify and seal
    int n = 0;
    for (int op = -1; op <= mck::kOpUnpack + 1; op++)
        for (int width : {32, 64})
            for (int mode = 0; mode <= kOffsets; mode++)
                for (int f = 0; f < 8; f++) {
                    const mck::KernelKey k{width, CRC_GPU_MAX_LOG2G, mode, op, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, mck::kFrameDetached};
                    if (!mck::kernel_key_valid(k)) continue;
                    n++;
                    CHECK(width == 32 && mode == kOffsets && !k.split && !(k.nt && k.light));
                    CHECK(op == mck::kOpVerify || op == mck::kOpSeal);
                    // its sibling in place: the payloads frame's kernel (kernel_key folds kFrameInPlace into it)
                    mck::KernelKey in_place = k;
                    in_place.frame = mck::kFramePayloads;
                    CHECK(mck::kernel_key_valid(in_place) && !(in_place == k));
                }
    CHECK(n == 6);
    {
        // kernel_key(plan, op, frame) yields them, and kernel_key(plan, op) does not
        mck::LaunchPlan p;
        p.width = 32, p.lg = CRC_GPU_MAX_LOG2G, p.mode = kOffsets;
        for (mck::BatchOp op : {mck::kOpVerify, mck::kOpSeal}) {
            const mck::KernelKey k = mck::kernel_key(p, op, mck::kFrameDetached);
            CHECK(mck::kernel_key_valid(k) && k.frame == mck::kFrameDetached && k.op == op);
            CHECK(mck::kernel_key(p, op).frame == mck::kFramePayloads);
        }
    }
    std::printf("%llu messages: %llu with a slot, %llu without\n", msgs, with_slot, without);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
