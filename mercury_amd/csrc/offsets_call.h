// offsets_call.h -- one offsets-shaped batch call as its entry point names it
// (OffsetsCall), what such a call must supply (offsets_needs) and the kernel
// argument it becomes (batch_args_of).  Pure functions of the call: no HIP
// runtime call, no global, so the CPU checks every entry point's call shape
// (tests/native/offsets_call.cpp).  mchecksum_gpu.hip's offsets_call keeps the
// order of the checks, the error texts, the model, the device and the launch.
#ifndef MCK_OFFSETS_CALL_H
#define MCK_OFFSETS_CALL_H

#include <cstddef>
#include <cstdint>

#include "launch_plan.h"

namespace mck {

// The payloads (or, in a frame with headers, the messages that hold them) lie
// at src by the table src_off.
struct OffsetsCall {
    BatchOp op;
    const char *method;
    const void *src;
    const uint64_t *src_off;
    size_t count;
    MsgFrame frame = kFramePayloads;
    void *out = nullptr;             // checksum: the CRCs; update: the running registers; seal (in place, RPC): src, writable
    void *dst = nullptr;             // pack, unpack: where the payloads are copied to, by the table dst_off
    const uint64_t *dst_off = nullptr;
    const void *expected = nullptr;  // verify_offsets
    uint8_t *status = nullptr;
    uint32_t *mismatches = nullptr;  // RPC verify: the six class counts, RPC unpack: the seven
    size_t pay_off = 0, hash_off = 0;  // payload_offset, hash_offset of the frames with headers
    void *stream = nullptr;
    // kFrameDetached: src holds the payloads alone, and the hash slots lie hash_off bytes into the eager
    // messages hdr[hdr_off[i], hdr_off[i + 1])
    void *hdr = nullptr;
    const uint64_t *hdr_off = nullptr;
    // kFrameRpc: the core header's kind and its 16-bit method.  The buffers are the in-place frame's: an unpack's
    // messages at src, a pack's at dst.
    int kind = 0;
    const char *hdr_method = nullptr;
    // kFrameRpc by address list: the message side -- src_off, a pack's dst_off -- holds `count` absolute addresses
    // and msg_len their lengths; that side's buffer pointer (src, a pack's dst, a seal's out) is null
    bool list = false;
    const uint64_t *msg_len = nullptr;
    // kFrameDetached with both sides by address list: src_off holds the payloads' addresses and payload_len their
    // lengths, hdr_off the eager messages' addresses and msg_len theirs; src and hdr are null
    bool both_lists = false;
    const uint64_t *payload_len = nullptr;
};

constexpr bool op_copies(BatchOp op) { return op == kOpPack || op == kOpUnpack; }

// What a non-empty call must supply besides src and src_off, and whether its
// method is checked ahead of the device, as an argument (the calls on HG and
// RPC messages but verify_messages; as verify_core_headers does) or after it.
// A list call needs its lengths, and no buffer for its message side: src_buf and dst_buf say which of the
// two buffer pointers a call still needs (both, but for a list), and a list seal writes through its addresses.
struct OffsetsNeeds {
    bool out, dst, hdr, expected, method_first;
    bool msg_len = false, src_buf = true, dst_buf = true;
    bool payload_len = false, hdr_buf = true;  // both sides by list: a second lengths array, and no buffer under either
};
constexpr OffsetsNeeds offsets_needs(BatchOp op, MsgFrame frame, bool list = false, bool both_lists = false) {
    return {op == kOpChecksum || op == kOpUpdate || (op == kOpSeal && frame != kFrameDetached && !list),  // values or hashes stored
            op_copies(op), frame == kFrameDetached, op == kOpVerify && frame == kFramePayloads,
            op_copies(op) || op == kOpSeal || frame == kFrameDetached || frame == kFrameRpc,
            list || both_lists, !(list || both_lists) || op == kOpPack, !list || op != kOpPack,
            both_lists, !both_lists};
}
// Whether a call lacks a pointer it must supply: an empty batch needs no buffers (not even the one-entry table).
inline bool offsets_lacks_pointer(const OffsetsCall &c) {
    const OffsetsNeeds need = offsets_needs(c.op, c.frame, c.list, c.both_lists);
    return c.count && ((need.src_buf && !c.src) || !c.src_off || (need.out && !c.out) ||
                       (need.dst && ((need.dst_buf && !c.dst) || !c.dst_off)) ||
                       (need.hdr && ((need.hdr_buf && !c.hdr) || !c.hdr_off)) || (need.expected && !c.expected) ||
                       (need.msg_len && !c.msg_len) || (need.payload_len && !c.payload_len));
}

// The kernels' argument of a call: pack = the model's table pack, shift = its
// Z^n pack (an update's, else null), hdr_pack = the header model's (kFrameRpc,
// else null), msb = an MSB-first model.  The launch adds the queue slot.
inline BatchArgs batch_args_of(const OffsetsCall &c, const void *pack, const void *shift, const void *hdr_pack, bool msb,
                               uint32_t *err_word) {
    BatchArgs a{};
    a.base = (const uint8_t *)c.src;
    a.offsets = c.src_off;
    a.count = c.count;
    a.shift = shift;
    if (op_copies(c.op)) {
        a.copy_dst = (uint8_t *)c.dst;
        a.dst_offsets = c.dst_off;
        if (c.frame == kFrameRpc) a.rpc_copy_hdr_pack = hdr_pack;
    } else if (c.frame == kFrameDetached) {
        a.msgs = (uint8_t *)c.hdr;
        a.dst_offsets = c.hdr_off;
    } else {
        a.out = c.out;
        if (c.frame == kFrameRpc) a.rpc_hdr_pack = hdr_pack;
        else a.expected = c.expected;
    }
    if (c.frame == kFrameRpc) a.set_rpc_pay_off(c.pay_off);
    if (c.list) {
        // the list's entries are whole addresses: the kernels add them to a null buffer pointer, whatever the call holds
        a.set_rpc_list_len(c.msg_len);
        if (c.op == kOpPack) a.copy_dst = nullptr;
        else a.base = nullptr;
        if (c.op == kOpSeal) a.msgs = nullptr;
    }
    if (c.both_lists) {
        // both tables' entries are whole addresses: null buffers whatever the call holds, and a length array each
        a.set_rpc_list_len(c.payload_len);
        a.set_slot_list_len(c.msg_len);
        a.base = nullptr;
        a.msgs = nullptr;
    }
    a.status = c.status;
    a.mismatches = c.mismatches;
    a.pack = pack;
    a.msg = c.frame == kFrameInPlace ? 1u : 0u;
    a.pay_off = (uint32_t)c.pay_off;
    a.hash_off = (uint32_t)c.hash_off;
    a.err_word = err_word;
    a.bswap = c.op == kOpVerify && msb ? 1u : 0u;  // checksum calls swap after the launch
    return a;
}

}  // namespace mck

#endif  // MCK_OFFSETS_CALL_H
