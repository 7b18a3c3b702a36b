// launch_plan.h -- which batch kernel a call launches, and how: a pure
// function of the call's shape, the device's CU count and ONE settings
// snapshot (the entry point reads mck_settings() once and passes it down, so
// mchecksum_gpu_reload_settings() on another thread cannot change a launch
// half way through its decisions).  No HIP runtime call, no global: the host
// compiles and checks it on the CPU (tests/native/launch_plan.cpp), down to
// the kernel a plan leads to for the call's operation (BatchOp, kernel_key);
// mchecksum_gpu.hip only turns that key into a function pointer (kernel_for).
#ifndef MCK_LAUNCH_PLAN_H
#define MCK_LAUNCH_PLAN_H

#include <cstddef>
#include <cstdint>

#include "crc_gpu_plan.h"
#include "crc_gpu_shape.h"
#include "mchecksum_models.h"

namespace mck {

// The work queue counts chunk ids and per-workgroup slots in 32 bits
// (crc_gpu_queue.h, WgQueue): 2^31 payloads per call keeps both in range.
constexpr uint64_t kMaxUnits = 1ull << 31;

struct LaunchPlan {
    int width = 0;         // 32 or 64
    int lg = 0;            // log2 lanes per payload (the table pack's), after the count / CU adjustment
    int mode = 0;          // kFixedAligned / kFixedGeneric / kOffsets
    bool light = false;    // small-batch CRC-32C layout
    bool aligned = false;  // mode == kFixedAligned
    bool nt = false;       // the kernel's non-temporal payload loads
    bool split = false;    // CRC-64 payloads as kSplitBytes pieces on the work queue
    uint32_t split_log2 = 0;    // log2 pieces per payload (split only)
    bool split_lds_ok = false;  // split: pieces combine in their workgroup IF the launch gets a slot
    bool zero_out = false;      // split: out[] is zeroed before the launch whether it gets a slot or not
    bool dyn = false;      // takes a work-queue slot (dyn_policy, or split)
    uint64_t units = 0;    // waves' worth of work: payload groups, payloads (offsets) or pieces (split)
    int block = 0, blocks_per_cu = 0;
    unsigned grid = 0;
};

// MCHECKSUM_GPU_LOG2G=g: 2^g lanes per payload for every fixed batch (A/B)
inline bool lg_forced(const mck_settings_t &s) { return s.gpu_log2g >= 0; }
// (the settings parser admits 0..CRC_GPU_MAX_LOG2G only; anything larger in a
// hand-made snapshot reads as the largest, so lg always indexes a pack)
inline int forced_lg(const mck_settings_t &s) { return s.gpu_log2g > CRC_GPU_MAX_LOG2G ? CRC_GPU_MAX_LOG2G : s.gpu_log2g; }

inline int choose_log2g(const mck_settings_t &s, size_t len, int width) {
    if (lg_forced(s)) return forced_lg(s);
    // CRC-32, 1 KiB to under 8 KiB: 16 steps per payload -- 4 lanes at 1 KiB,
    // 8 at 2 KiB, 16 at 4 KiB.  Round 6 timed these shapes on cold lines
    // (4 copies of each batch read in turn, so no launch re-reads what the
    // last one left in the 256 MiB Infinity Cache; tools/ab_variants.py
    // --rotate 4, profiles/r06/ab_lgcold.log): C2's 4 KiB at 16 lanes 50.5 us
    // against 61.6 at 4 (+22%), 2 KiB at 8 lanes +3%; round 4 had chosen 4
    // lanes throughout from back-to-back replays of one batch, which the
    // cache served (-1.9% for 16 lanes there).  From 8 KiB about 32 steps
    // per payload (8 KiB: 16 lanes, 16 KiB: 32 -- both still the best cold),
    // 64 lanes from 32 KiB (the headline).
    if (width == 32 && len >= 1024) {
        if (len < 8192) {
            int lg = 2;
            while (lg < 4 && ((size_t)512 << lg) <= len) lg++;
            return lg;
        }
        int lg = 0;
        while (lg < CRC_GPU_MAX_LOG2G && ((size_t)512 << (lg + 1)) <= len) lg++;
        return lg;
    }
    // CRC-64 (profiles/r04/ab_crc64_log2g.log): about 128 steps per payload,
    // 4 lanes at least -- 4 KiB: 4 lanes -6.9%, 16 KiB: 8 lanes -6.7%, 64 KiB:
    // 32 lanes -3.5% against the >= 16-step rule's 16 / 64 / 64.
    if (width == 64 && len >= 1024) {
        int lg = 2;
        while (lg < CRC_GPU_MAX_LOG2G && ((size_t)2048 << (lg + 1)) <= len) lg++;
        return lg;
    }
    // Otherwise aim for >= 16 steps per payload, at most 64 lanes per payload.
    const size_t target = len / 256;
    int lg = 0;
    while (lg < CRC_GPU_MAX_LOG2G && ((size_t)1 << (lg + 1)) <= target) lg++;
    return lg;
}

// Small batches (<= 16 MiB) take the light CRC-32C layout (16 KiB LDS fill, 256-thread
// workgroups over every CU, 64 lanes per payload): the full layout's 140 KiB
// fill and 1024-thread workgroups cost ~6-12 us per call there
// (profiles/r01/latency.json).  MCHECKSUM_GPU_LIGHT=0/1 overrides.
constexpr uint64_t kLightMaxBytes = 16ull << 20;  // crossover ~24 MiB (latency.json)
inline bool use_light(const mck_settings_t &s, bool small) { return s.gpu_light >= 0 ? s.gpu_light == 1 : small; }

// Lanes per payload for the light layout: as many as keep K >= kRing whole steps.
inline int light_log2g(const mck_settings_t &s, size_t len) {
    if (lg_forced(s)) return forced_lg(s);
    int lg = CRC_GPU_MAX_LOG2G;
    while (lg > 0 && ((size_t)16 << lg) * kRing > len) lg--;
    return lg;
}

// Non-temporal payload loads when the batch is far larger than the 256 MiB
// Infinity Cache (MCHECKSUM_GPU_NT=0/1 overrides).
inline bool use_nt(const mck_settings_t &s, bool large) { return s.gpu_nt >= 0 ? s.gpu_nt == 1 : large; }
inline bool nt_by_bytes(const mck_settings_t &s, uint64_t batch_bytes) { return use_nt(s, batch_bytes >= (512ull << 20)); }
// Offsets and XDR batches: the offsets table stays on the device, so size the
// batch by its count: 8192+ payloads of the C4 mix are ~270 MB and up.
inline bool nt_by_count(const mck_settings_t &s, size_t count) { return use_nt(s, count >= 8192); }

// A receive queue's worth of RPCs: offsets batches up to this many payloads
// take the light layout, XDR batches past it the throughput layout.
constexpr size_t kRecvQueueBatch = 1024;

// Large aligned CRC-64 payloads go to the work queue as kSplitBytes pieces
// (crc64_batch_kernel<..., SPLIT>) once the batch is big enough for the
// non-temporal path; MCHECKSUM_GPU_SPLIT=0/1 overrides.
inline bool use_split(const mck_settings_t &s, int width, int lg, bool aligned, bool nt, size_t len, size_t stride) {
    if (s.gpu_split == 0) return false;
    const bool shape = width == 64 && lg == CRC_GPU_MAX_LOG2G && aligned && len % kSplitBytes == 0 &&
                       len / kSplitBytes >= 2 && len / kSplitBytes <= 64 && ((len / kSplitBytes) & (len / kSplitBytes - 1)) == 0 &&
                       stride % 16 == 0;
    if (s.gpu_split == 1) return shape;
    return shape && nt;
}

// Block size and workgroups per CU of a kernel (Shape<>, crc_gpu_shape.h; it
// does not depend on the lane count).
inline void plan_shape(LaunchPlan &p) {
    if (p.light) {
        p.block = Shape<32, kFixedAligned, true>::block;
        p.blocks_per_cu = Shape<32, kFixedAligned, true>::blocks_per_cu;
    } else if (p.width == 64 && p.mode == kOffsets) {
        p.block = Shape<64, kOffsets>::block;
        p.blocks_per_cu = Shape<64, kOffsets>::blocks_per_cu;
    } else {
        p.block = Shape<32, kFixedAligned>::block;
        p.blocks_per_cu = Shape<32, kFixedAligned>::blocks_per_cu;
    }
}

// Workgroups for p.units waves' worth of work: no more than fit the device at once.
inline unsigned plan_grid(const LaunchPlan &p, int cus) {
    const uint64_t wpb = (uint64_t)p.block / 64;
    uint64_t blocks = (p.units + wpb - 1) / wpb;
    if (blocks > (uint64_t)cus * p.blocks_per_cu) blocks = (uint64_t)cus * p.blocks_per_cu;
    return blocks ? (unsigned)blocks : 1u;
}

// A fixed batch: count payloads of len bytes, stride apart, from base.
inline LaunchPlan plan_fixed(const mck_settings_t &s, int cus, int width, uintptr_t base, size_t stride, size_t len,
                             size_t count) {
    LaunchPlan p;
    p.width = width;
    p.light = width == 32 && use_light(s, (uint64_t)len * count <= kLightMaxBytes);
    if (p.light) {
        p.lg = light_log2g(s, len);
        // light layout: no more lanes per payload than give every CU about
        // four waves (4096 x 4 KiB: 16 lanes -12% against 64; 1024 x 4 KiB
        // keeps 64, profiles/r04/ab_small_knobs.log)
        if (!lg_forced(s))
            while (p.lg > 0 && ((uint64_t)count << (p.lg - 1)) >= (uint64_t)cus * 4 * 64) p.lg--;
    } else {
        p.lg = choose_log2g(s, len, width);
        // a batch too small for the chosen payloads per wave to occupy every wave
        // slot (16 per CU) gets more lanes per payload: 8192 x 4 KiB at 4 lanes
        // ran 2x slower than at 64 (profiles/r04/ab_small_knobs.log)
        if (!lg_forced(s))
            while (p.lg < CRC_GPU_MAX_LOG2G && ((count + (64u >> p.lg) - 1) >> (6 - p.lg)) < (uint64_t)cus * 16) p.lg++;
    }
    const uint64_t step = 16ull << p.lg;
    // The aligned path needs whole steps and K = len/step a multiple of the
    // load ring depth; everything else takes the generic path.
    p.aligned = (base % 16 == 0) && (stride % 16 == 0 || count == 1) && len >= step * kRing &&
                (len % (step * kRing) == 0) && (len >> (4 + p.lg)) < (1ull << 31) && !s.gpu_force_generic;
    p.mode = p.aligned ? kFixedAligned : kFixedGeneric;
    // (only the aligned kernels of the full layout have a non-temporal form)
    const bool nt = !p.light && nt_by_bytes(s, (uint64_t)len * count);
    p.nt = nt && p.aligned;
    while ((kSplitBytes << p.split_log2) < len && p.split_log2 < 63) p.split_log2++;
    p.split = use_split(s, width, p.lg, p.aligned, nt, len, count > 1 ? stride : 16) &&
              ((uint64_t)count << p.split_log2) <= kMaxUnits;
    plan_shape(p);
    if (p.split) {
        p.dyn = true;
        p.units = (uint64_t)count << p.split_log2;
        p.grid = plan_grid(p, cus);
        // With a slot and queue chunks of whole payloads the pieces combine in
        // their workgroup (crc_gpu_crc64.h, split_lds).  Otherwise they XOR
        // their terms into out[], zeroed first.  MCHECKSUM_GPU_SPLIT_LDS=0:
        // always through the zeroed output (tests, A/B).
        p.split_lds_ok = s.gpu_split_lds != 0 && SplitPlan(count, p.split_log2, p.grid).whole();
        p.zero_out = !p.split_lds_ok;
        return p;
    }
    p.split_log2 = 0;
    const uint64_t ppw = 64u >> p.lg;
    p.dyn = dyn_policy(width, p.mode, nt, p.light);
    p.units = (count + ppw - 1) / ppw;
    p.grid = plan_grid(p, cus);
    // CRC-64 static split with fewer units than one full workgroup per CU:
    // one workgroup per unit, at most one per CU (each pays a 66 KiB LDS
    // fill); the kernel then numbers waves across workgroups first
    if (width == 64 && !p.dyn && p.units < (uint64_t)cus * (uint64_t)(p.block / 64))
        p.grid = (unsigned)(p.units < (uint64_t)cus ? (p.units ? p.units : 1) : cus);
    return p;
}

// An offsets, verify or message batch of count payloads: 64 lanes per payload.
inline LaunchPlan plan_offsets(const mck_settings_t &s, int cus, int width, size_t count) {
    LaunchPlan p;
    p.width = width;
    p.lg = CRC_GPU_MAX_LOG2G;
    p.mode = kOffsets;
    // small offsets batches take the light layout
    p.light = width == 32 && use_light(s, count <= kRecvQueueBatch);
    const bool nt = nt_by_count(s, count);
    p.nt = nt && !p.light;  // (the light kernels have no non-temporal form)
    p.dyn = dyn_policy(width, kOffsets, nt, p.light);
    p.units = count;
    plan_shape(p);
    p.grid = plan_grid(p, cus);
    return p;
}

// What a batch call does with each payload's CRC x: the one name an entry
// point gives its call, carried through the host front into the kernels'
// template arguments.  The kernels derive their compile-time variants from it
// (VERIFY = verify or unpack, SEED = update, SEAL = seal or pack, COPY = pack
// or unpack), so a kernel without one of them is the code it was.
enum BatchOp : int {
    // out[p] = x ^ xorout.
    kOpChecksum,
    // Compares instead of storing: status[p], and the launch's count in
    // *mismatches.  verify_offsets compares with expected[p]; verify_messages
    // (kFrameInPlace) with the big-endian hash in the message's header, and a
    // message shorter than its headers fails.
    kOpVerify,
    // Offsets batches, mchecksum_gpu_update_offsets: instead of storing
    // x ^ xorout, the lane that owns payload p advances the running register
    // state[p] (BatchArgs::out) over the payload: state[p] = x ^ Z^n(state[p] ^
    // init), crc_gpu_seed.h.  Only that lane reads or writes state[p]: no
    // atomics, no extra pass.
    kOpUpdate,
    // Message mode, mchecksum_gpu_seal_messages: the mirror of the message
    // verify -- the owning lane stores x ^ xorout big-endian in the message's
    // hash slot (BatchArgs::msgs) instead of
    // comparing it, and status[p] = 1 only for a message shorter than its
    // headers, which is not written.
    kOpSeal,
    // Seal and copy, mchecksum_gpu_pack_messages: payload p comes from the
    // source table (base, offsets) and is also stored behind the headers of
    // message p of the destination (copy_dst, with its message table in
    // dst_offsets), by the payload loop itself; a message that does not fit --
    // its size is not pay_off + the payload's -- gets status 1 and no byte
    // written.
    kOpPack,
    // Verify and copy, mchecksum_gpu_unpack_messages: pack's mirror on the
    // receiver -- payload p of the message table (base, offsets) is also stored
    // at its place in the destination (copy_dst, with its table in dst_offsets), and
    // the owning lane's epilogue is the message verify's; a message whose size
    // is not pay_off + its destination's gets status 1, one mismatch and no
    // byte written.
    kOpUnpack,
};

// What surrounds a payload and where its hash slot is: the one name an entry
// point gives its call's layout, beside the operation, carried through the host
// front (offsets_call.h) into the kernels' template arguments.
enum MsgFrame : int {
    // bare payloads: checksum_offsets, verify_offsets, update_offsets
    kFramePayloads,
    // an HG message, headers then payload in one buffer and one table: verify_messages, seal_messages, and with
    // the payload moved pack_messages, unpack_messages.  A run-time field of the payloads frame's kernels
    // (BatchArgs::msg, pay_off, hash_off): kernel_key folds it, and no key says in-place.
    kFrameInPlace,
    // an overflow RPC: the table (base, offsets) addresses the payloads alone, and the slots are in the eager
    // messages, another buffer (BatchArgs::msgs) with a table of its own (dst_offsets): verify_detached_messages,
    // seal_detached_messages.  The epilogue is kOpVerify's or kOpSeal's, at another address.
    kFrameDetached,
    // a whole RPC message -- core header, flags, HG header, payload -- in one pass (the rules below):
    // verify_rpc_messages, seal_rpc_messages, and with the payload moved unpack_rpc_messages, pack_rpc_messages
    kFrameRpc,
};

// The slot rule of the detached calls (and of state_verify_messages and
// state_seal_messages, which end a streamed pull with the same epilogue):
// message [m0, m1) carries its slot iff it holds hash_off + 4 bytes -- a table
// that runs backwards never does --, and the slot's four bytes start hash_off
// bytes in.  A message without its slot is never read or written: verify
// counts it as a mismatch, seal gives it status 1.
MCK_HOST_DEVICE_INLINE bool msg_slot_ok(uint64_t m0, uint64_t m1, uint64_t hash_off) {
    return m1 >= m0 && m1 - m0 >= hash_off && m1 - m0 - hash_off >= 4;
}
MCK_HOST_DEVICE_INLINE uint64_t msg_slot_at(uint64_t m0, uint64_t hash_off) { return m0 + hash_off; }
// hash_offset is carried in 32 bits (BatchArgs::hash_off), capped as payload_offset is
constexpr uint64_t kMaxHashOff = 1ull << 30;

// The detached calls with both sides by address list (the _detached_message_list
// and _state_*_message_list calls): entry i is `len` bytes at `addr`, anywhere.
// An eager message whose end wraps the address space holds no bytes -- its slot
// rule is then msg_slot_ok(addr, addr + list_msg_len(addr, len), hash_off),
// never true of an empty message, so a message without its slot is never
// dereferenced and its address may be NULL.
MCK_HOST_DEVICE_INLINE uint64_t list_msg_len(uint64_t addr, uint64_t len) { return addr + len >= addr ? len : 0; }
// A payload whose end wraps fails its entry (status 1; a verify's mismatch, no
// store of a seal) and none of it is read: the wave hashes list_payload_len bytes
// at list_payload_at.  The empty payload -- a legitimate one too, whose CRC is
// compared or stored as any other -- runs at address 0, where the
// one-payload-per-wave window has no step (crc_gpu_window.h): its own address is
// never dereferenced and may be NULL.
MCK_HOST_DEVICE_INLINE bool list_payload_ok(uint64_t addr, uint64_t len) { return addr + len >= addr; }
MCK_HOST_DEVICE_INLINE uint64_t list_payload_len(uint64_t addr, uint64_t len) { return list_payload_ok(addr, len) ? len : 0; }
MCK_HOST_DEVICE_INLINE uint64_t list_payload_at(uint64_t addr, uint64_t len) { return list_payload_len(addr, len) ? addr : 0; }

// ---- whole RPC messages: mchecksum_gpu_verify_rpc_messages, _seal_rpc_messages,
// ---- and with the payload copied: _unpack_rpc_messages, _pack_rpc_messages ----
//
// A message is a 16-byte core header (src/mercury_core_header.c:175-289), the
// HG header with the payload hash at hash_off, and from pay_off the payload.
// The core header's CRC-16 runs over the host-order field image, 12 bytes of a
// request and 4 of a response; bit 0 of its flags byte is HG_CORE_MORE_DATA
// (src/mercury_core.h:75): the payload is then elsewhere, and neither hashed
// nor compared here.  The rules below are the kernels' (crc_gpu_crc32.h, kFrameRpc)
// and the CPU's (tests/native/rpc_msg.cpp): the same code.
constexpr uint64_t kRpcHdrBytes = 16;
// (MCHECKSUM_GPU_CORE_HEADER_REQUEST / _RESPONSE and MCHECKSUM_GPU_RPC_*; mchecksum_gpu.hip asserts they agree)
constexpr uint32_t kRpcRequest = 0, kRpcResponse = 1;
enum RpcClass : uint32_t { kRpcOk = 0, kRpcPayload, kRpcHeader, kRpcShort, kRpcDeferred, kRpcFault, kRpcClasses };
// The copying calls' seventh verdict (MCHECKSUM_GPU_COPY_RPC_MISFIT, _CLASSES): eager and whole, but the message
// is not pay_off + the other range's bytes.  Constants of their own: verify and seal keep their six classes.
constexpr uint32_t kRpcMisfit = 6, kRpcCopyClasses = 7;

// A table that runs backwards holds an empty message.
MCK_HOST_DEVICE_INLINE uint64_t rpc_len(uint64_t m0, uint64_t m1) { return m1 >= m0 ? m1 - m0 : 0; }
// Bytes of the hashed image, and where on the wire the flags byte and the big-endian header hash lie.
MCK_HOST_DEVICE_INLINE uint32_t rpc_img_bytes(uint32_t kind) { return kind == kRpcRequest ? 12u : 4u; }
MCK_HOST_DEVICE_INLINE uint32_t rpc_flags_at(uint32_t kind) { return kind == kRpcRequest ? 10u : 1u; }
MCK_HOST_DEVICE_INLINE uint32_t rpc_hash_at(uint32_t kind) { return kind == kRpcRequest ? 12u : 4u; }
// Wire byte j < rpc_img_bytes of the header is byte rpc_img_index of the image:
// the request's id (wire 2..9, big-endian) and the response's cookie (wire
// 2..3) are hashed as little-endian host values, every other field is a byte.
MCK_HOST_DEVICE_INLINE uint32_t rpc_img_index(uint32_t kind, uint32_t j) {
    if (kind == kRpcRequest) return j >= 2 && j < 10 ? 11u - j : j;
    return j >= 2 ? 5u - j : j;
}

// The CRC-16 of so short an image, by position: a CRC register after n bytes
// is Z^n(init) ^ XOR_i Z^(n-1-i)(T[b_i]) (Z: one zero byte, T: the byte table),
// so row[k][b] = Z^k(T[b]) gives each byte's term in ONE lookup and the terms
// XOR together in any order -- sixteen lanes look up a header byte each, where
// a byte-table walk would be twelve dependent loads on one lane for every
// message.  Row kRpcIdRow is the identity: the lanes that hold the hash bytes
// (and the bytes no hash covers) pass theirs through the same lookup.
constexpr uint32_t kRpcIdRow = 12;
struct RpcHdrPack {
    uint16_t row[kRpcIdRow + 1][256];
    uint16_t c;     // Z^n(init) ^ xorout for the kind's n
    uint16_t kind;  // kRpcRequest / kRpcResponse
};
MCK_HOST_DEVICE_INLINE uint32_t rpc_hdr_row(uint32_t kind, uint32_t j) {
    return j < rpc_img_bytes(kind) ? rpc_img_bytes(kind) - 1u - rpc_img_index(kind, j) : kRpcIdRow;
}
// Lane j's term (j < 16): of the CRC-16 if j < rpc_img_bytes, else the wire byte itself.
MCK_HOST_DEVICE_INLINE uint32_t rpc_hdr_term_index(uint32_t kind, uint32_t j, uint32_t byte) {
    return rpc_hdr_row(kind, j) * 256u + (byte & 0xFFu);
}
MCK_HOST_DEVICE_INLINE uint32_t rpc_hdr_term(const RpcHdrPack *pk, uint32_t kind, uint32_t j, uint32_t byte) {
    return (&pk->row[0][0])[rpc_hdr_term_index(kind, j, byte)];
}
// The header's CRC-16 from the XOR of the terms of lanes j < rpc_img_bytes.
MCK_HOST_DEVICE_INLINE uint32_t rpc_hdr_crc(uint32_t c, uint32_t terms) { return (c ^ terms) & 0xFFFFu; }

// The pack of one 16-bit model (poly in normal form, as mck_model_t has it) and kind; both bit orders.
inline void rpc_hdr_pack_build(uint32_t poly, bool reflected, uint32_t init, uint32_t xorout, uint32_t kind, RpcHdrPack *pk) {
    auto reflect16 = [](uint32_t v) {
        uint32_t r = 0;
        for (int i = 0; i < 16; i++) r |= ((v >> i) & 1u) << (15 - i);
        return r;
    };
    const uint32_t rp = reflect16(poly);
    uint16_t T[256];
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t r = reflected ? i : i << 8;
        for (int k = 0; k < 8; k++)
            r = reflected ? (r & 1u ? (r >> 1) ^ rp : r >> 1) : (r & 0x8000u ? (r << 1) ^ poly : r << 1) & 0xFFFFu;
        T[i] = (uint16_t)r;
    }
    auto zero_byte = [&](uint32_t r) { return reflected ? (r >> 8) ^ T[r & 0xFFu] : ((r << 8) ^ T[r >> 8]) & 0xFFFFu; };
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t r = T[b];
        for (uint32_t k = 0; k < kRpcIdRow; k++, r = zero_byte(r)) pk->row[k][b] = (uint16_t)r;
        pk->row[kRpcIdRow][b] = (uint16_t)b;
    }
    uint32_t r = reflected ? reflect16(init) : init & 0xFFFFu;
    for (uint32_t k = 0; k < rpc_img_bytes(kind); k++) r = zero_byte(r);
    pk->c = (uint16_t)(r ^ xorout);
    pk->kind = (uint16_t)kind;
}

// Whether the payload bytes of a message of L bytes are hashed here: the test
// the whole wave makes ahead of its first payload load.  Otherwise the wave
// hashes an empty payload and no byte behind the headers is read.
MCK_HOST_DEVICE_INLINE bool rpc_hashes_payload(uint64_t L, bool more, uint64_t pay_off) {
    return L >= kRpcHdrBytes && !more && L >= pay_off;
}
// The receiver's verdict, first matching rule first.  hdr_ok, more: of a whole
// header only; payload_ok: of a hashed payload only (L < 16 has neither).
MCK_HOST_DEVICE_INLINE uint32_t rpc_verify_class(uint64_t L, bool hdr_ok, bool more, uint64_t pay_off, bool payload_ok) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (!hdr_ok) return kRpcHeader;
    if (more) return kRpcDeferred;
    if (L < pay_off) return kRpcShort;
    return payload_ok ? kRpcOk : kRpcPayload;
}
// The sender's: kRpcOk = both hashes are written, kRpcDeferred = the header's
// alone (the HG slot is seal_detached_messages'), kRpcShort = nothing.
MCK_HOST_DEVICE_INLINE uint32_t rpc_seal_class(uint64_t L, bool more, uint64_t pay_off) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (more) return kRpcDeferred;
    return L < pay_off ? kRpcShort : kRpcOk;
}

// The copying twins (kOpUnpack, kOpPack in kFrameRpc).  R is the length
// of the other range -- the destination's of an unpack, the source's of a pack
// (rpc_len of its table entries: backwards is empty).  Whether the payload is
// copied and hashed: the whole wave's test ahead of its first payload load or
// store.  Otherwise it copies and hashes an empty payload: no byte behind the
// core header is read, none of the other range is read or written, and R is
// not looked at when `more` is set.  The header's verdict does not enter.
MCK_HOST_DEVICE_INLINE bool rpc_copies_payload(uint64_t L, bool more, uint64_t pay_off, uint64_t R) {
    return rpc_hashes_payload(L, more, pay_off) && L - pay_off == R;
}
// The receiver's verdict, first matching rule first.  payload_ok: of a copied payload only.
MCK_HOST_DEVICE_INLINE uint32_t rpc_unpack_class(uint64_t L, bool hdr_ok, bool more, uint64_t pay_off, uint64_t R,
                                                 bool payload_ok) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (!hdr_ok) return kRpcHeader;
    if (more) return kRpcDeferred;
    if (L < pay_off) return kRpcShort;
    if (L - pay_off != R) return kRpcMisfit;
    return payload_ok ? kRpcOk : kRpcPayload;
}
// The sender's: kRpcOk = the payload and both hashes are written, kRpcDeferred
// = the header's hash alone, kRpcShort and kRpcMisfit = nothing.
MCK_HOST_DEVICE_INLINE uint32_t rpc_pack_class(uint64_t L, bool more, uint64_t pay_off, uint64_t R) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (more) return kRpcDeferred;
    if (L < pay_off) return kRpcShort;
    return L - pay_off != R ? kRpcMisfit : kRpcOk;
}

// ---- whole RPC messages in XDR mode: mchecksum_gpu_verify_rpc_xdr_messages,
// ---- _seal_rpc_xdr_messages, _unpack_rpc_xdr_messages, _pack_rpc_xdr_messages ----
//
// The frame above around the XDR walkers (mchecksum_gpu_ext.hip: xdr_message,
// xdr_pack_message): what lies behind pay_off is not hashed as bytes but walked
// by a field schema, so two facts of the walk enter the rules.  `fits`: the
// schema stays inside [pay_off, L) (xdr_decoded_len; the sender's `exact`: the
// schema consumes the image exactly, xdr_encoded_len).  `decoded` / `encoded`:
// the length the pre-walk found for the other side.  Both are of a message the
// walk may touch only (rpc_hashes_payload): every rule that reads them stands
// behind the three that say so, and no byte behind the core header is read for
// a message those three decide.  The kernels' rules and the CPU's
// (tests/native/rpc_xdr_msg.cpp): the same code.
//
// Whether the schema is walked over the message: verify and seal.
MCK_HOST_DEVICE_INLINE bool rpc_xdr_walks(uint64_t L, bool more, uint64_t pay_off) { return rpc_hashes_payload(L, more, pay_off); }
// The receiver's verdict, first matching rule first.  payload_ok: of a message whose schema fits only.
MCK_HOST_DEVICE_INLINE uint32_t rpc_xdr_verify_class(uint64_t L, bool hdr_ok, bool more, uint64_t pay_off, bool fits,
                                                     bool payload_ok) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (!hdr_ok) return kRpcHeader;
    if (more) return kRpcDeferred;
    if (L < pay_off || !fits) return kRpcShort;  // shorter than its headers, or than its own fields need
    return payload_ok ? kRpcOk : kRpcPayload;
}
// The sender's in place: kRpcOk = both hashes are written, kRpcDeferred = the header's alone, kRpcShort = nothing.
MCK_HOST_DEVICE_INLINE uint32_t rpc_xdr_seal_class(uint64_t L, bool more, uint64_t pay_off, bool fits) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (more) return kRpcDeferred;
    return L < pay_off || !fits ? kRpcShort : kRpcOk;
}
// unpack: whether the destination range (R bytes) is written, and the fields hashed.  The header's verdict does not enter.
MCK_HOST_DEVICE_INLINE bool rpc_xdr_unpacks(uint64_t L, bool more, uint64_t pay_off, bool fits, uint64_t decoded, uint64_t R) {
    return rpc_hashes_payload(L, more, pay_off) && fits && decoded == R;
}
MCK_HOST_DEVICE_INLINE uint32_t rpc_xdr_unpack_class(uint64_t L, bool hdr_ok, bool more, uint64_t pay_off, bool fits,
                                                     uint64_t decoded, uint64_t R, bool payload_ok) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (!hdr_ok) return kRpcHeader;
    if (more) return kRpcDeferred;
    if (L < pay_off || !fits) return kRpcShort;
    if (decoded != R) return kRpcMisfit;
    return payload_ok ? kRpcOk : kRpcPayload;
}
// pack: whether the image is read and its XDR bytes written.  exact, encoded: of the image, the source range.
MCK_HOST_DEVICE_INLINE bool rpc_xdr_packs(uint64_t L, bool more, uint64_t pay_off, bool exact, uint64_t encoded) {
    return rpc_hashes_payload(L, more, pay_off) && exact && L - pay_off == encoded;
}
MCK_HOST_DEVICE_INLINE uint32_t rpc_xdr_pack_class(uint64_t L, bool more, uint64_t pay_off, bool exact, uint64_t encoded) {
    if (L < kRpcHdrBytes) return kRpcShort;
    if (more) return kRpcDeferred;
    if (L < pay_off) return kRpcShort;
    return !exact || L - pay_off != encoded ? kRpcMisfit : kRpcOk;
}

// The message side by address list (the _rpc_xdr_message_list calls): entry i
// is `len` bytes at `addr`, anywhere.  The frame a wave takes from the entry:
// L, with the list rule above (an end past the address space holds no bytes),
// and the address it may touch -- 0 for a message without a whole core header,
// of which the ladders read no byte (rule 1), so that entry's address forms no
// pointer and may be NULL.  From 16 bytes on the core header is read, and what
// lies behind it only where rpc_xdr_walks / _unpacks / _packs say so, as in the
// table form.  The walkers run over [at, at + L) from base 0; at + L never wraps.
MCK_HOST_DEVICE_INLINE uint64_t rpc_xdr_list_len(uint64_t addr, uint64_t len) { return list_msg_len(addr, len); }
MCK_HOST_DEVICE_INLINE uint64_t rpc_xdr_list_at(uint64_t addr, uint64_t len) {
    return rpc_xdr_list_len(addr, len) >= kRpcHdrBytes ? addr : 0;
}

// One instantiation of the batch kernels (crc32c_batch_kernel,
// crc64_batch_kernel): what kernel_for (mchecksum_gpu.hip) looks up.
struct KernelKey {
    int width, lg, mode, op;
    bool nt, light, split;
    MsgFrame frame = kFramePayloads;
    // the message side by address list (the _rpc_message_list calls): message p is the len[p] bytes at address
    // addr[p], where the table form has buf[off[p], off[p + 1]).  Twins of the RPC frame's kernels, no others.
    bool list = false;
    // both sides by address list (the _detached_message_list calls): payload p is the len[p] bytes at its
    // address, and its slot lies in the eager message at an address with a length of its own.  Twins of the
    // detached frame's six kernels, no others; never together with `list`, which names the RPC frame's.
    bool both_lists = false;
};
constexpr bool operator==(const KernelKey &a, const KernelKey &b) {
    return a.width == b.width && a.lg == b.lg && a.mode == b.mode && a.op == b.op && a.nt == b.nt && a.light == b.light &&
           a.split == b.split && a.frame == b.frame && a.list == b.list && a.both_lists == b.both_lists;
}

// The instantiations there are -- kernel_for has exactly these, and each
// kernel asserts it is one of them.
constexpr bool kernel_key_valid(const KernelKey &k) {
    if ((k.width != 32 && k.width != 64) || k.lg < 0 || k.lg > CRC_GPU_MAX_LOG2G) return false;
    if (k.light && (k.width != 32 || k.nt)) return false;  // light: CRC-32C only, and no non-temporal form
    const bool checks = k.op == kOpVerify || k.op == kOpSeal, copies = k.op == kOpPack || k.op == kOpUnpack;
    if (k.list && k.frame != kFrameRpc) return false;  // the list form: of whole RPC messages only (all twelve)
    if (k.both_lists && (k.frame != kFrameDetached || k.list)) return false;  // of the detached frame only (all six)
    switch (k.frame) {
        case kFramePayloads: break;
        // twins of the CRC-32C offsets kernels (light, full, non-temporal), never split: a detached verify or
        // seal; an RPC verify, seal, pack or unpack
        case kFrameDetached:
        case kFrameRpc:
            if (k.width != 32 || k.mode != kOffsets || k.split) return false;
            if (!checks && !(k.frame == kFrameRpc && copies)) return false;
            break;
        default: return false;  // in place is the payloads frame's kernels (kernel_key)
    }
    if (k.split)  // pieces of aligned CRC-64 payloads, 64 lanes each: checksums only
        return k.width == 64 && k.mode == kFixedAligned && k.lg == CRC_GPU_MAX_LOG2G && k.op == kOpChecksum;
    switch (k.mode) {
        case kFixedAligned: return k.op == kOpChecksum;
        case kFixedGeneric: return k.op == kOpChecksum && !k.nt;  // no non-temporal form
        case kOffsets: break;
        default: return false;
    }
    if (k.lg != CRC_GPU_MAX_LOG2G) return false;  // offsets batches: one payload per wave
    switch (k.op) {
        case kOpChecksum:
        case kOpVerify:
        case kOpUpdate: return true;
        case kOpSeal:
        case kOpPack:
        case kOpUnpack: return k.width == 32;  // the HG header carries a 32-bit hash
        default: return false;
    }
}

// The kernel a plan launches for op.  A plan's fields say what the batch is
// like; the key drops what the kernel in question has no form for.
inline KernelKey kernel_key(const LaunchPlan &p, BatchOp op, MsgFrame frame = kFramePayloads, bool list = false,
                            bool both_lists = false) {
    KernelKey k{p.width, p.lg, p.mode, op, p.nt, p.light, p.split, frame == kFrameInPlace ? kFramePayloads : frame, list,
                both_lists};
    if (p.split) k.width = 64, k.lg = CRC_GPU_MAX_LOG2G, k.mode = kFixedAligned, k.light = false;
    if (k.mode == kOffsets) k.lg = CRC_GPU_MAX_LOG2G;
    if (k.width != 32) k.light = false;
    if (k.light || k.mode == kFixedGeneric) k.nt = false;
    return k;
}

}  // namespace mck

#endif  // MCK_LAUNCH_PLAN_H
