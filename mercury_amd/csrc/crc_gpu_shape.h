// crc_gpu_shape.h -- launch shapes of the batch kernels: block sizes, ring
// depths, LDS maps, Shape<>, the kernels' argument struct and the work-queue
// layout constants.  Plain C++ compiles it (no HIP header): the host's launch
// plan (launch_plan.h) and its CPU tests read the same numbers as the kernels.
#ifndef CRC_GPU_SHAPE_H
#define CRC_GPU_SHAPE_H

#include <cstdint>

#include "crc_gpu_layout.h"

// (crc_gpu_mask.h's MCK_HD pattern, for constexpr functions and members;
// spelled without __forceinline__, which only <hip/hip_runtime.h> defines, so
// hipcc too compiles these headers on their own)
#if defined(__HIPCC__)
#    define MCK_HOST_DEVICE __host__ __device__
#    define MCK_HOST_DEVICE_INLINE __host__ __device__ inline __attribute__((always_inline))
#else
#    define MCK_HOST_DEVICE
#    define MCK_HOST_DEVICE_INLINE inline
#endif

namespace {

// Tuning constants are the measured best (their A/Bs: DESIGN.md and
// HISTORY.md; losing alternatives are not kept in the source).
constexpr int kBlock = 1024;  // 16 waves: 4 per SIMD
constexpr int kRing = 4;      // dwordx4 pieces in flight per lane
// Offsets batches (one payload per wave, ~32 KiB average) want a deeper ring:
// 8 measured +4% over 4 on C4, while 8 costs 1-5% on the aligned batches.
constexpr int kRingOff = 8;

// CRC-32C LDS map: [0,128K) main byte tables x32 copies; then op nibble
// tables; then the two-level combine operators (crc_gpu_layout.h lv, 8 KiB).
constexpr uint32_t kL32Main = 131072;
constexpr uint32_t kL32Lv = kL32Main + CRC32_NOPS_MAX * 512;
constexpr uint32_t kL32Bytes = kL32Lv + 2 * 8 * 16 * 8 * 4;
// Light layout for small batches: the 4 byte tables unreplicated (4 KiB, so
// the per-workgroup LDS fill is 16 KiB instead of 140 KiB) and 256-thread
// workgroups spread over every CU; lookups may bank-conflict, which a small
// batch never notices.
constexpr uint32_t kL32LightMain = 4096;
constexpr uint32_t kL32LightBytes = kL32LightMain + CRC32_NOPS_MAX * 512;
constexpr int kLightBlock = 256;

// CRC-64 LDS map.  A 64-bit word is looked up in 12 tables (pack f5 / f6,
// crc_gpu_layout.h): bits 3..7 of each of its 8 bytes index a 32-entry table
// at 8-B stride -- one 256-B row, entry v on bank pair v, so distinct entries
// never share a bank and equal ones broadcast: conflict-free without lane
// copies, and the address is (byte & 0xF8) itself --, and bits 0..2 of bytes i
// and i + 4, gathered into one 6-bit index by one shift + bit-select for all
// four, index a 64-entry table replicated 32x (entry v at v*256 B + lane copy
// (lane % 32)*8: 16 KiB per table).  Then the combine operators (16 nibble
// tables, 2 KiB each).  (Round 1's 16-lookup nibble form needed a third more
// LDS reads; 11 lookups over 7-bit tables, a wide-row map with cheaper address
// ops and two workgroups per CU all measured slower: HISTORY.md.)
constexpr uint32_t kL64P5 = 0;
constexpr uint32_t kL64P6 = 8 * 256;
constexpr uint32_t kL64Main = kL64P6 + 4 * 16384;
constexpr uint32_t kL64Bytes = kL64Main + CRC64_NOPS_MAX * 2048;
// Where the CRC-64 combine operators live: all in LDS (one 1024-thread
// workgroup per CU: the aligned batches and the merged segment pass), all in
// global memory (the XDR throughput kernel), or the six butterflies
// Z^-(16*2^k) in LDS and Z^-8 and the tail operators -- the two ends of the
// offsets path's dependent chain -- in global memory (the offsets path: two
// workgroups per CU at 79.9 KiB each, +6-8% on C4-layout CRC-64 over either
// pure form, profiles/r01/ab20_crc64_offsets_mix.log).
enum OpsMode : int { kOpsLds = 0, kOpsGlobal = 1, kOpsMix = 2 };

// Launch shape per kernel.  CRC-32C: one 1024-thread workgroup per CU (the
// replicated tables take 140 KiB), or the light layout's 256-thread
// workgroups, 8 per CU.  CRC-64 aligned and generic fixed batches: one
// 1024-thread workgroup per CU with every operator in LDS (round 4: C3 -2.6%
// in time against two workgroups per CU with the operators in global memory,
// profiles/r04/ab_c3_onewg.log).  CRC-64 offsets batches: two workgroups per
// CU, the mixed operator placement and a 4-deep ring so the loop fits 64
// VGPRs (a ring of 8 at two workgroups spills: -42%).
template <int W, int MODE, bool LIGHT = false, int LG = -1>
struct Shape {
    static constexpr bool two = W == 64 && MODE == 2;
    static constexpr int block = LIGHT ? kLightBlock : kBlock;
    static constexpr int blocks_per_cu = LIGHT ? 8 : two ? 2 : 1;
    static constexpr int ops_mode = two ? kOpsMix : kOpsLds;
    static constexpr uint32_t lds64_bytes = two ? kL64Main + 6 * 2048 : kL64Bytes;
};
constexpr int kRingOff64 = 4;
// single-argument aliases keyed MODE * 16 + LOG2G (a comma inside
// __launch_bounds__ splits the macro)
template <int KEY>
constexpr int kBlk64 = Shape<64, KEY / 16, false, KEY % 16>::block;
template <int KEY>
constexpr int kWpe64 = Shape<64, KEY / 16, false, KEY % 16>::blocks_per_cu * Shape<64, KEY / 16, false, KEY % 16>::block / 256;

enum Mode : int { kFixedAligned = 0, kFixedGeneric = 1, kOffsets = 2 };

// The kernels' argument.  One layout for every batch call: a field that a kind
// of call has no use for carries what that kind needs instead, as a named
// member of an anonymous union at the same offset -- host and kernels use the
// name that says what they mean (the host side: offsets_call.h, batch_args_of).
struct BatchArgs {
    const uint8_t *base;
    const uint64_t *offsets;
    uint64_t stride;
    // whole RPC messages by address list (kFrameRpc, KernelKey::list): the lengths array, in `stride`'s place -- no
    // offsets-mode kernel has a stride.  (An accessor, for the reason below.)
    MCK_HOST_DEVICE const uint64_t *rpc_list_len() const { return reinterpret_cast<const uint64_t *>(stride); }
    MCK_HOST_DEVICE void set_rpc_list_len(const uint64_t *v) { stride = reinterpret_cast<uint64_t>(v); }
    // The detached calls with both sides by list (kFrameDetached, KernelKey::both_lists) carry the PAYLOADS' lengths
    // there, and the eager messages' lengths in `len`'s place -- a detached call has no fixed length.
    MCK_HOST_DEVICE const uint64_t *slot_list_len() const { return reinterpret_cast<const uint64_t *>(len); }
    MCK_HOST_DEVICE void set_slot_list_len(const uint64_t *v) { len = reinterpret_cast<uint64_t>(v); }
    uint64_t len;  // fixed batches: bytes per payload
    // whole RPC messages (kFrameRpc): payload_offset in 64 bits, in `len`'s place.  (An accessor, not a member of a
    // union as below: a union here moved an instruction in every fixed generic CRC-32C kernel.)
    MCK_HOST_DEVICE uint64_t rpc_pay_off() const { return len; }
    MCK_HOST_DEVICE void set_rpc_pay_off(uint64_t v) { len = v; }
    uint64_t count;
    union {
        void *out;          // the CRCs; update: the running registers, one per payload, advanced in place
        uint8_t *msgs;      // the messages, writable: `base` again (a seal in place, of RPC messages), the eager
                            // messages of the detached calls (a verify only reads them), an RPC pack's (= copy_dst)
        uint8_t *copy_dst;  // pack and unpack: where the payloads go, by the table dst_offsets
    };
    union {
        const void *expected;         // verify_offsets: the expected CRCs
        const uint64_t *dst_offsets;  // the table of the other buffer: copy_dst's, the detached calls' msgs'
        const void *rpc_hdr_pack;     // RPC verify and seal: the header model's pack (launch_plan.h, RpcHdrPack)
    };
    uint8_t *status;
    uint32_t *mismatches;
    const void *pack;
    // message mode (kFrameInPlace): payload i = [offsets[i] + pay_off,
    // offsets[i+1]), its CRC the big-endian u32 at offsets[i] + hash_off
    uint32_t msg, pay_off, hash_off;
    // work-queue slot (WgQueue, crc_gpu_queue.h), exclusive to this launch's stream;
    // nullptr = static assignment
    unsigned long long *queue;
    // optional caller word (mchecksum_gpu_set_error_word): +1 when this launch
    // could not hash every payload (fail-closed report for checksum modes)
    uint32_t *err_word;
    union {
        // the Z^n shift pack: recombines the 2^split_log2 pieces of kSplitBytes of a split CRC-64 payload
        // (crc64_batch_kernel<..., SPLIT>), advances the running registers of an update (kOpUpdate)
        const void *shift;
        const void *rpc_copy_hdr_pack;  // RPC pack and unpack: the header pack (their dst_offsets is in use)
    };
    uint32_t split_log2;
    // MSB-first model on a verify call: the kernel's value is the CRC
    // byte-swapped (crc_gpu_layout.h), so swap before comparing
    uint32_t bswap;
    // split CRC-64: 1 = every queue chunk holds whole payloads (SplitPlan::whole),
    // so the pieces combine in the workgroup's LDS and out[] needs no zeroing
    uint32_t split_lds;
};
// The layout is the kernels' kernarg: pinned here, not by prose.
#define MCK_AT(S, m, o) static_assert(__builtin_offsetof(S, m) == o, #S "::" #m " moved")
MCK_AT(BatchArgs, base, 0);
MCK_AT(BatchArgs, offsets, 8);
MCK_AT(BatchArgs, stride, 16);
MCK_AT(BatchArgs, len, 24);
MCK_AT(BatchArgs, count, 32);
MCK_AT(BatchArgs, out, 40);
MCK_AT(BatchArgs, msgs, 40);
MCK_AT(BatchArgs, copy_dst, 40);
MCK_AT(BatchArgs, expected, 48);
MCK_AT(BatchArgs, dst_offsets, 48);
MCK_AT(BatchArgs, rpc_hdr_pack, 48);
MCK_AT(BatchArgs, status, 56);
MCK_AT(BatchArgs, mismatches, 64);
MCK_AT(BatchArgs, pack, 72);
MCK_AT(BatchArgs, msg, 80);
MCK_AT(BatchArgs, pay_off, 84);
MCK_AT(BatchArgs, hash_off, 88);
MCK_AT(BatchArgs, queue, 96);
MCK_AT(BatchArgs, err_word, 104);
MCK_AT(BatchArgs, shift, 112);
MCK_AT(BatchArgs, rpc_copy_hdr_pack, 112);
MCK_AT(BatchArgs, split_log2, 120);
MCK_AT(BatchArgs, bswap, 124);
MCK_AT(BatchArgs, split_lds, 128);
static_assert(sizeof(BatchArgs) == 136 && alignof(BatchArgs) == 8, "BatchArgs changed size");
// Piece size of a split payload: 256 KiB = 256 steps of the G = 64 loop.
// (A/B, round 4: 128 KiB pieces +2.9%, 512 KiB +6.8% on C3 time, profiles/r04/ab_split_piece.log)
constexpr uint64_t kSplitBytes = 256u << 10;
// Payloads per queue chunk whose pieces a workgroup can combine in LDS, and
// the accumulator sets (chunks with pieces in flight) it keeps.
constexpr uint32_t kSplitAcc = 16;
constexpr uint32_t kAccSets = 32;

// ------------------------------------------------------------ work queue --
// Layout of a work-queue slot and the chunk sizes (the protocol itself, its
// banks and who may use a slot: crc_gpu_queue.h; the chunk plan: crc_gpu_plan.h).
constexpr uint32_t kQSub = 8;
constexpr uint32_t kQStride = 32;  // u64 words between counters
constexpr uint32_t kQFault = kQSub;
constexpr uint32_t kQAbort = kQSub + 1;
constexpr uint32_t kQBankLines = kQAbort + 1;  // protocol lines, zeroed before the bank's next use
constexpr uint64_t kQBankBytes = 8192;
constexpr uint32_t kQBankWords = (uint32_t)(kQBankBytes / 8);
constexpr uint32_t kQSlotWords = 2 * kQBankWords;  // slots 2 * kQBankBytes aligned: bank ^ kQBankBytes = the other
static_assert(kQBankLines * kQStride <= kQBankWords, "bank overflow");
// Chunk size: a power of two, about a quarter of a workgroup's fair share
// of units, between 1 and 32 (C4: 32 units; a 5000-payload batch: 4).
// Fixed 16 starved half the workgroups of C3's 8192 units at 2 WGs per CU; 32
// beat 16 on the large batches.  The next chunk is fetched when a quarter of
// the current one is left to take: early enough to hide the fetch (~1.3 us
// mean), late enough that a workgroup holds little unstarted work when the
// queue runs dry.
constexpr uint32_t kWgChunkMaxLog2 = 5;
// Which batches take the queue (profiles/r01/ab12_work_queue.log, medians
// vs the static split): variable-length (offsets) batches, +4% C4 and +8%
// C4-layout CRC-64 over the byte-balanced static split, and the large
// (non-temporal, >= 512 MiB) aligned CRC-32C batches, +2.3% on the headline.
// Smaller fixed batches and CRC-64 fixed batches keep the static stride:
// there the queue's fixed costs outweigh the balance (C2 -11% warm, -14%
// with cold lines, profiles/r06/ab_c2cold.log; 2 KiB -16% and 8/16 KiB
// +-0.3% at the round-6 lane counts, profiles/r06/ab_c2dyn.log; C3 -5%).
MCK_HOST_DEVICE constexpr bool dyn_policy(int width, int mode, bool nt, bool light) {
    return !light && (mode == 2 || (width == 32 && nt && mode == 0));  // 2 = kOffsets
}

// Tail chunks are 2^-kQTailShift of a full one, over the last full chunk per
// workgroup.  Eighths since round 4 (quarters before): never slower in two
// one-process A/Bs, headline -0.4% / -0.6%, C3 -0.7%, seg -0.7%, C4 +-0 in
// time (profiles/r04/ab_qtail.log, ab_round4_knobs.log: "t3"); single-unit
// tail chunks lost 2.3% on C4 (one fetch per unit), two full chunks per
// workgroup of tail +0.5% on the headline.
constexpr uint32_t kQTailShift = 3;
constexpr uint32_t kWgRing = 8;    // LDS ring of published chunk ids
constexpr uint64_t kNoChunk = 0xFFFFFFFFull;

}  // namespace

#endif  // CRC_GPU_SHAPE_H
