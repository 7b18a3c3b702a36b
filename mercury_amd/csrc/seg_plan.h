// seg_plan.h -- the arithmetic of the segment passes (checksum_segments,
// gather_segments, scatter_segments; mchecksum_gpu_ext.hip): how a segment is
// cut into chunks, where each region of the caller's workspace lies, which
// bytes a chunk covers and where it sits in its object -- with every guard
// that keeps a chunk pass inside the caller's memory when the scan's tables
// cannot be trusted -- and a chunk's two addresses in a copying call.  Pure
// arithmetic, like launch_plan.h and copy_plan.h: the kernels include it, and
// the host compiler walks it on the CPU (tests/native/seg_plan.cpp) together
// with the store rule (crc_gpu_pack_store.h).  Plain C++ compiles it.
//
// Object j = segments [first[j], first[j + 1]) in order; P and C are the
// exclusive prefix sums of the segment lengths and chunk counts (the scan's).
// A chunk is bytes [off, off + n) of segment s, off a multiple of the chunk
// size.  It starts at
//   segment side:    addr[s] + off
//   contiguous side: base + starts[j] + (P[s] + off - P[first[j]])
// and the direction says which of the two is loaded and which is stored.
//
// The functions below take values the kernels have already loaded; when and
// where each word is loaded stays the kernels' business (seg_locate).  A scan
// whose look-back gave up leaves the workspace as some earlier call wrote it:
// tables that are valid for ANOTHER list.  A chunk pass that runs on them must
// read and write only inside the caller's segments, so every word taken from
// the workspace is checked here before it becomes an index, a length or a
// shift count, and a chunk that fails a check is skipped.  A trusted scan
// never trips one.
#ifndef MCK_SEG_PLAN_H
#define MCK_SEG_PLAN_H

#include <cstddef>
#include <cstdint>

#include "crc_gpu_shape.h"

namespace mck {

// gather: segments -> contiguous; scatter: contiguous -> segments
enum SegCopyDir : int { kSegGather, kSegScatter };

// The segment passes' chunk size.  CH is a parameter so that a test can make
// chunk edges dense.
constexpr uint64_t kSegChunk = 256u << 10;

template <uint64_t CH = kSegChunk>
MCK_HOST_DEVICE_INLINE uint64_t seg_chunk_count(uint64_t len) {
    return (len + CH - 1) / CH;
}
// bytes of the chunk at offset off (< len) of a segment of len bytes
template <uint64_t CH = kSegChunk>
MCK_HOST_DEVICE_INLINE uint64_t seg_chunk_len(uint64_t len, uint64_t off) {
    return len - off < CH ? len - off : CH;
}

// The scan launch: kScanThreads threads take kScanPer segments each, and every
// scan block keeps kDescWords look-back words in the workspace: flag,
// aggregate (p, c, r), inclusive (p, c, r), pad.
constexpr uint32_t kScanThreads = 256, kScanPer = 4, kScanBlk = kScanThreads * kScanPer;
constexpr uint32_t kDescWords = 8;
// scan blocks of a list (one at least: the scan launch writes the totals)
MCK_HOST_DEVICE_INLINE uint64_t seg_scan_blocks(uint64_t nseg) { return nseg ? (nseg + kScanBlk - 1) / kScanBlk : 1; }

// More segments than this (far beyond device memory) are rejected, so the
// workspace size cannot wrap.
constexpr uint64_t kMaxSegs = 1ull << 40;

// The caller's workspace, as 8-byte word offsets of its regions in order: P
// and C (nseg + 1 words each), the ragged flag, the scan's fault claim, the
// workspace's count of scans (gen), a spare word, the look-back descriptors
// (kDescWords per scan block), each segment's object record {object, first[j],
// first[j + 1], head segment} (4 nseg), then the chunk -> segment map: map_cap
// u32 entries, 4 per segment + 64 Ki, i.e. lists averaging up to ~1 MiB per
// segment, or one huge segment up to 16 GiB; none from 2^32 segments on (an
// entry could not hold the index).  fault_claim and gen live across calls:
// where they sit is part of what one call leaves to the next.
struct SegWorkLayout {
    uint64_t P, C, ragged, fault_claim, gen, spare, desc, obj, map;
    uint64_t map_cap;
    uint64_t bytes;
};
MCK_HOST_DEVICE_INLINE SegWorkLayout seg_work_layout(uint64_t nseg) {
    SegWorkLayout w{};
    w.P = 0;
    w.C = w.P + (nseg + 1);
    w.ragged = w.C + (nseg + 1);
    w.fault_claim = w.ragged + 1;
    w.gen = w.fault_claim + 1;
    w.spare = w.gen + 1;
    w.desc = w.spare + 1;
    w.obj = w.desc + kDescWords * seg_scan_blocks(nseg);
    w.map = w.obj + 4 * nseg;
    w.map_cap = nseg < (1ull << 32) ? 4 * nseg + 65536 : 0;
    w.bytes = 8 * w.map + 4 * w.map_cap;
    return w;
}
// what mchecksum_gpu_segments_work_size returns: SIZE_MAX makes any
// allocation of it fail
MCK_HOST_DEVICE_INLINE size_t seg_work_bytes(uint64_t nseg) {
    return nseg > kMaxSegs ? SIZE_MAX : (size_t)seg_work_layout(nseg).bytes;
}

// verify_segments has no output array, so the chunk pass accumulates in the
// workspace: a word per object that has segments, indexed by the object's
// first segment (distinct among such objects, below nseg; an object without
// segments has no chunk and needs no word).  The words are the tail of the
// map's region -- the call uses a map of 2 nseg + 64 Ki entries instead of 4
// nseg + 64 Ki, and a list with more chunks than that searches C, as any list
// past the map does -- so the workspace keeps its size.  From 2^32 segments on
// there is no map to take them from: such a call is refused.  The chunk pass
// leaves its own fault claim in the spare word, as the scan leaves its in
// fault_claim: the call's key when a wait of that pass gave up.
constexpr uint64_t kMaxVerifySegs = (1ull << 32) - 1;
struct SegVerifyLayout {
    uint64_t acc;      // 8-byte word offset of the nseg accumulator words
    uint64_t map_cap;  // map entries left to the call
    uint64_t chunk_claim;
};
MCK_HOST_DEVICE_INLINE bool seg_verify_layout(uint64_t nseg, SegVerifyLayout *v) {
    const SegWorkLayout w = seg_work_layout(nseg);
    if (nseg > kMaxVerifySegs || w.map_cap < 2 * nseg) return false;
    v->map_cap = w.map_cap - 2 * nseg;
    v->acc = w.map + v->map_cap / 2;  // (map_cap is even: the words stay 8-byte aligned)
    v->chunk_claim = w.spare;
    return true;
}

// The workspace's regions as pointers, shared by the scan (which writes them
// through its own writable view) and the chunk passes (which only read).
template <class U64, class U32>
struct SegWorkT {
    U64 *P, *C;        // byte / chunk exclusive prefix sums, nseg + 1 each
    U64 *ragged;       // non-zero if any chunk needs the ragged loop
    U64 *fault_claim;  // the key of the call whose scan reported a fault
    U64 *gen;          // scans run in this workspace (the key's second half)
    U64 *desc;         // look-back descriptors
    U64 *obj;          // object records, 4 words per segment
    U32 *map;          // the segment of each chunk, while the chunks fit map_cap
    uint64_t map_cap;
};
using SegWork = SegWorkT<const uint64_t, const uint32_t>;
inline SegWork seg_work(const void *base, uint64_t nseg) {
    const SegWorkLayout l = seg_work_layout(nseg);
    const uint64_t *w = static_cast<const uint64_t *>(base);
    return SegWork{w + l.P,   w + l.C,   w + l.ragged, w + l.fault_claim,
                   w + l.gen, w + l.desc, w + l.obj,    reinterpret_cast<const uint32_t *>(w + l.map), l.map_cap};
}

// A segment outside every object, and an object whose head segment the scan
// block could not place (object records, words 0 and 3).
constexpr uint64_t kNoObj = ~0ull;

// A chunk as the chunk passes hold it: what the pass loaded (at, obj_at, end:
// byte offsets in the list's order, from P) and what the rules below make of it.
struct SegChunk {
    uint64_t addr = 0, n = 0;  // its bytes [addr, addr + n) on the segment side
    uint64_t obj = 0;          // its object
    uint64_t at = 0;           // its first byte: P[s] + off
    uint64_t obj_at = 0;       // its object's first byte, P[first[obj]] (where the pass loads it)
    uint64_t end = 0;          // its object's end, P[first[obj + 1]]
    uint64_t after = 0;        // object bytes that follow it: its Z^n shift count (seg_chunk_after)
    uint64_t obj_off = 0;      // its offset in the object (seg_chunk_place)
    bool in = false;           // belongs to an object and passed every check so far: hash it
    bool head = false;         // starts its object
};

// The segment index a pass found for a chunk, and the words of that segment's
// object record: each may index the tables only inside them (P and C have
// nseg + 1 entries, out and starts nobj).
MCK_HOST_DEVICE_INLINE bool seg_segment_ok(uint64_t s, uint64_t nseg) { return s < nseg; }
MCK_HOST_DEVICE_INLINE bool seg_record_ok(uint64_t obj, uint64_t nobj, uint64_t fs, uint64_t ls, uint64_t nseg) {
    return obj < nobj && fs <= nseg && ls <= nseg;  // (kNoObj is no object)
}

// Bytes of chunk c inside its segment: cs = C[s], len = len[s].  false: the
// chunk is not one of that segment's -- skip it.  (A difference that wraps in
// the product still passes only with off < len: the bytes are the segment's.)
template <uint64_t CH = kSegChunk>
MCK_HOST_DEVICE_INLINE bool seg_chunk_bytes(uint64_t c, uint64_t cs, uint64_t len, uint64_t *off, uint64_t *n) {
    *off = (c - cs) * CH;
    if (cs > c || *off >= len) return false;
    *n = seg_chunk_len<CH>(len, *off);
    return true;
}

// The shift packs hold the operators of 12 base-16 digits (CRC_SHIFT_DIGITS):
// a count from 2^48 on would index past them.
constexpr uint64_t kSegShiftEnd = 1ull << 48;

// The chunk's place in its object: the object bytes that follow it ...
MCK_HOST_DEVICE_INLINE bool seg_chunk_after(SegChunk *k) {
    k->after = k->end - k->at - k->n;
    return k->at <= k->end && k->n <= k->end - k->at && k->after < kSegShiftEnd;
}
// ... and its offset in the object (k->obj_at loaded too).  false from either:
// prefixes that put the chunk outside its object -- skip it.
MCK_HOST_DEVICE_INLINE bool seg_chunk_place(SegChunk *k) {
    k->obj_off = k->at - k->obj_at;
    return seg_chunk_after(k) && k->at >= k->obj_at;
}

// Whether a chunk starts its object: it is the first chunk of the object's
// head segment hs (its first non-empty one), or, where the scan block could
// not tell (kNoObj), it lies at the object's first byte.
MCK_HOST_DEVICE_INLINE bool seg_head_known(uint64_t hs) { return hs != kNoObj; }
MCK_HOST_DEVICE_INLINE bool seg_chunk_head(uint64_t hs, uint64_t s, uint64_t off, uint64_t at, uint64_t obj_at) {
    return seg_head_known(hs) ? hs == s && off == 0 : at == obj_at;
}

struct SegCopyAddr {
    uint64_t load, store;
};

// seg_at = addr[s] + off; obj_off: the chunk's offset in its object
// (seg_chunk_place); start = starts[j].
MCK_HOST_DEVICE_INLINE SegCopyAddr seg_copy_addr(int dir, uint64_t seg_at, uint64_t base, uint64_t start,
                                                 uint64_t obj_off) {
    const uint64_t flat = base + start + obj_off;
    return dir == kSegGather ? SegCopyAddr{seg_at, flat} : SegCopyAddr{flat, seg_at};
}

// verify_segments fails closed.  Its compare runs after the chunk pass and
// first reads the call's fault state from the workspace: the scan's claim
// and the chunk pass's, each equal to the call's key when that stage gave up.
MCK_HOST_DEVICE_INLINE bool seg_call_faulted(uint64_t scan_claim, uint64_t chunk_claim, uint64_t key) {
    return scan_claim == key || chunk_claim == key;
}
// What the compare writes for object j: after a faulted call status 1 whatever
// the value holds (it may be half accumulated), otherwise whether the value
// differs from the expected one.  Returns what j adds to the mismatch counter
// (the caller sums it and adds the sum where there is a counter), so a faulted
// call adds nobj between its objects.  status may be NULL.  state_verify
// decides with the same function: it has no fault state to read (faulted =
// false).
MCK_HOST_DEVICE_INLINE uint32_t seg_verify_decide(bool faulted, uint64_t value, uint64_t expected, uint8_t *status,
                                                  uint64_t j) {
    const uint32_t bad = faulted || value != expected ? 1u : 0u;
    if (status) status[j] = (uint8_t)bad;
    return bad;
}

// The message calls (pack_segment_messages, unpack_segment_messages): object
// j's segments are the fields of message j = buf[offsets[j], offsets[j + 1]),
// whose payload starts payload_offset bytes in.  The calls take more objects
// than the workspace of a plain segment call has room for, so theirs is that
// workspace (seg_work_layout, unchanged: the scan writes it as ever) with two
// per-object regions behind it: the accumulator words (u32, CRC-32C only) the
// chunk pass XORs into, indexed by the object, and the fit gates (a byte
// each, non-zero: the message does not fit, its chunks are skipped).
constexpr uint64_t kMaxMsgObjs = 1ull << 31;
struct SegMsgLayout {
    uint64_t acc;   // 8-byte word offset of the nobj u32 accumulator words
    uint64_t gate;  // 8-byte word offset of the nobj gate bytes
    uint64_t bytes;
};
MCK_HOST_DEVICE_INLINE bool seg_msg_layout(uint64_t nseg, uint64_t nobj, SegMsgLayout *m) {
    if (nseg > kMaxVerifySegs || nobj > kMaxMsgObjs) return false;
    m->acc = (seg_work_layout(nseg).bytes + 7) / 8;
    m->gate = m->acc + (nobj + 1) / 2;
    m->bytes = 8 * (m->gate + (nobj + 7) / 8);
    return true;
}
// what mchecksum_gpu_segment_messages_work_size returns
MCK_HOST_DEVICE_INLINE size_t seg_msg_work_bytes(uint64_t nseg, uint64_t nobj) {
    SegMsgLayout m{};
    return seg_msg_layout(nseg, nobj, &m) ? (size_t)m.bytes : SIZE_MAX;
}

// The fit rule: message [m0, m1) holds payload_offset header bytes and then
// exactly the object's n bytes.  A table that runs backwards, or a message
// shorter than its headers, never fits.
MCK_HOST_DEVICE_INLINE bool seg_msg_fits(uint64_t m0, uint64_t m1, uint64_t payload_offset, uint64_t n) {
    return m1 >= m0 && m1 - m0 >= payload_offset && m1 - m0 - payload_offset == n;
}
// The gate of object j, from the words the launch ahead of the chunk pass
// loaded: f0 = first[j], f1 = first[j + 1] (a range outside the segment table
// has no prefix to read: gated; p0 = P[f0], p1 = P[f1] are read only inside
// it, by the caller).
MCK_HOST_DEVICE_INLINE bool seg_msg_range_ok(uint64_t f0, uint64_t f1, uint64_t nseg) {
    return f0 <= f1 && f1 <= nseg;
}
MCK_HOST_DEVICE_INLINE uint8_t seg_msg_gate(bool range_ok, uint64_t p0, uint64_t p1, uint64_t m0, uint64_t m1,
                                            uint64_t payload_offset) {
    return range_ok && p1 >= p0 && seg_msg_fits(m0, m1, payload_offset, p1 - p0) ? 0 : 1;
}

// After the chunk pass, per message.  Pack: whether the value is sealed into
// the header -- never after a faulted call (the value may be half
// accumulated), never for a gated message (nothing of it was written) --;
// status = 1 where it is not.  Returns the seal decision.
MCK_HOST_DEVICE_INLINE bool seg_msg_seal_decide(bool faulted, uint8_t gate, uint8_t *status, uint64_t j) {
    const bool seal = !faulted && gate == 0;
    if (status) status[j] = seal ? 0 : 1;
    return seal;
}
// Unpack: whether the header word may be read and compared at all (a gated
// message may be shorter than its headers), and the verdict -- verify_segments'
// rule, a gated message counting as a faulted one: status 1, one mismatch.
MCK_HOST_DEVICE_INLINE bool seg_msg_compares(bool faulted, uint8_t gate) { return !faulted && gate == 0; }
MCK_HOST_DEVICE_INLINE uint32_t seg_msg_open_decide(bool faulted, uint8_t gate, uint64_t value, uint64_t header,
                                                    uint8_t *status, uint64_t j) {
    return seg_verify_decide(!seg_msg_compares(faulted, gate), value, header, status, j);
}

}  // namespace mck

#endif  // MCK_SEG_PLAN_H
