/*
 * mchecksum_gpu.h -- MI355X batch entry points of libmchecksum.
 *
 * These are ADDITIONAL extern "C" entry points next to the unchanged
 * mchecksum streaming API (<mchecksum.h>).  Where Mercury streams the bytes
 * of one serialized proc buffer through mchecksum_update/get
 * (src/mercury_proc.c:387-406, 358-384), a batch entry point computes the
 * same value for many independent, device-resident payloads at once:
 *
 *   value[i] == mchecksum_get() after mchecksum_update(payload_i, len_i)
 *
 * bit for bit, for every method the GPU supports (every 32/64-bit catalogue
 * method: crc32c, crc32, crc64 and its variants, MSB-first ECMA-182 included).  The
 * whole-buffer form is exact because, in Mercury's default non-XDR build, the
 * proc checksum is the CRC of the contiguous serialized bytes
 * buf[0 : hg_proc_get_size_used) (src/mercury_proc.h:124-143,162-181;
 * SURVEY.md 0.4).  It is NOT exact for a Mercury built with XDR encoding:
 * hash such buffers with mchecksum_gpu_checksum_xdr() below.
 *
 * Memory: dev_base, dev_offsets and dev_out are device pointers (hipMalloc or
 * any device-accessible allocation).  Payload bytes are read in aligned
 * 16-byte granules, so the allocation must be readable up to the next 16-byte
 * boundary after the last payload byte (hipMalloc allocations always are).
 * dev_out receives `count` host-order integers of the method's size
 * (uint32_t for crc32c, uint64_t for crc64).
 *
 * Streams: `stream` is a hipStream_t (NULL = the default stream).  Calls are
 * asynchronous and capture-safe once mchecksum_gpu_prepare() has run for the
 * method on the current device (it uploads the lookup tables).  Large batches
 * balance their payloads through a device-side work-queue slot: each launch
 * takes an idle one of the device's 2048 slots and holds it until it
 * completes (a HIP event recorded by the launch's completion, queried without
 * blocking), so no slot ever serves two launches at once -- whatever the
 * streams, host threads, stream handle reuse or hipStreamDestroy timing.
 * Calls captured into a hipGraph, and calls that find the oldest in-flight
 * slots all still busy with no idle one left, take a plain static split of
 * the batch instead: a graph replays its captured arguments, possibly on two
 * execs at once, so no slot could be exclusive to it.  Destroying a stream
 * with calls in flight follows the HIP rules for the memory those calls use;
 * the library itself keeps no per-stream state.
 *
 * Fail closed: every wait on the device is bounded, and so is every call.  A
 * wait gives up after 1 s of real time (time the wave spends switched out of
 * the GPU does not count); once one wait of a call has given up, every other
 * wait of that call gives up at once (the launch's abort flag; a segments
 * call whose scan gave up hashes nothing more), so a call that meets any
 * number of stalls still returns within about one deadline.  A call in which
 * a wait gave up (a protocol fault; 0 in every test run) adds 1 -- once per
 * call -- to the error word set with mchecksum_gpu_set_error_word(), adds
 * `count` to the mismatch counter of a verify call and marks every payload it
 * cannot vouch for with status 1, so unhashed bytes never read as verified.
 *
 * Sender side: mchecksum_gpu_pack_messages copies device-resident payloads
 * behind their message headers, hashes them in the same pass and stores each
 * value network-order in the message's HG header slot (what HG_PROC_TYPE's
 * memcpy + mchecksum_update and hg_set_struct do per field and per handle,
 * src/mercury_proc.h:124-143,162-181, src/mercury.c:699-707);
 * mchecksum_gpu_seal_messages hashes payloads already in place, and
 * mchecksum_gpu_seal_core_headers stores the CRC-16 of the core headers.  They
 * write only the bytes named at their declarations, fail closed as the verify
 * calls do (status 1 on every message the launch cannot vouch for; the hash
 * slots of such messages are unspecified) and are capture-safe after
 * mchecksum_gpu_prepare(): a replay packs or seals the current contents again.
 * For a Mercury built with XDR encoding, mchecksum_gpu_pack_xdr_messages is
 * the same one pass with an encoder in it: it reads each message's host-order
 * field values, writes their XDR wire bytes behind the headers, hashes the
 * values and seals (what hg_proc_<type> does per field on HG_ENCODE under
 * HG_HAS_XDR: xdr_<type> into the buffer, mchecksum_update over the host
 * variable, src/mercury_proc.h:110-122,147-160);
 * mchecksum_gpu_seal_xdr_messages hashes messages already encoded, and
 * mchecksum_gpu_xdr_encoded_sizes gives the message table's lengths.
 * An overflow RPC -- serialized arguments that do not fit the eager buffer --
 * keeps its payload in the proc's extra buffer, sent by bulk, while the hash
 * of that buffer still goes into the HG header of the short eager message
 * (hg_set_struct, src/mercury.c:699-707 ahead of :715-776):
 * mchecksum_gpu_seal_detached_messages hashes such payloads where they lie and
 * stores each value in its message's slot in another buffer, and
 * mchecksum_gpu_state_seal_messages stores the values of streamed states
 * (state_init, update_* stages) there.
 *
 * Receiver side: mchecksum_gpu_verify_messages checks received messages in
 * place; mchecksum_gpu_unpack_messages also copies each payload out of the
 * receive buffer to where it is consumed, in the same pass over its bytes
 * (HG_PROC_TYPE on HG_DECODE copies each field out and feeds the same bytes to
 * mchecksum_update, src/mercury_proc.h:124-143,162-181; hg_get_struct then
 * compares, src/mercury.c:565-573).  For an overflow RPC (HG_CORE_MORE_DATA
 * set in the core header) the receiver pulls the extra buffer by bulk
 * (hg_get_extra_payload, src/mercury.c:866-958), decodes from it (:544-546)
 * and compares its checksum with the eager message's header hash; the bytes
 * behind the eager message's headers are a bulk descriptor, which that hash
 * does not cover.  mchecksum_gpu_verify_detached_messages checks a batch of
 * such RPCs in one call -- the pulled payloads by one table, the hashes read
 * from the eager messages by another --, and
 * mchecksum_gpu_state_verify_messages ends a pull that was hashed in stages.
 *
 * Settings: the MCHECKSUM_* environment variables (variants, log level, the
 * MCHECKSUM_GPU_* launch-policy overrides of the A/B tools) are read once,
 * at the library's first use, never on the call path.
 *
 * There is NO host fallback: without a usable HIP device every call returns
 * MCHECKSUM_GPU_ENODEV.
 */
#ifndef MCHECKSUM_GPU_H
#define MCHECKSUM_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "mchecksum.h"

#define MCHECKSUM_GPU_OK        0
#define MCHECKSUM_GPU_EINVAL    (-1) /* bad argument */
#define MCHECKSUM_GPU_ENODEV    (-2) /* no usable HIP device */
#define MCHECKSUM_GPU_EMETHOD   (-3) /* method not supported on GPU (16-bit methods on the
                                         payload paths; MSB-first ones on XDR) */
#define MCHECKSUM_GPU_EHIP      (-4) /* HIP runtime error (see error string) */

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if a HIP device is usable by this process, else 0. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_available(void);

/* Build and upload the lookup tables for hash_method on the current device:
 * the payload kernels' packs and the Z^n shift pack (32/64-bit models), or
 * the core-header byte table (16-bit models).  Optional (done lazily on first
 * use); call it before hipGraph capture -- a first use inside a capture
 * would upload tables there and invalidate the capture. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_prepare(const char *hash_method);

/* Fixed-size batch: payload i = dev_base[i*stride, i*stride + len), i < count.
 * (Every batch entry point takes at most 2^31 payloads per call.) */
MCHECKSUM_PUBLIC int
mchecksum_gpu_checksum_fixed(const char *hash_method, const void *dev_base,
    size_t stride, size_t len, size_t count, void *dev_out, void *stream);

/* Variable-size batch: payload i = dev_base[dev_offsets[i], dev_offsets[i+1]),
 * i < count; dev_offsets holds count + 1 non-decreasing byte offsets
 * (the C4 "offsets table" layout; payloads may start at any byte). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_checksum_offsets(const char *hash_method, const void *dev_base,
    const uint64_t *dev_offsets, size_t count, void *dev_out, void *stream);

/* Streaming batch checksums: init / update / get over many device-resident
 * streams at once, for objects that arrive in chunks (a pipelined bulk
 * transfer, an object larger than its staging buffer) and are never resident
 * in one piece.
 *
 *   state_init, then ANY sequence of update_offsets calls, then state_get
 *     == mchecksum_get() after mchecksum_update() over the same bytes in the
 *        same order, bit for bit, per stream i;
 *   state_init followed directly by state_get yields the CRC of the empty
 *   message.
 *
 * dev_state holds `count` elements of the method's size (uint32_t /
 * uint64_t): the running registers in the kernels' internal form -- opaque;
 * only these calls interpret them.  Every 32/64-bit catalogue method,
 * MSB-first ones included; 16-bit methods return MCHECKSUM_GPU_EMETHOD.
 * Error codes, the stream convention, the 2^31-payload cap, the empty-batch
 * rules (count 0 needs no buffers) and MCHECKSUM_GPU_ENODEV are those of
 * mchecksum_gpu_checksum_offsets; update_offsets launches the seeded twin of
 * the kernel checksum_offsets picks for the same count, with the same
 * work-queue rules.
 *
 * All four calls are asynchronous and stream-ordered: an update sees the
 * state its predecessors on the stream left.  They are capture-safe after
 * mchecksum_gpu_prepare() (which uploads the Z^n shift pack they use: nothing
 * is uploaded inside a capture); a replayed update_offsets advances the state
 * again on every replay.  One stream of states must not be updated by two
 * calls running at once.
 *
 * Fail closed as the checksum calls: an update_offsets call in which a device
 * wait gave up adds 1 to the error word (mchecksum_gpu_set_error_word) and to
 * mchecksum_gpu_queue_faults(); after such a call the states it touched are
 * unspecified (some advanced, some not) and must be initialised again. */

/* dev_state[i] = the method's initial register, i < count. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_state_init(const char *hash_method, void *dev_state,
    size_t count, void *stream);

/* dev_state[i] <- dev_state[i] advanced over dev_base[dev_offsets[i],
 * dev_offsets[i+1]) (the checksum_offsets layout and memory rules).  A
 * zero-length chunk leaves dev_state[i] unchanged: that is how a stream with
 * nothing new this round is expressed. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_update_offsets(const char *hash_method, const void *dev_base,
    const uint64_t *dev_offsets, size_t count, void *dev_state, void *stream);

/* dev_out[i] = what mchecksum_get() returns after all updates so far (host
 * order, method size).  Does not modify the state: more updates may follow.
 * dev_out may alias dev_state (the states then hold values, not registers). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_state_get(const char *hash_method, const void *dev_state,
    size_t count, void *dev_out, void *stream);

/* state_get and the compare in one launch: dev_status[i] = 1 where the value
 * state_get would return for dev_state[i] differs from dev_expected[i] (count
 * host-order values of the method's size), else 0; *dev_mismatches (a device
 * uint32_t the caller zeroes) is increased by the number of mismatches.
 * Either of the two may be NULL.  The states are not modified.  No
 * device-side wait, no work-queue slot and no workspace, like combine_runs,
 * so nothing to fail closed on -- and no way to know whether an earlier
 * update failed: check the error word first, as after update_offsets.
 * Arguments as mchecksum_gpu_state_get (dev_expected required when
 * count > 0).  Capture-safe. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_state_verify(const char *hash_method, const void *dev_state,
    size_t count, const void *dev_expected, uint8_t *dev_status,
    uint32_t *dev_mismatches, void *stream);

/* dev_out[i] = CRC(A_i || B_i) from dev_crc_a[i] = CRC(A_i), dev_crc_b[i] =
 * CRC(B_i) -- finalized values as the checksum_* calls and state_get return
 * them -- and dev_len_b[i] = the bytes of B_i (< 2^48).  For chunks that
 * complete out of order: hash each on its own, join afterwards, left to
 * right (all of an object's chunks in one launch:
 * mchecksum_gpu_combine_runs).  dev_out may alias dev_crc_a or dev_crc_b. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_combine(const char *hash_method, const void *dev_crc_a,
    const void *dev_crc_b, const uint64_t *dev_len_b, size_t count,
    void *dev_out, void *stream);

/* The last step of a pipelined transfer, in one call: the CRCs of each
 * object's chunks, which completed in any order, joined into the object's CRC.
 * Also the per-object CRC from per-block CRCs (checksum_fixed over the blocks)
 * without reading the data again.
 *
 * Chunk k has the finalized CRC dev_crc[k] (host order, method size: what the
 * checksum_* / copy_offsets calls and state_get return) and dev_len[k] bytes.
 * dev_run_first holds nruns + 1 non-decreasing indices <= nchunks (the shape
 * of checksum_segments' dev_obj_first); run j is chunks [dev_run_first[j],
 * dev_run_first[j+1]), in that order.
 *
 *   - dev_out[j] = what mchecksum_get() returns after hashing the run's chunks
 *     concatenated in order (nruns host-order values of the method's size).
 *   - dev_out_len[j] (optional: may be NULL) = the run's byte total.  With it a
 *     call's outputs are valid chunk inputs of a further call: join a very
 *     long run in two levels (runs of about a thousand chunks, then one run
 *     over the results), or join partial joins as more chunks arrive.
 *   - An empty run gets the CRC of the empty message and length 0.  A chunk
 *     with dev_len[k] == 0 contributes nothing, whatever dev_crc[k] holds.
 *     Chunks outside [first[0], first[nruns]) are not read.
 *   - Every 32/64-bit catalogue method, MSB-first ones included; values go in
 *     and come out in the checksum calls' form (no swap launch follows).
 *     16-bit methods return MCHECKSUM_GPU_EMETHOD.
 *   - A run's byte total must be < 2^48, the shift pack's range, as in
 *     mchecksum_gpu_combine (beyond it the value is unspecified; nothing is
 *     read out of range).  nchunks and nruns are at most 2^31 each.
 *   - Arguments are checked in combine's order: NULL pointers and the caps
 *     (MCHECKSUM_GPU_EINVAL), then the device, then the method.  dev_run_first
 *     and dev_out are required when nruns > 0, dev_crc and dev_len when
 *     nchunks > 0.  nruns == 0 passes those checks and returns
 *     MCHECKSUM_GPU_OK without a launch; nchunks == 0 with nruns > 0 is legal
 *     (every run is empty).
 *   - dev_out and dev_out_len must not overlap dev_crc, dev_len or
 *     dev_run_first: runs are joined in parallel, and one run's output would
 *     land in a table another is still reading.
 *   - Asynchronous and stream-ordered; capture-safe after
 *     mchecksum_gpu_prepare().  A replay reads all three tables again, so
 *     CRCs, lengths and run boundaries may change between replays.
 *   - The kernel has no device-side wait, takes no work-queue slot and needs
 *     no workspace: there is nothing to fail closed on, and the call adds
 *     nothing to the error word or to mchecksum_gpu_queue_faults().
 *   - One launch whatever the run sizes: a wave per run, the whole workgroup
 *     for a run of more than 4096 chunks.  One very long run is one
 *     workgroup's work -- correct, but slow (2^20 chunks: 7 ms crc32c, 29 ms
 *     crc64); join it in two levels through dev_out_len (runs of 1024, then
 *     one run of 1024: 0.09 and 0.14 ms).  DESIGN.md 4.15 has the numbers. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_combine_runs(const char *hash_method,
    const void *dev_crc, const uint64_t *dev_len, size_t nchunks,
    const uint64_t *dev_run_first, size_t nruns,
    void *dev_out, uint64_t *dev_out_len, void *stream);

/* Copy and checksum in one pass: many device-resident chunks are copied to
 * independent destinations and hashed in the same read -- a chunk of a bulk
 * transfer hashed in its staging buffer and moved to its place in the object,
 * without a second pass over its bytes.  A one-shot form and a streaming form.
 *
 * Chunk i = dev_src[dev_src_offsets[i], dev_src_offsets[i+1]) (the
 * checksum_offsets layout and memory rules: count + 1 non-decreasing byte
 * offsets, any start byte, readable to the next 16-byte boundary), n_i bytes.
 * It is copied to dev_dst[dev_dst_starts[i], dev_dst_starts[i] + n_i).
 * dev_dst_starts holds `count` byte offsets into dev_dst, in any order:
 * destinations need not be adjacent or monotonic, so there is no fit rule and
 * no status array; the length of each copy comes from the source table.
 *
 *   - The values are those of mchecksum_gpu_checksum_offsets, and the state
 *     rules those of mchecksum_gpu_update_offsets, bit for bit; every 32/64-bit
 *     catalogue method.
 *   - A zero-length chunk writes nothing and leaves its state unchanged.
 *   - Exactly the n_i destination bytes of each chunk are written: no byte
 *     before them, after them or between them, so dev_dst needs no padding.
 *   - dev_src is never written.
 *   - Destination ranges must not overlap one another or the source range.  The
 *     library cannot check this (the tables are on the device): an overlapping
 *     call copies and hashes unspecified bytes.
 *   - Chunks of any size, 2 GiB and more included.
 *   - Asynchronous and stream-ordered; capture-safe after
 *     mchecksum_gpu_prepare().  A replay copies and hashes the current contents
 *     again, and a replayed update advances the state again.
 *   - Launch plan, work-queue slot and static-split rules are those of
 *     checksum_offsets / update_offsets for the same count.
 *   - MSB-first methods: copy_offsets swaps its outputs after the launch, as
 *     checksum_offsets does; states stay in the kernels' form.
 *   - Fail closed as update_offsets: a call in which a device wait gave up adds
 *     1 -- once per call -- to the error word and to
 *     mchecksum_gpu_queue_faults(); after such a call the outputs, the states
 *     and the destination bytes it touched are unspecified.
 *   - Arguments are checked in checksum_offsets' order: NULL pointers and
 *     count > 2^31 (MCHECKSUM_GPU_EINVAL), then the device (_ENODEV), then the
 *     method (_EMETHOD: unknown, or 16-bit).  count == 0 needs no buffers, but
 *     passes those checks first.
 *   - CRC-32C: the fused call took 19-38% less time than update_offsets plus
 *     a separate contiguous copy.  CRC-64: the copy twins carry more scratch
 *     per lane than the plain kernels; fusing saved 21% on a large batch (8192
 *     chunks, 269 MB) but on 1024 x 64 KiB it saves the second launch, not
 *     time (52% slower than the two passes).  DESIGN.md 4.13 has the numbers. */

/* dev_out[i] = CRC(chunk i), host order, method size. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_copy_offsets(const char *hash_method, const void *dev_src,
    const uint64_t *dev_src_offsets, void *dev_dst,
    const uint64_t *dev_dst_starts, size_t count, void *dev_out, void *stream);

/* dev_state[i] advanced over chunk i (mchecksum_gpu_state_init before,
 * mchecksum_gpu_state_get after). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_update_copy_offsets(const char *hash_method, const void *dev_src,
    const uint64_t *dev_src_offsets, void *dev_dst,
    const uint64_t *dev_dst_starts, size_t count, void *dev_state,
    void *stream);

/* Batched verify of received payloads against expected values (e.g. the
 * payload hash carried in the 4-byte HG header, src/mercury_header.c:111-112,
 * after ntohl): dev_status[i] = 1 if CRC(payload i) != dev_expected[i] else 0,
 * and *dev_mismatches (device uint32) is incremented by the number of
 * mismatches (caller zeroes it).  dev_expected holds host-order values of the
 * method's size.  Either status pointer may be NULL. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_offsets(const char *hash_method, const void *dev_base,
    const uint64_t *dev_offsets, size_t count, const void *dev_expected,
    uint8_t *dev_status, uint32_t *dev_mismatches, void *stream);

/* Batched verify of received RPC messages in place.
 * Message i = dev_buf[dev_msg_offsets[i], dev_msg_offsets[i+1]) as it sits in
 * an NA multi-recv buffer (src/mercury_core.c:2092-2132, 4667-4714): headers,
 * then the serialized payload from payload_offset on.  The expected CRC is
 * the network-order u32 at hash_offset -- in Mercury the HG header's payload
 * hash (src/mercury_header.c:111-112) right after the 16-byte core header, so
 * hash_offset = 16 and payload_offset = 20 for HG_INPUT without user offset.
 * dev_status[i] = 1 when the payload CRC differs (what hg_get_struct reports
 * as HG_CHECKSUM_ERROR, src/mercury.c:565-573) or the message is shorter than
 * payload_offset; *dev_mismatches is incremented per failure.  crc32c only
 * (the header slot is 32 bits). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_messages(const char *hash_method, const void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, uint32_t *dev_mismatches,
    void *stream);

/* Verify and copy out in one pass over the payload bytes: pack_messages'
 * mirror on the receiver.  Message i = dev_buf[dev_msg_offsets[i],
 * dev_msg_offsets[i+1]) with the table and memory rules of
 * mchecksum_gpu_verify_messages (dev_buf readable to the next 16-byte
 * boundary).  Its payload dev_buf[dev_msg_offsets[i] + payload_offset,
 * dev_msg_offsets[i+1]) is copied to dev_dst[dev_dst_offsets[i],
 * dev_dst_offsets[i+1]), its CRC-32C is computed in the same read and compared
 * with the network-order u32 at dev_msg_offsets[i] + hash_offset; both tables
 * hold count + 1 entries.  Message i fits iff
 *   dev_msg_offsets[i+1] - dev_msg_offsets[i]
 *       == payload_offset + (dev_dst_offsets[i+1] - dev_dst_offsets[i])
 * (a message shorter than payload_offset never fits); one that does not gets
 * dev_status[i] = 1, counts as one mismatch, and no destination byte of it is
 * written.  A fitting message gets status 0 when its CRC matches, and status 1
 * and one mismatch when it differs -- its destination then holds the payload
 * bytes AS RECEIVED: the copy happens before the value is known, as Mercury
 * has decoded by the time hg_get_struct compares.  Look at the status before
 * the bytes.  The call writes exactly the destination bytes of fitting
 * messages -- nothing before dev_dst_offsets[0], no gap between payloads,
 * nothing past dev_dst_offsets[count] -- so dev_dst needs no padding; dev_buf
 * is never written.  Payloads of any size (2 GiB and more included).  The
 * destination range and dev_buf's range must not overlap: the library cannot
 * check that (the tables are on the device), and an overlapping call copies
 * and hashes unspecified bytes.  Either of dev_status and dev_mismatches may
 * be NULL; *dev_mismatches is added to (the caller zeroes it).  Argument
 * rules and their order are mchecksum_gpu_seal_messages' (layout, then the
 * method -- crc32c only --, then the device); count == 0 needs no buffers.
 * Plan, work-queue slot and capture rules of verify_messages: a replay
 * unpacks the buffer's current contents.  Fails closed as the verify calls do
 * (error word + 1, count added to *dev_mismatches, status 1 on every message
 * the launch cannot vouch for, whose destination bytes are unspecified). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_unpack_messages(const char *hash_method, const void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, void *dev_dst, const uint64_t *dev_dst_offsets,
    uint8_t *dev_status, uint32_t *dev_mismatches, void *stream);

/* Sender side of mchecksum_gpu_verify_messages, in place: the same message
 * table and argument rules (hash_offset + 4 <= payload_offset; crc32c only,
 * and the method is checked before the device).  For message i the CRC of
 * dev_buf[dev_msg_offsets[i] + payload_offset, dev_msg_offsets[i+1]) is stored
 * big-endian in the 4 bytes at dev_msg_offsets[i] + hash_offset, as
 * hg_set_struct stores it (src/mercury.c:699-707), and dev_status[i]
 * (optional) = 0.  A message shorter than payload_offset gets status 1 and is
 * not written.  No byte other than the 4 hash bytes of a sealed message is
 * written.  The payloads are read as in verify_messages (readable to the next
 * 16-byte boundary). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_messages(const char *hash_method, void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

/* Overflow RPCs: payloads held outside their messages.  "Detached" means that
 * one table addresses the eager messages -- message i =
 * dev_msgs[dev_msg_offsets[i], dev_msg_offsets[i+1]): the headers, then
 * whatever follows them (for Mercury a bulk descriptor, which no hash covers)
 * -- and a second buffer and table address the payloads: payload i =
 * dev_payloads[dev_payload_offsets[i], dev_payload_offsets[i+1]), the whole
 * range (the extra buffer hg_get_extra_payload pulled, or the one
 * hg_set_struct is about to register).  Both tables hold count + 1
 * non-decreasing byte offsets.  The hash slot of message i is the 4 bytes at
 * dev_msg_offsets[i] + hash_offset, network order, at any alignment
 * (hash_offset = 16 for HG_INPUT without user offset; at most 2^30).  A
 * message shorter than hash_offset + 4 has no slot: no byte of it is read or
 * written past its end, and it fails.
 *
 *   - Method: a 32-bit model (the slot is 32 bits; crc32c for Mercury).  Every
 *     other method and every unknown name returns MCHECKSUM_GPU_EMETHOD (so
 *     would an MSB-first 32-bit model; the catalogue has none).
 *   - Arguments are checked first (MCHECKSUM_GPU_EINVAL: a NULL required
 *     pointer with count > 0, count > 2^31, hash_offset > 2^30), then the
 *     method (_EMETHOD, ahead of the device as in mchecksum_gpu_seal_messages),
 *     then the device (_ENODEV).  count == 0 needs no buffers, but passes those
 *     checks first.
 *   - The payloads are read as in mchecksum_gpu_checksum_offsets (any start
 *     byte, any size, dev_payloads readable to the next 16-byte boundary); the
 *     messages are touched only at their slots, byte by byte, so dev_msgs needs
 *     no padding.
 *   - Asynchronous and stream-ordered; capture-safe after
 *     mchecksum_gpu_prepare(); no workspace, nothing allocated on the call path.
 *   - The two calls over payloads launch twins of the kernels checksum_offsets
 *     picks for the same count, with its work-queue and static-split rules, and
 *     fail closed as verify_messages and seal_messages do: a call in which a
 *     device wait gave up adds 1 -- once -- to the error word, a verify adds
 *     `count` to *dev_mismatches, and every status the launch cannot vouch for
 *     is 1 (the slots of such messages are unspecified after a seal).
 *   - The two state calls end a transfer that was hashed in stages:
 *     mchecksum_gpu_state_init, then any number of update_offsets,
 *     update_copy_offsets or update_segments calls, then one of them.  They are
 *     element kernels like mchecksum_gpu_state_verify: no work-queue slot and no
 *     device-side wait, so nothing to fail closed on -- and no way to know
 *     whether an earlier update failed: check the error word first.  The states
 *     are not modified.
 *   - DESIGN.md 4.21 has the measurements against the routes through
 *     verify_offsets, checksum_offsets and state_get. */

/* Receiver: dev_status[i] = 1 and one mismatch added to *dev_mismatches (a
 * device uint32_t the caller zeroes) when the CRC of payload i differs from
 * the value in message i's slot, or message i has no slot; else status 0.
 * Either of the two may be NULL.  Neither buffer is written. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_detached_messages(const char *hash_method,
    const void *dev_msgs, const uint64_t *dev_msg_offsets, size_t hash_offset,
    const void *dev_payloads, const uint64_t *dev_payload_offsets,
    size_t count, uint8_t *dev_status, uint32_t *dev_mismatches, void *stream);

/* Sender: the CRC of payload i is stored big-endian in the 4 slot bytes of
 * message i and dev_status[i] (optional) = 0; a message without a slot gets
 * status 1 and no store.  No other byte is written: the bytes behind the
 * headers keep their values, and dev_payloads is only read. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_detached_messages(const char *hash_method,
    void *dev_msgs, const uint64_t *dev_msg_offsets, size_t hash_offset,
    const void *dev_payloads, const uint64_t *dev_payload_offsets,
    size_t count, uint8_t *dev_status, void *stream);

/* mchecksum_gpu_state_verify with the expected values read from the messages'
 * slots: the value state_get would return for dev_state[i] (count uint32_t
 * registers) against message i's slot; verdicts as
 * mchecksum_gpu_verify_detached_messages. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_state_verify_messages(const char *hash_method,
    const void *dev_state, size_t count, const void *dev_msgs,
    const uint64_t *dev_msg_offsets, size_t hash_offset, uint8_t *dev_status,
    uint32_t *dev_mismatches, void *stream);

/* Its mirror on the sender: the value state_get would return for dev_state[i]
 * stored big-endian in message i's slot; statuses and the bytes written as
 * mchecksum_gpu_seal_detached_messages. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_state_seal_messages(const char *hash_method,
    const void *dev_state, size_t count, void *dev_msgs,
    const uint64_t *dev_msg_offsets, size_t hash_offset, uint8_t *dev_status,
    void *stream);

/* The four calls above with BOTH sides addressed by lists: what Mercury holds
 * of overflow RPCs.  The eager messages are those of a drain (one address and
 * one length per completion, as mchecksum_gpu_verify_rpc_message_list takes
 * them), and every payload is an allocation of its own: hg_get_extra_payload
 * allocates one page-aligned extra buffer per handle (src/mercury.c:933-934),
 * and so does the sender's out_extra_buf.  A base pointer and a table of
 * non-decreasing offsets cannot name either.
 *
 * All four arrays are device-resident and hold `count` entries each (not
 * count + 1).  Everything not said here is the table call's of the same name,
 * by reference: statuses 0 / 1, the mismatch counter, the methods, the
 * argument bounds and their order (EINVAL -- each array is a required pointer
 * with count > 0 --, then the method's EMETHOD ahead of the device, then
 * ENODEV; count == 0 needs no buffers but passes the checks first), and the
 * launch, capture and fail-closed rules (a replay reads the current contents
 * of all four arrays).  What follows from entries that lie anywhere:
 *
 * Message side.  Message i is the L = dev_msg_len[i] bytes at the device
 * address dev_msg_addr[i]; an end that wraps the address space gives L = 0.
 * Its slot exists iff L >= hash_offset + 4, and is the 4 bytes at
 * dev_msg_addr[i] + hash_offset, read or written byte by byte at any
 * alignment.  A message without a slot is never dereferenced and its address
 * may be NULL: a verify counts it as a mismatch with status 1, a seal gives
 * status 1 and makes no store.  A seal writes exactly those 4 bytes per entry
 * and nothing else; slots that are written must not overlap one another.
 *
 * Payload side.  Payload i is the N = dev_payload_len[i] bytes at the device
 * address dev_payload_addr[i].  A payload whose end wraps the address space
 * fails its entry -- status 1, a mismatch on verify, no store on seal -- and
 * nothing of it is read.  N = 0 is a legitimate payload: its CRC is the
 * model's value of the empty message, compared or stored as any other, and
 * its address is never dereferenced and may be NULL.  Reads: per payload, in
 * aligned 16-byte pieces that stay inside the aligned 128-byte lines holding
 * its first and its last byte -- a payload inside any device allocation
 * satisfies this, a page-aligned extra buffer certainly --, and nothing
 * between, before or behind payloads enters a value.
 *
 * The two state calls end a streamed transfer whose update_segments calls took
 * the payloads by address already (dev_seg_addr / dev_seg_len).  DESIGN.md
 * 4.26 has the design and the measurements against the table calls. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_detached_message_list(const char *hash_method,
    const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len,
    size_t hash_offset, const uint64_t *dev_payload_addr,
    const uint64_t *dev_payload_len, size_t count, uint8_t *dev_status,
    uint32_t *dev_mismatches, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_detached_message_list(const char *hash_method,
    const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len,
    size_t hash_offset, const uint64_t *dev_payload_addr,
    const uint64_t *dev_payload_len, size_t count, uint8_t *dev_status,
    void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_state_verify_message_list(const char *hash_method,
    const void *dev_state, size_t count, const uint64_t *dev_msg_addr,
    const uint64_t *dev_msg_len, size_t hash_offset, uint8_t *dev_status,
    uint32_t *dev_mismatches, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_state_seal_message_list(const char *hash_method,
    const void *dev_state, size_t count, const uint64_t *dev_msg_addr,
    const uint64_t *dev_msg_len, size_t hash_offset, uint8_t *dev_status,
    void *stream);

/* Pack, hash and seal in one pass over the payload bytes.  Payload i =
 * dev_src[dev_src_offsets[i], dev_src_offsets[i+1]) (the checksum_offsets
 * layout: any start byte, readable to the next 16-byte boundary) is copied to
 * dev_buf[dev_msg_offsets[i] + payload_offset, dev_msg_offsets[i+1]), and its
 * CRC-32C is stored big-endian at dev_msg_offsets[i] + hash_offset; both
 * tables hold count + 1 entries.  Message i fits iff
 *   dev_msg_offsets[i+1] - dev_msg_offsets[i]
 *       == payload_offset + (dev_src_offsets[i+1] - dev_src_offsets[i]);
 * one that does not gets dev_status[i] = 1 and is not touched, a packed one 0.
 * The call writes exactly the payload bytes and the 4 hash bytes of each
 * fitting message -- no other header byte (the caller fills those), no gap, no
 * byte past dev_msg_offsets[count] -- so dev_buf needs no padding.  Payloads
 * of any size (2 GiB and more included).  The source range and the
 * destination range must not overlap: the library cannot check that (the
 * tables are on the device), and an overlapping call copies and hashes
 * unspecified bytes.  Argument rules of mchecksum_gpu_seal_messages. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_pack_messages(const char *hash_method, const void *dev_src,
    const uint64_t *dev_src_offsets, void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

/* Scatter-gather objects: object j is the
 * concatenation, in order, of segments [dev_obj_first[j], dev_obj_first[j+1])
 * of the segment list (dev_seg_addr[s], dev_seg_len[s]) -- the shape of a bulk
 * handle's segments, HG_Bulk_create(count, buf_ptrs, buf_sizes)
 * (src/mercury_bulk.h:55,79), registered as device memory (hg_bulk_attr
 * mem_type HG_MEM_TYPE_ROCM, src/mercury_types.h:38,44-47).  dev_out[j] =
 * mchecksum_get() after one mchecksum_update() per segment of object j
 * (count = nobj host-order values; an object with no bytes gets the CRC of the
 * empty message).  All arrays are device-resident: dev_seg_addr holds device
 * addresses (each segment readable to its next 16-byte boundary),
 * dev_obj_first holds nobj + 1 non-decreasing indices <= nseg; segments
 * outside [first[0], first[nobj]) are ignored.  dev_work: caller-owned device
 * scratch (8-byte aligned) of at least mchecksum_gpu_segments_work_size(nseg)
 * bytes, not shared with a concurrent call (SIZE_MAX for nseg > 2^40, which
 * is rejected).  A call captured into a graph may be replayed after the
 * contents of dev_seg_addr, dev_seg_len and dev_obj_first have changed (every
 * replay scans the tables again), one replay at a time per workspace.
 * Every 32/64-bit method.  Segments are
 * cut into 256 KiB chunks hashed in parallel and recombined with GF(2) shift
 * operators, so one huge segment still spreads over the whole GPU. */
MCHECKSUM_PUBLIC size_t
mchecksum_gpu_segments_work_size(size_t nseg);

MCHECKSUM_PUBLIC int
mchecksum_gpu_checksum_segments(const char *hash_method,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj, void *dev_work,
    size_t work_size, void *dev_out, void *stream);

/* checksum_segments that also moves the bytes, in the same read: a bulk
 * handle's segments linearised into one contiguous buffer (gather), or a
 * contiguous object spread over the handle's segments (scatter).
 *
 * gather_segments: object j's segments, concatenated in order (N_j bytes, the
 * sum of its segment lengths), are copied to dev_dst[dev_dst_starts[j],
 * dev_dst_starts[j] + N_j) and hashed.  scatter_segments: object j =
 * dev_src[dev_src_starts[j], dev_src_starts[j] + N_j) is spread over its
 * segments in order -- dev_seg_addr are now destinations -- and hashed.
 *
 * Tables and limits.  The segment table, dev_obj_first, the workspace
 * (mchecksum_gpu_segments_work_size(nseg), one per concurrent call) and the
 * 2^40-segment cap are those of checksum_segments.  dev_dst_starts /
 * dev_src_starts hold nobj byte offsets, in any order.  The lengths live on
 * the device, so there is no fit rule and no status array, exactly as for
 * mchecksum_gpu_copy_offsets.
 *
 * Values.  dev_out[j] equals what checksum_segments returns for the same
 * tables, bit for bit, for every 32/64-bit catalogue method, MSB-first methods
 * included (their outputs are swapped after the launch, as there).  An object
 * with no bytes gets the CRC of the empty message, and nothing is written for
 * it.
 *
 * Which bytes are written.  Gather writes exactly the N_j destination bytes of
 * each object: no byte before them, after them or between objects; segment
 * memory is never written.  Scatter writes exactly dev_seg_len[s] bytes of
 * each segment s in [first[0], first[nobj]) and no other byte; dev_src is
 * never written.  Segments outside [first[0], first[nobj]) are neither read
 * nor written.  An empty segment contributes nothing.
 *
 * Memory and ordering.  The side that is read (each segment for gather, each
 * object's source range for scatter) must be readable to the next 16-byte
 * boundary after its last byte.  Written ranges must not overlap one another
 * or anything read: the library cannot check this, because the tables are on
 * the device, and an overlapping call copies and hashes unspecified bytes.
 * Calls are asynchronous and stream-ordered, and capture-safe after
 * mchecksum_gpu_prepare(): a replay scans the tables again, so lengths may
 * change between replays, and it copies the current contents.
 *
 * Failure.  The calls fail closed as checksum_segments does: error word + 1
 * once per call, and mchecksum_gpu_queue_faults().  A call whose scan gave up
 * stores nothing.  After a failed call the outputs and the written bytes are
 * unspecified.
 *
 * Arguments are checked in checksum_segments' order: NULL pointers first
 * (dev_dst / dev_src and the starts table are required when nobj > 0), then
 * the segment cap, then the workspace, then the device, then the method.
 * nobj == 0 passes those checks and returns MCHECKSUM_GPU_OK.
 *
 * Cost.  Every chunk takes the any-alignment payload loop, also where
 * checksum_segments would take its aligned or pipelined loop, so on lists of
 * 16-byte aligned KiB-multiple segments the hash itself is slower than
 * checksum_segments'; the call is meant to replace checksum_segments plus a
 * copy per segment, not checksum_segments alone (DESIGN.md 4.14 has the
 * measured shapes). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_gather_segments(const char *hash_method,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj,
    void *dev_dst, const uint64_t *dev_dst_starts,
    void *dev_work, size_t work_size, void *dev_out, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_scatter_segments(const char *hash_method,
    const void *dev_src, const uint64_t *dev_src_starts,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj,
    void *dev_work, size_t work_size, void *dev_out, void *stream);

/* Streaming over segment lists: a pipelined bulk transfer moves an object in
 * stages, each stage a list of segments.  The three calls below are
 * checksum_segments, gather_segments and scatter_segments with a running
 * state in place of the output: dev_state[j] -- the opaque element of
 * mchecksum_gpu_state_init / update_offsets / state_get, of the method's
 * size -- is advanced over object j's segments, concatenated in order.  A
 * state does not remember which call advanced it: offsets updates and
 * segments updates mix in any order.
 *
 * Values.  state_init, any sequence of these updates, then state_get equals
 * mchecksum_get() after mchecksum_update() over the same bytes in the same
 * order, bit for bit, for every 32/64-bit catalogue method.  MSB-first
 * methods included: states stay in the kernels' form, nothing is swapped.  An
 * object with no bytes leaves its state unchanged and writes nothing.
 *
 * Everything else is the one-shot call's of the same shape: which bytes are
 * written, the memory and overlap rules, the 2^40-segment cap, the workspace
 * (mchecksum_gpu_segments_work_size(nseg), one per concurrent call), the
 * work-queue and static-split rules.  An object's byte total in one call must
 * be below 2^48 (the shift tables' range, as for combine_runs); larger totals
 * read nothing out of range and leave an unspecified state.  Capture-safe
 * after mchecksum_gpu_prepare(): a replay scans the tables again and advances
 * the states again, seeded with that replay's byte totals.  One array of
 * states must not be advanced by two calls at once.
 *
 * Failure.  As the one-shot calls: error word + 1 once per call and
 * mchecksum_gpu_queue_faults().  A call whose scan gave up leaves every state
 * as it was; after any other failed call the states are unspecified.  Check
 * the error word before trusting them, as for update_offsets.
 *
 * Arguments are checked in checksum_segments' order: NULL pointers (dev_state
 * is required when nobj > 0), the segment cap, the workspace, the device, the
 * method.  nobj == 0 passes those checks and returns MCHECKSUM_GPU_OK.
 *
 * Cost.  One small launch more than the one-shot call (a thread per object
 * seeds the states between the scan and the chunk pass); the chunk passes
 * are the one-shot calls' kernels.  DESIGN.md 4.17 records what was and what
 * was not measured. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_update_segments(const char *hash_method,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj, void *dev_work,
    size_t work_size, void *dev_state, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_update_gather_segments(const char *hash_method,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj,
    void *dev_dst, const uint64_t *dev_dst_starts,
    void *dev_work, size_t work_size, void *dev_state, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_update_scatter_segments(const char *hash_method,
    const void *dev_src, const uint64_t *dev_src_starts,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj,
    void *dev_work, size_t work_size, void *dev_state, void *stream);

/* checksum_segments with the compare on the device: dev_expected holds nobj
 * host-order values of the method's size; dev_status[j] = 1 if the CRC of
 * object j's segments differs from dev_expected[j], else 0, and
 * *dev_mismatches (a device uint32_t the caller zeroes) is increased by the
 * number of mismatches.  Either of the two may be NULL.  An object with no
 * bytes is compared with the CRC of the empty message; MSB-first methods
 * compare in the checksum calls' form.  Segment memory is never written.
 * Tables, memory rules and the workspace (its size included) are
 * checksum_segments'; the values are kept in the workspace, which is why the
 * call takes fewer than 2^32 segments (more is MCHECKSUM_GPU_EINVAL, with the
 * segment cap's rank) and why a list of more than 2 nseg + 65536 chunks of
 * 256 KiB searches the scan's table per chunk instead of reading a map.
 *
 * Fail closed, as the verify calls: unhashed bytes never read as verified.
 * A call whose scan or chunk pass gave up adds 1 to the error word, once, adds
 * nobj to *dev_mismatches and sets every status to 1.  The compare runs after
 * the chunk pass and reads the call's fault state first, so a value that is
 * only half accumulated is never compared.
 *
 * Arguments are checked in checksum_segments' order, dev_expected required
 * when nobj > 0; nobj == 0 returns MCHECKSUM_GPU_OK without a launch.
 * Capture-safe after mchecksum_gpu_prepare(). */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_segments(const char *hash_method,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj, void *dev_work,
    size_t work_size, const void *dev_expected, uint8_t *dev_status,
    uint32_t *dev_mismatches, void *stream);

/* Per-field pack and unpack of RPC messages: pack_messages / unpack_messages
 * with a segment list per message in place of one contiguous range -- what
 * HG_PROC_TYPE does field by field (copy the field, feed the same bytes to
 * mchecksum_update, src/mercury_proc.h:124-143,162-181) before hg_set_struct
 * stores and hg_get_struct compares the hash (src/mercury.c:565-573,699-707).
 * One pass over the payload bytes each; CRC-32C.
 *
 * Tables.  Message j = dev_buf[dev_msg_offsets[j], dev_msg_offsets[j+1]): nobj
 * + 1 non-decreasing entries.  Its fields are segments [dev_obj_first[j],
 * dev_obj_first[j+1]) of the segment table, in order, under checksum_segments'
 * rules: segments outside every object are neither read nor written, an empty
 * segment contributes nothing.  N_j = the sum of object j's segment lengths.
 * Message j fits iff
 *   dev_msg_offsets[j+1] - dev_msg_offsets[j] == payload_offset + N_j
 * (a message shorter than payload_offset never fits; an object with no bytes
 * fits a message of exactly payload_offset bytes, and its value is the CRC of
 * the empty message).
 *
 * pack: a fitting message's segments are copied, concatenated, to
 * dev_buf[dev_msg_offsets[j] + payload_offset, dev_msg_offsets[j+1]) and hashed
 * in the same read; the CRC-32C is stored big-endian in the 4 bytes at
 * dev_msg_offsets[j] + hash_offset, and dev_status[j] = 0.  A message that does
 * not fit gets status 1, and no byte of it is written.  The call writes exactly
 * the payload bytes and the 4 hash bytes of fitting messages -- no other header
 * byte (the caller fills those), nothing before, between or after messages --
 * and never writes segment memory.  dev_status may be NULL.
 *
 * unpack: a fitting message's payload is spread over its segments in order
 * (dev_seg_addr are destinations: exactly dev_seg_len[s] bytes of each are
 * written), hashed in the same read and compared with the network-order u32 at
 * dev_msg_offsets[j] + hash_offset.  Status 0 on a match; status 1 and one
 * mismatch when the CRC differs -- the segments then hold the bytes AS
 * RECEIVED, as after unpack_messages: look at the status before the bytes.  A
 * message that does not fit gets status 1 and one mismatch, and no segment byte
 * of it is written.  dev_buf is never written.  Either of dev_status and
 * dev_mismatches may be NULL; *dev_mismatches is added to (the caller zeroes
 * it).
 *
 * Memory.  The side that is read must be readable to the next 16-byte boundary
 * (each segment for pack; dev_buf after its last message byte for unpack).
 * Written ranges must not overlap one another or anything read; the library
 * cannot check that (the tables are on the device).
 *
 * Arguments, in this order: MCHECKSUM_GPU_EINVAL for a NULL pointer (the
 * segment arrays only when nseg > 0; dev_status and dev_mismatches are
 * optional), hash_offset + 4 > payload_offset, nobj > 2^31, nseg >= 2^32, a
 * workspace smaller than mchecksum_gpu_segment_messages_work_size(nseg, nobj)
 * or not 8-byte aligned; then the method -- crc32c only, as pack_messages:
 * every other name is MCHECKSUM_GPU_EMETHOD, on a box without a GPU too --;
 * then the device.  nobj == 0 passes the same checks except those of the
 * buffers: it needs none, the workspace included, and makes no launch.
 *
 * Workspace: mchecksum_gpu_segment_messages_work_size(nseg, nobj) >=
 * mchecksum_gpu_segments_work_size(nseg): that workspace plus, per object, the
 * accumulator word of the pass and the fit gate; SIZE_MAX beyond the caps.  One
 * workspace per concurrent call.
 *
 * Asynchronous and stream-ordered; capture-safe after
 * mchecksum_gpu_prepare("crc32c").  A replay scans the tables again: segment
 * lengths, the message table and the contents may all change between replays.
 *
 * Fail closed, as verify_segments: a call whose scan gave up writes nothing --
 * no payload byte, no hash byte, no segment byte --, sets every status to 1
 * and adds 1 to the error word, once; unpack also adds nobj to
 * *dev_mismatches.  The launch after the chunk pass reads the call's fault
 * state before it stores or compares any value, so a half-accumulated CRC is
 * never sealed or accepted.
 *
 * Cost: four launches (scan, fit, chunk pass, seal or compare); the chunk pass
 * gives a wave to every field (every 256 KiB chunk of it).  Against the two
 * calls it replaces over the same tables (gather_segments + seal_messages;
 * verify_messages + scatter_segments), measured on an MI355X (DESIGN.md 4.20,
 * one run, medians): 8192 messages of 64 KiB in 4 segments, pack 0.56x and
 * unpack 0.74x the time of the pair; 65536 messages of 4 KiB in 3 unequal
 * fields at odd addresses, 0.83x both ways -- there the wave per field, not
 * the second read, is most of either route. */
MCHECKSUM_PUBLIC size_t
mchecksum_gpu_segment_messages_work_size(size_t nseg, size_t nobj);

MCHECKSUM_PUBLIC int
mchecksum_gpu_pack_segment_messages(const char *hash_method,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first, size_t nobj,
    void *dev_buf, const uint64_t *dev_msg_offsets,
    size_t payload_offset, size_t hash_offset,
    void *dev_work, size_t work_size, uint8_t *dev_status, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_unpack_segment_messages(const char *hash_method,
    const void *dev_buf, const uint64_t *dev_msg_offsets, size_t nobj,
    size_t payload_offset, size_t hash_offset,
    const uint64_t *dev_seg_addr, const uint64_t *dev_seg_len, size_t nseg,
    const uint64_t *dev_obj_first,
    void *dev_work, size_t work_size,
    uint8_t *dev_status, uint32_t *dev_mismatches, void *stream);

/* Batched check of Mercury core headers for received
 * messages in device memory: message i = dev_buf[dev_msg_offsets[i],
 * dev_msg_offsets[i+1]) starts with the 16-byte core header that
 * hg_core_header_request_proc / _response_proc encode
 * (src/mercury_core_header.c:175-289).  The 16-bit hash_method ("crc16") is
 * recomputed over the host-order field values exactly as those functions
 * stream them into mchecksum_update and compared with the big-endian hash on
 * the wire (request: offset 12, response: offset 4).  dev_status[i] = 1 on a
 * mismatch or a message shorter than 16 bytes (HG_CHECKSUM_ERROR /
 * HG_INVALID_ARG in Mercury); *dev_mismatches is incremented per failure. */
#define MCHECKSUM_GPU_CORE_HEADER_REQUEST  0
#define MCHECKSUM_GPU_CORE_HEADER_RESPONSE 1
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_core_headers(const char *hash_method, int kind,
    const void *dev_buf, const uint64_t *dev_msg_offsets, size_t count,
    uint8_t *dev_status, uint32_t *dev_mismatches, void *stream);

/* Sender side of mchecksum_gpu_verify_core_headers, with its argument rules
 * (kind, a 16-bit hash_method): the CRC over the host-order field images is
 * stored big-endian in the header's hash field (request: offset 12, response:
 * offset 4), as hg_core_header_request_proc / _response_proc encode it;
 * dev_status[i] (optional) = 0.  A message shorter than 16 bytes gets status 1
 * and is not touched.  Only the 2 hash bytes of each sealed header are
 * written. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_core_headers(const char *hash_method, int kind,
    void *dev_buf, const uint64_t *dev_msg_offsets, size_t count,
    uint8_t *dev_status, void *stream);

/* Whole RPC messages: the core header, its flags and the payload in one pass.
 * A receiver that drains a multi-recv buffer checks the core header's CRC-16
 * (hg_core_header_request_proc / _response_proc), then reads the header's
 * flags -- with HG_CORE_MORE_DATA (src/mercury_core.h:75, bit 0) the payload
 * is not in the message: it is pulled by bulk and checked later against the
 * same HG slot --, and only otherwise compares the CRC of the bytes behind the
 * headers with the HG header's hash (src/mercury_core.c:4754-4828,
 * src/mercury.c:473-594).  mchecksum_gpu_verify_core_headers and
 * mchecksum_gpu_verify_messages are the first and the third step in a launch
 * each; the second knows nothing of flags, so it reports a checksum error for
 * an overflow RPC (it hashes the bulk descriptor) and vouches for a payload
 * whose header is corrupt.  These two calls treat a message as Mercury does.
 *
 * Message i = dev_buf[dev_msg_offsets[i], dev_msg_offsets[i+1]), count + 1
 * table entries, L its length; a table that runs backwards counts as L = 0.
 * `kind` names the core header's layout, as for the core-header calls:
 *     request : 12 hashed host-order bytes, flags = byte 10, hash big-endian at 12
 *     response:  4 hashed host-order bytes, flags = byte  1, hash big-endian at  4
 * payload_offset and hash_offset are mchecksum_gpu_verify_messages'.
 *
 *   - header_method: a 16-bit model, either bit order ("crc16");
 *     payload_method: a reflected 32-bit model ("crc32c").
 *   - Arguments are checked first (MCHECKSUM_GPU_EINVAL: a NULL required
 *     pointer with count > 0, an unknown kind, count > 2^31, hash_offset < 16,
 *     hash_offset + 4 > payload_offset, hash_offset > 2^30), then the methods
 *     (_EMETHOD: a header_method that is not a 16-bit model, a payload_method
 *     that is not a reflected 32-bit one, an unknown name), then the device
 *     (_ENODEV).  count == 0 needs no buffers, but passes those checks first.
 *   - Read, launch and capture rules of verify_messages / seal_messages: any
 *     start byte, dev_buf readable to the next 16-byte boundary, payloads of
 *     any size; asynchronous and stream-ordered; capture-safe after
 *     mchecksum_gpu_prepare() of BOTH methods (a replay reads the buffer's and
 *     the table's current contents); no workspace, nothing allocated on the
 *     call path; one launch, a twin of the kernel verify_messages picks for the
 *     same count.
 *   - Fail closed: a call in which a device wait gave up adds 1 -- once -- to
 *     the error word and to mchecksum_gpu_queue_faults(), every status it
 *     cannot vouch for is MCHECKSUM_GPU_RPC_FAULT, and a verify adds `count` to
 *     dev_counts[MCHECKSUM_GPU_RPC_FAULT].  No message that fails a rule reads
 *     OK or DEFERRED; the sealed bytes of a FAULT message are unspecified.
 *   - DESIGN.md 4.22 has the design and the measurements against the two-call
 *     route. */
#define MCHECKSUM_GPU_RPC_OK       0  /* header good, payload good */
#define MCHECKSUM_GPU_RPC_PAYLOAD  1  /* header good, eager, payload CRC differs */
#define MCHECKSUM_GPU_RPC_HEADER   2  /* core header CRC-16 differs */
#define MCHECKSUM_GPU_RPC_SHORT    3  /* no whole core header, or eager and shorter
                                         than payload_offset */
#define MCHECKSUM_GPU_RPC_DEFERRED 4  /* header good, MORE_DATA set: payload elsewhere,
                                         nothing hashed or compared here */
#define MCHECKSUM_GPU_RPC_FAULT    5  /* the launch cannot vouch for this message */
#define MCHECKSUM_GPU_RPC_CLASSES  6

/* Receiver.  dev_status[i] is the first rule that matches:
 *   1. L < 16                                              -> SHORT
 *   2. the CRC-16 of the field image differs from the hash -> HEADER (whatever
 *      the flags say: the flags byte is inside the image)
 *   3. MORE_DATA set -> DEFERRED: no byte behind the core header is looked at,
 *      L may be anything >= 16; whether the HG slot exists is
 *      mchecksum_gpu_verify_detached_messages' rule, later
 *   4. L < payload_offset                                  -> SHORT
 *   5. the CRC of [payload_offset, L) differs from the network-order u32 at
 *      hash_offset                                         -> PAYLOAD
 *   6. OK
 * dev_counts: MCHECKSUM_GPU_RPC_CLASSES device uint32_t words the caller
 * zeroes; dev_counts[k] grows by the number of messages of status k.  Either of
 * dev_status and dev_counts may be NULL.  dev_buf is never written. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_rpc_messages(const char *header_method,
    const char *payload_method, int kind, const void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, uint32_t *dev_counts, void *stream);

/* Sender: the caller has filled every header byte except the two hashes.
 *   L < 16                                 -> SHORT, nothing written
 *   MORE_DATA clear, L < payload_offset    -> SHORT, nothing written (Mercury
 *                                             never sends such a message)
 *   MORE_DATA clear otherwise              -> the payload CRC big-endian at
 *       hash_offset and the header CRC-16 big-endian at 12 / 4; status OK
 *   MORE_DATA set                          -> the header CRC-16 alone; status
 *       DEFERRED (the HG slot is mchecksum_gpu_seal_detached_messages')
 * Exactly those 2 or 6 bytes of a message are written, no others. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_rpc_messages(const char *header_method,
    const char *payload_method, int kind, void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

/* Whole RPC messages with the payload moved in the same pass: what
 * mchecksum_gpu_unpack_messages and mchecksum_gpu_pack_messages do, under the
 * rules of the two calls above.  A receiver that copies payloads out of a
 * drained multi-recv buffer need not verify first and unpack afterwards (two
 * reads of every payload, and unpack_messages reports each overflow RPC as
 * corrupt); a sender that packs payloads behind pre-filled headers need not
 * split its batch by flag and seal the core headers in a launch of their own.
 *
 * Notation.  Message i, L, `kind`, `more` (bit 0 of the flags byte AS IT SITS
 * IN THE BUFFER: byte 10 of a request, byte 1 of a response) as above.  The
 * other range is [t[i], t[i+1]) of dev_dst_offsets / dev_src_offsets, count + 1
 * entries, and R its length -- a table that runs backwards gives R = 0, as it
 * gives L = 0.  Ranges are packed or not as the caller likes.
 *
 * Inherited, not restated: the argument checks and their order (EINVAL, then
 * both methods EMETHOD ahead of the device, then ENODEV; the bounds on kind,
 * count, hash_offset and payload_offset; dev_dst / dev_src and their tables
 * are required pointers with count > 0; count == 0 needs no buffers but passes
 * the checks first), the two methods, and the launch, capture and fail-closed
 * rules are verify_rpc_messages' and seal_rpc_messages'; the read padding (the
 * side that is read must be readable to the next 16-byte boundary, the written
 * side needs none) and the no-overlap rule between what is read and what is
 * written are unpack_messages' and pack_messages'.  No workspace, one launch, a
 * twin of the kernel unpack_messages / pack_messages picks for the same count.
 * Fail closed: error word + 1, once; every status the launch cannot vouch for
 * is MCHECKSUM_GPU_RPC_FAULT; an unpack adds `count` to
 * dev_counts[MCHECKSUM_GPU_RPC_FAULT]; the bytes written for a FAULT message
 * are unspecified (never outside what the rules below allow to be written).
 * DESIGN.md 4.23 has the design and the measurements. */
#define MCHECKSUM_GPU_COPY_RPC_MISFIT   6   /* eager, whole, but message size != payload_offset + range size */
#define MCHECKSUM_GPU_COPY_RPC_CLASSES  7   /* words of dev_counts for the unpack call */

/* Receiver.  dev_status[i] is the first rule that matches:
 *   1. L < 16                                              -> SHORT
 *   2. the CRC-16 of the field image differs from the hash -> HEADER
 *   3. `more`                                              -> DEFERRED
 *   4. L < payload_offset                                  -> SHORT
 *   5. L != payload_offset + R                             -> MISFIT
 *   6. the payload's CRC differs from the network-order u32 at hash_offset
 *                                                          -> PAYLOAD
 *   7. OK
 * What is written does not wait for the verdicts: message i's destination
 * range is written iff L >= 16, `more` is clear, L >= payload_offset and
 * L == payload_offset + R, and then receives exactly the R payload bytes AS
 * RECEIVED -- whatever rules 2 and 6 say: look at the status before the bytes,
 * as after unpack_messages.  So a HEADER message that passes that test is
 * copied, and one that does not is untouched.  For a DEFERRED, SHORT or MISFIT
 * message no destination byte is written, whatever R is, and no byte behind
 * the core header is read; a DEFERRED message's R is not looked at.  Nothing
 * else is written: nothing before t[0], in a skipped range, or past t[count];
 * dev_buf is never written.  dev_counts: MCHECKSUM_GPU_COPY_RPC_CLASSES words
 * the caller zeroes, dev_counts[k] grows by the number of messages of status k.
 * Either of dev_status and dev_counts may be NULL. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_unpack_rpc_messages(const char *header_method,
    const char *payload_method, int kind, const void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, void *dev_dst, const uint64_t *dev_dst_offsets,
    uint8_t *dev_status, uint32_t *dev_counts, void *stream);

/* Sender: the caller has filled every header byte of dev_buf except the two
 * hashes; the flags byte is read from dev_buf.  First rule that matches:
 *   1. L < 16                   -> SHORT: nothing written, source range not read
 *   2. `more`                   -> DEFERRED: the header CRC-16 alone (2 bytes);
 *                                  source range not read, whatever R is
 *   3. L < payload_offset       -> SHORT: nothing written
 *   4. L != payload_offset + R  -> MISFIT: nothing written
 *   5. OK: the R source bytes are copied to dev_buf[mo[i] + payload_offset,
 *      mo[i+1]), their CRC is stored big-endian at hash_offset and the header
 *      CRC-16 big-endian at 12 (request) or 4 (response)
 * Exactly those R + 6 or 2 bytes of a message are written: no other header
 * byte, no gap, nothing past the last message.  dev_src is never written.
 * dev_status may be NULL. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_pack_rpc_messages(const char *header_method,
    const char *payload_method, int kind, const void *dev_src,
    const uint64_t *dev_src_offsets, void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

/* The four calls above with the message side addressed by a LIST: what a
 * receiver holds after draining several multi-recv buffers (one actual_buf /
 * actual_buf_size pair per completion, src/na/na_types.h:187), and what a
 * sender holds with an out_buf per handle.  One table cannot name messages
 * that lie in several allocations, with gaps, in any order; two arrays can.
 *
 * Message side.  Message i is the dev_msg_len[i] bytes at the device address
 * dev_msg_addr[i]: both arrays are device-resident, `count` entries each (not
 * count + 1), as dev_seg_addr / dev_seg_len of the segment calls.  L =
 * dev_msg_len[i]; a message whose end would pass the end of the address space
 * counts as L = 0, as a table that runs backwards does.  Messages may lie in
 * any number of allocations, in any order, with any gaps, at any byte
 * alignment.  Messages that are WRITTEN (seal, pack) must not overlap one
 * another; an unpack's destination and a pack's source must not overlap the
 * messages.
 *
 * Other side (unpack, pack): the table form as it is -- dev_dst / dev_src with
 * count + 1 offsets, R and the backwards rule as above.  A list on both sides
 * is not offered.
 *
 * Inherited word for word, not restated: the rule ladders and the statuses of
 * the table call of the same name, dev_counts (6 words for verify, 7 for
 * unpack), exactly which bytes are written, "what is written does not wait
 * for the verdicts", both header bit orders and a reflected 32-bit payload
 * method, the argument bounds and their order (EINVAL, then both methods
 * EMETHOD ahead of the device, then ENODEV; dev_msg_addr and dev_msg_len are
 * required pointers with count > 0; count == 0 needs no buffers but passes the
 * checks first), the launch rules, and the fail-closed rules.  Capture-safe
 * after mchecksum_gpu_prepare() of BOTH methods; a replay reads the current
 * contents of both arrays, so a captured call serves the next drain by
 * rewriting them in place.  No workspace, one launch: a twin of the kernel
 * the table call picks for the same count.
 *
 * Reads.  Per message, in aligned 16-byte pieces that stay inside the aligned
 * 128-byte lines holding the first and the last byte the call reads of that
 * message: any message lying inside a device allocation satisfies this, and
 * nothing between, before or behind messages is read into a verdict.  A
 * message with L < 16 is SHORT and its address is never dereferenced (it may
 * be NULL).  A DEFERRED message is read in its first 16 bytes only, and so is
 * an eager one shorter than payload_offset or -- unpack, pack -- one that
 * does not fit.  Nothing outside the messages and the other range is written.
 * DESIGN.md 4.25 has the design and the measurements against the table calls.
 * The DEFERRED messages of a list go on to
 * mchecksum_gpu_verify_detached_message_list as they are: a sub-list of the
 * same two arrays. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_rpc_message_list(const char *header_method,
    const char *payload_method, int kind, const uint64_t *dev_msg_addr,
    const uint64_t *dev_msg_len, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, uint32_t *dev_counts, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_rpc_message_list(const char *header_method,
    const char *payload_method, int kind, const uint64_t *dev_msg_addr,
    const uint64_t *dev_msg_len, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_unpack_rpc_message_list(const char *header_method,
    const char *payload_method, int kind, const uint64_t *dev_msg_addr,
    const uint64_t *dev_msg_len, size_t count, size_t payload_offset,
    size_t hash_offset, void *dev_dst, const uint64_t *dev_dst_offsets,
    uint8_t *dev_status, uint32_t *dev_counts, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_pack_rpc_message_list(const char *header_method,
    const char *payload_method, int kind, const void *dev_src,
    const uint64_t *dev_src_offsets, const uint64_t *dev_msg_addr,
    const uint64_t *dev_msg_len, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

/* XDR-mode proc checksum.  In a Mercury built with
 * MERCURY_USE_XDR (HG_HAS_XDR) the serialized buffer holds XDR -- every
 * integer big-endian and rounded up to 4 bytes, byte arrays zero-padded to a
 * multiple of 4 -- while the proc checksum covers the HOST-order field values
 * (src/mercury_proc.h:110-122,147-160).  The whole-buffer entry points above
 * are exact only for the default non-XDR encoding; they cannot tell an XDR
 * buffer apart and must not be used on one.  This entry point takes the
 * message's field schema instead, the sequence of hg_proc_* calls its proc
 * function makes:
 *   MCHECKSUM_XDR_INT         size 1, 2, 4 or 8: hg_proc_[u]int<8*size>_t
 *                             (wire: 4 or 8 bytes big-endian; hashed: the
 *                             size little-endian bytes of the value)
 *   MCHECKSUM_XDR_OPAQUE      size bytes of hg_proc_bytes/raw/memcpy (wire:
 *                             the bytes + zero pad to a multiple of 4)
 *   MCHECKSUM_XDR_OPAQUE_LEN  as OPAQUE, byte count = the value of the last
 *                             INT field (hg_string_t: u64 length, then bytes)
 *   MCHECKSUM_XDR_RAW         size bytes reserved by hg_proc_save_ptr and
 *                             hashed by hg_proc_restore_ptr (exact size, no
 *                             XDR rounding; src/mercury_proc.c:277-335)
 *   MCHECKSUM_XDR_RAW_LEN     as RAW, size = the last INT field's value
 *                             (bulk handles, src/mercury_proc_bulk.c:91-125)
 *   MCHECKSUM_XDR_SKIP_IF_ZERO if the last INT field was 0, skip the next
 *                             `size` schema entries (an empty hg_string_t
 *                             carries no bytes and no flags)
 *   MCHECKSUM_XDR_SINT        INT for a signed type (hg_proc_int<8*size>_t):
 *                             mchecksum_gpu_pack_xdr_messages sign-extends a
 *                             1-, 2- or 4-byte value into its 32-bit word
 *                             where INT zero-extends.  Every other call
 *                             treats it exactly as INT -- the low `size`
 *                             bytes are hashed and decoded, and the value a
 *                             following _LEN or SKIP entry reads is the
 *                             zero-extended one -- so one schema serves
 *                             sender and receiver
 * Message i = dev_buf[dev_msg_offsets[i], dev_msg_offsets[i+1]) starting
 * where the proc buffer starts; dev_out[i] = the value hg_proc_checksum_get
 * returns for it (host-order, method size).  dev_status[i] (optional) = 1
 * when the schema runs past the message (dev_out[i] is then 0).  At most 64
 * schema entries; reflected 32/64-bit methods (crc32c, crc64). */
#define MCHECKSUM_XDR_INT          0
#define MCHECKSUM_XDR_OPAQUE       1
#define MCHECKSUM_XDR_OPAQUE_LEN   2
#define MCHECKSUM_XDR_RAW          3
#define MCHECKSUM_XDR_RAW_LEN      4
#define MCHECKSUM_XDR_SKIP_IF_ZERO 5
#define MCHECKSUM_XDR_SINT         6
typedef struct mchecksum_xdr_field {
    uint32_t kind;
    uint32_t size;
} mchecksum_xdr_field_t;

MCHECKSUM_PUBLIC int
mchecksum_gpu_checksum_xdr(const char *hash_method,
    const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, void *dev_out,
    uint8_t *dev_status, void *stream);

/* XDR-mode messages in place: the three calls a non-XDR build makes with
 * mchecksum_gpu_verify_messages, _seal_messages and _unpack_messages, for a
 * Mercury built with MERCURY_USE_XDR.  Message i = dev_buf[dev_msg_offsets[i],
 * dev_msg_offsets[i+1]); its proc buffer -- what mchecksum_gpu_checksum_xdr
 * calls the message -- starts payload_offset bytes in, and the header hash is
 * the network-order u32 at hash_offset, hash_offset + 4 <= payload_offset
 * (Mercury: 20 and 16).  fields / nfields: checksum_xdr's schema, with its
 * rules; bytes after the schema's end are ignored (slices of a multi-recv
 * buffer carry slack).  The header slot is 32 bits: reflected 32-bit methods
 * only (crc32c, crc32); every other method gives MCHECKSUM_GPU_EMETHOD.
 * Arguments are checked in this order: MCHECKSUM_GPU_EINVAL (NULL pointers,
 * the offsets rule, a bad schema, count > 2^31), then the method, then the
 * device; count == 0 needs no buffers and passes the same checks.
 *
 * verify: dev_status[i] = 1 when the message is shorter than payload_offset,
 *   the schema runs past it, or the value checksum_xdr would return differs
 *   from the header hash; else 0.  *dev_mismatches (zeroed by the caller) is
 *   increased by the number of failures.  Either may be NULL.  dev_buf is
 *   not written.
 * seal: the value is stored big-endian in the 4 hash bytes, dev_status[i] =
 *   0; a short or truncated message gets status 1 and is not written.  No
 *   other byte is written.
 * unpack: verify, and in the same pass the hashed stream -- the little-endian
 *   `size` bytes of every INT, the unpadded bytes of every OPAQUE and RAW
 *   field, in schema order: the message's non-XDR image -- is written to
 *   dev_dst[dev_dst_offsets[i], dev_dst_offsets[i+1]) (count + 1 entries).  A
 *   message fits when its decoded length, which depends on its data, equals
 *   its slot's length; one that is short, truncated or does not fit gets
 *   status 1, one mismatch and no destination byte written.  A fitting
 *   message whose CRC differs gets status 1, one mismatch, and its slot holds
 *   the bytes as decoded: look at the status before the bytes.  Exactly the
 *   destination bytes of fitting messages are written.  dev_buf is not
 *   written; the two ranges must not overlap.
 *
 * Launch, work-queue slot and graph capture as checksum_xdr (capture-safe
 * after mchecksum_gpu_prepare(); a replay reads the buffer's current
 * contents).  Fail closed: a call whose throughput layout gave up a wait adds
 * 1 to the error word, adds count to *dev_mismatches and sets every status to
 * 1; hash slots (seal) and destination bytes (unpack) of messages it cannot
 * vouch for are unspecified.  (Statuses are flagged by a short launch after
 * the walk, made only by calls that hold a work-queue slot and pass
 * dev_status.) */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_xdr_messages(const char *hash_method,
    const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, uint32_t *dev_mismatches,
    void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_xdr_messages(const char *hash_method,
    const mchecksum_xdr_field_t *fields, size_t nfields, void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_unpack_xdr_messages(const char *hash_method,
    const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, void *dev_dst, const uint64_t *dev_dst_offsets,
    uint8_t *dev_status, uint32_t *dev_mismatches, void *stream);

/* XDR-mode sender: encode, hash and seal in one pass -- what
 * mchecksum_gpu_pack_messages is for the default build, and the mirror of
 * mchecksum_gpu_unpack_xdr_messages.  Source i = dev_src[dev_src_offsets[i],
 * dev_src_offsets[i+1]) (count + 1 entries, as dev_msg_offsets) is message
 * i's non-XDR image in schema order: the little-endian `size` bytes of every
 * INT / SINT, then the unpadded bytes of every OPAQUE and RAW field -- byte
 * for byte what unpack_xdr_messages writes.  It may start at any byte and
 * must be readable up to the next 16-byte boundary.  The walk follows the
 * schema over the image and writes its XDR encoding to
 * dev_buf[dev_msg_offsets[i] + payload_offset, dev_msg_offsets[i+1]):
 * integers big-endian in 4- or 8-byte slots (INT zero-extended, SINT
 * sign-extended), OPAQUE bytes followed by a zero pad to a multiple of 4, RAW
 * fields at their exact size; a _LEN field takes its byte count from the
 * preceding integer as read from the image, SKIP_IF_ZERO as in the other
 * calls.  In the same read it hashes the image -- the hashed stream -- and
 * stores the value big-endian in the 4 bytes at dev_msg_offsets[i] +
 * hash_offset.
 *
 * Message i fits iff the schema consumes the image exactly (it neither runs
 * past the image's end nor stops short of it) and dev_msg_offsets[i+1] -
 * dev_msg_offsets[i] == payload_offset + the encoded length, with no slack
 * (mchecksum_gpu_xdr_encoded_sizes computes that length).  A message that
 * does not fit gets dev_status[i] = 1 and no byte of it is written; a packed
 * one gets 0 (dev_status may be NULL).  Exactly the XDR bytes (pads included)
 * and the 4 hash bytes of fitting messages are written: no other header byte,
 * nothing before, between or after them, and dev_src is never written.  The
 * source and destination ranges must not overlap (not checked).
 *
 * Methods, the order of the argument checks (the NULL pointers here: fields,
 * dev_src, dev_src_offsets, dev_buf, dev_msg_offsets), layout, work-queue slot
 * and graph capture as the other XDR message calls (capture-safe after
 * mchecksum_gpu_prepare(); a replay reads the current contents and tables).
 * Fail closed, like seal: a call whose throughput layout gave up a wait adds
 * 1 to the error word and sets every status to 1; the written bytes of
 * messages it cannot vouch for are unspecified.  There is no mismatch counter
 * on the sender side.
 *
 * Cost (MI355X): the one pass takes 0.77x (8192 x 64 KiB) and
 * 0.87x (65536 x 4 KiB) the time of a device copy of the wire bytes followed
 * by mchecksum_gpu_seal_xdr_messages, and what unpack_xdr_messages takes. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_pack_xdr_messages(const char *hash_method,
    const mchecksum_xdr_field_t *fields, size_t nfields, const void *dev_src,
    const uint64_t *dev_src_offsets, void *dev_buf,
    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
    size_t hash_offset, uint8_t *dev_status, void *stream);

/* Whole RPC messages of an XDR build: the core header, its flags and the
 * fields in one pass -- what mchecksum_gpu_verify_rpc_messages and its three
 * siblings are for the default build.  The core header is not XDR-encoded
 * (hg_core_header_request_proc / _response_proc are the same in both builds),
 * so an XDR receiver that drains a multi-recv buffer stood where the default
 * build did: a launch of verify_core_headers and one of verify_xdr_messages,
 * two status arrays to join on the host, a payload vouched for under a corrupt
 * header, and every message flagged MORE_DATA reported corrupt because the
 * schema was walked over its bulk descriptor (Mercury's XDR sender refuses to
 * make such messages, src/mercury.c:718-721; a receiver must not trust a peer
 * on that).  These four calls run the XDR walk inside the RPC frame.
 *
 * By reference, not restated:
 *   - Message i, L, `kind`, `more` (bit 0 of the flags byte as it sits in the
 *     buffer), the other range and R, the backwards-table rule, hash_offset >=
 *     16, hash_offset + 4 <= payload_offset and the 2^30 cap on hash_offset:
 *     the plain RPC calls' (mchecksum_gpu_verify_rpc_messages ..
 *     mchecksum_gpu_pack_rpc_messages).
 *   - fields / nfields, the 64-entry cap, MCHECKSUM_XDR_SINT, "bytes after the
 *     schema's end are ignored" on the receiver and "the schema consumes the
 *     image exactly, the message has no slack" on the sender, the image's
 *     layout, the read padding and the no-overlap rule: the XDR message calls'
 *     (mchecksum_gpu_verify_xdr_messages .. mchecksum_gpu_pack_xdr_messages).
 *   - header_method: a 16-bit model of either bit order; payload_method: a
 *     reflected 32-bit model.
 *   - Argument checks, in this order: MCHECKSUM_GPU_EINVAL (a NULL required
 *     pointer with count > 0, an unknown kind, the offsets rules, a bad
 *     schema, count > 2^31), then both methods' _EMETHOD ahead of the device,
 *     then _ENODEV.  count == 0 needs no buffers but passes the same checks.
 *   - Statuses: MCHECKSUM_GPU_RPC_* and, for the copying two,
 *     MCHECKSUM_GPU_COPY_RPC_MISFIT; dev_counts: MCHECKSUM_GPU_RPC_CLASSES
 *     words for verify, MCHECKSUM_GPU_COPY_RPC_CLASSES for unpack, zeroed by
 *     the caller; dev_status and dev_counts may each be NULL.
 *   - Layout, work-queue slot and loads as the XDR message calls pick them for
 *     the same count; asynchronous and stream-ordered; no workspace; capture-
 *     safe after mchecksum_gpu_prepare() of BOTH methods (a replay reads the
 *     current contents).  Fail closed: a call whose throughput layout gave up
 *     a wait adds 1 to the error word, a verify or unpack adds `count` to
 *     dev_counts[MCHECKSUM_GPU_RPC_FAULT], and every status becomes
 *     MCHECKSUM_GPU_RPC_FAULT (flagged by a short launch after the walk, made
 *     only by calls that hold a work-queue slot and pass dev_status); bytes
 *     written for messages it cannot vouch for are unspecified.
 *
 * First rule that matches.
 * verify:
 *   1. L < 16                                    -> SHORT (no byte is read)
 *   2. the core header's CRC-16 differs          -> HEADER
 *   3. `more`                                    -> DEFERRED: no byte behind
 *                                                   the core header is read
 *   4. L < payload_offset                        -> SHORT
 *   5. the schema runs past the message          -> SHORT (shorter than its own
 *                                                   fields need)
 *   6. the value checksum_xdr would return differs from the network-order u32
 *      at hash_offset                            -> PAYLOAD
 *   7. OK
 * unpack: rules 1-5, then decoded length != R -> MISFIT, then PAYLOAD, then
 *   OK.  What is written does not wait for the verdicts: message i's
 *   destination range is written iff L >= 16, `more` is clear, L >=
 *   payload_offset, the schema fits and the decoded length == R; it then holds
 *   the decoded bytes AS RECEIVED, whatever rules 2 and 6 say.  Nothing of a
 *   SHORT, DEFERRED or MISFIT message's range is written.
 * seal:
 *   1. L < 16                                    -> SHORT, nothing written
 *   2. `more`                                    -> DEFERRED, the header's
 *                                                   CRC-16 alone (2 bytes)
 *   3. L < payload_offset, or the schema runs past the message
 *                                                -> SHORT, nothing written
 *   4. OK: the value big-endian at hash_offset and the CRC-16 at 12 (request)
 *      or 4 (response): exactly those 6 bytes.
 * pack:
 *   1. L < 16                                    -> SHORT
 *   2. `more`                                    -> DEFERRED: the CRC-16 alone,
 *                                                   the source range is not read
 *   3. L < payload_offset                        -> SHORT
 *   4. the schema does not consume the image exactly, or L != payload_offset +
 *      the encoded length                        -> MISFIT, nothing written
 *   5. OK: exactly the XDR bytes (pads included), the 4 hash bytes and the 2
 *      CRC-16 bytes.
 *
 * Not offered: 64-bit payload methods (the HG slot is 32 bits).
 * Cost (MI355X), each call against the two launches it
 * replaces (the core-header call and the XDR message call), iovec schema:
 * 0.97 .. 1.00x at 8192 x 64 KiB and 0.81 .. 0.90x at 64 x 4 KiB, but SLOWER
 * at 65536 x 4 KiB -- verify 1.05x, seal 1.07x, unpack 1.03x, pack 1.09x,
 * beyond the measurement's spread: there the header read ahead of each
 * message's walk is not hidden.  A caller of that shape that needs neither the
 * DEFERRED class nor one status array may keep the two launches. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_rpc_xdr_messages(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, const void *dev_buf, const uint64_t *dev_msg_offsets,
    size_t count, size_t payload_offset, size_t hash_offset,
    uint8_t *dev_status, uint32_t *dev_counts, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_rpc_xdr_messages(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, void *dev_buf, const uint64_t *dev_msg_offsets,
    size_t count, size_t payload_offset, size_t hash_offset,
    uint8_t *dev_status, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_unpack_rpc_xdr_messages(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, const void *dev_buf, const uint64_t *dev_msg_offsets,
    size_t count, size_t payload_offset, size_t hash_offset, void *dev_dst,
    const uint64_t *dev_dst_offsets, uint8_t *dev_status, uint32_t *dev_counts,
    void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_pack_rpc_xdr_messages(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, const void *dev_src, const uint64_t *dev_src_offsets,
    void *dev_buf, const uint64_t *dev_msg_offsets, size_t count,
    size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
    void *stream);

/* The four calls above with the message side addressed by a LIST, as
 * mchecksum_gpu_verify_rpc_message_list and its siblings are for the default
 * build: the core header and the NA layer are the same in an XDR build, so
 * its receiver drains several multi-recv buffers into one actual_buf /
 * actual_buf_size pair per completion and its sender holds an out_buf per
 * handle all the same.  dev_buf and dev_msg_offsets become dev_msg_addr and
 * dev_msg_len, device-resident, `count` entries each (not count + 1).
 *
 * Inherited word for word from the table call of the same name
 * (mchecksum_gpu_verify_rpc_xdr_messages .. _pack_rpc_xdr_messages), not
 * restated: the rule ladders, the statuses and dev_counts (6 words for verify,
 * 7 for unpack), exactly which bytes are written and "what is written does
 * not wait for the verdicts", the schema rules (slack ignored on the
 * receiver, an exact fit on the sender), a reflected 32-bit payload method
 * and both 16-bit header bit orders, the argument checks and their order
 * (EINVAL, then both methods' EMETHOD ahead of the device, then ENODEV;
 * dev_msg_addr and dev_msg_len are required pointers with count > 0; count ==
 * 0 needs no buffers but passes the checks first), the layout, the work-queue
 * slot, and the fail-closed rules with MCHECKSUM_GPU_RPC_FAULT flagged by the
 * short launch after the walk.  One launch, no workspace: the LIST twin of the
 * kernel the table call picks for the same count.
 *
 * Inherited from the plain list calls (mchecksum_gpu_verify_rpc_message_list
 * ..), not restated: L = dev_msg_len[i], a message whose end would pass the
 * end of the address space counts as L = 0; messages in any number of
 * allocations, in any order, with any gaps, at any byte alignment; written
 * messages must not overlap one another and the other side must not overlap
 * the messages; the other side of unpack and pack stays a table (dev_dst /
 * dev_src with count + 1 offsets); capture-safe after mchecksum_gpu_prepare()
 * of BOTH methods, and a captured call serves the next drain by rewriting the
 * two arrays in place.
 *
 * Reads, of this form (narrower than the plain list calls').  A message with
 * L < 16 is SHORT and its address is never dereferenced (it may be NULL).
 * From 16 bytes on the 16 core header bytes are read, one byte a lane, and of
 * a DEFERRED message, of an eager one shorter than payload_offset and of a
 * pack's message, whatever its class, nothing else: a pack reads the header
 * and writes the rest.  An unpack's MISFIT is not header-only: the decoded
 * length is known only from the message's integer fields, which are read
 * (bytes of the message) before it is rejected.  Of every other message the
 * walk reads bytes of the message only -- the integers, the hash slot and
 * every field of fewer than 256 bytes byte by byte, whatever the layout --
 * with one exception: in the throughput layout (count > 1024, or
 * MCHECKSUM_GPU_XDR_FAST=1) an opaque or raw field of 256 bytes or more is
 * read in aligned 16-byte pieces, from the piece holding the field's first
 * byte (at most 15 bytes before it: header or field bytes of the same message,
 * since a field starts payload_offset >= 20 bytes in) to the end of the
 * aligned 128-byte line holding the field's last byte (at most 127 bytes
 * behind it, which may lie behind the message).  No byte before a message is
 * ever read, and none behind it outside the 128-byte line that holds one of
 * its own bytes: any message lying inside a device allocation satisfies this.
 * The bytes so read beside a field are masked out of its CRC; nothing
 * between, before or behind messages enters a verdict or is written.  A pack
 * reads its fields from the SOURCE images, so its 16-byte pieces fall there,
 * by the table call's read-padding rule for dev_src, never on a message.
 * Cost (MI355X, DESIGN.md 4.28, iovec schema, 64 x 4 KiB, 65536 x 4 KiB and
 * 8192 x 64 KiB): no difference from the table call of the same name shows
 * beyond the measurement's own spread -- every cell within about 4% either
 * way, on the table's bytes and with the messages shuffled over 64
 * allocations, which is how far identical table kernels of two builds
 * measured apart in the same run.  Some cells are slower, some faster; none
 * was shown to be the list form's doing.  DESIGN.md 4.28 has the table. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_verify_rpc_xdr_message_list(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len,
    size_t count, size_t payload_offset, size_t hash_offset,
    uint8_t *dev_status, uint32_t *dev_counts, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_seal_rpc_xdr_message_list(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len,
    size_t count, size_t payload_offset, size_t hash_offset,
    uint8_t *dev_status, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_unpack_rpc_xdr_message_list(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len,
    size_t count, size_t payload_offset, size_t hash_offset, void *dev_dst,
    const uint64_t *dev_dst_offsets, uint8_t *dev_status, uint32_t *dev_counts,
    void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_pack_rpc_xdr_message_list(const char *header_method,
    const char *payload_method, int kind, const mchecksum_xdr_field_t *fields,
    size_t nfields, const void *dev_src, const uint64_t *dev_src_offsets,
    const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
    size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
    void *stream);

/* The data-dependent lengths the XDR message tables are built from, computed
 * where the data is: one small launch per call that reads the integer fields
 * only, with the walks' own bounds tests.
 *
 * encoded_sizes: dev_sizes[i] = the XDR length pack_xdr_messages would write
 *   for image i = dev_src[dev_src_offsets[i], dev_src_offsets[i+1]); 0, with
 *   dev_status[i] = 1, when the schema does not consume the image exactly.
 *   An exclusive prefix sum of payload_offset + dev_sizes is the message
 *   table pack_xdr_messages accepts.
 * decoded_sizes: dev_sizes[i] = the decoded length of message i (what decides
 *   unpack_xdr_messages' fit; their exclusive prefix sum is its destination
 *   table); dev_wire_sizes[i] (optional, may be NULL) = the XDR bytes the
 *   schema consumed from payload_offset on, so a receiver can tell the slack.
 *   Both are 0, with dev_status[i] = 1, when the message is shorter than
 *   payload_offset or the schema runs past it.
 *
 * dev_status may be NULL; a sized entry gets 0.  No hash method, no tables,
 * no work-queue slot, no workspace and no wait on the device: nothing to fail
 * closed on, and capture-safe without mchecksum_gpu_prepare().
 * MCHECKSUM_GPU_EINVAL (NULL pointers, a bad schema, count > 2^31) comes
 * before the device check; count == 0 needs no buffers. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_xdr_encoded_sizes(const mchecksum_xdr_field_t *fields,
    size_t nfields, const void *dev_src, const uint64_t *dev_src_offsets,
    size_t count, uint64_t *dev_sizes, uint8_t *dev_status, void *stream);

MCHECKSUM_PUBLIC int
mchecksum_gpu_xdr_decoded_sizes(const mchecksum_xdr_field_t *fields,
    size_t nfields, const void *dev_buf, const uint64_t *dev_msg_offsets,
    size_t count, size_t payload_offset, uint64_t *dev_sizes,
    uint64_t *dev_wire_sizes, uint8_t *dev_status, void *stream);

/* Lanes cooperating on one payload that checksum_fixed would choose for
 * this length (1..64) in a batch large enough to fill the device; a smaller
 * batch gets more lanes per payload until it fills every wave slot (a small
 * one in the light layout may get fewer).  For reporting; -1 on error. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_lanes_per_payload(const char *hash_method, size_t len);

/* Fail-closed report for the batch calls this host thread makes from now on:
 * each call whose launch could not hash every payload adds 1 to *dev_word
 * (a device-resident uint32_t the caller owns, zeroes and reads after the
 * calls' streams are synchronized).  The word is captured by value into
 * graph-captured calls.  NULL (the default) turns the report off; the
 * process-wide count mchecksum_gpu_queue_faults() is always kept. */
MCHECKSUM_PUBLIC int
mchecksum_gpu_set_error_word(uint32_t *dev_word);

/* Human-readable text for the last error on this thread. */
MCHECKSUM_PUBLIC const char *
mchecksum_gpu_last_error(void);

/* Re-read the MCHECKSUM_* environment settings (normally read once, at first
 * use) for calls made from now on -- for tests and tuning tools that change
 * the environment between calls; calls already made are not affected. */
MCHECKSUM_PUBLIC void
mchecksum_gpu_reload_settings(void);

/* Diagnostics: the number of work-queue protocol faults the batch kernels
 * counted on the current device since the library was loaded (0 in a
 * healthy run; every wait inside a launch is bounded, and a wait that gives
 * up is counted here instead of hanging the GPU).  Synchronizes the device.
 * Returns -1 without a usable device. */
MCHECKSUM_PUBLIC long long
mchecksum_gpu_queue_faults(void);

/* Diagnostics: work-queue slot bookkeeping of the current device since the
 * library was loaded, written to stats[0 .. min(n, MCHECKSUM_GPU_QSTAT_COUNT)):
 * launches given a slot, launches that took the static split for want of one
 * (graph captures, no idle slot), slots returned to the idle pool once their
 * launch had completed, busy in-flight slots looked at while reaping, and
 * slots handed out and not yet reaped.  Host-side counters only: no device
 * sync. */
#define MCHECKSUM_GPU_QSTAT_SLOT 0
#define MCHECKSUM_GPU_QSTAT_NOSLOT 1
#define MCHECKSUM_GPU_QSTAT_REAPED 2
#define MCHECKSUM_GPU_QSTAT_BUSY_SKIP 3
#define MCHECKSUM_GPU_QSTAT_IN_FLIGHT 4
#define MCHECKSUM_GPU_QSTAT_COUNT 5
MCHECKSUM_PUBLIC int
mchecksum_gpu_queue_stats(long long *stats, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* MCHECKSUM_GPU_H */
