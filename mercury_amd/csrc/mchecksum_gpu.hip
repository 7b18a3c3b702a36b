// mchecksum_gpu.hip -- MI355X (gfx950) batch CRC kernels behind the C ABI in
// include/mchecksum_gpu.h.
//
// What is computed.  For each payload i, the value mchecksum_get() returns
// after mchecksum_update(payload_i) -- the CRC Mercury stores in the HG header
// for a serialized proc buffer (src/mercury_proc.c:358-406,
// src/mercury.c:699-707, src/mercury_header.c:111-112).
//
// How (algebra in crc_gpu_layout.h; validated by tests/native/kernel_emulator):
//  * A payload is covered by a 16-byte-aligned window whose END is aligned to
//    the step grid; G lanes (one group) cover one step of 16*G bytes, each lane
//    one coalesced dwordx4 (so a G = 64 wave reads 1 KiB per instruction).
//  * Every W-bit word slot of a lane is an independent sub-stream with a
//    uniform stride of 16*G bytes, so "advance by the stride" is folded into
//    the lookup tables: s <- F(s ^ w) costs 4 byte lookups (CRC-32C) or 16
//    nibble lookups (CRC-64) and no shift/multiply.
//  * Lookup tables live in LDS, laid out so that every ds_read_b32/b64 is
//    conflict-free: CRC-32C byte tables and CRC-64 low-nibble tables are
//    replicated 32x (lane l reads copy l % 32), CRC-64 high-nibble tables sit
//    at a 16-B entry stride.  One VALU op forms each lookup address (v_perm_b32
//    or v_and_b32_sdwa: the byte or nibble as entry, the lane copy in the low
//    byte).
//  * Sub-streams are combined by a tree (in-lane, then xor-shuffles across the
//    group) whose level operators Z^-(2^k * W/8) are nibble tables in LDS;
//    Z^-t removes the t pad bytes after the payload end.
//  * Persistent grid: one 1024-thread workgroup per CU for CRC-32C (the
//    replicated tables take 128 KiB of the 160 KiB LDS), two for CRC-64.  Waves
//    take payloads from a device-side work queue (large aligned CRC-32C and
//    all offsets batches) or by a static stride (crc_gpu_shape.h, dyn_policy).
//    Batches <= 16 MiB take a light layout: unreplicated tables, 256-thread
//    workgroups on every CU.
//  * Host side: each entry point validates its arguments, resolves the method
//    once (resolve_model), takes the device context, decides the whole launch
//    in one pure plan from one settings snapshot (launch_plan.h: plan_fixed,
//    plan_offsets), fetches the table pack for the plan's lane count, names
//    the kernel for the plan and the call's operation (launch_plan.h: BatchOp,
//    kernel_key), looks it up (kernel_for) and launches it with its
//    work-queue slot, if the plan takes one (gpu_host.h: launch_slot).  The
//    offsets-shaped calls share one front, offsets_call.  The two
//    copy-and-checksum calls have copy_call beside it: the same plan, pack and
//    slot, and a kernel of the copy family (crc_gpu_copy.h, copy_plan.h).
// No MFMA: this is HBM-bound byte scanning; the roofline is HBM read bandwidth.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <type_traits>

#include "copy_plan.h"
#include "crc_gpu_copy.h"
#include "crc_gpu_device.h"
#include "gpu_host.h"
#include "launch_plan.h"
#include "mchecksum_gpu.h"
#include "mchecksum_models.h"
#include "offsets_call.h"
#include "seg_plan.h"

namespace mck {
// ------------------------------------------------------------ host side ----

thread_local char t_err[256] = "";
// mchecksum_gpu_set_error_word(): device word bumped by a launch that could
// not hash every payload (per host thread; nullptr = none).  Launches read it
// through error_word().
static thread_local uint32_t *t_err_word = nullptr;
uint32_t *error_word() { return t_err_word; }

int set_err(int rc, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof(t_err), fmt, ap);
    va_end(ap);
    return rc;
}

int hip_err(hipError_t e, const char *what) {
    snprintf(t_err, sizeof(t_err), "%s: %s", what, hipGetErrorString(e));
    return MCHECKSUM_GPU_EHIP;
}

std::mutex g_mu;
DevCtx g_dev[kMaxDev];

// Method -> model for GPU-capable (32/64-bit) models.
int gpu_model(const char *method, Model *out) {
    const int idx = mck_model_index(method);
    if (idx < 0) return -1;
    const mck_model_t &m = mck_models[idx];
    if (m.width != 32 && m.width != 64) return -2;
    *out = Model{idx, m.width, !m.reflected};
    return 0;
}

int resolve_model(const char *method, Model *out) {
    const int r = gpu_model(method, out);
    if (r == -1) return set_err(MCHECKSUM_GPU_EMETHOD, "unknown hash method \"%s\"", method ? method : "(null)");
    if (r < 0) return set_err(MCHECKSUM_GPU_EMETHOD, "method \"%s\" has no GPU kernel (32/64-bit only)", method);
    return MCHECKSUM_GPU_OK;
}

// A reflected model as is; an MSB-first model as the reflected model of the
// same polynomial over bit-reversed bytes, conjugated by R (crc_gpu_layout.h):
// rinit / xorout reflected, then R-mapped.
// (crc_gpu_seed.h has the construction, so the CPU tests build the same model)
crc_rmodel_t gpu_rmodel(int idx) { return mck_gpu_rmodel(&mck_models[idx]); }

__global__ __launch_bounds__(256) void bswap_kernel(void *out, uint64_t n, int width) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if (width == 64) {
            unsigned long long *p = reinterpret_cast<unsigned long long *>(out) + i;
            *p = __builtin_bswap64(*p);
        } else {
            uint32_t *p = reinterpret_cast<uint32_t *>(out) + i;
            *p = __builtin_bswap32(*p);
        }
    }
}

// Grid of the 256-thread element kernels (bswap_kernel, zero_u64_kernel): they stride past 1024 workgroups.
unsigned elem_grid(uint64_t n) {
    const uint64_t blocks = (n + 255) / 256;
    return blocks > 1024 ? 1024u : (unsigned)blocks;
}

int swap_outputs(void *dev_out, uint64_t count, int width, void *stream) {
    if (!count) return MCHECKSUM_GPU_OK;
    const hipError_t e =
        launch_kernel(bswap_kernel, dim3(elem_grid(count)), dim3(256), (hipStream_t)stream, nullptr, dev_out, count, width);
    if (e != hipSuccess) return hip_err(e, "output byte swap");
    return MCHECKSUM_GPU_OK;
}

int device_ctx(DevCtx **out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_err(e, "hipGetDevice");
    if (dev < 0 || dev >= kMaxDev) return set_err(MCHECKSUM_GPU_ENODEV, "device id %d out of range", dev);
    DevCtx &c = g_dev[dev];
    if (c.init.load(std::memory_order_acquire)) {
        *out = &c;
        return 0;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (!c.init.load(std::memory_order_relaxed)) {
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return hip_err(e, "hipDeviceGetAttribute");
        c.cus = cus > 0 ? cus : 1;
        // tests only: a smaller slot pool (MCHECKSUM_GPU_QUEUE_SLOTS=n), so a
        // test can hold every slot in flight
        const uint32_t qs = mck_settings()->gpu_queue_slots;
        if (qs >= 1 && qs < kQueueSlots) c.nslots = qs;
        // slots aligned to two banks, so a bank's partner is its address ^ kQBankBytes
        const size_t slot_bytes = (size_t)kQSlotWords * sizeof(unsigned long long);
        const size_t qbytes = (size_t)kQueueSlots * slot_bytes + slot_bytes;
        e = hipMalloc(&c.queue_mem, qbytes);
        if (e == hipSuccess) e = hipMemset(c.queue_mem, 0, qbytes);
        if (e == hipSuccess)
            c.queue = reinterpret_cast<unsigned long long *>((reinterpret_cast<uintptr_t>(c.queue_mem) + slot_bytes - 1) /
                                                             slot_bytes * slot_bytes);
        if (e != hipSuccess) {
            if (c.queue_mem) (void)hipFree(c.queue_mem);
            c.queue_mem = nullptr;
            c.queue = nullptr;
            return hip_err(e, "work-queue allocation");
        }
        c.init.store(true, std::memory_order_release);
    }
    *out = &c;
    return 0;
}

// Returns the device table pack for (model, log2g), building it on first use.
int get_pack(DevCtx *c, int idx, int log2g, const void **pack) {
    if (void *p = c->pack[idx][log2g].load(std::memory_order_acquire)) {
        *pack = p;
        return 0;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (void *p = c->pack[idx][log2g].load(std::memory_order_relaxed)) {
        *pack = p;
        return 0;
    }
    const mck_model_t &m = mck_models[idx];
    const crc_rmodel_t rm = gpu_rmodel(idx);
    void *host = nullptr;
    size_t bytes = 0;
    int rc;
    if (m.width == 32) {
        bytes = sizeof(crc32_gpu_pack_t);
        host = calloc(1, bytes);
        rc = host ? crc32_gpu_pack_build(&rm, log2g, (crc32_gpu_pack_t *)host) : -1;
    } else {
        bytes = sizeof(crc64_gpu_pack_t);
        host = calloc(1, bytes);
        rc = host ? crc64_gpu_pack_build(&rm, log2g, (crc64_gpu_pack_t *)host) : -1;
    }
    if (rc != 0) {
        free(host);
        return set_err(MCHECKSUM_GPU_EINVAL, "table build failed for %s (G = %d)", m.name, 1 << log2g);
    }
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess) e = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return hip_err(e, "table upload");
    }
    c->pack[idx][log2g].store(d, std::memory_order_release);
    *pack = d;
    return 0;
}

// Whether slot i is idle: handed to no launch that has not yet been enqueued,
// and its latest launch is done with it -- its `done` event, recorded by that
// launch's completion (launch_kernel's stop event), queried without blocking:
// not a device round trip, so it may run under the pool lock.  A
// never-recorded event reads as complete.  (Late round 5 had the launch's
// last workgroup store a completion word to host-mapped memory instead:
// correct, +-0 without a profiler, not kept.)
bool slot_idle(const DevCtx *c, uint32_t i) {
    const SlotState &s = c->slot[i];
    if (s.pending.load(std::memory_order_acquire)) return false;
    const hipError_t e = hipEventQuery(s.done);
    if (e == hipSuccess) return true;
    if (e != hipErrorNotReady) (void)hipGetLastError();
    return false;
}

// In-flight slots looked at per queue_slot call: a couple while the pool has
// idle slots (so the most recently used lines, warm in L2, are reused first),
// more when it is empty.
constexpr uint32_t kReapSome = 2, kReapMax = 8;

SlotRef queue_slot(DevCtx *c, void *stream) {
    SlotRef r;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) {
        (void)hipGetLastError();
        st = hipStreamCaptureStatusNone;
    }
    std::lock_guard<std::mutex> lk(c->pool_mu);
    // A captured launch replays with these arguments, possibly on two graph
    // execs at once: no slot can be exclusive to it, so it takes the static
    // split (crc_gpu_queue.h, "Exclusivity").
    if (st != hipStreamCaptureStatusNone) {
        c->n_noslot++;
        return r;
    }
    if (c->idle.empty() && c->in_flight.empty())  // first use on this device: every slot idle, slot 0 on top
        for (uint32_t k = c->nslots; k-- > 0;) c->idle.push_back(k);
    // Reap: look at the oldest in-flight slots; those whose launches have
    // completed return to the pool, busy ones go to the back of the FIFO
    // (left at the head, a few long-blocked launches -- a stream
    // waiting on an event -- were looked at by every call while completed
    // slots behind them were never reaped, and every launch fell back to the
    // static split once the idle stack ran out).
    const uint32_t limit = c->idle.empty() ? kReapMax : kReapSome;
    const size_t nlook = c->in_flight.size() < limit ? c->in_flight.size() : limit;
    uint32_t busy = 0;
    for (size_t k = 0; k < nlook; k++) {
        const uint32_t i = c->in_flight.front();
        c->in_flight.pop_front();
        if (slot_idle(c, i)) {
            c->idle.push_back(i);
            c->n_reaped++;
        } else {
            c->in_flight.push_back(i);
            busy++;
        }
    }
    if (c->idle.empty()) {  // the oldest launches are all still running: static split
        c->n_busy_skip += busy;
        c->n_noslot++;
        return r;
    }
    const uint32_t i = c->idle.back();
    SlotState &s = c->slot[i];
    if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        s.done = nullptr;
        c->n_noslot++;
        return r;
    }
    c->idle.pop_back();
    c->in_flight.push_back(i);
    c->n_busy_skip += busy;
    c->n_slot++;
    s.pending.store(true, std::memory_order_relaxed);
    r.q = c->queue + (size_t)i * kQSlotWords + (s.seq & 1u) * kQBankWords;
    s.seq++;
    r.idx = (int)i;
    r.done = s.done;
    r.st = &s;
    return r;
}

// The launch holding r is enqueued and its completion event recorded: the
// slot now reads busy until that launch completes.
void slot_issued(SlotRef &r) {
    if (r.st) r.st->pending.store(false, std::memory_order_release);
}

// The launch call failed, so the kernel was not enqueued (launch_kernel
// reports the call's own status): the bank it was given is still clean, and
// the slot goes straight back to the pool.
void slot_unissue(DevCtx *c, SlotRef &r) {
    if (r.idx < 0) return;
    std::lock_guard<std::mutex> lk(c->pool_mu);
    SlotState &s = c->slot[r.idx];
    s.seq--;
    for (auto it = c->in_flight.end(); it != c->in_flight.begin();) {
        if (*--it == (uint32_t)r.idx) {
            c->in_flight.erase(it);
            break;
        }
    }
    c->idle.push_back((uint32_t)r.idx);
    c->n_slot--;
    c->n_noslot++;
    s.pending.store(false, std::memory_order_release);
    r.idx = -1;
    r.st = nullptr;
}

typedef void (*kern_t)(BatchArgs);

__global__ __launch_bounds__(256) void zero_u64_kernel(unsigned long long *p, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) p[i] = 0;
}

struct KLaunch {
    kern_t k = nullptr;
    int block = 0, blocks_per_cu = 0;
};

// The kernel of one key, if there is one (kernel_key_valid): only those are instantiated.
template <int W, int LOG2G, int MODE, int OP, bool NT, bool LIGHT, bool SPLIT, MsgFrame FRAME, bool LIST, bool BOTH>
KLaunch kernel_ptr() {
    if constexpr (kernel_key_valid(KernelKey{W, LOG2G, MODE, OP, NT, LIGHT, SPLIT, FRAME, LIST, BOTH})) {
        using S = Shape<W, MODE, LIGHT, LOG2G>;
        if constexpr (W == 32)
            return {crc32c_batch_kernel<LOG2G, MODE, OP, NT, LIGHT, FRAME, LIST, BOTH>, S::block, S::blocks_per_cu};
        else return {crc64_batch_kernel<LOG2G, MODE, OP, NT, SPLIT>, S::block, S::blocks_per_cu};
    }
    return {};
}

// f(std::integral_constant<int, x>) for a run-time x in [0, N); no kernel outside.
template <int N, class F>
KLaunch lift(int x, const F &f) {
    if constexpr (N > 0) return x == N - 1 ? f(std::integral_constant<int, N - 1>{}) : lift<N - 1>(x, f);
    return {};
}

// The kernel of a key (launch_plan.h: kernel_key): each field becomes a
// template argument in turn.  A key with no kernel gives a null KLaunch, which
// the callers report as an error and never launch.
KLaunch kernel_for(const KernelKey &k) {
    if (!kernel_key_valid(k)) return {};
    return lift<2>(k.width == 32 ? 0 : k.width == 64 ? 1 : -1, [&](auto w64) {
        return lift<CRC_GPU_MAX_LOG2G + 1>(k.lg, [&](auto lg) {
            return lift<kOffsets + 1>(k.mode, [&](auto mode) {
                return lift<kOpUnpack + 1>(k.op, [&](auto op) {
                    return lift<2>(k.nt, [&](auto nt) {
                        return lift<2>(k.light, [&](auto light) {
                            return lift<2>(k.split, [&](auto split) {
                                return lift<kFrameRpc + 1>(k.frame, [&](auto frame) {
                                    return lift<2>(k.list, [&](auto list) {
                                        return lift<2>(k.both_lists, [&](auto both) {
                                            return kernel_ptr<w64() ? 64 : 32, lg(), mode(), op(), nt() != 0, light() != 0,
                                                              split() != 0, (MsgFrame)frame(), list() != 0, both() != 0>();
                                        });
                                    });
                                });
                            });
                        });
                    });
                });
            });
        });
    });
}

// The header pack of a 16-bit model and kind on the device (launch_plan.h,
// RpcHdrPack), built and uploaded once (under g_mu), then read without a lock.
int get_rpc_pack(DevCtx *c, int idx, int kind, const void **out) {
    if (void *p = c->rpc[idx][kind].load(std::memory_order_acquire)) {
        *out = p;
        return 0;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (void *p = c->rpc[idx][kind].load(std::memory_order_relaxed)) {
        *out = p;
        return 0;
    }
    const mck_model_t &m = mck_models[idx];
    RpcHdrPack *host = (RpcHdrPack *)calloc(1, sizeof(RpcHdrPack));
    if (!host) return set_err(MCHECKSUM_GPU_EINVAL, "table build failed for %s", m.name);
    rpc_hdr_pack_build((uint32_t)m.poly, m.reflected != 0, (uint32_t)m.init, (uint32_t)m.xorout, (uint32_t)kind, host);
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(RpcHdrPack));
    if (e == hipSuccess) e = hipMemcpy(d, host, sizeof(RpcHdrPack), hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return hip_err(e, "table upload");
    }
    c->rpc[idx][kind].store(d, std::memory_order_release);
    *out = d;
    return 0;
}
static_assert(kRpcRequest == MCHECKSUM_GPU_CORE_HEADER_REQUEST && kRpcResponse == MCHECKSUM_GPU_CORE_HEADER_RESPONSE &&
                  kRpcOk == MCHECKSUM_GPU_RPC_OK && kRpcPayload == MCHECKSUM_GPU_RPC_PAYLOAD &&
                  kRpcHeader == MCHECKSUM_GPU_RPC_HEADER && kRpcShort == MCHECKSUM_GPU_RPC_SHORT &&
                  kRpcDeferred == MCHECKSUM_GPU_RPC_DEFERRED && kRpcFault == MCHECKSUM_GPU_RPC_FAULT &&
                  kRpcClasses == MCHECKSUM_GPU_RPC_CLASSES && kRpcMisfit == MCHECKSUM_GPU_COPY_RPC_MISFIT &&
                  kRpcCopyClasses == MCHECKSUM_GPU_COPY_RPC_CLASSES,
              "launch_plan.h and mchecksum_gpu.h name the kinds and classes alike");

// The front of every offsets-shaped entry point (offsets_call.h: the call, what
// it must supply, its BatchArgs): argument checks, model, device context, plan,
// table packs, slot and launch.  The calls on HG and RPC messages but
// verify_messages check the method ahead of the device, as an argument (as
// verify_core_headers does); the others the device first.
int offsets_call(const OffsetsCall &c) {
    const bool method_first = offsets_needs(c.op, c.frame).method_first;
    const bool rpc = c.frame == kFrameRpc, detached = c.frame == kFrameDetached, in_place = c.frame == kFrameInPlace;
    if (offsets_lacks_pointer(c)) return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if (rpc && c.kind != MCHECKSUM_GPU_CORE_HEADER_REQUEST && c.kind != MCHECKSUM_GPU_CORE_HEADER_RESPONSE)
        return set_err(MCHECKSUM_GPU_EINVAL, "unknown core header kind %d", c.kind);
    if (rpc && (c.hash_off < kRpcHdrBytes || c.hash_off > kMaxHashOff || c.hash_off + 4 > c.pay_off))
        return set_err(MCHECKSUM_GPU_EINVAL, "hash_offset must lie behind the core header, at most 2^30, and hash_offset + 4 "
                                             "must not exceed payload_offset");
    if (in_place && (c.hash_off + 4 > c.pay_off || c.pay_off > (1u << 30)))
        return set_err(MCHECKSUM_GPU_EINVAL, "hash_offset + 4 must not exceed payload_offset");
    if (detached && c.hash_off > kMaxHashOff) return set_err(MCHECKSUM_GPU_EINVAL, "hash_offset must not exceed 2^30");
    if ((uint64_t)c.count > kMaxUnits) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 payloads in one call");
    Model m;
    int rc;
    if (method_first) {
        if ((rc = resolve_model(c.method, &m))) return rc;
        if (m.width != 32) return set_err(MCHECKSUM_GPU_EMETHOD, "the HG header carries a 32-bit payload hash: crc32c only");
        // the detached epilogue stores and compares x ^ xorout unswapped: reflected models (both 32-bit ones are)
        if (detached && m.msb) return set_err(MCHECKSUM_GPU_EMETHOD, "MSB-first methods have no detached message kernel");
        if (rpc && m.msb) return set_err(MCHECKSUM_GPU_EMETHOD, "MSB-first methods have no RPC message kernel");
    }
    int hdr_idx = -1;
    if (rpc) {
        hdr_idx = mck_model_index(c.hdr_method);
        if (hdr_idx < 0)
            return set_err(MCHECKSUM_GPU_EMETHOD, "unknown hash method \"%s\"", c.hdr_method ? c.hdr_method : "(null)");
        if (mck_models[hdr_idx].width != 16)
            return set_err(MCHECKSUM_GPU_EMETHOD, "core headers carry a 16-bit hash: \"%s\" is not a crc16 model", c.hdr_method);
    }
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    if (!method_first && (rc = resolve_model(c.method, &m))) return rc;
    DevCtx *dc = nullptr;
    const void *pack = nullptr, *shift = nullptr, *hdr_pack = nullptr;
    if ((rc = device_ctx(&dc))) return rc;
    const LaunchPlan p = plan_offsets(*mck_settings(), dc->cus, m.width, c.count);
    // (an empty batch too resolves its method and builds its tables)
    if ((rc = get_pack(dc, m.idx, p.lg, &pack))) return rc;
    if (c.op == kOpUpdate && (rc = get_ext(dc, m.idx, &shift))) return rc;
    if (rpc && (rc = get_rpc_pack(dc, hdr_idx, c.kind, &hdr_pack))) return rc;
    if (c.count == 0) return MCHECKSUM_GPU_OK;
    if (in_place && m.width != 32)
        return set_err(MCHECKSUM_GPU_EMETHOD, "message verify carries a 32-bit header hash: crc32c only");
    const KLaunch k = kernel_for(kernel_key(p, c.op, c.frame, c.list, c.both_lists));
    if (!k.k) return set_err(MCHECKSUM_GPU_EINVAL, "no batch kernel for this call");
    BatchArgs a = batch_args_of(c, pack, shift, hdr_pack, m.msb, error_word());
    SlotRef sr;
    if (p.dyn) sr = queue_slot(dc, c.stream);
    a.queue = sr.q;
    static const char *const what[] = {"kernel launch",      "kernel launch",      "kernel launch",
                                       "seal kernel launch", "pack kernel launch", "unpack kernel launch"};
    rc = launch_slot(dc, sr, k.k, p.grid, k.block, c.stream, a, what[c.op]);
    // (running registers stay in the kernels' form: state_get swaps an MSB-first model's)
    if (rc == MCHECKSUM_GPU_OK && m.msb && c.op == kOpChecksum) rc = swap_outputs(c.out, c.count, m.width, c.stream);
    return rc;
}

// ---- copy-and-checksum: the copy kernels (crc_gpu_copy.h) ----
typedef void (*copy_kern_t)(CopyArgs);
struct CopyLaunch {
    copy_kern_t k = nullptr;
    int block = 0;
};

// The kernel of one key, if there is one (copy_key_valid): only those are instantiated.
template <int W, int OP, bool NT, bool LIGHT>
CopyLaunch copy_kernel_ptr() {
    if constexpr (copy_key_valid(CopyKey{W, OP, NT, LIGHT})) {
        if constexpr (W == 32) return {crc32c_copy_kernel<OP, NT, LIGHT>, Shape<32, kOffsets, LIGHT>::block};
        else return {crc64_copy_kernel<OP, NT>, Shape<64, kOffsets>::block};
    }
    return {};
}

// Key I of the 16 (width, op, nt, light) combinations, searched in turn: a
// key with no kernel gives a null CopyLaunch, which copy_call reports as an
// error and never launches.
template <int I = 0>
CopyLaunch copy_kernel_at(int i) {
    if constexpr (I < 16)
        return i == I ? copy_kernel_ptr<(I & 8) ? 64 : 32, (I >> 2) & 1, ((I >> 1) & 1) != 0, (I & 1) != 0>()
                      : copy_kernel_at<I + 1>(i);
    return {};
}
CopyLaunch copy_kernel_for(const CopyKey &k) {
    if ((k.width != 32 && k.width != 64) || k.op < kCopyChecksum || k.op > kCopyUpdate) return {};
    return copy_kernel_at((k.width == 64 ? 8 : 0) | k.op << 2 | (k.nt ? 2 : 0) | (k.light ? 1 : 0));
}

// One copy call, as its entry point names it: chunk i = src[src_off[i],
// src_off[i+1]) goes to dst + dst_starts[i]; out holds the CRCs
// (kCopyChecksum) or the running registers (kCopyUpdate).
struct CopyCall {
    CopyOp op;
    const char *method;
    const void *src;
    const uint64_t *src_off;
    void *dst;
    const uint64_t *dst_starts;
    size_t count;
    void *out;
    void *stream;
};

// The front of both copy entry points, beside offsets_call: its checks in
// checksum_offsets' / update_offsets' order, and the same plan, table pack,
// slot and launch for the same count.
int copy_call(const CopyCall &c) {
    // an empty batch needs no buffers
    if (c.count && (!c.src || !c.src_off || !c.dst || !c.dst_starts || !c.out))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if ((uint64_t)c.count > kMaxUnits) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 payloads in one call");
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    Model m;
    int rc;
    if ((rc = resolve_model(c.method, &m))) return rc;
    DevCtx *dc = nullptr;
    const void *pack = nullptr, *shift = nullptr;
    if ((rc = device_ctx(&dc))) return rc;
    const LaunchPlan p = plan_offsets(*mck_settings(), dc->cus, m.width, c.count);
    if ((rc = get_pack(dc, m.idx, p.lg, &pack))) return rc;
    if (c.op == kCopyUpdate && (rc = get_ext(dc, m.idx, &shift))) return rc;
    if (c.count == 0) return MCHECKSUM_GPU_OK;
    const CopyLaunch k = copy_kernel_for(copy_key(p, c.op));
    if (!k.k) return set_err(MCHECKSUM_GPU_EINVAL, "no copy kernel for this call");
    CopyArgs a{};
    a.b.base = (const uint8_t *)c.src;
    a.b.offsets = c.src_off;
    a.b.count = c.count;
    a.b.out = c.out;
    a.b.pack = pack;
    a.b.err_word = error_word();
    a.b.shift = shift;
    a.dst = (uint8_t *)c.dst;
    a.dst_starts = c.dst_starts;
    SlotRef sr;
    if (p.dyn) sr = queue_slot(dc, c.stream);
    a.b.queue = sr.q;
    rc = launch_slot(dc, sr, k.k, p.grid, k.block, c.stream, a, "copy kernel launch");
    // (running registers stay in the kernels' form: state_get swaps an MSB-first model's)
    if (rc == MCHECKSUM_GPU_OK && m.msb && c.op == kCopyChecksum) rc = swap_outputs(c.out, c.count, m.width, c.stream);
    return rc;
}

// ---- streaming state: 256-thread element kernels (grid: elem_grid) ----
template <typename T>
__global__ __launch_bounds__(256) void state_init_kernel(T *st, uint64_t n, T init) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) st[i] = init;
}

// out may alias st: every element is read, then written, by one thread
template <typename T>
__global__ __launch_bounds__(256) void state_get_kernel(const T *st, T *out, uint64_t n, T xorout, int msb) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if constexpr (sizeof(T) == 8) out[i] = mck_reg_to_crc64(st[i], xorout, msb);
        else out[i] = mck_reg_to_crc32(st[i], xorout, msb);
    }
}

// state_get and the compare in one launch (seg_plan.h: seg_verify_decide, the
// verdict verify_segments writes; no fault state to read here).  The states
// are only read.
template <typename T>
__global__ __launch_bounds__(256) void state_verify_kernel(const T *st, const T *expected, uint64_t n, T xorout, int msb,
                                                           uint8_t *status, uint32_t *mism) {
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        uint64_t v;
        if constexpr (sizeof(T) == 8) v = mck_reg_to_crc64(st[i], xorout, msb);
        else v = mck_reg_to_crc32(st[i], xorout, msb);
        nbad += mck::seg_verify_decide(false, v, expected[i], status, i);
    }
    add_mismatches(mism, nbad);  // once per workgroup (crc_gpu_common.h)
}

// state_verify with the expected values read from the eager messages' hash
// slots, and its mirror on the sender (SEAL): the end of a streamed pull or
// push of overflow payloads.  The slot rule is the detached kernels'
// (launch_plan.h: msg_slot_ok, msg_slot_at); 32-bit models only, all of them
// reflected, so the value is the register ^ xorout.  The states are only read.
// (state_message_list_kernel below: the same element with the slot by address and length.)
template <bool SEAL>
__global__ __launch_bounds__(256) void state_messages_kernel(const uint32_t *st, uint64_t n, uint32_t xorout, uint8_t *msgs,
                                                             const uint64_t *msg_off, uint32_t hash_off, uint8_t *status,
                                                             uint32_t *mism) {
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t m0 = msg_off[i], m1 = msg_off[i + 1];
        const bool short_msg = !mck::msg_slot_ok(m0, m1, hash_off);
        uint8_t *slot = msgs + mck::msg_slot_at(m0, hash_off);
        const uint32_t v = mck_reg_to_crc32(st[i], xorout, 0);
        if constexpr (SEAL) {
            if (!short_msg) store_be32(slot, v);
            if (status) status[i] = short_msg ? 1 : 0;
        } else {
            nbad += mck::seg_verify_decide(short_msg, v, short_msg ? 0 : load_be32(slot), status, i);
        }
    }
    if constexpr (!SEAL) add_mismatches(mism, nbad);  // once per workgroup (crc_gpu_common.h)
}

// state_messages_kernel with the eager messages by address list: message i is the msg_len[i] bytes at msg_addr[i],
// anywhere, and an end that wraps the address space an empty message (launch_plan.h: list_msg_len).  A message
// without its slot is never dereferenced.
template <bool SEAL>
__global__ __launch_bounds__(256) void state_message_list_kernel(const uint32_t *st, uint64_t n, uint32_t xorout,
                                                                 const uint64_t *msg_addr, const uint64_t *msg_len,
                                                                 uint32_t hash_off, uint8_t *status, uint32_t *mism) {
    uint32_t nbad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t m0 = msg_addr[i], m1 = m0 + mck::list_msg_len(m0, msg_len[i]);
        const bool short_msg = !mck::msg_slot_ok(m0, m1, hash_off);
        uint8_t *slot = reinterpret_cast<uint8_t *>(mck::msg_slot_at(m0, hash_off));
        const uint32_t v = mck_reg_to_crc32(st[i], xorout, 0);
        if constexpr (SEAL) {
            if (!short_msg) store_be32(slot, v);
            if (status) status[i] = short_msg ? 1 : 0;
        } else {
            nbad += mck::seg_verify_decide(short_msg, v, short_msg ? 0 : load_be32(slot), status, i);
        }
    }
    if constexpr (!SEAL) add_mismatches(mism, nbad);  // once per workgroup (crc_gpu_common.h)
}

// out may alias a or b, element for element
template <typename T>
__global__ __launch_bounds__(256) void combine_kernel(const T *a, const T *b, const uint64_t *len_b, T *out, uint64_t n,
                                                      const void *shift, T init, T xorout, int msb) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if constexpr (sizeof(T) == 8)
            out[i] = mck_combine64(reinterpret_cast<const crc64_shift_pack_t *>(shift), a[i], b[i], len_b[i], init, xorout, msb);
        else
            out[i] = mck_combine32(reinterpret_cast<const crc32_shift_pack_t *>(shift), a[i], b[i], len_b[i], init, xorout, msb);
    }
}

// ---- combine_runs: the CRCs of a run's chunks joined in order ----
// The join is crc_gpu_seed.h's monoid over (r, n); what is decided here is the
// bracketing.  W lanes share one run of K chunks: lane l folds the l-th of W
// contiguous slices of ceil(K / W) chunks left to right -- every lane a chain
// of its own, so the 64 chains of a wave advance together --, then the lanes'
// elements meet in an ordered tree, log2(W) joins deep: a shuffle down by 1,
// 2, 4, ..., the lower lane the left operand.  A run of K chunks has K / W +
// log2(W) joins on its critical path, and a run of up to W chunks the tree
// alone.
// A workgroup is four waves and takes four consecutive runs, a wave each
// (W = 64).  A run of more than kJoinBlockRun chunks is taken by the whole
// workgroup instead (W = 256: the four wave results meet in LDS).  Which runs
// are long is read once per workgroup, into LDS, so every wave takes the same
// branches around the barriers whatever happens to the table meanwhile.
constexpr uint32_t kJoinWaves = 4;           // waves, and runs, per workgroup
constexpr uint64_t kJoinBlockRun = 4096;     // longer runs: the workgroup, not one wave
constexpr uint32_t kJoinMaxGrid = 65536;     // workgroups stride past this many

template <typename T>
struct JoinOps;
template <>
struct JoinOps<uint32_t> {
    using E = mck_join32_t;
    using SP = crc32_shift_pack_t;
    static __device__ __forceinline__ E in(uint32_t v, uint64_t n, uint32_t init, uint32_t xorout, int msb) {
        return mck_join_in32(v, n, init, xorout, msb);
    }
    static __device__ __forceinline__ E join(const SP *sp, E a, E b, uint32_t init) { return mck_join32(sp, a, b, init); }
    static __device__ __forceinline__ uint32_t out(E e, uint32_t xorout, int msb) { return mck_join_out32(e, xorout, msb); }
    // lane l reads lane (l + d) % 64's word: one ds_bpermute_b32, what __shfl lowers to.  (The builtin, not
    // __shfl_down: a second user with a run-time distance made hipcc invert a compare and its select in the
    // CRC-64 batch kernels' lane combine -- equivalent code, but not the shipped instruction stream.)
    static __device__ __forceinline__ uint32_t shfl_down(uint32_t r, int d) {
        return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((threadIdx.x + d) & 63u) << 2), (int)r);
    }
};
template <>
struct JoinOps<uint64_t> {
    using E = mck_join64_t;
    using SP = crc64_shift_pack_t;
    static __device__ __forceinline__ E in(uint64_t v, uint64_t n, uint64_t init, uint64_t xorout, int msb) {
        return mck_join_in64(v, n, init, xorout, msb);
    }
    static __device__ __forceinline__ E join(const SP *sp, E a, E b, uint64_t init) { return mck_join64(sp, a, b, init); }
    static __device__ __forceinline__ uint64_t out(E e, uint64_t xorout, int msb) { return mck_join_out64(e, xorout, msb); }
    static __device__ __forceinline__ uint64_t shfl_down(uint64_t r, int d) {  // the 32-bit halves
        const uint32_t lo = JoinOps<uint32_t>::shfl_down((uint32_t)r, d),
                       hi = JoinOps<uint32_t>::shfl_down((uint32_t)(r >> 32), d);
        return (uint64_t)hi << 32 | lo;
    }
};

template <typename T>
struct JoinArgs {
    const T *crc;           // chunk k's finalized CRC
    const uint64_t *len;    // and byte count
    const void *shift;      // the model's Z^n pack
    T init, xorout;
    int msb;
};

// Lane `lane` of `width` folds its slice of chunks [lo, hi), left to right.
// The next chunk's words are loaded before the join that waits for this one's tables.
template <typename T>
__device__ __forceinline__ typename JoinOps<T>::E join_slice(const JoinArgs<T> &a, uint64_t lo, uint64_t hi, uint32_t lane,
                                                             uint32_t width) {
    using J = JoinOps<T>;
    const typename J::SP *sp = reinterpret_cast<const typename J::SP *>(a.shift);
    const uint64_t k = hi - lo, m = (k + width - 1) / width;
    const uint64_t s0 = (uint64_t)lane * m, s1 = s0 + m;  // (k <= 2^31, lane < 256)
    const uint64_t b = lo + (s0 < k ? s0 : k), e = lo + (s1 < k ? s1 : k);
    if (b >= e) return J::in(0, 0, a.init, a.xorout, a.msb);  // the identity
    typename J::E acc = J::in(a.crc[b], a.len[b], a.init, a.xorout, a.msb);
    if (b + 1 >= e) return acc;
    T v = a.crc[b + 1];
    uint64_t n = a.len[b + 1];
    for (uint64_t i = b + 1; i < e; i++) {
        const typename J::E x = J::in(v, n, a.init, a.xorout, a.msb);
        if (i + 1 < e) {
            v = a.crc[i + 1];
            n = a.len[i + 1];
        }
        acc = J::join(sp, acc, x, a.init);
    }
    return acc;
}

// The wave's 64 elements joined in lane order; the result is lane 0's.  Step
// d joins lane l (a multiple of 2d, holding lanes [l, l + d)) with lane l + d
// (holding [l + d, l + 2d)); the other lanes' elements are no longer needed.
template <typename T>
__device__ __forceinline__ typename JoinOps<T>::E join_wave(const JoinArgs<T> &a, typename JoinOps<T>::E e, uint32_t lane) {
    using J = JoinOps<T>;
    const typename J::SP *sp = reinterpret_cast<const typename J::SP *>(a.shift);
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) {
        typename J::E o;
        o.r = J::shfl_down(e.r, d);
        o.n = JoinOps<uint64_t>::shfl_down(e.n, d);
        if ((lane & (2 * d - 1)) == 0) e = J::join(sp, e, o, a.init);
    }
    return e;
}

// out and out_len must not overlap the tables: runs are joined in parallel
template <typename T>
__global__ __launch_bounds__(256) void combine_runs_kernel(JoinArgs<T> a, uint64_t nchunks, const uint64_t *first,
                                                           uint64_t nruns, T *out, uint64_t *out_len) {
    using J = JoinOps<T>;
    __shared__ uint64_t s_first[kJoinWaves + 1];
    __shared__ T s_r[kJoinWaves];
    __shared__ uint64_t s_n[kJoinWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t ngroups = (nruns + kJoinWaves - 1) / kJoinWaves;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t j0 = g * kJoinWaves;
        const uint32_t nr = nruns - j0 < kJoinWaves ? (uint32_t)(nruns - j0) : kJoinWaves;
        // the group's run bounds, clamped to the chunk tables: no read past them
        if (threadIdx.x <= nr) {
            const uint64_t f = first[j0 + threadIdx.x];
            s_first[threadIdx.x] = f < nchunks ? f : nchunks;
        }
        __syncthreads();
        uint64_t my_lo = 0, my_hi = 0;
        bool mine = false;
        for (uint32_t w = 0; w < nr; w++) {  // (block-uniform: nr and s_first)
            const uint64_t lo = s_first[w], hi = s_first[w + 1] > lo ? s_first[w + 1] : lo;
            if (hi - lo <= kJoinBlockRun) {
                if (w == wave) {
                    my_lo = lo;
                    my_hi = hi;
                    mine = true;
                }
                continue;
            }
            typename J::E e = join_wave<T>(a, join_slice<T>(a, lo, hi, threadIdx.x, 256), lane);
            if (lane == 0) {
                s_r[wave] = e.r;
                s_n[wave] = e.n;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (uint32_t v = 1; v < kJoinWaves; v++) {
                    typename J::E o;
                    o.r = s_r[v];
                    o.n = s_n[v];
                    e = J::join(reinterpret_cast<const typename J::SP *>(a.shift), e, o, a.init);
                }
                out[j0 + w] = J::out(e, a.xorout, a.msb);
                if (out_len) out_len[j0 + w] = e.n;
            }
            __syncthreads();  // s_r, s_n are free again
        }
        if (mine) {
            const typename J::E e = join_wave<T>(a, join_slice<T>(a, my_lo, my_hi, lane, 64), lane);
            if (lane == 0) {
                out[j0 + wave] = J::out(e, a.xorout, a.msb);
                if (out_len) out_len[j0 + wave] = e.n;
            }
        }
        __syncthreads();  // s_first is free again
    }
}

template <typename T>
hipError_t launch_combine_runs(const crc_rmodel_t &rm, const void *shift, const void *dev_crc, const uint64_t *dev_len,
                               size_t nchunks, const uint64_t *dev_run_first, size_t nruns, void *dev_out,
                               uint64_t *dev_out_len, void *stream) {
    const JoinArgs<T> a{(const T *)dev_crc, dev_len, shift, (T)rm.rinit, (T)rm.xorout, rm.msb};
    const uint64_t groups = ((uint64_t)nruns + kJoinWaves - 1) / kJoinWaves;
    return launch_kernel(combine_runs_kernel<T>, dim3(groups > kJoinMaxGrid ? kJoinMaxGrid : (unsigned)groups), dim3(256),
                         (hipStream_t)stream, nullptr, a, (uint64_t)nchunks, dev_run_first, (uint64_t)nruns, (T *)dev_out,
                         dev_out_len);
}

// Common front of the element calls: the count cap, the device, the model
// (its kernels' form in *rm) and the device context.
int state_call(const char *method, size_t count, Model *m, crc_rmodel_t *rm, DevCtx **c) {
    if ((uint64_t)count > kMaxUnits) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 payloads in one call");
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    int rc = resolve_model(method, m);
    if (!rc) rc = device_ctx(c);
    if (!rc) *rm = gpu_rmodel(m->idx);
    return rc;
}

// state_verify_messages and state_seal_messages: arguments, then the method
// (a 32-bit model, ahead of the device, as the calls on HG messages check
// it), then the device.  An element kernel: no work-queue slot, no workspace,
// no device-side wait.
// dev_msg_len: the list form -- dev_msg_offsets holds `count` addresses with no buffer under them, dev_msg_len
// their lengths.
int state_messages_call(bool seal, const char *method, const void *dev_state, size_t count, void *dev_msgs,
                        const uint64_t *dev_msg_offsets, size_t hash_off, uint8_t *status, uint32_t *mism, void *stream,
                        bool list = false, const uint64_t *dev_msg_len = nullptr) {
    if (count && (!dev_state || !dev_msg_offsets || (list ? !dev_msg_len : !dev_msgs)))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if (hash_off > kMaxHashOff) return set_err(MCHECKSUM_GPU_EINVAL, "hash_offset must not exceed 2^30");
    if ((uint64_t)count > kMaxUnits) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 payloads in one call");
    Model m;
    if (int rc = resolve_model(method, &m)) return rc;
    if (m.width != 32) return set_err(MCHECKSUM_GPU_EMETHOD, "the HG header carries a 32-bit payload hash: crc32c only");
    // state_messages_kernel takes the value as register ^ xorout, unswapped: reflected models (both 32-bit ones are)
    if (m.msb) return set_err(MCHECKSUM_GPU_EMETHOD, "MSB-first methods have no state message kernel");
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    DevCtx *c = nullptr;
    if (int rc = device_ctx(&c)) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    const crc_rmodel_t rm = gpu_rmodel(m.idx);
    const dim3 grid(elem_grid(count)), block(256);
    const hipError_t e =
        list ? launch_kernel(seal ? state_message_list_kernel<true> : state_message_list_kernel<false>, grid, block,
                             (hipStream_t)stream, nullptr, (const uint32_t *)dev_state, (uint64_t)count, (uint32_t)rm.xorout,
                             dev_msg_offsets, dev_msg_len, (uint32_t)hash_off, status, mism)
             : launch_kernel(seal ? state_messages_kernel<true> : state_messages_kernel<false>, grid, block,
                             (hipStream_t)stream, nullptr, (const uint32_t *)dev_state, (uint64_t)count, (uint32_t)rm.xorout,
                             (uint8_t *)dev_msgs, dev_msg_offsets, (uint32_t)hash_off, status, mism);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, seal ? "state seal" : "state verify");
}

int launch_fixed(DevCtx *c, const Model &m, const LaunchPlan &p, const void *pack, const void *dev_base, size_t stride,
                 size_t len, size_t count, void *dev_out, void *stream) {
    BatchArgs a{};
    a.base = (const uint8_t *)dev_base;
    a.stride = stride;
    a.len = len;
    a.count = count;
    a.out = dev_out;
    a.pack = pack;
    a.err_word = error_word();
    if (p.split) {
        const void *shift = nullptr;
        if (int rc = get_ext(c, m.idx, &shift)) return rc;
        a.shift = shift;
        a.split_log2 = p.split_log2;
    }
    const KLaunch k = kernel_for(kernel_key(p, kOpChecksum));
    if (!k.k) return set_err(MCHECKSUM_GPU_EINVAL, "no batch kernel for this call");
    SlotRef sr;
    if (p.dyn) sr = queue_slot(c, stream);
    a.queue = sr.q;
    // Split pieces that cannot combine in their workgroup (no slot, or chunks
    // of part payloads: launch_plan.h) XOR their terms into out[]: zero it
    // first, in stream order, with a kernel -- a hipMemsetAsync captured into
    // a graph did not order against the kernel node on replays after the
    // first (the pieces landed in a half-zeroed output:
    // tests/test_gpu_queue.py, concurrent replays).
    a.split_lds = sr.q && p.split_lds_ok ? 1u : 0u;
    if (p.split && (p.zero_out || !sr.q)) {
        const hipError_t e = launch_kernel(zero_u64_kernel, dim3(elem_grid(count)), dim3(256), (hipStream_t)stream, nullptr,
                                           reinterpret_cast<unsigned long long *>(dev_out), (uint64_t)count);
        if (e != hipSuccess) {
            slot_unissue(c, sr);
            return hip_err(e, "output zeroing");
        }
    }
    int rc = launch_slot(c, sr, k.k, p.grid, k.block, stream, a, "kernel launch");
    if (rc == MCHECKSUM_GPU_OK && m.msb) rc = swap_outputs(dev_out, count, m.width, stream);
    return rc;
}

}  // namespace mck

using namespace mck;

extern "C" {

int mchecksum_gpu_available(void) {
    // The device count cannot change for the life of the process: ask HIP
    // once (every batch call checks this first; ~1 us saved per call).
    static std::atomic<int> cached{-1};
    int v = cached.load(std::memory_order_relaxed);
    if (v >= 0) return v;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    v = n > 0 ? 1 : 0;
    cached.store(v, std::memory_order_relaxed);
    return v;
}

int mchecksum_gpu_prepare(const char *hash_method) {
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    const int idx = mck_model_index(hash_method);
    if (idx < 0) return set_err(MCHECKSUM_GPU_EMETHOD, "unknown hash method \"%s\"", hash_method ? hash_method : "(null)");
    DevCtx *c = nullptr;
    int rc = device_ctx(&c);
    // payload kernels (32/64-bit models): a table pack per lanes-per-payload width
    for (int lg = 0; mck_models[idx].width != 16 && !rc && lg <= CRC_GPU_MAX_LOG2G; lg++) {
        const void *pack = nullptr;
        rc = get_pack(c, idx, lg, &pack);
    }
    if (rc) return rc;
    // ... and the extension tables every entry point may need (Z^n shift pack:
    // split CRC-64 pieces, segments, XDR; CRC-16 byte table: core headers),
    // so that no call captured into a graph uploads anything
    const void *ext = nullptr;
    if ((rc = get_ext(c, idx, &ext))) return rc;
    // ... and a 16-bit model's header packs of both kinds (the RPC message calls)
    for (int kind = 0; mck_models[idx].width == 16 && !rc && kind < 2; kind++) rc = get_rpc_pack(c, idx, kind, &ext);
    return rc;
}

int mchecksum_gpu_lanes_per_payload(const char *hash_method, size_t len) {
    Model m;
    if (gpu_model(hash_method, &m) < 0) return -1;
    return 1 << choose_log2g(*mck_settings(), len, m.width);
}

int mchecksum_gpu_checksum_fixed(const char *hash_method, const void *dev_base, size_t stride, size_t len,
                                 size_t count, void *dev_out, void *stream) {
    if (count && (!dev_base || !dev_out)) return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if (count > 1 && stride < len) return set_err(MCHECKSUM_GPU_EINVAL, "stride smaller than len");
    if ((uint64_t)count > kMaxUnits) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 payloads in one call");
    // the batch must fit the address space: stride * (count - 1) + len
    if (count > 1 && (uint64_t)stride > (UINT64_MAX - (uint64_t)len) / (count - 1))
        return set_err(MCHECKSUM_GPU_EINVAL, "stride * (count - 1) + len overflows");
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    Model m;
    DevCtx *c = nullptr;
    const void *pack = nullptr;
    int rc = resolve_model(hash_method, &m);
    if (!rc) rc = device_ctx(&c);
    if (rc) return rc;
    const LaunchPlan p = plan_fixed(*mck_settings(), c->cus, m.width, (uintptr_t)dev_base, stride, len, count);
    if ((rc = get_pack(c, m.idx, p.lg, &pack))) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    return launch_fixed(c, m, p, pack, dev_base, stride, len, count, dev_out, stream);
}

int mchecksum_gpu_checksum_offsets(const char *hash_method, const void *dev_base, const uint64_t *dev_offsets,
                                   size_t count, void *dev_out, void *stream) {
    OffsetsCall c{kOpChecksum, hash_method, dev_base, dev_offsets, count};
    c.out = dev_out;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_verify_offsets(const char *hash_method, const void *dev_base, const uint64_t *dev_offsets,
                                 size_t count, const void *dev_expected, uint8_t *dev_status,
                                 uint32_t *dev_mismatches, void *stream) {
    OffsetsCall c{kOpVerify, hash_method, dev_base, dev_offsets, count};
    c.expected = dev_expected;
    c.status = dev_status;
    c.mismatches = dev_mismatches;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_verify_messages(const char *hash_method, const void *dev_buf, const uint64_t *dev_msg_offsets,
                                  size_t count, size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
                                  uint32_t *dev_mismatches, void *stream) {
    OffsetsCall c{kOpVerify, hash_method, dev_buf, dev_msg_offsets, count};
    c.frame = kFrameInPlace;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_mismatches;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_seal_messages(const char *hash_method, void *dev_buf, const uint64_t *dev_msg_offsets, size_t count,
                                size_t payload_offset, size_t hash_offset, uint8_t *dev_status, void *stream) {
    OffsetsCall c{kOpSeal, hash_method, dev_buf, dev_msg_offsets, count};  // in place: the payloads are dev_buf's own
    c.out = dev_buf;
    c.frame = kFrameInPlace;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_pack_messages(const char *hash_method, const void *dev_src, const uint64_t *dev_src_offsets,
                                void *dev_buf, const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                size_t hash_offset, uint8_t *dev_status, void *stream) {
    // payload i = src[src_off[i], src_off[i+1]) goes behind the headers of message i of dev_buf
    OffsetsCall c{kOpPack, hash_method, dev_src, dev_src_offsets, count};
    c.dst = dev_buf;
    c.dst_off = dev_msg_offsets;
    c.frame = kFrameInPlace;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_unpack_messages(const char *hash_method, const void *dev_buf, const uint64_t *dev_msg_offsets,
                                  size_t count, size_t payload_offset, size_t hash_offset, void *dev_dst,
                                  const uint64_t *dev_dst_offsets, uint8_t *dev_status, uint32_t *dev_mismatches,
                                  void *stream) {
    // pack's mirror: the messages are the source, and the launch counts mismatches
    OffsetsCall c{kOpUnpack, hash_method, dev_buf, dev_msg_offsets, count};
    c.dst = dev_dst;
    c.dst_off = dev_dst_offsets;
    c.frame = kFrameInPlace;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_mismatches;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_verify_detached_messages(const char *hash_method, const void *dev_msgs, const uint64_t *dev_msg_offsets,
                                           size_t hash_offset, const void *dev_payloads,
                                           const uint64_t *dev_payload_offsets, size_t count, uint8_t *dev_status,
                                           uint32_t *dev_mismatches, void *stream) {
    // an overflow RPC: the payloads are the batch, the eager messages only carry the hashes (and are only read)
    OffsetsCall c{kOpVerify, hash_method, dev_payloads, dev_payload_offsets, count};
    c.frame = kFrameDetached;
    c.hdr = const_cast<void *>(dev_msgs);
    c.hdr_off = dev_msg_offsets;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_mismatches;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_seal_detached_messages(const char *hash_method, void *dev_msgs, const uint64_t *dev_msg_offsets,
                                         size_t hash_offset, const void *dev_payloads,
                                         const uint64_t *dev_payload_offsets, size_t count, uint8_t *dev_status,
                                         void *stream) {
    OffsetsCall c{kOpSeal, hash_method, dev_payloads, dev_payload_offsets, count};
    c.frame = kFrameDetached;
    c.hdr = dev_msgs;
    c.hdr_off = dev_msg_offsets;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

// The detached calls with both sides by address list: the payloads' addresses ride where their table does and the
// eager messages' where theirs does, with no buffer under either (offsets_call.h: OffsetsCall::both_lists).
int mchecksum_gpu_verify_detached_message_list(const char *hash_method, const uint64_t *dev_msg_addr,
                                               const uint64_t *dev_msg_len, size_t hash_offset,
                                               const uint64_t *dev_payload_addr, const uint64_t *dev_payload_len,
                                               size_t count, uint8_t *dev_status, uint32_t *dev_mismatches, void *stream) {
    OffsetsCall c{kOpVerify, hash_method, nullptr, dev_payload_addr, count};
    c.frame = kFrameDetached;
    c.both_lists = true;
    c.payload_len = dev_payload_len;
    c.hdr_off = dev_msg_addr;
    c.msg_len = dev_msg_len;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_mismatches;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_seal_detached_message_list(const char *hash_method, const uint64_t *dev_msg_addr,
                                             const uint64_t *dev_msg_len, size_t hash_offset,
                                             const uint64_t *dev_payload_addr, const uint64_t *dev_payload_len, size_t count,
                                             uint8_t *dev_status, void *stream) {
    OffsetsCall c{kOpSeal, hash_method, nullptr, dev_payload_addr, count};  // (the slots are written through their addresses)
    c.frame = kFrameDetached;
    c.both_lists = true;
    c.payload_len = dev_payload_len;
    c.hdr_off = dev_msg_addr;
    c.msg_len = dev_msg_len;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_verify_rpc_messages(const char *header_method, const char *payload_method, int kind, const void *dev_buf,
                                      const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                      size_t hash_offset, uint8_t *dev_status, uint32_t *dev_counts, void *stream) {
    OffsetsCall c{kOpVerify, payload_method, dev_buf, dev_msg_offsets, count};
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_counts;  // the six class counts
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_seal_rpc_messages(const char *header_method, const char *payload_method, int kind, void *dev_buf,
                                    const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                    size_t hash_offset, uint8_t *dev_status, void *stream) {
    OffsetsCall c{kOpSeal, payload_method, dev_buf, dev_msg_offsets, count};
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.out = dev_buf;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_unpack_rpc_messages(const char *header_method, const char *payload_method, int kind, const void *dev_buf,
                                      const uint64_t *dev_msg_offsets, size_t count, size_t payload_offset,
                                      size_t hash_offset, void *dev_dst, const uint64_t *dev_dst_offsets,
                                      uint8_t *dev_status, uint32_t *dev_counts, void *stream) {
    // unpack_messages' buffers under verify_rpc_messages' rules: the messages are the source
    OffsetsCall c{kOpUnpack, payload_method, dev_buf, dev_msg_offsets, count};
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.dst = dev_dst;
    c.dst_off = dev_dst_offsets;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_counts;  // the seven class counts
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_pack_rpc_messages(const char *header_method, const char *payload_method, int kind, const void *dev_src,
                                    const uint64_t *dev_src_offsets, void *dev_buf, const uint64_t *dev_msg_offsets,
                                    size_t count, size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
                                    void *stream) {
    // pack_messages' buffers under seal_rpc_messages' rules: the headers (and their flags) are read from dev_buf
    OffsetsCall c{kOpPack, payload_method, dev_src, dev_src_offsets, count};
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.dst = dev_buf;
    c.dst_off = dev_msg_offsets;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

// The four RPC calls with the message side by address list: the addresses ride where the message table does, with
// no buffer under them (offsets_call.h: OffsetsCall::list, msg_len).
int mchecksum_gpu_verify_rpc_message_list(const char *header_method, const char *payload_method, int kind,
                                          const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
                                          size_t payload_offset, size_t hash_offset, uint8_t *dev_status,
                                          uint32_t *dev_counts, void *stream) {
    OffsetsCall c{kOpVerify, payload_method, nullptr, dev_msg_addr, count};
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.list = true;
    c.msg_len = dev_msg_len;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_counts;  // the six class counts
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_seal_rpc_message_list(const char *header_method, const char *payload_method, int kind,
                                        const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
                                        size_t payload_offset, size_t hash_offset, uint8_t *dev_status, void *stream) {
    OffsetsCall c{kOpSeal, payload_method, nullptr, dev_msg_addr, count};  // (no `out`: the addresses are written through)
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.list = true;
    c.msg_len = dev_msg_len;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_unpack_rpc_message_list(const char *header_method, const char *payload_method, int kind,
                                          const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
                                          size_t payload_offset, size_t hash_offset, void *dev_dst,
                                          const uint64_t *dev_dst_offsets, uint8_t *dev_status, uint32_t *dev_counts,
                                          void *stream) {
    OffsetsCall c{kOpUnpack, payload_method, nullptr, dev_msg_addr, count};
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.list = true;
    c.msg_len = dev_msg_len;
    c.dst = dev_dst;
    c.dst_off = dev_dst_offsets;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.mismatches = dev_counts;  // the seven class counts
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_pack_rpc_message_list(const char *header_method, const char *payload_method, int kind,
                                        const void *dev_src, const uint64_t *dev_src_offsets,
                                        const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t count,
                                        size_t payload_offset, size_t hash_offset, uint8_t *dev_status, void *stream) {
    // the list is the written side: the headers (and their flags) are read through it, the source stays a table
    OffsetsCall c{kOpPack, payload_method, dev_src, dev_src_offsets, count};
    c.frame = kFrameRpc;
    c.kind = kind;
    c.hdr_method = header_method;
    c.list = true;
    c.msg_len = dev_msg_len;
    c.dst_off = dev_msg_addr;
    c.pay_off = payload_offset;
    c.hash_off = hash_offset;
    c.status = dev_status;
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_state_verify_messages(const char *hash_method, const void *dev_state, size_t count,
                                        const void *dev_msgs, const uint64_t *dev_msg_offsets, size_t hash_offset,
                                        uint8_t *dev_status, uint32_t *dev_mismatches, void *stream) {
    return state_messages_call(false, hash_method, dev_state, count, const_cast<void *>(dev_msgs), dev_msg_offsets,
                               hash_offset, dev_status, dev_mismatches, stream);
}

int mchecksum_gpu_state_seal_messages(const char *hash_method, const void *dev_state, size_t count, void *dev_msgs,
                                      const uint64_t *dev_msg_offsets, size_t hash_offset, uint8_t *dev_status,
                                      void *stream) {
    return state_messages_call(true, hash_method, dev_state, count, dev_msgs, dev_msg_offsets, hash_offset, dev_status,
                               nullptr, stream);
}

int mchecksum_gpu_state_verify_message_list(const char *hash_method, const void *dev_state, size_t count,
                                            const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t hash_offset,
                                            uint8_t *dev_status, uint32_t *dev_mismatches, void *stream) {
    return state_messages_call(false, hash_method, dev_state, count, nullptr, dev_msg_addr, hash_offset, dev_status,
                               dev_mismatches, stream, true, dev_msg_len);
}

int mchecksum_gpu_state_seal_message_list(const char *hash_method, const void *dev_state, size_t count,
                                          const uint64_t *dev_msg_addr, const uint64_t *dev_msg_len, size_t hash_offset,
                                          uint8_t *dev_status, void *stream) {
    return state_messages_call(true, hash_method, dev_state, count, nullptr, dev_msg_addr, hash_offset, dev_status, nullptr,
                               stream, true, dev_msg_len);
}

int mchecksum_gpu_state_init(const char *hash_method, void *dev_state, size_t count, void *stream) {
    if (count && !dev_state) return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    Model m;
    crc_rmodel_t rm;
    DevCtx *c = nullptr;
    if (int rc = state_call(hash_method, count, &m, &rm, &c)) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    const dim3 grid(elem_grid(count)), block(256);
    const hipError_t e =
        m.width == 64 ? launch_kernel(state_init_kernel<uint64_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (uint64_t *)dev_state, (uint64_t)count, (uint64_t)rm.rinit)
                      : launch_kernel(state_init_kernel<uint32_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (uint32_t *)dev_state, (uint64_t)count, (uint32_t)rm.rinit);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "state init");
}

int mchecksum_gpu_update_offsets(const char *hash_method, const void *dev_base, const uint64_t *dev_offsets,
                                 size_t count, void *dev_state, void *stream) {
    OffsetsCall c{kOpUpdate, hash_method, dev_base, dev_offsets, count};
    c.out = dev_state;  // advanced in place by the seeded twin of the checksum kernel the same plan picks
    c.stream = stream;
    return offsets_call(c);
}

int mchecksum_gpu_copy_offsets(const char *hash_method, const void *dev_src, const uint64_t *dev_src_offsets,
                               void *dev_dst, const uint64_t *dev_dst_starts, size_t count, void *dev_out,
                               void *stream) {
    return copy_call(CopyCall{kCopyChecksum, hash_method, dev_src, dev_src_offsets, dev_dst, dev_dst_starts, count,
                              dev_out, stream});
}

int mchecksum_gpu_update_copy_offsets(const char *hash_method, const void *dev_src, const uint64_t *dev_src_offsets,
                                      void *dev_dst, const uint64_t *dev_dst_starts, size_t count, void *dev_state,
                                      void *stream) {
    // the registers are advanced in place, as update_offsets does, by the seeded twin of the same plan's copy kernel
    return copy_call(CopyCall{kCopyUpdate, hash_method, dev_src, dev_src_offsets, dev_dst, dev_dst_starts, count,
                              dev_state, stream});
}

int mchecksum_gpu_state_get(const char *hash_method, const void *dev_state, size_t count, void *dev_out,
                            void *stream) {
    if (count && (!dev_state || !dev_out)) return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    Model m;
    crc_rmodel_t rm;
    DevCtx *c = nullptr;
    if (int rc = state_call(hash_method, count, &m, &rm, &c)) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    const dim3 grid(elem_grid(count)), block(256);
    const hipError_t e =
        m.width == 64 ? launch_kernel(state_get_kernel<uint64_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (const uint64_t *)dev_state, (uint64_t *)dev_out, (uint64_t)count,
                                      (uint64_t)rm.xorout, rm.msb)
                      : launch_kernel(state_get_kernel<uint32_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (const uint32_t *)dev_state, (uint32_t *)dev_out, (uint64_t)count,
                                      (uint32_t)rm.xorout, rm.msb);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "state get");
}

int mchecksum_gpu_state_verify(const char *hash_method, const void *dev_state, size_t count, const void *dev_expected,
                               uint8_t *dev_status, uint32_t *dev_mismatches, void *stream) {
    if (count && (!dev_state || !dev_expected)) return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    Model m;
    crc_rmodel_t rm;
    DevCtx *c = nullptr;
    if (int rc = state_call(hash_method, count, &m, &rm, &c)) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    // no work-queue slot, no workspace, no device-side wait: nothing to fail closed on
    const dim3 grid(elem_grid(count)), block(256);
    const hipError_t e =
        m.width == 64 ? launch_kernel(state_verify_kernel<uint64_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (const uint64_t *)dev_state, (const uint64_t *)dev_expected, (uint64_t)count,
                                      (uint64_t)rm.xorout, rm.msb, dev_status, dev_mismatches)
                      : launch_kernel(state_verify_kernel<uint32_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (const uint32_t *)dev_state, (const uint32_t *)dev_expected, (uint64_t)count,
                                      (uint32_t)rm.xorout, rm.msb, dev_status, dev_mismatches);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "state verify");
}

int mchecksum_gpu_combine(const char *hash_method, const void *dev_crc_a, const void *dev_crc_b,
                          const uint64_t *dev_len_b, size_t count, void *dev_out, void *stream) {
    if (count && (!dev_crc_a || !dev_crc_b || !dev_len_b || !dev_out))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    Model m;
    crc_rmodel_t rm;
    DevCtx *c = nullptr;
    if (int rc = state_call(hash_method, count, &m, &rm, &c)) return rc;
    const void *shift = nullptr;
    if (int rc = get_ext(c, m.idx, &shift)) return rc;
    if (count == 0) return MCHECKSUM_GPU_OK;
    const dim3 grid(elem_grid(count)), block(256);
    const hipError_t e =
        m.width == 64 ? launch_kernel(combine_kernel<uint64_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (const uint64_t *)dev_crc_a, (const uint64_t *)dev_crc_b, dev_len_b,
                                      (uint64_t *)dev_out, (uint64_t)count, shift, (uint64_t)rm.rinit,
                                      (uint64_t)rm.xorout, rm.msb)
                      : launch_kernel(combine_kernel<uint32_t>, grid, block, (hipStream_t)stream, nullptr,
                                      (const uint32_t *)dev_crc_a, (const uint32_t *)dev_crc_b, dev_len_b,
                                      (uint32_t *)dev_out, (uint64_t)count, shift, (uint32_t)rm.rinit,
                                      (uint32_t)rm.xorout, rm.msb);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "combine");
}

int mchecksum_gpu_combine_runs(const char *hash_method, const void *dev_crc, const uint64_t *dev_len, size_t nchunks,
                               const uint64_t *dev_run_first, size_t nruns, void *dev_out, uint64_t *dev_out_len,
                               void *stream) {
    if ((nruns && (!dev_run_first || !dev_out)) || (nchunks && (!dev_crc || !dev_len)))
        return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if ((uint64_t)nchunks > kMaxUnits) return set_err(MCHECKSUM_GPU_EINVAL, "more than 2^31 chunks in one call");
    Model m;
    crc_rmodel_t rm;
    DevCtx *c = nullptr;
    if (int rc = state_call(hash_method, nruns, &m, &rm, &c)) return rc;  // (nruns <= 2^31, the device, the method)
    const void *shift = nullptr;
    if (int rc = get_ext(c, m.idx, &shift)) return rc;
    if (nruns == 0) return MCHECKSUM_GPU_OK;
    // no work-queue slot, no workspace, no device-side wait: nothing to fail closed on
    const hipError_t e = m.width == 64 ? launch_combine_runs<uint64_t>(rm, shift, dev_crc, dev_len, nchunks, dev_run_first,
                                                                       nruns, dev_out, dev_out_len, stream)
                                       : launch_combine_runs<uint32_t>(rm, shift, dev_crc, dev_len, nchunks, dev_run_first,
                                                                       nruns, dev_out, dev_out_len, stream);
    return e == hipSuccess ? MCHECKSUM_GPU_OK : hip_err(e, "combine_runs");
}

const char *mchecksum_gpu_last_error(void) { return t_err; }

void mchecksum_gpu_reload_settings(void) { mck_settings_reload(); }

int mchecksum_gpu_set_error_word(uint32_t *dev_word) {
    t_err_word = dev_word;
    return MCHECKSUM_GPU_OK;
}

long long mchecksum_gpu_queue_faults(void) {
    if (!mchecksum_gpu_available()) return -1;
    unsigned int n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_mck_queue_faults), sizeof(n), 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    // mchecksum_gpu_ext.hip's kernels (the segment chunk queue) count into
    // their own translation unit's copy of the counter
    const long long ext = ext_queue_faults();
    if (ext < 0) return -1;
    return (long long)n + ext;
}

int mchecksum_gpu_queue_stats(long long *stats, size_t n) {
    if (!stats) return set_err(MCHECKSUM_GPU_EINVAL, "NULL pointer argument");
    if (!mchecksum_gpu_available()) return set_err(MCHECKSUM_GPU_ENODEV, "no HIP device");
    DevCtx *c = nullptr;
    int rc = device_ctx(&c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->pool_mu);
    const long long v[MCHECKSUM_GPU_QSTAT_COUNT] = {c->n_slot, c->n_noslot, c->n_reaped, c->n_busy_skip,
                                                    (long long)c->in_flight.size()};
    for (size_t i = 0; i < n && i < MCHECKSUM_GPU_QSTAT_COUNT; i++) stats[i] = v[i];
    return MCHECKSUM_GPU_OK;
}

#if MCK_TRACE
// Diagnostic builds only: copy what the last launch left in a device symbol.
#define MCK_DEBUG_READ(name, sym)                                                                                     \
    MCHECKSUM_PUBLIC int name(void *host, size_t bytes) {                                                             \
        if (bytes > sizeof(sym)) bytes = sizeof(sym);                                                                 \
        return hipMemcpyFromSymbol(host, HIP_SYMBOL(sym), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;    \
    }
MCK_DEBUG_READ(mck_debug_trace_read, g_mck_trace)          // the per-wave stamps
MCK_DEBUG_READ(mck_debug_qwave_read, g_mck_qwave)          // the per-wave work-queue timings
MCK_DEBUG_READ(mck_debug_units_read, g_mck_unit_end)       // the per-unit completion stamps
MCK_DEBUG_READ(mck_debug_trace_xcc_read, g_mck_trace_xcc)  // the XCD of each wave
MCK_DEBUG_READ(mck_debug_trace_clk_read, g_mck_trace_clk)  // the shader-clock stamps (entry, exit) of each wave
#undef MCK_DEBUG_READ
// ... and the work-queue fault records (count, then 4 words per record).
MCHECKSUM_PUBLIC int mck_debug_qdiag_read(unsigned int *n, unsigned long long *rec) {
    if (hipMemcpyFromSymbol(n, HIP_SYMBOL(g_mck_qdiag_n), sizeof(*n), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(rec, HIP_SYMBOL(g_mck_qdiag), sizeof(g_mck_qdiag), 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
