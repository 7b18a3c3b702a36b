// copy_plan.h -- which copy kernel a copy-and-checksum call launches
// (mchecksum_gpu_copy_offsets, mchecksum_gpu_update_copy_offsets): the kernels
// of crc_gpu_copy.h are a family of their own beside the batch kernels, keyed
// here.  The launch itself -- layout, non-temporal loads, grid, work-queue
// slot -- is the plan of checksum_offsets / update_offsets for the same count
// (launch_plan.h: plan_offsets, unchanged).  Pure, like launch_plan.h: the host
// compiler checks it on the CPU (tests/native/copy_plan.cpp).
#ifndef MCK_COPY_PLAN_H
#define MCK_COPY_PLAN_H

#include "launch_plan.h"

namespace mck {

// What the owning lane does with a chunk's CRC x, the chunk having been copied
// by the payload loop: store x ^ xorout in out[p], or advance the running
// register state[p] over the chunk (kOpChecksum's and kOpUpdate's epilogues).
enum CopyOp : int { kCopyChecksum, kCopyUpdate };

// One instantiation of the copy kernels (crc32c_copy_kernel,
// crc64_copy_kernel): offsets mode, one chunk per wave.
struct CopyKey {
    int width, op;
    bool nt, light;
};
constexpr bool operator==(const CopyKey &a, const CopyKey &b) {
    return a.width == b.width && a.op == b.op && a.nt == b.nt && a.light == b.light;
}

// The 10 instantiations there are: CRC-32C {checksum, update} x {light, full,
// non-temporal}, CRC-64 {checksum, update} x {full, non-temporal}.
// copy_kernel_for has exactly these, and each kernel asserts it is one of them.
constexpr bool copy_key_valid(const CopyKey &k) {
    if (k.width != 32 && k.width != 64) return false;
    if (k.op != kCopyChecksum && k.op != kCopyUpdate) return false;
    if (k.light && (k.width != 32 || k.nt)) return false;  // light: CRC-32C only, and no non-temporal form
    return true;
}

// The kernel an offsets plan launches for op.
inline CopyKey copy_key(const LaunchPlan &p, CopyOp op) {
    CopyKey k{p.width, op, p.nt, p.light};
    if (k.width != 32) k.light = false;
    if (k.light) k.nt = false;
    return k;
}

}  // namespace mck

#endif  // MCK_COPY_PLAN_H
