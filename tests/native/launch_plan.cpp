// Host check of the launch plan (launch_plan.h): which batch kernel a call
// launches and how, as a table of literal expectations.  Every number below
// was taken from the scattered decision functions this header replaced (a
// differential sweep over ~800 000 shapes agreed with them in every field),
// so an edit that moves a threshold, a lane count or a grid fails here, on the
// CPU.  So does one that changes which kernel a plan leads to for the call's
// operation (kernel_key), or which kernels there are (kernel_key_valid).
// Plain C++: no HIP header.
#include "launch_plan.h"

#include <cstdio>
#include <initializer_list>

using namespace mck;

static int fails = 0, checks = 0;
#define CHECK(c, ...)                       \
    do {                                    \
        checks++;                           \
        if (!(c)) {                         \
            if (fails++ < 20) {             \
                printf("FAIL: " __VA_ARGS__); \
                printf("\n");               \
            }                               \
        }                                   \
    } while (0)

// a settings snapshot: gpu_log2g, gpu_light, gpu_nt, gpu_split, gpu_split_lds, gpu_force_generic
struct Set {
    int lg, light, nt, split, split_lds, generic;
    mck_settings_t snapshot() const {
        mck_settings_t s{};
        s.gpu_log2g = lg, s.gpu_light = light, s.gpu_nt = nt, s.gpu_split = split;
        s.gpu_split_lds = split_lds, s.gpu_force_generic = generic, s.gpu_xdr_fast = -1;
        return s;
    }
};
static const Set D{-1, -1, -1, -1, 1, 0};  // nothing set: the library decides
static const Set LG0{0, -1, -1, -1, 1, 0}, LG6{6, -1, -1, -1, 1, 0}, LIGHT0{-1, 0, -1, -1, 1, 0}, LIGHT1{-1, 1, -1, -1, 1, 0},
    NT0{-1, -1, 0, -1, 1, 0}, NT1{-1, -1, 1, -1, 1, 0}, SPLIT0{-1, -1, -1, 0, 1, 0}, SPLIT1{-1, -1, -1, 1, 1, 0},
    LDS0{-1, -1, -1, -1, 0, 0}, SPLIT1_LDS0{-1, -1, -1, 1, 0, 0}, GENERIC{-1, -1, -1, -1, 1, 1};
static const uintptr_t A = 0x7f0000000000ull;  // a 16-byte aligned device address

struct FixedRow {
    const char *name;
    Set set;
    int cus, width;
    uintptr_t base;
    size_t stride, len, count;
    // expected
    int lg, mode;
    bool light, aligned, nt, split;
    uint32_t split_log2;
    bool split_lds_ok, zero_out, dyn;
    uint64_t units;
    int block, blocks_per_cu;
    unsigned grid;
};
static const FixedRow kFixed[] = {
    {"headline: 65536 x 64 KiB crc32c", D, 256, 32, A + 0, 65536, 65536, 65536, /**/ 6, kFixedAligned, 0, 1, 1, 0, 0, 0, 0, 1, 65536ull, 1024, 1, 256},
    {"C2: 65536 x 4 KiB crc32c", D, 256, 32, A + 0, 4096, 4096, 65536, /**/ 4, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 16384ull, 1024, 1, 256},
    {"C3: 8192 x 1 MiB crc64", D, 256, 64, A + 0, 1048576, 1048576, 8192, /**/ 6, kFixedAligned, 0, 1, 1, 1, 2, 1, 0, 1, 32768ull, 1024, 1, 256},
    {"light, 1024 x 4 KiB: keeps 64 lanes", D, 256, 32, A + 0, 4096, 4096, 1024, /**/ 6, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 1024ull, 256, 8, 256},
    {"light, 4096 x 4 KiB: four waves per CU at 16 lanes", D, 256, 32, A + 0, 4096, 4096, 4096, /**/ 4, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 1024ull, 256, 8, 256},
    {"light, 2048 x 4 KiB", D, 256, 32, A + 0, 4096, 4096, 2048, /**/ 5, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 1024ull, 256, 8, 256},
    {"full, 8192 x 4 KiB: lanes raised to fill 16 wave slots per CU", D, 256, 32, A + 0, 4096, 4096, 8192, /**/ 5, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 4096ull, 1024, 1, 256},
    {"full, 16384 x 4 KiB", D, 256, 32, A + 0, 4096, 4096, 16384, /**/ 4, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 4096ull, 1024, 1, 256},
    {"full, 4097 x 4 KiB: just past the light layout's 16 MiB", D, 256, 32, A + 0, 4096, 4096, 4097, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 4097ull, 1024, 1, 256},
    {"nt, 131072 x 4 KiB: 512 MiB", D, 256, 32, A + 0, 4096, 4096, 131072, /**/ 4, kFixedAligned, 0, 1, 1, 0, 0, 0, 0, 1, 32768ull, 1024, 1, 256},
    {"not nt, 131071 x 4 KiB: just under 512 MiB", D, 256, 32, A + 0, 4096, 4096, 131071, /**/ 4, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 32768ull, 1024, 1, 256},
    {"misaligned base", D, 256, 32, A + 8, 65536, 65536, 65536, /**/ 6, kFixedGeneric, 0, 0, 0, 0, 0, 0, 0, 0, 65536ull, 1024, 1, 256},
    {"stride not a multiple of 16", D, 256, 32, A + 0, 65544, 65536, 65536, /**/ 6, kFixedGeneric, 0, 0, 0, 0, 0, 0, 0, 0, 65536ull, 1024, 1, 256},
    {"stride not a multiple of 16, one payload", D, 256, 32, A + 0, 65544, 65536, 1, /**/ 6, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 1ull, 256, 8, 1},
    {"len not a multiple of step * kRing", D, 256, 32, A + 0, 66560, 66560, 65536, /**/ 6, kFixedGeneric, 0, 0, 0, 0, 0, 0, 0, 0, 65536ull, 1024, 1, 256},
    {"light, len not a multiple of step * kRing", D, 256, 32, A + 0, 4112, 4112, 1024, /**/ 6, kFixedGeneric, 1, 0, 0, 0, 0, 0, 0, 0, 1024ull, 256, 8, 256},
    {"crc64 misaligned base", D, 256, 64, A + 8, 1048576, 1048576, 8192, /**/ 6, kFixedGeneric, 0, 0, 0, 0, 0, 0, 0, 0, 8192ull, 1024, 1, 256},
    {"crc64 static, 255 units", D, 256, 64, A + 0, 4096, 4096, 255, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 255ull, 1024, 1, 255},
    {"crc64 static, 256 units", D, 256, 64, A + 0, 4096, 4096, 256, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 256ull, 1024, 1, 256},
    {"crc64 static, 4095 units", D, 256, 64, A + 0, 4096, 4096, 4095, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 4095ull, 1024, 1, 256},
    {"crc64 static, 4096 units", D, 256, 64, A + 0, 4096, 4096, 4096, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 4096ull, 1024, 1, 256},
    {"crc64 static, one payload", D, 256, 64, A + 0, 4096, 4096, 1, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 1ull, 1024, 1, 1},
    {"crc64 64 KiB x 65536: 32 lanes, static", D, 256, 64, A + 0, 65536, 65536, 65536, /**/ 5, kFixedAligned, 0, 1, 1, 0, 0, 0, 0, 0, 32768ull, 1024, 1, 256},
    {"crc64 512 KiB x 3: too small to split by default", D, 256, 64, A + 0, 524288, 524288, 3, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 3ull, 1024, 1, 3},
    {"cus 304 headline", D, 304, 32, A + 0, 65536, 65536, 65536, /**/ 6, kFixedAligned, 0, 1, 1, 0, 0, 0, 0, 1, 65536ull, 1024, 1, 304},
    // every override, on one shape each
    {"gpu_log2g 0 on C2", LG0, 256, 32, A + 0, 4096, 4096, 65536, /**/ 0, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 1024ull, 1024, 1, 64},
    {"gpu_log2g 6 on C2", LG6, 256, 32, A + 0, 4096, 4096, 65536, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 65536ull, 1024, 1, 256},
    {"gpu_log2g 0 on a light batch", LG0, 256, 32, A + 0, 4096, 4096, 4096, /**/ 0, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 64ull, 256, 8, 16},
    {"gpu_log2g 6 on a light batch", LG6, 256, 32, A + 0, 4096, 4096, 4096, /**/ 6, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 4096ull, 256, 8, 1024},
    {"gpu_light 0 on 1024 x 4 KiB", LIGHT0, 256, 32, A + 0, 4096, 4096, 1024, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 1024ull, 1024, 1, 64},
    {"gpu_light 1 on the headline", LIGHT1, 256, 32, A + 0, 65536, 65536, 65536, /**/ 0, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 1024ull, 256, 8, 256},
    {"gpu_light 1 leaves crc64 alone", LIGHT1, 256, 64, A + 0, 4096, 4096, 1024, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 1024ull, 1024, 1, 256},
    {"gpu_nt 0 on the headline", NT0, 256, 32, A + 0, 65536, 65536, 65536, /**/ 6, kFixedAligned, 0, 1, 0, 0, 0, 0, 0, 0, 65536ull, 1024, 1, 256},
    {"gpu_nt 1 on 64 x 4 KiB", NT1, 256, 32, A + 0, 4096, 4096, 64, /**/ 6, kFixedAligned, 1, 1, 0, 0, 0, 0, 0, 0, 64ull, 256, 8, 16},
    {"gpu_nt 1 on C2", NT1, 256, 32, A + 0, 4096, 4096, 65536, /**/ 4, kFixedAligned, 0, 1, 1, 0, 0, 0, 0, 1, 16384ull, 1024, 1, 256},
    {"gpu_split 0 on C3", SPLIT0, 256, 64, A + 0, 1048576, 1048576, 8192, /**/ 6, kFixedAligned, 0, 1, 1, 0, 0, 0, 0, 0, 8192ull, 1024, 1, 256},
    {"gpu_split 1 on 3 x 512 KiB crc64", SPLIT1, 256, 64, A + 0, 524288, 524288, 3, /**/ 6, kFixedAligned, 0, 1, 0, 1, 1, 0, 1, 1, 6ull, 1024, 1, 1},
    {"gpu_split 1, gpu_split_lds 0 on 3 x 512 KiB crc64", SPLIT1_LDS0, 256, 64, A + 0, 524288, 524288, 3, /**/ 6, kFixedAligned, 0, 1, 0, 1, 1, 0, 1, 1, 6ull, 1024, 1, 1},
    {"gpu_split_lds 0 on C3", LDS0, 256, 64, A + 0, 1048576, 1048576, 8192, /**/ 6, kFixedAligned, 0, 1, 1, 1, 2, 0, 1, 1, 32768ull, 1024, 1, 256},
    {"gpu_force_generic 1 on the headline", GENERIC, 256, 32, A + 0, 65536, 65536, 65536, /**/ 6, kFixedGeneric, 0, 0, 0, 0, 0, 0, 0, 0, 65536ull, 1024, 1, 256},
    {"gpu_force_generic 1 on C3", GENERIC, 256, 64, A + 0, 1048576, 1048576, 8192, /**/ 6, kFixedGeneric, 0, 0, 0, 0, 0, 0, 0, 0, 8192ull, 1024, 1, 256},
};

struct OffsetsRow {
    const char *name;
    Set set;
    int cus, width;
    size_t count;
    // expected (lg 6, kOffsets, one unit per payload)
    bool light, nt, dyn;
    uint64_t units;
    int block, blocks_per_cu;
    unsigned grid;
};
static const OffsetsRow kOffsetsRows[] = {
    {"crc32c x 1", D, 256, 32, 1, /**/ 1, 0, 0, 1ull, 256, 8, 1},
    {"crc32c x 1024", D, 256, 32, 1024, /**/ 1, 0, 0, 1024ull, 256, 8, 256},
    {"crc32c x 1025", D, 256, 32, 1025, /**/ 0, 0, 1, 1025ull, 1024, 1, 65},
    {"crc32c x 8191", D, 256, 32, 8191, /**/ 0, 0, 1, 8191ull, 1024, 1, 256},
    {"crc32c x 8192", D, 256, 32, 8192, /**/ 0, 1, 1, 8192ull, 1024, 1, 256},
    {"crc32c x 1000000", D, 256, 32, 1000000, /**/ 0, 1, 1, 1000000ull, 1024, 1, 256},
    {"crc64 x 1", D, 256, 64, 1, /**/ 0, 0, 1, 1ull, 1024, 2, 1},
    {"crc64 x 1024", D, 256, 64, 1024, /**/ 0, 0, 1, 1024ull, 1024, 2, 64},
    {"crc64 x 1025", D, 256, 64, 1025, /**/ 0, 0, 1, 1025ull, 1024, 2, 65},
    {"crc64 x 8191", D, 256, 64, 8191, /**/ 0, 0, 1, 8191ull, 1024, 2, 512},
    {"crc64 x 8192", D, 256, 64, 8192, /**/ 0, 1, 1, 8192ull, 1024, 2, 512},
    {"crc64 x 1000000", D, 256, 64, 1000000, /**/ 0, 1, 1, 1000000ull, 1024, 2, 512},
    {"gpu_light 0 at 1024", LIGHT0, 256, 32, 1024, /**/ 0, 0, 1, 1024ull, 1024, 1, 64},
    {"gpu_light 1 at 8192", LIGHT1, 256, 32, 8192, /**/ 1, 0, 0, 8192ull, 256, 8, 2048},
    {"gpu_light 1 leaves crc64 alone", LIGHT1, 256, 64, 1024, /**/ 0, 0, 1, 1024ull, 1024, 2, 64},
    {"gpu_nt 1 at 1025", NT1, 256, 32, 1025, /**/ 0, 1, 1, 1025ull, 1024, 1, 65},
    {"gpu_nt 1 at 1024 (light: no non-temporal form)", NT1, 256, 32, 1024, /**/ 1, 0, 0, 1024ull, 256, 8, 256},
    {"gpu_nt 0 at 8192", NT0, 256, 64, 8192, /**/ 0, 0, 1, 8192ull, 1024, 2, 512},
    {"cus 8", D, 8, 64, 8192, /**/ 0, 1, 1, 8192ull, 1024, 2, 16},
};

// The kernel a plan leads to for the call's operation (kernel_key): the
// expected KernelKey is {width, lg, mode, op, nt, light, split}.
struct OffsetsKeyRow {
    const char *name;
    Set set;
    int width;
    size_t count;
    BatchOp op;
    KernelKey key;
};
#define OP_ROWS32(OP)                                                                                   \
    {#OP " crc32c x 1024: light", D, 32, 1024, OP, {32, 6, kOffsets, OP, 0, 1, 0}},                     \
    {#OP " crc32c x 1025: full", D, 32, 1025, OP, {32, 6, kOffsets, OP, 0, 0, 0}},                      \
    {#OP " crc32c x 8191: full", D, 32, 8191, OP, {32, 6, kOffsets, OP, 0, 0, 0}},                      \
    {#OP " crc32c x 8192: nt", D, 32, 8192, OP, {32, 6, kOffsets, OP, 1, 0, 0}},                        \
    {#OP " gpu_light 0 at 1024: full", LIGHT0, 32, 1024, OP, {32, 6, kOffsets, OP, 0, 0, 0}},           \
    {#OP " gpu_light 1 at 8192: light, no nt form", LIGHT1, 32, 8192, OP, {32, 6, kOffsets, OP, 0, 1, 0}}, \
    {#OP " gpu_nt 0 at 8192: full", NT0, 32, 8192, OP, {32, 6, kOffsets, OP, 0, 0, 0}},                 \
    {#OP " gpu_nt 1 at 1025: nt", NT1, 32, 1025, OP, {32, 6, kOffsets, OP, 1, 0, 0}},                   \
    {#OP " gpu_nt 1 at 1024: light, no nt form", NT1, 32, 1024, OP, {32, 6, kOffsets, OP, 0, 1, 0}}
#define OP_ROWS64(OP)                                                                                   \
    {#OP " crc64 x 1024: full", D, 64, 1024, OP, {64, 6, kOffsets, OP, 0, 0, 0}},                       \
    {#OP " crc64 x 1025: full", D, 64, 1025, OP, {64, 6, kOffsets, OP, 0, 0, 0}},                       \
    {#OP " crc64 x 8191: full", D, 64, 8191, OP, {64, 6, kOffsets, OP, 0, 0, 0}},                       \
    {#OP " crc64 x 8192: nt", D, 64, 8192, OP, {64, 6, kOffsets, OP, 1, 0, 0}},                         \
    {#OP " crc64, gpu_light 0 at 1024", LIGHT0, 64, 1024, OP, {64, 6, kOffsets, OP, 0, 0, 0}},          \
    {#OP " crc64, gpu_light 1 at 1024: no light form", LIGHT1, 64, 1024, OP, {64, 6, kOffsets, OP, 0, 0, 0}}, \
    {#OP " crc64, gpu_nt 0 at 8192", NT0, 64, 8192, OP, {64, 6, kOffsets, OP, 0, 0, 0}},                \
    {#OP " crc64, gpu_nt 1 at 1024", NT1, 64, 1024, OP, {64, 6, kOffsets, OP, 1, 0, 0}}
static const OffsetsKeyRow kOffsetsKeys[] = {
    OP_ROWS32(kOpChecksum), OP_ROWS32(kOpVerify), OP_ROWS32(kOpUpdate), OP_ROWS32(kOpSeal), OP_ROWS32(kOpPack),
    OP_ROWS32(kOpUnpack),   OP_ROWS64(kOpChecksum), OP_ROWS64(kOpVerify), OP_ROWS64(kOpUpdate),
};
#undef OP_ROWS32
#undef OP_ROWS64

// (fixed batches are checksums)
struct FixedKeyRow {
    const char *name;
    Set set;
    int width;
    uintptr_t base;
    size_t len, count;
    KernelKey key;
};
static const FixedKeyRow kFixedKeys[] = {
    {"headline", D, 32, A, 65536, 65536, {32, 6, kFixedAligned, kOpChecksum, 1, 0, 0}},
    {"C2", D, 32, A, 4096, 65536, {32, 4, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"C3: split, nt", D, 64, A, 1048576, 8192, {64, 6, kFixedAligned, kOpChecksum, 1, 0, 1}},
    {"light 1024 x 4 KiB", D, 32, A, 4096, 1024, {32, 6, kFixedAligned, kOpChecksum, 0, 1, 0}},
    {"light 4096 x 4 KiB", D, 32, A, 4096, 4096, {32, 4, kFixedAligned, kOpChecksum, 0, 1, 0}},
    {"full 4097 x 4 KiB", D, 32, A, 4096, 4097, {32, 6, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"nt, 131072 x 4 KiB", D, 32, A, 4096, 131072, {32, 4, kFixedAligned, kOpChecksum, 1, 0, 0}},
    {"not nt, 131071 x 4 KiB", D, 32, A, 4096, 131071, {32, 4, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"misaligned headline: generic, no nt form", D, 32, A + 8, 65536, 65536, {32, 6, kFixedGeneric, kOpChecksum, 0, 0, 0}},
    {"light generic", D, 32, A, 4112, 1024, {32, 6, kFixedGeneric, kOpChecksum, 0, 1, 0}},
    {"crc64 misaligned C3: generic", D, 64, A + 8, 1048576, 8192, {64, 6, kFixedGeneric, kOpChecksum, 0, 0, 0}},
    {"crc64 1024 x 4 KiB", D, 64, A, 4096, 1024, {64, 6, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"crc64 64 KiB x 65536: 32 lanes, nt", D, 64, A, 65536, 65536, {64, 5, kFixedAligned, kOpChecksum, 1, 0, 0}},
    {"gpu_log2g 0 on C2", LG0, 32, A, 4096, 65536, {32, 0, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"gpu_light 0 on 1024 x 4 KiB", LIGHT0, 32, A, 4096, 1024, {32, 6, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"gpu_light 1 on the headline: light, no nt form", LIGHT1, 32, A, 65536, 65536, {32, 0, kFixedAligned, kOpChecksum, 0, 1, 0}},
    {"gpu_light 1 leaves crc64 alone", LIGHT1, 64, A, 4096, 1024, {64, 6, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"gpu_nt 0 on the headline", NT0, 32, A, 65536, 65536, {32, 6, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"gpu_nt 1 on C2", NT1, 32, A, 4096, 65536, {32, 4, kFixedAligned, kOpChecksum, 1, 0, 0}},
    {"gpu_nt 1 on 64 x 4 KiB: light, no nt form", NT1, 32, A, 4096, 64, {32, 6, kFixedAligned, kOpChecksum, 0, 1, 0}},
    {"gpu_nt 1 on the misaligned headline: generic, no nt form", NT1, 32, A + 8, 65536, 65536, {32, 6, kFixedGeneric, kOpChecksum, 0, 0, 0}},
    {"gpu_split 0 on C3", SPLIT0, 64, A, 1048576, 8192, {64, 6, kFixedAligned, kOpChecksum, 1, 0, 0}},
    {"gpu_split 1 on 3 x 512 KiB crc64: split, not nt", SPLIT1, 64, A, 524288, 3, {64, 6, kFixedAligned, kOpChecksum, 0, 0, 1}},
    {"gpu_force_generic 1 on C3", GENERIC, 64, A, 1048576, 8192, {64, 6, kFixedGeneric, kOpChecksum, 0, 0, 0}},
};

// kernel_key_valid: no kernel has these forms
static const struct {
    const char *name;
    KernelKey key;
} kNoKernel[] = {
    {"update of a fixed batch", {32, 6, kFixedAligned, kOpUpdate, 0, 0, 0}},
    {"update below 64 lanes", {32, 5, kOffsets, kOpUpdate, 0, 0, 0}},
    {"crc64 update of a fixed batch", {64, 6, kFixedGeneric, kOpUpdate, 0, 0, 0}},
    {"crc64 update below 64 lanes", {64, 0, kOffsets, kOpUpdate, 0, 0, 0}},
    {"crc64 update of split pieces", {64, 6, kFixedAligned, kOpUpdate, 1, 0, 1}},
    {"seal of a fixed batch", {32, 6, kFixedAligned, kOpSeal, 0, 0, 0}},
    {"seal below 64 lanes", {32, 4, kOffsets, kOpSeal, 0, 1, 0}},
    {"crc64 seal", {64, 6, kOffsets, kOpSeal, 0, 0, 0}},
    {"pack of a fixed batch", {32, 6, kFixedGeneric, kOpPack, 0, 0, 0}},
    {"pack below 64 lanes", {32, 3, kOffsets, kOpPack, 1, 0, 0}},
    {"crc64 pack", {64, 6, kOffsets, kOpPack, 1, 0, 0}},
    {"unpack of a fixed batch", {32, 6, kFixedAligned, kOpUnpack, 1, 0, 0}},
    {"unpack below 64 lanes", {32, 5, kOffsets, kOpUnpack, 0, 0, 0}},
    {"crc64 unpack", {64, 6, kOffsets, kOpUnpack, 0, 0, 0}},
    {"verify of a fixed batch", {32, 6, kFixedAligned, kOpVerify, 0, 0, 0}},
    {"verify of split pieces", {64, 6, kFixedAligned, kOpVerify, 1, 0, 1}},
    {"split below 64 lanes", {64, 5, kFixedAligned, kOpChecksum, 1, 0, 1}},
    {"split generic", {64, 6, kFixedGeneric, kOpChecksum, 0, 0, 1}},
    {"split offsets", {64, 6, kOffsets, kOpChecksum, 0, 0, 1}},
    {"split crc32c", {32, 6, kFixedAligned, kOpChecksum, 1, 0, 1}},
    {"offsets checksum below 64 lanes", {32, 5, kOffsets, kOpChecksum, 0, 0, 0}},
    {"light with nt", {32, 6, kOffsets, kOpChecksum, 1, 1, 0}},
    {"light crc64", {64, 6, kOffsets, kOpChecksum, 0, 1, 0}},
    {"generic with nt", {32, 6, kFixedGeneric, kOpChecksum, 1, 0, 0}},
    {"no such width", {16, 6, kOffsets, kOpChecksum, 0, 0, 0}},
    {"no such lane count", {32, 7, kFixedAligned, kOpChecksum, 0, 0, 0}},
    {"no such mode", {32, 6, 3, kOpChecksum, 0, 0, 0}},
    {"no such operation", {32, 6, kOffsets, kOpUnpack + 1, 0, 0, 0}},
    {"in place is no key's frame (kernel_key folds it)", {32, 6, kOffsets, kOpVerify, 0, 0, 0, kFrameInPlace}},
    {"no such frame", {32, 6, kOffsets, kOpVerify, 0, 0, 0, (MsgFrame)(kFrameRpc + 1)}},
    {"detached pack", {32, 6, kOffsets, kOpPack, 0, 0, 0, kFrameDetached}},
    {"detached checksum", {32, 6, kOffsets, kOpChecksum, 0, 0, 0, kFrameDetached}},
    {"RPC update", {32, 6, kOffsets, kOpUpdate, 0, 0, 0, kFrameRpc}},
    {"crc64 RPC verify", {64, 6, kOffsets, kOpVerify, 0, 0, 0, kFrameRpc}},
    {"RPC verify of a fixed batch", {32, 6, kFixedAligned, kOpVerify, 0, 0, 0, kFrameRpc}},
};

// choose_log2g(width, len) with nothing forced
static const struct {
    int width;
    size_t len;
    int lg;
} kLanes[] = {
    {32, 0, 0},
    {32, 255, 0},
    {32, 512, 1},
    {32, 1023, 1},
    {32, 1024, 2},
    {32, 2048, 3},
    {32, 4096, 4},
    {32, 8191, 4},
    {32, 8192, 4},
    {32, 16384, 5},
    {32, 32768, 6},
    {32, 65536, 6},
    {32, 1048576, 6},
    {64, 0, 0},
    {64, 255, 0},
    {64, 512, 1},
    {64, 1023, 1},
    {64, 1024, 2},
    {64, 2048, 2},
    {64, 4096, 2},
    {64, 8191, 2},
    {64, 8192, 2},
    {64, 16384, 3},
    {64, 32768, 4},
    {64, 65536, 5},
    {64, 1048576, 6},
};
// light_log2g(len) with nothing forced
static const struct {
    size_t len;
    int lg;
} kLightLanes[] = {
    {0, 0},
    {63, 0},
    {64, 0},
    {1024, 4},
    {2047, 4},
    {2048, 5},
    {4095, 5},
    {4096, 6},
    {65536, 6},
};

static void check_fixed(const FixedRow &r, const LaunchPlan &p) {
    CHECK(p.width == r.width && p.lg == r.lg && p.mode == r.mode, "%s: width %d lg %d mode %d", r.name, p.width, p.lg, p.mode);
    CHECK(p.light == r.light && p.aligned == r.aligned && p.nt == r.nt, "%s: light %d aligned %d nt %d", r.name, p.light,
          p.aligned, p.nt);
    CHECK(p.split == r.split && p.split_log2 == r.split_log2 && p.split_lds_ok == r.split_lds_ok && p.zero_out == r.zero_out,
          "%s: split %d split_log2 %u split_lds_ok %d zero_out %d", r.name, p.split, p.split_log2, p.split_lds_ok, p.zero_out);
    CHECK(p.dyn == r.dyn && p.units == r.units, "%s: dyn %d units %llu", r.name, p.dyn, (unsigned long long)p.units);
    CHECK(p.block == r.block && p.blocks_per_cu == r.blocks_per_cu && p.grid == r.grid, "%s: block %d x %d per CU, grid %u",
          r.name, p.block, p.blocks_per_cu, p.grid);
}

static void check_offsets(const OffsetsRow &r, const LaunchPlan &p) {
    CHECK(p.width == r.width && p.lg == CRC_GPU_MAX_LOG2G && p.mode == kOffsets && !p.aligned && !p.split && !p.zero_out,
          "%s: width %d lg %d mode %d", r.name, p.width, p.lg, p.mode);
    CHECK(p.light == r.light && p.nt == r.nt && p.dyn == r.dyn && p.units == r.units, "%s: light %d nt %d dyn %d units %llu",
          r.name, p.light, p.nt, p.dyn, (unsigned long long)p.units);
    CHECK(p.block == r.block && p.blocks_per_cu == r.blocks_per_cu && p.grid == r.grid, "%s: block %d x %d per CU, grid %u",
          r.name, p.block, p.blocks_per_cu, p.grid);
}

int main() {
    // the table a plan's lg indexes in the library (DevCtx::pack[model][lg]):
    // a sanitizer build of this program sees any lg outside it
    int pack_use[CRC_GPU_MAX_LOG2G + 1] = {};
    for (const FixedRow &r : kFixed) {
        const mck_settings_t s = r.set.snapshot();
        const LaunchPlan p = plan_fixed(s, r.cus, r.width, r.base, r.stride, r.len, r.count);
        check_fixed(r, p);
        pack_use[p.lg]++;
    }
    for (const OffsetsRow &r : kOffsetsRows) {
        const mck_settings_t s = r.set.snapshot();
        const LaunchPlan p = plan_offsets(s, r.cus, r.width, r.count);
        check_offsets(r, p);
        pack_use[p.lg]++;
    }
    // the kernel each plan leads to
    auto same_key = [](const char *name, const KernelKey &k, const KernelKey &want) {
        CHECK(k == want && kernel_key_valid(k), "%s: key {%d, %d, %d, %d, nt %d, light %d, split %d}%s", name, k.width, k.lg,
              k.mode, k.op, k.nt, k.light, k.split, kernel_key_valid(k) ? "" : " (not valid)");
    };
    for (const OffsetsKeyRow &r : kOffsetsKeys)
        same_key(r.name, kernel_key(plan_offsets(r.set.snapshot(), 256, r.width, r.count), r.op), r.key);
    for (const FixedKeyRow &r : kFixedKeys)
        same_key(r.name, kernel_key(plan_fixed(r.set.snapshot(), 256, r.width, r.base, r.len, r.len, r.count), kOpChecksum), r.key);
    for (const auto &r : kNoKernel) CHECK(!kernel_key_valid(r.key), "%s: valid", r.name);
    // what a plan says of the batch and the kernel has no form for is dropped
    {
        LaunchPlan p;
        p.width = 64, p.lg = 3, p.mode = kOffsets, p.nt = true, p.light = true;
        same_key("hand-made crc64 offsets plan", kernel_key(p, kOpVerify), {64, 6, kOffsets, kOpVerify, 1, 0, 0});
        p.width = 32;
        same_key("hand-made light offsets plan", kernel_key(p, kOpSeal), {32, 6, kOffsets, kOpSeal, 0, 1, 0});
        p.mode = kFixedGeneric, p.light = false;
        same_key("hand-made generic plan", kernel_key(p, kOpChecksum), {32, 3, kFixedGeneric, kOpChecksum, 0, 0, 0});
        p.split = true;
        same_key("hand-made split plan", kernel_key(p, kOpChecksum), {64, 6, kFixedAligned, kOpChecksum, 1, 0, 1});
    }
    // Every plan of the tables above, with every operation: a key is valid
    // exactly when the operation is one the plan's kind of batch has (fixed
    // batches: checksums; offsets batches: all six for CRC-32C, no seal, pack
    // or unpack for CRC-64).
    for (int op = kOpChecksum; op <= kOpUnpack; op++) {
        for (const FixedRow &r : kFixed) {
            const LaunchPlan p = plan_fixed(r.set.snapshot(), r.cus, r.width, r.base, r.stride, r.len, r.count);
            CHECK(kernel_key_valid(kernel_key(p, (BatchOp)op)) == (op == kOpChecksum), "%s, op %d: valid key", r.name, op);
        }
        for (const OffsetsRow &r : kOffsetsRows) {
            const LaunchPlan p = plan_offsets(r.set.snapshot(), r.cus, r.width, r.count);
            CHECK(kernel_key_valid(kernel_key(p, (BatchOp)op)) == (op <= kOpUpdate || r.width == 32), "%s, op %d: valid key",
                  r.name, op);
        }
    }
    // ... and how many kernels that makes: 35 fixed CRC-32C, 21 fixed CRC-64,
    // 2 split, 15 offsets checksum / verify / update, 9 seal / pack / unpack
    {
        int n[5] = {};
        for (int width : {16, 32, 64})
            for (int lg = -1; lg <= CRC_GPU_MAX_LOG2G + 1; lg++)
                for (int mode = -1; mode <= kOffsets + 1; mode++)
                    for (int op = -1; op <= kOpUnpack + 1; op++)
                        for (int f = 0; f < 8; f++) {
                            const KernelKey k{width, lg, mode, op, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0};
                            if (kernel_key_valid(k)) n[k.split ? 2 : mode != kOffsets ? (width == 64) : op <= kOpUpdate ? 3 : 4]++;
                        }
        CHECK(n[0] == 35 && n[1] == 21 && n[2] == 2 && n[3] == 15 && n[4] == 9, "valid keys: %d %d %d %d %d", n[0], n[1], n[2],
              n[3], n[4]);
        // ... and in the other frames (MsgFrame): 6 detached, 12 RPC, none in place or past the last
        int nf[kFrameRpc + 2] = {};
        for (int frame = kFrameInPlace; frame <= kFrameRpc + 1; frame++)
            for (int width : {16, 32, 64})
                for (int lg = -1; lg <= CRC_GPU_MAX_LOG2G + 1; lg++)
                    for (int mode = -1; mode <= kOffsets + 1; mode++)
                        for (int op = -1; op <= kOpUnpack + 1; op++)
                            for (int f = 0; f < 8; f++)
                                nf[frame] += kernel_key_valid(KernelKey{width, lg, mode, op, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (MsgFrame)frame});
        CHECK(nf[kFrameInPlace] == 0 && nf[kFrameDetached] == 6 && nf[kFrameRpc] == 12 && nf[kFrameRpc + 1] == 0,
              "valid keys by frame: %d %d %d %d", nf[kFrameInPlace], nf[kFrameDetached], nf[kFrameRpc], nf[kFrameRpc + 1]);
    }
    const mck_settings_t d = D.snapshot();
    for (const auto &r : kLanes) CHECK(choose_log2g(d, r.len, r.width) == r.lg, "choose_log2g(%zu, %d) = %d", r.len, r.width, choose_log2g(d, r.len, r.width));
    for (const auto &r : kLightLanes) CHECK(light_log2g(d, r.len) == r.lg, "light_log2g(%zu) = %d", r.len, light_log2g(d, r.len));
    // the two thresholds the offsets and XDR paths share
    CHECK(kRecvQueueBatch == 1024, "kRecvQueueBatch");
    CHECK(!nt_by_count(d, 8191) && nt_by_count(d, 8192), "nt_by_count threshold");
    CHECK(nt_by_count(NT1.snapshot(), 1) && !nt_by_count(NT0.snapshot(), 1u << 20), "nt_by_count overrides");
    CHECK(!nt_by_bytes(d, (512ull << 20) - 1) && nt_by_bytes(d, 512ull << 20), "nt_by_bytes threshold");
    // C3's plan is the one tests/native/split_plan.cpp checks chunk by chunk
    {
        const LaunchPlan p = plan_fixed(d, 256, 64, A, 1u << 20, 1u << 20, 8192);
        const SplitPlan c3(8192, p.split_log2, p.grid);
        CHECK(p.split && c3.whole() && c3.n == p.units && c3.cl == 5 && c3.sl == 2, "C3 split plan");
    }
    // A plan depends on the snapshot passed in and on nothing else: two
    // snapshots, used in turn, give each its own result every time.
    {
        const mck_settings_t a = D.snapshot(), b = LG0.snapshot(), c = LIGHT0.snapshot();
        for (int turn = 0; turn < 2; turn++) {
            const LaunchPlan pa = plan_fixed(a, 256, 32, A, 4096, 4096, 65536), pb = plan_fixed(b, 256, 32, A, 4096, 4096, 65536);
            CHECK(pa.lg == 4 && pa.units == 16384 && pa.grid == 256, "plan_fixed, default snapshot: lg %d", pa.lg);
            CHECK(pb.lg == 0 && pb.units == 1024 && pb.grid == 64, "plan_fixed, gpu_log2g 0 snapshot: lg %d", pb.lg);
            const LaunchPlan oa = plan_offsets(a, 256, 32, 1024), oc = plan_offsets(c, 256, 32, 1024);
            CHECK(oa.light && !oa.dyn && oa.block == 256 && oa.grid == 256, "plan_offsets, default snapshot");
            CHECK(!oc.light && oc.dyn && oc.block == 1024 && oc.grid == 64, "plan_offsets, gpu_light 0 snapshot");
            CHECK(choose_log2g(a, 4096, 32) == 4 && choose_log2g(b, 4096, 32) == 0, "choose_log2g by snapshot");
            CHECK(light_log2g(a, 4096) == 6 && light_log2g(b, 4096) == 0, "light_log2g by snapshot");
        }
    }
    // Total: whatever gpu_log2g a snapshot holds (the parser admits 0..6; a
    // hand-made one need not), lg stays a valid pack index and shift count.
    for (int forced = -3; forced <= 40; forced++) {
        Set f = D;
        f.lg = forced;
        const mck_settings_t s = f.snapshot();
        for (int width : {32, 64})
            for (size_t len : {(size_t)0, (size_t)4096, (size_t)1 << 20})
                for (size_t count : {(size_t)0, (size_t)1, (size_t)100000}) {
                    const LaunchPlan p = plan_fixed(s, 256, width, A, len, len, count);
                    CHECK(p.lg >= 0 && p.lg <= CRC_GPU_MAX_LOG2G, "gpu_log2g %d: lg %d", forced, p.lg);
                    if (p.lg >= 0 && p.lg <= CRC_GPU_MAX_LOG2G) pack_use[p.lg]++;
                    CHECK(forced < 0 || forced > CRC_GPU_MAX_LOG2G || p.lg == forced, "gpu_log2g %d not honoured: lg %d", forced, p.lg);
                }
    }
    int used = 0;
    for (int n : pack_use) used += n > 0;
    CHECK(used == CRC_GPU_MAX_LOG2G + 1, "rows reach %d of the lane counts", used);
    printf("launch plan: %d checks, %d failures\n", checks, fails);
    return fails ? 1 : 0;
}
