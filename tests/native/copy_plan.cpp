// Host check of the copy kernels' key (copy_plan.h): which of the 10 copy
// kernels an offsets plan leads to for mchecksum_gpu_copy_offsets and
// mchecksum_gpu_update_copy_offsets, on both sides of the plan's thresholds and
// under its override settings, and that copy_key_valid states exactly those 10.
// The plan itself is plan_offsets (tests/native/launch_plan.cpp pins it): here
// every key is also compared with the batch kernel the same plan gives
// checksum_offsets / update_offsets.  Plain C++: no HIP header.
#include "copy_plan.h"

#include <cstdio>
#include <initializer_list>

using namespace mck;

static int fails = 0, checks = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        checks++;                             \
        if (!(c)) {                           \
            if (fails++ < 20) {               \
                printf("FAIL: " __VA_ARGS__); \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

static mck_settings_t snapshot(int light, int nt) {
    mck_settings_t s{};
    s.gpu_log2g = -1, s.gpu_light = light, s.gpu_nt = nt, s.gpu_split = -1;
    s.gpu_split_lds = 1, s.gpu_force_generic = 0, s.gpu_xdr_fast = -1;
    return s;
}

struct Row {
    const char *name;
    int light_set, nt_set;  // MCHECKSUM_GPU_LIGHT, MCHECKSUM_GPU_NT (-1: not set)
    int width;
    size_t count;
    bool nt, light;  // expected
};
static const Row kRows[] = {
    {"1024 chunks crc32c: light", -1, -1, 32, 1024, false, true},
    {"1025 chunks crc32c: full", -1, -1, 32, 1025, false, false},
    {"8191 chunks crc32c: full", -1, -1, 32, 8191, false, false},
    {"8192 chunks crc32c: non-temporal", -1, -1, 32, 8192, true, false},
    {"1024 chunks crc64: full (no light form)", -1, -1, 64, 1024, false, false},
    {"1025 chunks crc64: full", -1, -1, 64, 1025, false, false},
    {"8191 chunks crc64: full", -1, -1, 64, 8191, false, false},
    {"8192 chunks crc64: non-temporal", -1, -1, 64, 8192, true, false},
    {"1 chunk crc32c: light", -1, -1, 32, 1, false, true},
    {"1 chunk crc64: full", -1, -1, 64, 1, false, false},
    // MCHECKSUM_GPU_LIGHT
    {"LIGHT=0, 1024 chunks crc32c: full", 0, -1, 32, 1024, false, false},
    {"LIGHT=0, 1 chunk crc32c: full", 0, -1, 32, 1, false, false},
    {"LIGHT=1, 1025 chunks crc32c: light", 1, -1, 32, 1025, false, true},
    {"LIGHT=1, 8192 chunks crc32c: light, so not non-temporal", 1, -1, 32, 8192, false, true},
    {"LIGHT=1, 1024 chunks crc64: full", 1, -1, 64, 1024, false, false},
    {"LIGHT=1, 8192 chunks crc64: non-temporal", 1, -1, 64, 8192, true, false},
    // MCHECKSUM_GPU_NT
    {"NT=1, 1025 chunks crc32c: non-temporal", -1, 1, 32, 1025, true, false},
    {"NT=1, 1024 chunks crc32c: light, so not non-temporal", -1, 1, 32, 1024, false, true},
    {"NT=1, 1 chunk crc64: non-temporal", -1, 1, 64, 1, true, false},
    {"NT=0, 8192 chunks crc32c: full", -1, 0, 32, 8192, false, false},
    {"NT=0, 8192 chunks crc64: full", -1, 0, 64, 8192, false, false},
    {"LIGHT=0 NT=1, 1 chunk crc32c: non-temporal", 0, 1, 32, 1, true, false},
};

int main() {
    for (const Row &r : kRows) {
        const mck_settings_t s = snapshot(r.light_set, r.nt_set);
        const LaunchPlan p = plan_offsets(s, 256, r.width, r.count);
        for (int op : {(int)kCopyChecksum, (int)kCopyUpdate}) {
            const CopyKey k = copy_key(p, (CopyOp)op);
            CHECK((k == CopyKey{r.width, op, r.nt, r.light}), "%s, op %d: key {%d, %d, nt %d, light %d}", r.name, op, k.width,
                  k.op, k.nt, k.light);
            CHECK(copy_key_valid(k), "%s, op %d: no such kernel", r.name, op);
            // ... the layout of the batch kernel the same plan gives the call without the copy
            const KernelKey b = kernel_key(p, op == kCopyUpdate ? kOpUpdate : kOpChecksum);
            CHECK(b.nt == k.nt && b.light == k.light && b.width == k.width, "%s, op %d: differs from the batch kernel's key",
                  r.name, op);
        }
    }

    // copy_key_valid over the whole key space: exactly the 10 kernels
    int valid = 0, valid32 = 0, valid64 = 0;
    for (int width : {0, 16, 32, 64, 128})
        for (int op = -1; op <= 3; op++)
            for (int nt = 0; nt < 2; nt++)
                for (int light = 0; light < 2; light++) {
                    const bool v = copy_key_valid(CopyKey{width, op, nt != 0, light != 0});
                    const bool want = (width == 32 || width == 64) && (op == kCopyChecksum || op == kCopyUpdate) &&
                                      !(light && (width == 64 || nt));
                    CHECK(v == want, "copy_key_valid{%d, %d, nt %d, light %d} = %d", width, op, nt, light, (int)v);
                    valid += v;
                    valid32 += v && width == 32;
                    valid64 += v && width == 64;
                }
    CHECK(valid == 10 && valid32 == 6 && valid64 == 4, "%d valid keys (%d CRC-32C, %d CRC-64)", valid, valid32, valid64);
    CHECK(!copy_key_valid(CopyKey{64, kCopyChecksum, false, true}), "light CRC-64");
    CHECK(!copy_key_valid(CopyKey{64, kCopyUpdate, false, true}), "light CRC-64 update");
    CHECK(!copy_key_valid(CopyKey{32, kCopyChecksum, true, true}), "light with nt");
    CHECK(!copy_key_valid(CopyKey{16, kCopyChecksum, false, false}), "unknown width");
    CHECK(!copy_key_valid(CopyKey{32, kCopyUpdate + 1, false, false}), "unknown op");
    CHECK(!copy_key_valid(CopyKey{32, -1, false, false}), "negative op");
    static_assert(copy_key_valid(CopyKey{32, kCopyUpdate, false, true}) && copy_key_valid(CopyKey{64, kCopyUpdate, true, false}),
                  "constexpr: the kernels assert their keys with it");

    printf("%d checks, %d failures\n", checks, fails);
    return fails ? 1 : 0;
}
