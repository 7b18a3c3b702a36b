/*
 * seg_verify.cpp -- what mchecksum_gpu_verify_segments decides and where it
 * keeps its values (seg_plan.h: seg_call_faulted, seg_verify_decide,
 * seg_verify_layout), on the CPU.  The compare kernel is this loop: the fault
 * state once, then one decision per object, the sum added where there is a
 * counter.  Stand-alone, so that the sanitizers see its loads and stores.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "seg_plan.h"

static int fails = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                            \
        }                                                       \
    } while (0)

// the compare kernel's walk over nobj objects
static void compare(uint64_t scan_claim, uint64_t chunk_claim, uint64_t key, const std::vector<uint64_t> &value,
                    const std::vector<uint64_t> &expected, uint8_t *status, uint32_t *counter) {
    const bool faulted = mck::seg_call_faulted(scan_claim, chunk_claim, key);
    uint32_t nbad = 0;
    for (uint64_t j = 0; j < value.size(); j++) nbad += mck::seg_verify_decide(faulted, value[j], expected[j], status, j);
    if (counter && nbad) *counter += nbad;
}

int main() {
    const uint64_t key = 0x1234567890ABCDEFull, other = key ^ 1;
    const std::vector<uint64_t> want = {5, 0, ~0ull, 0xFFFFFFFFull, 77};
    const size_t n = want.size();

    // the fault state: either stage's claim holding the call's key
    CHECK(!mck::seg_call_faulted(other, other, key));
    CHECK(!mck::seg_call_faulted(0, 0, key));
    CHECK(mck::seg_call_faulted(key, other, key));
    CHECK(mck::seg_call_faulted(other, key, key));
    CHECK(mck::seg_call_faulted(key, key, key));

    // clean run, every value equal: status 0, no count (the counter is added to, not set)
    {
        std::vector<uint8_t> st(n, 9);
        uint32_t ctr = 40;
        compare(other, other, key, want, want, st.data(), &ctr);
        for (size_t j = 0; j < n; j++) CHECK(st[j] == 0);
        CHECK(ctr == 40);
    }
    // clean run, values 1 and 3 differ (one bit each): exactly those, one count each
    {
        std::vector<uint64_t> got = want;
        got[1] ^= 1ull << 63;
        got[3] ^= 1;
        std::vector<uint8_t> st(n, 9);
        uint32_t ctr = 3;
        compare(other, other, key, got, want, st.data(), &ctr);
        for (size_t j = 0; j < n; j++) CHECK(st[j] == (j == 1 || j == 3 ? 1 : 0));
        CHECK(ctr == 5);
    }
    // any fault state: every object flagged and nobj counted, whatever the values hold
    for (int which = 0; which < 3; which++) {
        const uint64_t sc = which != 1 ? key : other, cc = which != 0 ? key : other;
        for (int equal = 0; equal < 2; equal++) {
            std::vector<uint64_t> got = want;
            if (!equal) got[2] = 1;
            std::vector<uint8_t> st(n, 0);  // a stale "verified" everywhere
            uint32_t ctr = 7;
            compare(sc, cc, key, got, want, st.data(), &ctr);
            for (size_t j = 0; j < n; j++) CHECK(st[j] == 1);
            CHECK(ctr == 7 + n);
        }
    }
    // no status array, no counter, neither: tolerated, and the other still right
    {
        std::vector<uint64_t> got = want;
        got[4] = 0;
        uint32_t ctr = 0;
        compare(other, other, key, got, want, nullptr, &ctr);
        CHECK(ctr == 1);
        std::vector<uint8_t> st(n, 9);
        compare(other, other, key, got, want, st.data(), nullptr);
        CHECK(st[4] == 1 && st[0] == 0);
        compare(key, other, key, got, want, nullptr, nullptr);
        ctr = 0;
        compare(key, other, key, got, want, nullptr, &ctr);
        CHECK(ctr == n);
    }
    // no objects: nothing written
    {
        uint32_t ctr = 2;
        compare(key, key, key, {}, {}, nullptr, &ctr);
        CHECK(ctr == 2);
    }

    // where the values live: nseg words at the end of the map's region, 8-byte
    // aligned, behind the map entries left to the call, inside the workspace
    for (uint64_t nseg : {0ull, 1ull, 2ull, 12ull, 1023ull, 1024ull, 1025ull, 100000ull, (1ull << 32) - 1}) {
        mck::SegVerifyLayout v{};
        CHECK(mck::seg_verify_layout(nseg, &v));
        const mck::SegWorkLayout w = mck::seg_work_layout(nseg);
        CHECK(v.map_cap == 2 * nseg + 65536 && v.map_cap <= w.map_cap);
        CHECK(8 * v.acc == 8 * w.map + 4 * v.map_cap);           // right behind the call's map entries
        CHECK(8 * (v.acc + nseg) == w.bytes);                     // and up to the workspace's end
        CHECK(w.bytes == mck::seg_work_bytes(nseg));              // whose size has not moved
        CHECK(v.chunk_claim == w.spare && v.chunk_claim != w.fault_claim && v.chunk_claim != w.gen);
    }
    for (uint64_t nseg : {uint64_t(1) << 32, (uint64_t(1) << 32) + 5, uint64_t(mck::kMaxSegs)}) {
        mck::SegVerifyLayout v{};
        CHECK(!mck::seg_verify_layout(nseg, &v));  // no map to take the words from: the call refuses
    }
    if (fails) return 1;
    std::printf("segment verify decisions: all checks passed\n");
    return 0;
}
