// The message calls' host-compilable rules (mercury_amd/csrc/seg_plan.h:
// seg_msg_layout, seg_msg_fits, seg_msg_gate, seg_msg_seal_decide,
// seg_msg_open_decide) walked over random tables against a naive model that
// knows nothing of prefix sums: which messages fit, where each object's
// accumulator word and gate byte lie in the workspace, and what the launch
// after the chunk pass stores, flags and counts.  Stand-alone: plain and
// under the sanitizers (tests/test_segmsg_plan.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "seg_plan.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            if (g_fail++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                               \
    } while (0)

struct Counts {
    uint64_t tables = 0, msgs = 0, fit = 0, misfit = 0, no_seg = 0, all_empty = 0, long1 = 0, short1 = 0, runt = 0;
};

// the fit rule as the contract words it: sizes added up one by one
bool naive_fits(const std::vector<uint64_t> &len, uint64_t f0, uint64_t f1, uint64_t m0, uint64_t m1, uint64_t pay) {
    if (m1 < m0) return false;
    const uint64_t size = m1 - m0;
    if (size < pay) return false;
    uint64_t n = 0;
    for (uint64_t s = f0; s < f1; s++) n += len[s];
    return size == pay + n;
}

void layout_checks() {
    const uint64_t nsegs[] = {0, 1, 3, 1023, 1024, 1025, 70000};
    const uint64_t nobjs[] = {0, 1, 2, 7, 8, 9, 4097};
    for (uint64_t nseg : nsegs)
        for (uint64_t nobj : nobjs) {
            mck::SegMsgLayout m{};
            CHECK(mck::seg_msg_layout(nseg, nobj, &m));
            const uint64_t base = mck::seg_work_layout(nseg).bytes;
            // the scan's workspace is untouched, the regions follow it in order,
            // 8-byte aligned, and each object's slots are inside them
            CHECK(8 * m.acc >= base && 8 * m.acc < base + 8);
            CHECK(8 * m.gate >= 8 * m.acc + 4 * nobj);
            CHECK(m.bytes >= 8 * m.gate + nobj);
            CHECK(m.bytes % 8 == 0);
            CHECK(m.bytes == mck::seg_msg_work_bytes(nseg, nobj));
            CHECK(m.bytes >= mck::seg_work_bytes(nseg));
            // a model workspace: write every object's slots, nothing else moves
            if (nseg <= 1025) {
                std::vector<uint8_t> w(m.bytes + 16, 0xEE);
                uint32_t *acc = reinterpret_cast<uint32_t *>(w.data() + 8 * m.acc);
                uint8_t *gate = w.data() + 8 * m.gate;
                for (uint64_t j = 0; j < nobj; j++) {
                    acc[j] = 0;
                    gate[j] = 1;
                }
                for (uint64_t i = 0; i < base; i++) CHECK(w[i] == 0xEE);
                for (uint64_t i = m.bytes; i < w.size(); i++) CHECK(w[i] == 0xEE);
                for (uint64_t j = 0; j < nobj; j++) CHECK(acc[j] == 0 && gate[j] == 1);
            }
        }
    // monotonic in both arguments
    size_t prev = 0;
    for (uint64_t n = 0; n < 5000; n += 37) {
        const size_t b = mck::seg_msg_work_bytes(n, 100);
        CHECK(b >= prev);
        prev = b;
    }
    prev = 0;
    for (uint64_t n = 0; n < 5000; n += 37) {
        const size_t b = mck::seg_msg_work_bytes(100, n);
        CHECK(b >= prev);
        prev = b;
    }
    // the caps: 2^31 objects and 2^32 - 1 segments are the last sizes taken
    mck::SegMsgLayout m{};
    CHECK(mck::seg_msg_layout(10, 1ull << 31, &m));
    CHECK(!mck::seg_msg_layout(10, (1ull << 31) + 1, &m));
    CHECK(mck::seg_msg_layout((1ull << 32) - 1, 10, &m));
    CHECK(!mck::seg_msg_layout(1ull << 32, 10, &m));
    CHECK(mck::seg_msg_work_bytes(1ull << 32, 10) == SIZE_MAX);
    CHECK(mck::seg_msg_work_bytes(10, (1ull << 31) + 1) == SIZE_MAX);
}

void walk(std::mt19937_64 &rng, Counts *cn) {
    auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    const uint64_t lens_of[] = {0, 0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 1000, 4103, 300000};
    const uint64_t pays[] = {4, 9, 20, 64};
    const uint64_t nobj = 1 + pick(40), pay = pays[pick(4)];
    const uint64_t lead = pick(3), trail = pick(3);  // segments outside every object
    std::vector<uint64_t> len, first;
    for (uint64_t i = 0; i < lead; i++) len.push_back(lens_of[pick(16)]);
    first.push_back(len.size());
    std::vector<int> kind(nobj);  // 0 fits, 1 one byte long, 2 one byte short, 3 shorter than the headers, 4 far off
    for (uint64_t j = 0; j < nobj; j++) {
        const uint64_t shape = pick(8);
        const uint64_t k = shape == 0 ? 0 : 1 + pick(6);  // no segments at all
        for (uint64_t i = 0; i < k; i++) len.push_back(shape == 1 ? 0 : lens_of[pick(16)]);  // all empty
        first.push_back(len.size());
        kind[j] = pick(3) ? 0 : 1 + (int)pick(4);
    }
    for (uint64_t i = 0; i < trail; i++) len.push_back(lens_of[pick(16)]);
    const uint64_t nseg = len.size();
    std::vector<uint64_t> P(nseg + 1, 0);  // what the scan leaves
    for (uint64_t s = 0; s < nseg; s++) P[s + 1] = P[s] + len[s];
    // the message table: arbitrary start, sizes by kind
    std::vector<uint64_t> off(nobj + 1);
    off[0] = pick(100);
    for (uint64_t j = 0; j < nobj; j++) {
        const uint64_t n = P[first[j + 1]] - P[first[j]];
        uint64_t size = pay + n;
        if (kind[j] == 1) size += 1;
        if (kind[j] == 2) size -= 1;  // (pay >= 4: never wraps; may fall below pay when n == 0)
        if (kind[j] == 3) size = pick(pay);
        if (kind[j] == 4) size += 2 + pick(5000);
        off[j + 1] = off[j] + size;
    }
    mck::SegMsgLayout ml{};
    CHECK(mck::seg_msg_layout(nseg, nobj, &ml));
    std::vector<uint8_t> work(ml.bytes, 0xEE);
    uint32_t *acc = reinterpret_cast<uint32_t *>(work.data() + 8 * ml.acc);
    uint8_t *gate = work.data() + 8 * ml.gate;
    // the launch ahead of the chunk pass
    for (uint64_t j = 0; j < nobj; j++) {
        const uint64_t f0 = first[j], f1 = first[j + 1];
        const bool ok = mck::seg_msg_range_ok(f0, f1, nseg);
        CHECK(ok);
        acc[j] = 0;
        gate[j] = mck::seg_msg_gate(ok, ok ? P[f0] : 0, ok ? P[f1] : 0, off[j], off[j + 1], pay);
    }
    cn->tables++;
    std::vector<uint8_t> st_pack(nobj, 0xAA), st_open(nobj, 0xAA), st_fault(nobj, 0xAA);
    uint32_t nbad = 0, nbad_fault = 0, expect_bad = 0;
    for (uint64_t j = 0; j < nobj; j++) {
        const uint64_t f0 = first[j], f1 = first[j + 1];
        const bool fits = naive_fits(len, f0, f1, off[j], off[j + 1], pay);
        CHECK((gate[j] == 0) == fits);
        CHECK(fits == (kind[j] == 0));
        CHECK(mck::seg_msg_fits(off[j], off[j + 1], pay, P[f1] - P[f0]) == fits);
        cn->msgs++;
        (fits ? cn->fit : cn->misfit)++;
        bool all_empty = f1 > f0;
        for (uint64_t s = f0; s < f1; s++) all_empty = all_empty && len[s] == 0;
        if (f0 == f1) cn->no_seg++;
        if (all_empty) cn->all_empty++;
        if (kind[j] == 1) cn->long1++;
        if (kind[j] == 2) cn->short1++;
        if (off[j + 1] - off[j] < pay) cn->runt++;
        // an object without bytes fits exactly a message of its headers
        if (P[f1] == P[f0]) CHECK(fits == (off[j + 1] - off[j] == pay));
        // after the pass: pack seals fitting messages only, never after a fault
        const uint32_t value = (uint32_t)rng(), same = value, other = value ^ (1u << pick(32));
        CHECK(mck::seg_msg_seal_decide(false, gate[j], st_pack.data(), j) == fits);
        CHECK(st_pack[j] == (fits ? 0 : 1));
        CHECK(!mck::seg_msg_seal_decide(true, gate[j], st_fault.data(), j) && st_fault[j] == 1);
        CHECK(!mck::seg_msg_seal_decide(true, gate[j], nullptr, j));
        // unpack: the header is read only for a fitting message of a sound call
        CHECK(mck::seg_msg_compares(false, gate[j]) == fits && !mck::seg_msg_compares(true, gate[j]));
        const bool corrupt = pick(4) == 0;
        const uint32_t b = mck::seg_msg_open_decide(false, gate[j], value, corrupt ? other : same, st_open.data(), j);
        CHECK(b == ((!fits || corrupt) ? 1u : 0u) && st_open[j] == b);
        CHECK(mck::seg_msg_open_decide(false, gate[j], value, corrupt ? other : same, nullptr, j) == b);
        nbad += b;
        expect_bad += (!fits || corrupt) ? 1 : 0;
        nbad_fault += mck::seg_msg_open_decide(true, gate[j], value, same, st_fault.data(), j);
        CHECK(st_fault[j] == 1);
    }
    CHECK(nbad == expect_bad);
    CHECK(nbad_fault == nobj);  // a faulted call adds nobj
    // nothing but the objects' slots was written
    for (uint64_t i = 0; i < 8 * ml.acc; i++) CHECK(work[i] == 0xEE);
    // tables that run backwards never fit, whatever the sizes
    CHECK(!mck::seg_msg_fits(100, 99, 0, 0));
    CHECK(mck::seg_msg_gate(false, 0, 0, 0, pay, pay) == 1);
    CHECK(mck::seg_msg_gate(true, 5, 4, 0, pay, pay) == 1);
    CHECK(!mck::seg_msg_range_ok(3, 2, 10) && !mck::seg_msg_range_ok(3, 11, 10) && mck::seg_msg_range_ok(10, 10, 10));
}

}  // namespace

int main() {
    std::mt19937_64 rng(20260101);
    Counts cn;
    layout_checks();
    for (int t = 0; t < 3000; t++) walk(rng, &cn);
    std::printf("%llu tables, %llu messages: %llu fit, %llu do not; %llu without segments, %llu all empty, "
                "%llu one byte long, %llu one byte short, %llu shorter than the headers\n",
                (unsigned long long)cn.tables, (unsigned long long)cn.msgs, (unsigned long long)cn.fit,
                (unsigned long long)cn.misfit, (unsigned long long)cn.no_seg, (unsigned long long)cn.all_empty,
                (unsigned long long)cn.long1, (unsigned long long)cn.short1, (unsigned long long)cn.runt);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
