// test_trial.cpp -- the planner of the trial snapshot without a GPU (rust-lp_amd/csrc/relp_trial.hpp: plain C++17, no HIP).
// `make -C tests/cpp`; exit code 0 = all checks passed.  The Makefile builds it a second time with
// -fsanitize=address,undefined (test_trial_asan): it has its own main and needs no preload.
//
// Pins, for 0, 1 and 32 segments with the byte counts 0, 1, 15, 16 and 17 (and 4,099):
//   * every offset in the snapshot buffer is 16-byte aligned, the segments do not overlap and keep the order they were named in;
//   * buffer_bytes is a multiple of 16 that holds them all, payload_bytes is the sum of the lengths;
//   * unit_end is the prefix sum of bytes / 16 (a segment below 16 bytes owns no unit: it is all tail), the same in both directions;
//   * save is live -> buffer and restore is buffer -> live, segment for segment;
//   * a 33rd segment, a negative length and a misaligned address are refused and leave the plan as it was;
//   * the copy the kernel makes from such a table (modelled here byte for byte: units, then tails) moves exactly the named bytes.
#include "relp_trial.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

#include "check.hpp"

using namespace relp;


// what k_tab_trial_copy does with a table: the whole units of every segment, then each tail
static void model_copy(const TrialTable& t) {
    const int64_t total = t.count > 0 ? t.unit_end[t.count - 1] : 0;
    for (int64_t u = 0; u < total; ++u) {
        int64_t begin = 0;
        for (int32_t s = 0; s < t.count; ++s) {
            if (u >= begin && u < t.unit_end[s])
                std::memcpy(static_cast<char*>(t.seg[s].dst) + (u - begin) * kTrialUnit, static_cast<const char*>(t.seg[s].src) + (u - begin) * kTrialUnit, kTrialUnit);
            begin = t.unit_end[s];
        }
    }
    for (int32_t s = 0; s < t.count; ++s) {
        const int64_t whole = t.seg[s].bytes / kTrialUnit * kTrialUnit;
        for (int64_t x = whole; x < t.seg[s].bytes; ++x) static_cast<char*>(t.seg[s].dst)[x] = static_cast<const char*>(t.seg[s].src)[x];
    }
}

static void check_plan(const std::vector<int64_t>& lengths) {
    const int32_t n = (int32_t)lengths.size();
    // the live arrays: one arena, every array at a 16-byte-aligned offset with 16 bytes of canary between neighbours
    int64_t arena_bytes = 16;
    std::vector<int64_t> at(n);
    for (int32_t s = 0; s < n; ++s) { at[s] = arena_bytes; arena_bytes += (lengths[s] + 15) / 16 * 16 + 16; }
    alignas(16) static char arena[1 << 18];
    alignas(16) static char buffer[1 << 18];
    CHECK(arena_bytes <= (int64_t)sizeof arena);
    for (int64_t x = 0; x < arena_bytes; ++x) arena[x] = (char)(x * 7 + 3);
    TrialPlan plan;
    for (int32_t s = 0; s < n; ++s) CHECK(plan.add(arena + at[s], lengths[s]));
    CHECK(plan.count() == n);
    int64_t payload = 0, units = 0, end_prev = 0;
    for (int32_t s = 0; s < n; ++s) {
        CHECK(plan.offset(s) % 16 == 0);
        CHECK(plan.offset(s) >= end_prev);                         // no overlap, the order kept
        CHECK(plan.bytes(s) == lengths[s] && plan.live(s) == arena + at[s]);
        end_prev = plan.offset(s) + lengths[s];
        payload += lengths[s];
    }
    CHECK(plan.buffer_bytes() % 16 == 0 && plan.buffer_bytes() >= end_prev && plan.buffer_bytes() < end_prev + 16);
    CHECK(plan.payload_bytes() == payload);
    CHECK(plan.buffer_bytes() + 16 <= (int64_t)sizeof buffer);
    std::memset(buffer, 0x5A, sizeof buffer);
    const TrialTable save = plan.table(buffer, true), back = plan.table(buffer, false);
    CHECK(save.count == n && back.count == n);
    for (int32_t s = 0; s < kTrialMaxSegments; ++s) {
        if (s < n) {
            units += lengths[s] / 16;
            CHECK(save.seg[s].src == arena + at[s] && save.seg[s].dst == buffer + plan.offset(s) && save.seg[s].bytes == lengths[s]);
            CHECK(back.seg[s].dst == arena + at[s] && back.seg[s].src == buffer + plan.offset(s) && back.seg[s].bytes == lengths[s]);
        } else {
            CHECK(save.seg[s].bytes == 0 && save.seg[s].src == nullptr && save.seg[s].dst == nullptr);
        }
        CHECK(save.unit_end[s] == units && back.unit_end[s] == units);
    }
    // forward, scramble the live arrays, back: the named bytes return, the canaries between them and the bytes of the buffer that
    // belong to no segment are never written
    std::vector<char> before(arena, arena + arena_bytes);
    model_copy(save);
    for (int32_t s = 0; s < n; ++s) {
        CHECK(std::memcmp(buffer + plan.offset(s), arena + at[s], (size_t)lengths[s]) == 0);
        for (int64_t x = plan.offset(s) + lengths[s]; x < (s + 1 < n ? plan.offset(s + 1) : plan.buffer_bytes() + 16); ++x) CHECK(buffer[x] == 0x5A);
        for (int64_t x = 0; x < lengths[s]; ++x) arena[at[s] + x] ^= (char)0xFF;
    }
    model_copy(back);
    CHECK(std::memcmp(arena, before.data(), (size_t)arena_bytes) == 0);
}

int main() {
    check_plan({});
    for (int64_t len : {0, 1, 15, 16, 17, 4099}) check_plan({len});
    {
        std::vector<int64_t> lengths;
        const int64_t pool[] = {0, 1, 15, 16, 17, 4099, 7, 8, 32, 33};
        for (int32_t s = 0; s < kTrialMaxSegments; ++s) lengths.push_back(pool[s % 10]);
        check_plan(lengths);
        check_plan(std::vector<int64_t>(kTrialMaxSegments, 0));
        check_plan(std::vector<int64_t>(kTrialMaxSegments, 17));
    }
    {   // refusals leave the plan as it was
        alignas(16) static char room[64 * 40];
        TrialPlan plan;
        CHECK(!plan.add(room + 8, 16) && !plan.add(room + 1, 1) && !plan.add(room, -1));
        CHECK(plan.count() == 0 && plan.buffer_bytes() == 0);
        for (int32_t s = 0; s < kTrialMaxSegments; ++s) CHECK(plan.add(room + 64 * s, 17));
        const int64_t bytes = plan.buffer_bytes();
        CHECK(bytes == 32 * kTrialMaxSegments);
        CHECK(!plan.add(room + 64 * 32, 16));                      // the 33rd
        CHECK(plan.count() == kTrialMaxSegments && plan.buffer_bytes() == bytes && plan.payload_bytes() == 17 * kTrialMaxSegments);
        CHECK(plan.add(nullptr, 0) == false);                      // (still full)
        TrialPlan empty;
        CHECK(empty.add(nullptr, 0) && empty.count() == 1 && empty.buffer_bytes() == 0);   // an array this engine does not have
    }
    return finish("test_trial");
}
