// The host side of a column pool (rust-lp_amd/csrc/relp_pool.hpp: the sliced-ELL packer, the segment arithmetic of relp_pool_price,
// the stale rule, the argument checks, the chosen columns of an add) on hand-made pools.  Plain C++17, no library, no GPU; built by
// tests/cpp/Makefile once as it is and once with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "relp_pool.hpp"
#include "check.hpp"

using namespace relp;


struct Csc {
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> idx;
    std::vector<double> val, cost;
    void column(const std::vector<std::pair<int32_t, double>>& entries, double c) {
        for (const auto& e : entries) { idx.push_back(e.first); val.push_back(e.second); }
        ptr.push_back((int64_t)idx.size());
        cost.push_back(c);
    }
    PoolImage pack(int32_t m) const { return pool_pack((int32_t)cost.size(), ptr.data(), idx.data(), val.data(), cost.data(), m); }
};

// every invariant of the image against the host copy: slices of 64 lanes, entry-major, rows ascending, padding (-1, +0.0) behind
// the entries of a column and in the lanes behind the last column, nothing else stored
static void check_image(const PoolImage& im) {
    const int32_t slices = (im.count + kPoolSlice - 1) / kPoolSlice;
    CHECK(im.slices() == slices);
    CHECK((int32_t)im.ptr.size() == im.count + 1 && im.ptr[0] == 0);
    CHECK(im.slice_ptr[0] == 0 && (int64_t)im.ell_idx.size() == im.stored() && (int64_t)im.ell_val.size() == im.stored());
    int64_t held = 0;
    for (int32_t s = 0; s < slices; ++s) {
        int32_t longest = 0;
        for (int32_t k = s * kPoolSlice; k < std::min(im.count, (s + 1) * kPoolSlice); ++k) longest = std::max(longest, im.length(k));
        CHECK(im.width(s) == longest);
        CHECK((im.slice_ptr[s + 1] - im.slice_ptr[s]) % kPoolSlice == 0);
        for (int32_t lane = 0; lane < kPoolSlice; ++lane) {
            const int32_t k = s * kPoolSlice + lane;
            const int32_t len = k < im.count ? im.length(k) : 0;
            for (int32_t e = 0; e < im.width(s); ++e) {
                const int64_t at = im.slice_ptr[s] + (int64_t)e * kPoolSlice + lane;
                if (k < im.count) CHECK(at == im.at(k, e));
                if (e < len) {
                    CHECK(im.ell_idx[at] == im.idx[im.ptr[k] + e] && im.ell_val[at] == im.values[im.ptr[k] + e]);
                    CHECK(im.ell_val[at] != 0.0 && im.ell_idx[at] >= 0 && im.ell_idx[at] < im.bound);
                    if (e > 0) CHECK(im.ell_idx[at] > im.ell_idx[at - kPoolSlice]);
                    ++held;
                } else {
                    CHECK(im.ell_idx[at] == -1 && im.ell_val[at] == 0.0 && !std::signbit(im.ell_val[at]));
                }
            }
        }
    }
    CHECK(held == im.nonzeros());
}

static void test_packer() {
    {   // an empty pool
        Csc c;
        const PoolImage im = c.pack(5);
        CHECK(im.count == 0 && im.slices() == 0 && im.stored() == 0 && im.nonzeros() == 0);
        check_image(im);
        const PoolImage none = pool_pack(0, nullptr, nullptr, nullptr, nullptr, 5);
        CHECK(none.count == 0 && none.stored() == 0 && none.nonzeros() == 0);
    }
    {   // one column, the caller's rows descending, an explicit zero and a negative zero dropped
        Csc c;
        c.column({{6, 2.5}, {4, 0.0}, {3, -1.0}, {1, -0.0}, {0, 4.0}}, 7.0);
        const PoolImage im = c.pack(7);
        CHECK(im.count == 1 && im.slices() == 1 && im.width(0) == 3 && im.stored() == 3 * kPoolSlice && im.nonzeros() == 3);
        CHECK(im.idx == (std::vector<int32_t>{0, 3, 6}) && im.values == (std::vector<double>{4.0, -1.0, 2.5}));
        CHECK(im.ell_idx[0] == 0 && im.ell_idx[kPoolSlice] == 3 && im.ell_idx[2 * kPoolSlice] == 6 && im.ell_idx[1] == -1);
        CHECK(im.scalar == std::vector<double>{7.0} && im.bound == 7);
        check_image(im);
    }
    for (int32_t count : {64, 65}) {   // exactly one slice; a second slice of one column
        Csc c;
        for (int32_t k = 0; k < count; ++k) {
            std::vector<std::pair<int32_t, double>> e;
            for (int32_t x = 0; x < k % 5; ++x) e.push_back({(k + 7 * x) % 30, 1.0 + k + 0.25 * x});   // (k % 5 == 0: an empty column inside a slice)
            // distinct rows: (k + 7x) % 30 for x < 5 are distinct since 7x % 30 is
            c.column(e, -1.0 * k);
        }
        const PoolImage im = c.pack(30);
        CHECK(im.slices() == (count + 63) / 64 && im.width(0) == 4);
        if (count == 65) CHECK(im.width(1) == 4 && im.stored() == 2 * 4 * kPoolSlice);   // column 64: 64 % 5 = 4 entries
        CHECK(im.length(0) == 0 && im.length(5) == 0 && im.length(4) == 4);
        check_image(im);
    }
    {   // one column of 300 entries beside short ones: the slice is as wide as the long column, the next slice is not
        Csc c;
        for (int32_t k = 0; k < 130; ++k) {
            std::vector<std::pair<int32_t, double>> e;
            const int32_t len = k == 17 ? 300 : 1 + k % 3;
            for (int32_t x = len - 1; x >= 0; --x) e.push_back({x + (k == 17 ? 10 : k), 0.5 * (x + 1)});     // descending on purpose
            c.column(e, 1.0);
        }
        const PoolImage im = c.pack(320);
        CHECK(im.slices() == 3 && im.width(0) == 300 && im.width(1) == 3 && im.width(2) == 3);
        CHECK(im.stored() == (300 + 3 + 3) * kPoolSlice);
        check_image(im);
        // the chosen columns of an add: ids in any order, the union of their rows, the longest
        const int32_t ids[3] = {129, 17, 0};
        const PoolChoice ch = pool_choose(im, ids, 3);
        CHECK(ch.ptr == (std::vector<int64_t>{0, 1, 301, 302}) && ch.longest == 300 && ch.scalar.size() == 3);
        CHECK(ch.idx[0] == 129 && ch.idx[1] == 10 && ch.idx[300] == 309 && ch.idx[301] == 0);
        CHECK(ch.touched == 301);                       // rows 10 .. 309 (row 129 is among them) and row 0
        const int32_t one[1] = {5};
        const PoolChoice c1 = pool_choose(im, one, 1);
        CHECK(c1.touched == 3 && c1.longest == 3 && c1.values == (std::vector<double>{0.5, 1.0, 1.5}));
        CHECK(pool_choose(im, nullptr, 0).touched == 0);
    }
}

static void test_segments() {
    // segments == 1, == count, not dividing count; shares tile [0, count) in order, the last ones short or empty
    struct Case { int32_t count, segments, size; };
    for (const Case& c : {Case{257, 1, 257}, Case{257, 257, 1}, Case{65, 3, 22}, Case{10, 4, 3}, Case{10, 7, 2}, Case{1, 1, 1}, Case{5000, 2, 2500}}) {
        CHECK(pool_segment_size(c.count, c.segments) == c.size);
        int32_t covered = 0;
        for (int32_t s = 0; s < c.segments; ++s) {
            const int32_t lo = pool_segment_lo(c.count, c.segments, s), hi = pool_segment_hi(c.count, c.segments, s);
            CHECK(lo == covered && hi >= lo && hi - lo <= c.size && hi <= c.count);
            if (hi < c.count) CHECK(hi - lo == c.size);
            covered = hi;
        }
        CHECK(covered == c.count);
    }
    CHECK(pool_segment_lo(10, 7, 5) == 10 && pool_segment_hi(10, 7, 6) == 10);      // 10 over 7: shares of 2, the last two empty
    CHECK(kPoolChunk == 256 && pool_segment_chunks(5000, 2) == 10 && pool_segment_chunks(5000, 1) == 20 && pool_segment_chunks(256, 1) == 1);
    CHECK(pool_segment_chunks(257, 1) == 2 && pool_segment_chunks(7, 7) == 1 && pool_segment_chunks(0, 1) == 1);
    CHECK(pool_segment_size(INT32_MAX, 1) == INT32_MAX && pool_segment_lo(INT32_MAX, 2, 2) == INT32_MAX);
    // the total order of the winners
    CHECK(pool_better(-2.0, 9, -1.0, 3) && !pool_better(-1.0, 3, -2.0, 9));
    CHECK(pool_better(-1.0, 3, -1.0, 9) && !pool_better(-1.0, 9, -1.0, 3) && !pool_better(-1.0, 3, -1.0, 3));
    CHECK(pool_better(-1.0, 3, 0.0, -1) && !pool_better(0.0, -1, -1.0, 3) && !pool_better(0.0, -1, 0.0, -1));
    // the argument checks of relp_pool_price
    int dummy = 0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(pool_check_sweep_args(kColumnPoolWords, 10, 1, 0.0, &dummy, &dummy, &dummy).empty());
    CHECK(pool_check_sweep_args(kColumnPoolWords, 10, 10, 1e-7, &dummy, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 0, 0.0, &dummy, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 11, 0.0, &dummy, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, -1, 0.0, &dummy, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 1, -1e-9, &dummy, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 1, inf, &dummy, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 1, nan, &dummy, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 1, 0.0, nullptr, &dummy, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 1, 0.0, &dummy, nullptr, &dummy).empty());
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 10, 1, 0.0, &dummy, &dummy, nullptr).empty());
    CHECK(pool_check_sweep_args(kColumnPoolWords, 0, 3, 0.0, &dummy, &dummy, &dummy).empty());      // an empty pool: any segments >= 1
    CHECK(!pool_check_sweep_args(kColumnPoolWords, 0, 0, 0.0, &dummy, &dummy, &dummy).empty());
}

static void test_lists_and_stale_rule() {
    const int32_t fine[3] = {4, 0, 2}, twice[3] = {4, 0, 4}, outside[2] = {1, 5}, negative[1] = {-1};
    CHECK(pool_check_ids(kColumnPoolWords, fine, 3, 5).empty() && pool_check_ids(kColumnPoolWords, nullptr, 0, 5).empty() && pool_check_ids(kColumnPoolWords, fine, 0, 0).empty());
    CHECK(pool_check_ids(kColumnPoolWords, twice, 3, 5).find("twice") != std::string::npos);
    CHECK(pool_check_ids(kColumnPoolWords, outside, 2, 5).find("range") != std::string::npos);
    CHECK(!pool_check_ids(kColumnPoolWords, negative, 1, 5).empty() && !pool_check_ids(kColumnPoolWords, nullptr, 2, 5).empty() && !pool_check_ids(kColumnPoolWords, fine, -1, 5).empty());
    CHECK(!pool_check_ids(kColumnPoolWords, fine, 3, 4).empty());
    // a pool created over 30 rows; cuts came later as rows 30, 31, 32
    const int32_t later[2] = {32, 30}, mixed[2] = {31, 29}, first[1] = {0};
    CHECK(!pool_stale_after_removal(30, later, 2));
    CHECK(pool_stale_after_removal(30, mixed, 2));
    CHECK(pool_stale_after_removal(30, first, 1));
    CHECK(!pool_stale_after_removal(30, nullptr, 0));
    CHECK(pool_stale_after_removal(31, later, 2));     // created after the first cut: that cut's row is the pool's
    // a trial added the cut row 30 and is rolled back to 30 rows: a pool created inside it over 31 rows loses its last row
    CHECK(pool_stale_after_rollback(31, 30) && !pool_stale_after_rollback(30, 30) && !pool_stale_after_rollback(30, 31));
}

int main() {
    test_packer();
    test_segments();
    test_lists_and_stale_rule();
    return finish("test_pool");
}
