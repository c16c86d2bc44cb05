// The host side of a cut pool (rust-lp_amd/csrc/relp_cutpool.hpp: the adapter onto the sliced-ELL packer of the column pool, the
// norms, the segment arithmetic of relp_cutpool_separate, the key, the argument checks, the chosen cuts of an add) on hand-made
// pools.  Plain C++17, no library, no GPU; built by tests/cpp/Makefile once as it is and once with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "relp_cutpool.hpp"
#include "check.hpp"

using namespace relp;


struct Csr {
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> idx;
    std::vector<double> val, rhs;
    void cut(const std::vector<std::pair<int32_t, double>>& entries, double beta) {
        for (const auto& e : entries) { idx.push_back(e.first); val.push_back(e.second); }
        ptr.push_back((int64_t)idx.size());
        rhs.push_back(beta);
    }
    CutPoolImage pack(int32_t nr_normal) const { return cutpool_pack((int32_t)rhs.size(), ptr.data(), idx.data(), val.data(), rhs.data(), nr_normal); }
};

// every invariant of the image against the host copy: slices of 64 lanes, entry-major, columns ascending inside a cut, padding
// (-1, +0.0) behind the entries of a cut and in the lanes behind the last cut, nothing else stored; the norms
static void check_image(const CutPoolImage& cim, int32_t nr_normal) {
    const PoolImage& im = cim.ell;
    const int32_t slices = (im.count + kPoolSlice - 1) / kPoolSlice;
    CHECK(cim.ell.count == im.count && im.slices() == slices && (int32_t)cim.norm.size() == im.count && (int32_t)im.scalar.size() == im.count);
    CHECK((int32_t)im.ptr.size() == im.count + 1 && im.ptr[0] == 0 && im.slice_ptr[0] == 0);
    CHECK((int64_t)im.ell_idx.size() == im.stored() && (int64_t)im.ell_val.size() == im.stored());
    int64_t held = 0;
    for (int32_t s = 0; s < slices; ++s) {
        int32_t longest = 0;
        for (int32_t k = s * kPoolSlice; k < std::min(im.count, (s + 1) * kPoolSlice); ++k) longest = std::max(longest, im.length(k));
        CHECK(im.width(s) == longest);
        for (int32_t lane = 0; lane < kPoolSlice; ++lane) {
            const int32_t k = s * kPoolSlice + lane;
            const int32_t len = k < im.count ? im.length(k) : 0;
            for (int32_t e = 0; e < im.width(s); ++e) {
                const int64_t at = im.slice_ptr[s] + (int64_t)e * kPoolSlice + lane;
                if (e < len) {
                    CHECK(im.ell_idx[at] == im.idx[im.ptr[k] + e] && im.ell_val[at] == im.values[im.ptr[k] + e]);
                    CHECK(im.ell_val[at] != 0.0 && im.ell_idx[at] >= 0 && im.ell_idx[at] < nr_normal);
                    if (e > 0) CHECK(im.ell_idx[at] > im.ell_idx[at - kPoolSlice]);
                    ++held;
                } else {
                    CHECK(im.ell_idx[at] == -1 && im.ell_val[at] == 0.0 && !std::signbit(im.ell_val[at]));
                }
            }
        }
    }
    CHECK(held == im.nonzeros());
    for (int32_t k = 0; k < im.count; ++k) {
        double acc = 0.0;
        for (int64_t e = im.ptr[k]; e < im.ptr[k + 1]; ++e) acc = std::fma(im.values[e], im.values[e], acc);
        CHECK(cim.norm[k] == std::sqrt(acc));
    }
}

static void test_packer_and_norms() {
    {   // an empty pool
        Csr c;
        const CutPoolImage im = c.pack(5);
        CHECK(im.ell.count == 0 && im.ell.slices() == 0 && im.ell.stored() == 0 && im.ell.nonzeros() == 0 && im.norm.empty());
        check_image(im, 5);
        CHECK(cutpool_pack(0, nullptr, nullptr, nullptr, nullptr, 5).ell.count == 0);
    }
    {   // one cut, the caller's columns descending, an explicit zero and a negative zero dropped; a cut without entries
        Csr c;
        c.cut({{6, 3.0}, {4, 0.0}, {3, -4.0}, {1, -0.0}, {0, 12.0}}, 7.0);
        c.cut({}, -2.0);
        c.cut({{2, 0.0}}, 1.0);
        const CutPoolImage im = c.pack(7);
        CHECK(im.ell.count == 3 && im.ell.slices() == 1 && im.ell.width(0) == 3 && im.ell.stored() == 3 * kPoolSlice && im.ell.nonzeros() == 3);
        CHECK(im.ell.idx == (std::vector<int32_t>{0, 3, 6}) && im.ell.values == (std::vector<double>{12.0, -4.0, 3.0}));
        CHECK(im.ell.scalar == (std::vector<double>{7.0, -2.0, 1.0}));
        CHECK(im.norm[0] == 13.0 && im.norm[1] == 0.0 && !std::signbit(im.norm[1]) && im.norm[2] == 0.0);
        CHECK(im.ell.ell_idx[0] == 0 && im.ell.ell_idx[kPoolSlice] == 3 && im.ell.ell_idx[2 * kPoolSlice] == 6 && im.ell.ell_idx[1] == -1);
        check_image(im, 7);
    }
    {   // the norm is one fma chain in ascending column order, not a sum of rounded squares
        Csr c;
        const double a = 1.0 + std::ldexp(1.0, -30), b = std::ldexp(1.0, -40);
        c.cut({{5, b}, {1, a}}, 0.0);
        const CutPoolImage im = c.pack(6);
        CHECK(im.norm[0] == std::sqrt(std::fma(b, b, std::fma(a, a, 0.0))));
        CHECK(cutpool_norm(nullptr, 0) == 0.0);
    }
    for (int32_t count : {1, 63, 64, 65, 257}) {   // slice edges
        Csr c;
        for (int32_t k = 0; k < count; ++k) {
            std::vector<std::pair<int32_t, double>> e;
            for (int32_t x = 0; x < k % 5; ++x) e.push_back({(k + 7 * x) % 30, 1.0 + k + 0.25 * x});   // (k % 5 == 0: a cut without entries)
            c.cut(e, -1.0 * k);
        }
        const CutPoolImage im = c.pack(30);
        CHECK(im.ell.slices() == (count + 63) / 64);
        check_image(im, 30);
    }
    {   // one cut of 300 entries beside short ones: the slice is as wide as the long cut, the next slice is not
        Csr c;
        for (int32_t k = 0; k < 130; ++k) {
            std::vector<std::pair<int32_t, double>> e;
            const int32_t len = k == 17 ? 300 : 1 + k % 3;
            for (int32_t x = len - 1; x >= 0; --x) e.push_back({x + (k == 17 ? 10 : k), 0.5 * (x + 1)});     // descending on purpose
            c.cut(e, 1.0 + k);
        }
        const CutPoolImage im = c.pack(320);
        CHECK(im.ell.slices() == 3 && im.ell.width(0) == 300 && im.ell.width(1) == 3 && im.ell.width(2) == 3);
        check_image(im, 320);
        // the chosen cuts of an add: ids in any order, the columns they touch, the longest
        const int32_t ids[3] = {129, 17, 0};
        const PoolChoice ch = pool_choose(im.ell, ids, 3);
        CHECK(ch.ptr == (std::vector<int64_t>{0, 1, 301, 302}) && ch.longest == 300);
        CHECK(ch.scalar == (std::vector<double>{130.0, 18.0, 1.0}));
        CHECK(ch.idx[0] == 129 && ch.idx[1] == 10 && ch.idx[300] == 309 && ch.idx[301] == 0);
        CHECK(ch.touched == 301);                       // columns 10 .. 309 (column 129 is among them) and column 0
        const int32_t one[1] = {5};
        const PoolChoice c1 = pool_choose(im.ell, one, 1);
        CHECK(c1.touched == 3 && c1.longest == 3 && c1.values == (std::vector<double>{0.5, 1.0, 1.5}));
        CHECK(pool_choose(im.ell, nullptr, 0).touched == 0);
    }
}

static void test_segments_key_and_checks() {
    // the shares are those of relp_pool_price: they tile [0, count) in order
    for (const auto& c : {std::pair<int32_t, int32_t>{257, 1}, {257, 257}, {65, 3}, {10, 7}, {5000, 2}}) {
        int32_t covered = 0;
        for (int32_t s = 0; s < c.second; ++s) {
            CHECK(pool_segment_lo(c.first, c.second, s) == covered);
            covered = pool_segment_hi(c.first, c.second, s);
        }
        CHECK(covered == c.first);
    }
    CHECK(pool_segment_chunks(5000, 2) == 10 && pool_segment_chunks(257, 1) == 2 && pool_segment_chunks(257, 257) == 1);
    // the key
    CHECK(cutpool_key(-3.0, 2.0, 0) == -3.0 && cutpool_key(-3.0, 2.0, 1) == -1.5 && cutpool_key(-3.0, 0.0, 1) == -3.0);
    CHECK(cutpool_key(-1.0, 3.0, 1) == -1.0 / 3.0);
    // the argument checks of relp_cutpool_separate
    int dummy = 0;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(cutpool_check_separate_args(10, 1, 0.0, 0, &dummy, &dummy, &dummy).empty());
    CHECK(cutpool_check_separate_args(10, 10, 1e-7, 1, &dummy, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 0, 0.0, 0, &dummy, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 11, 0.0, 0, &dummy, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, -1, 0.0, 0, &dummy, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 1, -1e-9, 0, &dummy, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 1, inf, 0, &dummy, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 1, nan, 0, &dummy, &dummy, &dummy).empty());
    CHECK(cutpool_check_separate_args(10, 1, 0.0, 2, &dummy, &dummy, &dummy).find("by_efficacy") != std::string::npos);
    CHECK(!cutpool_check_separate_args(10, 1, 0.0, -1, &dummy, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 1, 0.0, 0, nullptr, &dummy, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 1, 0.0, 0, &dummy, nullptr, &dummy).empty());
    CHECK(!cutpool_check_separate_args(10, 1, 0.0, 0, &dummy, &dummy, nullptr).empty());
    CHECK(cutpool_check_separate_args(0, 3, 0.0, 0, &dummy, &dummy, &dummy).empty());      // an empty pool: any segments >= 1
    CHECK(!cutpool_check_separate_args(0, 0, 0.0, 0, &dummy, &dummy, &dummy).empty());
    // the lists
    const int32_t fine[3] = {4, 0, 2}, twice[3] = {4, 0, 4}, outside[2] = {1, 5}, negative[1] = {-1};
    CHECK(pool_check_ids(kCutPoolWords, fine, 3, 5).empty() && pool_check_ids(kCutPoolWords, nullptr, 0, 5).empty() && pool_check_ids(kCutPoolWords, fine, 0, 0).empty());
    CHECK(pool_check_ids(kCutPoolWords, twice, 3, 5).find("twice") != std::string::npos);
    CHECK(pool_check_ids(kCutPoolWords, outside, 2, 5).find("range") != std::string::npos);
    CHECK(!pool_check_ids(kCutPoolWords, negative, 1, 5).empty() && !pool_check_ids(kCutPoolWords, nullptr, 2, 5).empty() && !pool_check_ids(kCutPoolWords, fine, -1, 5).empty());
    CHECK(!pool_check_ids(kCutPoolWords, fine, 3, 4).empty());
}

int main() {
    test_packer_and_norms();
    test_segments_key_and_checks();
    return finish("test_cutpool");
}
