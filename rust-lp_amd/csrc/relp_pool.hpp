// relp_pool.hpp -- the host side of a column pool (relp_pool_create .. relp_pool_stats, include/relp_engine.h): the sliced-ELL
// packer, the segment arithmetic of relp_pool_price, the stale rule and the argument checks.  Plain C++17: no HIP, no engine, so a
// C++ test includes this file alone (tests/cpp/test_pool.cpp).
//
// The device layout (relp_kernels.h: PoolView).  Pool column k sits in slice k / 64 as lane k % 64: one wave prices one slice.
// slice_ptr[s] is the first stored entry of slice s, in entries, and the slice is as wide as its longest column,
//   width(s) = (slice_ptr[s + 1] - slice_ptr[s]) / 64,      entry e of column k at  slice_ptr[k / 64] + e * 64 + k % 64,
// entry-major, so the 64 lanes of a wave read 64 consecutive entries (512 B of values, 256 B of rows).  Inside a column the rows
// ascend -- the summation order of the reduced cost -- whatever the order in the caller's CSC, explicit zeros are dropped, and the
// column is padded to the width of its slice with (row -1, value 0.0).  A padded entry is skipped by its row: it never reaches an
// fma.  The last slice has 64 lanes too; the lanes behind the last column hold padding only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace relp {

static constexpr int32_t kPoolSlice = 64;              // pool columns per slice: one wave
static constexpr int32_t kPoolChunk = 256;             // pool columns per workgroup of k_pool_price: one per thread, four slices

struct PoolImage {
    int32_t count = 0;                                 // pool columns
    int32_t rows_at_create = 0;                        // relp_nr_rows() at the create: every row index is below it
    // the host copy: CSC with ascending rows and without explicit zeros (what Layout::add_columns and the rebuilds are given)
    std::vector<int64_t> col_ptr;
    std::vector<int32_t> row_idx;
    std::vector<double> values, cost;
    // the device image
    std::vector<int64_t> slice_ptr;                    // slices() + 1 offsets, in entries
    std::vector<int32_t> ell_row;                      // stored() rows, -1 = padding
    std::vector<double> ell_val;                       // stored() values, 0.0 at padding
    int32_t slices() const { return (int32_t)slice_ptr.size() - 1; }
    int64_t nonzeros() const { return col_ptr.empty() ? 0 : col_ptr.back(); }
    int64_t stored() const { return slice_ptr.back(); }
    int32_t length(int32_t k) const { return (int32_t)(col_ptr[k + 1] - col_ptr[k]); }
    int32_t width(int32_t s) const { return (int32_t)((slice_ptr[s + 1] - slice_ptr[s]) / kPoolSlice); }
    int64_t at(int32_t k, int32_t e) const { return slice_ptr[k / kPoolSlice] + (int64_t)e * kPoolSlice + k % kPoolSlice; }
};

// The pool of `count` columns in CSC over `m` rows.  The caller has run the checks of relp_add_columns (Layout::check_columns):
// the arrays are there, col_ptr ascends from 0, every row is in [0, m), none twice in a column, everything finite.
inline PoolImage pool_pack(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost, int32_t m) {
    PoolImage im;
    im.count = count;
    im.rows_at_create = m;
    im.col_ptr.assign(1, 0);
    im.cost.assign(cost, cost + count);
    std::vector<std::pair<int32_t, double>> entries;
    for (int32_t k = 0; k < count; ++k) {
        entries.clear();
        for (int64_t x = col_ptr[k]; x < col_ptr[k + 1]; ++x)
            if (values[x] != 0.0) entries.emplace_back(row_idx[x], values[x]);
        std::sort(entries.begin(), entries.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (const auto& e : entries) { im.row_idx.push_back(e.first); im.values.push_back(e.second); }
        im.col_ptr.push_back((int64_t)im.row_idx.size());
    }
    const int32_t slices = (count + kPoolSlice - 1) / kPoolSlice;
    im.slice_ptr.assign(1, 0);
    for (int32_t s = 0; s < slices; ++s) {
        int32_t width = 0;
        for (int32_t k = s * kPoolSlice; k < std::min(count, (s + 1) * kPoolSlice); ++k) width = std::max(width, im.length(k));
        im.slice_ptr.push_back(im.slice_ptr.back() + (int64_t)width * kPoolSlice);
    }
    im.ell_row.assign((size_t)im.stored(), -1);
    im.ell_val.assign((size_t)im.stored(), 0.0);
    for (int32_t k = 0; k < count; ++k)
        for (int32_t e = 0; e < im.length(k); ++e) {
            im.ell_row[(size_t)im.at(k, e)] = im.row_idx[(size_t)(im.col_ptr[k] + e)];
            im.ell_val[(size_t)im.at(k, e)] = im.values[(size_t)(im.col_ptr[k] + e)];
        }
    return im;
}

// relp_pool_price cuts the pool indices [0, count) into `segments` equal shares of ceil(count / segments) columns; the last
// shares may be short or empty.  A share is priced in chunks of kPoolChunk columns, one workgroup each.
inline int32_t pool_segment_size(int32_t count, int32_t segments) { return segments > 0 ? (int32_t)(((int64_t)count + segments - 1) / segments) : 0; }
inline int32_t pool_segment_lo(int32_t count, int32_t segments, int32_t s) {
    return (int32_t)std::min<int64_t>(count, (int64_t)s * pool_segment_size(count, segments));
}
inline int32_t pool_segment_hi(int32_t count, int32_t segments, int32_t s) { return pool_segment_lo(count, segments, s + 1); }
inline int32_t pool_segment_chunks(int32_t count, int32_t segments) {
    return std::max(1, (pool_segment_size(count, segments) + kPoolChunk - 1) / kPoolChunk);
}

// The total order of the winners: smaller d first, the lower pool index among equal d.  k < 0 is "no candidate" and loses to
// everything.
inline bool pool_better(double d_a, int32_t k_a, double d_b, int32_t k_b) {
    if (k_a < 0) return false;
    if (k_b < 0) return true;
    return d_a < d_b || (d_a == d_b && k_a < k_b);
}

// The stale rule: a pool holds row indices below rows_at_create.  Cut rows added later lie behind them and have coefficient 0 in
// every pool column; taking those out again moves no row of the pool.  Taking out an engine row below rows_at_create does.
// Rows also go when a trial is rolled back (the cut rows added inside it, the last rows): a pool created inside that trial over
// them then has rows_at_create above the engine's rows, which is the same test with "every row from m on" as the list.
inline bool pool_stale_after_rollback(int32_t rows_at_create, int32_t m) { return rows_at_create > m; }
inline bool pool_stale_after_removal(int32_t rows_at_create, const int32_t* rows, int32_t count) {
    for (int32_t x = 0; x < count; ++x)
        if (rows[x] < rows_at_create) return true;
    return false;
}

// The RELP_E_ARG cases of relp_pool_price (nullptr: none).  A pool without columns takes any segments >= 1.
inline const char* pool_check_price_args(int32_t count, int32_t segments, double tol, const void* ids_out, const void* d_out, const void* found) {
    if (!ids_out || !d_out || !found) return "ids_out, d_out or found missing";
    if (segments < 1 || (count > 0 && segments > count)) return "segments outside [1, pool columns]";
    if (!std::isfinite(tol) || tol < 0.0) return "tol is negative or not finite";
    return nullptr;
}

// A list of pool columns (relp_pool_add, relp_pool_set_active): there, every index in [0, bound), none twice (nullptr: fine).
inline const char* pool_check_ids(const int32_t* ids, int32_t count, int32_t bound) {
    if (count < 0 || (count > 0 && !ids)) return "count < 0 or ids missing";
    std::vector<uint8_t> named((size_t)std::max(bound, 0), 0);
    for (int32_t x = 0; x < count; ++x) {
        if (ids[x] < 0 || ids[x] >= bound) return "a pool column out of range";
        if (named[ids[x]]) return "a pool column named twice";
        named[ids[x]] = 1;
    }
    return nullptr;
}

// The columns ids[0 .. count) of the pool as a CSC of their own (what relp_add_columns would be given), and what the add needs to
// know before it launches: the rows with an entry in some chosen column (the length of the union list) and the longest chosen column.
struct PoolChoice {
    std::vector<int64_t> col_ptr;
    std::vector<int32_t> row_idx;
    std::vector<double> values, cost;
    int32_t entries = 0, longest = 0;
};
inline PoolChoice pool_choose(const PoolImage& im, const int32_t* ids, int32_t count, int32_t m) {
    PoolChoice ch;
    ch.col_ptr.assign(1, 0);
    std::vector<uint8_t> touched((size_t)std::max(m, 0), 0);
    for (int32_t x = 0; x < count; ++x) {
        const int32_t k = ids[x];
        for (int64_t e = im.col_ptr[k]; e < im.col_ptr[k + 1]; ++e) {
            ch.row_idx.push_back(im.row_idx[(size_t)e]);
            ch.values.push_back(im.values[(size_t)e]);
            if (!touched[im.row_idx[(size_t)e]]) { touched[im.row_idx[(size_t)e]] = 1; ++ch.entries; }
        }
        ch.col_ptr.push_back((int64_t)ch.row_idx.size());
        ch.cost.push_back(im.cost[k]);
        ch.longest = std::max(ch.longest, im.length(k));
    }
    return ch;
}

}  // namespace relp
