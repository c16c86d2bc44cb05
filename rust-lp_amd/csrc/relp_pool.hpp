// relp_pool.hpp -- the host side of a pool of sparse vectors kept on the device in sliced ELL: the column pool (relp_pool_create ..
// relp_pool_stats, include/relp_engine.h) and, with the roles transposed, the cut pool (relp_cutpool.hpp).  The packer, the segment
// arithmetic of a sweep, the stale rule of the column pool and the argument checks.  Plain C++17: no HIP, no engine, so a C++ test
// includes this file alone (tests/cpp/test_pool.cpp).
//
// The device layout (relp_kernels.h: PoolView).  A pool holds `count` items -- pool columns, or cuts -- each a sparse vector over
// [0, bound) -- the engine rows, or the structural columns -- with one scalar -- the cost, or the right-hand side.  Item k sits in
// slice k / 64 as lane k % 64: one wave sweeps one slice.  slice_ptr[s] is the first stored entry of slice s, in entries, and the
// slice is as wide as its longest item,
//   width(s) = (slice_ptr[s + 1] - slice_ptr[s]) / 64,      entry e of item k at  slice_ptr[k / 64] + e * 64 + k % 64,
// entry-major, so the 64 lanes of a wave read 64 consecutive entries (512 B of values, 256 B of indices).  Inside an item the
// indices ascend -- the summation order of the reduced cost and of the slack -- whatever the order in the caller's CSC or CSR,
// explicit zeros are dropped, and the item is padded to the width of its slice with (index -1, value 0.0).  A padded entry is
// skipped by its index: it never reaches an fma.  The last slice has 64 lanes too; the lanes behind the last item hold padding only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace relp {

static constexpr int32_t kPoolSlice = 64;              // pool items per slice: one wave
static constexpr int32_t kPoolChunk = 256;             // pool items per workgroup of k_pool_sweep: one per thread, four slices

struct PoolImage {
    int32_t count = 0;                                 // pool items
    int32_t bound = 0;                                 // every index is below it (the column pool: relp_nr_rows() at the create)
    // the host copy: CSC (CSR) with ascending indices and without explicit zeros (what Layout::add_columns / add_cuts and the
    // rebuilds are given)
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx;
    std::vector<double> values, scalar;
    // the device image
    std::vector<int64_t> slice_ptr;                    // slices() + 1 offsets, in entries
    std::vector<int32_t> ell_idx;                      // stored() indices, -1 = padding
    std::vector<double> ell_val;                       // stored() values, 0.0 at padding
    int32_t slices() const { return (int32_t)slice_ptr.size() - 1; }
    int64_t nonzeros() const { return ptr.empty() ? 0 : ptr.back(); }
    int64_t stored() const { return slice_ptr.back(); }
    int32_t length(int32_t k) const { return (int32_t)(ptr[k + 1] - ptr[k]); }
    int32_t width(int32_t s) const { return (int32_t)((slice_ptr[s + 1] - slice_ptr[s]) / kPoolSlice); }
    int64_t at(int32_t k, int32_t e) const { return slice_ptr[k / kPoolSlice] + (int64_t)e * kPoolSlice + k % kPoolSlice; }
};

// The pool of `count` items in CSC (CSR) over [0, bound).  The caller has run the checks of relp_add_columns (Layout::check_columns;
// for cuts Layout::check_cuts): the arrays are there, ptr ascends from 0, every index is in [0, bound), none twice in an item,
// everything finite.
inline PoolImage pool_pack(int32_t count, const int64_t* ptr, const int32_t* idx, const double* values, const double* scalar, int32_t bound) {
    PoolImage im;
    im.count = count;
    im.bound = bound;
    im.ptr.assign(1, 0);
    im.scalar.assign(scalar, scalar + count);
    std::vector<std::pair<int32_t, double>> entries;
    for (int32_t k = 0; k < count; ++k) {
        entries.clear();
        for (int64_t x = ptr[k]; x < ptr[k + 1]; ++x)
            if (values[x] != 0.0) entries.emplace_back(idx[x], values[x]);
        std::sort(entries.begin(), entries.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (const auto& e : entries) { im.idx.push_back(e.first); im.values.push_back(e.second); }
        im.ptr.push_back((int64_t)im.idx.size());
    }
    const int32_t slices = (count + kPoolSlice - 1) / kPoolSlice;
    im.slice_ptr.assign(1, 0);
    for (int32_t s = 0; s < slices; ++s) {
        int32_t width = 0;
        for (int32_t k = s * kPoolSlice; k < std::min(count, (s + 1) * kPoolSlice); ++k) width = std::max(width, im.length(k));
        im.slice_ptr.push_back(im.slice_ptr.back() + (int64_t)width * kPoolSlice);
    }
    im.ell_idx.assign((size_t)im.stored(), -1);
    im.ell_val.assign((size_t)im.stored(), 0.0);
    for (int32_t k = 0; k < count; ++k)
        for (int32_t e = 0; e < im.length(k); ++e) {
            im.ell_idx[(size_t)im.at(k, e)] = im.idx[(size_t)(im.ptr[k] + e)];
            im.ell_val[(size_t)im.at(k, e)] = im.values[(size_t)(im.ptr[k] + e)];
        }
    return im;
}

// A sweep (relp_pool_price, relp_cutpool_separate) cuts the pool indices [0, count) into `segments` equal shares of
// ceil(count / segments) items; the last shares may be short or empty.  A share is swept in chunks of kPoolChunk items, one
// workgroup each.
inline int32_t pool_segment_size(int32_t count, int32_t segments) { return segments > 0 ? (int32_t)(((int64_t)count + segments - 1) / segments) : 0; }
inline int32_t pool_segment_lo(int32_t count, int32_t segments, int32_t s) {
    return (int32_t)std::min<int64_t>(count, (int64_t)s * pool_segment_size(count, segments));
}
inline int32_t pool_segment_hi(int32_t count, int32_t segments, int32_t s) { return pool_segment_lo(count, segments, s + 1); }
inline int32_t pool_segment_chunks(int32_t count, int32_t segments) {
    return std::max(1, (pool_segment_size(count, segments) + kPoolChunk - 1) / kPoolChunk);
}

// The total order of the winners: smaller key (d, or the cut's key) first, the lower pool index among equal keys.  k < 0 is "no candidate" and loses to
// everything.
inline bool pool_better(double d_a, int32_t k_a, double d_b, int32_t k_b) {
    if (k_a < 0) return false;
    if (k_b < 0) return true;
    return d_a < d_b || (d_a == d_b && k_a < k_b);
}

// The stale rule of a column pool: it holds row indices below its bound, the rows at the create.  Cut rows added later lie behind
// them and have coefficient 0 in every pool column; taking those out again moves no row of the pool.  Taking out an engine row
// below the bound does.  Rows also go when a trial is rolled back (the cut rows added inside it, the last rows): a pool created
// inside that trial over them then has its bound above the engine's rows, which is the same test with "every row from m on" as the
// list.  (A cut pool has no such rule: the structural columns never move.)
inline bool pool_stale_after_rollback(int32_t bound, int32_t m) { return bound > m; }
inline bool pool_stale_after_removal(int32_t bound, const int32_t* rows, int32_t count) {
    for (int32_t x = 0; x < count; ++x)
        if (rows[x] < bound) return true;
    return false;
}

// The words in which a pool's messages name what it holds; the column pool's and the cut pool's (relp_cutpool.hpp) differ in them alone.
struct PoolWords { const char* pool; const char* item; const char* items; const char* out; };
static constexpr PoolWords kColumnPoolWords{"a pool", "column", "columns", "d_out"};

// The RELP_E_ARG cases of a sweep, relp_pool_price or relp_cutpool_separate (empty: none).  A pool without items takes any
// segments >= 1.
inline std::string pool_check_sweep_args(const PoolWords& w, int32_t count, int32_t segments, double tol, const void* ids_out, const void* out,
                                         const void* found) {
    if (!ids_out || !out || !found) return std::string("ids_out, ") + w.out + " or found missing";
    if (segments < 1 || (count > 0 && segments > count)) return std::string("segments outside [1, pool ") + w.items + "]";
    if (!std::isfinite(tol) || tol < 0.0) return "tol is negative or not finite";
    return {};
}

// A list of pool items (the adds, the set_actives): there, every index in [0, bound), none twice (empty: fine).
inline std::string pool_check_ids(const PoolWords& w, const int32_t* ids, int32_t count, int32_t bound) {
    if (count < 0 || (count > 0 && !ids)) return "count < 0 or ids missing";
    std::vector<uint8_t> named((size_t)std::max(bound, 0), 0);
    for (int32_t x = 0; x < count; ++x) {
        if (ids[x] < 0 || ids[x] >= bound) return std::string("a pool ") + w.item + " out of range";
        if (named[ids[x]]) return std::string("a pool ") + w.item + " named twice";
        named[ids[x]] = 1;
    }
    return {};
}

// The items ids[0 .. count) of the pool as a CSC (CSR) of their own (what relp_add_columns or relp_add_cuts would be given), and
// what the add needs to know before it launches: the number of indices with an entry in some chosen item -- the rows of the union
// list of relp_pool_add; the structural columns that bound the one of relp_cutpool_add -- and the longest chosen item.
struct PoolChoice {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx;
    std::vector<double> values, scalar;
    int32_t touched = 0, longest = 0;
};
inline PoolChoice pool_choose(const PoolImage& im, const int32_t* ids, int32_t count) {
    PoolChoice ch;
    ch.ptr.assign(1, 0);
    std::vector<uint8_t> touched((size_t)std::max(im.bound, 0), 0);
    for (int32_t x = 0; x < count; ++x) {
        const int32_t k = ids[x];
        for (int64_t e = im.ptr[k]; e < im.ptr[k + 1]; ++e) {
            ch.idx.push_back(im.idx[(size_t)e]);
            ch.values.push_back(im.values[(size_t)e]);
            if (!touched[im.idx[(size_t)e]]) { touched[im.idx[(size_t)e]] = 1; ++ch.touched; }
        }
        ch.ptr.push_back((int64_t)ch.idx.size());
        ch.scalar.push_back(im.scalar[k]);
        ch.longest = std::max(ch.longest, im.length(k));
    }
    return ch;
}

}  // namespace relp
