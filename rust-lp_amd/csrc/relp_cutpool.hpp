// relp_cutpool.hpp -- the host side of a cut pool (relp_cutpool_create .. relp_cutpool_stats, include/relp_engine.h): the adapter
// onto the sliced-ELL packer of the column pool, the norms, the order of the winners and the argument checks.  Plain C++17: no HIP,
// no engine, so a C++ test includes this file alone (tests/cpp/test_cutpool.cpp).
//
// A cut pool is the column pool with the roles transposed: `count` cuts g_k' x <= rhs_k in CSR over the structural columns
// [0, nr_normal) are `count` sparse vectors over nr_normal positions with one scalar each, which is what pool_pack packs.  So the
// device layout is the one of relp_pool.hpp with "pool column" read as "cut", "row" as "structural column" and "cost" as "rhs":
// cut k is lane k % 64 of slice k / 64, entry e of it stands at slice_ptr[k / 64] + e * 64 + k % 64, the columns ascend inside a
// cut -- the summation order of the slack -- explicit zeros are dropped and padding is (column -1, value 0.0), skipped by its column.
// The segment arithmetic of relp_cutpool_separate is pool_segment_size / _lo / _hi / _chunks as they stand.
//
// There is no stale rule: the structural columns never move (added columns lie behind them, and a cut holds no coefficient on one).
#pragma once
#include "relp_pool.hpp"

namespace relp {

struct CutPoolImage {
    PoolImage ell;                                     // col_ptr / row_idx / values / cost there = row_ptr / col_idx / values / rhs here
    std::vector<double> norm;                          // the Euclidean norm of every cut (cutpool_norm)
    int32_t count() const { return ell.count; }
    const std::vector<int64_t>& row_ptr() const { return ell.col_ptr; }
    const std::vector<int32_t>& col_idx() const { return ell.row_idx; }
    const std::vector<double>& values() const { return ell.values; }
    const std::vector<double>& rhs() const { return ell.cost; }
};

// norm_k: the square root of ONE fma chain of squares from 0.0 over the stored entries in stored (ascending column) order.
inline double cutpool_norm(const double* values, int64_t n) {
    double acc = 0.0;
    for (int64_t e = 0; e < n; ++e) acc = std::fma(values[e], values[e], acc);
    return std::sqrt(acc);
}

// The pool of `count` cuts in CSR over `nr_normal` structural columns.  The caller has run the checks of relp_add_cuts
// (Layout::check_cuts): the arrays are there, row_ptr ascends from 0, every column is structural, none twice in a cut, everything
// finite.
inline CutPoolImage cutpool_pack(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs,
                                 int32_t nr_normal) {
    CutPoolImage im;
    im.ell = pool_pack(count, row_ptr, col_idx, values, rhs, nr_normal);
    im.norm.resize((size_t)count);
    for (int32_t k = 0; k < count; ++k) im.norm[(size_t)k] = cutpool_norm(im.ell.values.data() + im.ell.col_ptr[k], im.ell.length(k));
    return im;
}

// The key of a cut with slack s: s itself, or (by_efficacy) s / norm, a cut of norm 0 ranking with norm 1.  One rounding.
inline double cutpool_key(double s, double norm, int32_t by_efficacy) { return by_efficacy ? s / (norm == 0.0 ? 1.0 : norm) : s; }

// The RELP_E_ARG cases of relp_cutpool_separate (nullptr: none): those of relp_pool_price, and a by_efficacy outside {0, 1}.
inline const char* cutpool_check_separate_args(int32_t count, int32_t segments, double tol, int32_t by_efficacy, const void* ids_out,
                                               const void* slack_out, const void* found) {
    if (!ids_out || !slack_out || !found) return "ids_out, slack_out or found missing";
    if (segments < 1 || (count > 0 && segments > count)) return "segments outside [1, pool cuts]";
    if (!std::isfinite(tol) || tol < 0.0) return "tol is negative or not finite";
    if (by_efficacy != 0 && by_efficacy != 1) return "by_efficacy is neither 0 nor 1";
    return nullptr;
}

// A list of pool cuts (relp_cutpool_add, relp_cutpool_set_active): there, every index in [0, bound), none twice (nullptr: fine).
inline const char* cutpool_check_ids(const int32_t* ids, int32_t count, int32_t bound) {
    if (count < 0 || (count > 0 && !ids)) return "count < 0 or ids missing";
    std::vector<uint8_t> named((size_t)std::max(bound, 0), 0);
    for (int32_t x = 0; x < count; ++x) {
        if (ids[x] < 0 || ids[x] >= bound) return "a pool cut out of range";
        if (named[ids[x]]) return "a pool cut named twice";
        named[ids[x]] = 1;
    }
    return nullptr;
}

// The cuts ids[0 .. count) of the pool as a CSR of their own (what relp_add_cuts would be given), and what the add needs to know
// before it launches: the structural columns with an entry in some chosen cut -- the union list of the add is the basic ones among
// them, so this bounds its length -- and the longest chosen cut.
struct CutPoolChoice {
    std::vector<int64_t> row_ptr;
    std::vector<int32_t> col_idx;
    std::vector<double> values, rhs;
    int32_t touched = 0, longest = 0;
};
inline CutPoolChoice cutpool_choose(const CutPoolImage& im, const int32_t* ids, int32_t count, int32_t nr_normal) {
    PoolChoice ch = pool_choose(im.ell, ids, count, nr_normal);
    CutPoolChoice out;
    out.row_ptr = std::move(ch.col_ptr);
    out.col_idx = std::move(ch.row_idx);
    out.values = std::move(ch.values);
    out.rhs = std::move(ch.cost);
    out.touched = ch.entries;
    out.longest = ch.longest;
    return out;
}

}  // namespace relp
