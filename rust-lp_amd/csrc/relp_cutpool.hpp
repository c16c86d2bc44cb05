// relp_cutpool.hpp -- what the host side of a cut pool (relp_cutpool_create .. relp_cutpool_stats, include/relp_engine.h) has of its
// own beside relp_pool.hpp: the norms and the key of the winners.  Plain C++17: no HIP, no engine, so a C++ test includes this file
// alone (tests/cpp/test_cutpool.cpp).
//
// A cut pool is a pool of relp_pool.hpp as it stands: `count` cuts g_k' x <= rhs_k in CSR over the structural columns
// [0, nr_normal) are `count` sparse vectors over nr_normal positions with one scalar each -- the items are cuts, the indices
// structural columns, the scalar the right-hand side.  The packer, the segment arithmetic, the id lists and pool_choose are used as
// they are.  There is no stale rule: the structural columns never move (added columns lie behind them, and a cut holds no
// coefficient on one).
#pragma once
#include "relp_pool.hpp"

namespace relp {

static constexpr PoolWords kCutPoolWords{"a cut pool", "cut", "cuts", "slack_out"};

struct CutPoolImage {
    PoolImage ell;                                     // ptr / idx / values / scalar = row_ptr / col_idx / values / rhs
    std::vector<double> norm;                          // the Euclidean norm of every cut (cutpool_norm)
};

// norm_k: the square root of ONE fma chain of squares from 0.0 over the stored entries in stored (ascending column) order.
inline double cutpool_norm(const double* values, int64_t n) {
    double acc = 0.0;
    for (int64_t e = 0; e < n; ++e) acc = std::fma(values[e], values[e], acc);
    return std::sqrt(acc);
}

// The pool of `count` cuts in CSR over `nr_normal` structural columns (pool_pack; the checks are those of relp_add_cuts).
inline CutPoolImage cutpool_pack(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs,
                                 int32_t nr_normal) {
    CutPoolImage im;
    im.ell = pool_pack(count, row_ptr, col_idx, values, rhs, nr_normal);
    im.norm.resize((size_t)count);
    for (int32_t k = 0; k < count; ++k) im.norm[(size_t)k] = cutpool_norm(im.ell.values.data() + im.ell.ptr[k], im.ell.length(k));
    return im;
}

// The key of a cut with slack s: s itself, or (by_efficacy) s / norm, a cut of norm 0 ranking with norm 1.  One rounding.
inline double cutpool_key(double s, double norm, int32_t by_efficacy) { return by_efficacy ? s / (norm == 0.0 ? 1.0 : norm) : s; }

// The RELP_E_ARG cases of relp_cutpool_separate (empty: none): those of a sweep, then a by_efficacy outside {0, 1}.
inline std::string cutpool_check_separate_args(int32_t count, int32_t segments, double tol, int32_t by_efficacy, const void* ids_out,
                                               const void* slack_out, const void* found) {
    std::string why = pool_check_sweep_args(kCutPoolWords, count, segments, tol, ids_out, slack_out, found);
    if (why.empty() && by_efficacy != 0 && by_efficacy != 1) why = "by_efficacy is neither 0 nor 1";
    return why;
}

}  // namespace relp
