// C++ host-side test of cut rows and added columns removed in place over include/relp.hpp (no counterpart in the reference, whose
// provider is immutable): remove_cuts, remove_columns, removal_stats on the dense 24 x 32 LP of rust-lp_amd/synthetic.py (seed 1),
// whose last three columns are held back.  Runs on the GPU box: `tests/cpp/test_remove` (built by tests/cpp/Makefile,
// `__graft_entry__.build()`); exit code 0 = all checks passed.  tests/test_cpp_remove.py runs it under pytest (-m gpu).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "relp.hpp"
#include "check.hpp"

using namespace relp_host;


static bool near(double a, double b) { return near(a, b, 1e-9); }

// synthetic.splitmix64(seed, stream, idx)
static uint64_t splitmix64(uint64_t seed, uint64_t stream, uint64_t idx) {
    uint64_t z = seed + stream * 0xD1B54A32D192ED03ull + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// synthetic.dense_lp(m, n, seed): entry (i, j), b and c; b depends on the full width n
static double a_of(int m, uint64_t seed, int i, int j) { return (double)(1 + splitmix64(seed, 0, (uint64_t)j * m + i) % 999) / 1000.0; }
static double c_of(uint64_t seed, int j) { return -(double)(1000 + (int64_t)(splitmix64(seed, 2, j) % 1000)) / 1000.0; }

// the first `keep` columns of dense_lp(m, n, seed) as <= rows
static MatrixData dense_le(int m, int n, uint64_t seed, int keep) {
    std::vector<std::vector<double>> rows(m, std::vector<double>(keep));
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < keep; ++j) rows[i][j] = a_of(m, seed, i, j);
    std::vector<double> b(m), c(keep);
    for (int i = 0; i < m; ++i) b[i] = (double)(n * (1000 + (int64_t)(splitmix64(seed, 1, i) % 1000))) / 4000.0;
    for (int j = 0; j < keep; ++j) c[j] = c_of(seed, j);
    return MatrixData::from_rows(rows, keep, b, {}, 0, 0, m, 0, c);
}

template <class T>
static std::vector<T> without(const std::vector<T>& v, const std::vector<int>& gone) {
    std::vector<T> out;
    for (int x = 0; x < (int)v.size(); ++x) {
        bool g = false;
        for (int y : gone) g = g || y == x;
        if (!g) out.push_back(v[x]);
    }
    return out;
}

int main() {
    try {
        const Options tableau = Options().inverse_maintenance(InverseMaintenance::DenseTableau);
        const int m = 24, n = 32, k = 3, n0 = n - k;
        {
            Tableau t(dense_le(m, n, 1, n0), tableau);
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            const double narrow = t.objective_function_value();
            CHECK((t.removal_stats() == std::array<int64_t, 4>{0, 0, 0, 0}));
            // the three columns held back, at cost +1: none prices out, all stay non-basic
            std::vector<int64_t> ptr{0};
            std::vector<int32_t> idx;
            std::vector<double> val;
            for (int c = 0; c < k; ++c) {
                for (int i = 0; i < m; ++i) { idx.push_back(i); val.push_back(a_of(m, 1, i, n0 + c)); }
                ptr.push_back((int64_t)idx.size());
            }
            t.add_columns(ptr, idx, val, {1.0, 1.0, 1.0});
            const int64_t before = t.iterations();
            CHECK(t.run() == RELP_OPTIMAL && t.iterations() == before);
            // two cuts sum x <= 1e6 that cannot bind (slack basic in its own row), then one violated at x* (its slack leaves)
            std::vector<int64_t> cptr{0, n0, 2 * n0};
            std::vector<int32_t> cidx;
            for (int c = 0; c < 2; ++c)
                for (int j = 0; j < n0; ++j) cidx.push_back(j);
            t.add_cuts(cptr, cidx, std::vector<double>(2 * n0, 1.0), {1e6, 2e6});
            double sum_x = 0.0;
            for (const auto& e : t.current_bfs()) if (e.first < n0) sum_x += e.second;
            t.add_cuts({0, n0}, std::vector<int32_t>(cidx.begin(), cidx.begin() + n0), std::vector<double>(n0, 1.0), {0.9 * sum_x});
            CHECK(t.run_dual() == RELP_OPTIMAL);
            CHECK(t.nr_rows() == m + 3 && t.nr_columns() == n0 + m + k + 3);
            const double with_cut = t.objective_function_value();
            CHECK(with_cut > narrow);
            // (the removals flush the open block: a flush moves T0, not a bit of d, b or -obj)
            const std::vector<double> d = t.relative_costs(), b = t.b(), pi = t.minus_pi(), rhs = t.right_hand_side();
            const std::vector<int32_t> basis = t.basis_indices();
            const int first_added = n0 + m, first_slack = n0 + m + k;

            // ---- the refusals leave the handle as it was ----
            CHECK_THROWS(t.remove_cuts({m - 1}), RELP_E_ARG);                          // a constraint row
            CHECK_THROWS(t.remove_cuts({m + 3}), RELP_E_ARG);
            CHECK_THROWS(t.remove_cuts({m, m}), RELP_E_ARG);                           // named twice
            CHECK_THROWS(t.remove_cuts({m + 2}), RELP_E_STATE);                        // the violated cut is tight: its slack is not basic
            CHECK_THROWS(t.remove_cuts({m, m + 2}), RELP_E_STATE);
            CHECK_THROWS(t.remove_columns({0}), RELP_E_ARG);                           // a structural column
            CHECK_THROWS(t.remove_columns({first_slack}), RELP_E_ARG);                 // a cut slack is no added column
            CHECK_THROWS(t.remove_columns({first_added, first_added}), RELP_E_ARG);
            CHECK(t.relative_costs() == d && t.b() == b && t.basis_indices() == basis && t.nr_rows() == m + 3);
            CHECK((t.removal_stats() == std::array<int64_t, 4>{0, 0, 0, 0}));
            t.remove_cuts({});                                                          // count == 0: a no-op
            t.remove_columns({});
            CHECK(t.relative_costs() == d && t.nr_columns() == n0 + m + k + 3);

            // ---- the first and the third added column go: the cut slacks behind them close up ----
            t.remove_columns({first_added + 2, first_added});
            CHECK(t.nr_rows() == m + 3 && t.nr_columns() == n0 + m + 1 + 3);
            CHECK(t.relative_costs() == without(d, {first_added, first_added + 2}) && t.b() == b && t.minus_pi() == pi);
            CHECK(t.objective_function_value() == with_cut && t.reinversions() == 0);
            std::vector<int32_t> moved = basis;
            for (int32_t& j : moved) j -= j > first_added + 2 ? 2 : (j > first_added ? 1 : 0);
            CHECK(t.basis_indices() == moved);
            CHECK(t.removal_stats()[0] == 0 && t.removal_stats()[1] == 2 && t.removal_stats()[2] == (int64_t)(m + 3) * (k + 3));
            CHECK(t.column_stats()[0] == 1 && t.column_stats()[1] == 16);

            // ---- the second loose cut goes with its slack: row m + 1, the column behind the remaining added column ----
            int row_of_slack = -1;
            for (int r = 0; r < m + 3; ++r) if (moved[r] == first_added + 1 + 1) row_of_slack = r;
            CHECK(row_of_slack == m + 1);                                               // never pivoted: basic in its own row
            t.remove_cuts({m + 1});
            CHECK(t.nr_rows() == m + 2 && t.nr_columns() == n0 + m + 1 + 2);
            CHECK(t.b() == without(b, {m + 1}) && t.minus_pi() == without(pi, {m + 1}) && t.right_hand_side() == without(rhs, {m + 1}));
            CHECK(t.relative_costs() == without(d, {first_added, first_added + 2, first_slack + 1}));
            CHECK(t.objective_function_value() == with_cut && t.reinversions() == 0);
            CHECK(t.removal_stats()[0] == 1 && t.removal_stats()[1] == 2 && t.cut_stats()[0] == 2 && t.cut_stats()[1] == 16);
            CHECK(t.run() == RELP_OPTIMAL && t.run_dual() == RELP_OPTIMAL && near(t.objective_function_value(), with_cut));

            // ---- the freed room is used again: the held-back columns at their own costs; the re-solve against a rebuild ----
            std::vector<double> cost;
            for (int c = 0; c < k; ++c) cost.push_back(c_of(1, n0 + c));
            std::vector<int64_t> ptr2{0};
            std::vector<int32_t> idx2;
            std::vector<double> val2;
            for (int c = 0; c < k; ++c) {
                for (int i = 0; i < m; ++i) { idx2.push_back(i); val2.push_back(a_of(m, 1, i, n0 + c)); }
                ptr2.push_back((int64_t)idx2.size());
            }
            t.add_columns(ptr2, idx2, val2, cost);
            CHECK(t.column_stats()[0] == 4 && t.column_stats()[1] == 16);
            CHECK(t.run() == RELP_OPTIMAL);
            const double in_place = t.objective_function_value();
            t.from_basis(t.basis_indices());                                            // the rebuild works on the smaller LP
            CHECK(near(t.objective_function_value(), in_place) && t.run() == RELP_OPTIMAL && near(t.objective_function_value(), in_place));
            std::printf("objective %.12f narrow, %.12f with the cut, %.12f after the removals and the columns\n", narrow, with_cut, in_place);
        }
        {   // phase 1 and the other engines refuse
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 1}}, 2, {2, 1}, {}, 0, 0, 1, 1, {1, 1}), tableau);
            CHECK_THROWS(t.remove_cuts({2}), RELP_E_STATE);
            CHECK_THROWS(t.remove_columns({2}), RELP_E_STATE);
            CHECK_THROWS(t.removal_stats(), RELP_E_STATE);
            Tableau lu(MatrixData::from_rows({{1, 1}}, 2, {3}, {}, 0, 0, 1, 0, {-1, -1}, {2, 2}),
                       Options().inverse_maintenance(InverseMaintenance::LUDecomposition));
            CHECK(lu.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK_THROWS(lu.remove_cuts({1}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(lu.remove_columns({1}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(lu.removal_stats(), RELP_E_UNSUPPORTED);
        }
    } catch (const std::exception& e) {
        std::printf("unexpected exception: %s\n", e.what());
        return 2;
    }
    return finish("test_remove");
}
