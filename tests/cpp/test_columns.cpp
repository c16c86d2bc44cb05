// C++ host-side test of columns added in place over include/relp.hpp (no counterpart in the reference, whose provider is immutable):
// add_columns, reserve_columns, column_stats, run, objective on the dense 24 x 32 LP of rust-lp_amd/synthetic.py (seed 1), whose last
// three columns are held back and added on the optimal basis of the first 29.  Runs on the GPU box: `tests/cpp/test_columns` (built by
// tests/cpp/Makefile, `__graft_entry__.build()`); exit code 0 = all checks passed.  tests/test_cpp_columns.py runs it under pytest
// (-m gpu).
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
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

int main() {
    try {
        const Options tableau = Options().inverse_maintenance(InverseMaintenance::DenseTableau);
        const int m = 24, n = 32, k = 3, n0 = n - k;
        {
            Tableau t(dense_le(m, n, 1, n0), tableau);
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            const double narrow = t.objective_function_value();
            CHECK(t.nr_rows() == m && t.nr_columns() == n0 + m);
            CHECK((t.column_stats() == std::array<int64_t, 4>{0, 0, 0, 0}));
            // the three columns held back, CSC with the rows of each in descending order (the order inside a column is free)
            std::vector<int64_t> ptr{0};
            std::vector<int32_t> idx;
            std::vector<double> val, cost;
            for (int c = 0; c < k; ++c) {
                for (int i = m - 1; i >= 0; --i) { idx.push_back(i); val.push_back(a_of(m, 1, i, n0 + c)); }
                ptr.push_back((int64_t)idx.size());
                cost.push_back(c_of(1, n0 + c));
            }
            const std::vector<double> d = t.relative_costs(), b = t.b(), minus_pi = t.minus_pi();
            const std::vector<int32_t> basis = t.basis_indices();
            const std::array<int64_t, 4> cuts = t.cut_stats();
            t.reserve_columns(2);
            CHECK((t.column_stats() == std::array<int64_t, 4>{0, 2, 0, 0}));
            CHECK(t.relative_costs() == d && t.b() == b && t.objective_function_value() == narrow && t.cut_stats() == cuts);
            t.add_columns(ptr, idx, val, cost);                                        // grows: 3 > 2
            CHECK(t.nr_rows() == m && t.nr_columns() == n0 + m + k);
            CHECK((t.column_stats() == std::array<int64_t, 4>{3, 16, m, 0}));
            CHECK(t.objective_function_value() == narrow && t.reinversions() == 0 && t.cut_stats() == cuts);
            const std::vector<double> d2 = t.relative_costs();
            bool old_same = t.b() == b && t.basis_indices() == basis, priced = true, some_negative = false;
            for (int j = 0; j < n0 + m; ++j) old_same = old_same && d2[j] == d[j];
            for (int c = 0; c < k; ++c) {
                double want = cost[c];
                for (int i = 0; i < m; ++i) want += minus_pi[i] * a_of(m, 1, i, n0 + c);
                priced = priced && near(d2[n0 + m + c], want);
                some_negative = some_negative || d2[n0 + m + c] < -1e-6;
                // B^-1 a of the new column against generate_column_of of its entries
                SparseVector a;
                for (int i = 0; i < m; ++i) a.emplace_back(i, a_of(m, 1, i, n0 + c));
                const std::vector<double> got = t.generate_column(n0 + m + c), ref = t.generate_column(a);
                for (int i = 0; i < m; ++i) priced = priced && near(got[i], ref[i]);
            }
            CHECK(old_same);
            CHECK(priced);
            const int64_t before = t.iterations();
            CHECK(t.run() == RELP_OPTIMAL);
            CHECK((t.iterations() > before) == some_negative);
            // the fresh two-phase solve of the wide LP
            Tableau fresh(dense_le(m, n, 1, n), tableau);
            CHECK(fresh.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            std::printf("objective %.12f on %d columns, %.12f with %d columns added in place, %.12f solved afresh\n", narrow, n0,
                        t.objective_function_value(), k, fresh.objective_function_value());
            CHECK(near(t.objective_function_value(), fresh.objective_function_value()));
            CHECK(t.objective_function_value() <= narrow + 1e-9);
            // the refusals leave the handle as it was
            const std::vector<double> d3 = t.relative_costs();
            const double inf = std::numeric_limits<double>::infinity();
            CHECK_THROWS(t.add_columns({0, 1}, {m}, {1.0}, {1.0}), RELP_E_ARG);        // behind the last row
            CHECK_THROWS(t.add_columns({0, 1}, {-1}, {1.0}, {1.0}), RELP_E_ARG);
            CHECK_THROWS(t.add_columns({0, 2}, {1, 1}, {1.0, 1.0}, {1.0}), RELP_E_ARG);   // named twice
            CHECK_THROWS(t.add_columns({1, 2}, {0, 1}, {1.0, 1.0}, {1.0}), RELP_E_ARG);   // col_ptr not from 0
            CHECK_THROWS(t.add_columns({0, 1}, {0}, {inf}, {1.0}), RELP_E_ARG);
            CHECK_THROWS(t.add_columns({0, 1}, {0}, {1.0}, {std::numeric_limits<double>::quiet_NaN()}), RELP_E_ARG);
            CHECK_THROWS(t.reserve_columns(-1), RELP_E_ARG);
            t.add_columns({0}, {}, {}, {});                                            // count == 0: a no-op
            CHECK(t.relative_costs() == d3 && t.nr_columns() == n0 + m + k && t.column_stats()[0] == 3);
        }
        {   // phase 1 and the other engines refuse
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 1}}, 2, {2, 1}, {}, 0, 0, 1, 1, {1, 1}), tableau);
            CHECK_THROWS(t.add_columns({0, 1}, {0}, {1.0}, {1.0}), RELP_E_STATE);
            CHECK_THROWS(t.reserve_columns(4), RELP_E_STATE);
            CHECK_THROWS(t.column_stats(), RELP_E_STATE);
            Tableau lu(MatrixData::from_rows({{1, 1}}, 2, {3}, {}, 0, 0, 1, 0, {-1, -1}, {2, 2}),
                       Options().inverse_maintenance(InverseMaintenance::LUDecomposition));
            CHECK(lu.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK_THROWS(lu.add_columns({0, 1}, {0}, {1.0}, {1.0}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(lu.reserve_columns(4), RELP_E_UNSUPPORTED);
            CHECK_THROWS(lu.column_stats(), RELP_E_UNSUPPORTED);
        }
    } catch (const std::exception& e) {
        std::printf("unexpected exception: %s\n", e.what());
        return 2;
    }
    return finish("test_columns");
}
