// C++ host-side test of cut rows added in place over include/relp.hpp (no counterpart in the reference, whose provider is immutable):
// add_cuts, reserve_cuts, cut_stats, run_dual, objective on the dense 24 x 32 LP of rust-lp_amd/synthetic.py (seed 1).  Runs on the GPU
// box: `tests/cpp/test_cuts` (built by tests/cpp/Makefile, `__graft_entry__.build()`); exit code 0 = all checks passed.
// tests/test_cpp_cuts.py runs it under pytest (-m gpu).
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

// synthetic.dense_lp(m, n, seed) with `cuts` further <= rows (G, beta) stacked under A
static MatrixData dense_le(int m, int n, uint64_t seed, const std::vector<std::vector<double>>& G = {}, const std::vector<double>& beta = {}) {
    std::vector<std::vector<double>> rows(m, std::vector<double>(n));
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) rows[i][j] = (double)(1 + splitmix64(seed, 0, (uint64_t)j * m + i) % 999) / 1000.0;
    std::vector<double> b(m), c(n);
    for (int i = 0; i < m; ++i) b[i] = (double)(n * (1000 + (int64_t)(splitmix64(seed, 1, i) % 1000))) / 4000.0;
    for (int j = 0; j < n; ++j) c[j] = -(double)(1000 + (int64_t)(splitmix64(seed, 2, j) % 1000)) / 1000.0;
    for (size_t k = 0; k < G.size(); ++k) { rows.push_back(G[k]); b.push_back(beta[k]); }
    return MatrixData::from_rows(rows, n, b, {}, 0, 0, m + (int)G.size(), 0, c);
}

int main() {
    try {
        const Options tableau = Options().inverse_maintenance(InverseMaintenance::DenseTableau);
        const int m = 24, n = 32;
        {
            Tableau t(dense_le(m, n, 1), tableau);
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            const double plain = t.objective_function_value();
            CHECK(t.nr_rows() == m && t.nr_columns() == n + m);
            CHECK((t.cut_stats() == std::array<int64_t, 4>{0, 0, 0, 0}));
            // x* and three cuts with coefficients in 0 .. 7, each 10 % inside x*
            std::vector<double> x(n, 0.0);
            for (auto& e : t.current_bfs()) if (e.first < n) x[e.first] = e.second;
            const int k = 3;
            std::vector<std::vector<double>> G(k, std::vector<double>(n));
            std::vector<double> beta(k, 0.0);
            std::vector<int64_t> ptr{0};
            std::vector<int32_t> idx;
            std::vector<double> val;
            for (int c = 0; c < k; ++c) {
                for (int j = n - 1; j >= 0; --j) {                                     // (descending: the order inside a cut is free)
                    G[c][j] = (double)(splitmix64(77, 3 + c, j) % 8);
                    beta[c] += G[c][j] * x[j];
                    if (G[c][j] != 0.0) { idx.push_back(j); val.push_back(G[c][j]); }
                }
                beta[c] *= 0.9;
                ptr.push_back((int64_t)idx.size());
            }
            const std::vector<double> d = t.relative_costs(), b = t.b();
            t.reserve_cuts(2);
            CHECK((t.cut_stats() == std::array<int64_t, 4>{0, 2, 0, 0}));
            CHECK(t.relative_costs() == d && t.b() == b && t.objective_function_value() == plain);
            t.add_cuts(ptr, idx, val, beta);                                           // grows: 3 > 2
            CHECK(t.nr_rows() == m + k && t.nr_columns() == n + m + k);
            CHECK(t.cut_stats()[0] == 3 && t.cut_stats()[1] == 16 && t.cut_stats()[2] >= 1);
            CHECK(t.objective_function_value() == plain && t.reinversions() == 0);
            const std::vector<double> d2 = t.relative_costs(), b2 = t.b();
            const std::vector<int32_t> basis = t.basis_indices();
            bool old_same = true, violated = true;
            for (int j = 0; j < n + m; ++j) old_same = old_same && d2[j] == d[j];
            for (int i = 0; i < m; ++i) old_same = old_same && b2[i] == b[i];
            for (int c = 0; c < k; ++c) { violated = violated && b2[m + c] < 0.0; CHECK(basis[m + c] == n + m + c && d2[n + m + c] == 0.0); }
            CHECK(old_same);
            CHECK(violated);
            std::vector<double> rhs = t.right_hand_side();
            CHECK((int)rhs.size() == m + k && rhs[m] == beta[0] && rhs[m + 2] == beta[2]);
            CHECK(t.run_dual() == RELP_OPTIMAL);
            // the fresh two-phase solve of the stacked LP
            Tableau fresh(dense_le(m, n, 1, G, beta), tableau);
            CHECK(fresh.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            std::printf("objective %.12f without cuts, %.12f with %d cuts in place, %.12f solved afresh\n", plain, t.objective_function_value(), k,
                        fresh.objective_function_value());
            CHECK(near(t.objective_function_value(), fresh.objective_function_value()));
            CHECK(t.objective_function_value() > plain + 1e-6);
            // the refusals leave the handle as it was
            const std::vector<double> d3 = t.relative_costs();
            const double inf = std::numeric_limits<double>::infinity();
            CHECK_THROWS(t.add_cuts({0, 1}, {n}, {1.0}, {1.0}), RELP_E_ARG);           // a virtual column
            CHECK_THROWS(t.add_cuts({0, 1}, {-1}, {1.0}, {1.0}), RELP_E_ARG);
            CHECK_THROWS(t.add_cuts({0, 2}, {1, 1}, {1.0, 1.0}, {1.0}), RELP_E_ARG);   // named twice
            CHECK_THROWS(t.add_cuts({1, 2}, {0, 1}, {1.0, 1.0}, {1.0}), RELP_E_ARG);   // row_ptr not from 0
            CHECK_THROWS(t.add_cuts({0, 1}, {0}, {inf}, {1.0}), RELP_E_ARG);
            CHECK_THROWS(t.add_cuts({0, 1}, {0}, {1.0}, {std::numeric_limits<double>::quiet_NaN()}), RELP_E_ARG);
            CHECK_THROWS(t.reserve_cuts(-1), RELP_E_ARG);
            t.add_cuts({0}, {}, {}, {});                                               // count == 0: a no-op
            CHECK(t.relative_costs() == d3 && t.nr_rows() == m + k && t.cut_stats()[0] == 3);
        }
        {   // phase 1 and the other engines refuse
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 1}}, 2, {2, 1}, {}, 0, 0, 1, 1, {1, 1}), tableau);
            CHECK_THROWS(t.add_cuts({0, 1}, {0}, {1.0}, {1.0}), RELP_E_STATE);
            CHECK_THROWS(t.reserve_cuts(4), RELP_E_STATE);
            CHECK_THROWS(t.cut_stats(), RELP_E_STATE);
            Tableau lu(MatrixData::from_rows({{1, 1}}, 2, {3}, {}, 0, 0, 1, 0, {-1, -1}, {2, 2}),
                       Options().inverse_maintenance(InverseMaintenance::LUDecomposition));
            CHECK(lu.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK_THROWS(lu.add_cuts({0, 1}, {0}, {1.0}, {1.0}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(lu.reserve_cuts(4), RELP_E_UNSUPPORTED);
            CHECK_THROWS(lu.cut_stats(), RELP_E_UNSUPPORTED);
        }
    } catch (const std::exception& e) {
        std::printf("unexpected exception: %s\n", e.what());
        return 2;
    }
    return finish("test_cuts");
}
