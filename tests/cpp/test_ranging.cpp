// C++ host-side test of the batched ratio queries over include/relp.hpp (no counterpart in the reference): row_ratios, rhs_ranging,
// ranging_stats on one LP solved by hand, and the refusals.  Runs on the GPU box: `tests/cpp/test_ranging` (built by
// tests/cpp/Makefile, `__graft_entry__.build()`); exit code 0 = all checks passed.  tests/test_cpp_ranging.py runs it under pytest
// (-m gpu).
#include <cmath>
#include <cstdio>
#include <limits>

#include "relp.hpp"
#include "check.hpp"

using namespace relp_host;


static bool near(double a, double b) { return near(a, b, 1e-12); }

int main() {
    try {
        const Options tableau = Options().inverse_maintenance(InverseMaintenance::DenseTableau);
        const double inf = std::numeric_limits<double>::infinity();
        {   // min -x1 - 2 x2, x1 + x2 <= 4, x1 + 3 x2 <= 6: optimum -5 at x = (3, 1), both slacks (columns 2, 3) non-basic with
            // reduced cost 1/2; the rows of T are x1: [1 0 3/2 -1/2], x2: [0 1 -1/2 1/2]
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 3}}, 2, {4, 6}, {}, 0, 0, 2, 0, {-1, -2}), tableau);
            CHECK_THROWS(t.row_ratios({0}), RELP_E_STATE);                              // phase 1
            CHECK_THROWS(t.rhs_ranging({0}), RELP_E_STATE);
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK(near(t.objective_function_value(), -5));
            const std::vector<int32_t> basis = t.basis_indices();
            const std::vector<double> b = t.b(), d = t.relative_costs();
            const int32_t r1 = basis[0] == 0 ? 0 : 1, r2 = 1 - r1;                      // the rows of x1 and x2
            CHECK(basis[r1] == 0 && basis[r2] == 1);
            const Tableau::RowRatios rr = t.row_ratios({r1, r2, r1});
            // x1 keeps the basis optimal for its cost in [-1 - 1, -1 + 1/3], x2 for its cost in [-2 - 1, -2 + 1]
            CHECK(near(rr.down_ratio[0], 1) && rr.down_column[0] == 3 && near(rr.up_ratio[0], 1.0 / 3) && rr.up_column[0] == 2);
            CHECK(near(rr.down_ratio[1], 1) && rr.down_column[1] == 2 && near(rr.up_ratio[1], 1) && rr.up_column[1] == 3);
            CHECK(rr.down_ratio[2] == rr.down_ratio[0] && rr.up_column[2] == rr.up_column[0]);   // a row named twice
            // rhs_0 = 4 may move within [2, 6], rhs_1 = 6 within [4, 12]
            const Tableau::RhsRanging rg = t.rhs_ranging({0, 1});
            CHECK(near(rg.decrease[0], 2) && rg.decrease_row[0] == r1 && near(rg.increase[0], 2) && rg.increase_row[0] == r2);
            CHECK(near(rg.decrease[1], 2) && rg.decrease_row[1] == r2 && near(rg.increase[1], 6) && rg.increase_row[1] == r1);
            CHECK(t.ranging_stats()[0] == 1 && t.ranging_stats()[1] == 3 && t.ranging_stats()[2] == 1);
            // read-only
            CHECK(t.b() == b && t.relative_costs() == d && t.basis_indices() == basis && t.reinversions() == 0);
            // just past the decrease bound of rhs_0 the row of x1 leaves and column 3 enters, as reported
            t.change_right_hand_side({0}, {1.5});
            CHECK(t.run_dual() == RELP_OPTIMAL);
            CHECK(t.basis_indices()[r1] == 3);
            CHECK(near(t.objective_function_value(), -3));                              // x = (0, 1.5)
            CHECK_THROWS(t.row_ratios({2}), RELP_E_ARG);
            CHECK_THROWS(t.rhs_ranging({-1}), RELP_E_ARG);
            CHECK(t.row_ratios({}).down_ratio.empty());
        }
        {   // slack basis of a <= LP with A > 0: nothing bounds a move down of a slack or an increase of an rhs
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 3}}, 2, {4, 6}, {}, 0, 0, 2, 0, {-1, -2}), tableau);
            t.from_basis({2, 3});
            const Tableau::RowRatios rr = t.row_ratios({0, 1});
            CHECK(rr.down_ratio[0] == inf && rr.down_column[0] == -1 && rr.up_ratio[1] == 0 && rr.up_column[1] == 0);
            const Tableau::RhsRanging rg = t.rhs_ranging({1});
            CHECK(rg.decrease[0] == 6 && rg.decrease_row[0] == 1 && rg.increase[0] == inf && rg.increase_row[0] == -1);
        }
        {   // the other engines refuse
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 3}}, 2, {4, 6}, {}, 0, 0, 2, 0, {-1, -2}),
                      Options().inverse_maintenance(InverseMaintenance::LUDecomposition));
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK_THROWS(t.row_ratios({0}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(t.rhs_ranging({0}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(t.ranging_stats(), RELP_E_UNSUPPORTED);
        }
    } catch (const std::exception& e) {
        std::printf("unexpected exception: %s\n", e.what());
        return 2;
    }
    return finish("test_ranging");
}
