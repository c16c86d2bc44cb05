// C++ host-side test of the in-place right-hand-side change over include/relp.hpp (no counterpart in the reference, which borrows an
// immutable provider): change, run_dual, objective.  Runs on the GPU box: `tests/cpp/test_rhs_in_place` (built by
// tests/cpp/Makefile, `__graft_entry__.build()`); exit code 0 = all checks passed.  tests/test_cpp_rhs_in_place.py runs it under
// pytest (-m gpu).
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
        {   // min x1 + x2, x1 + x2 <= 2, x1 + x2 >= 1: optimum 1; the >= row moved to 1.5, 4 (infeasible) and back
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 1}}, 2, {2, 1}, {}, 0, 0, 1, 1, {1, 1}), tableau);
            CHECK_THROWS(t.change_right_hand_side({1}, {1.5}), RELP_E_STATE);          // phase 1
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK(near(t.objective_function_value(), 1));
            const std::vector<double> d = t.relative_costs();
            t.change_right_hand_side({1}, {1.5});
            CHECK(t.right_hand_side() == std::vector<double>({2, 1.5}));
            CHECK(t.relative_costs() == d);
            CHECK(t.run_dual() == RELP_OPTIMAL);
            CHECK(near(t.objective_function_value(), 1.5));
            t.change_right_hand_side({1}, {4});
            CHECK(t.run_dual() == RELP_INFEASIBLE);
            t.change_right_hand_side({1}, {1});
            CHECK(t.run_dual() == RELP_OPTIMAL);
            CHECK(near(t.objective_function_value(), 1));
            CHECK(t.rhs_stats()[0] == 3 && t.rhs_stats()[1] == 3);
            CHECK_THROWS(t.change_right_hand_side({2}, {1}), RELP_E_ARG);
            CHECK_THROWS(t.change_right_hand_side({0, 0}, {1, 1}), RELP_E_ARG);
            CHECK_THROWS(t.set_upper_bound(0, 1), RELP_E_ARG);                          // no bound row
            CHECK(t.rhs_stats()[0] == 3 && t.reinversions() == 0);
        }
        {   // min -x1 - x2, x1 + x2 <= 3, x1 <= 2, x2 <= 2: optimum -3; x1 <= 0.5 leaves x = (0.5, 2)
            Tableau t(MatrixData::from_rows({{1, 1}}, 2, {3}, {}, 0, 0, 1, 0, {-1, -1}, {2, 2}), tableau);
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK(near(t.objective_function_value(), -3));
            t.set_upper_bound(0, 0.5);
            CHECK(t.right_hand_side() == std::vector<double>({3, 0.5, 2}));
            CHECK(t.run_dual() == RELP_OPTIMAL);
            CHECK(near(t.objective_function_value(), -2.5));
            CHECK(t.run() == RELP_OPTIMAL);
            CHECK_THROWS(t.set_upper_bound(2, 1), RELP_E_ARG);
            CHECK_THROWS(t.set_upper_bound(0, std::numeric_limits<double>::infinity()), RELP_E_ARG);
        }
        {   // the other engines refuse
            Tableau t(MatrixData::from_rows({{1, 1}}, 2, {3}, {}, 0, 0, 1, 0, {-1, -1}, {2, 2}),
                      Options().inverse_maintenance(InverseMaintenance::LUDecomposition));
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK_THROWS(t.set_upper_bound(0, 0.5), RELP_E_UNSUPPORTED);
            CHECK_THROWS(t.right_hand_side(), RELP_E_UNSUPPORTED);
        }
    } catch (const std::exception& e) {
        std::printf("unexpected exception: %s\n", e.what());
        return 2;
    }
    return finish("test_rhs_in_place");
}
