// C++ host-side test of the in-place cost change over include/relp.hpp (no counterpart in the reference, which borrows an immutable
// provider): change_cost, set_cost, run, objective.  Runs on the GPU box: `tests/cpp/test_cost_in_place` (built by
// tests/cpp/Makefile, `__graft_entry__.build()`); exit code 0 = all checks passed.  tests/test_cpp_cost_in_place.py runs it
// under pytest (-m gpu).
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
        {   // min x1 + x2, x1 + x2 <= 2, x1 + x2 >= 1: optimum 1; c1 moved to 0.5 (optimum 0.5), to -1 (x1 = 2: -2) and all back
            Tableau t(MatrixData::from_rows({{1, 1}, {1, 1}}, 2, {2, 1}, {}, 0, 0, 1, 1, {1, 1}), tableau);
            CHECK_THROWS(t.change_cost({0}, {0.5}), RELP_E_STATE);                     // phase 1
            CHECK_THROWS(t.cost(), RELP_E_STATE);
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK(near(t.objective_function_value(), 1));
            CHECK(t.cost() == std::vector<double>({1, 1}));
            const std::vector<double> b = t.right_hand_side();
            t.change_cost({0}, {0.5});
            CHECK(t.cost() == std::vector<double>({0.5, 1}));
            CHECK(t.right_hand_side() == b);
            CHECK(t.run() == RELP_OPTIMAL);
            CHECK(near(t.objective_function_value(), 0.5));
            t.change_cost({0}, {-1});
            CHECK(t.run() == RELP_OPTIMAL);
            CHECK(near(t.objective_function_value(), -2));
            t.change_cost({1, 0}, {-3, -1});                                           // c1 unchanged: one nonzero delta
            CHECK(t.run() == RELP_OPTIMAL);
            CHECK(near(t.objective_function_value(), -6));
            CHECK(t.cost_stats()[0] == 3);
            t.set_cost({1, 1});
            CHECK(t.cost() == std::vector<double>({1, 1}));
            CHECK(t.run() == RELP_OPTIMAL);
            CHECK(near(t.objective_function_value(), 1));
            const std::vector<double> d = t.relative_costs();
            t.change_cost({}, {});                                                      // a no-op, not counted
            CHECK_THROWS(t.change_cost({2}, {1}), RELP_E_ARG);
            CHECK_THROWS(t.change_cost({-1}, {1}), RELP_E_ARG);
            CHECK_THROWS(t.change_cost({0, 0}, {1, 1}), RELP_E_ARG);
            CHECK_THROWS(t.change_cost({0}, {std::numeric_limits<double>::infinity()}), RELP_E_ARG);
            CHECK_THROWS(t.change_cost({0}, {std::numeric_limits<double>::quiet_NaN()}), RELP_E_ARG);
            CHECK_THROWS(t.set_cost({1}), RELP_E_ARG);
            CHECK_THROWS(t.set_cost({1, std::numeric_limits<double>::infinity()}), RELP_E_ARG);
            CHECK(t.relative_costs() == d);
            CHECK(t.cost() == std::vector<double>({1, 1}));
            CHECK(t.cost_stats()[0] == 3 && t.reinversions() == 0);
        }
        {   // the other engines refuse
            Tableau t(MatrixData::from_rows({{1, 1}}, 2, {3}, {}, 0, 0, 1, 0, {-1, -1}, {2, 2}),
                      Options().inverse_maintenance(InverseMaintenance::LUDecomposition));
            CHECK(t.solve_relaxation().kind == OptimizationResult::FiniteOptimum);
            CHECK_THROWS(t.change_cost({0}, {0.5}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(t.set_cost({1, 1}), RELP_E_UNSUPPORTED);
            CHECK_THROWS(t.cost(), RELP_E_UNSUPPORTED);
            CHECK_THROWS(t.cost_stats(), RELP_E_UNSUPPORTED);
        }
    } catch (const std::exception& e) {
        std::printf("unexpected exception: %s\n", e.what());
        return 2;
    }
    return finish("test_cost_in_place");
}
