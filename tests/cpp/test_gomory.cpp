// test_gomory.cpp -- the host side of relp_gomory_cuts without a GPU (rust-lp_amd/csrc/relp_gomory.hpp over relp_layout.{hpp,cpp}).
// `make -C tests/cpp`; exit code 0 = all checks passed.  The Makefile builds it a second time with
// -fsanitize=address,undefined (test_gomory_asan): it has its own main and needs no preload.
//
// Pins, on a layout with an ==, a <= and a >= row, two bounded columns and two cut rows (in phase 2):
//   * gomory_check_args: every RELP_E_ARG case of the header, and the arguments that are in order;
//   * gomory_entry: f0 and the statuses 3, 1, 2, 0 in that order of precedence, away = 0 and the edges of [away, 1 - away];
//   * gomory_slack_rows: which provider column is the slack of which row and with which sign (none for the equality), that a
//     removed row's slack and an added column are left out;
//   * gomory_beta: the fma chain from -f0 in ascending row order over the rows with y != 0 (against the same chain written out,
//     and against a sum whose order matters).
#include "relp_gomory.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "check.hpp"

using namespace relp;


static const double kInf = std::numeric_limits<double>::infinity();

// 3 structural columns, rows: x0 + 2 x1 == 4 | x0 + x2 <= 5 | x1 + 3 x2 >= 1; x0 <= 4, x2 <= 7
struct Lp {
    std::vector<int64_t> col_ptr{0, 2, 4, 6};
    std::vector<int32_t> row_idx{0, 1, 0, 2, 1, 2};
    std::vector<double> values{1, 1, 2, 1, 1, 3}, b{4, 5, 1}, cost{1, 2, 3}, upper{4, kInf, 7};
    relp_matrix_data_t md() const {
        relp_matrix_data_t d{};
        d.nr_normal = 3; d.nr_eq = 1; d.nr_le = 1; d.nr_ge = 1;
        d.format = RELP_FORMAT_CSC; d.matrix_memory = RELP_MEM_HOST;
        d.col_ptr = col_ptr.data(); d.row_idx = row_idx.data(); d.values = values.data();
        d.b = b.data(); d.cost = cost.data(); d.upper_bound = upper.data();
        return d;
    }
};

int main() {
    // ---- the argument checks ----
    {
        const int32_t rows[3] = {0, 4, 2}, low[1] = {-1}, high[2] = {0, 5};
        double c[1], r[1]; int32_t s[1];
        CHECK(gomory_check_args(rows, 3, 5, RELP_GOMORY_FRACTIONAL, 1e-6, c, r, s) == nullptr);
        CHECK(gomory_check_args(rows, 3, 5, RELP_GOMORY_MIXED, 0.0, c, r, s) == nullptr);
        CHECK(gomory_check_args(nullptr, 0, 5, 0, 0.25, nullptr, nullptr, nullptr) == nullptr);      // count == 0 needs no array
        CHECK(gomory_check_args(rows, -1, 5, 0, 1e-6, c, r, s) != nullptr);
        CHECK(gomory_check_args(low, 1, 5, 0, 1e-6, c, r, s) != nullptr);
        CHECK(gomory_check_args(high, 2, 5, 0, 1e-6, c, r, s) != nullptr);
        CHECK(gomory_check_args(rows, 3, 4, 0, 1e-6, c, r, s) != nullptr);                           // row 4 of 4 rows
        CHECK(gomory_check_args(rows, 3, 5, 2, 1e-6, c, r, s) != nullptr && gomory_check_args(rows, 3, 5, -1, 1e-6, c, r, s) != nullptr);
        for (double away : {-1e-12, 0.5, 0.75, kInf, -kInf, std::nan("")}) CHECK(gomory_check_args(rows, 3, 5, 0, away, c, r, s) != nullptr);
        CHECK(gomory_check_args(rows, 3, 5, 0, std::nextafter(0.5, 0.0), c, r, s) == nullptr);
        CHECK(gomory_check_args(nullptr, 3, 5, 0, 1e-6, c, r, s) != nullptr);
        CHECK(gomory_check_args(rows, 3, 5, 0, 1e-6, nullptr, r, s) != nullptr);
        CHECK(gomory_check_args(rows, 3, 5, 0, 1e-6, c, nullptr, s) != nullptr);
        CHECK(gomory_check_args(rows, 3, 5, 0, 1e-6, c, r, nullptr) != nullptr);
    }
    // ---- f0 and the statuses decided per entry ----
    {
        const uint8_t flags[4] = {1, 0, 1, 1};
        double f0 = -1.0;
        CHECK(gomory_entry(2.75, 0, flags, 4, 1e-6, &f0) == kGomoryCut && f0 == 0.75);
        CHECK(gomory_entry(-2.75, 0, nullptr, 4, 1e-6, &f0) == kGomoryCut && f0 == 0.25);           // floor, not truncation
        CHECK(gomory_entry(2.75, 1, flags, 4, 1e-6, &f0) == kGomoryNotInteger && f0 == 0.75);
        CHECK(gomory_entry(2.75, 1, nullptr, 4, 1e-6, &f0) == kGomoryCut);                          // NULL flags: all integer
        CHECK(gomory_entry(3.0, 0, flags, 4, 1e-6, &f0) == kGomoryFraction && f0 == 0.0);
        CHECK(gomory_entry(3.0, 0, flags, 4, 0.0, &f0) == kGomoryCut);                              // away = 0 skips nothing
        CHECK(gomory_entry(2.25, 0, flags, 4, 0.25, &f0) == kGomoryCut && gomory_entry(2.75, 0, flags, 4, 0.25, &f0) == kGomoryCut);
        CHECK(gomory_entry(2.125, 0, flags, 4, 0.25, &f0) == kGomoryFraction && gomory_entry(2.875, 0, flags, 4, 0.25, &f0) == kGomoryFraction);
        CHECK(gomory_entry(2.5, kWrappedArtificialBase + 3, flags, 4, 1e-6, &f0) == kGomoryArtificial && f0 == 0.5);
        CHECK(gomory_entry(3.0, INT32_MAX, flags, 4, 1e-6, &f0) == kGomoryArtificial);              // 3 comes before 1 and 2
        CHECK(gomory_entry(3.0, 1, flags, 4, 1e-6, &f0) == kGomoryNotInteger);                      // 1 comes before 2
        CHECK(gomory_entry(2.5, 4, flags, 4, 1e-6, &f0) == kGomoryArtificial && gomory_entry(2.5, -1, flags, 4, 1e-6, &f0) == kGomoryArtificial);
    }
    // ---- the rows whose slack carries a coefficient out of the cut ----
    {
        const Lp lp;
        Layout L;
        std::string err;
        relp_config_t cfg{};
        cfg.engine = RELP_ENGINE_TABLEAU; cfg.shard_count = 1;
        CHECK(L.build(lp.md(), cfg, &err) == RELP_OK);
        L.wrapped_na = L.nr_artificial;                     // as after the phase switch
        L.nr_artificial = 0;
        const std::vector<int64_t> ptr{0, 2, 3};
        const std::vector<int32_t> idx{0, 2, 1};
        const std::vector<double> val{1.5, -2.0, 7.0}, rhs{3.0, -1.0};
        CHECK(L.add_cuts(2, ptr.data(), idx.data(), val.data(), rhs.data(), &err) == RELP_OK);
        // rows: == 0 | <= 1 | >= 2 | bound rows 3 (x0), 4 (x2) | cut rows 5, 6; columns: 3 structural | <= | >= | 2 bound | 2 cut slacks
        std::vector<int32_t> column, sign;
        gomory_slack_rows(L, &column, &sign);
        CHECK(column == std::vector<int32_t>({-1, 3, 4, 5, 6, 7, 8}));
        CHECK(sign == std::vector<int32_t>({0, 1, -1, 1, 1, 1, 1}));
        CHECK(L.bound_row == std::vector<int32_t>({3, -1, 4}) && L.cut_row0 == 5 && L.mc == 3);
        // an added column has no row and takes none; a slack whose row was removed is left out
        const std::vector<int64_t> cptr{0, 2};
        const std::vector<int32_t> ridx{1, 5};
        const std::vector<double> cval{2.0, 1.0}, ccost{1.0};
        CHECK(L.add_columns(1, cptr.data(), ridx.data(), cval.data(), ccost.data(), &err) == RELP_OK);
        gomory_slack_rows(L, &column, &sign);
        CHECK(column == std::vector<int32_t>({-1, 3, 4, 5, 6, 7, 8}));
        L.vrow0[1] = -1;
        gomory_slack_rows(L, &column, &sign);
        CHECK(column == std::vector<int32_t>({-1, 3, -1, 5, 6, 7, 8}) && sign[2] == 0);
    }
    // ---- beta ----
    {
        const double y[5] = {0.0, 0.25, -0.0, -1.0 / 3.0, 0.1}, rhs[5] = {1e300, 5.0, kInf, 3.0, 7.0};
        double want = -0.4;
        want = std::fma(0.25, 5.0, want);
        want = std::fma(-1.0 / 3.0, 3.0, want);
        want = std::fma(0.1, 7.0, want);
        CHECK(gomory_beta(0.4, y, rhs, 5) == want);                                                  // rows with y == 0 (either sign) are not read into the sum
        CHECK(gomory_beta(0.4, y, rhs, 0) == -0.4 && gomory_beta(0.0, y, rhs, 1) == 0.0);
        // the order is the specification: 1e16 - 1e16 + 1 ascending is 1 - f0, any other order loses the 1 or keeps it differently
        const double y2[3] = {1.0, -1.0, 1.0}, rhs2[3] = {1e16, 1e16, 1.0};
        CHECK(gomory_beta(0.5, y2, rhs2, 3) == 1.0);                                                 // ((-0.5 + 1e16) - 1e16) + 1 = 0 + 1
    }
    return finish("test_gomory");
}
