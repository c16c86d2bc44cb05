// test_layout_columns.cpp -- Layout::add_columns without a GPU (rust-lp_amd/csrc/relp_layout.{hpp,cpp}): columns from outside behind
// every column.  `make -C tests/cpp test_layout_columns`; exit code 0 = all checks passed.
//
// Pins, on a layout with an ==, a <= and a >= row and two bounded columns (in phase 2: no artificial columns in front):
//   * the indices of the new columns, and that m, rhs, the row classes, bound_row and every old descriptor stay;
//   * for_each_entry of an added column, rows ascending whatever the caller's order, explicit zeros dropped (the same entries
//     whether the column is basic or not: the basis is not the layout's business), and of the old columns;
//   * costs (cost_of), added_of;
//   * interleaved with add_cuts in both orders: columns, cuts, columns with entries in the cut rows; cuts, then columns;
//   * every RELP_E_ARG case leaves the layout equal to a copy taken before.
#include "relp_layout.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "check.hpp"

using namespace relp;
using Entries = std::vector<std::pair<int32_t, double>>;


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

static Entries column(const Layout& L, const Lp& lp, int32_t j) {
    Entries out;
    auto csc = [&](int32_t p, auto&& put) {
        for (int64_t e = lp.col_ptr[p]; e < lp.col_ptr[p + 1]; ++e) put(lp.row_idx[e], lp.values[e]);
    };
    if (!L.for_each_entry(j, csc, [&](int32_t r, double v) { out.emplace_back(r, v); })) out.emplace_back(-99, 0.0);
    return out;
}

static bool same(const Layout& a, const Layout& b) {
    return a.nr_normal == b.nr_normal && a.mc == b.mc && a.nr_bounds == b.nr_bounds && a.m == b.m && a.nr_virtual == b.nr_virtual &&
           a.n_provider == b.n_provider && a.cost == b.cost && a.rhs == b.rhs && a.bound_row == b.bound_row && a.vrow0 == b.vrow0 &&
           a.vrow1 == b.vrow1 && a.vsign == b.vsign && a.nr_cuts == b.nr_cuts && a.cut_row0 == b.cut_row0 && a.cut_entries == b.cut_entries &&
           a.nr_added == b.nr_added && a.added_virtual == b.added_virtual && a.added_slot == b.added_slot && a.added_entries == b.added_entries &&
           a.added_cost == b.added_cost && a.nr_artificial == b.nr_artificial && a.row_lo == b.row_lo && a.row_hi == b.row_hi &&
           a.row_stride == b.row_stride && a.sc_lo == b.sc_lo && a.sc_hi == b.sc_hi && a.candidate_len == b.candidate_len && a.basis == b.basis;
}

static Layout phase_two_layout(const Lp& lp) {
    Layout L;
    std::string err;
    relp_config_t cfg{};
    cfg.engine = RELP_ENGINE_TABLEAU; cfg.shard_count = 1;
    CHECK(L.build(lp.md(), cfg, &err) == RELP_OK);
    L.wrapped_na = L.nr_artificial;                     // as after the phase switch: provider columns are the tableau columns
    L.nr_artificial = 0;
    return L;
}

int main() {
    const Lp lp;
    std::string err;
    Layout L = phase_two_layout(lp);
    // rows: == 0 | <= 1 | >= 2 | bound rows 3 (x0), 4 (x2); virtual: <= slack, >= slack, two bound slacks
    CHECK(L.m == 5 && L.mc == 3 && L.nr_virtual == 4 && L.n_provider == 7 && L.nr_added == 0);
    CHECK(L.added_of(3) == -1 && L.cost_of(1) == 2.0 && L.cost_of(5) == 0.0);
    const Layout before = L;

    // ---- first add: two columns, the second with its rows in descending order and an explicit zero ----
    {
        const std::vector<int64_t> ptr{0, 2, 5};
        const std::vector<int32_t> idx{0, 4, 3, 2, 1};
        const std::vector<double> val{1.5, -2.0, 4.0, 0.0, 0.5}, cost{-3.0, 0.25};
        CHECK(L.add_columns(2, ptr.data(), idx.data(), val.data(), cost.data(), &err) == RELP_OK);
    }
    CHECK(L.nr_added == 2 && L.nr_virtual == 6 && L.n_provider == 9 && L.nr_columns() == 9);
    CHECK(L.m == 5 && L.mc == before.mc && L.rhs == before.rhs && L.bound_row == before.bound_row && L.cost == before.cost && L.nr_cuts == 0);
    CHECK(std::vector<int32_t>(L.vrow0.begin(), L.vrow0.begin() + 4) == before.vrow0 && L.vrow0[4] == -1 && L.vrow0[5] == -1);
    CHECK(L.vrow1[4] == -1 && L.vrow1[5] == -1 && L.vsign[4] == 1 && L.vsign[5] == 1);
    CHECK(L.row_lo == before.row_lo && L.row_hi == before.row_hi && L.candidate_len == before.candidate_len);
    CHECK(column(L, lp, 7) == Entries({{0, 1.5}, {4, -2.0}}));
    CHECK(column(L, lp, 8) == Entries({{1, 0.5}, {3, 4.0}}));                          // ascending, its 0.0 in row 2 is no entry
    CHECK(column(L, lp, 9) == Entries({{-99, 0.0}}));
    for (int32_t j = 0; j < 7; ++j) CHECK(column(L, lp, j) == column(before, lp, j));
    CHECK(L.added_of(7) == 0 && L.added_of(8) == 1 && L.added_of(6) == -1 && L.added_of(2) == -1 && L.added_of(9) == -1);
    CHECK(L.cost_of(7) == -3.0 && L.cost_of(8) == 0.25 && L.cost_of(6) == 0.0 && L.cost_of(0) == 1.0);
    {   // provider columns without artificial columns in front
        Entries out;
        CHECK(L.for_each_provider_entry(8, [](int32_t, auto&&) {}, [&](int32_t r, double v) { out.emplace_back(r, v); }));
        CHECK(out == Entries({{1, 0.5}, {3, 4.0}}));
    }

    // ---- cuts behind the columns: the cut slacks come behind the added columns, the added columns have no entry in the cut rows ----
    {
        const std::vector<int64_t> ptr{0, 2};
        const std::vector<int32_t> idx{0, 2};
        const std::vector<double> val{1.0, 2.0}, rhs{6.0};
        CHECK(L.add_cuts(1, ptr.data(), idx.data(), val.data(), rhs.data(), &err) == RELP_OK);
    }
    CHECK(L.m == 6 && L.nr_cuts == 1 && L.cut_row0 == 5 && L.nr_virtual == 7 && L.n_provider == 10 && L.nr_added == 2);
    CHECK(column(L, lp, 9) == Entries({{5, 1.0}}) && L.added_of(9) == -1 && L.cost_of(9) == 0.0);
    CHECK(column(L, lp, 7) == Entries({{0, 1.5}, {4, -2.0}}) && column(L, lp, 0) == Entries({{0, 1.0}, {1, 1.0}, {3, 1.0}, {5, 1.0}}));

    // ---- columns again, now with entries in the cut row; one without entries ----
    {
        const std::vector<int64_t> ptr{0, 2, 2};
        const std::vector<int32_t> idx{5, 0};
        const std::vector<double> val{7.0, 1.0}, cost{1.0, 2.0};
        CHECK(L.add_columns(2, ptr.data(), idx.data(), val.data(), cost.data(), &err) == RELP_OK);
    }
    CHECK(L.nr_added == 4 && L.nr_virtual == 9 && L.n_provider == 12 && L.m == 6);
    CHECK(column(L, lp, 10) == Entries({{0, 1.0}, {5, 7.0}}) && column(L, lp, 11).empty());
    CHECK(L.added_virtual == std::vector<int32_t>({4, 5, 7, 8}));
    CHECK(L.added_of(10) == 2 && L.added_of(11) == 3 && L.cost_of(11) == 2.0 && L.added_of(9) == -1);
    CHECK(column(L, lp, 9) == Entries({{5, 1.0}}) && column(L, lp, 8) == Entries({{1, 0.5}, {3, 4.0}}));

    // ---- the other order on a fresh layout: cuts, then columns ----
    {
        Layout M = phase_two_layout(lp);
        const std::vector<int64_t> cptr{0, 1};
        const std::vector<int32_t> cidx{1};
        const std::vector<double> cval{3.0}, crhs{2.0};
        CHECK(M.add_cuts(1, cptr.data(), cidx.data(), cval.data(), crhs.data(), &err) == RELP_OK);
        const std::vector<int64_t> ptr{0, 2};
        const std::vector<int32_t> idx{5, 2};
        const std::vector<double> val{-1.0, 2.0}, cost{4.0};
        CHECK(M.add_columns(1, ptr.data(), idx.data(), val.data(), cost.data(), &err) == RELP_OK);
        CHECK(M.m == 6 && M.n_provider == 9 && M.nr_added == 1 && M.nr_cuts == 1);
        CHECK(column(M, lp, 7) == Entries({{5, 1.0}}) && column(M, lp, 8) == Entries({{2, 2.0}, {5, -1.0}}));
        CHECK(M.added_of(7) == -1 && M.added_of(8) == 0 && M.cost_of(8) == 4.0);
        CHECK(M.add_cuts(1, cptr.data(), cidx.data(), cval.data(), crhs.data(), &err) == RELP_OK);      // and a cut behind them
        CHECK(M.added_of(9) == -1 && column(M, lp, 9) == Entries({{6, 1.0}}) && column(M, lp, 8) == Entries({{2, 2.0}, {5, -1.0}}));
    }

    // ---- every RELP_E_ARG case leaves the layout as it was; count == 0 too ----
    const Layout keep = L;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    struct Case { int32_t count; std::vector<int64_t> ptr; std::vector<int32_t> idx; std::vector<double> val, cost; bool no_ptr, no_idx, no_val, no_cost; };
    const std::vector<Case> bad = {
        {-1, {0, 1}, {0}, {1.0}, {1.0}, false, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, true, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, false, true, false, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, false, false, true, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, false, false, false, true},
        {1, {1, 2}, {0, 1}, {1.0, 1.0}, {1.0}, false, false, false, false},            // does not start at 0
        {2, {0, 2, 1}, {0, 1}, {1.0, 1.0}, {1.0, 1.0}, false, false, false, false},    // descends
        {1, {0, 1}, {-1}, {1.0}, {1.0}, false, false, false, false},
        {1, {0, 1}, {6}, {1.0}, {1.0}, false, false, false, false},                    // behind the last row (the cut row 5 is one)
        {1, {0, 2}, {2, 2}, {1.0, 1.0}, {1.0}, false, false, false, false},            // named twice in one column
        {1, {0, 1}, {0}, {nan}, {1.0}, false, false, false, false},
        {1, {0, 1}, {0}, {kInf}, {1.0}, false, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {-kInf}, false, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {nan}, false, false, false, false},
    };
    for (const Case& c : bad) {
        err.clear();
        CHECK(L.add_columns(c.count, c.no_ptr ? nullptr : c.ptr.data(), c.no_idx ? nullptr : c.idx.data(), c.no_val ? nullptr : c.val.data(),
                            c.no_cost ? nullptr : c.cost.data(), &err) == RELP_E_ARG);
        CHECK(!err.empty());
        CHECK(same(L, keep));
    }
    CHECK(L.add_columns(0, nullptr, nullptr, nullptr, nullptr, &err) == RELP_OK && same(L, keep));
    {   // the same row in two different columns is fine
        const std::vector<int64_t> ptr{0, 1, 2};
        const std::vector<int32_t> idx{2, 2};
        const std::vector<double> val{1.0, 2.0}, cost{1.0, 2.0};
        CHECK(L.add_columns(2, ptr.data(), idx.data(), val.data(), cost.data(), &err) == RELP_OK);
        CHECK(L.nr_added == 6 && column(L, lp, 12) == Entries({{2, 1.0}}) && column(L, lp, 13) == Entries({{2, 2.0}}));
    }
    return finish("test_layout_columns");
}
