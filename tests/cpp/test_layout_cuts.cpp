// test_layout_cuts.cpp -- Layout::add_cuts without a GPU (rust-lp_amd/csrc/relp_layout.{hpp,cpp}): cut rows behind every row, their
// slacks behind every column.  `make -C tests/cpp test_layout_cuts`; exit code 0 = all checks passed.
//
// Pins, on a layout with an ==, a <= and a >= row and two bounded columns (in phase 2: no artificial columns in front):
//   * the indices of the new rows and columns, and that mc, the row classes, bound_row and every old descriptor stay;
//   * for_each_entry of structural, bound-slack and cut-slack columns, rows ascending, the structural callback asked for
//     constraint rows only;
//   * two successive adds;
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

static int g_rows_asked_max = -1;
static Entries column(const Layout& L, const Lp& lp, int32_t j) {
    Entries out;
    auto csc = [&](int32_t p, auto&& put) {
        for (int64_t e = lp.col_ptr[p]; e < lp.col_ptr[p + 1]; ++e) { g_rows_asked_max = std::max(g_rows_asked_max, lp.row_idx[e]); put(lp.row_idx[e], lp.values[e]); }
    };
    if (!L.for_each_entry(j, csc, [&](int32_t r, double v) { out.emplace_back(r, v); })) out.emplace_back(-99, 0.0);
    return out;
}

static bool ascending(const Entries& e) {
    for (size_t k = 1; k < e.size(); ++k) if (e[k].first <= e[k - 1].first) return false;
    return true;
}

static bool same(const Layout& a, const Layout& b) {
    return a.nr_normal == b.nr_normal && a.nr_eq == b.nr_eq && a.nr_range == b.nr_range && a.nr_le == b.nr_le && a.nr_ge == b.nr_ge && a.mc == b.mc &&
           a.nr_bounds == b.nr_bounds && a.m == b.m && a.nr_virtual == b.nr_virtual && a.n_provider == b.n_provider && a.cost == b.cost &&
           a.rhs == b.rhs && a.bound_row == b.bound_row && a.vrow0 == b.vrow0 && a.vrow1 == b.vrow1 && a.vsign == b.vsign &&
           a.nr_cuts == b.nr_cuts && a.cut_row0 == b.cut_row0 && a.cut_entries == b.cut_entries && a.nr_artificial == b.nr_artificial &&
           a.row_lo == b.row_lo && a.row_hi == b.row_hi && a.row_stride == b.row_stride && a.sc_lo == b.sc_lo && a.sc_hi == b.sc_hi &&
           a.candidate_len == b.candidate_len && a.basis == b.basis && a.column_to_row == b.column_to_row;
}

int main() {
    const Lp lp;
    Layout L;
    std::string err;
    relp_config_t cfg{};
    cfg.engine = RELP_ENGINE_TABLEAU; cfg.shard_count = 1;
    CHECK(L.build(lp.md(), cfg, &err) == RELP_OK);
    // rows: == 0 | <= 1 | >= 2 | bound rows 3 (x0), 4 (x2); virtual: <= slack, >= slack, two bound slacks
    CHECK(L.m == 5 && L.mc == 3 && L.nr_virtual == 4 && L.n_provider == 7);
    L.wrapped_na = L.nr_artificial;                     // as after the phase switch: provider columns are the tableau columns
    L.nr_artificial = 0;
    const Layout before = L;

    // ---- first add: two cuts, entries of the second cut in descending column order and with an explicit zero ----
    {
        const std::vector<int64_t> ptr{0, 2, 5};
        const std::vector<int32_t> idx{0, 2, 2, 1, 0};
        const std::vector<double> val{1.5, -2.0, 4.0, 0.0, 0.5}, rhs{3.0, -1.0};
        CHECK(L.add_cuts(2, ptr.data(), idx.data(), val.data(), rhs.data(), &err) == RELP_OK);
    }
    CHECK(L.nr_cuts == 2 && L.cut_row0 == 5 && L.m == 7 && L.nr_virtual == 6 && L.n_provider == 9 && L.nr_columns() == 9);
    CHECK(L.mc == before.mc && L.nr_eq == 1 && L.nr_le == 1 && L.nr_ge == 1 && L.nr_bounds == 2 && L.bound_row == before.bound_row);
    CHECK(L.rhs == std::vector<double>({4, 5, 1, 4, 7, 3, -1}));
    CHECK(std::vector<int32_t>(L.vrow0.begin(), L.vrow0.begin() + 4) == before.vrow0 && L.vrow0[4] == 5 && L.vrow0[5] == 6);
    CHECK(L.vrow1[4] == -1 && L.vrow1[5] == -1 && L.vsign[4] == 1 && L.vsign[5] == 1);
    CHECK(L.row_lo == 0 && L.row_hi == 7 && L.candidate_len >= 3 + 7);
    // structural columns: constraint rows, the bound row, the cut rows -- ascending; the callback supplies constraint rows only
    CHECK(column(L, lp, 0) == Entries({{0, 1.0}, {1, 1.0}, {3, 1.0}, {5, 1.5}, {6, 0.5}}));
    CHECK(column(L, lp, 1) == Entries({{0, 2.0}, {2, 1.0}}));                          // its 0.0 in cut 1 is no entry
    CHECK(column(L, lp, 2) == Entries({{1, 1.0}, {2, 3.0}, {4, 1.0}, {5, -2.0}, {6, 4.0}}));
    CHECK(g_rows_asked_max == 2);
    CHECK(column(L, lp, 3) == Entries({{1, 1.0}}));                                    // <= slack
    CHECK(column(L, lp, 4) == Entries({{2, -1.0}}));                                   // >= slack
    CHECK(column(L, lp, 5) == Entries({{3, 1.0}}) && column(L, lp, 6) == Entries({{4, 1.0}}));      // bound slacks
    CHECK(column(L, lp, 7) == Entries({{5, 1.0}}) && column(L, lp, 8) == Entries({{6, 1.0}}));      // cut slacks
    CHECK(column(L, lp, 9) == Entries({{-99, 0.0}}));
    for (int32_t j = 0; j < 9; ++j) CHECK(ascending(column(L, lp, j)));

    // ---- second add: one cut; cut_row0 stays ----
    {
        const std::vector<int64_t> ptr{0, 1};
        const std::vector<int32_t> idx{1};
        const std::vector<double> val{7.0}, rhs{0.25};
        CHECK(L.add_cuts(1, ptr.data(), idx.data(), val.data(), rhs.data(), &err) == RELP_OK);
    }
    CHECK(L.nr_cuts == 3 && L.cut_row0 == 5 && L.m == 8 && L.nr_virtual == 7 && L.n_provider == 10);
    CHECK(column(L, lp, 1) == Entries({{0, 2.0}, {2, 1.0}, {7, 7.0}}));
    CHECK(column(L, lp, 0) == Entries({{0, 1.0}, {1, 1.0}, {3, 1.0}, {5, 1.5}, {6, 0.5}}));
    CHECK(column(L, lp, 9) == Entries({{7, 1.0}}) && column(L, lp, 7) == Entries({{5, 1.0}}));
    CHECK(L.rhs.back() == 0.25 && L.rhs.size() == 8);
    // the basis [old rows' columns | cut slacks] has B with the cuts below: every column has its rows ascending
    for (int32_t j = 0; j < 10; ++j) CHECK(ascending(column(L, lp, j)));

    // ---- every RELP_E_ARG case leaves the layout as it was; count == 0 too ----
    const Layout keep = L;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    struct Case { int32_t count; std::vector<int64_t> ptr; std::vector<int32_t> idx; std::vector<double> val, rhs; bool no_ptr, no_idx, no_val, no_rhs; };
    const std::vector<Case> bad = {
        {-1, {0, 1}, {0}, {1.0}, {1.0}, false, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, true, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, false, true, false, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, false, false, true, false},
        {1, {0, 1}, {0}, {1.0}, {1.0}, false, false, false, true},
        {1, {1, 2}, {0, 1}, {1.0, 1.0}, {1.0}, false, false, false, false},            // does not start at 0
        {2, {0, 2, 1}, {0, 1}, {1.0, 1.0}, {1.0, 1.0}, false, false, false, false},    // descends
        {1, {0, 1}, {-1}, {1.0}, {1.0}, false, false, false, false},
        {1, {0, 1}, {3}, {1.0}, {1.0}, false, false, false, false},                    // a virtual column
        {1, {0, 2}, {2, 2}, {1.0, 1.0}, {1.0}, false, false, false, false},            // named twice in one cut
        {1, {0, 1}, {0}, {nan}, {1.0}, false, false, false, false},
        {1, {0, 1}, {0}, {kInf}, {1.0}, false, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {-kInf}, false, false, false, false},
        {1, {0, 1}, {0}, {1.0}, {nan}, false, false, false, false},
    };
    for (const Case& c : bad) {
        err.clear();
        CHECK(L.add_cuts(c.count, c.no_ptr ? nullptr : c.ptr.data(), c.no_idx ? nullptr : c.idx.data(), c.no_val ? nullptr : c.val.data(),
                         c.no_rhs ? nullptr : c.rhs.data(), &err) == RELP_E_ARG);
        CHECK(!err.empty());
        CHECK(same(L, keep));
    }
    CHECK(L.add_cuts(0, nullptr, nullptr, nullptr, nullptr, &err) == RELP_OK && same(L, keep));
    {   // the same column in two different cuts is fine, and so is a cut without entries
        const std::vector<int64_t> ptr{0, 1, 2, 2};
        const std::vector<int32_t> idx{2, 2};
        const std::vector<double> val{1.0, 2.0}, rhs{1.0, 2.0, 3.0};
        CHECK(L.add_cuts(3, ptr.data(), idx.data(), val.data(), rhs.data(), &err) == RELP_OK);
        CHECK(L.nr_cuts == 6 && L.m == 11);
        CHECK(column(L, lp, 2) == Entries({{1, 1.0}, {2, 3.0}, {4, 1.0}, {5, -2.0}, {6, 4.0}, {8, 1.0}, {9, 2.0}}));
        CHECK(column(L, lp, 12) == Entries({{10, 1.0}}));
    }
    return finish("test_layout_cuts");
}
