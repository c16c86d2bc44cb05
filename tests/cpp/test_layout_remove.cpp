// test_layout_remove.cpp -- Layout::remove_cuts / remove_columns without a GPU (rust-lp_amd/csrc/relp_layout.{hpp,cpp}): cut rows and
// added columns taken back.  `make -C tests/cpp test_layout_remove`; exit code 0 = all checks passed.
//
// Pins, on the layout of test_layout_columns.cpp (an ==, a <= and a >= row, two bounded columns, phase 2):
//   * a layout that added cuts and columns interleaved (both orders) and then removed some of them EQUALS, member by member, the
//     layout that only ever added the survivors (with the rows of their entries renumbered), and for_each_entry of every column
//     agrees: the host LU and the re-tabulation see the smaller LP;
//   * cut numbers, the vrow0 of later slacks, added_virtual / added_slot and the rows of added_entries close up in order; cut_row0
//     stays; removing everything and adding again works;
//   * every refusal (RELP_E_ARG, RELP_E_STATE) leaves the layout equal to a copy taken before; count == 0 is a no-op.
#include "relp_layout.hpp"

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

// (added_slot is compared while there are added columns, cut_row0 and cut_entries while there are cuts: not read otherwise)
static bool same(const Layout& a, const Layout& b) {
    const bool slots = a.nr_added == 0 || a.added_slot == b.added_slot;
    return a.nr_normal == b.nr_normal && a.mc == b.mc && a.nr_bounds == b.nr_bounds && a.m == b.m && a.nr_virtual == b.nr_virtual &&
           a.n_provider == b.n_provider && a.cost == b.cost && a.rhs == b.rhs && a.bound_row == b.bound_row && a.vrow0 == b.vrow0 &&
           a.vrow1 == b.vrow1 && a.vsign == b.vsign && a.nr_cuts == b.nr_cuts &&
           (a.nr_cuts == 0 || (a.cut_row0 == b.cut_row0 && a.cut_entries == b.cut_entries)) && a.nr_added == b.nr_added && a.added_virtual == b.added_virtual && slots &&
           a.added_entries == b.added_entries && a.added_cost == b.added_cost && a.nr_artificial == b.nr_artificial && a.row_lo == b.row_lo &&
           a.row_hi == b.row_hi && a.row_stride == b.row_stride && a.sc_lo == b.sc_lo && a.sc_hi == b.sc_hi &&
           a.candidate_len == b.candidate_len && a.basis == b.basis;
}

static bool same_columns(const Layout& a, const Layout& b, const Lp& lp) {
    if (a.nr_columns() != b.nr_columns()) return false;
    for (int32_t j = 0; j <= a.nr_columns(); ++j)
        if (column(a, lp, j) != column(b, lp, j)) return false;
    return true;
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

// one cut over the structural columns (dense coefficients, zeros dropped), one column over the rows (row, value)
static void add_cut(Layout& L, const std::vector<double>& g, double rhs) {
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> idx;
    std::vector<double> val;
    for (int32_t p = 0; p < (int32_t)g.size(); ++p) if (g[p] != 0.0) { idx.push_back(p); val.push_back(g[p]); }
    ptr.push_back((int64_t)idx.size());
    std::string err;
    CHECK(L.add_cuts(1, ptr.data(), idx.data(), val.data(), &rhs, &err) == RELP_OK);
}
static void add_column(Layout& L, const Entries& entries, double cost) {
    std::vector<int64_t> ptr{0, (int64_t)entries.size()};
    std::vector<int32_t> idx;
    std::vector<double> val;
    for (const auto& e : entries) { idx.push_back(e.first); val.push_back(e.second); }
    std::string err;
    CHECK(L.add_columns(1, ptr.data(), idx.data(), val.data(), &cost, &err) == RELP_OK);
}

int main() {
    const Lp lp;
    std::string err;
    // rows: == 0 | <= 1 | >= 2 | bound rows 3 (x0), 4 (x2); provider columns 0-2 structural, 3-6 the slacks of build()

    // ---- cuts, columns, a cut, a column: provider columns c0 = 7, c1 = 8, x0 = 9, x1 = 10, c2 = 11, x2 = 12; cut rows 5, 6, 7 ----
    Layout L = phase_two_layout(lp);
    add_cut(L, {1.0, 0.0, 2.0}, 6.0);
    add_cut(L, {0.0, 3.0, 4.0}, 7.0);
    add_column(L, {{0, 1.5}, {5, -1.0}, {6, 2.5}}, -3.0);
    add_column(L, {{1, 0.5}, {6, 9.0}}, 0.25);
    add_cut(L, {5.0, 6.0, 0.0}, 8.0);
    add_column(L, {{3, 4.0}, {5, 1.0}, {7, -2.0}}, 1.0);
    CHECK(L.m == 8 && L.nr_cuts == 3 && L.cut_row0 == 5 && L.nr_added == 3 && L.n_provider == 13);
    CHECK(L.cut_slacks() == std::vector<int32_t>({4, 5, 8}));
    // a basis with the slacks of c1 and c2 (and x1) in it, c1's slack in a row that is not its own
    const std::vector<int32_t> basis{8, 0, 1, 5, 6, 3, 10, 11};
    const Layout big = L;

    {   // remove cut c1 (row 6): its slack 8 goes, x0 = 8, x1 = 9, c2 = 10 (row 6), x2 = 11
        const int32_t rows[1] = {6};
        CHECK(L.remove_cuts(rows, 1, basis, &err) == RELP_OK);
        Layout S = phase_two_layout(lp);
        add_cut(S, {1.0, 0.0, 2.0}, 6.0);
        add_column(S, {{0, 1.5}, {5, -1.0}}, -3.0);
        add_column(S, {{1, 0.5}}, 0.25);
        add_cut(S, {5.0, 6.0, 0.0}, 8.0);
        add_column(S, {{3, 4.0}, {5, 1.0}, {6, -2.0}}, 1.0);
        CHECK(same(L, S) && same_columns(L, S, lp));
        CHECK(L.m == 7 && L.nr_cuts == 2 && L.cut_row0 == 5 && L.rhs == std::vector<double>({4, 5, 1, 4, 7, 6, 8}));
        CHECK(L.added_virtual == std::vector<int32_t>({5, 6, 8}) && L.added_of(8) == 0 && L.added_of(10) == -1 && L.added_of(11) == 2);
        CHECK(column(L, lp, 10) == Entries({{6, 1.0}}) && column(L, lp, 0) == Entries({{0, 1.0}, {1, 1.0}, {3, 1.0}, {5, 1.0}, {6, 5.0}}));
        CHECK(L.cut_slacks() == std::vector<int32_t>({4, 7}));
    }
    {   // then the added column x0 (now provider column 8; the basis in the new numbering): x1 = 8, c2 = 9, x2 = 10
        const std::vector<int32_t> now{0, 1, 5, 6, 7, 9, 10};
        const int32_t cols[1] = {8};
        CHECK(L.remove_columns(cols, 1, now, &err) == RELP_OK);
        Layout S = phase_two_layout(lp);
        add_cut(S, {1.0, 0.0, 2.0}, 6.0);
        add_column(S, {{1, 0.5}}, 0.25);
        add_cut(S, {5.0, 6.0, 0.0}, 8.0);
        add_column(S, {{3, 4.0}, {5, 1.0}, {6, -2.0}}, 1.0);
        CHECK(same(L, S) && same_columns(L, S, lp));
        CHECK(L.cost_of(8) == 0.25 && L.cost_of(10) == 1.0 && L.cost_of(9) == 0.0 && L.nr_added == 2 && L.n_provider == 11);
        // add after remove: a cut and a column behind everything, as on the layout that never had the removed ones
        add_cut(L, {0.0, 1.0, 0.0}, 2.0); add_cut(S, {0.0, 1.0, 0.0}, 2.0);
        add_column(L, {{7, 3.0}, {2, 1.0}}, 5.0); add_column(S, {{7, 3.0}, {2, 1.0}}, 5.0);
        CHECK(same(L, S) && same_columns(L, S, lp) && L.m == 8 && L.cut_row0 == 5);
    }
    {   // several at once, unordered: cuts c2 and c0 (rows 7, 5), then columns x2 and x0 (12 - 2 = 10, 9 - 1 = 8)
        Layout M = big;
        const std::vector<int32_t> b2{8, 0, 1, 5, 6, 7, 10, 11};
        const int32_t rows[2] = {7, 5};
        CHECK(M.remove_cuts(rows, 2, b2, &err) == RELP_OK);
        const int32_t cols[2] = {10, 8};
        CHECK(M.remove_columns(cols, 2, {0, 1, 2, 3, 4, 5}, &err) == RELP_OK);
        Layout S = phase_two_layout(lp);
        add_cut(S, {0.0, 3.0, 4.0}, 7.0);
        add_column(S, {{1, 0.5}, {5, 9.0}}, 0.25);
        CHECK(same(M, S) && same_columns(M, S, lp));
    }
    {   // the other order of adding (columns first), and everything removed: the layout of build() again, and adding works after it
        Layout M = phase_two_layout(lp);
        const Layout fresh = M;
        add_column(M, {{0, 1.0}, {4, 2.0}}, 1.0);                    // 7
        add_cut(M, {1.0, 1.0, 1.0}, 9.0);                            // row 5, slack 8
        add_column(M, {{5, 3.0}}, 2.0);                              // 9
        add_cut(M, {0.0, 0.0, 1.0}, 3.0);                            // row 6, slack 10
        const int32_t cols[2] = {7, 9};
        CHECK(M.remove_columns(cols, 2, {0, 1, 2, 3, 4, 8, 10}, &err) == RELP_OK);
        {
            Layout S = phase_two_layout(lp);
            add_cut(S, {1.0, 1.0, 1.0}, 9.0);
            add_cut(S, {0.0, 0.0, 1.0}, 3.0);
            CHECK(same(M, S) && same_columns(M, S, lp));
        }
        const int32_t rows[2] = {5, 6};
        CHECK(M.remove_cuts(rows, 2, {0, 1, 2, 3, 4, 7, 8}, &err) == RELP_OK);
        CHECK(same(M, fresh) && same_columns(M, fresh, lp) && M.nr_cuts == 0 && M.nr_added == 0 && M.m == 5);
        add_cut(M, {2.0, 0.0, 0.0}, 1.0);
        add_column(M, {{5, 1.0}}, 1.0);
        Layout S = phase_two_layout(lp);
        add_cut(S, {2.0, 0.0, 0.0}, 1.0);
        add_column(S, {{5, 1.0}}, 1.0);
        CHECK(same(M, S) && same_columns(M, S, lp));
    }

    // ---- the refusals touch nothing ----
    {
        Layout M = big;
        struct Bad { std::vector<int32_t> list; int32_t count; bool null; relp_status_t want; };
        const std::vector<Bad> cuts = {
            {{6}, -1, false, RELP_E_ARG}, {{6}, 1, true, RELP_E_ARG}, {{4}, 1, false, RELP_E_ARG}, {{8}, 1, false, RELP_E_ARG},
            {{-1}, 1, false, RELP_E_ARG}, {{6, 6}, 2, false, RELP_E_ARG}, {{6, 7, 6}, 3, false, RELP_E_ARG},
            {{5}, 1, false, RELP_E_STATE},                               // the slack 7 of c0 is not in the basis
            {{6, 5}, 2, false, RELP_E_STATE},
        };
        for (const Bad& c : cuts) {
            err.clear();
            CHECK(M.remove_cuts(c.null ? nullptr : c.list.data(), c.count, basis, &err) == c.want);
            CHECK(!err.empty() && same(M, big));
        }
        const std::vector<Bad> cols = {
            {{9}, -1, false, RELP_E_ARG}, {{9}, 1, true, RELP_E_ARG}, {{2}, 1, false, RELP_E_ARG}, {{6}, 1, false, RELP_E_ARG},
            {{8}, 1, false, RELP_E_ARG},                                 // a cut slack is no added column
            {{13}, 1, false, RELP_E_ARG}, {{-3}, 1, false, RELP_E_ARG}, {{9, 9}, 2, false, RELP_E_ARG},
            {{10}, 1, false, RELP_E_STATE}, {{9, 10}, 2, false, RELP_E_STATE},           // x1 is basic
        };
        for (const Bad& c : cols) {
            err.clear();
            CHECK(M.remove_columns(c.null ? nullptr : c.list.data(), c.count, basis, &err) == c.want);
            CHECK(!err.empty() && same(M, big));
        }
        CHECK(M.remove_cuts(nullptr, 0, basis, &err) == RELP_OK && M.remove_columns(nullptr, 0, basis, &err) == RELP_OK && same(M, big));
        // phase 1: artificial columns in front
        Layout P = big;
        P.nr_artificial = 2;
        const Layout keep = P;
        const int32_t rows[1] = {6}, cs[1] = {9};
        CHECK(P.remove_cuts(rows, 1, basis, &err) == RELP_E_STATE && same(P, keep));
        CHECK(P.remove_columns(cs, 1, basis, &err) == RELP_E_STATE && same(P, keep));
        // a layout without cuts or added columns
        Layout F = phase_two_layout(lp);
        const Layout keep_f = F;
        CHECK(F.remove_cuts(rows, 1, {0, 1, 2, 3, 4}, &err) == RELP_E_ARG && F.remove_columns(cs, 1, {0, 1, 2, 3, 4}, &err) == RELP_E_ARG && same(F, keep_f));
    }
    return finish("test_layout_remove");
}
