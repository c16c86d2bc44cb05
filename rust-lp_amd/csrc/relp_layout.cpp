// relp_layout.cpp -- the standard form of a relp_matrix_data_t.  See relp_layout.hpp.
#include "relp_layout.hpp"

#include <algorithm>
#include <cmath>

namespace relp {

static relp_status_t fail(std::string* err, relp_status_t code, const char* msg) {
    if (err) *err = msg;
    return code;
}

static int64_t round_up_even(int64_t v) { return (v + 1) & ~int64_t(1); }

void shard_column_range(int32_t n, int32_t rank, int32_t count, int32_t* lo, int32_t* hi) {
    if (count < 1) count = 1;
    const int32_t per = (n + count - 1) / count;
    const int32_t a = std::min(n, rank * per);
    if (lo) *lo = a;
    if (hi) *hi = std::min(n, a + per);
}

relp_status_t Layout::plan(const relp_matrix_data_t& md, const relp_config_t& cfg, std::string* err) {
    if (md.nr_normal < 0 || md.nr_eq < 0 || md.nr_range < 0 || md.nr_le < 0 || md.nr_ge < 0)
        return fail(err, RELP_E_ARG, "negative size");
    const int32_t G = std::max(cfg.shard_count, 1), g = cfg.shard_rank;
    if (g < 0 || g >= G) return fail(err, RELP_E_ARG, "bad shard rank");

    nr_normal = md.nr_normal; nr_eq = md.nr_eq; nr_range = md.nr_range; nr_le = md.nr_le; nr_ge = md.nr_ge;
    mc = nr_eq + nr_range + nr_le + nr_ge;
    bound_row.assign(nr_normal, -1);
    nr_bounds = 0;
    for (int32_t j = 0; j < nr_normal; ++j)
        if (md.upper_bound && std::isfinite(md.upper_bound[j])) bound_row[j] = mc + nr_bounds++;
    m = mc + nr_bounds + nr_range;
    engine = cfg.engine;
    if (engine == RELP_ENGINE_AUTO) {
        // INTEGRATION.md "which engine for which LP": the dense tableau while it fits comfortably, the LU engine beyond
        const double n_all = (double)nr_normal + nr_range + nr_le + nr_ge + nr_bounds + nr_range + m;       // (+ m: identity / artificial block)
        const bool fits = 8.0 * (double)m * n_all <= 64e9 && m <= 50000;
        engine = (G > 1 || fits) ? RELP_ENGINE_TABLEAU : RELP_ENGINE_LU;
    }
    if (m < 1) return fail(err, RELP_E_ARG, "empty problem");
    const int32_t row_start[7] = {0, nr_eq, nr_eq + nr_range, nr_eq + nr_range + nr_le, mc, mc + nr_bounds, m};
    nr_virtual = nr_range + nr_le + nr_ge + nr_bounds + nr_range;
    n_provider = nr_normal + nr_virtual;
    vrow0.clear(); vrow1.clear(); vsign.clear();
    auto slacks = [&](int32_t count, int32_t row, int32_t row1, int32_t sign) {
        for (int32_t k = 0; k < count; ++k) { vrow0.push_back(row + k); vrow1.push_back(row1 < 0 ? -1 : row1 + k); vsign.push_back(sign); }
    };
    slacks(nr_range, row_start[1], row_start[5], 1);      // range slack: its row and its range-bound row
    slacks(nr_le, row_start[2], -1, 1);
    slacks(nr_ge, row_start[3], -1, -1);
    slacks(nr_bounds, row_start[4], -1, 1);
    slacks(nr_range, row_start[5], -1, 1);                // range-bound slack

    // initial basis: <=-slacks, bound slacks, range-bound slacks are real pivots (matrix_data.rs:432-452);
    // every other row gets an artificial, numbered before all provider columns (partially.rs:72-80)
    std::vector<int32_t> real_row, real_col;
    const int32_t col_start2 = nr_normal + nr_range;                    // <= slacks
    const int32_t col_start4 = nr_normal + nr_range + nr_le + nr_ge;    // bound slacks
    const int32_t col_start5 = col_start4 + nr_bounds;                  // range-bound slacks
    for (int32_t k = 0; k < nr_le; ++k) { real_row.push_back(row_start[2] + k); real_col.push_back(col_start2 + k); }
    for (int32_t k = 0; k < nr_bounds; ++k) { real_row.push_back(row_start[4] + k); real_col.push_back(col_start4 + k); }
    for (int32_t k = 0; k < nr_range; ++k) { real_row.push_back(row_start[5] + k); real_col.push_back(col_start5 + k); }
    const int32_t nr_real = (int32_t)real_row.size();
    nr_artificial = m - nr_real;
    wrapped_na = 0;
    if (G > 1 && nr_artificial > 0 && engine != RELP_ENGINE_TABLEAU)
        return fail(err, RELP_E_UNSUPPORTED, "the sharded revised engine needs a full slack basis (no artificial variables); "
                                             "the sharded tableau engine runs both phases");
    column_to_row.assign(nr_artificial, 0);
    for (int32_t ith = 0, i = 0; ith < nr_artificial; ++ith) {
        while (i < nr_real && ith + i == real_row[i]) ++i;
        column_to_row[ith] = ith + i;
    }
    basis.assign(m, 0);
    for (int32_t row = 0, ac = 0; row < m; ++row) {
        const bool can_a = ac < nr_artificial, can_r = (row - ac) < nr_real;
        if (can_a && (!can_r || column_to_row[ac] < real_row[row - ac])) basis[row] = ac++;
        else basis[row] = nr_artificial + real_col[row - ac];
    }
    plan_shards(G, g);
    return RELP_OK;
}

relp_status_t Layout::build(const relp_matrix_data_t& md, const relp_config_t& cfg, std::string* err) {
    if (md.nr_normal < 0 || md.nr_eq < 0 || md.nr_range < 0 || md.nr_le < 0 || md.nr_ge < 0)
        return fail(err, RELP_E_ARG, "negative size");
    if (cfg.shard_rank < 0 || cfg.shard_rank >= std::max(cfg.shard_count, 1)) return fail(err, RELP_E_ARG, "bad shard rank");
    const int32_t mc_in = md.nr_eq + md.nr_range + md.nr_le + md.nr_ge;
    if ((mc_in > 0 && !md.b) || (md.nr_normal > 0 && (!md.cost || !md.upper_bound)) || (md.nr_range > 0 && !md.ranges))
        return fail(err, RELP_E_ARG, "missing b / cost / upper_bound / ranges");
    const relp_status_t st = plan(md, cfg, err);
    if (st) return st;

    cost.assign(md.cost, md.cost + nr_normal);
    rhs.assign(m, 0.0);
    for (int32_t i = 0; i < mc; ++i) rhs[i] = md.b[i];
    for (int32_t j = 0; j < nr_normal; ++j) if (bound_row[j] >= 0) rhs[bound_row[j]] = md.upper_bound[j];
    for (int32_t k = 0; k < nr_range; ++k) rhs[mc + nr_bounds + k] = md.ranges[k];
    // Carry::create_for_partially_artificial, carry/mod.rs:381-426
    minus_pi.assign(m, 0.0);
    phase1_objective = 0.0;
    for (int32_t k = 0; k < nr_artificial; ++k) { phase1_objective += rhs[column_to_row[k]]; minus_pi[column_to_row[k]] = -1.0; }
    return RELP_OK;
}

int64_t Layout::candidate_len_for(int32_t rows) const {
    return round_up_even(3 + (int64_t)rows + (engine == RELP_ENGINE_TABLEAU ? (rows + 255) / 256 : 0));
}

void Layout::plan_shards(int32_t G, int32_t g) {
    // structural columns and rows of B^-1
    shard_column_range(nr_normal, g, G, &col_lo, &col_hi);
    row_stride = (int32_t)round_up_even((m + G - 1) / G);
    row_lo = std::min(m, g * row_stride);
    row_hi = std::min(m, row_lo + row_stride);
    candidate_len = candidate_len_for(m);
    sc_lo = sc_hi = 0;
    if (engine == RELP_ENGINE_TABLEAU) {
        // the tableau shards its STORED columns [artificial | structural | virtual] contiguously; the
        // structural part of the owned range is what the caller supplies in `dense`
        const int32_t n_store = nr_columns();
        const int32_t per = (int32_t)round_up_even((n_store + G - 1) / G);
        sc_lo = std::min(n_store, g * per);
        sc_hi = std::min(n_store, sc_lo + per);
        col_lo = std::min(nr_normal, std::max(0, sc_lo - nr_artificial));
        col_hi = std::min(nr_normal, std::max(0, sc_hi - nr_artificial));
        if (col_hi < col_lo) col_hi = col_lo;
    }
}

void Layout::remove_rows(const std::vector<int32_t>& map) {
    auto remap = [&](std::vector<int32_t>& v) { for (auto& x : v) if (x >= 0) x = map[x]; };
    remap(bound_row); remap(vrow0); remap(vrow1);
    // a slack whose row disappears keeps its column index and becomes an empty column (vrow0 = -1), as
    // Column::into_filtered does (matrix_data.rs:592-614)
    for (auto& x : column_to_row) x = map[x] >= 0 ? map[x] : 0;
    int32_t kept = 0, kept_constraints = 0;
    for (int32_t i = 0; i < m; ++i) {
        if (map[i] < 0) continue;
        rhs[kept++] = rhs[i];
        if (i < mc) ++kept_constraints;
    }
    rhs.resize(kept);
    m = kept; mc = kept_constraints;
    row_lo = 0; row_hi = m;
    row_stride = (int32_t)round_up_even(m);
    candidate_len = candidate_len_for(m);
}

relp_status_t Layout::check_cuts(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* cut_rhs,
                                 std::string* err) const {
    if (count < 0) return fail(err, RELP_E_ARG, "relp_add_cuts: count < 0");
    if (count == 0) return RELP_OK;
    if (!row_ptr || !cut_rhs) return fail(err, RELP_E_ARG, "relp_add_cuts: row_ptr or rhs missing");
    if (row_ptr[0] != 0) return fail(err, RELP_E_ARG, "relp_add_cuts: row_ptr does not start at 0");
    for (int32_t k = 0; k < count; ++k)
        if (row_ptr[k + 1] < row_ptr[k]) return fail(err, RELP_E_ARG, "relp_add_cuts: row_ptr does not ascend");
    if (row_ptr[count] > 0 && (!col_idx || !values)) return fail(err, RELP_E_ARG, "relp_add_cuts: col_idx or values missing");
    std::vector<int32_t> named(nr_normal, -1);         // the last cut that named the column
    for (int32_t k = 0; k < count; ++k) {
        if (!std::isfinite(cut_rhs[k])) return fail(err, RELP_E_ARG, "relp_add_cuts: a right-hand side that is not finite");
        for (int64_t e = row_ptr[k]; e < row_ptr[k + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= nr_normal) return fail(err, RELP_E_ARG, "relp_add_cuts: not a structural column");
            if (named[col_idx[e]] == k) return fail(err, RELP_E_ARG, "relp_add_cuts: a column named twice in one cut");
            if (!std::isfinite(values[e])) return fail(err, RELP_E_ARG, "relp_add_cuts: a coefficient that is not finite");
            named[col_idx[e]] = k;
        }
    }
    return RELP_OK;
}

relp_status_t Layout::add_cuts(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* cut_rhs,
                               std::string* err) {
    const relp_status_t st = check_cuts(count, row_ptr, col_idx, values, cut_rhs, err);
    if (st || count == 0) return st;
    if (nr_cuts == 0) { cut_row0 = m; cut_entries.assign(nr_normal, {}); }
    for (int32_t k = 0; k < count; ++k) {
        for (int64_t e = row_ptr[k]; e < row_ptr[k + 1]; ++e)
            if (values[e] != 0.0) cut_entries[col_idx[e]].emplace_back(nr_cuts + k, values[e]);      // (ascending by cut: k ascends)
        rhs.push_back(cut_rhs[k]);
        vrow0.push_back(m + k); vrow1.push_back(-1); vsign.push_back(1);
        if (nr_added > 0) added_slot.push_back(-1);
    }
    nr_cuts += count; m += count; nr_virtual += count; n_provider += count;
    row_lo = 0; row_hi = m;
    row_stride = (int32_t)round_up_even(m);
    candidate_len = candidate_len_for(m);
    return RELP_OK;
}

relp_status_t Layout::check_columns(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* col_cost,
                                    std::string* err) const {
    if (count < 0) return fail(err, RELP_E_ARG, "relp_add_columns: count < 0");
    if (count == 0) return RELP_OK;
    if (!col_ptr || !col_cost) return fail(err, RELP_E_ARG, "relp_add_columns: col_ptr or cost missing");
    if (col_ptr[0] != 0) return fail(err, RELP_E_ARG, "relp_add_columns: col_ptr does not start at 0");
    for (int32_t k = 0; k < count; ++k)
        if (col_ptr[k + 1] < col_ptr[k]) return fail(err, RELP_E_ARG, "relp_add_columns: col_ptr does not ascend");
    if (col_ptr[count] > 0 && (!row_idx || !values)) return fail(err, RELP_E_ARG, "relp_add_columns: row_idx or values missing");
    std::vector<int32_t> named(m, -1);                 // the last column that named the row
    for (int32_t k = 0; k < count; ++k) {
        if (!std::isfinite(col_cost[k])) return fail(err, RELP_E_ARG, "relp_add_columns: a cost that is not finite");
        for (int64_t e = col_ptr[k]; e < col_ptr[k + 1]; ++e) {
            if (row_idx[e] < 0 || row_idx[e] >= m) return fail(err, RELP_E_ARG, "relp_add_columns: row out of range");
            if (named[row_idx[e]] == k) return fail(err, RELP_E_ARG, "relp_add_columns: a row named twice in one column");
            if (!std::isfinite(values[e])) return fail(err, RELP_E_ARG, "relp_add_columns: a coefficient that is not finite");
            named[row_idx[e]] = k;
        }
    }
    return RELP_OK;
}

relp_status_t Layout::add_columns(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* col_cost,
                                  std::string* err) {
    const relp_status_t st = check_columns(count, col_ptr, row_idx, values, col_cost, err);
    if (st || count == 0) return st;
    if (nr_added == 0) added_slot.assign(nr_virtual, -1);
    for (int32_t k = 0; k < count; ++k) {
        std::vector<std::pair<int32_t, double>> entries;
        for (int64_t e = col_ptr[k]; e < col_ptr[k + 1]; ++e)
            if (values[e] != 0.0) entries.emplace_back(row_idx[e], values[e]);
        std::sort(entries.begin(), entries.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        added_entries.push_back(std::move(entries));
        added_cost.push_back(col_cost[k]);
        added_virtual.push_back(nr_virtual + k);
        added_slot.push_back(nr_added + k);
        vrow0.push_back(-1); vrow1.push_back(-1); vsign.push_back(1);
    }
    nr_added += count; nr_virtual += count; n_provider += count;
    return RELP_OK;
}

std::vector<int32_t> Layout::cut_slacks() const {
    std::vector<int32_t> slack(nr_cuts, -1);
    if (nr_cuts > 0)
        for (int32_t v = 0; v < nr_virtual; ++v)
            if (vrow0[v] >= cut_row0) slack[vrow0[v] - cut_row0] = v;       // (every row from cut_row0 on is a cut row)
    return slack;
}

relp_status_t Layout::check_remove_cuts(const int32_t* rows, int32_t count, const std::vector<int32_t>& basis_now, std::string* err) const {
    if (count < 0) return fail(err, RELP_E_ARG, "relp_remove_cuts: count < 0");
    if (count == 0) return RELP_OK;
    if (!rows) return fail(err, RELP_E_ARG, "relp_remove_cuts: rows missing");
    std::vector<uint8_t> named(nr_cuts, 0);
    for (int32_t x = 0; x < count; ++x) {
        if (nr_cuts == 0 || rows[x] < cut_row0 || rows[x] >= cut_row0 + nr_cuts) return fail(err, RELP_E_ARG, "relp_remove_cuts: not a cut row");
        if (named[rows[x] - cut_row0]) return fail(err, RELP_E_ARG, "relp_remove_cuts: a row named twice");
        named[rows[x] - cut_row0] = 1;
    }
    if (nr_artificial > 0) return fail(err, RELP_E_STATE, "relp_remove_cuts: phase 1");
    std::vector<uint8_t> basic(nr_virtual, 0);
    for (int32_t j : basis_now)
        if (j >= nr_normal && j < n_provider) basic[j - nr_normal] = 1;
    const std::vector<int32_t> slack = cut_slacks();
    for (int32_t k = 0; k < nr_cuts; ++k)
        if (named[k] && (slack[k] < 0 || !basic[slack[k]]))
            return fail(err, RELP_E_STATE, "relp_remove_cuts: the slack of a cut is not basic (the cut is tight: pivot its slack in, or relax it)");
    return RELP_OK;
}

relp_status_t Layout::check_remove_columns(const int32_t* columns, int32_t count, const std::vector<int32_t>& basis_now, std::string* err) const {
    if (count < 0) return fail(err, RELP_E_ARG, "relp_remove_columns: count < 0");
    if (count == 0) return RELP_OK;
    if (!columns) return fail(err, RELP_E_ARG, "relp_remove_columns: columns missing");
    std::vector<uint8_t> named(nr_added, 0);
    for (int32_t x = 0; x < count; ++x) {
        const int32_t a = added_of(columns[x]);
        if (a < 0) return fail(err, RELP_E_ARG, "relp_remove_columns: not a column added by relp_add_columns");
        if (named[a]) return fail(err, RELP_E_ARG, "relp_remove_columns: a column named twice");
        named[a] = 1;
    }
    if (nr_artificial > 0) return fail(err, RELP_E_STATE, "relp_remove_columns: phase 1");
    for (int32_t j : basis_now) {
        const int32_t a = added_of(j);
        if (a >= 0 && named[a]) return fail(err, RELP_E_STATE, "relp_remove_columns: a column that is basic");
    }
    return RELP_OK;
}

void Layout::drop_virtuals(const std::vector<uint8_t>& gone_v, const std::vector<uint8_t>& gone_a) {
    std::vector<int32_t> a_map(nr_added, -1);
    int32_t kept_a = 0;
    for (int32_t a = 0; a < nr_added; ++a) {
        if (gone_a[a]) continue;
        if (kept_a != a) { added_entries[kept_a] = std::move(added_entries[a]); added_cost[kept_a] = added_cost[a]; }
        a_map[a] = kept_a++;
    }
    added_entries.resize(kept_a); added_cost.resize(kept_a); added_virtual.assign(kept_a, -1);
    const bool slots = nr_added > 0;
    int32_t kept_v = 0;
    for (int32_t v = 0; v < nr_virtual; ++v) {
        if (gone_v[v]) continue;
        vrow0[kept_v] = vrow0[v]; vrow1[kept_v] = vrow1[v]; vsign[kept_v] = vsign[v];
        if (slots) {
            const int32_t a = added_slot[v] >= 0 ? a_map[added_slot[v]] : -1;
            added_slot[kept_v] = a;
            if (a >= 0) added_virtual[a] = kept_v;
        }
        ++kept_v;
    }
    vrow0.resize(kept_v); vrow1.resize(kept_v); vsign.resize(kept_v);
    if (slots) added_slot.resize(kept_v);
    n_provider -= nr_virtual - kept_v;
    nr_virtual = kept_v; nr_added = kept_a;
}

relp_status_t Layout::remove_cuts(const int32_t* rows, int32_t count, const std::vector<int32_t>& basis_now, std::string* err) {
    const relp_status_t st = check_remove_cuts(rows, count, basis_now, err);
    if (st || count == 0) return st;
    const std::vector<int32_t> slack = cut_slacks();
    std::vector<int32_t> cut_map(nr_cuts, 0);          // cut -> its new number, -1 = removed
    std::vector<uint8_t> gone_v(nr_virtual, 0);
    for (int32_t x = 0; x < count; ++x) { cut_map[rows[x] - cut_row0] = -1; gone_v[slack[rows[x] - cut_row0]] = 1; }
    int32_t kept = 0;
    for (int32_t k = 0; k < nr_cuts; ++k)
        if (cut_map[k] >= 0) { cut_map[k] = kept; rhs[cut_row0 + kept] = rhs[cut_row0 + k]; ++kept; }
    rhs.resize(cut_row0 + kept);
    auto keep_entries = [&](std::vector<std::pair<int32_t, double>>& entries, int32_t first) {       // first: the index of cut 0 in `entries`
        size_t o = 0;
        for (const auto& e : entries) {
            if (e.first < first) { entries[o++] = e; continue; }
            if (cut_map[e.first - first] >= 0) entries[o++] = {first + cut_map[e.first - first], e.second};
        }
        entries.resize(o);
    };
    for (auto& entries : cut_entries) keep_entries(entries, 0);
    for (auto& entries : added_entries) keep_entries(entries, cut_row0);
    for (int32_t v = 0; v < nr_virtual; ++v)
        if (!gone_v[v] && vrow0[v] >= cut_row0) vrow0[v] = cut_row0 + cut_map[vrow0[v] - cut_row0];
    drop_virtuals(gone_v, std::vector<uint8_t>(nr_added, 0));
    nr_cuts = kept; m = cut_row0 + kept;
    row_lo = 0; row_hi = m;
    row_stride = (int32_t)round_up_even(m);
    candidate_len = candidate_len_for(m);
    return RELP_OK;
}

relp_status_t Layout::remove_columns(const int32_t* columns, int32_t count, const std::vector<int32_t>& basis_now, std::string* err) {
    const relp_status_t st = check_remove_columns(columns, count, basis_now, err);
    if (st || count == 0) return st;
    std::vector<uint8_t> gone_v(nr_virtual, 0), gone_a(nr_added, 0);
    for (int32_t x = 0; x < count; ++x) { gone_v[columns[x] - nr_normal] = 1; gone_a[added_of(columns[x])] = 1; }
    drop_virtuals(gone_v, gone_a);
    return RELP_OK;
}

}  // namespace relp
