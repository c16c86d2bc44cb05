// relp_layout.hpp -- the standard form of a relp_matrix_data_t, decided once on the host (plain C++17, no HIP).
//
// `Layout` is what the reference's `MatrixData` provider and the partially artificial start describe (file:line under the
// reference's src/algorithm/two_phase/):
//   rows, columns, right-hand side     matrix_provider/matrix_data.rs:198-268, 359-371, 432-452
//   artificial columns, initial basis  tableau/kind/artificial/partially.rs:72-80, 125-206
//   phase-1 -pi and objective          tableau/inverse_maintenance/carry/mod.rs:381-426
// plus the engine kind (RELP_ENGINE_AUTO resolved) and the split of the columns over shards.  The engine keeps one and
// uploads its arrays; relp_shard_plan asks the same code which columns a rank must supply.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/relp_engine.h"

namespace relp {

// Column indices at or above this value are artificial variables that survived phase 1 (see
// Engine::switch_to_phase_two): INT32_MAX - (na - 1 - a).  They have no flag, no cost and no column.
static constexpr int32_t kWrappedArtificialBase = 0x40000000;

// Structural columns [lo, hi) of `rank` when `count` ranks split `n` columns contiguously (relp_shard_column_range)
void shard_column_range(int32_t n, int32_t rank, int32_t count, int32_t* lo, int32_t* hi);

struct Layout {
    // rows: == | range | <= | >= (the mc constraints) | bound rows | range-bound rows  (m in all)
    int32_t nr_normal = 0, nr_eq = 0, nr_range = 0, nr_le = 0, nr_ge = 0;
    int32_t mc = 0;           // constraint rows of A
    int32_t nr_bounds = 0;    // variables with an upper bound
    int32_t m = 0;            // tableau rows
    // provider columns: structural | range slack | <= slack | >= slack | bound slack | range-bound slack
    int32_t nr_virtual = 0;
    int32_t n_provider = 0;   // structural + virtual
    std::vector<double> cost;                 // per structural column
    std::vector<double> rhs;                  // (b, upper bounds, ranges), matrix_data.rs:359-371
    std::vector<int32_t> bound_row;           // per structural column: its bound row, -1 = none
    std::vector<int32_t> vrow0, vrow1, vsign; // per virtual column: its row (-1: removed), the second row or -1, the sign
    int32_t engine = RELP_ENGINE_AUTO;        // relp_engine_kind_t, AUTO resolved
    // cut rows added behind every other row (relp_add_cuts): cut k is row cut_row0 + k, its slack the k-th virtual column behind
    // the ones of build() that is no added column; cut_row0 is fixed at the first add: the phase switch removes rows before any cut,
    // and relp_remove_cuts removes cut rows only (the cuts behind a removed one move down a number, cut_row0 stays)
    int32_t nr_cuts = 0, cut_row0 = 0;
    std::vector<std::vector<std::pair<int32_t, double>>> cut_entries;   // per structural column: (cut, coefficient != 0), ascending by cut
    // columns added behind every other column (relp_add_columns): the a-th added column is the virtual column added_virtual[a] with
    // the empty descriptor of a removed row (vrow0 = vrow1 = -1: device code reads an empty column); its entries (row, coefficient
    // != 0, rows ascending) and its cost are kept here.  added_slot: per virtual column its a, or -1 (empty while nothing was added)
    int32_t nr_added = 0;
    std::vector<int32_t> added_virtual, added_slot;
    std::vector<std::vector<std::pair<int32_t, double>>> added_entries;
    std::vector<double> added_cost;

    // Kind: the artificial columns are numbered before all provider columns
    int32_t nr_artificial = 0;                // 0 from phase 2 on
    int32_t wrapped_na = 0;                   // nr_artificial at the phase switch (decodes wrapped artificial indices)
    std::vector<int32_t> column_to_row;       // row of artificial column k
    std::vector<int32_t> basis;               // initial basis (tableau column indices)
    std::vector<double> minus_pi;             // initial -pi of phase 1
    double phase1_objective = 0.0;            // initial objective of phase 1 (the sum of the artificial rows' rhs)

    // shards: structural columns [col_lo, col_hi) and rows of B^-1 [row_lo, row_hi) (revised engine); the tableau engine
    // stores the columns [sc_lo, sc_hi) of [artificial | structural | virtual] and supplies the structural ones among them
    int32_t col_lo = 0, col_hi = 0, row_lo = 0, row_hi = 0, row_stride = 0;
    int32_t sc_lo = 0, sc_hi = 0;
    int64_t candidate_len = 0;                // [key, j, d_j, column (m)] (+ the tableau's block minima of the ratio test)

    // Counts, descriptors, engine kind, artificial columns, initial basis and shards from md's sizes and upper bounds
    // alone (b, cost and ranges are not read).  A status other than RELP_OK comes with a message in *err.
    relp_status_t plan(const relp_matrix_data_t& md, const relp_config_t& cfg, std::string* err);
    // The whole standard form: plan() plus cost, rhs, -pi and the phase-1 objective.
    relp_status_t build(const relp_matrix_data_t& md, const relp_config_t& cfg, std::string* err);
    // Rows deleted (map: old row -> new row, -1 = removed; only constraint rows go): every remaining row index shifts
    // down (Column::into_filtered, matrix_data.rs:592-614), rhs loses the rows, the shards own all rows.
    void remove_rows(const std::vector<int32_t>& map);
    // `count` cuts  sum_e values[e] x[col_idx[e]] <= cut_rhs[k]  (e in [row_ptr[k], row_ptr[k + 1])) over the structural columns, as
    // rows behind every existing row, each with a +1 slack behind every existing column: appends to rhs, vrow0 (the cut row),
    // vrow1 (-1) and vsign (+1), raises m, nr_virtual and n_provider; mc, the row classes, bound_row and every existing index stay.
    // check_cuts decides the RELP_E_ARG cases alone; add_cuts runs it first and touches nothing when it fails.
    relp_status_t check_cuts(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* cut_rhs,
                             std::string* err) const;
    relp_status_t add_cuts(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* cut_rhs,
                           std::string* err);

    // `count` columns x >= 0 in CSC over the rows in their current order (cut and bound rows included), cost[k] each, behind every
    // existing column: appends an empty descriptor per column to vrow0 / vrow1 / vsign, keeps entries and costs (above), raises
    // nr_virtual and n_provider; m, rhs, the rows and every existing index stay.  An explicit zero is dropped, the entries of a
    // column are kept by ascending row whatever the caller's order.  check_columns decides the RELP_E_ARG cases alone; add_columns
    // runs it first and touches nothing when it fails.
    relp_status_t check_columns(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* col_cost,
                                std::string* err) const;
    relp_status_t add_columns(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* col_cost,
                              std::string* err);
    // Cut rows taken back (relp_remove_cuts): `rows` are engine rows in [cut_row0, cut_row0 + nr_cuts), each once, each with its slack
    // in `basis` (the current basis as tableau columns, one per row).  The constraint goes from rhs, cut_entries and the entries the
    // added columns hold in it, its slack from the virtual columns; both index spaces close up in order: cut numbers, the vrow0 of
    // later slacks and the rows of added_entries move down, added_virtual / added_slot are renumbered, m, nr_cuts, nr_virtual and
    // n_provider drop by count.  After it for_each_entry yields the LP without the cuts.  check_remove_cuts decides RELP_E_ARG
    // (count < 0, a missing array, not a cut row, named twice) and RELP_E_STATE (phase 1; a slack that is not basic) alone;
    // remove_cuts runs it first and touches nothing when it fails.
    relp_status_t check_remove_cuts(const int32_t* rows, int32_t count, const std::vector<int32_t>& basis, std::string* err) const;
    relp_status_t remove_cuts(const int32_t* rows, int32_t count, const std::vector<int32_t>& basis, std::string* err);
    // Added columns taken back (relp_remove_columns): `columns` are provider columns added by add_columns, each once, none in
    // `basis`.  The virtual column, its entries and its cost go; the virtual columns behind it (cut slacks included) close up in
    // order.  The same pair of check and removal as above.
    relp_status_t check_remove_columns(const int32_t* columns, int32_t count, const std::vector<int32_t>& basis, std::string* err) const;
    relp_status_t remove_columns(const int32_t* columns, int32_t count, const std::vector<int32_t>& basis, std::string* err);
    // per cut k the virtual column of its slack (the one whose descriptor names row cut_row0 + k)
    std::vector<int32_t> cut_slacks() const;
    // the a of provider column p when it is an added column, else -1; the phase-2 cost of provider column p
    int32_t added_of(int32_t p) const { return (nr_added > 0 && p >= nr_normal && p < n_provider) ? added_slot[p - nr_normal] : -1; }
    double cost_of(int32_t p) const {
        if (p < nr_normal) return cost[p];
        const int32_t a = added_of(p);
        return a >= 0 ? added_cost[a] : 0.0;
    }

    int32_t nr_columns() const { return nr_artificial + n_provider; }

    // the row of an artificial column: j < nr_artificial, or a wrapped index after the phase switch
    int32_t artificial_row(int32_t j) const {
        return column_to_row[j >= kWrappedArtificialBase ? wrapped_na - 1 - (INT32_MAX - j) : j];
    }

    // The entries (row, value) of tableau column j, in order: an artificial column is e_row; a structural column is what
    // `structural(p, put)` supplies for it (constraint rows only), then its bound row, then its cut rows (rows ascend); a virtual
    // column its descriptor rows, an added column (relp_add_columns) its entries, rows ascending.  False if j is no column.
    // It runs for every basis column of every LU refactorisation: forced inline (left to itself the compiler calls it per
    // column, 20 % slower at 64,000 rows); the unsigned compares also reject j < 0.
    template <class S, class P>
    __attribute__((always_inline)) bool for_each_entry(int32_t j, S&& structural, P&& put) const {
        if ((uint32_t)j < (uint32_t)nr_artificial || j >= kWrappedArtificialBase) {
            put(artificial_row(j), 1.0);
            return true;
        }
        const int32_t p = j - nr_artificial;
        if ((uint32_t)p < (uint32_t)nr_normal) {
            structural(p, put);
            if (bound_row[p] >= 0) put(bound_row[p], 1.0);
            if (nr_cuts > 0)
                for (const auto& e : cut_entries[p]) put(cut_row0 + e.first, e.second);
            return true;
        }
        const uint32_t v = (uint32_t)(p - nr_normal);
        if (v >= (uint32_t)nr_virtual) return false;
        if (vrow0[v] >= 0) put(vrow0[v], (double)vsign[v]);     // -1: its row was removed
        if (vrow1[v] >= 0) put(vrow1[v], 1.0);
        if (nr_added > 0 && added_slot[v] >= 0)
            for (const auto& e : added_entries[added_slot[v]]) put(e.first, e.second);
        return true;
    }
    // the same for provider column p (no artificial columns in front)
    template <class S, class P>
    bool for_each_provider_entry(int32_t p, S&& structural, P&& put) const {
        return p >= 0 && for_each_entry(nr_artificial + p, structural, put);
    }

  private:
    // the virtual columns with gone_v set and the added columns with gone_a set leave vrow0 / vrow1 / vsign / added_*; the rest
    // closes up in order
    void drop_virtuals(const std::vector<uint8_t>& gone_v, const std::vector<uint8_t>& gone_a);
    void plan_shards(int32_t count, int32_t rank);
    int64_t candidate_len_for(int32_t rows) const;
};

}  // namespace relp
