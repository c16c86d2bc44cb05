// relp_engine_trial.cpp -- the trial scope of the unsharded tableau engine in phase 2 (relp_trial_begin / relp_trial_end /
// relp_trial_stats) and relp_strong_branch on top of it.  See relp_engine.hpp and DESIGN.md 10.
//
// Between two flushes the tableau is T = (I + W S') T0, and nothing a trial may call writes T0 over the rows and columns that exist
// at the begin or a row of R0 that is pending then: only the flush and the rebuilds do, and a trial refuses them (in_trial).  So the
// way back is a copy of the small arrays below, not of the tableau.
#include "relp_engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace relp {

relp_status_t Engine::in_trial(const char* what) {
    if (!trial_open_) return RELP_OK;
    return fail(RELP_E_STATE, std::string(what) + " inside a trial (it flushes, rebuilds, re-allocates or compacts: relp_trial_end first)");
}

// The snapshot by meaning: "b" is whatever d_b_ is when the plan is made (d_b_ / d_b_alt_ and d_basis_ / d_basis_alt_ swap inside
// the fused loop), so the plan is made from the extents of the begin and the buffers of the moment, once to save and once to
// restore: the same extents in the same order give the same offsets.  Old extents only; what a cut added inside the trial leaves
// behind the old m and n_store (its T0 row and slack column, its rows of A, its entries of W, d_idcol_, vrow / vsign) becomes
// unreachable when the counts come back.
//
//   saved                      why
//   d_d_ [n_store]             every pivot updates the reduced costs; relp_change_cost moves them
//   d_b_ [m]                   every pivot, relp_change_right_hand_side
//   d_basis_ [m]               every pivot
//   d_in_basis_ [n]            every pivot flips two flags (by tableau column)
//   d_cost_ [nr_normal]        relp_change_cost (ColumnTable)
//   d_cost_store_ [n_store]    relp_change_cost (by stored column)
//   d_W_ [p columns]           W <- E W rewrites every pending column at every pivot (whole pitch: the room rows go along)
//   d_wr_, d_S_ [block]        the bookkeeping of the block: row r of W before a pivot, the pivot row of every column of W
//   d_pos_of_row_ [m]          row -> column of W
//   d_shadow_meta_             {row, length} of the fused update's shadow row (settled at the begin: row = -1)
//   d_rec_                     the record: -obj, the iteration and degenerate-pivot counts, n_eta, the rule memory
//   not saved                  why not
//   dT0_                       written by the flush and the rebuilds only (refused); relp_add_cuts writes row m .. of the old columns
//                              and the new slack columns, both behind the old extent
//   dR0_                       a pivot appends row n_eta .. (behind the p pending rows) and the scratch row; relp_add_cuts clears the
//                              new columns' entries only; launch_tab_rhs_change / launch_tab_cost_change read it
//   d_trace_                   a pivot writes entry `iterations` ..: behind the count, which comes back with the record
//   d_minus_pi_,               the tableau path keeps neither up to date in phase 2 (-pi is read off d; there are no artificial
//   d_column_to_row_           columns to map)
//   d_idcol_, d_vrow*, d_vsign_, dA_   written behind the old extents only (relp_add_cuts)
//   d_fstats_, d_fcols_ ..     the flush's own
//   the PRICE partials         marked invalid at the end, as the in-place calls do
//   d_alpha_, d_rmin_, d_w_, the in-place lists and the query scratch     scratch: written before they are read
TrialPlan Engine::trial_layout(const TrialExtents& x, bool* ok) {
    TrialPlan plan;
    bool fine = true;
    auto add = [&](auto& buf, int64_t count) {
        using T = std::remove_pointer_t<decltype(buf + 0)>;
        fine = fine && buf.count() >= count && plan.add(static_cast<void*>(buf + 0), count * (int64_t)sizeof(T));
    };
    add(d_d_, x.n_store);
    add(d_b_, x.m);
    add(d_basis_, x.m);
    add(d_in_basis_, x.n);
    add(d_cost_, x.nr_normal);
    add(d_cost_store_, x.n_store);
    add(d_W_, (int64_t)x.p * ld_b_);
    add(d_wr_, d_wr_.count());
    add(d_S_, d_S_.count());
    add(d_pos_of_row_, x.m);
    add(d_shadow_meta_, d_shadow_meta_.count());
    add(d_rec_, 1);
    *ok = fine;
    return plan;
}

relp_status_t Engine::trial_copy(bool save) {
    bool ok = false;
    const TrialPlan plan = trial_layout(trial_host_.extents, &ok);
    if (!ok) return fail(RELP_E_STATE, "the trial snapshot does not fit the engine's buffers");
    if (save) {
        HIP_TRY(d_trial_.ensure_raw((size_t)std::max<int64_t>(plan.buffer_bytes(), kTrialUnit)));
        trial_last_bytes_ = plan.payload_bytes();
    }
    const TrialTable t = plan.table(d_trial_ + 0, save);
    if (sw_.trial_memcpy) {
        // the control (RELP_TRIAL_MEMCPY=1): the same copies as a chain of transfers
        hipError_t e = hipSuccess;
        for (int32_t s = 0; s < t.count; ++s)
            if (t.seg[s].bytes > 0) e = first_error(e, hipMemcpyAsync(t.seg[s].dst, t.seg[s].src, (size_t)t.seg[s].bytes, hipMemcpyDeviceToDevice, stream_));
        HIP_TRY(e);
    } else {
        launch_tab_trial_copy(t, stream_);
    }
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "the trial snapshot: a kernel launch failed");
    return RELP_OK;
}

// The host side: the layout (it holds the rhs, the costs and the cuts), the stored-column mirrors, the flush and re-inversion
// counters (suspended inside a trial, saved all the same) and every counter a *_stats call reports.
void Engine::trial_host_save() {
    TrialHost& h = trial_host_;
    h.lay = lay_;
    h.n_store = n_store_; h.n_alloc = n_alloc_;
    h.idcol_h = idcol_h_; h.cost_store_h = cost_store_h_;
    h.since_flush = since_flush_; h.since_reinvert = since_reinvert_; h.reinvert_interval = reinvert_interval_; h.reinversions = reinversions_;
    h.flushes_since_reprice = flushes_since_reprice_; h.last_reinvert_drift = last_reinvert_drift_; h.retab_done = retab_done_;
    h.rhs_changes = rhs_changes_; h.rhs_columns = rhs_columns_; h.rhs_last_p = rhs_last_p_; h.rhs_last_splits = rhs_last_splits_;
    h.cost_changes = cost_changes_; h.cost_rows = cost_rows_; h.cost_last_p = cost_last_p_; h.cost_last_splits = cost_last_splits_;
    h.cut_last_rows = cut_last_rows_; h.cut_last_p = cut_last_p_; h.col_last_cols = col_last_cols_; h.col_last_p = col_last_p_;
    h.rm_cuts = rm_cuts_; h.rm_columns = rm_columns_; h.rm_last_moved = rm_last_moved_; h.rm_last_p = rm_last_p_;
    h.rng_ratio_calls = rng_ratio_calls_; h.rng_ratio_rows = rng_ratio_rows_; h.rng_ranging_calls = rng_ranging_calls_; h.rng_last_p = rng_last_p_;
    h.gom_calls = gom_calls_; h.gom_entries = gom_entries_; h.gom_cuts = gom_cuts_; h.gom_last_p = gom_last_p_;
}

void Engine::trial_host_restore() {
    TrialHost& h = trial_host_;
    std::swap(lay_, h.lay);                            // (the next begin assigns over what is left here)
    n_store_ = h.n_store; n_alloc_ = h.n_alloc;
    idcol_h_.swap(h.idcol_h); cost_store_h_.swap(h.cost_store_h);
    since_flush_ = h.since_flush; since_reinvert_ = h.since_reinvert; reinvert_interval_ = h.reinvert_interval; reinversions_ = h.reinversions;
    flushes_since_reprice_ = h.flushes_since_reprice; last_reinvert_drift_ = h.last_reinvert_drift; retab_done_ = h.retab_done;
    rhs_changes_ = h.rhs_changes; rhs_columns_ = h.rhs_columns; rhs_last_p_ = h.rhs_last_p; rhs_last_splits_ = h.rhs_last_splits;
    cost_changes_ = h.cost_changes; cost_rows_ = h.cost_rows; cost_last_p_ = h.cost_last_p; cost_last_splits_ = h.cost_last_splits;
    cut_last_rows_ = h.cut_last_rows; cut_last_p_ = h.cut_last_p; col_last_cols_ = h.col_last_cols; col_last_p_ = h.col_last_p;
    rm_cuts_ = h.rm_cuts; rm_columns_ = h.rm_columns; rm_last_moved_ = h.rm_last_moved; rm_last_p_ = h.rm_last_p;
    rng_ratio_calls_ = h.rng_ratio_calls; rng_ratio_rows_ = h.rng_ratio_rows; rng_ranging_calls_ = h.rng_ranging_calls; rng_last_p_ = h.rng_last_p;
    gom_calls_ = h.gom_calls; gom_entries_ = h.gom_entries; gom_cuts_ = h.gom_cuts; gom_last_p_ = h.gom_last_p;
}

relp_status_t Engine::trial_begin() {
    relp_status_t st = dual_ready("relp_trial_begin");
    if (st) return st;
    if (trial_open_) return fail(RELP_E_STATE, "relp_trial_begin: a trial is open (trials do not nest)");
    int32_t p;
    if ((st = settled_pending(&p))) return st;          // the shadow row settled, no flush
    trial_host_.extents = TrialExtents{lay_.m, n_store_, nr_columns(), lay_.nr_normal, p};
    if ((st = trial_copy(true))) return st;
    trial_host_save();
    trial_open_ = true;
    ++trials_begun_;
    return RELP_OK;
}

relp_status_t Engine::trial_end(int32_t keep) {
    relp_status_t st = dual_ready("relp_trial_end");
    if (st) return st;
    if (!trial_open_) return fail(RELP_E_STATE, "relp_trial_end: no trial is open");
    if (keep != 0 && keep != 1) return fail(RELP_E_ARG, "relp_trial_end: keep is neither 0 nor 1");
    tab_settle();
    trial_last_room_ = std::max<int64_t>(0, (int64_t)block_ - 1 - since_flush_);
    if (keep) {                                         // the state stays; a due flush or re-inversion happens at the next loop
        trial_open_ = false;
        return RELP_OK;
    }
    if ((st = trial_copy(false))) return st;
    trial_host_restore();
    pools_mark_stale(nullptr, 0);                      // a pool created inside the trial over a cut row the rollback took back
    tab_partials_valid_ = false;
    trial_open_ = false;
    ++trials_rolled_back_;
    return edit_rec();                                  // re-armed, as the in-place calls leave it; the download waits for the copy
}

relp_status_t Engine::trial_stats(int64_t* out4) const {
    return in_place_stats(out4, trials_begun_, trials_rolled_back_, trial_last_bytes_, trial_last_room_);
}

// Strong branching on the rows of fractional structural columns: per evaluated entry two trials -- x_j <= floor(b_r), then
// -x_j <= -ceil(b_r), each as one cut (relp_add_cuts), at most max_pivots dual pivots (relp_run_dual), the objective, the way
// back (relp_trial_end(0)).  Host code over those calls: no kernel of its own.
relp_status_t Engine::strong_branch(const int32_t* rows, int32_t count, int32_t max_pivots, double away, double* objective, int32_t* outcome,
                                    int32_t* pivots, int32_t* status) {
    relp_status_t st = dual_ready("relp_strong_branch");
    if (st) return st;
    if (count < 0 || (count > 0 && (!rows || !objective || !outcome || !pivots || !status)))
        return fail(RELP_E_ARG, "relp_strong_branch: count < 0 or rows, objective, outcome, pivots or status missing");
    for (int32_t k = 0; k < count; ++k)
        if (rows[k] < 0 || rows[k] >= lay_.m) return fail(RELP_E_ARG, "relp_strong_branch: row out of range");
    if (max_pivots < 1 || max_pivots > block_ - 1) return fail(RELP_E_ARG, "relp_strong_branch: max_pivots outside [1, update_block - 1]");
    if (!std::isfinite(away) || away < 0.0 || !(away < 0.5)) return fail(RELP_E_ARG, "relp_strong_branch: away outside [0, 0.5)");
    if (trial_open_) return fail(RELP_E_STATE, "relp_strong_branch: a trial is open (trials do not nest)");
    if (count == 0) return RELP_OK;
    if ((st = check_dual_feasible("relp_strong_branch"))) return st;
    tab_partials_valid_ = false;                       // (the partial slots hold the scan of the check)

    const int32_t m = lay_.m;
    std::vector<double> b(m);
    std::vector<int32_t> basis(m);
    hipError_t e = d_b_.download(b, enqueue_only(stream_));
    HIP_TRY(first_error(e, d_basis_.download(basis, stream_)));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> obj(2 * (size_t)count, nan);
    std::vector<int32_t> oc(2 * (size_t)count, -1), piv(2 * (size_t)count, 0), stat(count, 0);
    int32_t evaluated = 0;
    for (int32_t k = 0; k < count; ++k) {
        const int32_t j = basis[rows[k]];
        const double f0 = b[rows[k]] - std::floor(b[rows[k]]);
        if (j < 0 || j >= lay_.nr_normal) stat[k] = 1;
        else if (f0 < away || f0 > 1.0 - away) stat[k] = 2;
        else ++evaluated;
    }
    if (evaluated > 0) {
        // room for the one cut of a trial (grown as relp_add_cuts itself would grow), and for max_pivots pivots in the open block
        if (lay_.nr_cuts + 1 > cut_room_) {
            const int64_t want = std::max<int64_t>({(int64_t)lay_.nr_cuts + 1, 2 * (int64_t)cut_room_, 16});
            if (want > INT32_MAX / 2) return fail(RELP_E_ARG, "relp_strong_branch: too many cuts");
            if ((st = grow_for_cuts((int32_t)want))) return st;
        }
        if (since_flush_ + max_pivots + 1 > block_ && (st = flush())) return st;
    }
    for (int32_t k = 0; k < count; ++k) {
        if (stat[k] != 0) continue;
        const int32_t j = basis[rows[k]];
        for (int32_t side = 0; side < 2; ++side) {
            const int64_t row_ptr[2] = {0, 1};
            const double value = side == 0 ? 1.0 : -1.0;
            const double rhs = side == 0 ? std::floor(b[rows[k]]) : -std::ceil(b[rows[k]]);
            if ((st = trial_begin())) return st;
            int64_t done = 0;
            int32_t o = RELP_RUNNING;
            double z = nan;
            st = add_cuts(1, row_ptr, &j, &value, &rhs);
            if (!st) st = run_dual(max_pivots, &done, &o);
            if (!st) st = get_objective(&z);
            const relp_status_t back = trial_end(0);
            if (st || back) return st ? st : back;
            const size_t slot = 2 * (size_t)k + side;
            obj[slot] = o == RELP_INFEASIBLE ? std::numeric_limits<double>::infinity() : z;
            oc[slot] = o;
            piv[slot] = (int32_t)done;
        }
    }
    std::copy(obj.begin(), obj.end(), objective);
    std::copy(oc.begin(), oc.end(), outcome);
    std::copy(piv.begin(), piv.end(), pivots);
    std::copy(stat.begin(), stat.end(), status);
    return RELP_OK;
}

}  // namespace relp
