// relp_engine_pool.cpp -- the pools of the unsharded tableau engine in phase 2, kept on the device in sliced ELL, swept there, the
// winners picked there, the chosen items added in place.  See relp_pool.hpp (the layout, the segments, the stale rule),
// relp_cutpool.hpp (the norms), relp_kernels.h (the launches) and DESIGN.md 10.
//
// The column pool (relp_pool_create .. relp_pool_stats): the candidate columns of a column-generation master, priced against -pi as
// the tableau holds it, added as relp_add_columns adds them.  Pricing reads d_d_, d_cost_store_ and d_idcol_ --
// (-pi)_i = d[idcol[i]] - cost_store[idcol[i]], what relp_get_minus_pi forms on the host -- and the pool.
// The cut pool (relp_cutpool_create .. relp_cutpool_stats): the candidate rows of a row-generation scheme, separated against the
// vertex as the tableau holds it, added as relp_add_cuts adds them.  Separation reads d_b_ and d_basis_ -- x_j = b[r] where
// structural column j is basic in row r -- and the pool.
// Either sweep writes scratch alone.  The tableau engine keeps d, b and the basis up to date at every pivot and every in-place call,
// so nothing is flushed, settled beyond the shadow row or re-armed, and the record is not even downloaded.
#include "relp_engine_internal.hpp"

#include <algorithm>
#include <cmath>

namespace relp {

namespace {
// the one buffer a sweep downloads: [values of the winners (segments doubles: d, or the slack) | their pool indices (segments) | their number]
struct SweepOut {
    double* value; int32_t* k; int32_t* found;
    static size_t bytes(int32_t segments) { return sizeof(double) * (size_t)segments + sizeof(int32_t) * ((size_t)segments + 1); }
    SweepOut(char* base, int32_t segments)
        : value(reinterpret_cast<double*>(base)), k(reinterpret_cast<int32_t*>(base + sizeof(double) * (size_t)segments)), found(k + segments) {}
};
constexpr int32_t kPoolOneDownload = 4096;             // segments up to which the whole buffer comes down in one copy

template <class List>
auto find_pool(List& list, const DevicePool* pool) {
    return std::find_if(list.begin(), list.end(), [&](const auto& p) { return static_cast<const DevicePool*>(p.get()) == pool; });
}
}  // namespace

// ---- what both kinds of pool do alike ------------------------------------------------------------------------------------------
// The shared front: the engine and phase, the pool is one of this handle's.
template <class List>
relp_status_t Engine::pool_mine(const char* what, const PoolWords& w, const List& list, const DevicePool* pool) {
    const relp_status_t st = dual_ready(what);
    if (st) return st;
    if (!pool || find_pool(list, pool) == list.end()) return fail(RELP_E_ARG, std::string(what) + ": not " + w.pool + " of this handle");
    return RELP_OK;
}

template <class List>
relp_status_t Engine::pool_drop(const char* what, const PoolWords& w, List& list, const DevicePool* pool) {
    const auto it = find_pool(list, pool);
    if (it == list.end()) return fail(RELP_E_ARG, std::string(what) + ": not " + w.pool + " of this handle");
    (void)hipStreamSynchronize(stream_);
    list.erase(it);
    return RELP_OK;
}

template <class List>
relp_status_t Engine::pool_stats_in(const List& list, const DevicePool* pool, int64_t* out4) const {
    if (!pool || find_pool(list, pool) == list.end()) return RELP_E_ARG;
    return in_place_stats(out4, pool->image.count, pool->image.nonzeros(), pool->image.stored(), pool->sweep_calls);
}

// The checks of a create are those of relp_add_columns / relp_add_cuts, in its words but for the name of the call.
void Engine::rename_prefix(const char* from, const char* to) {
    const std::string f = from;
    if (err_.compare(0, f.size(), f) == 0) err_.replace(0, f.size(), to);
}

// The device copy of dp.image (and of the norms, where the pool has them) under one wait, every activity flag set.
relp_status_t Engine::pool_upload(DevicePool& dp, const std::vector<double>* norm, DeviceBuf<double>* d_norm) {
    const PoolImage& im = dp.image;
    HIP_TRY(dp.d_slice_ptr.alloc((int64_t)im.slice_ptr.size()));
    HIP_TRY(dp.d_idx.alloc(im.stored()));
    HIP_TRY(dp.d_val.alloc(im.stored()));
    HIP_TRY(dp.d_scalar.alloc(im.count));
    if (d_norm) HIP_TRY(d_norm->alloc(im.count));
    HIP_TRY(dp.d_active.alloc(im.count));
    // under one wait (no return before it: the image is in flight)
    hipError_t e = dp.d_slice_ptr.upload(im.slice_ptr, enqueue_only(stream_));
    e = first_error(e, dp.d_idx.upload(im.ell_idx, enqueue_only(stream_)));
    e = first_error(e, dp.d_val.upload(im.ell_val, enqueue_only(stream_)));
    e = first_error(e, dp.d_scalar.upload(im.scalar, enqueue_only(stream_)));
    if (d_norm) e = first_error(e, d_norm->upload(*norm, enqueue_only(stream_)));
    HIP_TRY(first_error(e, dp.d_active.fill_bytes(1, im.count, stream_)));
    return RELP_OK;
}

PoolView Engine::pool_view(const DevicePool& dp) const {
    return PoolView{dp.d_slice_ptr, dp.d_idx, dp.d_val, dp.d_scalar, dp.d_active, dp.image.count};
}

// active[ids[x]] = flag on the device, the ids under one wait with the launch (the caller has room in d_pool_ids_).
relp_status_t Engine::pool_flags(const DevicePool& dp, const int32_t* ids, int32_t count, int32_t flag) {
    const hipError_t e = d_pool_ids_.upload(ids, count, enqueue_only(stream_));
    if (e == hipSuccess) launch_pool_set_active(pool_view(dp), d_pool_ids_, count, flag, stream_);
    HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
    return RELP_OK;
}

relp_status_t Engine::pool_flags_checked(const char* what, const PoolWords& w, const DevicePool& dp, const int32_t* ids, int32_t count,
                                         int32_t flag) {
    if (flag != 0 && flag != 1) return fail(RELP_E_ARG, std::string(what) + ": flag is neither 0 nor 1");
    const std::string why = pool_check_ids(w, ids, count, dp.image.count);
    if (!why.empty()) return fail(RELP_E_ARG, std::string(what) + ": " + why);
    if (count == 0) return RELP_OK;
    HIP_TRY(d_pool_ids_.ensure(count, 256));
    const relp_status_t st = pool_flags(dp, ids, count, flag);
    if (st) return st;
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, std::string(what) + ": a kernel launch failed");
    return RELP_OK;
}

// The scratch of a sweep over `segments` shares (0: the values alone); `all`: the vector of every item's value is wanted.
relp_status_t Engine::pool_sweep_scratch(DevicePool& dp, int32_t segments, bool all) {
    const int32_t count = dp.image.count;
    if (all) HIP_TRY(dp.d_all.ensure_raw(sizeof(double) * (size_t)std::max(count, 1)));
    if (segments > 0) {
        const size_t parts = (size_t)segments * (size_t)pool_segment_chunks(count, segments);
        HIP_TRY(dp.d_part_d.ensure_raw(sizeof(double) * parts));
        HIP_TRY(dp.d_part_k.ensure_raw(sizeof(int32_t) * parts));
        HIP_TRY(dp.d_out.ensure_raw(SweepOut::bytes(segments)));
    }
    return RELP_OK;
}

// The winners of the sweep just launched.  One download: the whole buffer while it is small, else the number of winners first and
// then the winners alone.
relp_status_t Engine::pool_winners(const char* what, DevicePool& dp, int32_t segments, int32_t* ids_out, double* out, int32_t* found) {
    const SweepOut so(dp.d_out, segments);
    int32_t n = 0;
    if (segments <= kPoolOneDownload) {
        std::vector<char> host(SweepOut::bytes(segments));
        HIP_TRY(download_from(host.data(), (const char*)dp.d_out, host.size(), stream_));
        const SweepOut ho(host.data(), segments);
        n = std::min(std::max(*ho.found, 0), segments);
        std::copy(ho.k, ho.k + n, ids_out);
        std::copy(ho.value, ho.value + n, out);
    } else {
        HIP_TRY(download_from(&n, so.found, 1, stream_));
        n = std::min(std::max(n, 0), segments);
        const hipError_t e = download_from(ids_out, so.k, (size_t)n, enqueue_only(stream_));
        HIP_TRY(first_error(e, n ? download_from(out, so.value, (size_t)n, stream_) : hipStreamSynchronize(stream_)));
    }
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, std::string(what) + ": a kernel launch failed");
    *found = n;
    ++dp.sweep_calls;                                  // (a call that failed is not counted)
    return RELP_OK;
}

// ---- the column pool -----------------------------------------------------------------------------------------------------------
// The front of its calls: pool_mine and, where `fresh` is asked, not stale.
relp_status_t Engine::pool_ready(const char* what, const relp_pool* pool, bool fresh) {
    const relp_status_t st = pool_mine(what, kColumnPoolWords, pools_, pool);
    if (st) return st;
    // (bound > m cannot outlive pools_mark_stale; tested all the same: a pool row beyond the engine's rows is never read)
    if (fresh && (pool->stale || pool_stale_after_rollback(pool->image.bound, lay_.m)))
        return fail(RELP_E_STATE, std::string(what) + ": the pool is stale (relp_remove_cuts or the rollback of a trial took out an engine row below the " +
                                      std::to_string(pool->image.bound) + " rows the pool was created over)");
    return RELP_OK;
}

// The stale rule where engine rows go (relp_pool.hpp).  rows == nullptr: the rows from lay_.m on went (the rollback of a trial takes
// back the cut rows added inside it); else the listed engine rows did (relp_remove_cuts).  Stale is for good: a cut added later in
// the place of a row that went is another row.
void Engine::pools_mark_stale(const int32_t* rows, int32_t count) {
    for (auto& pool : pools_)
        if (rows ? pool_stale_after_removal(pool->image.bound, rows, count) : pool_stale_after_rollback(pool->image.bound, lay_.m))
            pool->stale = true;
}

relp_status_t Engine::pool_create(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost,
                                  relp_pool** out) {
    relp_status_t st = dual_ready("relp_pool_create");
    if (st) return st;
    if (!out) return fail(RELP_E_ARG, "relp_pool_create: the pool pointer is missing");
    *out = nullptr;
    if ((st = lay_.check_columns(count, col_ptr, row_idx, values, cost, &err_))) {      // the checks of relp_add_columns, in its words
        rename_prefix("relp_add_columns", "relp_pool_create");
        return st;
    }
    auto pool = std::make_unique<relp_pool>();
    pool->image = pool_pack(count, col_ptr, row_idx, values, cost, lay_.m);
    if ((st = pool_upload(*pool, nullptr, nullptr))) return st;
    *out = pool.get();
    pools_.push_back(std::move(pool));
    return RELP_OK;
}

relp_status_t Engine::pool_destroy(relp_pool* pool) { return pool_drop("relp_pool_destroy", kColumnPoolWords, pools_, pool); }

relp_status_t Engine::pool_stats(const relp_pool* pool, int64_t* out4) const { return pool_stats_in(pools_, pool, out4); }

relp_status_t Engine::pool_set_active(relp_pool* pool, const int32_t* ids, int32_t count, int32_t flag) {
    const relp_status_t st = pool_ready("relp_pool_set_active", pool, false);
    return st ? st : pool_flags_checked("relp_pool_set_active", kColumnPoolWords, *pool, ids, count, flag);
}

// The launches of a price (segments >= 1) or of the reduced costs alone (segments == 0, d_all written); the caller downloads.
relp_status_t Engine::pool_launch_price(relp_pool& pool, int32_t segments, double tol, bool all) {
    const relp_status_t st = pool_sweep_scratch(pool, segments, all);
    if (st) return st;
    const SweepOut so = segments > 0 ? SweepOut(pool.d_out, segments) : SweepOut(nullptr, 0);
    HIP_TRY(d_pool_minus_pi_.ensure(lay_.m, 256));
    tab_settle();
    launch_pool_price(pool_view(pool), minus_pi_view(), segments, tol, all ? (double*)pool.d_all : nullptr, pool.d_part_d, pool.d_part_k, so.k,
                      so.value, so.found, stream_);
    return RELP_OK;
}

relp_status_t Engine::pool_reduced_costs(relp_pool* pool, double* out_count) {
    relp_status_t st = pool_ready("relp_pool_reduced_costs", pool, true);
    if (st) return st;
    if (pool->image.count == 0) return RELP_OK;
    if (!out_count) return fail(RELP_E_ARG, "relp_pool_reduced_costs: the output array is missing");
    if ((st = pool_launch_price(*pool, 0, 0.0, true))) return st;
    HIP_TRY(download_from(out_count, (const double*)pool->d_all, (size_t)pool->image.count, stream_));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_pool_reduced_costs: a kernel launch failed");
    return RELP_OK;
}

relp_status_t Engine::pool_price(relp_pool* pool, int32_t segments, double tol, int32_t* ids_out, double* d_out, int32_t* found) {
    relp_status_t st = pool_ready("relp_pool_price", pool, true);
    if (st) return st;
    const std::string why = pool_check_sweep_args(kColumnPoolWords, pool->image.count, segments, tol, ids_out, d_out, found);
    if (!why.empty()) return fail(RELP_E_ARG, "relp_pool_price: " + why);
    *found = 0;
    if (pool->image.count == 0) { ++pool->sweep_calls; return RELP_OK; }
    if ((st = pool_launch_price(*pool, segments, tol, false))) return st;
    return pool_winners("relp_pool_price", *pool, segments, ids_out, d_out, found);
}

// relp_add_columns of the pool columns ids[0 .. count), in that order.  The host decides what it must know before a launch -- the
// checks, the room, the length of the union list and the longest chosen column, all from its copy of the pool -- and runs
// Layout::add_columns afterwards; the operands of launch_tab_add_columns (the union list, coef, d_new, cost_new, the new rows of
// d_col_a_) are formed on the device from the device copy (launch_pool_add_operands), in the order and with the arithmetic of
// Engine::add_columns, so both leave the same bits.  RELP_POOL_HOST_ADD=1: Engine::add_columns itself on the host copy, the control.
relp_status_t Engine::pool_add(relp_pool* pool, const int32_t* ids, int32_t count) {
    relp_status_t st = pool_ready("relp_pool_add", pool, true);
    if (st) return st;
    if ((st = in_trial("relp_pool_add"))) return st;
    if (count > kTabColTile * 65535) return fail(RELP_E_ARG, "relp_pool_add: more than 524,280 columns in one call");
    const std::string why = pool_check_ids(kColumnPoolWords, ids, count, pool->image.count);
    if (!why.empty()) return fail(RELP_E_ARG, "relp_pool_add: " + why);
    if (count == 0) return RELP_OK;
    const PoolChoice ch = pool_choose(pool->image, ids, count);
    HIP_TRY(d_pool_ids_.ensure(count, 256));
    if (sw_.pool_host_add) {
        if ((st = add_columns(count, ch.ptr.data(), ch.idx.data(), ch.values.data(), ch.scalar.data()))) return st;
        return pool_flags(*pool, ids, count, 0);
    }
    if ((st = room_for_columns("relp_pool_add", count))) return st;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    const int32_t entries = ch.touched, added_old = lay_.nr_added;      // the union list: the rows the chosen columns touch
    HIP_TRY(d_col_cols_.ensure(std::max(entries, 1), lay_.m));
    HIP_TRY(d_col_coef_.ensure(std::max<int64_t>((int64_t)entries * count, 1)));
    HIP_TRY(d_col_d_.ensure(count, 16));
    HIP_TRY(d_col_cost_.ensure(count, 16));
    HIP_TRY(d_pool_rank_.ensure(lay_.m, 256));
    HIP_TRY(d_pool_entries_.ensure(1));
    HIP_TRY(d_pool_minus_pi_.ensure(lay_.m, 256));

    const TableauView tv = tview();                    // the tableau before the add
    const ColumnAdd ca{d_col_cols_, d_col_coef_, entries, count, d_col_d_, d_col_cost_};
    const ColumnTail ct{d_cost_store_, d_in_basis_, d_vrow0_, d_vrow1_, d_vsign_, lay_.nr_virtual, block_ + 1};
    const PoolAdd pa{d_pool_ids_, count, lay_.m, ch.longest, entries, d_pool_rank_, d_col_cols_, d_pool_entries_, d_col_coef_,
                     d_col_a_, ld_c_, added_old, d_col_d_, d_col_cost_};
    // the ids under one wait with the launches (no return before it: ids is in flight; no launch on a lost list)
    hipError_t e = d_pool_ids_.upload(ids, count, enqueue_only(stream_));
    if (e == hipSuccess) {
        launch_pool_add_operands(pool_view(*pool), minus_pi_view(), pa, stream_);
        launch_tab_add_columns(tv, deferred(), ca, p, ct, stream_);
    }
    int32_t entries_dev = -1;
    HIP_TRY(first_error(e, d_pool_entries_.download(&entries_dev, 1, stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_pool_add: a kernel launch failed");
    // Unreachable while the device copy of the pool is the image of the host copy: both count the rows the same columns touch.  It
    // is looked at behind the launches -- a look in front of launch_tab_add_columns would cost every add a second wait -- so if it
    // ever fires the device tableau holds columns the layout does not: the handle is unusable from here on, like after a failed
    // launch of a pivot (include/relp_engine.h says so).
    if (entries_dev != entries)
        return fail(RELP_E_HIP, "relp_pool_add: the device's union list and the host's differ in length (the device copy of the pool is "
                                "damaged; the tableau has been written: destroy the handle)");
    return columns_added(count, ch.ptr.data(), ch.idx.data(), ch.values.data(), ch.scalar.data(), entries, p);
}

// ---- the cut pool --------------------------------------------------------------------------------------------------------------
// (The front of its calls is pool_mine alone: no stale rule, the structural columns never move.)
relp_status_t Engine::cutpool_create(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs,
                                     relp_cutpool** out) {
    relp_status_t st = dual_ready("relp_cutpool_create");
    if (st) return st;
    if (!out) return fail(RELP_E_ARG, "relp_cutpool_create: the pool pointer is missing");
    *out = nullptr;
    if ((st = lay_.check_cuts(count, row_ptr, col_idx, values, rhs, &err_))) {           // the checks of relp_add_cuts, in its words
        rename_prefix("relp_add_cuts", "relp_cutpool_create");
        return st;
    }
    auto pool = std::make_unique<relp_cutpool>();
    CutPoolImage im = cutpool_pack(count, row_ptr, col_idx, values, rhs, lay_.nr_normal);
    pool->image = std::move(im.ell);
    pool->norm = std::move(im.norm);
    if ((st = pool_upload(*pool, &pool->norm, &pool->d_norm))) return st;
    *out = pool.get();
    cutpools_.push_back(std::move(pool));
    return RELP_OK;
}

relp_status_t Engine::cutpool_destroy(relp_cutpool* pool) { return pool_drop("relp_cutpool_destroy", kCutPoolWords, cutpools_, pool); }

relp_status_t Engine::cutpool_stats(const relp_cutpool* pool, int64_t* out4) const { return pool_stats_in(cutpools_, pool, out4); }

relp_status_t Engine::cutpool_set_active(relp_cutpool* pool, const int32_t* ids, int32_t count, int32_t flag) {
    const relp_status_t st = pool_mine("relp_cutpool_set_active", kCutPoolWords, cutpools_, pool);
    return st ? st : pool_flags_checked("relp_cutpool_set_active", kCutPoolWords, *pool, ids, count, flag);
}

// The launches of a separation (segments >= 1) or of the slacks alone (segments == 0); the caller downloads.
relp_status_t Engine::cutpool_launch_separate(relp_cutpool& pool, int32_t segments, double tol, int32_t by_efficacy) {
    const relp_status_t st = pool_sweep_scratch(pool, segments, true);
    if (st) return st;
    const SweepOut so = segments > 0 ? SweepOut(pool.d_out, segments) : SweepOut(nullptr, 0);
    HIP_TRY(d_cutpool_x_.ensure(std::max(lay_.nr_normal, 1), 256));
    tab_settle();
    launch_cutpool_separate(cutpool_view(pool), vertex_view(), segments, tol, by_efficacy, pool.d_all, pool.d_part_d, pool.d_part_k, so.k,
                            so.value, so.found, stream_);
    return RELP_OK;
}

relp_status_t Engine::cutpool_slacks(relp_cutpool* pool, double* out_count) {
    relp_status_t st = pool_mine("relp_cutpool_slacks", kCutPoolWords, cutpools_, pool);
    if (st) return st;
    if (pool->image.count == 0) return RELP_OK;
    if (!out_count) return fail(RELP_E_ARG, "relp_cutpool_slacks: the output array is missing");
    if ((st = cutpool_launch_separate(*pool, 0, 0.0, 0))) return st;
    HIP_TRY(download_from(out_count, (const double*)pool->d_all, (size_t)pool->image.count, stream_));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_cutpool_slacks: a kernel launch failed");
    return RELP_OK;
}

relp_status_t Engine::cutpool_separate(relp_cutpool* pool, int32_t segments, double tol, int32_t by_efficacy, int32_t* ids_out,
                                       double* slack_out, int32_t* found) {
    relp_status_t st = pool_mine("relp_cutpool_separate", kCutPoolWords, cutpools_, pool);
    if (st) return st;
    const std::string why = cutpool_check_separate_args(pool->image.count, segments, tol, by_efficacy, ids_out, slack_out, found);
    if (!why.empty()) return fail(RELP_E_ARG, "relp_cutpool_separate: " + why);
    *found = 0;
    if (pool->image.count == 0) { ++pool->sweep_calls; return RELP_OK; }
    if ((st = cutpool_launch_separate(*pool, segments, tol, by_efficacy))) return st;
    return pool_winners("relp_cutpool_separate", *pool, segments, ids_out, slack_out, found);
}

// relp_add_cuts of the pool cuts ids[0 .. count), in that order.  The host decides what it can know before a launch -- the checks,
// the room, the structural columns the chosen cuts touch and the longest chosen cut, all from its copy of the pool -- and runs
// Layout::add_cuts afterwards; the operands of launch_tab_add_cuts (the union list, coef, the cut rows of A, b of the new rows) are
// formed on the device from the device copy, b and the basis of the moment (launch_cutpool_add_operands), in the order and with the
// arithmetic of Engine::add_cuts, so both leave the same bits.  The one thing that comes down in between is the length of the union
// list, four bytes: which of the touched columns are basic only the device knows, and launch_tab_add_cuts takes the length by
// value.  The host checks it against its bound there, in front of the first write to the tableau.
// RELP_CUTPOOL_HOST_ADD=1: Engine::add_cuts itself on the host copy, the control.
relp_status_t Engine::cutpool_add(relp_cutpool* pool, const int32_t* ids, int32_t count) {
    relp_status_t st = pool_mine("relp_cutpool_add", kCutPoolWords, cutpools_, pool);
    if (st) return st;
    const std::string why = pool_check_ids(kCutPoolWords, ids, count, pool->image.count);
    if (!why.empty()) return fail(RELP_E_ARG, "relp_cutpool_add: " + why);
    if (count == 0) return RELP_OK;
    const PoolChoice ch = pool_choose(pool->image, ids, count);
    HIP_TRY(d_pool_ids_.ensure(count, 256));
    if (sw_.cutpool_host_add) {
        if ((st = add_cuts(count, ch.ptr.data(), ch.idx.data(), ch.values.data(), ch.scalar.data()))) {
            rename_prefix("relp_add_cuts", "relp_cutpool_add");
            return st;
        }
        return pool_flags(*pool, ids, count, 0);
    }
    if ((st = room_for_cuts("relp_cutpool_add", count))) return st;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    const int32_t m_old = lay_.m, cuts_old = lay_.nr_cuts;
    const int32_t room = std::min(ch.touched, m_old);      // the union list: the basic ones among the touched columns, one row each
    HIP_TRY(d_cut_rows_.ensure(std::max(room, 1), std::min<int64_t>(lay_.m, lay_.nr_normal)));
    HIP_TRY(d_cut_coef_.ensure(std::max<int64_t>((int64_t)room * count, 1)));
    HIP_TRY(d_cut_u_.ensure((int64_t)count * std::max(block_, 1)));
    HIP_TRY(d_cutpool_mark_.ensure(std::max(lay_.nr_normal, 1), 256));
    HIP_TRY(d_pool_entries_.ensure(1));

    const TableauView tv = tview();                    // the tableau before the add
    const CutPoolAdd ca{d_pool_ids_, count, m_old, lay_.nr_normal, ch.longest, room, d_basis_, d_b_, d_cutpool_mark_, d_cut_rows_,
                        d_pool_entries_, d_cut_coef_, A_base(), ld_a_, lay_.mc + cuts_old, d_b_ + m_old};
    // the ids under one wait with the operand launches (no return before it: ids is in flight; no launch on a lost list)
    hipError_t e = d_pool_ids_.upload(ids, count, enqueue_only(stream_));
    if (e == hipSuccess) launch_cutpool_add_operands(cutpool_view(*pool), ca, stream_);
    int32_t entries = -1;
    HIP_TRY(first_error(e, d_pool_entries_.download(&entries, 1, stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_cutpool_add: a kernel launch failed");
    // Unreachable while the device copy of the pool is the image of the host copy: the list holds one row per basic touched column.
    // Nothing of the old rows and columns has been written; the room rows of A and b behind them and the chosen flags have.
    if (entries < 0 || entries > room)
        return fail(RELP_E_HIP, "relp_cutpool_add: the device's union list is longer than the columns the chosen cuts touch (the device copy "
                                "of the pool is damaged: destroy the handle)");
    const CutRows cr{d_cut_rows_, d_cut_coef_, entries, count, A_base(), ld_a_, lay_.mc + cuts_old, tab_na_, lay_.nr_normal};
    const CutTail ct{d_cost_store_, d_in_basis_, d_idcol_, d_basis_, d_vrow0_, d_vrow1_, d_vsign_, lay_.nr_virtual, block_ + 1};
    launch_tab_add_cuts(tv, deferred(), cr, d_in_basis_, p, d_cut_u_, ct, stream_);
    HIP_TRY(hipStreamSynchronize(stream_));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_cutpool_add: a kernel launch failed");
    return cuts_added(count, ch.ptr.data(), ch.idx.data(), ch.values.data(), ch.scalar.data(), entries, p);
}

}  // namespace relp
