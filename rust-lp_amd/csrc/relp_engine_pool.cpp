// relp_engine_pool.cpp -- the column pools of the unsharded tableau engine in phase 2 (relp_pool_create .. relp_pool_stats): the
// candidate columns of a column-generation master kept on the device, priced there against -pi as the tableau holds it, the
// winners picked there, the chosen ones added as relp_add_columns adds them.  See relp_pool.hpp (the layout, the segments, the
// stale rule), relp_kernels.h (the launches) and DESIGN.md 10.
//
// Pricing reads d_d_, d_cost_store_ and d_idcol_ -- (-pi)_i = d[idcol[i]] - cost_store[idcol[i]], what relp_get_minus_pi forms on
// the host -- and the pool; it writes scratch of the pool alone.  The tableau engine keeps d up to date at every pivot and every
// in-place call, so nothing is flushed, settled beyond the shadow row or re-armed, and the record is not even downloaded.
#include "relp_engine_internal.hpp"

#include <algorithm>
#include <cmath>

namespace relp {

namespace {
// the one buffer a price downloads: [d of the winners (segments doubles) | their pool indices (segments) | their number]
struct PriceOut {
    double* d; int32_t* k; int32_t* found;
    static size_t bytes(int32_t segments) { return sizeof(double) * (size_t)segments + sizeof(int32_t) * ((size_t)segments + 1); }
    PriceOut(char* base, int32_t segments)
        : d(reinterpret_cast<double*>(base)), k(reinterpret_cast<int32_t*>(base + sizeof(double) * (size_t)segments)), found(k + segments) {}
};
constexpr int32_t kPoolOneDownload = 4096;             // segments up to which the whole buffer comes down in one copy
}  // namespace

// The shared front: the engine and phase, the pool is one of this handle's and, where `fresh` is asked, not stale.
relp_status_t Engine::pool_ready(const char* what, const relp_pool* pool, bool fresh) {
    const relp_status_t st = dual_ready(what);
    if (st) return st;
    const bool mine = pool && std::any_of(pools_.begin(), pools_.end(), [&](const auto& p) { return p.get() == pool; });
    if (!mine) return fail(RELP_E_ARG, std::string(what) + ": not a pool of this handle");
    // (rows_at_create > m cannot outlive pools_mark_stale; tested all the same: a pool row beyond the engine's rows is never read)
    if (fresh && (pool->stale || pool_stale_after_rollback(pool->image.rows_at_create, lay_.m)))
        return fail(RELP_E_STATE, std::string(what) + ": the pool is stale (relp_remove_cuts or the rollback of a trial took out an engine row below the " +
                                      std::to_string(pool->image.rows_at_create) + " rows the pool was created over)");
    return RELP_OK;
}

// The stale rule where engine rows go (relp_pool.hpp).  rows == nullptr: the rows from lay_.m on went (the rollback of a trial takes
// back the cut rows added inside it); else the listed engine rows did (relp_remove_cuts).  Stale is for good: a cut added later in
// the place of a row that went is another row.
void Engine::pools_mark_stale(const int32_t* rows, int32_t count) {
    for (auto& pool : pools_)
        if (rows ? pool_stale_after_removal(pool->image.rows_at_create, rows, count) : pool_stale_after_rollback(pool->image.rows_at_create, lay_.m))
            pool->stale = true;
}

PoolView Engine::pool_view(const relp_pool& pool) const {
    return PoolView{pool.d_slice_ptr, pool.d_row, pool.d_val, pool.d_cost, pool.d_active, pool.image.count};
}

relp_status_t Engine::pool_create(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost,
                                  relp_pool** out) {
    relp_status_t st = dual_ready("relp_pool_create");
    if (st) return st;
    if (!out) return fail(RELP_E_ARG, "relp_pool_create: the pool pointer is missing");
    *out = nullptr;
    if ((st = lay_.check_columns(count, col_ptr, row_idx, values, cost, &err_))) {      // the checks of relp_add_columns, in its words
        const std::string from = "relp_add_columns";
        if (err_.compare(0, from.size(), from) == 0) err_.replace(0, from.size(), "relp_pool_create");
        return st;
    }
    auto pool = std::make_unique<relp_pool>();
    pool->image = pool_pack(count, col_ptr, row_idx, values, cost, lay_.m);
    const PoolImage& im = pool->image;
    HIP_TRY(pool->d_slice_ptr.alloc((int64_t)im.slice_ptr.size()));
    HIP_TRY(pool->d_row.alloc(im.stored()));
    HIP_TRY(pool->d_val.alloc(im.stored()));
    HIP_TRY(pool->d_cost.alloc(count));
    HIP_TRY(pool->d_active.alloc(count));
    // under one wait (no return before it: the image is in flight)
    hipError_t e = pool->d_slice_ptr.upload(im.slice_ptr, enqueue_only(stream_));
    e = first_error(e, pool->d_row.upload(im.ell_row, enqueue_only(stream_)));
    e = first_error(e, pool->d_val.upload(im.ell_val, enqueue_only(stream_)));
    e = first_error(e, pool->d_cost.upload(im.cost, enqueue_only(stream_)));
    HIP_TRY(first_error(e, pool->d_active.fill_bytes(1, count, stream_)));
    *out = pool.get();
    pools_.push_back(std::move(pool));
    return RELP_OK;
}

relp_status_t Engine::pool_destroy(relp_pool* pool) {
    const auto it = std::find_if(pools_.begin(), pools_.end(), [&](const auto& p) { return p.get() == pool; });
    if (it == pools_.end()) return fail(RELP_E_ARG, "relp_pool_destroy: not a pool of this handle");
    (void)hipStreamSynchronize(stream_);
    pools_.erase(it);
    return RELP_OK;
}

relp_status_t Engine::pool_stats(const relp_pool* pool, int64_t* out4) const {
    if (!pool || std::none_of(pools_.begin(), pools_.end(), [&](const auto& p) { return p.get() == pool; })) return RELP_E_ARG;
    return in_place_stats(out4, pool->image.count, pool->image.nonzeros(), pool->image.stored(), pool->price_calls);
}

relp_status_t Engine::pool_set_active(relp_pool* pool, const int32_t* ids, int32_t count, int32_t flag) {
    relp_status_t st = pool_ready("relp_pool_set_active", pool, false);
    if (st) return st;
    if (flag != 0 && flag != 1) return fail(RELP_E_ARG, "relp_pool_set_active: flag is neither 0 nor 1");
    if (const char* why = pool_check_ids(ids, count, pool->image.count)) return fail(RELP_E_ARG, std::string("relp_pool_set_active: ") + why);
    if (count == 0) return RELP_OK;
    HIP_TRY(d_pool_ids_.ensure(count, 256));
    hipError_t e = d_pool_ids_.upload(ids, count, enqueue_only(stream_));
    if (e == hipSuccess) launch_pool_set_active(pool_view(*pool), d_pool_ids_, count, flag, stream_);
    HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_pool_set_active: a kernel launch failed");
    return RELP_OK;
}

// The launches of a price (segments >= 1) or of the reduced costs alone (segments == 0, d_all written); the caller downloads.
relp_status_t Engine::pool_launch_price(relp_pool& pool, int32_t segments, double tol, bool all) {
    const int32_t count = pool.image.count;
    if (all) HIP_TRY(pool.d_all.ensure_raw(sizeof(double) * (size_t)std::max(count, 1)));
    PriceOut po(nullptr, 0);
    if (segments > 0) {
        const size_t parts = (size_t)segments * (size_t)pool_segment_chunks(count, segments);
        HIP_TRY(pool.d_part_d.ensure_raw(sizeof(double) * parts));
        HIP_TRY(pool.d_part_k.ensure_raw(sizeof(int32_t) * parts));
        HIP_TRY(pool.d_out.ensure_raw(PriceOut::bytes(segments)));
        po = PriceOut(pool.d_out, segments);
    }
    HIP_TRY(d_pool_minus_pi_.ensure(lay_.m, 256));
    tab_settle();
    launch_pool_price(pool_view(pool), minus_pi_view(), segments, tol, all ? (double*)pool.d_all : nullptr, pool.d_part_d, pool.d_part_k, po.k,
                      po.d, po.found, stream_);
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
    if (const char* why = pool_check_price_args(pool->image.count, segments, tol, ids_out, d_out, found))
        return fail(RELP_E_ARG, std::string("relp_pool_price: ") + why);
    *found = 0;
    if (pool->image.count == 0) { ++pool->price_calls; return RELP_OK; }
    if ((st = pool_launch_price(*pool, segments, tol, false))) return st;
    // one download: the whole buffer while it is small, else the number of winners first and then the winners alone
    const PriceOut po(pool->d_out, segments);
    int32_t n = 0;
    if (segments <= kPoolOneDownload) {
        std::vector<char> host(PriceOut::bytes(segments));
        HIP_TRY(download_from(host.data(), (const char*)pool->d_out, host.size(), stream_));
        const PriceOut ho(host.data(), segments);
        n = std::min(std::max(*ho.found, 0), segments);
        std::copy(ho.k, ho.k + n, ids_out);
        std::copy(ho.d, ho.d + n, d_out);
    } else {
        HIP_TRY(download_from(&n, po.found, 1, stream_));
        n = std::min(std::max(n, 0), segments);
        const hipError_t e = download_from(ids_out, po.k, (size_t)n, enqueue_only(stream_));
        HIP_TRY(first_error(e, n ? download_from(d_out, po.d, (size_t)n, stream_) : hipStreamSynchronize(stream_)));
    }
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_pool_price: a kernel launch failed");
    *found = n;
    ++pool->price_calls;                               // (a call that failed is not counted)
    return RELP_OK;
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
    if (const char* why = pool_check_ids(ids, count, pool->image.count)) return fail(RELP_E_ARG, std::string("relp_pool_add: ") + why);
    if (count == 0) return RELP_OK;
    const PoolChoice ch = pool_choose(pool->image, ids, count, lay_.m);
    HIP_TRY(d_pool_ids_.ensure(count, 256));
    if (sw_.pool_host_add) {
        if ((st = add_columns(count, ch.col_ptr.data(), ch.row_idx.data(), ch.values.data(), ch.cost.data()))) return st;
        hipError_t e = d_pool_ids_.upload(ids, count, enqueue_only(stream_));
        if (e == hipSuccess) launch_pool_set_active(pool_view(*pool), d_pool_ids_, count, 0, stream_);
        HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
        return RELP_OK;
    }
    if ((st = room_for_columns("relp_pool_add", count))) return st;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    const int32_t entries = ch.entries, added_old = lay_.nr_added;
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
    return columns_added(count, ch.col_ptr.data(), ch.row_idx.data(), ch.values.data(), ch.cost.data(), entries, p);
}

}  // namespace relp
