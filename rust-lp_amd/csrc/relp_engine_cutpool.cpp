// relp_engine_cutpool.cpp -- the cut pools of the unsharded tableau engine in phase 2 (relp_cutpool_create .. relp_cutpool_stats):
// the candidate rows of a row-generation scheme kept on the device, separated there against the vertex as the tableau holds it, the
// winners picked there, the chosen ones added as relp_add_cuts adds them.  The mirror image of relp_engine_pool.cpp.  See
// relp_cutpool.hpp (the layout, the norms), relp_kernels.h (the launches) and DESIGN.md 10.
//
// Separation reads d_b_ and d_basis_ -- x_j = b[r] where structural column j is basic in row r -- and the pool; it writes scratch
// alone.  The tableau engine keeps b and the basis up to date at every pivot and every in-place call, so nothing is flushed,
// settled beyond the shadow row or re-armed, and the record is not even downloaded.
#include "relp_engine_internal.hpp"

#include <algorithm>
#include <cmath>

namespace relp {

namespace {
// the one buffer a separation downloads: [slacks of the winners (segments doubles) | their pool indices (segments) | their number]
struct SeparateOut {
    double* s; int32_t* k; int32_t* found;
    static size_t bytes(int32_t segments) { return sizeof(double) * (size_t)segments + sizeof(int32_t) * ((size_t)segments + 1); }
    SeparateOut(char* base, int32_t segments)
        : s(reinterpret_cast<double*>(base)), k(reinterpret_cast<int32_t*>(base + sizeof(double) * (size_t)segments)), found(k + segments) {}
};
constexpr int32_t kCutPoolOneDownload = 4096;          // segments up to which the whole buffer comes down in one copy
}  // namespace

// The shared front: the engine and phase, the pool is one of this handle's.  (No stale rule: the structural columns never move.)
relp_status_t Engine::cutpool_ready(const char* what, const relp_cutpool* pool) {
    const relp_status_t st = dual_ready(what);
    if (st) return st;
    const bool mine = pool && std::any_of(cutpools_.begin(), cutpools_.end(), [&](const auto& p) { return p.get() == pool; });
    if (!mine) return fail(RELP_E_ARG, std::string(what) + ": not a cut pool of this handle");
    return RELP_OK;
}

CutPoolView Engine::cutpool_view(const relp_cutpool& pool) const {
    return CutPoolView{PoolView{pool.d_slice_ptr, pool.d_col, pool.d_val, pool.d_rhs, pool.d_active, pool.image.count()}, pool.d_norm};
}

relp_status_t Engine::cutpool_create(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs,
                                     relp_cutpool** out) {
    relp_status_t st = dual_ready("relp_cutpool_create");
    if (st) return st;
    if (!out) return fail(RELP_E_ARG, "relp_cutpool_create: the pool pointer is missing");
    *out = nullptr;
    if ((st = lay_.check_cuts(count, row_ptr, col_idx, values, rhs, &err_))) {           // the checks of relp_add_cuts, in its words
        const std::string from = "relp_add_cuts";
        if (err_.compare(0, from.size(), from) == 0) err_.replace(0, from.size(), "relp_cutpool_create");
        return st;
    }
    auto pool = std::make_unique<relp_cutpool>();
    pool->image = cutpool_pack(count, row_ptr, col_idx, values, rhs, lay_.nr_normal);
    const PoolImage& im = pool->image.ell;
    HIP_TRY(pool->d_slice_ptr.alloc((int64_t)im.slice_ptr.size()));
    HIP_TRY(pool->d_col.alloc(im.stored()));
    HIP_TRY(pool->d_val.alloc(im.stored()));
    HIP_TRY(pool->d_rhs.alloc(count));
    HIP_TRY(pool->d_norm.alloc(count));
    HIP_TRY(pool->d_active.alloc(count));
    // under one wait (no return before it: the image is in flight)
    hipError_t e = pool->d_slice_ptr.upload(im.slice_ptr, enqueue_only(stream_));
    e = first_error(e, pool->d_col.upload(im.ell_row, enqueue_only(stream_)));
    e = first_error(e, pool->d_val.upload(im.ell_val, enqueue_only(stream_)));
    e = first_error(e, pool->d_rhs.upload(im.cost, enqueue_only(stream_)));
    e = first_error(e, pool->d_norm.upload(pool->image.norm, enqueue_only(stream_)));
    HIP_TRY(first_error(e, pool->d_active.fill_bytes(1, count, stream_)));
    *out = pool.get();
    cutpools_.push_back(std::move(pool));
    return RELP_OK;
}

relp_status_t Engine::cutpool_destroy(relp_cutpool* pool) {
    const auto it = std::find_if(cutpools_.begin(), cutpools_.end(), [&](const auto& p) { return p.get() == pool; });
    if (it == cutpools_.end()) return fail(RELP_E_ARG, "relp_cutpool_destroy: not a cut pool of this handle");
    (void)hipStreamSynchronize(stream_);
    cutpools_.erase(it);
    return RELP_OK;
}

relp_status_t Engine::cutpool_stats(const relp_cutpool* pool, int64_t* out4) const {
    if (!pool || std::none_of(cutpools_.begin(), cutpools_.end(), [&](const auto& p) { return p.get() == pool; })) return RELP_E_ARG;
    return in_place_stats(out4, pool->image.count(), pool->image.ell.nonzeros(), pool->image.ell.stored(), pool->separate_calls);
}

relp_status_t Engine::cutpool_set_active(relp_cutpool* pool, const int32_t* ids, int32_t count, int32_t flag) {
    relp_status_t st = cutpool_ready("relp_cutpool_set_active", pool);
    if (st) return st;
    if (flag != 0 && flag != 1) return fail(RELP_E_ARG, "relp_cutpool_set_active: flag is neither 0 nor 1");
    if (const char* why = cutpool_check_ids(ids, count, pool->image.count())) return fail(RELP_E_ARG, std::string("relp_cutpool_set_active: ") + why);
    if (count == 0) return RELP_OK;
    HIP_TRY(d_pool_ids_.ensure(count, 256));
    hipError_t e = d_pool_ids_.upload(ids, count, enqueue_only(stream_));
    if (e == hipSuccess) launch_pool_set_active(cutpool_view(*pool).pv, d_pool_ids_, count, flag, stream_);
    HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_cutpool_set_active: a kernel launch failed");
    return RELP_OK;
}

// The launches of a separation (segments >= 1) or of the slacks alone (segments == 0); the caller downloads.
relp_status_t Engine::cutpool_launch_separate(relp_cutpool& pool, int32_t segments, double tol, int32_t by_efficacy) {
    const int32_t count = pool.image.count();
    HIP_TRY(pool.d_all.ensure_raw(sizeof(double) * (size_t)std::max(count, 1)));
    SeparateOut so(nullptr, 0);
    if (segments > 0) {
        const size_t parts = (size_t)segments * (size_t)pool_segment_chunks(count, segments);
        HIP_TRY(pool.d_part_d.ensure_raw(sizeof(double) * parts));
        HIP_TRY(pool.d_part_k.ensure_raw(sizeof(int32_t) * parts));
        HIP_TRY(pool.d_out.ensure_raw(SeparateOut::bytes(segments)));
        so = SeparateOut(pool.d_out, segments);
    }
    HIP_TRY(d_cutpool_x_.ensure(std::max(lay_.nr_normal, 1), 256));
    tab_settle();
    launch_cutpool_separate(cutpool_view(pool), vertex_view(), segments, tol, by_efficacy, pool.d_all, pool.d_part_d, pool.d_part_k, so.k, so.s,
                            so.found, stream_);
    return RELP_OK;
}

relp_status_t Engine::cutpool_slacks(relp_cutpool* pool, double* out_count) {
    relp_status_t st = cutpool_ready("relp_cutpool_slacks", pool);
    if (st) return st;
    if (pool->image.count() == 0) return RELP_OK;
    if (!out_count) return fail(RELP_E_ARG, "relp_cutpool_slacks: the output array is missing");
    if ((st = cutpool_launch_separate(*pool, 0, 0.0, 0))) return st;
    HIP_TRY(download_from(out_count, (const double*)pool->d_all, (size_t)pool->image.count(), stream_));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_cutpool_slacks: a kernel launch failed");
    return RELP_OK;
}

relp_status_t Engine::cutpool_separate(relp_cutpool* pool, int32_t segments, double tol, int32_t by_efficacy, int32_t* ids_out,
                                       double* slack_out, int32_t* found) {
    relp_status_t st = cutpool_ready("relp_cutpool_separate", pool);
    if (st) return st;
    if (const char* why = cutpool_check_separate_args(pool->image.count(), segments, tol, by_efficacy, ids_out, slack_out, found))
        return fail(RELP_E_ARG, std::string("relp_cutpool_separate: ") + why);
    *found = 0;
    if (pool->image.count() == 0) { ++pool->separate_calls; return RELP_OK; }
    if ((st = cutpool_launch_separate(*pool, segments, tol, by_efficacy))) return st;
    // one download: the whole buffer while it is small, else the number of winners first and then the winners alone
    const SeparateOut so(pool->d_out, segments);
    int32_t n = 0;
    if (segments <= kCutPoolOneDownload) {
        std::vector<char> host(SeparateOut::bytes(segments));
        HIP_TRY(download_from(host.data(), (const char*)pool->d_out, host.size(), stream_));
        const SeparateOut ho(host.data(), segments);
        n = std::min(std::max(*ho.found, 0), segments);
        std::copy(ho.k, ho.k + n, ids_out);
        std::copy(ho.s, ho.s + n, slack_out);
    } else {
        HIP_TRY(download_from(&n, so.found, 1, stream_));
        n = std::min(std::max(n, 0), segments);
        const hipError_t e = download_from(ids_out, so.k, (size_t)n, enqueue_only(stream_));
        HIP_TRY(first_error(e, n ? download_from(slack_out, so.s, (size_t)n, stream_) : hipStreamSynchronize(stream_)));
    }
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_cutpool_separate: a kernel launch failed");
    *found = n;
    ++pool->separate_calls;                            // (a call that failed is not counted)
    return RELP_OK;
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
    relp_status_t st = cutpool_ready("relp_cutpool_add", pool);
    if (st) return st;
    if (const char* why = cutpool_check_ids(ids, count, pool->image.count())) return fail(RELP_E_ARG, std::string("relp_cutpool_add: ") + why);
    if (count == 0) return RELP_OK;
    const CutPoolChoice ch = cutpool_choose(pool->image, ids, count, lay_.nr_normal);
    HIP_TRY(d_pool_ids_.ensure(count, 256));
    if (sw_.cutpool_host_add) {
        if ((st = add_cuts(count, ch.row_ptr.data(), ch.col_idx.data(), ch.values.data(), ch.rhs.data()))) {
            const std::string from = "relp_add_cuts";
            if (err_.compare(0, from.size(), from) == 0) err_.replace(0, from.size(), "relp_cutpool_add");
            return st;
        }
        hipError_t e = d_pool_ids_.upload(ids, count, enqueue_only(stream_));
        if (e == hipSuccess) launch_pool_set_active(cutpool_view(*pool).pv, d_pool_ids_, count, 0, stream_);
        HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
        return RELP_OK;
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
    return cuts_added(count, ch.row_ptr.data(), ch.col_idx.data(), ch.values.data(), ch.rhs.data(), entries, p);
}

}  // namespace relp
