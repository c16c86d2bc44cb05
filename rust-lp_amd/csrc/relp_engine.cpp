// relp_engine.cpp -- host driver: problem upload, phase logic, launch sequencing.  See relp_engine.hpp.
#include "relp_engine_internal.hpp"
#include "relp_gomory.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace relp {

bool Engine::hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    err_ = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}

// the buffers free themselves (members), the events and the stream go last (EngineQueue)
Engine::~Engine() { rccl_release(); luf_release(); }

ColumnTable Engine::table() const {
    ColumnTable ct;
    ct.nr_artificial = lay_.nr_artificial;
    ct.nr_normal = lay_.nr_normal;
    ct.nr_virtual = lay_.nr_virtual;
    ct.nr_constraints = lay_.mc;
    ct.column_to_row = d_column_to_row_;
    ct.bound_row = d_bound_row_;
    ct.vrow0 = d_vrow0_;
    ct.vrow1 = d_vrow1_;
    ct.vsign = d_vsign_;
    ct.cost = d_cost_;
    ct.cut_row0 = lay_.cut_row0;
    ct.nr_cuts = lay_.nr_cuts;
    return ct;
}

Tolerances Engine::tolerances() const { return Tolerances{cfg_.tol_cost, cfg_.tol_pivot, cfg_.tol_zero, cfg_.tol_tie, cfg_.ratio_rule, (pivot_guard_on_ && guard_rel_ > 0.0) ? 1 : 0, guard_rel_}; }

TableauView Engine::tview() const {
    TableauView tv;
    // only the owned storage columns [sc_lo, sc_hi) are stored; shift so kernels index globally
    tv.T0 = dT0_ - (int64_t)lay_.sc_lo * ld_t_; tv.ld_t = ld_t_;
    tv.R0 = dR0_ - (int64_t)lay_.sc_lo; tv.ld_r = ld_r_;
    tv.d = d_d_; tv.m = lay_.m; tv.n_store = n_store_;
    tv.col_off = phase_ == 1 ? 0 : tab_na_;
    tv.n = nr_columns();
    tv.c_lo = lay_.sc_lo; tv.c_hi = lay_.sc_hi;
    return tv;
}

FlushList Engine::flush_list() const {
    FlushList fl;
    fl.cols = d_fcols_; fl.count = d_fcount_; fl.mask = d_fmask_; fl.R0c = d_R0c_; fl.ld = ld_r_; fl.stats = d_fstats_;
    return fl;
}

SelectPartials Engine::tab_partials(int rule) const {
    SelectPartials sp;
    sp.k1 = d_part_k1_; sp.j = d_part_j_; sp.in_basis = d_in_basis_; sp.tol_cost = cfg_.tol_cost; sp.rule = rule;
    sp.n = nr_columns(); sp.offset = 0; sp.nb_struct = 0; sp.tol_tie = cfg_.tol_tie; sp.p_lo = 0; sp.cols_per_slot = 8;
    return sp;
}

DeferredUpdate Engine::deferred() const {
    DeferredUpdate du;
    du.W = d_W_; du.ld = ld_b_; du.kmax = block_; du.S = d_S_; du.pos_of_row = d_pos_of_row_; du.wr = d_wr_; du.R = d_R_;
    du.batch = load_batch_; du.w_split = w_split_;
    return du;
}

// device -> host on the engine's stream, and wait for it (a caller's output array, or a piece carved out of a buffer)
relp_status_t Engine::fetch(void* dst, const void* src, size_t bytes) { HIP_RETURN(download_from((char*)dst, src, bytes, stream_)); }

relp_status_t Engine::download_rec() { HIP_RETURN(d_rec_.download(h_rec_, 1, stream_)); }

relp_status_t Engine::upload_rec() { HIP_RETURN(d_rec_.upload(h_rec_, 1, stream_)); }

relp_status_t Engine::set_stream(hipStream_t s) {
    if (stream_) HIP_TRY(hipStreamSynchronize(stream_));       // the new stream does not order with work left on the old one
    if (owns_stream_ && stream_) HIP_TRY(hipStreamDestroy(stream_));
    stream_ = s;
    owns_stream_ = false;
    return RELP_OK;
}

Switches Switches::read() {
    Switches s;
    auto given = [](const char* name) { return std::getenv(name) != nullptr; };
    auto num = [](const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; };
    s.debug = given("RELP_DEBUG");
    s.pivot_guard_set = given("RELP_PIVOT_GUARD");
    if (s.pivot_guard_set) s.pivot_guard = std::atof(std::getenv("RELP_PIVOT_GUARD"));
    s.tab_flush_all = num("RELP_TAB_FLUSH_ALL", 0) != 0;
    s.tab_load_batch = num("RELP_TAB_LOAD_BATCH", 0);
    s.tab_w_split = num("RELP_TAB_W_SPLIT", 0);
    s.tab_column_rows = num("RELP_TAB_COLUMN_ROWS", 0);
    s.fused_update = num("RELP_FUSED_UPDATE", 1) != 0;
    s.lu_lookahead_set = given("RELP_LU_LOOKAHEAD");
    s.lu_lookahead = num("RELP_LU_LOOKAHEAD", 8);
    s.fuse_lanes = num("RELP_FUSE_LANES", 256);
    s.lu_device_factor = num("RELP_LU_DEVICE_FACTOR", 0);
    s.lu_pipeline_short = num("RELP_LU_PIPELINE_SHORT", 0) != 0;
    s.ft_big = num("RELP_FT_BIG", -1);
    s.ft_hyper_set = given("RELP_FT_HYPER");
    s.ft_hyper = num("RELP_FT_HYPER", 0x9);
    s.ft_grid_price = given("RELP_FT_GRID_PRICE") ? (num("RELP_FT_GRID_PRICE", 0) != 0 ? 1 : 0) : -1;
    if (given("RELP_LUF_BUMP_CAP")) s.luf_bump_cap = std::max(16, num("RELP_LUF_BUMP_CAP", 0));
    s.luf_dense = std::max(0, std::min(64, num("RELP_LUF_DENSE", 64)));
    s.luf_lds = num("RELP_LUF_LDS", 1) != 0;
    s.lu_peel_stacks = num("RELP_LU_PEEL_STACKS", 0) != 0;
    s.dump_basis_set = given("RELP_DUMP_BASIS");
    if (s.dump_basis_set) s.dump_basis = std::getenv("RELP_DUMP_BASIS");
    s.retab_global = num("RELP_RETAB_GLOBAL", 0) != 0;
    s.retab_groups = std::max(0, num("RELP_RETAB_GROUPS", 0));
    s.tab_rhs_splits = std::max(0, num("RELP_TAB_RHS_SPLITS", 0));
    s.tab_cost_splits = std::max(0, num("RELP_TAB_COST_SPLITS", 0));
    s.trial_memcpy = num("RELP_TRIAL_MEMCPY", 0) != 0;
    s.pool_host_add = num("RELP_POOL_HOST_ADD", 0) != 0;
    s.cutpool_host_add = num("RELP_CUTPOOL_HOST_ADD", 0) != 0;
    return s;
}

// ------------------------------------------------------------------------------------------------
// Construction: MatrixData layout (matrix_data.rs:198-268, 308-371, 432-452) and the partially
// artificial start (partially.rs:125-206, carry/mod.rs:381-426)
// ------------------------------------------------------------------------------------------------
relp_status_t Engine::create(const relp_matrix_data_t& md, const relp_config_t& cfg) {
    (void)hipGetLastError();                               // (the launch check at the end must only see this create's launches)
    cfg_ = cfg;
    sw_ = Switches::read();
    // (measurement aid: the relative threshold of the guard that relp_run's pivot rescue switches on)
    if (sw_.pivot_guard_set && cfg_.pivot_rescue && cfg_.shard_count <= 1) guard_rel_ = sw_.pivot_guard;
    if (cfg_.shard_count < 1) cfg_.shard_count = 1;
    if (cfg_.poll_interval < 1) cfg_.poll_interval = 64;
    if (const relp_status_t lst = lay_.build(md, cfg_, &err_)) return lst;
    if (cfg_.device >= 0) HIP_TRY(hipSetDevice(cfg_.device));
    phase_ = 1;
    n_alloc_ = lay_.nr_columns();

    // ---- device allocations ----
    HIP_TRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    owns_stream_ = true;
    const int32_t n_local = lay_.col_hi - lay_.col_lo;
    lu_ = lay_.engine == RELP_ENGINE_LU;
    tableau_ = lay_.engine == RELP_ENGINE_TABLEAU;
    if (lu_) {
        if (cfg_.shard_count > 1) return fail(RELP_E_UNSUPPORTED, "the LU engine is not sharded");
        relp_status_t lst = lu_load_matrix(md);
        if (lst) return lst;
    } else if (md.format == RELP_FORMAT_DENSE) {
        if (lay_.nr_normal > 0 && lay_.mc > 0 && !md.dense) return fail(RELP_E_ARG, "dense matrix missing");
        const int64_t src_ld = md.dense_ld > 0 ? md.dense_ld : lay_.mc;
        if (src_ld < lay_.mc) return fail(RELP_E_ARG, "dense_ld < nr_constraints");
        // In sharded mode `dense` holds only the owned columns [col_lo, col_hi).
        if (md.matrix_memory == RELP_MEM_DEVICE && (src_ld % 2) == 0) {
            dA_.adopt(const_cast<double*>(md.dense), src_ld * std::max(n_local, 1)); ld_a_ = src_ld;      // zero-copy adoption
        } else {
            ld_a_ = round_up(std::max<int64_t>(lay_.mc, 1), 2);
            HIP_TRY(dA_.alloc(ld_a_ * std::max(n_local, 1)));
            HIP_TRY(dA_.copy_2d(md.matrix_memory == RELP_MEM_DEVICE ? kFromDevice : kFromHost, md.dense, src_ld, lay_.mc, n_local, ld_a_, stream_));
        }
    } else if (md.format == RELP_FORMAT_CSC) {
        if (md.matrix_memory != RELP_MEM_HOST) return fail(RELP_E_UNSUPPORTED, "CSC input must be in host memory");
        if (!md.col_ptr) return fail(RELP_E_ARG, "col_ptr missing");
        ld_a_ = round_up(std::max<int64_t>(lay_.mc, 1), 2);
        // the dense engines' copy of the owned columns, scattered on the device from the CSC arrays (never staged dense on the host)
        const int64_t e0 = n_local > 0 ? md.col_ptr[lay_.col_lo] : 0, e1 = n_local > 0 ? md.col_ptr[lay_.col_hi] : 0;
        for (int64_t p = e0; p < e1; ++p)
            if (md.row_idx[p] < 0 || md.row_idx[p] >= lay_.mc) return fail(RELP_E_ARG, "row index out of range");
        const int64_t cells = ld_a_ * std::max(n_local, 1);
        HIP_TRY(dA_.alloc(cells));
        HIP_TRY(dA_.zero(cells, stream_));
        if (e1 > e0) {
            DeviceBuf<int64_t> t_ptr; DeviceBuf<int32_t> t_idx; DeviceBuf<double> t_val;       // staging: freed on every way out
            if (t_ptr.alloc_raw(sizeof(int64_t) * (size_t)(n_local + 1)) != hipSuccess ||
                t_idx.alloc_raw(sizeof(int32_t) * (size_t)(e1 - e0)) != hipSuccess ||
                t_val.alloc_raw(sizeof(double) * (size_t)(e1 - e0)) != hipSuccess)
                return fail(RELP_E_ALLOC, "staging the CSC arrays");
            hipError_t err = t_ptr.upload(md.col_ptr + lay_.col_lo, n_local + 1, stream_);
            if (err == hipSuccess) err = t_idx.upload(md.row_idx + e0, e1 - e0, stream_);
            if (err == hipSuccess) err = t_val.upload(md.values + e0, e1 - e0, stream_);
            if (err == hipSuccess) {
                launch_csc_to_dense(t_ptr, t_idx, t_val, n_local, dA_, ld_a_, nullptr);
                err = hipDeviceSynchronize();              // (the staging buffers are freed at the end of this block)
            }
            if (err != hipSuccess) return fail(RELP_E_HIP, "dense copy of the CSC input");
        }
    } else {
        return fail(RELP_E_ARG, "unknown matrix format");
    }

    ld_b_ = round_up(lay_.m, 16);
    const int64_t rows_local = std::max(lay_.row_hi - lay_.row_lo, 1);
    // the tableau engine reads B^-1 off the identity columns of T; the explicit inverse is not stored
    HIP_TRY(dBinv_.alloc((tableau_ || lu_) ? 16 : rows_local * ld_b_));
    HIP_TRY(d_minus_pi_.alloc(ld_b_));
    HIP_TRY(d_b_.alloc(ld_b_));
    HIP_TRY(d_alpha_.alloc(ld_b_));
    HIP_TRY(d_aq_.alloc(ld_b_));
    HIP_TRY(d_rho_.alloc(ld_b_));
    HIP_TRY(d_w_.alloc(ld_b_));
    HIP_TRY(d_d_.alloc(n_alloc_));
    HIP_TRY(d_cost_.alloc(lay_.nr_normal));
    HIP_TRY(d_basis_.alloc(lay_.m));
    HIP_TRY(d_column_to_row_.alloc(lay_.nr_artificial));
    HIP_TRY(d_bound_row_.alloc(lay_.nr_normal));
    HIP_TRY(d_vrow0_.alloc(lay_.nr_virtual));
    HIP_TRY(d_vrow1_.alloc(lay_.nr_virtual));
    HIP_TRY(d_vsign_.alloc(lay_.nr_virtual));
    HIP_TRY(d_in_basis_.alloc(n_alloc_));
    HIP_TRY(d_rec_.alloc(1));
    {
        const int64_t slots = price_structural_blocks(lay_.col_lo, lay_.col_hi) + (lay_.nr_artificial + lay_.nr_virtual + 255) / 256 + 8 +
                              tab_scan_blocks(n_alloc_) + price_csc_blocks(0, lay_.nr_normal);
        HIP_TRY(d_part_k1_.alloc(slots));
        HIP_TRY(d_part_j_.alloc(slots));
    }
    block_ = cfg_.update_block < 0 ? (lay_.m >= 4096 ? 64 : 0) : std::min(cfg_.update_block, 128);
    if (lu_) {
        // pivots between refactorisations (the reference refactors after 10 updates, lower_upper/mod.rs:199;
        // here an update is one column of W, so longer blocks are cheap)
        block_ = cfg_.update_block < 0 ? 128 : std::max(1, std::min(cfg_.update_block, 128));
        HIP_TRY(d_lu_scratch_.alloc(ld_b_));
        HIP_TRY(h_basis_.alloc(sizeof(int32_t) * (size_t)std::max(lay_.m, 1)));      // (rows are only ever removed)
        luf_enabled_ = sw_.lu_device_factor != 0;
        luf_download_ = sw_.lu_device_factor == 2;
        relp_status_t fst = ft_plan_and_alloc();           // Forrest-Tomlin on the device when the LDS budget allows
        if (fst) return fst;
    }
    if (tableau_) {
        if (block_ == 0) block_ = 64;                  // the tableau is always maintained in blocks
        // automatic choice for wide tableaus: 96 pivots per flush where the flush dominates the pivot.  Measured: 10,000 x
        // 50,000 (60,000 stored columns) 19,600 it/s against 18,600 with 64; at 10,000 x 10,000 (20,000 stored columns) the gain is
        // within the noise of the windows (+0.8 %) while the flush kernel leaves its best operating point (0.58 instead of 0.61
        // of HBM peak: more arithmetic per byte), so 64 stays there.
        if (cfg_.update_block < 0 && lay_.m >= 4096 && n_alloc_ >= 40000) block_ = 96;
        n_store_ = n_alloc_;
        tab_na_ = lay_.nr_artificial;
        const int64_t n_owned = std::max(lay_.sc_hi - lay_.sc_lo, 1);
        ld_t_ = round_up(lay_.m, 2);
        ld_r_ = round_up(n_owned, 2);
        HIP_TRY(dT0_.alloc(ld_t_ * n_owned));
        HIP_TRY(dR0_.alloc(ld_r_ * (block_ + 1)));        // + one scratch row (d_aq_big)
        {   // the flush rewrites only the columns with a nonzero R0 entry unless RELP_TAB_FLUSH_ALL=1
            flush_all_ = sw_.tab_flush_all;
            HIP_TRY(d_fstats_.alloc(2));
            if (!flush_all_) {
                HIP_TRY(d_fcols_.alloc(n_owned));
                HIP_TRY(d_fcount_.alloc(1));
                HIP_TRY(d_fmask_.alloc((n_owned + 63) / 64));
                HIP_TRY(d_R0c_.alloc(ld_r_ * block_));
            }
        }
        {   // pending rows loaded per round trip in the per-pivot kernels (1 = one by one, the control), and the workgroups per 256
            // rows that share W <- E W in the fused update: RELP_TAB_LOAD_BATCH, RELP_TAB_W_SPLIT
            load_batch_ = tab_load_batch(sw_.tab_load_batch);
            w_split_ = sw_.tab_w_split >= 1 ? std::min(sw_.tab_w_split, 16) : kTabSplitDefault;
            // rows per workgroup of the column kernel in the fused single-GPU loop: RELP_TAB_COLUMN_ROWS (256 = the control)
            col_rows_wanted_ = sw_.tab_column_rows;
        }
        {   // two launches per pivot instead of three in the single-GPU loop (RELP_FUSED_UPDATE=0: k_ratio_blocks + k_tab_update_all)
            fused_update_ = sw_.fused_update;               // (also the native sharded loop, relp_shard_run)
            if (cfg_.pivot_rescue && cfg_.shard_count == 1) fused_update_ = false;       // (the pivot guard lives in the shared ratio epilogue)
            if (fused_update_) {
                HIP_TRY(d_b_alt_.alloc(ld_b_));
                HIP_TRY(d_basis_alt_.alloc(lay_.m));
                HIP_TRY(d_shadow_.alloc(std::max(block_, 1) + 1));
                HIP_TRY(d_shadow_meta_.alloc_raw(2 * sizeof(int32_t)));
                const int32_t none[2] = {-1, 0};
                HIP_TRY(d_shadow_meta_.upload(none, 2, stream_));
            }
        }
        HIP_TRY(d_cost_store_.alloc(n_store_));
        HIP_TRY(d_idcol_.alloc(lay_.m));
        if (cfg_.shard_count == 1) {                       // scratch of relp_change_right_hand_side
            HIP_TRY(d_rhs_cols_.alloc(lay_.m));
            HIP_TRY(d_rhs_delta_.alloc(lay_.m));
            HIP_TRY(d_rhs_v_.alloc(std::max(block_, 1)));
            // ... and of relp_change_cost: a structural column is basic in at most one row, or not at all
            const int32_t basic_most = std::min(lay_.m, lay_.nr_normal);
            HIP_TRY(d_cost_rows_.alloc(basic_most));
            HIP_TRY(d_cost_delta_.alloc(basic_most));
            HIP_TRY(d_cost_ncols_.alloc(lay_.nr_normal));
            HIP_TRY(d_cost_ndelta_.alloc(lay_.nr_normal));
            HIP_TRY(d_cost_u_.alloc(std::max(block_, 1)));
        }
    }
    if (block_ > 0) HIP_TRY(d_v_.alloc(ld_b_));
    if (block_ > 0 && !ft_) {                              // (Forrest-Tomlin: no W, the update file lives in FtState)
        HIP_TRY(d_W_.alloc(ld_b_ * block_));
        if (!tableau_) HIP_TRY(d_R_.alloc(ld_b_ * block_));
        HIP_TRY(d_wr_.alloc(block_));
        HIP_TRY(d_S_.alloc(block_));
        HIP_TRY(d_pos_of_row_.alloc(lay_.m));
        HIP_TRY(d_pos_of_row_.fill_bytes(0xFF, lay_.m, stream_));               // -1 everywhere
    }
    HIP_TRY(d_rmin_.alloc(lay_.m / 8 + 2));          // block minima of the ratio test (8, 64, 128 or 256 rows per block)
    HIP_TRY(h_rec_.alloc(sizeof(PivotRecord)));
    trace_cap_ = std::max(cfg_.trace_capacity, 0);
    if (trace_cap_ > 0) HIP_TRY(d_trace_.alloc(4 * trace_cap_));

    HIP_TRY(d_cost_.upload(lay_.cost.data(), lay_.nr_normal, stream_));
    HIP_TRY(d_bound_row_.upload(lay_.bound_row.data(), lay_.nr_normal, stream_));
    HIP_TRY(d_vrow0_.upload(lay_.vrow0.data(), lay_.nr_virtual, stream_));
    HIP_TRY(d_vrow1_.upload(lay_.vrow1.data(), lay_.nr_virtual, stream_));
    HIP_TRY(d_vsign_.upload(lay_.vsign.data(), lay_.nr_virtual, stream_));
    HIP_TRY(d_column_to_row_.upload(lay_.column_to_row.data(), lay_.nr_artificial, stream_));
    HIP_TRY(d_basis_.upload(lay_.basis.data(), lay_.m, stream_));
    HIP_TRY(d_b_.upload(lay_.rhs.data(), lay_.m, stream_));
    HIP_TRY(d_minus_pi_.upload(lay_.minus_pi.data(), lay_.m, stream_));
    std::vector<uint8_t> flags(n_alloc_, 0);
    for (int32_t r = 0; r < lay_.m; ++r) flags[lay_.basis[r]] = 1;
    HIP_TRY(d_in_basis_.upload(flags, stream_));
    // identity rows [row_lo, row_hi): local row i has its 1 in column row_lo + i (BasisInverse::identity)
    if (lay_.row_hi > lay_.row_lo && !tableau_ && !lu_) launch_set_identity(dBinv_, ld_b_, lay_.row_lo, lay_.row_hi, stream_);
    if (tableau_) {
        // T0 = the original matrix in row space (B = I), d = c - c_B' T0 with the phase-1 costs
        idcol_h_ = lay_.basis;                               // the initial basis column of row k is e_k
        HIP_TRY(d_idcol_.upload(idcol_h_.data(), lay_.m, stream_));
        launch_tab_build(tview(), A_base(), ld_a_, table(), stream_);
        cost_store_h_.assign(n_store_, 0.0);
        for (int32_t k = 0; k < lay_.nr_artificial; ++k) cost_store_h_[k] = 1.0;
        std::vector<double> w(ld_b_, 0.0);
        for (int32_t k = 0; k < lay_.nr_artificial; ++k) w[lay_.column_to_row[k]] = 1.0;
        HIP_TRY(d_cost_store_.upload(cost_store_h_, stream_));
        HIP_TRY(d_w_.upload(w, stream_));
        launch_tab_price_init(tview(), d_w_, d_cost_store_, stream_);
    }
    // f64 only: the explicit inverse / the tableau is updated thousands of times on long solves; for sparse problems
    // below 4,097 rows (where the host factorisation of a basis is cheap: CSC input with at most 10 % nonzeros) it is
    // rebuilt from the basis columns every 1,000 pivots (relp_set_reinversion_interval changes or enables it)
    {
        bool sparse_input = false;
        if (md.format == RELP_FORMAT_CSC && md.col_ptr && lay_.nr_normal > 0 && lay_.mc > 0)
            sparse_input = (double)md.col_ptr[lay_.nr_normal] <= 0.10 * (double)lay_.nr_normal * (double)lay_.mc;
        reinvert_interval_ = (!lu_ && cfg_.shard_count == 1 && lay_.m <= 4096 && sparse_input) ? 1000 : 0;
        // relp_config_t.auto_reinversion: any LP, starting at 256 pivots; every rebuild measures what it corrected and adapts
        if (cfg_.auto_reinversion && !lu_ && cfg_.shard_count == 1) reinvert_interval_ = 256;
    }
    std::memset(h_rec_, 0, sizeof(PivotRecord));
    h_rec_->outcome = DEV_RUNNING;
    h_rec_->minus_objective = -lay_.phase1_objective;
    h_rec_->last_selected = -1;
    h_rec_->phase = 1;
    relp_status_t st = upload_rec();
    if (st) return st;
    HIP_TRY(hipDeviceSynchronize());   // the end of create: the set-up kernels have run before the launch check below reads their errors
    // (a refused launch -- e.g. more than 2^32 - 1 threads -- returns nothing by itself: without this the engine would start
    // from a tableau that was never built)
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "a kernel launch of the set-up failed");
    if (lu_ && (st = lu_refactor())) return st;
    return RELP_OK;
}

// ------------------------------------------------------------------------------------------------
// Profiling
// ------------------------------------------------------------------------------------------------
relp_status_t Engine::profile_enable(bool enable, int64_t max_launches, int32_t sample_every) {
    prof_stride_ = sample_every > 0 ? sample_every : 1;
    prof_tick_ = 0;
    HIP_TRY(hipStreamSynchronize(stream_));                // the events destroyed below may still be pending
    for (auto e : prof_ev_) (void)hipEventDestroy(e);
    prof_ev_.clear(); prof_kid_.clear(); prof_open_ = false;
    prof_on_ = enable;
    if (enable) {
        prof_ev_.resize((size_t)max_launches * 2);
        for (auto& e : prof_ev_) HIP_TRY(hipEventCreate(&e));
        prof_kid_.reserve((size_t)max_launches);
    }
    return RELP_OK;
}

void Engine::prof_begin(int kid, hipStream_t on) {
    prof_open_ = false;
    if (!prof_on_ || (prof_kid_.size() + 1) * 2 > prof_ev_.size()) return;
    if (kid != RELP_K_FLUSH && (prof_tick_ % prof_stride_) != 0) return;   // sampled pivots only
    (void)hipEventRecord(prof_ev_[2 * prof_kid_.size()], on ? on : stream_);
    prof_kid_.push_back(kid);
    prof_open_ = true;
}

void Engine::prof_end(hipStream_t on) {
    if (!prof_open_) return;
    (void)hipEventRecord(prof_ev_[2 * (prof_kid_.size() - 1) + 1], on ? on : stream_);
    prof_open_ = false;
}

relp_status_t Engine::profile_read(int kernel_id, int64_t* launches, double* total_ms) {
    HIP_TRY(hipStreamSynchronize(stream_));                // the events read below must have been reached
    int64_t n = 0; double ms = 0.0;
    for (size_t k = 0; k < prof_kid_.size(); ++k) {
        if (prof_kid_[k] != kernel_id) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, prof_ev_[2 * k], prof_ev_[2 * k + 1]) == hipSuccess) { ms += t; ++n; }
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    return RELP_OK;
}

// ------------------------------------------------------------------------------------------------
// One pivot on the device
// ------------------------------------------------------------------------------------------------
// PRICE over the owned structural columns and every virtual column with vector `vec` (= -pi).
void Engine::enqueue_price(int cost_mode, const double* vec, const PivotRecord* rec, int32_t p_lo, int32_t p_hi) {
    const ColumnTable ct = table();
    if (lu_) {
        launch_price_csc(csc(), ct, vec, d_d_, 0, lay_.nr_normal, cost_mode, SelectPartials{}, rec, stream_);
        launch_price_virtual(ct, vec, d_d_, cost_mode, rec, stream_);
        return;
    }
    launch_price_structural(A_base(), ld_a_, ct, vec, d_d_, p_lo, p_hi, cost_mode, rec, stream_);
    if (p_lo > 0 || p_hi < lay_.nr_normal) launch_price_mask_unowned(ct, d_d_, p_lo, p_hi, rec, stream_);
    launch_price_virtual(ct, vec, d_d_, cost_mode, rec, stream_);
}

// One pivot of the dense-tableau engine: 5 launches, O(K (m + n)) bytes.
void Engine::enqueue_iteration_tableau(int rule) {
    const TableauView tv = tview();
    DeferredUpdate du = deferred();
    const SelectPartials sp = tab_partials(rule);
    // 3 launches: [PRICE's final reduction + tableau column] -> [ratio test + block bookkeeping] ->
    // [tableau row / reduced costs / next PRICE partials  ||  W, b, basis]
    if (fused_update_ && in_loop_) {
        // 2 launches: [PRICE's final reduction + tableau column + block minima of the ratios] -> [ratio test in every
        // workgroup + tableau row / reduced costs / next PRICE partials || W, b, basis]
        du.col_rows = tab_column_rows_size();              // this loop alone: every other caller of the two launches keeps 256
        prof_begin(RELP_K_FTRAN);
        launch_tab_select_column_rmin(tv, du, sp, tab_scan_blocks(lay_.sc_hi - lay_.sc_lo), d_alpha_, d_b_, tolerances(), d_rmin_,
                                      d_rec_, stream_, d_shadow_, d_shadow_meta_);
        prof_end();
        prof_begin(RELP_K_PRICE);
        launch_tab_ratio_update_all(tv, du, sp, lay_.m, d_alpha_, d_b_, d_b_alt_, d_basis_, d_basis_alt_, d_in_basis_, d_trace_,
                                    trace_cap_, tolerances(), d_rmin_, d_shadow_, d_shadow_meta_, d_rec_, stream_);
        prof_end();
        d_b_.swap(d_b_alt_);
        d_basis_.swap(d_basis_alt_);
        shadow_pending_ = true;
        if (++since_flush_ >= block_) enqueue_flush();
        return;
    }
    tab_settle();
    prof_begin(RELP_K_FTRAN);
    launch_tab_select_column_rmin(tv, du, sp, tab_scan_blocks(lay_.sc_hi - lay_.sc_lo), d_alpha_, d_b_, tolerances(), d_rmin_,
                                  d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_RATIO);
    launch_ratio_blocks(d_alpha_, d_b_, d_basis_, lay_.m, tolerances(), du, d_rmin_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_PRICE);
    launch_tab_update_all(tv, du, sp, lay_.m, d_alpha_, d_b_, d_basis_, d_in_basis_, d_trace_, trace_cap_, d_rec_, stream_);
    prof_end();
    if (++since_flush_ >= block_) enqueue_flush();
}

void Engine::enqueue_iteration(int rule) {
    struct Tick { int64_t& t; ~Tick() { ++t; } } tick{prof_tick_};
    if (tableau_) { enqueue_iteration_tableau(rule); return; }
    if (lu_) { enqueue_iteration_lu(rule); return; }
    const ColumnTable ct = table();
    const double* A = A_base();
    double* Binv = Binv_base();
    // PRICE with the partial argmin fused in, then one single-workgroup launch that picks the
    // entering column and builds it in row space
    const int nb_struct = price_structural_blocks(lay_.col_lo, lay_.col_hi);
    SelectPartials sp = tab_partials(rule);
    sp.nb_struct = nb_struct; sp.p_lo = lay_.col_lo;
    const int nb_virt = price_virtual_blocks(ct);
    prof_begin(RELP_K_PRICE);
    if (lay_.col_lo > 0 || lay_.col_hi < lay_.nr_normal) {
        launch_price_structural_sel(A, ld_a_, ct, d_minus_pi_, d_d_, lay_.col_lo, lay_.col_hi, phase_, sp, d_rec_, stream_);
        launch_price_mask_unowned(ct, d_d_, lay_.col_lo, lay_.col_hi, d_rec_, stream_);
        SelectPartials spv = sp;
        spv.offset = nb_struct;
        launch_price_virtual_sel(ct, d_minus_pi_, d_d_, phase_, spv, d_rec_, stream_);
    } else {
        launch_price_all_sel(A, ld_a_, ct, d_minus_pi_, d_d_, lay_.col_lo, lay_.col_hi, phase_, sp, d_rec_, stream_);
    }
    prof_end();
    prof_begin(RELP_K_SELECT_COLUMN);
    launch_select_partials(sp, nb_struct + nb_virt, d_d_, A, ld_a_, ct, lay_.m, d_aq_, d_rec_, stream_);
    prof_end();
    if (block_ == 0) {
        // explicit inverse, rank-1 update at every pivot (basis_inverse_rows.rs:131-142)
        // FTRAN leaves the minimum ratio of every 8 rows behind; the ratio test starts from those
        prof_begin(RELP_K_FTRAN);
        launch_ftran_rmin(Binv, ld_b_, lay_.m, d_aq_, d_alpha_, d_b_, tolerances(), d_rmin_, d_rec_, stream_);
        prof_end();
        prof_begin(RELP_K_RATIO);
        launch_ratio_rows(d_alpha_, d_b_, d_basis_, lay_.m, tolerances(), DeferredUpdate{}, d_rmin_, ftran_rows_per_block(), d_rec_,
                          stream_);
        prof_end();
        prof_begin(RELP_K_UPDATE_VECTORS);
        launch_compute_rho(Binv, ld_b_, lay_.m, lay_.row_lo, lay_.row_hi, d_rho_, d_rec_, stream_);
        prof_end();
        // rank-1 update of B^-1 together with b, -pi, -obj, basis, flags, trace
        prof_begin(RELP_K_UPDATE_INVERSE);
        launch_update_inverse_vectors(Binv, ld_b_, lay_.m, d_alpha_, d_rho_, d_b_, d_minus_pi_, d_basis_, d_in_basis_, d_trace_,
                                      trace_cap_, d_rec_, stream_);
        prof_end();
        return;
    }
    // deferred update: B^-1 = (I + W S') B0inv
    const DeferredUpdate du = deferred();
    prof_begin(RELP_K_FTRAN);
    launch_ftran(Binv, ld_b_, lay_.m, lay_.row_lo, lay_.row_hi, d_aq_, d_v_, 0, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_APPLY_W);
    launch_apply_w_rmin(du, lay_.m, d_v_, d_alpha_, d_b_, tolerances(), d_rmin_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_RATIO);
    launch_ratio_rows(d_alpha_, d_b_, d_basis_, lay_.m, tolerances(), du, d_rmin_, 256, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_UPDATE_W);
    launch_update_w(du, lay_.m, d_alpha_, d_rec_, stream_);
    launch_rho_deferred(du, Binv, ld_b_, lay_.m, lay_.row_lo, lay_.row_hi, d_rho_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_UPDATE_VECTORS);
    launch_update_vectors(lay_.m, d_alpha_, d_rho_, d_b_, d_minus_pi_, d_basis_, d_in_basis_, d_trace_, trace_cap_, d_rec_,
                          stream_);
    prof_end();
    if (++since_flush_ >= block_) enqueue_flush();
}

void Engine::tab_settle() {
    if (shadow_pending_) {                             // the fused update's new row r of W is still in its shadow row
        launch_tab_apply_shadow(deferred(), d_shadow_, d_shadow_meta_, stream_);
        shadow_pending_ = false;
    }
}

// Fold the pending pivots into the explicit inverse: B0inv += W (S' B0inv).  Valid in any state
// (also after the loop froze): (B0inv, W, S) is consistent after every completed pivot.
void Engine::enqueue_flush() {
    if (block_ == 0) return;
    if (lu_) {
        if (since_flush_ == 0 && !ft_need_refactor_) return;   // the factors already describe the current basis
        prof_begin(RELP_K_FLUSH);
        const relp_status_t st = lu_refactor();
        prof_end();
        if (st && !lu_status_) lu_status_ = st;
        return;
    }
    if (tableau_) {
        tab_settle();
        // T0 += W R0 on the f64 matrix cores
        const DeferredUpdate dut = deferred();
        prof_begin(RELP_K_FLUSH);
        launch_tab_flush(tview(), dut, d_rec_, flush_list(), stream_);
        launch_flush_reset(dut, d_rec_, stream_);
        prof_end();
        since_flush_ = 0;
        // The reduced costs are only ever updated (d -= theta * row); every few flushes they are recomputed
        // from the flushed tableau, d = c - c_B' T0, so that rounding does not pile up over thousands of
        // pivots (one extra pass over T0 per kRepriceEveryFlushes * K pivots).
        if (++flushes_since_reprice_ >= kRepriceEveryFlushes) {
            tableau_reprice();
        }
        return;
    }
    const DeferredUpdate du = deferred();
    double* Binv = Binv_base();
    prof_begin(RELP_K_FLUSH);
    launch_flush_snapshot(du, Binv, ld_b_, lay_.row_lo, lay_.row_hi, d_rec_, stream_);
    launch_flush_apply(du, Binv, ld_b_, lay_.m, lay_.row_lo, lay_.row_hi, d_rec_, stream_);
    launch_flush_reset(du, d_rec_, stream_);
    prof_end();
    since_flush_ = 0;
}

// d = c - c_B' T0 from the tableau as it is, and the PRICE partials of the new d
void Engine::tableau_reprice() {
    const TableauView tv = tview();
    flushes_since_reprice_ = 0;
    launch_tab_basis_costs(tv, d_basis_, d_cost_store_, d_w_, stream_);
    launch_tab_price_init(tv, d_w_, d_cost_store_, stream_);
    launch_tab_scan(tv, tab_partials(current_rule()), d_rec_, stream_);
}

relp_status_t Engine::flush() {
    if (const relp_status_t st = in_trial("relp_flush")) return st;
    tab_settle();
    if (cfg_.shard_count > 1 && block_ > 0 && !tableau_) {
        // the rows S' B0inv live on different ranks: with the collective hooks attached the library completes the
        // snapshot itself (every rank must call), otherwise the caller drives relp_shard_flush_begin / _end
        if (!coll_allreduce_) return fail(RELP_E_STATE, "sharded flush needs relp_shard_flush_begin/end (or the collective hooks)");
        if (since_flush_ == 0) return RELP_OK;
        double* snap = nullptr; int64_t len = 0;
        relp_status_t st = shard_flush_begin(&snap, &len);
        if (st) return st;
        if (len > 0) {
            if (coll_allreduce_(coll_ctx_, snap, len, stream_)) return fail(RELP_E_HIP, "all-reduce of the flush snapshot failed");
            if ((st = shard_flush_end())) return st;
        }
        since_flush_ = 0;
        return RELP_OK;
    }
    enqueue_flush();                                   // sharded tableau: the flush is local to the owned columns
    return RELP_OK;
}

// ---- step-wise API ------------------------------------------------------------------------------
relp_status_t Engine::select_primal_pivot_column(int rule, int32_t* found, int32_t* column, double* cost) {
    relp_status_t st = edit_rec();
    if (st) return st;
    if (tableau_) {
        const SelectPartials sp = tab_partials(rule);
        launch_tab_scan(tview(), sp, d_rec_, stream_);
        launch_tab_select(tview(), sp, tab_scan_blocks(lay_.sc_hi - lay_.sc_lo), d_rec_, stream_);
    } else {
        enqueue_price(phase_, d_minus_pi_, d_rec_, lay_.col_lo, lay_.col_hi);
        launch_select_column(d_d_, d_in_basis_, nr_columns(), rule, cfg_.tol_cost, cfg_.tol_tie, d_rec_, stream_);
    }
    if ((st = download_rec())) return st;
    const bool ok = h_rec_->outcome == DEV_RUNNING;
    if (found) *found = ok ? 1 : 0;
    if (ok) { if (column) *column = h_rec_->q; if (cost) *cost = h_rec_->d_q; }
    h_rec_->outcome = DEV_RUNNING;
    return upload_rec();
}

relp_status_t Engine::relative_costs(double* out_n) {
    if (!tableau_) enqueue_price(phase_, d_minus_pi_, nullptr, lay_.col_lo, lay_.col_hi);
    HIP_RETURN(d_d_.download(out_n, nr_columns(), stream_, tableau_ && phase_ != 1 ? tab_na_ : 0));     // the tableau keeps d up to date
}

relp_status_t Engine::generate_column(int32_t column, double* out_m) {
    if (column < 0 || column >= nr_columns()) return fail(RELP_E_ARG, "column out of range");
    const relp_status_t st = edit_rec([&](PivotRecord& r) { r.q = column; });
    if (st) return st;
    if (tableau_) {
        launch_tab_column(tview(), deferred(), d_alpha_, d_rec_, stream_);
    } else if (lu_ && ft_) {
        launch_ft_ftran(dlu_, fts_, ft_problem(0), column, nullptr, d_alpha_, stream_);     // leaves the spike for change_basis
    } else if (lu_) {
        launch_build_column_csc(csc(), table(), lay_.m, d_aq_, d_rec_, stream_);
        launch_lu_ftran(dlu_, d_aq_, d_v_, d_lu_scratch_, d_rec_, stream_);
        launch_apply_w(deferred(), lay_.m, d_v_, d_alpha_, d_rec_, stream_);
    } else {
        enqueue_flush();                               // the step-wise calls work on the explicit inverse
        launch_build_column(A_base(), ld_a_, table(), lay_.m, d_aq_, d_rec_, stream_);
        launch_ftran(Binv_base(), ld_b_, lay_.m, lay_.row_lo, lay_.row_hi, d_aq_, d_alpha_, 0, d_rec_, stream_);
    }
    // step-wise call: a failure of its kernels is reported by this call, with or without an output array
    HIP_RETURN(out_m ? d_alpha_.download(out_m, lay_.m, stream_) : hipStreamSynchronize(stream_));
}

relp_status_t Engine::generate_element(int32_t row, int32_t column, double* out) {
    if (row < 0 || row >= lay_.m) return fail(RELP_E_ARG, "row out of range");
    std::vector<double> col(lay_.m);
    relp_status_t st = generate_column(column, col.data());
    if (st) return st;
    if (out) *out = col[row];
    return RELP_OK;
}

// what the ratio test just enqueued decided; the record is re-armed after it has been read
relp_status_t Engine::read_pivot_row(int32_t* found, int32_t* row) {
    const relp_status_t st = download_rec();
    if (st) return st;
    const bool ok = h_rec_->outcome == DEV_RUNNING;
    if (found) *found = ok ? 1 : 0;
    if (ok && row) *row = h_rec_->r;
    h_rec_->outcome = DEV_RUNNING;
    return upload_rec();
}

relp_status_t Engine::select_primal_pivot_row(int32_t* found, int32_t* row) {
    launch_ratio(d_alpha_, d_b_, d_basis_, lay_.m, tolerances(), d_rec_, stream_);
    return read_pivot_row(found, row);
}

relp_status_t Engine::select_primal_pivot_row_of(const double* column, int32_t* found, int32_t* row) {
    HIP_TRY(d_aq_.upload(column, lay_.m, stream_));
    launch_ratio(d_aq_, d_b_, d_basis_, lay_.m, tolerances(), d_rec_, stream_);
    return read_pivot_row(found, row);
}

relp_status_t Engine::bring_into_basis(int32_t column, int32_t row, double cost, int32_t* leaving) {
    if (column < 0 || column >= nr_columns() || row < 0 || row >= lay_.m) return fail(RELP_E_ARG, "index out of range");
    relp_status_t st = in_trial("relp_bring_into_basis");
    if (st) return st;
    st = download_rec();
    if (st) return st;
    double alpha_r = 0.0, b_r = 0.0; int32_t lv = 0;
    HIP_TRY(d_alpha_.download(&alpha_r, 1, stream_, row));
    HIP_TRY(d_b_.download(&b_r, 1, stream_, row));
    HIP_TRY(d_basis_.download(&lv, 1, stream_, row));
    if (alpha_r == 0.0) return fail(RELP_E_ZERO_PIVOT, "Pivot value can't be zero.");
    if (!tableau_ && !lu_) enqueue_flush();
    st = edit_rec([&](PivotRecord& r) {                 // (a download of its own: the flush may have reset the block counters)
        r.q = column; r.d_q = cost; r.r = row; r.leaving = lv; r.alpha_r = alpha_r; r.b_r = b_r;
    });
    if (st) return st;
    if (tableau_) {
        const TableauView tv = tview();
        const DeferredUpdate du = deferred();
        const SelectPartials sp = tab_partials(current_rule());
        launch_eta_prepare(du, d_rec_, stream_);
        launch_tab_row_update(tv, du, sp, d_rec_, stream_);
        launch_update_w(du, lay_.m, d_alpha_, d_rec_, stream_);
        launch_tab_update_vectors(lay_.m, d_alpha_, d_b_, d_basis_, d_in_basis_, d_trace_, trace_cap_, d_rec_, stream_);
        if (++since_flush_ >= block_) enqueue_flush();
        HIP_TRY(hipStreamSynchronize(stream_));            // step-wise call: a failure of its kernels is reported by this call
        if (leaving) *leaving = lv;
        return RELP_OK;
    }
    if (lu_ && ft_) {
        // Carry::change_basis (carry/mod.rs:549-570): b, then the basis inverse (Forrest-Tomlin update with the spike
        // of the last generate_column), then -pi from row r of the NEW inverse
        const FtProblem pb = ft_problem(0);
        launch_ft_update(dlu_, fts_, pb, stream_);
        if ((st = ft_read_hdr())) return st;
        if (h_ft_hdr_[2] == 2) {
            // r did not fit the eta pool: refactorise the CURRENT basis, form the spike of the entering column again on
            // the fresh factors (alpha itself is unchanged) and update those
            std::vector<double> keep_alpha(lay_.m);
            HIP_TRY(d_alpha_.download(keep_alpha, stream_));
            if ((st = lu_refactor())) return st;
            launch_ft_ftran(dlu_, fts_, pb, column, nullptr, d_alpha_, stream_);
            HIP_TRY(d_alpha_.upload(keep_alpha, stream_));
            launch_ft_update(dlu_, fts_, pb, stream_);
        }
        launch_ft_btran(dlu_, fts_, pb, -2, nullptr, d_rho_, stream_);
        launch_update_vectors(lay_.m, d_alpha_, d_rho_, d_b_, d_minus_pi_, d_basis_, d_in_basis_, d_trace_, trace_cap_,
                              d_rec_, stream_);
        if ((st = ft_read_hdr())) return st;
        if (leaving) *leaving = lv;
        if (ft_need_refactor_) return lu_refactor();       // Carry::after_basis_change (carry/mod.rs:602-614)
        return RELP_OK;
    }
    if (lu_) {
        const DeferredUpdate du = deferred();
        launch_eta_prepare(du, d_rec_, stream_);
        launch_update_w(du, lay_.m, d_alpha_, d_rec_, stream_);
        launch_lu_btran(dlu_, du, nullptr, -1, d_rho_, d_lu_scratch_, d_rec_, stream_);
        launch_update_vectors(lay_.m, d_alpha_, d_rho_, d_b_, d_minus_pi_, d_basis_, d_in_basis_, d_trace_, trace_cap_,
                              d_rec_, stream_);
        if (++since_flush_ >= block_) enqueue_flush();
        HIP_TRY(hipStreamSynchronize(stream_));            // as above
        if (leaving) *leaving = lv;
        return take_lu_status();
    }
    double* Binv = Binv_base();
    launch_compute_rho(Binv, ld_b_, lay_.m, lay_.row_lo, lay_.row_hi, d_rho_, d_rec_, stream_);
    launch_update_vectors(lay_.m, d_alpha_, d_rho_, d_b_, d_minus_pi_, d_basis_, d_in_basis_, d_trace_, trace_cap_, d_rec_,
                          stream_);
    launch_update_inverse(Binv, ld_b_, lay_.m, lay_.row_lo, lay_.row_hi, d_alpha_, d_rho_, d_rec_, stream_);
    HIP_TRY(hipStreamSynchronize(stream_));                // as above
    if (leaving) *leaving = lv;
    return RELP_OK;
}

// ------------------------------------------------------------------------------------------------
// Loops (phase_one.rs:125-170, phase_two.rs:22-51)
// ------------------------------------------------------------------------------------------------
static constexpr int32_t kHeldNoCandidate = 100;          // run_loop: no candidate left while columns are barred (pivot_rescue)

relp_status_t Engine::robust_stats(int64_t* out4) const {
    out4[0] = rescue_small_pivots_; out4[1] = rescue_barred_; out4[2] = rescue_confirmations_; out4[3] = reinvert_interval_;
    return RELP_OK;
}

relp_status_t Engine::rescue_unbar_all() {
    if (barred_.empty()) return RELP_OK;
    const uint8_t zero = 0;
    for (int32_t j : barred_) HIP_TRY(d_in_basis_.upload(&zero, 1, stream_, j));
    barred_.clear();
    return RELP_OK;
}

// phase_one::primal / phase_two::primal with relp_config_t.pivot_rescue: the loop itself is run_loop(); an exit without a pivot
// row (phase_one.rs:143 panics there, phase_two.rs:44 returns Unbounded) is believed only when the entering column really has no
// entry worth pivoting on.
relp_status_t Engine::run(int64_t max_iters, int64_t* done, int32_t* outcome) {
    if (const relp_status_t st0 = in_trial("relp_run")) return st0;
    if (!cfg_.pivot_rescue || cfg_.shard_count > 1) return run_loop(max_iters, done, outcome);
    struct GuardScope { bool& g; GuardScope(bool& x) : g(x) { g = true; } ~GuardScope() { g = false; } } guard_scope(pivot_guard_on_);
    int64_t total = 0;
    int32_t oc = RELP_RUNNING;
    relp_status_t st;
    bool confirming = false;                  // the outcome is being re-checked with every column priced again
    for (int guard = 0;; ++guard) {
        int64_t d = 0;
        hold_phase_end_ = !barred_.empty();
        st = run_loop(std::max<int64_t>(max_iters - total, 0), &d, &oc);
        hold_phase_end_ = false;
        if (st) return st;
        total += d;
        if (d > 0) confirming = false;
        const bool no_row = oc == RELP_NO_ROW_PHASE_ONE || oc == RELP_UNBOUNDED;
        if (no_row && guard < 100000) {
            if (d > 0 && (st = rescue_unbar_all())) return st;             // the basis has changed: the bars are out of date
            const int32_t q = h_rec_->q;
            const double d_q = h_rec_->d_q;
            std::vector<double> alpha(lay_.m);
            HIP_TRY(d_alpha_.download(alpha, stream_));
            double amax = 0.0, apos = 0.0;
            for (double v : alpha) { amax = std::max(amax, std::fabs(v)); apos = std::max(apos, v); }
            const double rel = guard_rel_ > 0.0 ? guard_rel_ : cfg_.tol_pivot;       // the rescue's tolerance is relative to the column
            if (apos > 0.0 && apos >= rel * amax && apos > cfg_.tol_zero) {
                // a column with entries worth pivoting on relative to its own size (all of it small, or the loop's choice was
                // small beside larger entries): ONE pivot by the full-scan ratio test with the tolerance relative to the column
                const double keep = cfg_.tol_pivot;
                cfg_.tol_pivot = std::min(keep, std::max(rel * amax, 1e-300) * (1.0 - 1e-12));
                pivot_guard_on_ = false;
                int32_t found = 0, r = -1;
                st = generate_column(q, nullptr);
                if (!st) st = select_primal_pivot_row(&found, &r);
                if (!st && found) st = bring_into_basis(q, r, d_q, nullptr);
                cfg_.tol_pivot = keep;
                pivot_guard_on_ = true;
                if (st) return st;
                if (found) {
                    ++rescue_small_pivots_; ++total;
                    if ((st = edit_rec())) return st;                        // (the update kernels have counted and traced the pivot)
                    if (total >= max_iters) { oc = RELP_RUNNING; break; }
                    continue;
                }
            }
            if (apos <= 0.0 && barred_.empty() && !confirming) break;      // nothing positive at all: the outcome stands
            if (apos > 0.0 || !barred_.empty()) {
                if (apos <= 0.0) break;                                    // a genuinely unbounded column beside barred ones
                // positive entries that are noise beside the column's size (or below every tolerance): not a column to enter now
                const uint8_t two = 2;
                HIP_TRY(d_in_basis_.upload(&two, 1, stream_, q));
                barred_.push_back(q);
                ++rescue_barred_;
                if ((st = edit_rec())) return st;
                continue;
            }
            break;
        }
        if (oc == kHeldNoCandidate) {
            // no candidate left, but some columns were barred: price them again and see whether the outcome survives
            if (!confirming) {
                if ((st = rescue_unbar_all())) return st;
                confirming = true;
                ++rescue_confirmations_;
                if ((st = edit_rec())) return st;
                continue;
            }
            // barred again without a pivot in between: they stay out, the phase ends
            if ((st = download_rec())) return st;
            h_rec_->outcome = DEV_NO_CANDIDATE;
            if (phase_ == 2) oc = RELP_OPTIMAL;
            else if ((st = finish_phase_one(&oc))) return st;
            barred_.clear();                                               // (the phase switch rebuilt the flags)
            break;
        }
        break;
    }
    if (done) *done = total;
    if (outcome) *outcome = oc;
    return RELP_OK;
}

// What the downloaded record says about the phase: no candidate ends it (phase 1: the phase boundary runs here, unless the
// pivot rescue holds it back), no pivot row is unbounded / the reference's panic; anything else leaves RELP_RUNNING.
relp_status_t Engine::outcome_of_record(int32_t* oc) {
    if (h_rec_->outcome == DEV_NO_CANDIDATE) {
        if (hold_phase_end_) *oc = kHeldNoCandidate;
        else if (phase_ == 2) *oc = RELP_OPTIMAL;
        else return finish_phase_one(oc);
    } else if (h_rec_->outcome == DEV_NO_ROW) {
        *oc = phase_ == 2 ? RELP_UNBOUNDED : RELP_NO_ROW_PHASE_ONE;
    }
    return RELP_OK;
}

relp_status_t Engine::run_loop(int64_t max_iters, int64_t* done, int32_t* outcome) {
    if (ft_) return run_ft(max_iters, done, outcome);
    relp_status_t st = download_rec();
    if (st) return st;
    const long long start = h_rec_->iterations;
    const int rule = current_rule();
    // Phase 1 often ends after very few pivots (none at all with a full slack basis): poll at 1, 2, 4, ...
    // there so that an early end does not leave a long tail of no-op launches queued.
    if (tableau_) {
        // (re)entering the loop: rebuild the PRICE partials from d (afterwards every pivot leaves them behind)
        launch_tab_scan(tview(), tab_partials(rule), d_rec_, stream_);
        tab_partials_valid_ = true;
    }
    int64_t next_poll = phase_ == 1 ? 1 : cfg_.poll_interval;
    const auto t_enq0 = std::chrono::steady_clock::now();
    int64_t enqueued = 0;
    {
    LoopScope loop(*this);
    for (int64_t it = 0; it < max_iters && h_rec_->outcome == DEV_RUNNING; ++it) {
        enqueue_iteration(rule);
        ++enqueued;
        if (lu_status_) return take_lu_status();
        if (reinvert_interval_ > 0 && ++since_reinvert_ >= reinvert_interval_) {
            if ((st = download_rec())) return st;
            if (h_rec_->outcome != DEV_RUNNING) break;
            if ((st = reinvert())) return st;
        }
        if (it + 1 == next_poll) {
            next_poll += phase_ == 1 ? std::min<int64_t>(next_poll, cfg_.poll_interval) : cfg_.poll_interval;
            if ((st = download_rec())) return st;
            if (h_rec_->outcome != DEV_RUNNING) break;
        }
    }
    }
    if (sw_.debug && enqueued >= 64)
        std::fprintf(stderr, "[relp] run: %lld pivots enqueued in %.1f us of host time each\n", (long long)enqueued,
                     std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enq0).count() / enqueued);
    if ((st = download_rec())) return st;
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "kernel launch failed");
    int32_t oc = RELP_RUNNING;
    if ((st = outcome_of_record(&oc))) return st;
    if (done) *done = h_rec_->iterations - start;          // includes the zero-level pivots of the phase boundary
    if (outcome) *outcome = oc;
    return RELP_OK;
}

relp_status_t Engine::solve_relaxation(int64_t max_iters, int32_t* outcome) {
    int32_t oc = RELP_RUNNING; int64_t done = 0, total = 0;
    relp_status_t st;
    if ((st = in_trial("relp_solve_relaxation"))) return st;
    if (phase_ == 1) {
        if ((st = run(max_iters, &done, &oc))) return st;
        total += done;
        if (oc != RELP_PHASE_ONE_DONE) { if (outcome) *outcome = oc; return RELP_OK; }
    }
    if ((st = run(std::max<int64_t>(max_iters - total, 0), &done, &oc))) return st;
    if (outcome) *outcome = oc;
    return RELP_OK;
}

// ------------------------------------------------------------------------------------------------
// Dual simplex on the tableau (the reference's primal_dual module is an empty placeholder): from a basis whose reduced costs
// are non-negative, pivot until b = B^-1 rhs is.  Selection by the dual kernels (relp_kernels.h), the pivot itself by the
// update of the primal loop; ratio_rule and pivot_rescue do not apply.
// ------------------------------------------------------------------------------------------------
relp_status_t Engine::dual_ready(const char* what) {
    if (!tableau_ || cfg_.shard_count > 1) return fail(RELP_E_UNSUPPORTED, std::string(what) + " is for the unsharded tableau engine");
    if (phase_ != 2) return fail(RELP_E_STATE, std::string(what) + " needs a phase-2 tableau (relp_from_basis, or phase 1 done)");
    return RELP_OK;
}

// The shared front of everything that works in place on the tableau as it stands: the fused update's shadow row settled, the
// record downloaded, *p = the pending rows of the open block.  Does not flush.
relp_status_t Engine::settled_pending(int32_t* p) {
    tab_settle();
    const relp_status_t st = download_rec();
    if (st) return st;
    *p = h_rec_->n_eta;
    return RELP_OK;
}

// The four counters of an in-place function's *_stats, behind the guard they share (no error text: a stats query leaves the
// handle's last error alone).
relp_status_t Engine::in_place_stats(int64_t* out4, int64_t s0, int64_t s1, int64_t s2, int64_t s3) const {
    if (!tableau_ || cfg_.shard_count > 1) return RELP_E_UNSUPPORTED;
    if (phase_ != 2) return RELP_E_STATE;
    out4[0] = s0; out4[1] = s1; out4[2] = s2; out4[3] = s3;
    return RELP_OK;
}

// A named list (index_k, value_k) of a change: the lists are there, every index is in [0, bound) (else `what`: `outside`), none is
// named twice (`noun`) and every value is finite.
relp_status_t Engine::check_named_list(const char* what, const int32_t* index, const double* values, int32_t count, int32_t bound,
                                       const char* noun, const char* outside) {
    const std::string fn = std::string(what) + ": ";
    if (count < 0 || (count > 0 && (!index || !values))) return fail(RELP_E_ARG, fn + "count < 0 or a list missing");
    std::vector<uint8_t> named(bound, 0);
    for (int32_t k = 0; k < count; ++k) {
        if (index[k] < 0 || index[k] >= bound) return fail(RELP_E_ARG, fn + outside);
        if (named[index[k]]) return fail(RELP_E_ARG, fn + "a " + noun + " named twice");
        if (!std::isfinite(values[k])) return fail(RELP_E_ARG, fn + "a value that is not finite");
        named[index[k]] = 1;
    }
    return RELP_OK;
}

// One dual pivot: 5 launches.  [block minima of the infeasible b_i] -> [row r of T + partial minima of the dual ratios] ->
// [entering column + tableau column] -> [alpha_r, b_r, block bookkeeping] -> [the update of the primal loop]
void Engine::enqueue_iteration_dual() {
    struct Tick { int64_t& t; ~Tick() { ++t; } } tick{prof_tick_};
    const TableauView tv = tview();
    const DeferredUpdate du = deferred();
    const SelectPartials sp = tab_partials(current_rule());
    const Tolerances tol = tolerances();
    // relp_profile_read has the primal loop's classes only: RATIO = block minima + commit (the row choice), PRICE = row r of T +
    // the update (as in the primal loop, whose update carries the next PRICE), FTRAN = entering column + tableau column
    prof_begin(RELP_K_RATIO);
    launch_dual_bmin(d_b_, lay_.m, cfg_.tol_feas, d_rmin_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_PRICE);
    launch_dual_row(tv, du, sp, d_b_, d_basis_, tol, cfg_.tol_feas, d_rmin_, -1, d_aq_big(), d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_FTRAN);
    launch_dual_select_column(tv, du, sp, d_b_, d_basis_, tol, cfg_.tol_feas, d_rmin_, -1, d_aq_big(), d_alpha_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_RATIO);
    launch_dual_commit(d_alpha_, d_b_, du, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_PRICE);
    launch_tab_update_all(tv, du, sp, lay_.m, d_alpha_, d_b_, d_basis_, d_in_basis_, d_trace_, trace_cap_, d_rec_, stream_);
    prof_end();
    if (++since_flush_ >= block_) enqueue_flush();
}

relp_status_t Engine::run_dual(int64_t max_iters, int64_t* done, int32_t* outcome) {
    relp_status_t st = dual_ready("relp_run_dual");
    if (st) return st;
    if ((st = check_dual_feasible("relp_run_dual"))) return st;
    const long long start = h_rec_->iterations;
    const int64_t since_flush_start = since_flush_;
    tab_partials_valid_ = false;
    int64_t next_poll = cfg_.poll_interval;
    {
    LoopScope loop(*this);
    for (int64_t it = 0; it < max_iters && h_rec_->outcome == DEV_RUNNING; ++it) {
        // Inside a trial nothing may flush or re-invert (T0 and the pending rows of R0 are not in the snapshot): the loop pivots
        // only while the block is not left full, and the interval is suspended.
        if (trial_open_ && since_flush_ + 1 >= block_) break;
        enqueue_iteration_dual();
        if (!trial_open_ && reinvert_interval_ > 0 && ++since_reinvert_ >= reinvert_interval_) {
            if ((st = download_rec())) return st;
            if (h_rec_->outcome != DEV_RUNNING) break;
            if ((st = reinvert())) return st;
        }
        if (it + 1 == next_poll) {
            next_poll += cfg_.poll_interval;
            if ((st = download_rec())) return st;
            if (h_rec_->outcome != DEV_RUNNING) break;
        }
    }
    }
    if ((st = download_rec())) return st;
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "kernel launch failed");
    int32_t oc = RELP_RUNNING;
    if (h_rec_->outcome == DEV_NO_ROW) oc = RELP_OPTIMAL;                  // no infeasible row left
    else if (h_rec_->outcome == DEV_NO_CANDIDATE) oc = RELP_INFEASIBLE;    // an infeasible row without an entry to pivot on
    if (done) *done = h_rec_->iterations - start;
    if (outcome) *outcome = oc;
    // (inside a trial the room is counted in pivots made, not in iterations enqueued: the no-op iterations up to a poll use none)
    if (trial_open_) since_flush_ = since_flush_start + (h_rec_->iterations - start);
    h_rec_->outcome = DEV_RUNNING;                                          // (a primal loop may follow on this handle)
    return upload_rec();
}

// Dual feasibility of the current basis: PRICE finds no candidate among the non-basic columns.  Settles, re-arms the record and
// leaves it downloaded; the PRICE partials hold the scan's.
relp_status_t Engine::check_dual_feasible(const char* what) {
    tab_settle();
    relp_status_t st = edit_rec();
    if (st) return st;
    const SelectPartials sp = tab_partials(RELP_RULE_STEEPEST_DESCENT);
    launch_tab_scan(tview(), sp, d_rec_, stream_);
    launch_tab_select(tview(), sp, tab_scan_blocks(lay_.sc_hi - lay_.sc_lo), d_rec_, stream_);
    if ((st = download_rec())) return st;
    const bool dual_feasible = h_rec_->outcome == DEV_NO_CANDIDATE;
    const int32_t q = h_rec_->q;
    const double d_q = h_rec_->d_q;
    h_rec_->outcome = DEV_RUNNING;
    if ((st = upload_rec())) return st;
    if (!dual_feasible) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "%s: the basis is not dual feasible (column %d has reduced cost %.3e)", what, (int)q, d_q);
        return fail(RELP_E_STATE, msg);
    }
    return RELP_OK;
}

relp_status_t Engine::select_dual_pivot_row(int32_t* found, int32_t* row) {
    relp_status_t st = dual_ready("relp_select_dual_pivot_row");
    if (st) return st;
    if ((st = edit_rec())) return st;
    launch_dual_bmin(d_b_, lay_.m, cfg_.tol_feas, d_rmin_, d_rec_, stream_);
    launch_dual_select_row(d_b_, d_basis_, lay_.m, cfg_.tol_feas, cfg_.tol_tie, d_rmin_, d_rec_, stream_);
    return read_pivot_row(found, row);
}

relp_status_t Engine::select_dual_pivot_column(int32_t row, int32_t* found, int32_t* column) {
    relp_status_t st = dual_ready("relp_select_dual_pivot_column");
    if (st) return st;
    if (row < 0 || row >= lay_.m) return fail(RELP_E_ARG, "row out of range");
    if ((st = edit_rec())) return st;
    const TableauView tv = tview();
    const DeferredUpdate du = deferred();
    const SelectPartials sp = tab_partials(current_rule());
    launch_dual_row(tv, du, sp, d_b_, d_basis_, tolerances(), cfg_.tol_feas, d_rmin_, row, d_aq_big(), d_rec_, stream_);
    launch_dual_select_column(tv, du, sp, d_b_, d_basis_, tolerances(), cfg_.tol_feas, d_rmin_, row, d_aq_big(), d_alpha_, d_rec_,
                              stream_);
    tab_partials_valid_ = false;                       // (the partial slots now hold dual ratios)
    if ((st = download_rec())) return st;
    const bool ok = h_rec_->outcome == DEV_RUNNING;
    if (found) *found = ok ? 1 : 0;
    if (ok && column) *column = h_rec_->q;
    h_rec_->outcome = DEV_RUNNING;
    return upload_rec();
}

// A new right-hand side for the current basis: b = B^-1 rhs, the reduced costs and -obj by a re-tabulation (the reduced costs
// do not depend on rhs: a basis that was optimal stays dual feasible, and relp_run_dual takes it from there).
relp_status_t Engine::set_right_hand_side(const double* rhs_m) {
    relp_status_t st = dual_ready("relp_set_right_hand_side");
    if (st) return st;
    if ((st = in_trial("relp_set_right_hand_side"))) return st;
    if ((st = edit_rec())) return st;
    std::vector<double> keep(rhs_m, rhs_m + lay_.m);
    keep.swap(lay_.rhs);
    st = retabulate(false);                            // (b moves with rhs: nothing the re-inversion interval should adapt to)
    if (st || !retab_done_) {
        // a basis the factorisation declines leaves the old tableau and the old rhs in place; after a HIP error (st) the handle
        // is not guaranteed consistent, as everywhere else: b on the device may already belong to the new rhs
        keep.swap(lay_.rhs);
        return st ? st : fail(RELP_E_SINGULAR, "relp_set_right_hand_side: the basis could not be factorised");
    }
    tab_partials_valid_ = false;
    return RELP_OK;
}

// Single rhs entries moved on the current basis without a re-tabulation.  B^-1 is in the tableau -- the stored columns that were
// the identity at the start -- so b += sum_k delta_k T[:, idcol[row_k]] with T = T0 + W R0 over the pending rows of the open block
// (launch_tab_rhs_change).  d, the PRICE partials, the basis, the flags, W, R0 and T0 stay as they are; -obj is re-formed from the
// downloaded b as retabulate() forms it.  Settles the fused update's shadow row first, does not flush.
relp_status_t Engine::change_right_hand_side(const int32_t* rows, const double* values, int32_t count) {
    relp_status_t st = dual_ready("relp_change_right_hand_side");
    if (st) return st;
    if ((st = check_named_list("relp_change_right_hand_side", rows, values, count, lay_.m, "row", "row out of range"))) return st;
    if (count == 0) return RELP_OK;
    std::vector<int32_t> cols;
    std::vector<double> delta;
    for (int32_t k = 0; k < count; ++k) {
        const double dk = values[k] - lay_.rhs[rows[k]];
        if (dk == 0.0) continue;
        cols.push_back(idcol_h_[rows[k]]);
        delta.push_back(dk);
    }
    const int32_t cnt = (int32_t)cols.size();
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    h_rec_->outcome = DEV_RUNNING;
    if (cnt > 0) {
        const int32_t splits = tab_rhs_splits(lay_.m, cnt, sw_.tab_rhs_splits);
        if (splits > 1) HIP_TRY(d_rhs_partial_.ensure((int64_t)splits * ld_b_));
        // the two lists, b and the basis under one wait (no return before it: cols, delta, b are in flight; no launch on lost lists)
        hipError_t e = d_rhs_cols_.upload(cols, enqueue_only(stream_));
        e = first_error(e, d_rhs_delta_.upload(delta, enqueue_only(stream_)));
        if (e == hipSuccess) launch_tab_rhs_change(tview(), deferred(), RhsChange{d_rhs_cols_, d_rhs_delta_, cnt}, p, splits, d_rhs_v_, d_b_,
                                                   d_rhs_partial_, ld_b_, stream_);
        std::vector<double> b(lay_.m);                     // (allocated while the kernel runs)
        std::vector<int32_t> basis(lay_.m);
        e = first_error(e, d_b_.download(b, enqueue_only(stream_)));
        HIP_TRY(first_error(e, d_basis_.download(basis, stream_)));
        if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_change_right_hand_side: a kernel launch failed");
        h_rec_->minus_objective = -objective_of(basis, b);
        rhs_last_splits_ = splits;
    }
    for (int32_t k = 0; k < count; ++k) lay_.rhs[rows[k]] = values[k];
    ++rhs_changes_;
    rhs_columns_ += cnt;
    rhs_last_p_ = p;
    return upload_rec();
}

relp_status_t Engine::set_upper_bound(int32_t column, double value) {
    const relp_status_t st = dual_ready("relp_set_upper_bound");
    if (st) return st;
    if (column < 0 || column >= lay_.nr_normal) return fail(RELP_E_ARG, "relp_set_upper_bound: not a structural column");
    const int32_t row = lay_.bound_row[column];
    if (row < 0) return fail(RELP_E_ARG, "relp_set_upper_bound: the column had no finite upper bound at create (a bound row cannot be added here)");
    if (!std::isfinite(value)) return fail(RELP_E_ARG, "relp_set_upper_bound: the bound must be finite (a bound row cannot be dropped here)");
    return change_right_hand_side(&row, &value, 1);
}

relp_status_t Engine::get_right_hand_side(double* out_m) {
    const relp_status_t st = dual_ready("relp_get_right_hand_side");
    if (st) return st;
    std::copy(lay_.rhs.begin(), lay_.rhs.begin() + lay_.m, out_m);
    return RELP_OK;
}

relp_status_t Engine::rhs_stats(int64_t* out4) const { return in_place_stats(out4, rhs_changes_, rhs_columns_, rhs_last_p_, rhs_last_splits_); }

// The three copies of lay_.cost[lo, hi) the tableau engine keeps: d_cost_ (ColumnTable), cost_store_h_ (relp_get_minus_pi) and
// d_cost_store_ (every reprice and re-tabulation), the latter two by storage column.
relp_status_t Engine::store_costs(int32_t lo, int32_t hi) {
    if (hi <= lo) return RELP_OK;
    std::copy(lay_.cost.begin() + lo, lay_.cost.begin() + hi, cost_store_h_.begin() + tab_na_ + lo);
    hipError_t e = d_cost_.upload(lay_.cost.data() + lo, hi - lo, enqueue_only(stream_), lo);
    HIP_RETURN(first_error(e, d_cost_store_.upload(lay_.cost.data() + lo, hi - lo, stream_, tab_na_ + lo)));
}

// Cost coefficients moved on the current basis without a flush or a re-tabulation: the mirror image of change_right_hand_side.
// d = c - c_B' T, so a changed basic column (basic in row r_k, delta_k) moves every non-basic d by -delta_k T[r_k, :] and a changed
// non-basic column moves its own d by +delta; T = T0 + W R0 over the pending rows of the open block (launch_tab_cost_change).  The
// basic list is sorted by row: the summation order, and neighbouring rows of a column of T0 share a sector.  b, the basis, the
// flags, W, R0 and T0 stay as they are; -obj is re-formed from the downloaded b with the new costs.
relp_status_t Engine::change_cost(const int32_t* columns, const double* values, int32_t count) {
    relp_status_t st = dual_ready("relp_change_cost");
    if (st) return st;
    if ((st = check_named_list("relp_change_cost", columns, values, count, lay_.nr_normal, "column", "not a structural column"))) return st;
    if (count == 0) return RELP_OK;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    h_rec_->outcome = DEV_RUNNING;
    std::vector<int32_t> basis(lay_.m);
    HIP_TRY(d_basis_.download(basis, stream_));
    std::vector<int32_t> row_of(lay_.nr_normal, -1);       // structural column -> the row it is basic in
    for (int32_t i = 0; i < lay_.m; ++i)
        if (basis[i] >= 0 && basis[i] < lay_.nr_normal) row_of[basis[i]] = i;
    std::vector<std::pair<int32_t, double>> basic, nonbasic;      // (row, delta), (storage column, delta)
    int32_t lo = lay_.nr_normal, hi = 0;
    for (int32_t k = 0; k < count; ++k) {
        const double dk = values[k] - lay_.cost[columns[k]];
        if (dk == 0.0) continue;
        lo = std::min(lo, columns[k]); hi = std::max(hi, columns[k] + 1);
        if (row_of[columns[k]] >= 0) basic.emplace_back(row_of[columns[k]], dk);
        else nonbasic.emplace_back(tab_na_ + columns[k], dk);
    }
    const auto by_index = [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) { return a.first < b.first; };
    std::sort(basic.begin(), basic.end(), by_index);
    std::sort(nonbasic.begin(), nonbasic.end(), by_index);
    const int32_t cnt = (int32_t)basic.size(), ncnt = (int32_t)nonbasic.size();
    if (cnt + ncnt > 0) {
        std::vector<int32_t> rows(cnt), ncols(ncnt);
        std::vector<double> delta(cnt), ndelta(ncnt);
        for (int32_t k = 0; k < cnt; ++k) { rows[k] = basic[k].first; delta[k] = basic[k].second; }
        for (int32_t k = 0; k < ncnt; ++k) { ncols[k] = nonbasic[k].first; ndelta[k] = nonbasic[k].second; }
        const int32_t splits = tab_cost_splits(n_store_, cnt, sw_.tab_cost_splits);
        if (splits > 1) HIP_TRY(d_cost_partial_.ensure((int64_t)splits * ld_r_));
        // the four lists and b under one wait (no return before it: the lists and b are in flight; no launch on lost lists)
        hipError_t e = d_cost_rows_.upload(rows, enqueue_only(stream_));
        e = first_error(e, d_cost_delta_.upload(delta, enqueue_only(stream_)));
        e = first_error(e, d_cost_ncols_.upload(ncols, enqueue_only(stream_)));
        e = first_error(e, d_cost_ndelta_.upload(ndelta, enqueue_only(stream_)));
        if (e == hipSuccess) launch_tab_cost_change(tview(), deferred(), CostChange{d_cost_rows_, d_cost_delta_, cnt, d_cost_ncols_, d_cost_ndelta_, ncnt},
                                                    d_in_basis_, p, splits, d_cost_u_, d_cost_partial_, ld_r_, stream_);
        std::vector<double> b(lay_.m);                     // (allocated while the kernel runs)
        HIP_TRY(first_error(e, d_b_.download(b, stream_)));
        if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_change_cost: a kernel launch failed");
        for (int32_t k = 0; k < count; ++k) lay_.cost[columns[k]] = values[k];
        if ((st = store_costs(lo, hi))) return st;
        h_rec_->minus_objective = -objective_of(basis, b);
        tab_partials_valid_ = false;
        cost_last_splits_ = splits;
    }
    ++cost_changes_;
    cost_rows_ += cnt;
    cost_last_p_ = p;
    return upload_rec();
}

// Every structural cost at once by the route the engine has: the open block flushed, d = c - c_B' T0 in one coalesced pass over T0
// (tableau_reprice), -obj from b.  No factorisation and no re-tabulation.
relp_status_t Engine::set_cost(const double* cost_n) {
    relp_status_t st = dual_ready("relp_set_cost");
    if (st) return st;
    if ((st = in_trial("relp_set_cost"))) return st;
    for (int32_t j = 0; j < lay_.nr_normal; ++j)
        if (!std::isfinite(cost_n[j])) return fail(RELP_E_ARG, "relp_set_cost: a value that is not finite");
    tab_settle();
    if ((st = edit_rec())) return st;
    if (h_rec_->n_eta > 0 && (st = flush())) return st;
    std::copy(cost_n, cost_n + lay_.nr_normal, lay_.cost.begin());
    if ((st = store_costs(0, lay_.nr_normal))) return st;
    tableau_reprice();
    tab_partials_valid_ = false;
    std::vector<double> b(lay_.m);
    std::vector<int32_t> basis(lay_.m);
    hipError_t e = d_b_.download(b, enqueue_only(stream_));
    HIP_TRY(first_error(e, d_basis_.download(basis, stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_set_cost: a kernel launch failed");
    return edit_rec([&](PivotRecord& r) { r.minus_objective = -objective_of(basis, b); });
}

relp_status_t Engine::get_cost(double* out_n) {
    const relp_status_t st = dual_ready("relp_get_cost");
    if (st) return st;
    std::copy(lay_.cost.begin(), lay_.cost.begin() + lay_.nr_normal, out_n);
    return RELP_OK;
}

relp_status_t Engine::cost_stats(int64_t* out4) const { return in_place_stats(out4, cost_changes_, cost_rows_, cost_last_p_, cost_last_splits_); }

// Room for `cut_room` cut rows with their slack columns and for `col_room` added columns in every buffer of the tableau path that
// create() sizes from the rows or the columns: the only function that grows the tableau engine, for both kinds of room (they are
// independent; neither ever shrinks).  The new pitches are the roundings of create() applied to the room.
// Every new buffer is allocated (zeroed: the kernels' 16-byte loads read the tails) before an old one is released, so a refused
// allocation leaves the handle as it was; then the contents move, 2-D where the pitch changes, and once every copy has succeeded
// the buffers are exchanged: old and new T0 live side by side for that moment.  A pending update block survives unchanged (same p, same bits); lay_, n_store_,
// n_alloc_ and the host mirrors are not touched (they follow at the add).
relp_status_t Engine::grow_tableau(int32_t cut_room, int32_t col_room) {
    cut_room = std::max(cut_room, cut_room_); col_room = std::max(col_room, col_room_);
    if (cut_room == cut_room_ && col_room == col_room_) return RELP_OK;
    tab_settle();
    HIP_TRY(hipStreamSynchronize(stream_));
    const int32_t room = cut_room;
    const int32_t m_now = lay_.m, n_now = n_store_;
    const int64_t m_cap = (int64_t)m_now - lay_.nr_cuts + room;
    const int64_t n_cap = (int64_t)n_now - lay_.nr_cuts + room - lay_.nr_added + col_room;
    const int64_t v_cap = (int64_t)lay_.nr_virtual - lay_.nr_cuts + room - lay_.nr_added + col_room;
    if (m_cap > INT32_MAX - 16 || n_cap > INT32_MAX - 16) return fail(RELP_E_ARG, "relp_reserve_cuts / relp_reserve_columns: more rows or columns than an index holds");
    // The pitches and sizes never shrink: after row removal at the phase switch (remove_rows lowers lay_.m and lay_.mc and leaves
    // every buffer as create() sized it) the rounding of the room can be below what is there.
    const int64_t ld_b = std::max(ld_b_, round_up(m_cap, 16)), ld_t = std::max(ld_t_, round_up(m_cap, 2));
    const int64_t ld_r = std::max(ld_r_, round_up(std::max<int64_t>(n_cap, 1), 2));
    const int64_t ld_a = std::max(ld_a_, round_up(std::max<int64_t>((int64_t)lay_.mc + room, 1), 2));
    const int64_t ld_c = std::max(ld_c_, round_up(m_cap, 2));

    // per buffer: copy old -> new, and exchange them; the closures own the new buffers.  The exchanges run only after every copy
    // has succeeded: a refused copy leaves the handle as it was, like a refused allocation.
    std::vector<std::function<hipError_t()>> copies;
    std::vector<std::function<void()>> exchanges;
    bool refused = false;
    // `columns` runs of `width` elements, old_ld apart in buf and new_ld apart in its replacement of at least `count` elements
    auto regrow = [&](auto& buf, int64_t count, int64_t width, int64_t columns, int64_t old_ld, int64_t new_ld, int fill, bool create = false) {
        using Buf = std::decay_t<decltype(buf)>;
        if (refused || (!buf && !create)) return;      // (a buffer this engine's configuration does not have)
        count = std::max(count, buf.count());
        auto fresh = std::make_shared<Buf>();
        hipError_t e = fresh->alloc(count);
        if (e == hipSuccess && fill) e = fresh->fill_bytes(fill, count, stream_);
        if (e != hipSuccess) { refused = true; return; }
        Buf* old = &buf;
        hipStream_t s = stream_;
        copies.push_back([=]() { return fresh->copy_2d(kFromDevice, *old, old_ld, width, columns, new_ld, s); });
        exchanges.push_back([=]() { old->swap(*fresh); });
    };
    auto regrow_1d = [&](auto& buf, int64_t count, int64_t keep, int fill = 0) { regrow(buf, count, keep, 1, keep, keep, fill); };

    // What only the rows size -- the m-sized and ld_b_-sized vectors, W and A -- moves only when the room for cut rows grows: room
    // for columns alone leaves them, and an adopted caller matrix stays adopted (no owned copy of A for a reserve of columns).
    const bool rows_grow = cut_room != cut_room_;
    if (rows_grow) {
        // m-sized
        regrow_1d(d_basis_, m_cap, m_now);
        regrow_1d(d_basis_alt_, m_cap, m_now);
        regrow_1d(d_idcol_, m_cap, m_now);
        regrow_1d(d_pos_of_row_, m_cap, m_now, 0xFF);      // -1 in the new part
        regrow_1d(d_rmin_, m_cap / 8 + 2, d_rmin_.count());
        regrow_1d(d_rhs_cols_, m_cap, 0);
        regrow_1d(d_rhs_delta_, m_cap, 0);
        {
            const int64_t basic_most = std::min<int64_t>(m_cap, lay_.nr_normal);
            regrow_1d(d_cost_rows_, basic_most, 0);
            regrow_1d(d_cost_delta_, basic_most, 0);
        }
        // ld_b_-sized
        for (DeviceBuf<double>* v : {&d_b_, &d_b_alt_, &d_alpha_, &d_aq_, &d_rho_, &d_w_, &d_v_, &d_minus_pi_}) regrow_1d(*v, ld_b, ld_b_);
        regrow(d_W_, ld_b * block_, ld_b_, block_, ld_b_, ld_b, 0);
        // A with room for the cut rows behind the constraints (an adopted caller matrix gets an owned copy and stays as it is)
        regrow(dA_, ld_a * std::max(lay_.nr_normal, 1), lay_.mc + lay_.nr_cuts, lay_.nr_normal, ld_a_, ld_a, 0);
    }
    // pitched
    regrow(dT0_, ld_t * std::max<int64_t>(n_cap, 1), ld_t_, n_now, ld_t_, ld_t, 0);
    regrow(dR0_, ld_r * (block_ + 1), ld_r_, block_ + 1, ld_r_, ld_r, 0);
    regrow(d_R0c_, ld_r * block_, ld_r_, block_, ld_r_, ld_r, 0);
    // per stored or tableau column
    regrow_1d(d_d_, n_cap, n_now);
    regrow_1d(d_in_basis_, n_cap, d_in_basis_.count());
    regrow_1d(d_cost_store_, n_cap, n_now);
    regrow_1d(d_fcols_, n_cap, d_fcols_.count());
    regrow_1d(d_fmask_, (n_cap + 63) / 64, d_fmask_.count());
    {
        const int64_t slots = price_structural_blocks(lay_.col_lo, lay_.col_hi) + (tab_na_ + v_cap + 255) / 256 + 8 + tab_scan_blocks((int32_t)n_cap) +
                              price_csc_blocks(0, lay_.nr_normal);
        regrow_1d(d_part_k1_, std::max(slots, d_part_k1_.count()), d_part_k1_.count());
        regrow_1d(d_part_j_, std::max(slots, d_part_j_.count()), d_part_j_.count());
    }
    regrow_1d(d_vrow0_, v_cap, lay_.nr_virtual);
    regrow_1d(d_vrow1_, v_cap, lay_.nr_virtual);
    regrow_1d(d_vsign_, v_cap, lay_.nr_virtual);
    // the added columns in row space (allocated with the first room for columns): the pitch follows the row capacity
    if (col_room > 0) regrow(d_col_a_, ld_c * col_room, std::min<int64_t>(m_now, ld_c_), lay_.nr_added, std::max<int64_t>(ld_c_, 1), ld_c, 0, true);
    if (refused) { (void)hipGetLastError(); return fail(RELP_E_ALLOC, "growing the tableau for cut rows or columns: out of device memory"); }

    hipError_t e = hipSuccess;
    for (auto& copy : copies) e = first_error(e, copy());
    HIP_TRY(e);                                        // (nothing exchanged: the new buffers go, the handle is as it was)
    for (auto& exchange : exchanges) exchange();
    copies.clear(); exchanges.clear();                 // releases the old buffers
    ld_b_ = ld_b; ld_t_ = ld_t; ld_r_ = ld_r; ld_a_ = ld_a; ld_c_ = ld_c;
    cut_room_ = cut_room; col_room_ = col_room;
    return RELP_OK;
}

relp_status_t Engine::reserve_cuts(int32_t rows) {
    relp_status_t st = dual_ready("relp_reserve_cuts");
    if (st) return st;
    if ((st = in_trial("relp_reserve_cuts"))) return st;
    if (rows < 0) return fail(RELP_E_ARG, "relp_reserve_cuts: rows < 0");
    return grow_for_cuts(rows);
}

// Cut rows added on the current basis without a flush or a re-tabulation.  The slack of cut k is basic in its new row, so the row
// in the current basis is g_k - sum_r g_k,B(r) T[r, :] over the rows r whose basic column is structural with a nonzero coefficient,
// T = T0 + W R0 over the pending rows of the open block (launch_tab_add_cuts), and b_new = beta_k - sum_r g_k,B(r) b_r.  The slack
// costs 0: d over the old columns, -obj, b and the basis entries of the old rows, W, R0 and T0 over the old rows and columns stay
// as they are.  The coefficients go into the engine's copy of A (rows mc + cut) and into lay_ (the host LU), so every later rebuild
// includes the cuts.
relp_status_t Engine::add_cuts(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs) {
    relp_status_t st = dual_ready("relp_add_cuts");
    if (st) return st;
    if ((st = lay_.check_cuts(count, row_ptr, col_idx, values, rhs, &err_))) return st;
    if (count == 0) return RELP_OK;
    if ((st = room_for_cuts("relp_add_cuts", count))) return st;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    const int32_t m_old = lay_.m, cuts_old = lay_.nr_cuts;
    std::vector<double> b(m_old);
    std::vector<int32_t> basis(m_old);
    hipError_t e = d_b_.download(b, enqueue_only(stream_));
    HIP_TRY(first_error(e, d_basis_.download(basis, stream_)));

    // the cuts as a dense block over the structural columns: column sp holds its `count` coefficients contiguously (the cut rows of A)
    std::vector<double> G((size_t)count * std::max(lay_.nr_normal, 1), 0.0);
    for (int32_t k = 0; k < count; ++k)
        for (int64_t x = row_ptr[k]; x < row_ptr[k + 1]; ++x) G[(size_t)col_idx[x] * count + k] = values[x];
    // the union list: rows, ascending, whose basic column is structural with a nonzero coefficient in some cut; coef[entry][cut]
    std::vector<int32_t> rows;
    std::vector<double> coef;
    for (int32_t i = 0; i < m_old; ++i) {
        const int32_t j = basis[i];
        if (j < 0 || j >= lay_.nr_normal) continue;
        const double* g = &G[(size_t)j * count];
        if (std::all_of(g, g + count, [](double v) { return v == 0.0; })) continue;
        rows.push_back(i);
        coef.insert(coef.end(), g, g + count);
    }
    const int32_t entries = (int32_t)rows.size();
    // b of the new rows: beta_k - sum_r g_k,B(r) b_r with fma in ascending r
    std::vector<double> b_new(count);
    for (int32_t k = 0; k < count; ++k) {
        double acc = 0.0;
        for (int32_t x = 0; x < entries; ++x) acc = std::fma(coef[(size_t)x * count + k], b[rows[x]], acc);
        b_new[k] = rhs[k] - acc;
    }
    HIP_TRY(d_cut_rows_.ensure(std::max(entries, 1), std::min<int64_t>(lay_.m, lay_.nr_normal)));
    HIP_TRY(d_cut_coef_.ensure(std::max<int64_t>((int64_t)entries * count, 1)));
    HIP_TRY(d_cut_u_.ensure((int64_t)count * std::max(block_, 1)));
    HIP_TRY(d_cut_g_.ensure((int64_t)G.size()));

    const TableauView tv = tview();                    // the tableau before the add
    CutRows cr{d_cut_rows_, d_cut_coef_, entries, count, A_base(), ld_a_, lay_.mc + cuts_old, tab_na_, lay_.nr_normal};
    CutTail ct{d_cost_store_, d_in_basis_, d_idcol_, d_basis_, d_vrow0_, d_vrow1_, d_vsign_, lay_.nr_virtual, block_ + 1};
    // the list, the cut rows of A and b of the new rows under one wait (no return before it: the host arrays are in flight; no
    // launch on a lost list)
    e = d_cut_rows_.upload(rows, enqueue_only(stream_));
    e = first_error(e, d_cut_coef_.upload(coef, enqueue_only(stream_)));
    // (G goes up in one piece and is spread over the columns of A on the device: a strided copy from host memory is a transfer per
    // column)
    e = first_error(e, d_cut_g_.upload(G, enqueue_only(stream_)));
    e = first_error(e, dA_.copy_2d(kFromDevice, d_cut_g_, count, count, lay_.nr_normal, ld_a_, enqueue_only(stream_), lay_.mc + cuts_old));
    e = first_error(e, d_b_.upload(b_new.data(), count, enqueue_only(stream_), m_old));
    if (e == hipSuccess) launch_tab_add_cuts(tv, deferred(), cr, d_in_basis_, p, d_cut_u_, ct, stream_);
    HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_add_cuts: a kernel launch failed");
    return cuts_added(count, row_ptr, col_idx, values, rhs, entries, p);
}

// room for `count` more cut rows: grown to max(cuts then in the tableau, 2 x the room so far, 16) when it lacks; inside a trial the
// reserved room is all there is
relp_status_t Engine::room_for_cuts(const char* what, int32_t count) {
    if ((int64_t)lay_.nr_cuts + count <= cut_room_) return RELP_OK;
    if (const relp_status_t st = in_trial((std::string(what) + " beyond the reserved room").c_str())) return st;
    const int64_t want = std::max<int64_t>({(int64_t)lay_.nr_cuts + count, 2 * (int64_t)cut_room_, 16});
    if (want > INT32_MAX / 2) return fail(RELP_E_ARG, std::string(what) + ": too many cuts");
    return grow_for_cuts((int32_t)want);
}

// the layout and the host mirrors follow the device (check_cuts passed: Layout::add_cuts cannot fail), the record is re-armed
relp_status_t Engine::cuts_added(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs,
                                 int32_t entries, int32_t p) {
    const int32_t n_old = n_store_;
    (void)lay_.add_cuts(count, row_ptr, col_idx, values, rhs, &err_);
    for (int32_t k = 0; k < count; ++k) idcol_h_.push_back(n_old + k);
    cost_store_h_.resize((size_t)n_old + count, 0.0);
    n_store_ += count; n_alloc_ += count; lay_.sc_hi += count;
    tab_partials_valid_ = false;
    cut_last_rows_ = entries;
    cut_last_p_ = p;
    h_rec_->outcome = DEV_RUNNING;
    return upload_rec();
}

relp_status_t Engine::cut_stats(int64_t* out4) const { return in_place_stats(out4, lay_.nr_cuts, cut_room_, cut_last_rows_, cut_last_p_); }

relp_status_t Engine::reserve_columns(int32_t columns) {
    relp_status_t st = dual_ready("relp_reserve_columns");
    if (st) return st;
    if ((st = in_trial("relp_reserve_columns"))) return st;
    if (columns < 0) return fail(RELP_E_ARG, "relp_reserve_columns: columns < 0");
    return grow_tableau(cut_room_, columns);
}

// Columns from outside added on the current basis without a flush or a re-tabulation: the mirror image of add_cuts.  B^-1 is in the
// tableau -- the stored columns that were the identity at the start -- in the form (I + W S') T0 like every other column, and that
// form is linear in T0: T0[:, new] = sum_i a_i T0[:, idcol[i]] over the rows i with a nonzero coefficient, ascending, and the new
// entries of R0 are the new T0 entries at the pending rows (launch_tab_add_columns; W is not read).  d_new = c + sum_i (-pi)_i a_i
// with -pi as relp_get_minus_pi reads it off d, an fma chain from c in ascending i, formed here.  The new variable is non-basic:
// b, -obj, the basis and everything over the old columns stay as they are.  The entries go into lay_ (the host LU) and into
// d_col_a_ (the re-tabulation), so every later rebuild includes the columns.
relp_status_t Engine::add_columns(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost) {
    relp_status_t st = dual_ready("relp_add_columns");
    if (st) return st;
    if ((st = in_trial("relp_add_columns"))) return st;
    if (count > kTabColTile * 65535) return fail(RELP_E_ARG, "relp_add_columns: more than 524,280 columns in one call");       // (the grid's second dimension)
    if ((st = lay_.check_columns(count, col_ptr, row_idx, values, cost, &err_))) return st;
    if (count == 0) return RELP_OK;
    if ((st = room_for_columns("relp_add_columns", count))) return st;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    const int32_t m = lay_.m, n_old = n_store_, added_old = lay_.nr_added;
    std::vector<double> d(n_old);
    HIP_TRY(d_d_.download(d, stream_));

    // the columns as a dense block in row space (explicit zeros dropped: they stay 0.0), and the union list: rows, ascending, with
    // a nonzero coefficient in some column of the call, as their identity columns; coef[entry][column]
    std::vector<double> dense((size_t)count * m, 0.0);
    std::vector<uint8_t> touched(m, 0);
    for (int32_t k = 0; k < count; ++k)
        for (int64_t x = col_ptr[k]; x < col_ptr[k + 1]; ++x)
            if (values[x] != 0.0) { dense[(size_t)k * m + row_idx[x]] = values[x]; touched[row_idx[x]] = 1; }
    std::vector<int32_t> cols;
    std::vector<double> coef;
    std::vector<double> d_new(cost, cost + count);
    for (int32_t i = 0; i < m; ++i) {
        if (!touched[i]) continue;
        cols.push_back(idcol_h_[i]);
        const double minus_pi = d[idcol_h_[i]] - cost_store_h_[idcol_h_[i]];      // as get_vector forms it
        for (int32_t k = 0; k < count; ++k) {
            const double a = dense[(size_t)k * m + i];
            coef.push_back(a);
            if (a != 0.0) d_new[k] = std::fma(minus_pi, a, d_new[k]);
        }
    }
    const int32_t entries = (int32_t)cols.size();
    HIP_TRY(d_col_cols_.ensure(std::max(entries, 1), lay_.m));
    HIP_TRY(d_col_coef_.ensure(std::max<int64_t>((int64_t)entries * count, 1)));
    HIP_TRY(d_col_d_.ensure(count, 16));
    HIP_TRY(d_col_cost_.ensure(count, 16));

    const TableauView tv = tview();                    // the tableau before the add
    const ColumnAdd ca{d_col_cols_, d_col_coef_, entries, count, d_col_d_, d_col_cost_};
    const ColumnTail ct{d_cost_store_, d_in_basis_, d_vrow0_, d_vrow1_, d_vsign_, lay_.nr_virtual, block_ + 1};
    // the list, d and cost of the new columns and their rows of d_col_a_ under one wait (no return before it: the host arrays are
    // in flight; no launch on a lost list)
    hipError_t e = d_col_cols_.upload(cols, enqueue_only(stream_));
    e = first_error(e, d_col_coef_.upload(coef, enqueue_only(stream_)));
    e = first_error(e, d_col_d_.upload(d_new, enqueue_only(stream_)));
    e = first_error(e, d_col_cost_.upload(cost, count, enqueue_only(stream_)));
    e = first_error(e, d_col_a_.copy_2d(kFromHost, dense.data(), m, m, count, ld_c_, enqueue_only(stream_), (int64_t)added_old * ld_c_));
    if (e == hipSuccess) launch_tab_add_columns(tv, deferred(), ca, p, ct, stream_);
    HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_add_columns: a kernel launch failed");
    return columns_added(count, col_ptr, row_idx, values, cost, entries, p);
}

// room for `count` more added columns: grown to max(added columns then in the tableau, 2 x the room so far, 16) when it lacks
relp_status_t Engine::room_for_columns(const char* what, int32_t count) {
    if ((int64_t)lay_.nr_added + count <= col_room_) return RELP_OK;
    const int64_t want = std::max<int64_t>({(int64_t)lay_.nr_added + count, 2 * (int64_t)col_room_, 16});
    if (want > INT32_MAX / 2) return fail(RELP_E_ARG, std::string(what) + ": too many columns");
    return grow_tableau(cut_room_, (int32_t)want);
}

// the layout and the host mirrors follow the device (check_columns passed: Layout::add_columns cannot fail), the record is re-armed
relp_status_t Engine::columns_added(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost,
                                    int32_t entries, int32_t p) {
    const int32_t n_old = n_store_;
    (void)lay_.add_columns(count, col_ptr, row_idx, values, cost, &err_);
    cost_store_h_.resize((size_t)n_old + count);
    std::copy(cost, cost + count, cost_store_h_.begin() + n_old);
    n_store_ += count; n_alloc_ += count; lay_.sc_hi += count;
    tab_partials_valid_ = false;
    col_last_cols_ = entries;
    col_last_p_ = p;
    h_rec_->outcome = DEV_RUNNING;
    return upload_rec();
}

relp_status_t Engine::column_stats(int64_t* out4) const { return in_place_stats(out4, lay_.nr_added, col_room_, col_last_cols_, col_last_p_); }

// Cut rows and added columns taken back: exact deletions, no arithmetic.  A cut whose slack is basic takes with it the tableau row
// the slack is basic in (basis position r, not necessarily the cut's own row i) and the slack's column: in the basis without them
// every other entry of the tableau keeps its value, because column s is e_r and no other basic column has an entry in row r.  A
// non-basic column is simply gone.  What moves: everything indexed by constraint loses i, everything indexed by basis position
// loses r, everything indexed by stored column loses s; survivors close up in order (launch_tab_compact for the images, the host
// for the small vectors: copies, nothing is recomputed).  The callers have validated, settled and flushed: p = 0, T = T0.
//   rows_t / rows_c: the basis positions and the constraints that go (ascending each, the same number); cols_p: the provider columns
//   that go (ascending); basis: the downloaded basis.
relp_status_t Engine::compact_tableau(const std::vector<int32_t>& rows_t, const std::vector<int32_t>& rows_c, const std::vector<int32_t>& cols_p,
                                      const std::vector<int32_t>& basis) {
    const int32_t m_old = lay_.m, n_old = n_store_, nr = (int32_t)rows_t.size(), nc = (int32_t)cols_p.size();
    const int32_t m_new = m_old - nr, n_new = n_old - nc, cuts_old = lay_.nr_cuts, added_old = lay_.nr_added;
    // the lists, one upload: [basis positions | constraints | stored columns | cut rows of A | added columns]
    std::vector<int32_t> lists;
    lists.insert(lists.end(), rows_t.begin(), rows_t.end());
    lists.insert(lists.end(), rows_c.begin(), rows_c.end());
    for (int32_t p : cols_p) lists.push_back(tab_na_ + p);
    for (int32_t i : rows_c) lists.push_back(lay_.mc + (i - lay_.cut_row0));
    int32_t na = 0;
    for (int32_t p : cols_p)
        if (lay_.added_of(p) >= 0) { lists.push_back(lay_.added_of(p)); ++na; }
    HIP_TRY(d_rm_lists_.ensure((int64_t)lists.size(), 256));
    const int32_t* l_rows_t = d_rm_lists_;
    const int32_t* l_rows_c = l_rows_t + nr;
    const int32_t* l_cols_s = l_rows_c + nr;
    const int32_t* l_rows_a = l_cols_s + nc;
    const int32_t* l_cols_a = l_rows_a + nr;

    // the small vectors on the host: d, b, the flags (by tableau column), the stored costs, idcol, the basis
    std::vector<double> b(m_old), d(n_old);
    std::vector<uint8_t> flags(n_old - tab_na_);
    hipError_t e = d_b_.download(b, enqueue_only(stream_));
    e = first_error(e, d_d_.download(d, enqueue_only(stream_)));
    HIP_TRY(first_error(e, d_in_basis_.download(flags, stream_)));
    std::vector<int32_t> col_map(n_old - tab_na_ + 1, 0);          // provider column -> its new index (a removed one: its successor's)
    {
        size_t f = 0;
        for (int32_t p = 0, out = 0; p <= n_old - tab_na_; ++p) {
            col_map[p] = out;
            if (f < cols_p.size() && cols_p[f] == p) ++f; else ++out;
        }
    }
    auto drop = [](auto& v, const std::vector<int32_t>& gone, int32_t offset) {      // v without the entries gone[k] + offset, padded with zeros
        size_t f = 0, o = 0;
        for (size_t x = 0; x < v.size(); ++x) {
            if (f < gone.size() && (size_t)(gone[f] + offset) == x) { ++f; continue; }
            v[o++] = v[x];
        }
        std::fill(v.begin() + o, v.end(), 0);
    };
    std::vector<int32_t> basis_new(basis);
    drop(b, rows_t, 0); drop(basis_new, rows_t, 0);
    for (int32_t r = 0; r < m_new; ++r)
        if (basis_new[r] >= 0 && basis_new[r] < n_old - tab_na_) basis_new[r] = col_map[basis_new[r]];      // (a wrapped artificial keeps its index)
    drop(d, cols_p, tab_na_); drop(cost_store_h_, cols_p, tab_na_); drop(flags, cols_p, 0);
    drop(idcol_h_, rows_c, 0);
    for (int32_t i = 0; i < m_new; ++i)
        if (idcol_h_[i] >= tab_na_) idcol_h_[i] = tab_na_ + col_map[idcol_h_[i] - tab_na_];

    // everything under one wait (no return before it: the host arrays are in flight).  The host mirrors above are already those of
    // the smaller tableau: a HIP error from here on leaves the handle unusable, like a failed launch of a pivot
    e = d_rm_lists_.upload(lists, enqueue_only(stream_));
    if (e == hipSuccess) {
        launch_tab_compact(dT0_, ld_t_, m_old, n_old, l_rows_t, nr, l_cols_s, nc, 0, stream_);
        launch_tab_compact(d_W_, ld_b_, m_old, block_, l_rows_t, nr, nullptr, 0, 0, stream_);
        // R0 and its compacted copy hold a stored column per "row" of their images
        launch_tab_compact(dR0_, ld_r_, n_old, block_ + 1, l_cols_s, nc, nullptr, 0, 0, stream_);
        if (d_R0c_) launch_tab_compact(d_R0c_, ld_r_, n_old, block_, l_cols_s, nc, nullptr, 0, 0, stream_);
        // the cut rows of the device matrix (an owned copy since the first room for cuts) and the added columns in row space
        if (nr > 0 && dA_.owned()) launch_tab_compact(dA_, ld_a_, lay_.mc + cuts_old, lay_.nr_normal, l_rows_a, nr, nullptr, 0, 0, stream_);
        if (added_old > 0) launch_tab_compact(d_col_a_, ld_c_, m_old, added_old, l_rows_c, nr, l_cols_a, na, 0, stream_);
    }
    e = first_error(e, d_b_.upload(b, enqueue_only(stream_)));
    e = first_error(e, d_basis_.upload(basis_new, enqueue_only(stream_)));
    e = first_error(e, d_d_.upload(d, enqueue_only(stream_)));
    e = first_error(e, d_cost_store_.upload(cost_store_h_, enqueue_only(stream_)));
    e = first_error(e, d_in_basis_.upload(flags, enqueue_only(stream_)));
    e = first_error(e, d_idcol_.upload(idcol_h_, enqueue_only(stream_)));
    e = first_error(e, d_pos_of_row_.fill_bytes(0xFF, m_old, enqueue_only(stream_)));              // (the flush left no pending row)
    // the tails of the other m-vectors are zero for the 16-byte loads
    for (DeviceBuf<double>* v : {&d_alpha_, &d_aq_, &d_rho_, &d_minus_pi_, &d_w_, &d_v_, &d_b_alt_})
        if (*v && nr > 0) e = first_error(e, fill_bytes_at(*v + m_new, 0, sizeof(double) * (size_t)nr, enqueue_only(stream_)));
    HIP_TRY(first_error(e, hipStreamSynchronize(stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "removing rows or columns of the tableau: a kernel launch failed");
    idcol_h_.resize(m_new); cost_store_h_.resize(n_new);
    for (int32_t& j : barred_) j = (j >= 0 && j < n_old - tab_na_) ? col_map[j] : j;
    n_store_ = n_new; n_alloc_ -= nc; lay_.sc_hi -= nc;
    tab_partials_valid_ = false;
    rm_last_moved_ = (nr > 0 ? (int64_t)(m_old - rows_t.front()) * n_old : 0) +
                     (nc > 0 ? (int64_t)m_new * (n_old - (tab_na_ + cols_p.front())) : 0);
    return RELP_OK;
}

// The shared front of the two removals: the flush of the open block exactly as relp_flush does it (a removed row that is pending
// would leave R0 = S' T0 without its row), p of that block for the stats.
relp_status_t Engine::flush_for_removal() {
    const relp_status_t st = settled_pending(&rm_last_p_);
    return st ? st : flush();
}

relp_status_t Engine::remove_cuts(const int32_t* rows, int32_t count) {
    relp_status_t st = dual_ready("relp_remove_cuts");
    if (st) return st;
    if ((st = in_trial("relp_remove_cuts"))) return st;
    if (count < 0 || (count > 0 && !rows)) return lay_.check_remove_cuts(rows, count, {}, &err_);
    if (count == 0) return RELP_OK;
    tab_settle();
    std::vector<int32_t> basis(lay_.m);
    HIP_TRY(d_basis_.download(basis, stream_));
    if ((st = lay_.check_remove_cuts(rows, count, basis, &err_))) return st;
    if ((st = flush_for_removal())) return st;

    const std::vector<int32_t> slack = lay_.cut_slacks();
    std::vector<int32_t> row_of(lay_.n_provider, -1);              // provider column -> its basis position
    for (int32_t r = 0; r < lay_.m; ++r)
        if (basis[r] >= 0 && basis[r] < lay_.n_provider) row_of[basis[r]] = r;
    std::vector<int32_t> rows_t, rows_c(rows, rows + count), cols_p;
    for (int32_t i : rows_c) {
        const int32_t s = lay_.nr_normal + slack[i - lay_.cut_row0];
        cols_p.push_back(s);
        rows_t.push_back(row_of[s]);
    }
    std::sort(rows_t.begin(), rows_t.end()); std::sort(rows_c.begin(), rows_c.end()); std::sort(cols_p.begin(), cols_p.end());
    if ((st = compact_tableau(rows_t, rows_c, cols_p, basis))) return st;
    // the layout follows (check_remove_cuts passed: remove_cuts cannot fail), then its tables on the device
    (void)lay_.remove_cuts(rows, count, basis, &err_);
    rm_cuts_ += count;
    pools_mark_stale(rows, count);                     // (relp_pool.hpp: a row below a pool's bound went)
    return finish_removal();
}

relp_status_t Engine::remove_columns(const int32_t* columns, int32_t count) {
    relp_status_t st = dual_ready("relp_remove_columns");
    if (st) return st;
    if ((st = in_trial("relp_remove_columns"))) return st;
    if (count < 0 || (count > 0 && !columns)) return lay_.check_remove_columns(columns, count, {}, &err_);
    if (count == 0) return RELP_OK;
    tab_settle();
    std::vector<int32_t> basis(lay_.m);
    HIP_TRY(d_basis_.download(basis, stream_));
    if ((st = lay_.check_remove_columns(columns, count, basis, &err_))) return st;
    if ((st = flush_for_removal())) return st;
    std::vector<int32_t> cols_p(columns, columns + count);
    std::sort(cols_p.begin(), cols_p.end());
    if ((st = compact_tableau({}, {}, cols_p, basis))) return st;
    (void)lay_.remove_columns(columns, count, basis, &err_);
    rm_columns_ += count;
    return finish_removal();
}

// the descriptors of the virtual columns as the layout has them now, and the record re-armed (a remembered column moves with the
// columns; the trace keeps the indices of its time)
relp_status_t Engine::finish_removal() {
    hipError_t e = d_vrow0_.upload(lay_.vrow0.data(), lay_.nr_virtual, enqueue_only(stream_));
    e = first_error(e, d_vrow1_.upload(lay_.vrow1.data(), lay_.nr_virtual, enqueue_only(stream_)));
    HIP_TRY(first_error(e, d_vsign_.upload(lay_.vsign.data(), lay_.nr_virtual, stream_)));
    return edit_rec([&](PivotRecord& r) { if (r.last_selected >= nr_columns()) r.last_selected = -1; });
}

relp_status_t Engine::removal_stats(int64_t* out4) const { return in_place_stats(out4, rm_cuts_, rm_columns_, rm_last_moved_, rm_last_p_); }

// The two batched ratio queries.  Both read the tableau as it stands -- T0, and W R0 over the p pending rows of an open block -- and
// write to scratch of their own: d, b, the basis, the flags, W, R0, T0, the PRICE partials and the record stay as they are (the
// record is downloaded for p, never uploaded).  Settles the fused update's shadow row first, does not flush.
// columns == false: rows of T against d (launch_tab_row_ratios); true: the rows' identity columns against b (launch_tab_rhs_ranging).
relp_status_t Engine::ranging_query(bool columns, const char* what, const int32_t* rows, int32_t count, double* ratio0, int32_t* index0,
                                    double* ratio1, int32_t* index1) {
    relp_status_t st = dual_ready(what);
    if (st) return st;
    if (count < 0 || (count > 0 && !rows)) return fail(RELP_E_ARG, std::string(what) + ": count < 0 or the list missing");
    for (int32_t k = 0; k < count; ++k)
        if (rows[k] < 0 || rows[k] >= lay_.m) return fail(RELP_E_ARG, std::string(what) + ": row out of range");
    if (count == 0) return RELP_OK;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    const TableauView tv = tview();
    const int64_t blocks = columns ? (lay_.m + 255) / 256 : tab_scan_blocks(lay_.sc_hi - lay_.sc_lo);
    HIP_TRY(d_rng_list_.ensure_raw(sizeof(int32_t) * (size_t)count));
    HIP_TRY(d_rng_ratio_.ensure_raw(sizeof(double) * 2 * (size_t)count));
    HIP_TRY(d_rng_index_.ensure_raw(sizeof(int32_t) * 2 * (size_t)count));
    HIP_TRY(d_rng_part_k_.ensure_raw(sizeof(double) * (size_t)(2 * count * blocks)));
    HIP_TRY(d_rng_part_j_.ensure_raw(sizeof(int32_t) * (size_t)(2 * count * blocks)));
    std::vector<int32_t> list(rows, rows + count);
    if (columns) for (int32_t& r : list) r = idcol_h_[r];
    // the list, the ratios and the indices under one wait (no return before it: list, ratio are in flight; no launch on a lost list)
    hipError_t e = d_rng_list_.upload(list, enqueue_only(stream_));
    if (e == hipSuccess && columns) launch_tab_rhs_ranging(tv, deferred(), d_b_, d_basis_, tolerances(), d_rng_list_, count, p, d_rng_part_k_,
                                                           d_rng_ratio_, d_rng_index_, stream_);
    else if (e == hipSuccess) launch_tab_row_ratios(tv, deferred(), tab_partials(current_rule()), tolerances(), d_rng_list_, count, p,
                                                    d_rng_part_k_, d_rng_part_j_, d_rng_ratio_, d_rng_index_, stream_);
    std::vector<double> ratio(2 * (size_t)count);          // (allocated while the kernel runs)
    std::vector<int32_t> index(2 * (size_t)count);
    e = first_error(e, d_rng_ratio_.download(ratio, enqueue_only(stream_)));
    HIP_TRY(first_error(e, d_rng_index_.download(index, stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, std::string(what) + ": a kernel launch failed");
    if (ratio0) std::copy(ratio.begin(), ratio.begin() + count, ratio0);
    if (index0) std::copy(index.begin(), index.begin() + count, index0);
    if (ratio1) std::copy(ratio.begin() + count, ratio.end(), ratio1);
    if (index1) std::copy(index.begin() + count, index.end(), index1);
    if (columns) ++rng_ranging_calls_;
    else { ++rng_ratio_calls_; rng_ratio_rows_ += count; }
    rng_last_p_ = p;
    return RELP_OK;
}

relp_status_t Engine::row_ratios(const int32_t* rows, int32_t count, double* down_ratio, int32_t* down_column, double* up_ratio,
                                 int32_t* up_column) {
    return ranging_query(false, "relp_row_ratios", rows, count, down_ratio, down_column, up_ratio, up_column);
}

relp_status_t Engine::rhs_ranging(const int32_t* rows, int32_t count, double* decrease, int32_t* decrease_row, double* increase,
                                  int32_t* increase_row) {
    return ranging_query(true, "relp_rhs_ranging", rows, count, decrease, decrease_row, increase, increase_row);
}

relp_status_t Engine::ranging_stats(int64_t* out4) const { return in_place_stats(out4, rng_ratio_calls_, rng_ratio_rows_, rng_ranging_calls_, rng_last_p_); }

// Gomory cuts from the listed rows of the tableau as it stands, in structural space.  The steps of ranging_query: validate, settle
// the fused update's shadow row (no flush), upload the list, launch, one download.  Decided here from b and the basis (one
// download before the launch): f0 and the statuses 1 - 3 of every entry (gomory_entry); a skipped entry goes up with f0 = -1 and
// comes back all zero.  Decided on the device: pi over the stored columns, y over the rows through the virtual descriptors the
// layout uploaded (table()), g over the structural columns from the engine's A (cut rows behind the constraints) and bound_row,
// and the status 4 of a fractional cut.  beta is the fma chain of gomory_beta over the downloaded y and lay_.rhs.
relp_status_t Engine::gomory_cuts(const int32_t* rows, int32_t count, const uint8_t* is_integer, int32_t kind, double away,
                                  double* coefficients, double* rhs, double* fraction, int32_t* status) {
    relp_status_t st = dual_ready("relp_gomory_cuts");
    if (st) return st;
    if (lay_.nr_range > 0) return fail(RELP_E_UNSUPPORTED, "relp_gomory_cuts: range rows are not substituted out of a cut");
    if (lay_.nr_added > 0) return fail(RELP_E_STATE, "relp_gomory_cuts: added columns in the tableau (relp_add_cuts holds no coefficient on one)");
    if (const char* why = gomory_check_args(rows, count, lay_.m, kind, away, coefficients, rhs, status)) return fail(RELP_E_ARG, std::string("relp_gomory_cuts: ") + why);
    if (count == 0) return RELP_OK;
    int32_t p;
    if ((st = settled_pending(&p))) return st;
    const int32_t m = lay_.m, nn = lay_.nr_normal;
    std::vector<double> b(m);
    std::vector<int32_t> basis(m);
    hipError_t e = d_b_.download(b, enqueue_only(stream_));
    HIP_TRY(first_error(e, d_basis_.download(basis, stream_)));
    std::vector<double> f0(count), f0_dev(count);
    std::vector<int32_t> stat(count);
    for (int32_t k = 0; k < count; ++k) {
        stat[k] = gomory_entry(b[rows[k]], basis[rows[k]], is_integer, lay_.n_provider, away, &f0[k]);
        f0_dev[k] = stat[k] == kGomoryCut ? f0[k] : -1.0;
    }
    const TableauView tv = tview();
    const int64_t n_st = tv.c_hi - tv.c_lo, nbc = tab_scan_blocks((int32_t)n_st);
    const size_t n_g = (size_t)count * nn, n_y = (size_t)count * m, n_bad = (size_t)count * nbc, n_pi = (size_t)count * n_st;
    HIP_TRY(d_gom_rows_.ensure_raw(sizeof(int32_t) * (size_t)count));
    HIP_TRY(d_gom_f0_.ensure_raw(sizeof(double) * (size_t)count));
    HIP_TRY(d_gom_out_.ensure_raw(sizeof(double) * (n_g + n_y + n_bad + n_pi)));
    if (is_integer) HIP_TRY(d_gom_int_.ensure_raw((size_t)lay_.n_provider));
    GomoryCuts gc{d_gom_rows_, d_gom_f0_, is_integer ? (const uint8_t*)d_gom_int_ : nullptr, count, kind, A_base(), ld_a_, tab_na_, nn,
                  d_gom_out_ + n_g + n_y + n_bad, d_gom_out_ + n_g, d_gom_out_ + n_g + n_y, d_gom_out_};
    // the list and the results under one wait (no return before it: the host arrays are in flight; no launch on a lost list)
    e = d_gom_rows_.upload(rows, count, enqueue_only(stream_));
    e = first_error(e, d_gom_f0_.upload(f0_dev, enqueue_only(stream_)));
    if (is_integer) e = first_error(e, d_gom_int_.upload(is_integer, lay_.n_provider, enqueue_only(stream_)));
    if (e == hipSuccess) launch_tab_gomory(tv, deferred(), table(), d_in_basis_, tolerances(), gc, p, stream_);
    std::vector<double> out(n_g + n_y + n_bad);            // (allocated while the kernels run)
    HIP_TRY(first_error(e, d_gom_out_.download(out, stream_)));
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "relp_gomory_cuts: a kernel launch failed");
    int64_t made = 0;
    for (int32_t k = 0; k < count; ++k) {
        const double* bad = &out[n_g + n_y + (size_t)k * nbc];
        if (stat[k] == kGomoryCut && std::any_of(bad, bad + nbc, [](double v) { return v != 0.0; })) stat[k] = kGomoryContinuous;
        double* g = coefficients + (size_t)k * nn;
        if (stat[k] == kGomoryCut) {
            std::copy(&out[(size_t)k * nn], &out[(size_t)k * nn] + nn, g);
            rhs[k] = gomory_beta(f0[k], &out[n_g + (size_t)k * m], lay_.rhs.data(), m);
            ++made;
        } else {
            std::fill(g, g + nn, 0.0);
            rhs[k] = 0.0;
        }
        if (fraction) fraction[k] = f0[k];
        status[k] = stat[k];
    }
    ++gom_calls_; gom_entries_ += count; gom_cuts_ += made;
    gom_last_p_ = p;
    return RELP_OK;
}

relp_status_t Engine::gomory_stats(int64_t* out4) const { return in_place_stats(out4, gom_calls_, gom_entries_, gom_cuts_, gom_last_p_); }

// phase_one.rs:146-166: objective == 0 -> feasible (remove artificials, switch) else infeasible
relp_status_t Engine::finish_phase_one(int32_t* outcome) {
    tab_settle();
    const double obj = -h_rec_->minus_objective;
    if (std::fabs(obj) > cfg_.tol_feas * std::max(1.0, lay_.phase1_objective)) { *outcome = RELP_INFEASIBLE; return RELP_OK; }
    std::vector<int32_t> rows_to_remove;
    if (cfg_.shard_count == 1 || tableau_) enqueue_flush();        // the phase boundary works on the explicit inverse
    relp_status_t st = (cfg_.shard_count > 1 && tableau_) ? remove_artificial_basis_variables_sharded(rows_to_remove)
                                                          : remove_artificial_basis_variables(rows_to_remove);
    if (st) return st;
    if ((st = switch_to_phase_two(rows_to_remove))) return st;
    *outcome = RELP_PHASE_ONE_DONE;
    return RELP_OK;
}

// The head the two zero-level removers share: the basis on the host and the basic artificial variables, ascending.
relp_status_t Engine::basic_artificials(std::vector<int32_t>* basis, std::vector<int32_t>* arts) {
    basis->resize(lay_.m);
    HIP_TRY(d_basis_.download(*basis, stream_));
    arts->clear();
    for (int32_t v : *basis) if (v < lay_.nr_artificial) arts->push_back(v);
    std::sort(arts->begin(), arts->end());
    return RELP_OK;
}

// No eligible column: phase_one.rs:252 pushes the artificial's index; RELP_ARTIFICIAL_TEXTBOOK its own row, and remove_rows
// moves the artificial into that position first (relp_engine.h)
void Engine::keep_artificial_row(int32_t a, std::vector<int32_t>& rows_to_remove) {
    if (cfg_.artificial_removal == RELP_ARTIFICIAL_TEXTBOOK) { stuck_artificials_.push_back(a); rows_to_remove.push_back(lay_.column_to_row[a]); }
    else rows_to_remove.push_back(a);
}

// phase_one.rs:223-260 (pivots "at zero level"; pushes the artificial index like the reference)
relp_status_t Engine::remove_artificial_basis_variables(std::vector<int32_t>& rows_to_remove) {
    std::vector<int32_t> basis, arts;
    relp_status_t st = basic_artificials(&basis, &arts);
    if (st) return st;
    if (arts.empty()) return RELP_OK;
    const int n = nr_columns();
    std::vector<double> d(n), tau(n);
    std::vector<uint8_t> inb(n);
    const bool textbook = cfg_.artificial_removal == RELP_ARTIFICIAL_TEXTBOOK;
    for (int32_t a : arts) {
        int32_t pivot_row = lay_.column_to_row[a];             // phase_one.rs:236: the row the artificial STARTED in
        if (textbook) pivot_row = (int32_t)(std::find(basis.begin(), basis.end(), a) - basis.begin());   // the row it is basic in
        if ((st = relative_costs(d.data()))) return st;
        // tableau row pivot_row over every column: (row of B^-1) . a_j, no cost term
        if (tableau_) {
            launch_tab_row(tview(), deferred(), pivot_row, d_aq_big(), d_rec_, stream_);        // single GPU: all columns
        } else if (lu_) {
            lu_btran(pivot_row, nullptr, d_rho_);
            enqueue_price(0, d_rho_, nullptr, 0, lay_.nr_normal);
        } else {
            enqueue_price(0, Binv_base() + (int64_t)pivot_row * ld_b_, nullptr, lay_.col_lo, lay_.col_hi);
        }
        if (tableau_) HIP_TRY(download_from(tau, d_aq_big(), stream_));
        else HIP_TRY(d_d_.download(tau, stream_));
        HIP_TRY(d_in_basis_.download(inb, stream_));
        int32_t q = -1;
        for (int32_t j = lay_.nr_artificial; j < n; ++j) {
            if (inb[j]) continue;
            if (!textbook && std::fabs(d[j]) > cfg_.tol_cost) continue;        // phase_one.rs:241: cost.is_zero()
            if (std::fabs(tau[j]) > cfg_.tol_pivot) { q = j; break; }
        }
        if (q < 0) { keep_artificial_row(a, rows_to_remove); continue; }
        if ((st = generate_column(q, nullptr))) return st;
        if ((st = bring_into_basis(q, pivot_row, d[q], nullptr))) return st;
        basis[pivot_row] = q;
    }
    return RELP_OK;
}

// kind/non_artificial.rs:151-220, carry/mod.rs:484-510 (+ :650-689 when rows are removed)
relp_status_t Engine::switch_to_phase_two(const std::vector<int32_t>& rows_to_remove) {
    relp_status_t st;
    if (cfg_.shard_count == 1 || tableau_) enqueue_flush();     // zero-level pivots may have left updates pending
    if (!rows_to_remove.empty()) {
        std::vector<int32_t> rows(rows_to_remove);          // ascending and distinct: remove_rows walks the list beside the rows
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        st = remove_rows(rows);
        stuck_artificials_.clear();
        if (st) return st;
    }
    std::vector<int32_t> basis(lay_.m);
    HIP_TRY(d_basis_.download(basis, stream_));
    const int32_t na = lay_.nr_artificial;
    // An artificial variable can survive remove_artificial_basis_variables: when it re-entered the basis in
    // another row than its own, the zero-level pivot of phase_one.rs:236 is made in its ORIGINAL row.  In
    // the reference's release-built integration tests `basis_column -= nr_artificial` (carry/mod.rs:524, 663)
    // then wraps to a huge usize: a column without cost that sorts last in Bland's tie-break and stays basic
    // at value zero until the ratio test removes it (Netlib BOEING2 walks through this state).  Same here
    // with the wrapped index squeezed into int32, order preserved: INT32_MAX - (na - 1 - a).
    for (auto& v : basis) v = v < na ? INT32_MAX - (na - 1 - v) : v - na;
    lay_.wrapped_na = na;
    lay_.nr_artificial = 0;
    phase_ = 2;
    HIP_TRY(d_basis_.upload(basis, stream_));
    std::vector<uint8_t> flags(n_alloc_, 0);
    for (int32_t v : basis) {
        if (v >= kWrappedArtificialBase) continue;
        if (v < 0 || v >= lay_.n_provider) return fail(RELP_E_STATE, "basis column out of range at the phase switch");
        flags[v] = 1;
    }
    HIP_TRY(d_in_basis_.upload(flags, stream_));
    // -pi = -(c_B' B^-1) (create_minus_pi_from_artificial, carry/mod.rs:214-248), accumulated over rows in order
    std::vector<double> w = basic_costs(basis, 2, 1.0), b(lay_.m);
    if (cfg_.shard_count > 1 && !tableau_)
        for (double v : w) if (v != 0.0) return fail(RELP_E_UNSUPPORTED, "sharded phase switch needs an all-slack basis");
    if (lu_) for (auto& v : w) v = -v;                 // BTRAN with rhs -c_B gives -pi directly
    HIP_TRY(d_w_.upload(w.data(), lay_.m, stream_));
    if (lu_) {
        if (lu_status_) return take_lu_status();
        lu_btran(-1, d_w_, d_minus_pi_);
    } else if (tableau_) {
        // phase-2 reduced costs of every stored column: d = c - c_B' T (the artificial block keeps cost 0)
        cost_store_h_.assign(n_store_, 0.0);
        for (int32_t p = 0; p < lay_.nr_normal; ++p) cost_store_h_[tab_na_ + p] = lay_.cost[p];
        HIP_TRY(d_cost_store_.upload(cost_store_h_, stream_));
        launch_tab_price_init(tview(), d_w_, d_cost_store_, stream_);
        tab_partials_valid_ = false;
    } else {
        launch_weighted_column_sums(Binv_base(), ld_b_, lay_.m, d_w_, d_minus_pi_, stream_);
    }
    // -obj = -sum_i b_i c_B(i) (create_minus_obj_from_artificial, carry/mod.rs:258-271)
    HIP_TRY(d_b_.download(b, stream_));
    return edit_rec([&](PivotRecord& r) { r.minus_objective = -objective_of(basis, b); r.last_selected = -1; r.phase = 2; });
}

// Costs of the basic columns by row, times `sign`: Cost::One on artificial columns in phase 1 (tableau column indices), the
// variable costs in phase 2 (provider indices); a wrapped artificial index has none.  ld_b_ long, zero elsewhere.
std::vector<double> Engine::basic_costs(const std::vector<int32_t>& basis, int phase, double sign) const {
    std::vector<double> w(ld_b_, 0.0);
    for (int32_t i = 0; i < lay_.m; ++i) {
        const int32_t j = basis[i];
        if (j >= kWrappedArtificialBase) continue;
        if (phase == 1) w[i] = j < lay_.nr_artificial ? sign : 0.0;
        else if (j < lay_.nr_normal) w[i] = sign * lay_.cost[j];
        else if (lay_.added_of(j) >= 0) w[i] = sign * lay_.cost_of(j);       // (relp_add_columns; every other virtual column costs 0)
    }
    return w;
}

// Objective of the basis with values b in the current phase: the artificial variables in phase 1, c_B' b in phase 2
// (summed over the rows in order)
double Engine::objective_of(const std::vector<int32_t>& basis, const std::vector<double>& b) const {
    double objective = 0.0;
    for (int32_t i = 0; i < lay_.m; ++i) {
        const int32_t j = basis[i];
        if (j >= kWrappedArtificialBase) continue;
        if (phase_ == 1) { if (j < lay_.nr_artificial) objective += b[i]; }
        else if (j < lay_.nr_normal) objective += lay_.cost[j] * b[i];
        else if (lay_.added_of(j) >= 0) objective += lay_.cost_of(j) * b[i];   // (relp_add_columns; every other virtual column costs 0)
    }
    return objective;
}

// Rank-deficient problems (filter/generic_wrapper.rs:51, carry/mod.rs:650-689, basis_inverse_rows.rs:190-204):
// delete the given rows (and the same columns of B^-1) everywhere.  Rare, host round trip.
// The steps are named in the order they run; their copies take their lengths from the buffers and from the old and the new m
// (lay_.m is the old one until lay_.remove_rows).
relp_status_t Engine::remove_rows(const std::vector<int32_t>& rows) {
    const int32_t m_old = lay_.m, m_new = lay_.m - (int32_t)rows.size();
    std::vector<int32_t> map(m_old, 0);                // old row -> new row, -1 = removed
    std::vector<int32_t> perm(m_old), basis_perm;      // RELP_ARTIFICIAL_TEXTBOOK (plan); basis_perm: the basis array after the exchange
    bool identity_perm = true;

    auto plan = [&]() -> relp_status_t {               // the row map and the permutation
        if (cfg_.shard_count > 1 && !tableau_) return fail(RELP_E_UNSUPPORTED, "row removal in the sharded revised engine");
        for (size_t k = 0; k < rows.size(); ++k)
            if (rows[k] < 0 || rows[k] >= lay_.m || (k > 0 && rows[k] <= rows[k - 1])) return fail(RELP_E_STATE, "rows to remove must be ascending and distinct");
        size_t f = 0; int32_t out = 0;
        for (int32_t i = 0; i < lay_.m; ++i) {
            if (f < rows.size() && rows[f] == i) { map[i] = -1; ++f; } else map[i] = out++;
        }
        for (int32_t r : rows) if (r >= lay_.mc) return fail(RELP_E_STATE, "only constraint rows can be redundant");
        // The reference marks the INDEX of a stuck artificial as the redundant row (phase_one.rs:252).  When that index
        // lands on a <= or >= row, a row that is not redundant is deleted and what remains is no longer the inverse of a
        // basis of the filtered problem: the literal state is kept from here on, never rebuilt from the columns.
        for (int32_t r : rows) if (r >= lay_.nr_eq + lay_.nr_range) reinvert_interval_ = 0;
        // RELP_ARTIFICIAL_TEXTBOOK: an artificial variable that is stuck in basis position r but started in row o != r takes
        // its own constraint with it, i.e. the pair (constraint o, position r) goes -- always a basis of the filtered problem,
        // which (r, r) is only if (B^-1)[r][r] != 0.  Positions are labels: exchanging r and o (rows of B^-1 / of the tableau,
        // b, the basis array) first lets one index name both.  perm: position i of the new order holds the old position perm[i].
        for (int32_t i = 0; i < lay_.m; ++i) perm[i] = i;
        if (!stuck_artificials_.empty()) {
            basis_perm.resize(lay_.m);
            HIP_TRY(d_basis_.download(basis_perm, stream_));
            for (int32_t a : stuck_artificials_) {
                const int32_t o = lay_.column_to_row[a];
                const int32_t cur = (int32_t)(std::find(basis_perm.begin(), basis_perm.end(), a) - basis_perm.begin());
                if (cur >= lay_.m) return fail(RELP_E_STATE, "a stuck artificial variable is not basic");
                if (cur == o) continue;
                std::swap(basis_perm[cur], basis_perm[o]); std::swap(perm[cur], perm[o]);
                identity_perm = false;
            }
        }
        return RELP_OK;
    };
    // The tableau: every stored column loses the rows; the columns that were the identity of those rows stay as (never priced)
    // artificial columns.  Column by column to bound the host buffer.
    auto tableau_columns = [&]() -> relp_status_t {
        std::vector<double> col(m_old), coln(ld_t_);
        const int32_t n_owned = lay_.sc_hi - lay_.sc_lo;               // the stored columns of this rank (all of them unsharded)
        for (int32_t c = 0; c < n_owned; ++c) {
            HIP_TRY(dT0_.download(col, stream_, (int64_t)c * ld_t_));
            std::fill(coln.begin(), coln.end(), 0.0);
            for (int32_t i = 0; i < m_old; ++i) if (map[i] >= 0) coln[map[i]] = col[perm[i]];
            HIP_TRY(dT0_.upload(coln, stream_, (int64_t)c * ld_t_));
        }
        std::vector<int32_t> idn;
        for (int32_t i = 0; i < m_old; ++i) if (map[i] >= 0) idn.push_back(idcol_h_[i]);
        idcol_h_ = idn;
        HIP_TRY(d_idcol_.upload(idcol_h_, stream_));
        HIP_RETURN(d_pos_of_row_.fill_bytes(0xFF, m_old, stream_));
    };
    // The LU engine: the CSC matrix loses the rows; the factors are rebuilt at the end
    auto csc_matrix = [&]() -> relp_status_t {
        std::vector<int64_t> np(lay_.nr_normal + 1, 0);
        size_t o = 0;
        for (int32_t j = 0; j < lay_.nr_normal; ++j) {
            for (int64_t e = hc_ptr_[j]; e < hc_ptr_[j + 1]; ++e)
                if (map[hc_idx_[e]] >= 0) { hc_idx_[o] = map[hc_idx_[e]]; hc_val_[o] = hc_val_[e]; ++o; }
            np[j + 1] = (int64_t)o;
        }
        hc_idx_.resize(o); hc_val_.resize(o); hc_ptr_ = np;
        HIP_TRY(d_cptr_.upload(hc_ptr_, stream_));
        HIP_TRY(d_cidx_.upload(hc_idx_, stream_));
        HIP_TRY(d_cval_.upload(hc_val_, stream_));
        return ft_ ? ft_build_price_ell() : RELP_OK;
    };
    // The m-vectors b and basis -- and the explicit inverse, whose rows move as they do and whose columns go with the rows
    auto m_vectors = [&]() -> relp_status_t {
        const bool no_inv = tableau_ || lu_;
        std::vector<double> Bh(no_inv ? 0 : (size_t)m_old * ld_b_), b(m_old);
        std::vector<int32_t> basis(m_old);
        HIP_TRY(dBinv_.download(Bh, stream_));
        HIP_TRY(d_b_.download(b, stream_));
        HIP_TRY(d_basis_.download(basis, stream_));
        if (!identity_perm) {                              // the stuck artificial variables move into their own rows (plan)
            const std::vector<double> b0(b), B0(Bh);
            for (int32_t i = 0; i < m_old; ++i) b[i] = b0[perm[i]];
            basis = basis_perm;
            for (int32_t i = 0; i < m_old && !no_inv; ++i)
                if (perm[i] != i) std::copy(B0.begin() + (size_t)perm[i] * ld_b_, B0.begin() + (size_t)(perm[i] + 1) * ld_b_, Bh.begin() + (size_t)i * ld_b_);
        }
        std::vector<double> Bn(Bh.size(), 0.0), bn(m_new, 0.0);
        std::vector<int32_t> basisn(m_new, 0);
        for (int32_t i = 0; i < m_old; ++i) {
            if (map[i] < 0) continue;
            if (!no_inv)
                for (int32_t j = 0; j < m_old; ++j) if (map[j] >= 0) Bn[(size_t)map[i] * ld_b_ + map[j]] = Bh[(size_t)i * ld_b_ + j];
            bn[map[i]] = b[i];
            basisn[map[i]] = basis[i];
        }
        HIP_TRY(dBinv_.upload(Bn, stream_));
        HIP_TRY(d_b_.zero(ld_b_, stream_));
        HIP_TRY(d_b_.upload(bn, stream_));
        HIP_RETURN(d_basis_.upload(basisn, stream_));
    };
    // A: drop the rows inside every structural column (the LU engine holds no dense A; a sharded tableau no longer reads it, the
    // unsharded one re-tabulates from it)
    auto dense_matrix = [&]() -> relp_status_t {
        if (lay_.nr_normal <= 0 || lu_ || cfg_.shard_count != 1) return RELP_OK;
        std::vector<double> Ah((size_t)ld_a_ * lay_.nr_normal);
        HIP_TRY(dA_.download(Ah, stream_));
        std::vector<double> An(Ah.size(), 0.0);
        for (int32_t j = 0; j < lay_.nr_normal; ++j)
            for (int32_t i = 0; i < lay_.mc; ++i) if (map[i] >= 0) An[(size_t)j * ld_a_ + map[i]] = Ah[(size_t)j * ld_a_ + i];
        if (!dA_.owned()) HIP_TRY(dA_.alloc((int64_t)An.size()));          // (the caller's matrix was adopted: it stays as it is)
        HIP_RETURN(dA_.upload(An, stream_));
    };
    // The layout's tables (from here on lay_.m is the new m), and the stale tails of the other m-vectors, which must be zero for
    // the 16-byte loads
    auto layout_tables = [&]() -> relp_status_t {
        lay_.remove_rows(map);
        HIP_TRY(d_bound_row_.upload(lay_.bound_row.data(), lay_.nr_normal, stream_));
        HIP_TRY(d_vrow0_.upload(lay_.vrow0.data(), lay_.nr_virtual, stream_));
        HIP_TRY(d_vrow1_.upload(lay_.vrow1.data(), lay_.nr_virtual, stream_));
        for (DeviceBuf<double>* v : {&d_alpha_, &d_aq_, &d_rho_, &d_minus_pi_}) HIP_TRY(v->zero(ld_b_, stream_));
        return RELP_OK;
    };
    relp_status_t st = plan();
    if (!st && tableau_) st = tableau_columns();
    if (!st && lu_ && !tableau_) st = csc_matrix();
    if (!st) st = m_vectors();
    if (!st) st = dense_matrix();
    if (!st) st = layout_tables();
    return !st && lu_ ? lu_refactor() : st;
}

relp_status_t Engine::set_reinversion_interval(int64_t pivots) {
    if (pivots < 0) return fail(RELP_E_ARG, "negative interval");
    if (const relp_status_t st = in_trial("relp_set_reinversion_interval")) return st;
    if (pivots > 0 && (lu_ || cfg_.shard_count > 1))
        return fail(RELP_E_UNSUPPORTED, "re-inversion is for the unsharded revised and tableau engines (the LU engine refactorises anyway)");
    reinvert_interval_ = pivots;
    since_reinvert_ = 0;
    return RELP_OK;
}

// Sparse columns of the current basis in row space, for the host factorisation: artificial columns (phase 1,
// and the ones that survived it with a wrapped index) are unit columns of their rows, structural columns come
// from the device-resident A (+ their bound row), virtual columns from the descriptors.
relp_status_t Engine::build_basis_columns(const std::vector<int32_t>& basis,
                                          std::vector<std::vector<std::pair<int32_t, double>>>* cols) {
    cols->assign(lay_.m, {});
    std::vector<double> colbuf(std::max(lay_.mc, 1));
    hipError_t copied = hipSuccess;
    auto dense_column = [&](int32_t p, auto&& put) {
        copied = dA_.download(colbuf.data(), lay_.mc, stream_, (int64_t)(p - lay_.col_lo) * ld_a_);
        if (copied == hipSuccess)
            for (int32_t r = 0; r < lay_.mc; ++r) if (colbuf[r] != 0.0) put(r, colbuf[r]);
    };
    for (int32_t i = 0; i < lay_.m; ++i) {
        auto& c = (*cols)[i];
        if (!lay_.for_each_entry(basis[i], dense_column, [&c](int32_t row, double v) { c.emplace_back(row, v); }))
            return fail(RELP_E_STATE, "basis column out of range");
        HIP_TRY(copied);
    }
    return RELP_OK;
}

// B^-1, b, -pi and -obj from scratch for the CURRENT basis (either phase): host LU of the basis columns, then on
// the device the m unit BTRANs, b = B^-1 rhs and -pi = -(c_B' B^-1) with the costs of the phase.  What
// `LUDecomposition` does every 11 updates (lower_upper/mod.rs:199-202) the f64 explicit inverse needs every now and
// then: it is only ever updated, and on ill-conditioned LPs its error reaches the pivot tolerance after a few
// thousand pivots.
// The dense tableau's counterpart: T0 = B^-1 [artificial | A + bound rows | virtual] recomputed column by column from
// a fresh factorisation of the basis (one launch: workgroup c solves stored column c), b = B^-1 rhs, d re-priced
// from the new T0, -obj from b.  T0 is otherwise only ever updated (every flush adds W R0 to it).
//
// The shared start of both rebuilds: pending updates folded in, b kept for relp_config_t.auto_reinversion, the basis on the
// host, its columns factorised (hlu_) and the factors on the device.  `factored` false: lu_factor declined (numerically
// singular for the LU) and the caller keeps the updated state.
relp_status_t Engine::refactor_current_basis(std::vector<int32_t>* basis, std::vector<double>* b_before, bool* factored) {
    *factored = false;
    since_reinvert_ = 0;
    enqueue_flush();
    if (cfg_.auto_reinversion) { b_before->resize(lay_.m); HIP_TRY(d_b_.download(*b_before, stream_)); }
    basis->resize(lay_.m);
    HIP_TRY(d_basis_.download(*basis, stream_));
    std::vector<std::vector<std::pair<int32_t, double>>> cols;
    relp_status_t st = build_basis_columns(*basis, &cols);
    if (st) return st;
    std::string msg;
    if (!lu_factor(lay_.m, cols, &hlu_, &msg, sw_.lu_peel_stacks)) return RELP_OK;
    if ((st = lu_upload_factors())) return st;
    if ((st = ensure_lu_scratch())) return st;
    *factored = true;
    return RELP_OK;
}

relp_status_t Engine::ensure_lu_scratch() { HIP_RETURN(d_lu_scratch_.ensure(ld_b_)); }

// Where the batch solve over `rhs_count` right-hand sides keeps x.  In LDS while it fits (groups = 0).  Otherwise, or with
// RELP_RETAB_GLOBAL=1, in slabs of global memory: G = min(right-hand sides, 2 workgroups per CU, the slabs that fit into
// 256 MiB, RELP_RETAB_GROUPS) workgroups with ld_b_ doubles each (profiles/r10_retab_any_m.md).
relp_status_t Engine::batch_solve_slabs(int32_t rhs_count, LuSlabs* slabs) {
    *slabs = LuSlabs{nullptr, ld_b_, 0};
    if (rhs_count <= 0) return RELP_OK;
    if (!sw_.retab_global && lu_batch_fits_lds(lay_.m)) { ++batch_solves_lds_; return RELP_OK; }
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    int64_t groups = std::min<int64_t>(rhs_count, 2 * (int64_t)std::max(cus, 1));
    groups = std::min<int64_t>(groups, (int64_t(256) << 20) / ((int64_t)sizeof(double) * ld_b_));
    if (sw_.retab_groups > 0) groups = std::min<int64_t>(groups, sw_.retab_groups);
    groups = std::max<int64_t>(groups, 1);
    HIP_TRY(d_lu_slabs_.ensure(groups * ld_b_));
    slabs->x = d_lu_slabs_;
    slabs->groups = (int32_t)groups;
    slab_groups_last_ = slabs->groups;
    ++batch_solves_slab_;
    return RELP_OK;
}

relp_status_t Engine::retab_stats(int64_t* out4) const {
    out4[0] = batch_solves_lds_; out4[1] = batch_solves_slab_; out4[2] = slab_groups_last_;
    out4[3] = d_lu_slabs_.count() * (int64_t)sizeof(double);
    return RELP_OK;
}

// With the factors of the basis on the device: the rows of B^-1 by m unit BTRANs written in place (the one-off
// `BasisInverseRows::invert`, basis_inverse_rows.rs:103-129), -pi = -(w' B^-1) (carry/mod.rs:214-248) and b = B^-1 rhs, also
// downloaded into `b`.  `rearm`: the record is re-armed before the FTRAN (a warm start may find it decided).
relp_status_t Engine::inverse_from_factors(const std::vector<double>& w, bool rearm, std::vector<double>* b) {
    LuSlabs slabs;
    if (const relp_status_t st = batch_solve_slabs(lay_.m, &slabs)) return st;
    HIP_TRY(dBinv_.zero((int64_t)lay_.m * ld_b_, stream_));
    DeferredUpdate none = deferred();
    none.kmax = 0;
    launch_lu_btran_rows(dlu_, none, dBinv_, ld_b_, slabs, stream_);
    HIP_TRY(d_w_.upload(w, stream_));
    HIP_TRY(d_aq_.upload(lay_.rhs.data(), lay_.m, stream_));
    launch_weighted_column_sums(dBinv_, ld_b_, lay_.m, d_w_, d_minus_pi_, stream_);
    if (rearm) { const relp_status_t st = edit_rec(); if (st) return st; }
    launch_ftran(dBinv_, ld_b_, lay_.m, 0, lay_.m, d_aq_, d_b_, 0, d_rec_, stream_);
    b->resize(lay_.m);
    HIP_RETURN(d_b_.download(*b, stream_));
}

static double weighted_sum(const std::vector<double>& w, const std::vector<double>& b) {     // over the rows in order
    double s = 0.0;
    for (size_t i = 0; i < b.size(); ++i) s += w[i] * b[i];
    return s;
}

relp_status_t Engine::retabulate(bool adapt_interval) {
    SettledScope settled(*this);
    retab_done_ = false;
    std::vector<double> b_before;
    std::vector<int32_t> basis;
    bool factored = false;
    relp_status_t st = refactor_current_basis(&basis, &b_before, &factored);
    if (st || !factored) return st;                     // (not factored: keep the updated tableau)
    const TableauView tv = tview();
    // every stored column, the artificial block included: phase 2 never prices it, but B^-1 and -pi are read off the
    // columns that were the identity originally (relp_get_basis_inverse, relp_basis_inverse_row, relp_get_minus_pi)
    const int32_t c_first = lay_.sc_lo;
    ColumnTable storage = table();
    storage.nr_artificial = tab_na_;                    // storage columns keep the artificial block in front
    LuSlabs slabs;
    if ((st = batch_solve_slabs(lay_.sc_hi - c_first, &slabs))) return st;
    // Without added columns one launch over all stored columns.  With them (relp_add_columns) the stored columns are walked in
    // segments, every column solved once: the columns between two runs of added columns from A and the column table as ever (a
    // column's solve does not depend on the launch it is in: the same bits), every contiguous run of added columns from d_col_a_
    // by the same kernel, presented as "structural" columns over all m rows.
    int32_t c_next = c_first;
    for (int32_t a = 0; a < lay_.nr_added;) {
        int32_t run = 1;
        while (a + run < lay_.nr_added && lay_.added_virtual[a + run] == lay_.added_virtual[a] + run) ++run;
        ColumnTable block = storage;
        block.nr_artificial = tab_na_ + lay_.nr_normal + lay_.added_virtual[a];      // the run's first storage column
        block.nr_normal = run; block.nr_constraints = lay_.m; block.nr_cuts = 0;
        launch_lu_ftran_cols(dlu_, tv, A_base(), ld_a_, storage, c_next, block.nr_artificial - c_next, slabs, stream_);
        launch_lu_ftran_cols(dlu_, tv, d_col_a_ + (int64_t)a * ld_c_, ld_c_, block, block.nr_artificial, run, slabs, stream_);
        c_next = block.nr_artificial + run;
        a += run;
    }
    launch_lu_ftran_cols(dlu_, tv, A_base(), ld_a_, storage, c_next, lay_.sc_hi - c_next, slabs, stream_);
    HIP_TRY(d_aq_.upload(lay_.rhs.data(), lay_.m, stream_));
    launch_lu_ftran(dlu_, d_aq_, d_b_, d_lu_scratch_, nullptr, stream_);                 // b = B^-1 rhs
    tableau_reprice();                                  // as after every few flushes
    tab_partials_valid_ = true;
    std::vector<double> b(lay_.m);
    HIP_TRY(d_b_.download(b, stream_));
    if ((st = download_rec())) return st;
    h_rec_->minus_objective = -objective_of(basis, b);
    ++reinversions_;
    retab_done_ = true;
    if (cfg_.auto_reinversion && adapt_interval) auto_reinversion_adapt(b_before, b);
    return upload_rec();
}

relp_status_t Engine::reinvert() {
    SettledScope settled(*this);
    if (lu_ || cfg_.shard_count > 1) return fail(RELP_E_UNSUPPORTED, "re-inversion is for the unsharded revised and tableau engines");
    if (tableau_) return retabulate();
    std::vector<double> b_before, b;
    std::vector<int32_t> basis;
    bool factored = false;
    relp_status_t st = refactor_current_basis(&basis, &b_before, &factored);
    if (st || !factored) return st;                     // (not factored: keep the updated inverse)
    const std::vector<double> w = basic_costs(basis, phase_, 1.0);
    if ((st = inverse_from_factors(w, false, &b))) return st;
    if ((st = download_rec())) return st;
    h_rec_->minus_objective = -weighted_sum(w, b);
    ++reinversions_;
    if (cfg_.auto_reinversion) auto_reinversion_adapt(b_before, b);
    return upload_rec();
}

// relp_config_t.auto_reinversion: a rebuild that moved b by more than 1e-7 (relative to its largest entry) came too late -- the
// interval is halved, down to 32 pivots; one that moved it by less than 1e-10 could have waited -- doubled, up to 1,024 (a small
// drift of b does not vouch for the inverse: GREENBEA's tableau is lost at 4,096)
void Engine::auto_reinversion_adapt(const std::vector<double>& before, const std::vector<double>& after) {
    double diff = 0.0, scale = 1.0;
    for (size_t i = 0; i < after.size() && i < before.size(); ++i) { diff = std::max(diff, std::fabs(after[i] - before[i])); scale = std::max(scale, std::fabs(after[i])); }
    last_reinvert_drift_ = diff / scale;
    if (last_reinvert_drift_ > 1e-7) reinvert_interval_ = std::max<int64_t>(32, reinvert_interval_ / 2);
    else if (last_reinvert_drift_ < 1e-10) reinvert_interval_ = std::min<int64_t>(1024, reinvert_interval_ * 2);
    if (sw_.debug) std::fprintf(stderr, "[relp] rebuild %lld: b moved by %.2e (relative), interval now %lld\n", (long long)reinversions_, last_reinvert_drift_, (long long)reinvert_interval_);
}

// from_basis: every column a provider column, none twice.  `flags`: the in_basis flags of the basis.
relp_status_t Engine::check_basis_columns(const std::vector<int32_t>& basis, std::vector<uint8_t>* flags) {
    flags->assign(n_alloc_, 0);
    for (int32_t v : basis) {
        if (v < 0 || v >= lay_.n_provider) return fail(RELP_E_ARG, "from_basis: column out of range");
        if ((*flags)[v]) return fail(RELP_E_SINGULAR, "from_basis: duplicate column");
        (*flags)[v] = 1;
    }
    return RELP_OK;
}

relp_status_t Engine::from_basis(const int32_t* basis_columns) {
    // InverseMaintener::from_basis (carry/mod.rs:428-463): any basis on the LU and the revised engine (the
    // latter factorises on the host and runs the m unit solves on the device; slack bases are a signed permutation and take a shortcut).
    if (cfg_.shard_count > 1) return fail(RELP_E_UNSUPPORTED, "from_basis in sharded mode");
    if (const relp_status_t st = in_trial("relp_from_basis")) return st;
    const std::vector<int32_t> basis(basis_columns, basis_columns + lay_.m);
    std::vector<uint8_t> flags;
    relp_status_t st;
    auto phase_two = [](PivotRecord& r) { r.last_selected = -1; r.phase = 2; };
    if (tableau_) {
        // T = B^-1 [A | I] for the given basis: factorise it (host, like every refactorisation), then every stored column
        // by one FTRAN each in a single launch (re-tabulation), b = B^-1 rhs, d = c - c_B' T
        enqueue_flush();
        if ((st = check_basis_columns(basis, &flags))) return st;
        const int32_t keep_na = lay_.nr_artificial, keep_phase = phase_;
        lay_.nr_artificial = 0; phase_ = 2;
        HIP_TRY(d_basis_.upload(basis, stream_));
        cost_store_h_.assign(n_store_, 0.0);
        for (int32_t p = 0; p < lay_.nr_normal; ++p) cost_store_h_[tab_na_ + p] = lay_.cost[p];
        for (int32_t a = 0; a < lay_.nr_added; ++a) cost_store_h_[tab_na_ + lay_.nr_normal + lay_.added_virtual[a]] = lay_.added_cost[a];
        HIP_TRY(d_cost_store_.upload(cost_store_h_, stream_));
        st = retabulate();
        if (st || !retab_done_) {
            lay_.nr_artificial = keep_na; phase_ = keep_phase;
            return st ? st : fail(RELP_E_SINGULAR, "from_basis: the basis could not be factorised");
        }
        HIP_TRY(d_in_basis_.upload(flags, stream_));
        tab_partials_valid_ = false;
        return edit_rec(phase_two);
    }
    if (lu_) {
        // any basis: factorise it, b = B^-1 rhs (FTRAN), -pi = -c_B' B^-1 (BTRAN), carry/mod.rs:428-463
        if ((st = check_basis_columns(basis, &flags))) return st;
        lay_.nr_artificial = 0; phase_ = 2;
        HIP_TRY(d_basis_.upload(basis, stream_));
        HIP_TRY(d_in_basis_.upload(flags, stream_));
        since_flush_ = 1;                              // force: the factors are stale
        if ((st = lu_refactor())) return st;
        const std::vector<double> w = basic_costs(basis, 2, -1.0);        // BTRAN with rhs -c_B gives -pi directly
        std::vector<double> b(lay_.m);
        HIP_TRY(d_w_.upload(w.data(), lay_.m, stream_));
        HIP_TRY(d_aq_.upload(lay_.rhs.data(), lay_.m, stream_));
        lu_ftran(d_aq_, d_b_, nullptr);
        lu_btran(-1, d_w_, d_minus_pi_);
        HIP_TRY(d_b_.download(b, stream_));
        return edit_rec([&](PivotRecord& r) { r.minus_objective = -objective_of(basis, b); phase_two(r); });
    }
    enqueue_flush();                                   // leaves the deferred state empty
    if ((st = check_basis_columns(basis, &flags))) return st;
    double objective = 0.0;
    bool unit_basis = true;
    for (int32_t p : basis)
        if (p < lay_.nr_normal || lay_.vrow1[p - lay_.nr_normal] >= 0) unit_basis = false;
    if (unit_basis) {
        // slack basis (two_phase/mod.rs:103-111 `FullInitialBasis`): the inverse is a signed permutation
        std::vector<double> Bn((size_t)lay_.m * ld_b_, 0.0), b(lay_.m, 0.0), minus_pi(ld_b_, 0.0);
        std::vector<uint8_t> seen(lay_.m, 0);
        for (int32_t i = 0; i < lay_.m; ++i) {
            const int32_t v = basis[i] - lay_.nr_normal;
            const int32_t row = lay_.vrow0[v];
            if (row < 0) return fail(RELP_E_SINGULAR, "from_basis: empty column in the basis");
            if (seen[row]) return fail(RELP_E_SINGULAR, "from_basis: duplicate pivot row");
            seen[row] = 1;
            // column i of B is sign * e_row  =>  row i of B^-1 is sign * e_row'
            Bn[(size_t)i * ld_b_ + row] = (double)lay_.vsign[v];
            b[i] = (double)lay_.vsign[v] * lay_.rhs[row];
        }
        HIP_TRY(dBinv_.upload(Bn, stream_));
        HIP_TRY(d_b_.upload(b, stream_));
        HIP_TRY(d_minus_pi_.upload(minus_pi, stream_));
    } else {
        // any basis: factorise it on the host (relp_lu.cpp, like every refactorisation); the rows of B^-1, -pi and b on the device
        std::vector<int32_t> columns(basis);               // tableau column indices of the current kind
        for (auto& j : columns) j += lay_.nr_artificial;
        std::vector<std::vector<std::pair<int32_t, double>>> cols;
        if ((st = build_basis_columns(columns, &cols))) return st;
        std::string msg;
        if (!lu_factor(lay_.m, cols, &hlu_, &msg, sw_.lu_peel_stacks)) return fail(RELP_E_SINGULAR, "from_basis: " + msg);
        if ((st = lu_upload_factors())) return st;
        if ((st = ensure_lu_scratch())) return st;
        const std::vector<double> w = basic_costs(basis, 2, 1.0);
        std::vector<double> b;
        if ((st = inverse_from_factors(w, true, &b))) return st;
        objective = weighted_sum(w, b);
    }
    HIP_TRY(d_basis_.upload(basis, stream_));
    HIP_TRY(d_in_basis_.upload(flags, stream_));
    lay_.nr_artificial = 0; phase_ = 2;
    return edit_rec([&](PivotRecord& r) { r.minus_objective = -objective; phase_two(r); });
}

// ------------------------------------------------------------------------------------------------
// Getters
// ------------------------------------------------------------------------------------------------
relp_status_t Engine::get_objective(double* out) {
    relp_status_t st = download_rec();
    if (st) return st;
    *out = -h_rec_->minus_objective;
    return RELP_OK;
}

relp_status_t Engine::get_vector(int which, double* out) {
    if (tableau_ && which == 1) {
        if (cfg_.shard_count > 1) return fail(RELP_E_UNSUPPORTED, "-pi of the sharded tableau: d is column-sharded");
        // -pi_k = d_j - c_j for the stored column j that was e_k originally
        std::vector<double> d(n_store_);
        HIP_TRY(d_d_.download(d, stream_));
        for (int32_t k = 0; k < lay_.m; ++k) out[k] = d[idcol_h_[k]] - cost_store_h_[idcol_h_[k]];
        return RELP_OK;
    }
    const DeviceBuf<double>& src = which == 0 ? d_b_ : which == 1 ? d_minus_pi_ : d_alpha_;
    HIP_RETURN(src.download(out, lay_.m, stream_));
}

relp_status_t Engine::get_basis_indices(int32_t* out) { HIP_RETURN(d_basis_.download(out, lay_.m, stream_)); }

relp_status_t Engine::get_basis_inverse(double* out) {
    if (cfg_.shard_count > 1) return fail(RELP_E_UNSUPPORTED, "B^-1 is row-sharded");
    if (const relp_status_t st = in_trial("relp_get_basis_inverse (it flushes the open block)")) return st;
    if (!lu_) enqueue_flush();
    if (lu_ || tableau_) {
        DeviceBuf<double> tmp;                             // (freed on every way out)
        HIP_TRY(tmp.alloc((int64_t)lay_.m * lay_.m));
        // LU: row i of B^-1 = BTRAN of e_i (with the pending updates); test / debugging path.  Tableau: B^-1 = the tableau
        // columns of the original identity columns
        if (lu_) for (int32_t i = 0; i < lay_.m; ++i) lu_btran(i, nullptr, tmp + (int64_t)i * lay_.m);
        else launch_tab_gather_columns(tview(), d_idcol_, tmp, stream_);
        HIP_RETURN(tmp.download(out, (int64_t)lay_.m * lay_.m, stream_));
    }
    HIP_RETURN(dBinv_.copy_2d(kToHost, out, lay_.m, lay_.m, lay_.m, ld_b_, stream_));
}

relp_status_t Engine::current_bfs(int32_t* cols, double* vals, int32_t cap, int32_t* count) {
    std::vector<double> b(lay_.m); std::vector<int32_t> basis(lay_.m);
    relp_status_t st = get_vector(0, b.data());
    if (st) return st;
    if ((st = get_basis_indices(basis.data()))) return st;
    std::vector<std::pair<int32_t, double>> t;
    for (int32_t i = 0; i < lay_.m; ++i) if (b[i] != 0.0) t.emplace_back(basis[i], b[i]);
    std::sort(t.begin(), t.end(), [](auto& a, auto& c) { return a.first < c.first; });
    int32_t k = 0;
    for (auto& e : t) { if (k < cap) { cols[k] = e.first; vals[k] = e.second; } ++k; }
    if (count) *count = k;
    return RELP_OK;
}

relp_status_t Engine::get_iterations(int64_t* out) {
    relp_status_t st = download_rec();
    if (st) return st;
    *out = h_rec_->iterations;
    return RELP_OK;
}

relp_status_t Engine::get_degenerate_pivots(int64_t* out) {
    relp_status_t st = download_rec();
    if (st) return st;
    *out = h_rec_->degenerate;
    return RELP_OK;
}

relp_status_t Engine::tab_flush_stats(int64_t* out2) {
    unsigned long long h[2] = {0, 0};
    if (d_fstats_) HIP_TRY(d_fstats_.download(h, 2, stream_));
    out2[0] = (int64_t)h[0]; out2[1] = (int64_t)h[1];
    return RELP_OK;
}

relp_status_t Engine::get_trace(int32_t* phase, int32_t* entering, int32_t* row, int32_t* leaving, int64_t cap,
                                int64_t* count) {
    relp_status_t st = download_rec();
    if (st) return st;
    const int64_t n = std::min<int64_t>(h_rec_->iterations, trace_cap_);
    const int64_t k = std::min(n, cap);
    int32_t* outs[4] = {phase, entering, row, leaving};
    for (int f = 0; f < 4; ++f)
        if (outs[f] && k > 0) HIP_TRY(d_trace_.download(outs[f], k, stream_, f * trace_cap_));
    if (count) *count = n;
    return RELP_OK;
}

// tableau/mod.rs:253-289: regenerate every basis column (must be e_i), basic reduced costs (0), b >= 0
relp_status_t Engine::check_basis(double* max_identity_error, double* max_basic_cost, double* min_b) {
    std::vector<int32_t> basis(lay_.m);
    relp_status_t st = get_basis_indices(basis.data());
    if (st) return st;
    std::vector<double> col(lay_.m), d(nr_columns()), b(lay_.m);
    double e1 = 0.0, e2 = 0.0, mb = std::numeric_limits<double>::infinity();
    for (int32_t i = 0; i < lay_.m; ++i) {
        if (basis[i] >= kWrappedArtificialBase) continue;       // no column to regenerate
        if ((st = generate_column(basis[i], col.data()))) return st;
        for (int32_t k = 0; k < lay_.m; ++k) e1 = std::max(e1, std::fabs(col[k] - (k == i ? 1.0 : 0.0)));
    }
    if ((st = relative_costs(d.data()))) return st;
    for (int32_t i = 0; i < lay_.m; ++i) if (basis[i] < kWrappedArtificialBase) e2 = std::max(e2, std::fabs(d[basis[i]]));
    if ((st = get_vector(0, b.data()))) return st;
    for (double v : b) mb = std::min(mb, v);
    if (max_identity_error) *max_identity_error = e1;
    if (max_basic_cost) *max_basic_cost = e2;
    if (min_b) *min_b = mb;
    return RELP_OK;
}

}  // namespace relp
