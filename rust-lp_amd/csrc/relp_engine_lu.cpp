// relp_engine_lu.cpp -- Engine: the sparse LU engine (RELP_ENGINE_LU): CSC upload, host refactorisation,
// one pivot.  See relp_engine.hpp and relp_lu.hpp.
#include "relp_engine_internal.hpp"
#include "relp_lu_image.hpp"

#include <algorithm>
#include <climits>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace relp {

// ------------------------------------------------------------------------------------------------
// Sparse LU engine: matrix in CSC, factors from the host (relp_lu.cpp), solves on the device
// ------------------------------------------------------------------------------------------------
relp_status_t Engine::lu_load_matrix(const relp_matrix_data_t& md) {
    hc_ptr_.assign(lay_.nr_normal + 1, 0);
    hc_idx_.clear(); hc_val_.clear();
    if (md.format == RELP_FORMAT_CSC) {
        if (md.matrix_memory != RELP_MEM_HOST) return fail(RELP_E_UNSUPPORTED, "CSC input must be in host memory");
        if (!md.col_ptr) return fail(RELP_E_ARG, "col_ptr missing");
        for (int32_t j = 0; j < lay_.nr_normal; ++j) {
            for (int64_t p = md.col_ptr[j]; p < md.col_ptr[j + 1]; ++p) {
                const int32_t i = md.row_idx[p];
                if (i < 0 || i >= lay_.mc) return fail(RELP_E_ARG, "row index out of range");
                if (md.values[p] == 0.0) continue;
                hc_idx_.push_back(i); hc_val_.push_back(md.values[p]);
            }
            hc_ptr_[j + 1] = (int64_t)hc_idx_.size();
        }
    } else if (md.format == RELP_FORMAT_DENSE) {
        if (lay_.nr_normal > 0 && lay_.mc > 0 && !md.dense) return fail(RELP_E_ARG, "dense matrix missing");
        const int64_t src_ld = md.dense_ld > 0 ? md.dense_ld : lay_.mc;
        if (src_ld < lay_.mc) return fail(RELP_E_ARG, "dense_ld < nr_constraints");
        std::vector<double> col(std::max(lay_.mc, 1));
        for (int32_t j = 0; j < lay_.nr_normal; ++j) {
            const double* src = md.dense + (int64_t)j * src_ld;
            if (md.matrix_memory == RELP_MEM_DEVICE) {
                if (const relp_status_t st = fetch(col.data(), src, sizeof(double) * lay_.mc)) return st;     // (the caller's matrix)
                src = col.data();
            }
            for (int32_t i = 0; i < lay_.mc; ++i)
                if (src[i] != 0.0) { hc_idx_.push_back(i); hc_val_.push_back(src[i]); }
            hc_ptr_[j + 1] = (int64_t)hc_idx_.size();
        }
    } else {
        return fail(RELP_E_ARG, "unknown matrix format");
    }
    HIP_TRY(d_cptr_.alloc(lay_.nr_normal + 1));
    HIP_TRY(d_cidx_.alloc((int64_t)hc_idx_.size()));
    HIP_TRY(d_cval_.alloc((int64_t)hc_val_.size()));
    HIP_TRY(d_cptr_.upload(hc_ptr_, stream_));
    HIP_TRY(d_cidx_.upload(hc_idx_, stream_));
    HIP_RETURN(d_cval_.upload(hc_val_, stream_));
}

// The basis as it is on the device -> pinned host memory.  Synchronises the stream.
relp_status_t Engine::lu_download_basis() { HIP_RETURN(d_basis_.download(h_basis_, lay_.m, stream_)); }

// the columns of the basis in h_basis_ from the host copy of the matrix (the LU engine never holds A densely)
relp_status_t Engine::lu_basis_columns(std::vector<std::vector<std::pair<int32_t, double>>>& cols) {
    cols.resize(lay_.m);
    for (int32_t i = 0; i < lay_.m; ++i) {
        auto& c = cols[i];
        c.clear();
        if (!lay_.for_each_entry(h_basis_[i], csc_column(), [&c](int32_t row, double v) { c.emplace_back(row, v); }))
            return fail(RELP_E_STATE, "basis column out of range");
    }
    return RELP_OK;
}

// The same columns as one flat copy (column i = entries [ptr[i], ptr[i + 1])): what lu_factor_csc wants -- at 64,000 rows the
// vector per column was a cache miss per column and pass.
relp_status_t Engine::lu_basis_flat(std::vector<int64_t>& ptr, std::vector<int32_t>& idx, std::vector<double>& val) {
    ptr.assign((size_t)lay_.m + 1, 0);
    idx.clear(); val.clear();
    auto put = [&](int32_t row, double v) { idx.push_back(row); val.push_back(v); };
    for (int32_t i = 0; i < lay_.m; ++i) {
        if (!lay_.for_each_entry(h_basis_[i], csc_column(), put)) return fail(RELP_E_STATE, "basis column out of range");
        ptr[(size_t)i + 1] = (int64_t)idx.size();
    }
    return RELP_OK;
}

// P B Q = L U on the host for the basis in h_basis_ (hlu_ is overwritten)
relp_status_t Engine::lu_factor_downloaded_basis() {
    if (!sw_.dump_basis_set) {
        const relp_status_t fst = lu_basis_flat(basis_ptr_, basis_idx_, basis_val_);
        if (fst) return fst;
        std::string msg;
        if (!lu_factor_csc(lay_.m, basis_ptr_.data(), basis_idx_.data(), basis_val_.data(), &hlu_, &msg, sw_.lu_peel_stacks)) return fail(RELP_E_SINGULAR, msg);
        return RELP_OK;
    }
    std::vector<std::vector<std::pair<int32_t, double>>>& cols = basis_cols_;     // (kept: no 790 allocations per refactorisation)
    const relp_status_t cst = lu_basis_columns(cols);
    if (cst) return cst;
    if (lu_refactors_ == 100) {                            // one mid-solve basis as text: m, then per column "n i v i v ..."
        if (FILE* f = std::fopen(sw_.dump_basis.c_str(), "w")) {
            std::fprintf(f, "%d\n", lay_.m);
            for (auto& c : cols) { std::fprintf(f, "%zu", c.size()); for (auto& e : c) std::fprintf(f, " %d %.17g", e.first, e.second); std::fprintf(f, "\n"); }
            std::fclose(f);
        }
    }
    std::string msg;
    if (!lu_factor(lay_.m, cols, &hlu_, &msg, sw_.lu_peel_stacks)) return fail(RELP_E_SINGULAR, msg);
    return RELP_OK;
}

void Engine::lu_refactor_clock(std::chrono::steady_clock::time_point tb, std::chrono::steady_clock::time_point t0,
                               std::chrono::steady_clock::time_point t1, std::chrono::steady_clock::time_point t2) {
    refactor_us_[0] += std::chrono::duration<double, std::micro>(t0 - tb).count();
    refactor_us_[1] += std::chrono::duration<double, std::micro>(t1 - t0).count();
    refactor_us_[2] += std::chrono::duration<double, std::micro>(t2 - t1).count();
    if (sw_.debug && lu_refactors_ % 60 == 59)
        std::fprintf(stderr, "[relp] refactorisations so far %lld: basis download + columns %.0f us, lu_factor %.0f us, schedules + upload %.0f us (averages)\n",
                     (long long)lu_refactors_ + 1, refactor_us_[0] / (lu_refactors_ + 1), refactor_us_[1] / (lu_refactors_ + 1),
                     refactor_us_[2] / (lu_refactors_ + 1));
}

// Refactorisation (lower_upper/mod.rs:199-202 + carry/mod.rs:602-614): B from the current basis
// columns, P B Q = L U on the host, schedules to the device, W := empty.  Synchronises the stream.
relp_status_t Engine::lu_refactor() {
    const auto tb = std::chrono::steady_clock::now();
    relp_status_t st = RELP_OK;
    bool on_device = false;
    if (luf_enabled_) {                                    // P B Q = L U by the device kernel: no basis download, no host search
        int32_t dev = 0;
        st = lu_factor_on_device(&dev);
        if (st == RELP_OK) on_device = true;
        else if (st != RELP_E_UNSUPPORTED) return st;
        else ++luf_fallbacks_;
    }
    if (!on_device && (st = lu_download_basis())) return st;
    const auto t0 = std::chrono::steady_clock::now();
    if (!on_device && (st = lu_factor_downloaded_basis())) return st;
    const auto t1 = std::chrono::steady_clock::now();
    // (a device-resident factorisation has installed its schedules where the kernels built them: nothing to pack or upload)
    if (!(on_device && luf_is_resident()) && (st = lu_upload_factors())) return st;
    if (ft_) { if ((st = ft_reset())) return st; }
    else launch_flush_reset(deferred(), d_rec_, stream_);
    HIP_TRY(hipStreamSynchronize(stream_));                // the reset has run: the clock below and the callers count on it
    lu_refactor_clock(tb, t0, t1, std::chrono::steady_clock::now());
    since_flush_ = 0;
    ++lu_refactors_;
    return RELP_OK;
}

// Refactorisation without stopping the pivot kernel (persistent-kernel mode).  The kernel has just returned with
// `max_updates - lookahead` updates pending.  Its basis is downloaded, the kernel is launched again on the OLD factors (it
// may fill the rest of the update file), and while it pivots the host factorises the downloaded basis into the other
// device buffer.  When both are done the new factors are installed and the basis changes made meanwhile (the kernel's
// journal) are applied to them as Forrest-Tomlin updates by k_ft_replay: the device pivots for the ~0.6 ms it used to
// wait.  If the kernel ended the phase meanwhile, the new factors are dropped: the old ones with their update file
// describe the final basis.
relp_status_t Engine::lu_refactor_lookahead(int rule, int64_t budget, bool have_basis) {
    const auto tb = std::chrono::steady_clock::now();
    relp_status_t st = have_basis ? RELP_OK : lu_download_basis();       // (have_basis: the kernel's own report held it)
    if (st) return st;
    FtState go = fts_;
    go.max_updates = std::max(go.max_updates, std::min(cfg_.update_block < 0 ? ft_tcap_ : cfg_.update_block, ft_tcap_));
    if (lu_pipeline_cap_ > 0) go.max_updates = std::min(lu_pipeline_cap_, ft_tcap_);       // (run_ft: RELP_LU_PIPELINE_SHORT)
    prof_tick_ = 0;
    prof_begin(RELP_K_FT_RUN);
    ft_enqueue_pivots(go, rule, budget);
    prof_end();
    const auto t0 = std::chrono::steady_clock::now();
    // the current factors stay valid (and in use) until the new ones are installed
    LUFactors old_h = std::move(hlu_);
    const DeviceLU old_d = dlu_;
    const FtState old_f = fts_;
    d_lu_buf_.swap(d_lu_buf_alt_);                         // the new factors go into the other buffer, the old one stays in use
    hlu_ = LUFactors{};
    auto restore = [&]() {
        d_lu_buf_.swap(d_lu_buf_alt_);                     // (the other buffer may be empty after a refused re-allocation)
        hlu_ = std::move(old_h); dlu_ = old_d; fts_ = old_f;
    };
    st = lu_factor_downloaded_basis();
    const auto t1 = std::chrono::steady_clock::now();
    if (!st) st = lu_upload_factors();                     // (its copy queues behind the kernel; it returns when both are done)
    if (st) {                                              // keep what works; the kernel's result decides what happens next
        restore();
        relp_status_t st2 = ft_read_report(nullptr);
        ft_need_refactor_ = true;
        return st2 ? st2 : st;
    }
    if ((st = ft_read_report(nullptr))) { restore(); return st; }
    const int32_t changes = h_ft_hdr_[3];
    if (h_rec_->outcome != DEV_RUNNING || h_ft_hdr_[2] == 2 || changes > ft_tcap_) {
        restore();                                         // phase over (or something off): nothing to install
        if (h_ft_hdr_[2] == 2 || changes > ft_tcap_) ft_need_refactor_ = true;
        return RELP_OK;
    }
    if ((st = ft_reset())) return st;
    prof_begin(RELP_K_FLUSH);
    launch_ft_replay(dlu_, fts_, ft_problem(rule), changes, stream_);
    prof_end();
    lu_refactor_clock(tb, t0, t1, std::chrono::steady_clock::now());
    since_flush_ = changes;
    ft_need_refactor_ = false;                             // (a replay that fails marks the header; the next launch returns at once)
    ++lu_refactors_;
    ++lu_lookahead_installs_;
    lu_replayed_changes_ += changes;
    return RELP_OK;
}

// What the steps of lu_upload_factors hand on.  Every piece is put into the pinned buffer by the step that makes it, which
// also says where its device address goes: into dlu / fts, which replace dlu_ / fts_ once everything has arrived.
struct Engine::LuUpload {
    // (assembled in pinned memory that lives as long as the engine: the copy to the device is one DMA, not a staged one)
    Packer<PinnedStore> pk;
    DeviceLU dlu{};
    FtState fts;
    const TriangularSchedule* sch[4];
    EllPacked ell[4]; EllImageShape shape[4]; int64_t o_ell[4] = {0, 0, 0, 0};
    std::vector<int32_t> lev_ub;
    explicit LuUpload(Engine& e) : pk(PinnedStore{e.h_lu_buf_}), fts(e.fts_), sch{&e.hlu_.Lf, &e.hlu_.Uf, &e.hlu_.Ub, &e.hlu_.Lb} {}
};

// hlu_ (host factors + level schedules) -> one device buffer, dlu_ points into it.  Also used by the revised
// engine's warm start, which forms the rows of B^-1 with the device BTRAN.
relp_status_t Engine::lu_upload_factors() {
    LuUpload u(*this);
    relp_status_t st = RELP_OK;
    lu_pack_permutations(u);
    if (ft_ && (st = lu_pack_images(u))) return st;
    lu_pack_pivot_info(u);
    lu_pack_row_schedules(u);
    if ((st = lu_copy_to_device(u))) return st;
    return lu_install(u);
}

// rowperm, colperm; for the Forrest-Tomlin kernels: original row -> pivot, basis position -> pivot, pivot -> its row in the
// U / U' schedules
void Engine::lu_pack_permutations(LuUpload& u) {
    const int32_t m = lay_.m;
    u.dlu.m = m; u.dlu.pad_ = 0;
    u.pk.put(&u.dlu.rowperm, hlu_.rowperm); u.pk.put(&u.dlu.colperm, hlu_.colperm);
    std::vector<int32_t> inv_rp(m), inv_cp(m), task_uf(m), task_ub(m);
    for (int32_t k = 0; k < m; ++k) {
        inv_rp[hlu_.rowperm[k]] = k; inv_cp[hlu_.colperm[k]] = k;
        task_uf[hlu_.Uf.level_rows[k]] = k; task_ub[hlu_.Ub.level_rows[k]] = k;
    }
    u.pk.put(&u.fts.inv_rowperm, inv_rp); u.pk.put(&u.fts.inv_colperm, inv_cp);
    u.pk.put(&u.fts.task_uf, task_uf); u.pk.put(&u.fts.task_ub, task_ub);
}

// The four schedules once more for the persistent pivot kernel: consecutive levels fused into groups one pass solves
// (relp_lu.hpp: fuse_levels), packed "ELL by pass", one contiguous image each (relp_lu_image.hpp); rows of U and U' without
// entries are kept, an update may mask them.  Behind the images what a sweep reads besides them.
relp_status_t Engine::lu_pack_images(LuUpload& u) {
    const int32_t m = lay_.m;
    const int32_t fuse_cap = sw_.fuse_lanes;           // (RELP_FUSE_LANES, read at create)
    // (fused schedules read copies of some right-hand sides behind x: ft_rhs_cap_ words of LDS, and of index space)
    const int32_t cap = ft_rhs_cap_ > 0 ? fuse_cap : 0;
    const int64_t index_room = ft_big_ ? (int64_t(1) << kEllLgShiftWide) : (int64_t(1) << kEllLgShift);
    for (EllSchedule& d : u.fts.ell) d = EllSchedule{};
    // fusion and packing of the four schedules are independent: U on this thread, U' and L + L' on two helpers (the
    // refactorisation runs beside the pivot kernel, and what the host takes longer than the kernel's look-ahead the
    // device waits)
    auto prepare = [&](int k) {
        const bool maskable = k == 1 || k == 2;
        EllPacked& e = u.ell[k];
        FusedSchedule fs;
        // (big layout: right-hand-side copies compacted, rows without entries as a list when that saves two passes or more;
        // all-in-LDS layout: a copy per pivot by one LDS loop and every row a slot, as measured fastest on 25FV47)
        const int32_t triv_min = ft_big_ ? 512 : 0x7fffffff;
        fuse_levels(*u.sch[k], maskable, maskable, cap, &fs);
        ell_pack(fs, maskable, &e, ft_big_, ft_big_, triv_min);
        if (ft_big_ && ((int64_t)e.rhs_src.size() > ft_rhs_cap_ || (int64_t)m + 1 + (int64_t)e.rhs_src.size() > index_room)) {
            fuse_levels(*u.sch[k], maskable, maskable, 0, &fs);      // more copies than the layout has room for: level by level
            ell_pack(fs, maskable, &e, ft_big_, ft_big_, triv_min);
        }
        bool uses_rhs = false;
        for (int32_t v : fs.s.idx) if (v >= fs.rhs_base) { uses_rhs = true; break; }
        if (k == 2) u.lev_ub = fs.start_after;
        u.fts.ell[k].rhs_base = uses_rhs ? fs.rhs_base : 0;
    };
    if (m >= 256) {
        host_pool_.run(0, [&] { prepare(2); });
        host_pool_.run(1, [&] { prepare(0); prepare(3); });
        prepare(1);
        host_pool_.wait();
    } else {
        for (int k = 0; k < 4; ++k) prepare(k);
    }
    for (int k = 0; k < 4; ++k) {
        u.shape[k] = ell_image_shape(u.ell[k], m, ft_big_);
        char* const dst = u.pk.reserve(u.shape[k].layout().total, &u.o_ell[k]);
        if (dst && !ell_image_write(u.ell[k], u.shape[k], dst)) return fail(RELP_E_STATE, "a packed schedule does not fit its image layout");
    }
    for (int k = 1; k <= 2; ++k) {
        const bool has_via = !u.ell[k].via_ptr.empty();
        u.pk.put(&u.fts.ell[k].via_ptr, u.ell[k].via_ptr, has_via);
        u.pk.put(&u.fts.ell[k].via_pos, u.ell[k].via_pos, has_via);
    }
    for (int k = 0; k < 4; ++k) {
        const EllPacked& e = u.ell[k];
        EllSchedule& d = u.fts.ell[k];
        u.pk.put(&d.rhs_src, e.rhs_src);
        u.pk.put(&d.triv, e.triv);
        d.n_triv = (int32_t)e.triv.size();
        d.n_rhs = ft_big_ ? (int32_t)e.rhs_src.size() : -1;
        if (ft_tier_ >= 2) {                           // layout 2 walks the non-zeros of x: the inverse of rhs_src, `triv` as a bitmap
            std::vector<int32_t> pos(m, -1);
            for (size_t i = 0; i < e.rhs_src.size(); ++i) pos[e.rhs_src[i]] = (int32_t)i;
            std::vector<uint32_t> tb((size_t)(m + 31) / 32 + 1, 0u);
            for (int32_t r : e.triv) tb[(size_t)r >> 5] |= 1u << (r & 31);
            u.pk.put(&d.rhs_pos, pos);
            u.pk.put(&d.triv_bits, tb);
        }
        u.pk.put(&d.reach, e.reach);
    }
    return RELP_OK;
}

// pivot -> level (group) of its row in the U' schedule, and what an update of a pivot needs in one load
void Engine::lu_pack_pivot_info(LuUpload& u) {
    const int32_t m = lay_.m;
    if (!ft_) {                                            // (the persistent kernel's images: start_after of the fused U', lu_pack_images)
        u.lev_ub.assign(m, 0);
        for (int32_t l = 0; l + 1 < (int32_t)hlu_.Ub.level_ptr.size(); ++l)
            for (int32_t t = hlu_.Ub.level_ptr[l]; t < hlu_.Ub.level_ptr[l + 1]; ++t) u.lev_ub[hlu_.Ub.level_rows[t]] = l;
    }
    u.pk.put(&u.fts.lev_ub, u.lev_ub);
    if (!ft_) return;
    std::vector<FtPivotInfo> pinfo(m);
    const std::vector<int32_t>& via_u = u.ell[1].via_ptr;
    const std::vector<int32_t>& via_t = u.ell[2].via_ptr;
    for (int32_t p = 0; p < m; ++p) {
        FtPivotInfo& q = pinfo[p];
        q.u_e0 = hlu_.Uf.ptr[p]; q.u_e1 = hlu_.Uf.ptr[p + 1];
        q.via_u0 = via_u.empty() ? 0 : via_u[p]; q.via_u1 = via_u.empty() ? 0 : via_u[p + 1];
        q.via_t0 = via_t.empty() ? 0 : via_t[p]; q.via_t1 = via_t.empty() ? 0 : via_t[p + 1];
        q.lev_ub = u.lev_ub[p]; q.pad_ = 0;
    }
    u.pk.put(&u.fts.pinfo, pinfo);
}

// the row-wise schedules of the product-form kernels: rows in solve order, entries, level offsets, runs of levels
void Engine::lu_pack_row_schedules(LuUpload& u) {
    DeviceSchedule* ds[4] = {&u.dlu.Lf, &u.dlu.Uf, &u.dlu.Ub, &u.dlu.Lb};
    std::vector<LuRow> rows(lay_.m);
    for (int k = 0; k < 4; ++k) {
        const TriangularSchedule& t = *u.sch[k];
        DeviceSchedule& d = *ds[k];
        d.n_levels = (int32_t)t.level_ptr.size() - 1;
        d.nnz = (int32_t)t.idx.size();
        if (ft_) {
            // the Forrest-Tomlin kernels solve from the ELL images; of the row-wise schedules they read one thing, the
            // entries of a row of U (the u_bar of an update)
            if (k == 1) { u.pk.put(&d.idx, t.idx); u.pk.put(&d.val, t.val); }
            continue;
        }
        for (int32_t i = 0; i < lay_.m; ++i) {
            const int32_t r = t.level_rows[i];
            rows[i] = LuRow{r, t.ptr[r], t.ptr[r + 1], 0, 1.0 / t.diag[r]};
        }
        u.pk.put(&d.rows, rows);
        u.pk.put(&d.idx, t.idx);
        u.pk.put(&d.val, t.val);
        u.pk.put(&d.level_ptr, t.level_ptr);
        // (directly behind level_ptr: the kernel stages all five arrays in one copy)
        const std::vector<int32_t> runs = lu_level_runs(t.level_ptr);
        u.pk.put(&d.seg, runs);
        d.n_seg = (int32_t)runs.size() / 3;
    }
}

// the pinned buffer -> the device buffer (grown when it is too small); the pieces' addresses -> u.dlu / u.fts
relp_status_t Engine::lu_copy_to_device(LuUpload& u) {
    if (u.pk.failed()) return fail(RELP_E_ALLOC, "pinned staging buffer for the factors");
    const int64_t bytes = u.pk.size();
    HIP_TRY(d_lu_buf_.ensure_raw((size_t)bytes, (size_t)(bytes * 3 / 2 + 256)));
    HIP_TRY(d_lu_buf_.upload(h_lu_buf_, bytes, stream_));  // (waits: the pinned buffer is rewritten by the next refactorisation)
    u.pk.bind(d_lu_buf_);
    return RELP_OK;
}

relp_status_t Engine::lu_install(LuUpload& u) {
    dlu_ = u.dlu;
    if (!ft_) return RELP_OK;
    if (ft_tier_ >= 2 && fts_.m != lay_.m) {               // rows were removed: the bitmaps saved between launches describe another m
        const int32_t reset[4] = {-1, -1, 0, 0};
        HIP_TRY(upload_to(fts_.nzc, reset, 4, stream_));
    }
    fts_ = u.fts;
    fts_.m = lay_.m;
    for (int k = 0; k < 4; ++k) ell_image_view(d_lu_buf_ + u.o_ell[k], u.shape[k], &fts_.ell[k]);
    const int64_t base = ft_plan_staging(fts_);
    if (sw_.debug && lu_refactors_ % 60 == 59)
        for (int k = 0; k < 4; ++k)
            std::fprintf(stderr, "[relp] schedule %d: %d levels, %d passes, %d lanes (%d entries), image %d bytes, staged %d (stage area %d, base %lld)\n",
                         k, fts_.ell[k].n_levels, fts_.ell[k].n_passes, fts_.ell[k].n_lanes, (int)u.sch[k]->idx.size(),
                         fts_.ell[k].bytes, fts_.stage[k], fts_.stage_bytes, (long long)base);
    return RELP_OK;
}

// What is left of the CU's LDS after the work vectors stages one schedule image at a time: which of f.ell fit, and the
// dynamic LDS the kernels ask for.
int64_t Engine::ft_plan_staging(FtState& f) const {
    const int64_t base = (int64_t)ft_lds_base_bytes(lay_.m, ft_tcap_, ft_eta_cap_, ft_tier_, ft_rhs_cap_);
    f.stage_bytes = (int32_t)std::max<int64_t>(0, kFtLdsBudget - base);
    int64_t need = 0;
    for (int k = 0; k < 4; ++k) {
        f.stage[k] = f.ell[k].bytes <= f.stage_bytes ? 1 : 0;
        // (layout 2 copies the pass headers of an image that is not staged: sweep())
        const int64_t hb = 16 * ((int64_t)f.ell[k].n_passes + kEllPadHeaders);
        if (f.stage[k]) need = std::max<int64_t>(need, f.ell[k].bytes);
        else if (ft_tier_ >= 2 && hb <= f.stage_bytes) need = std::max(need, hb);
    }
    f.lds_bytes = (int32_t)(base + need);
    return base;
}

// ------------------------------------------------------------------------------------------------
// Forrest-Tomlin mode (relp_kernels_ft.hip)
// ------------------------------------------------------------------------------------------------
relp_status_t Engine::ft_plan_and_alloc() {
    ft_ = false; ft_big_ = false; ft_tier_ = 0; ft_rhs_cap_ = 0;
    if (lay_.m > kFtMaxRows) return RELP_OK;
    // The dense tail of U (tcap x tcap in LDS) is as large as the refactorisation interval asks for, not larger: what it does
    // not take stages the triangular factors, and an image that does not fit is solved from L2 at several times the cost.
    // Default interval 48: with a refactorisation at ~0.7 ms and ~1,100 clocks per pending update and pivot, the optimum is
    // flat between 40 and 64, and 48 x 49 doubles leave 14 KB more for the images than 64 x 65.
    int32_t want = cfg_.update_block < 0 ? 48 : std::max(1, std::min(cfg_.update_block, kFtMaxSlots));
    // (RELP_LU_PIPELINE_SHORT, run_ft: a short interval pivots on into a tail twice as long while the host factorises)
    if (sw_.lu_pipeline_short && want < 24) want = 2 * want;
    // Two layouts (relp_kernels_ft.hip: ft_layout).  "All in LDS": x with m right-hand-side copies, spike, -pi, permutations,
    // eta pool -- 63 bytes per row.  "big": x, -pi and the slot tables only (17 bytes per row + 8 per right-hand-side copy the
    // fused schedules may use: as many as fit, a schedule that needs more is packed level by level), the rest read from L2;
    // slot indices of the images 32 bits wide.  The first is taken while it leaves the dense
    // tail the interval asks for AND >= kFtMinStage bytes to stage the factor images (an image that is not staged is solved
    // from L2 at several times the cost); RELP_FT_BIG = 0 / 1 forces one of them.
    const int64_t eta_cap = std::max<int64_t>((int64_t)2 * lay_.m + 64, 1024);   // (one eta never exceeds m entries)
    constexpr int64_t kFtMinStage = 64 * 1024;
    const int force_big = sw_.ft_big;
    auto plan = [&](int32_t tier, int32_t rhs_cap, int64_t min_stage, int32_t min_tcap = 16) {
        for (int32_t tcap : {64, 48, 32, 16}) {
            if (tcap != 16 && tcap - 16 >= want) continue;              // a smaller tail serves the interval
            if (tcap < std::min(want, min_tcap)) return false;          // (a refactorisation every 16 pivots is the last resort)
            if (tcap < want && min_stage > 4096) return false;          // (only the last resort shortens the interval)
            if ((int64_t)ft_lds_base_bytes(lay_.m, tcap, (int32_t)eta_cap, tier, rhs_cap) + min_stage <= kFtLdsBudget) {
                ft_tcap_ = tcap; ft_eta_cap_ = (int32_t)eta_cap; ft_tier_ = tier; ft_big_ = tier >= 1; ft_rhs_cap_ = rhs_cap; ft_ = true;
                return true;
            }
        }
        return false;
    };
    // (16-bit slot indices: m + 1 + copies < 8,192)
    const int32_t small_rhs = (int32_t)std::max<int64_t>(0, std::min<int64_t>(lay_.m, (int64_t(1) << kEllLgShift) - 2 - lay_.m));
    // (measured on GREENBEB, m = 2,228: all-in-LDS with a 32-slot tail and nothing staged 209,000 clocks per pivot, big with a
    // 48-slot tail and 78 KB of staging 235,000 -- what the big layout reads from L2 costs more than staging saves; so the
    // all-in-LDS layout is taken whenever it fits at all)
    // Layout 2 (nothing per row in LDS, x and -pi in L2) takes whatever the other two cannot hold: any m, every right-hand-side
    // copy the fused schedules ask for, the whole LDS minus the dense tail as the staging area.  RELP_FT_BIG = 2 forces it.
    // (the 16-bit row indices of the PRICE copy end at 32,767; the slot indices of the images at 2^24)
    const bool fits_tier1 = lay_.m < kPriceLongFlag;
    const bool fits_tier2 = 2 * (int64_t)lay_.m + 2 <= (int64_t(1) << kEllLgShiftWide);
    if (force_big < 1 && lay_.m < kPriceLongFlag && small_rhs > 0 && plan(0, small_rhs, 4096, force_big == 0 ? 16 : 32)) {}
    else if (force_big != 0 && force_big != 2 && fits_tier1 &&
             (plan(1, lay_.m, kFtMinStage) || plan(1, std::min(lay_.m, 2048), 32 * 1024) || plan(1, std::min(lay_.m, 1024), 8 * 1024) || plan(1, 0, 4096))) {}
    // (layout 2 by default refactorises every 64 updates and lets the kernel make 16 of them while the host factorises: at
    // 64,000 rows a refactorisation is 5 ms of host time against 0.35 ms per pivot, and a pending update costs a pivot whose
    // per-row loops dominate next to nothing -- measured 2,670 it/s at 48 / 8, 2,870 at 64 / 8, 2,975 at 64 / 16)
    else if (force_big != 0 && force_big != 1 && fits_tier2 && ((want = cfg_.update_block < 0 ? 64 : want), plan(2, lay_.m, kFtMinStage))) {}
    if (!ft_) return RELP_OK;
    if (sw_.debug)
        std::fprintf(stderr, "[relp] persistent pivot kernel: m %d, layout %s, %d right-hand-side copies, dense tail %d, LDS base %zu bytes\n",
                     lay_.m, ft_tier_ >= 2 ? "nothing per row in LDS" : ft_big_ ? "big" : "all-in-LDS", ft_rhs_cap_, ft_tcap_,
                     ft_lds_base_bytes(lay_.m, ft_tcap_, ft_eta_cap_, ft_tier_, ft_rhs_cap_));
    const int64_t tc = ft_tcap_, ldt = tc + 1, m = lay_.m, nwp = kFtWaves + 1, eta = ft_eta_cap_;
    const bool t1 = ft_tier_ >= 1, t2 = ft_tier_ >= 2;
    fts_ = FtState{};
    Carver c;
    // (what a refactorisation clears to 0 first, then what it clears to -1, then the rest: two memsets per reset)
    const int64_t o_zero = c.take(&fts_.hdr, 16);
    c.take(&fts_.slot_pivot, 4 * tc); c.take(&fts_.slot_live, 4 * tc); c.take(&fts_.TC, 8 * tc * ldt);
    c.take(&fts_.eta_off, 4 * tc * nwp); c.take(&fts_.spk_off, 4 * tc * nwp);
    const int64_t o_ones = c.take(&fts_.slot_prev, 4 * tc);
    c.take(&fts_.tslot, 4 * m);
    const int64_t o_rest = c.take(&fts_.eta_idx, 4 * eta);
    c.take(&fts_.eta_val, 8 * eta); c.take(&fts_.spk_idx, 4 * tc * m); c.take(&fts_.spk_val, 8 * tc * m); c.take(&fts_.spike, 8 * m);
    c.take(&fts_.prof, 8 * 32); c.take(&fts_.journal, 8 * tc); c.take(&fts_.sp_work, 8 * m);
    c.take_if(t2, &fts_.x_work, 8 * (m + 1 + ft_rhs_cap_));
    c.take_if(t1, &fts_.chunk_mask, 8 * ((m + 63) / 64 + 1)); c.take_if(t1, &fts_.nz_idx, 4 * m); c.take_if(t1, &fts_.nz_val, 8 * m);
    c.take_if(t2, &fts_.rho_idx, 4 * m);
    c.take(&fts_.nzc, 16);
    c.take_if(t2, &fts_.bits_save, kFtBitmapBytes + 1024);
    ft_zero_bytes_ = o_ones - o_zero; ft_ones_bytes_ = o_rest - o_ones;
    HIP_TRY(d_ft_buf_.alloc_raw((size_t)c.size()));
    HIP_TRY(d_ft_buf_.zero(d_ft_buf_.count(), stream_));
    c.bind(d_ft_buf_);
    HIP_TRY(h_ft_hdr_.alloc(4 * sizeof(int32_t)));
    std::memset(h_ft_hdr_, 0, 4 * sizeof(int32_t));
    {   // the kernel's report in mapped host memory; without it (allocation refused) the copies below do the same job
        if (h_mirror_.alloc(sizeof(FtMirror) + sizeof(int32_t) * (size_t)lay_.m, true) == hipSuccess) std::memset(h_mirror_, 0, sizeof(FtMirror));
        else (void)hipGetLastError();
    }
    fts_.m = lay_.m; fts_.tcap = ft_tcap_; fts_.ldt = (int32_t)ldt; fts_.eta_cap = ft_eta_cap_;
    {   // (pb.alpha / pb.rho unknown, no bitmaps saved yet)
        const int32_t reset[4] = {-1, -1, 0, 0};
        HIP_TRY(upload_to(fts_.nzc, reset, 4, stream_));
    }
    fts_.big = ft_tier_; fts_.rhs_cap = ft_rhs_cap_;
    {   // hyper-sparse starts: L and L' by default (U' starts from the leaving pivot's level anyway; on U the spike reaches the first groups: measured 31.4 of 31.4 passes on 25FV47, not worth the reduction); RELP_FT_HYPER = bit mask
        fts_.hyper = sw_.ft_hyper;
        hyper_forced_ = sw_.ft_hyper_set;
    }
    // refactor when this many updates are pending (lower_upper/mod.rs:199-202 refactors when updates.len() > 10, i.e.
    // relp_config_t.update_block = 11 reproduces the reference's cadence)
    fts_.max_updates = cfg_.update_block < 0 ? ft_tcap_ : std::max(1, std::min(cfg_.update_block, ft_tcap_));
    block_ = fts_.max_updates;
    {   // RELP_FT_GRID_PRICE = 0 / 1 forces the choice (any layout: -pi is current in global memory between launches)
        ft_grid_price_ = sw_.ft_grid_price >= 0 ? sw_.ft_grid_price != 0 : (ft_tier_ >= 2 && nr_columns() >= 32768);
    }
    return ft_build_price_ell();
}

// One table pair of the PRICE copy with elements of type T, from the row indices or the values of the CSC columns: slot k of
// column p at [k * ns + p] (the first kPriceSlots entries of every column), and the long columns once more, complete, at
// [k * n_long + i].  Padding slots are 0.
template <class T, class S>
static void price_tables(const std::vector<int64_t>& ptr, const std::vector<S>& src, const std::vector<int32_t>& longs,
                         std::vector<T>* tab, std::vector<T>* ltab) {
    const int64_t n = (int64_t)ptr.size() - 1, ns = std::max<int64_t>(n, 1), nl = std::max<int64_t>((int64_t)longs.size(), 1);
    tab->assign((size_t)kPriceSlots * ns, T(0));
    ltab->assign((size_t)kPriceLongSlots * nl, T(0));
    for (int64_t p = 0; p < n; ++p)
        for (int64_t k = 0; k < std::min<int64_t>(ptr[p + 1] - ptr[p], kPriceSlots); ++k) (*tab)[(size_t)(k * ns + p)] = (T)src[ptr[p] + k];
    for (size_t i = 0; i < longs.size(); ++i) {
        const int32_t p = longs[i];
        for (int64_t k = 0; k < ptr[p + 1] - ptr[p]; ++k) (*ltab)[(size_t)(k * nl) + i] = (T)src[ptr[p] + k];
    }
}

// k-major PRICE copy of the structural columns (relp_kernels.h: PriceEll; rebuilt when rows are removed)
relp_status_t Engine::ft_build_price_ell() {
    std::vector<int32_t> longs, very_long, more;           // columns beyond kPriceSlots entries: up to kPriceLongSlots, beyond, both
    for (int32_t p = 0; p < lay_.nr_normal; ++p) {
        const int64_t n = hc_ptr_[p + 1] - hc_ptr_[p];
        if (n <= kPriceSlots) continue;
        more.push_back(p);
        (n > kPriceLongSlots ? very_long : longs).push_back(p);
    }
    std::vector<uint16_t> long_of((size_t)std::max(lay_.nr_normal, 1), 0xFFFF);
    if (longs.size() < 0xFFFF) for (size_t i = 0; i < longs.size(); ++i) long_of[longs[i]] = (uint16_t)i;
    std::vector<double> val, lval;
    std::vector<uint16_t> idx, lidx;
    std::vector<uint32_t> idx32, lidx32;
    price_tables(hc_ptr_, hc_val_, longs, &val, &lval);
    price_tables(hc_ptr_, hc_idx_, longs, &idx, &lidx);
    for (int32_t p : more) idx[p] |= kPriceLongFlag;
    pe_ = PriceEll{};
    Packer<VectorStore> pk(VectorStore{}, 1);
    pk.put(&pe_.val, val); pk.put(&pe_.lval, lval);
    pk.put(&pe_.idx, idx); pk.put(&pe_.lidx, lidx);
    pk.put(&pe_.long_cols, longs); pk.put(&pe_.very_long, very_long);
    pk.put(&pe_.long_of, long_of);
    if (ft_tier_ >= 2) {                                   // the same two tables with 32-bit row indices (bit 31 = long column)
        price_tables(hc_ptr_, hc_idx_, longs, &idx32, &lidx32);
        for (int32_t p : more) idx32[p] |= kPriceLongFlag32;
        pk.put(&pe_.idx32, idx32); pk.put(&pe_.lidx32, lidx32);
    }
    pe_.n_long = (int32_t)longs.size(); pe_.n_very_long = (int32_t)very_long.size();
    HIP_TRY(d_pe_buf_.alloc_raw((size_t)pk.size()));       // (frees the copy of before a row removal)
    HIP_TRY(d_pe_buf_.upload(pk.data(), pk.size(), stream_));
    pk.bind(d_pe_buf_);
    return RELP_OK;
}

// empty update file: t = 0, every pivot "never updated", TC = 0 (after a refactorisation)
relp_status_t Engine::ft_reset() {
    HIP_TRY(fill_bytes_at(fts_.hdr, 0, (size_t)ft_zero_bytes_, stream_));                  // hdr, slot_pivot, slot_live, TC, offsets
    HIP_TRY(fill_bytes_at(fts_.slot_prev, 0xFF, (size_t)ft_ones_bytes_, stream_));         // slot_prev, tslot: -1
    ft_need_refactor_ = false;
    return RELP_OK;
}

// `with_record`: the pivot record comes down under the same wait
relp_status_t Engine::ft_read_hdr(bool with_record) {
    const hipError_t rec = with_record ? d_rec_.download(h_rec_, 1, enqueue_only(stream_)) : hipSuccess;
    HIP_TRY(first_error(rec, download_from(static_cast<int32_t*>(h_ft_hdr_), fts_.hdr, 4, stream_)));
    since_flush_ = h_ft_hdr_[0];
    ft_need_refactor_ = h_ft_hdr_[2] != 0;
    return RELP_OK;
}

// After a k_ft_run launch: record, header and (mirror only) the basis on the host.  Synchronises the stream.
relp_status_t Engine::ft_read_report(bool* have_basis) {
    if (have_basis) *have_basis = false;
    if (!h_mirror_) return ft_read_hdr(true);
    HIP_TRY(hipStreamSynchronize(stream_));                // the kernel has written its report into the mirror
    *h_rec_ = h_mirror_->rec;
    std::memcpy(h_ft_hdr_, h_mirror_->hdr, 4 * sizeof(int32_t));
    // Hyper-sparse starts pay when they skip more passes than the scan for the first group costs (~1,500 clocks = 2 passes):
    // a schedule whose sweeps saved less in this launch starts at the front in the next ones, and is probed again later.
    if (!hyper_forced_ && ft_big_) {
        for (int k : {0, 3}) {
            const int32_t sw = h_mirror_->sweeps[k];
            if (sw <= 0) continue;
            if ((fts_.hyper >> k) & 1) {
                if ((double)(h_mirror_->whole[k] - h_mirror_->walked[k]) < 2.0 * sw) { fts_.hyper &= ~(1 << k); hyper_probe_in_[k] = 64; }
            } else if (--hyper_probe_in_[k] <= 0) {
                fts_.hyper |= 1 << k;
            }
        }
    }
    since_flush_ = h_ft_hdr_[0];
    ft_need_refactor_ = h_ft_hdr_[2] != 0;
    if (have_basis) {
        std::memcpy(h_basis_, h_mirror_->basis, sizeof(int32_t) * (size_t)lay_.m);     // (the next launch rewrites the mirror)
        *have_basis = true;
    }
    return RELP_OK;
}

// Pivots of the persistent kernel on `go`: one launch that runs until something stops it, or -- Dantzig's rule over very many
// columns (ft_grid_price_) -- PRICE as a grid launch (every CU instead of one) followed by ONE pivot of the persistent kernel with
// the column the grid chose, as many times as the update file has room, enqueued without a synchronisation (a launch whose
// record says "decided" returns at once), plus one launch that only marks the refactorisation due.  The launches of a batch
// share the journal (hdr[3]) and honour each other's "refactorisation due" (hdr[2]); only the last one writes the host mirror.
void Engine::ft_enqueue_pivots(const FtState& go, int rule, int64_t left) {
    if (!(ft_grid_price_ && rule == RELP_RULE_STEEPEST_DESCENT)) {
        launch_ft_run(dlu_, go, ft_problem(rule), left, stream_);
        return;
    }
    const int64_t room = std::max<int64_t>((int64_t)go.max_updates - since_flush_, 0);
    const int64_t batch = std::min<int64_t>(left, room + 1);
    (void)fill_bytes_at(fts_.hdr + 2, 0, 2 * sizeof(int32_t), enqueue_only(stream_));    // (no host side; the launches below follow it on the stream)
    FtProblem pb = ft_problem(rule);
    pb.external_price = 1;
    const ColumnTable ct = table();
    const SelectPartials sp = lu_partials(rule);
    const int nb_struct = sp.nb_struct, nb_virt = price_virtual_blocks(ct);
    for (int64_t k = 0; k < batch; ++k) {
        if (nb_struct > 0 && nb_virt > 0) {
            launch_price_csc_all(csc(), ct, d_minus_pi_, d_d_, lay_.nr_normal, phase_, sp, nb_virt, d_rec_, stream_);
        } else {
            launch_price_csc(csc(), ct, d_minus_pi_, d_d_, 0, lay_.nr_normal, phase_, sp, d_rec_, stream_);
            SelectPartials spv = sp;
            spv.offset = nb_struct;
            launch_price_virtual_sel(ct, d_minus_pi_, d_d_, phase_, spv, d_rec_, stream_);
        }
        launch_select_partials_csc(sp, nb_struct + nb_virt, d_d_, csc(), ct, lay_.m, nullptr, d_rec_, stream_);
        pb.mirror = k + 1 == batch ? h_mirror_.device() : nullptr;
        launch_ft_run(dlu_, go, pb, 1, stream_);
    }
}

FtProblem Engine::ft_problem(int rule) const {
    FtProblem pb{};
    pb.csc = csc(); pb.ct = table(); pb.pe = pe_;
    pb.minus_pi = d_minus_pi_; pb.b = d_b_; pb.alpha = d_alpha_; pb.rho = d_rho_; pb.d = d_d_;
    pb.basis = d_basis_; pb.in_basis = d_in_basis_; pb.trace = d_trace_; pb.trace_cap = trace_cap_;
    pb.rec = d_rec_;
    pb.mirror = h_mirror_.device();
    pb.tol = tolerances();
    pb.rule = rule; pb.n = nr_columns(); pb.phase = phase_;
    return pb;
}

// phase_one::primal / phase_two::primal with the pivots themselves on the device: one launch runs until the outcome is
// decided, the iteration budget is spent or the update file is full (then: refactorise on the host, launch again)
relp_status_t Engine::run_ft(int64_t max_iters, int64_t* done, int32_t* outcome) {
    relp_status_t st = download_rec();
    if (st) return st;
    // (layout 2 keeps lists of where alpha and rho are not zero and rewrites those places only; whatever ran since the last call --
    // step-wise API, phase switch, warm start -- may have written the two vectors: the first pivot rewrites them densely)
    if (ft_tier_ >= 2) HIP_TRY(fill_bytes_at(fts_.nzc, 0xFF, 2 * sizeof(int32_t), stream_));
    const long long start = h_rec_->iterations;
    const int rule = current_rule();
    struct Tick { int64_t& t; ~Tick() { ++t; } };
    // Look-ahead refactorisation (lu_refactor_lookahead): the kernel returns `la` updates before the file is full, and fills
    // the rest while the host factorises.  On for refactorisation intervals from 24 on; RELP_LU_LOOKAHEAD = 0 switches it off.
    const int32_t la_env = luf_enabled_ ? 0 : (ft_tier_ >= 2 && !sw_.lu_lookahead_set) ? 16 : sw_.lu_lookahead;     // (RELP_LU_LOOKAHEAD, read at create; the device
                                                                     // factorisation is synchronous on the engine's stream)
    const int32_t la = (fts_.max_updates >= 24 && la_env > 0) ? std::min(la_env, fts_.max_updates / 3) : 0;
    // Short intervals (the reference's cadence of 11: too short for the look-ahead above, which needs its updates inside the interval):
    // RELP_LU_PIPELINE_SHORT=1 lets the kernel return at the interval, pivot on into the REST of the dense tail (up to twice the
    // interval) while the host factorises, and replays those pivots onto the new factors -- the factors lag one interval behind, the
    // pivots are the same, the device never waits for a whole factorisation.  Opt-in: a measurement (bench: reference cadence).
    const bool pipeline_short = sw_.lu_pipeline_short && la == 0 && !luf_enabled_ && la_env > 0 && fts_.max_updates < 24 && 2 * fts_.max_updates <= ft_tcap_;
    bool have_basis = false;                               // h_basis_ holds the basis as the last launch left it
    while (h_rec_->outcome == DEV_RUNNING && h_rec_->iterations - start < max_iters) {
        if (ft_need_refactor_) {
            const bool ahead = (la > 0 && h_ft_hdr_[2] == 1 && h_ft_hdr_[0] == fts_.max_updates - la) ||
                               (pipeline_short && h_ft_hdr_[2] == 1 && h_ft_hdr_[0] >= fts_.max_updates && h_ft_hdr_[0] < 2 * fts_.max_updates);
            prof_tick_ = 0;                                // refactorisations are always bracketed (like the flush)
            if (ahead) {
                lu_pipeline_cap_ = pipeline_short ? 2 * fts_.max_updates : 0;
                if ((st = lu_refactor_lookahead(rule, max_iters - (h_rec_->iterations - start), have_basis))) return st;
                have_basis = false;                        // (the relaunched kernel has changed the basis since)
                if (ft_need_refactor_ || h_rec_->outcome != DEV_RUNNING) continue;      // (re-examined at the loop head)
            } else {
                prof_begin(RELP_K_FLUSH);
                st = lu_refactor();
                prof_end();
                if (st) return st;
            }
            if (h_rec_->iterations - start >= max_iters) break;
        }
        prof_tick_ = 0;
        prof_begin(RELP_K_FT_RUN);
        FtState go = fts_;
        go.max_updates = fts_.max_updates - la;
        const int64_t left = max_iters - (h_rec_->iterations - start);
        ft_enqueue_pivots(go, rule, left);
        prof_end();
        if ((st = ft_read_report(&have_basis))) return st;
        if (!ft_need_refactor_ && h_rec_->outcome == DEV_RUNNING && h_rec_->iterations - start < max_iters)
            return fail(RELP_E_STATE, "the pivot kernel stopped without a reason");
    }
    if (hipGetLastError() != hipSuccess) return fail(RELP_E_HIP, "kernel launch failed");
    int32_t oc = RELP_RUNNING;
    if ((st = outcome_of_record(&oc))) return st;
    if (done) *done = h_rec_->iterations - start;
    if (outcome) *outcome = oc;
    return RELP_OK;
}

// shader clocks (thread 0 of the persistent kernel) per phase of the pivot, accumulated since create
relp_status_t Engine::lu_phase_cycles(int64_t* out16) {
    if (!lu_ || !ft_) return fail(RELP_E_UNSUPPORTED, "phase clocks are the persistent pivot kernel's");
    if (const relp_status_t st = fetch(out16, fts_.prof, 16 * sizeof(int64_t))) return st;
    if (sw_.debug) {                       // passes walked per sweep of L, U, U', L' against the whole schedule
        int64_t ex[16];
        if (const relp_status_t st = fetch(ex, fts_.prof + 16, sizeof ex)) return st;
        if (ex[15]) std::fprintf(stderr, "[relp] non-zeros per pivot (layout 2): entering column %.1f, eta row %.1f, spike %.1f\n",
                                 (double)ex[12] / ex[15], (double)ex[13] / ex[15], (double)ex[14] / ex[15]);
        static const char* nm[4] = {"L", "U", "U'", "L'"};
        for (int k = 0; k < 4; ++k)
            if (ex[4 + k]) std::fprintf(stderr, "[relp] %s: %lld sweeps, %.1f passes walked of %.1f on average\n", nm[k], (long long)ex[4 + k],
                                        (double)ex[k] / ex[4 + k], (double)ex[8 + k] / ex[4 + k]);
    }
    return RELP_OK;
}

relp_status_t Engine::lu_stats(int64_t* out8) const {
    if (!lu_) return RELP_E_STATE;
    out8[0] = lu_refactors_; out8[1] = hlu_.m; out8[2] = hlu_.nnz_l; out8[3] = hlu_.nnz_u;
    out8[4] = (int64_t)hlu_.Lf.level_ptr.size() - 1; out8[5] = (int64_t)hlu_.Uf.level_ptr.size() - 1;
    out8[6] = (int64_t)hlu_.Ub.level_ptr.size() - 1; out8[7] = (int64_t)hlu_.Lb.level_ptr.size() - 1;
    return RELP_OK;
}

relp_status_t Engine::lu_kernel_layout(int32_t* out4) const {
    if (!lu_) return RELP_E_STATE;
    out4[0] = ft_ ? 1 : 0; out4[1] = ft_ ? ft_tier_ : -1; out4[2] = ft_ ? ft_tcap_ : 0; out4[3] = (ft_ && ft_grid_price_) ? 1 : 0;
    return RELP_OK;
}

relp_status_t Engine::lu_lookahead_stats(int64_t* out4) const {
    if (!lu_) return RELP_E_STATE;
    out4[0] = lu_lookahead_installs_; out4[1] = lu_replayed_changes_; out4[2] = (ft_tier_ >= 2 && !sw_.lu_lookahead_set) ? 16 : sw_.lu_lookahead; out4[3] = sw_.fuse_lanes;
    return RELP_OK;
}

// the PRICE partials of the CSC kernels: 256 columns per slot, the structural blocks in front of the virtual ones
SelectPartials Engine::lu_partials(int rule) const {
    SelectPartials sp = tab_partials(rule);
    sp.nb_struct = price_csc_blocks(0, lay_.nr_normal); sp.cols_per_slot = 256;
    return sp;
}

void Engine::lu_btran(int32_t row, const double* rhs, double* out) {
    if (ft_) launch_ft_btran(dlu_, fts_, ft_problem(0), row, rhs, out, stream_);
    else launch_lu_btran(dlu_, deferred(), rhs, row, out, d_lu_scratch_, nullptr, stream_);
}

// (the product form's FTRAN leaves the pending W to the caller: launch_apply_w; `rec` is its alone)
void Engine::lu_ftran(const double* rhs, double* out, const PivotRecord* rec) {
    if (ft_) launch_ft_ftran(dlu_, fts_, ft_problem(0), -1, rhs, out, stream_);
    else launch_lu_ftran(dlu_, rhs, out, d_lu_scratch_, rec, stream_);
}

// One pivot of the LU engine: CSC PRICE -> select + scatter a_q -> FTRAN (L, U solves) -> W correction
// -> ratio test -> W update -> BTRAN for the pivot row -> b, -pi, basis.
void Engine::enqueue_iteration_lu(int rule) {
    const ColumnTable ct = table();
    const DeferredUpdate du = deferred();
    const SelectPartials sp = lu_partials(rule);
    const int nb_struct = sp.nb_struct, nb_virt = price_virtual_blocks(ct);
    prof_begin(RELP_K_PRICE);
    if (nb_struct > 0 && nb_virt > 0) {
        launch_price_csc_all(csc(), ct, d_minus_pi_, d_d_, lay_.nr_normal, phase_, sp, nb_virt, d_rec_, stream_);
    } else {
        launch_price_csc(csc(), ct, d_minus_pi_, d_d_, 0, lay_.nr_normal, phase_, sp, d_rec_, stream_);
        SelectPartials spv = sp;
        spv.offset = nb_struct;
        launch_price_virtual_sel(ct, d_minus_pi_, d_d_, phase_, spv, d_rec_, stream_);
    }
    prof_end();
    prof_begin(RELP_K_SELECT_COLUMN);
    launch_select_partials_csc(sp, nb_struct + nb_virt, d_d_, csc(), ct, lay_.m, d_aq_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_FTRAN);
    launch_lu_ftran(dlu_, d_aq_, d_v_, d_lu_scratch_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_APPLY_W);
    launch_apply_w_rmin(du, lay_.m, d_v_, d_alpha_, d_b_, tolerances(), d_rmin_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_RATIO);
    launch_ratio_rows(d_alpha_, d_b_, d_basis_, lay_.m, tolerances(), du, d_rmin_, 256, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_UPDATE_W);
    launch_update_w(du, lay_.m, d_alpha_, d_rec_, stream_);
    prof_end();
    prof_begin(RELP_K_UPDATE_VECTORS);
    launch_lu_btran(dlu_, du, nullptr, -1, d_rho_, d_lu_scratch_, d_rec_, stream_);
    launch_update_vectors(lay_.m, d_alpha_, d_rho_, d_b_, d_minus_pi_, d_basis_, d_in_basis_, d_trace_, trace_cap_, d_rec_,
                          stream_);
    prof_end();
    if (++since_flush_ >= block_) enqueue_flush();
}

}  // namespace relp
