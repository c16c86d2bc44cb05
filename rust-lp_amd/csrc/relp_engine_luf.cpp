// relp_engine_luf.cpp -- Engine: the refactorisation of the LU engine ON THE DEVICE (relp_lu_factor_core.h).
// What stays on the host is what is static: the row-major copy of the provider matrix the kernel enumerates basis rows
// from (built at create, after a row removal and at the phase switch), and the buffers.
#include "relp_engine_internal.hpp"
#include "relp_lu_factor_core.h"
#include "relp_lu_image.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace relp {

struct Engine::LufState {
    DeviceBuf<char> d_buf;
    LufMatrix M{}; LufWork W{}; LufOut O{};
    int32_t cap = 0, nb_cap = 0;
    bool dirty = true;
    int32_t key[4] = {-1, -1, -1, -1};                         // (m, artificial columns, phase, wrapped artificials) the tables were built for
    LufSchedWork SW[4]; LufSchedIn sin[4]; LufSchedOut sout[4];   // the schedules (relp_lu_schedule_core.h), one work set each
    int32_t x_cap = 0, pool_cap = 0;
    FtPivotInfo* pinfo = nullptr;
    int64_t img_cap = 0;
    bool resident = false;                                       // hlu_ does not hold the rows of the factors in use (they are on the device)
};

void Engine::luf_release() { delete luf_; luf_ = nullptr; }

// static tables + workspace for the current shape of the problem (rows may have been removed, the phase may have changed)
relp_status_t Engine::luf_prepare() {
    if (!luf_) luf_ = new LufState();
    LufState& S = *luf_;
    S.d_buf.reset();
    const int32_t m = lay_.m, nprov = lay_.n_provider, na = lay_.nr_artificial;
    // row-major copy of the provider columns (structural incl. bound rows, virtual), in column order
    std::vector<int32_t> rcount(m + 1, 0);
    auto each = [&](auto f) {
        for (int32_t p = 0; p < nprov; ++p) lay_.for_each_provider_entry(p, csc_column(), [&](int32_t i, double v) { f(i, p, v); });
    };
    int64_t nnz = 0;
    each([&](int32_t i, int32_t, double) { ++rcount[i + 1]; ++nnz; });
    for (int32_t i = 0; i < m; ++i) rcount[i + 1] += rcount[i];
    std::vector<int32_t> rcol((size_t)nnz), fill(rcount.begin(), rcount.end() - 1), art_of_row(m, -1);
    std::vector<double> rval((size_t)nnz);
    each([&](int32_t i, int32_t p, double v) { const int32_t o = fill[i]++; rcol[o] = p; rval[o] = v; });
    for (int32_t a = 0; a < na; ++a) art_of_row[lay_.column_to_row[a]] = a;
    // sizes: the bump is eliminated on sparse rows in an arena; RELP_LUF_BUMP_CAP bounds its rows (default: any), a bump or a
    // fill-in beyond the arrays falls back to the host
    S.nb_cap = std::min<int32_t>(m, sw_.luf_bump_cap);
    // (a small dense bump may fill in completely)
    const int64_t arena_cap = std::min<int64_t>(INT32_MAX / 4, 3 * (nnz + (int64_t)lay_.wrapped_na + na + m) + 64 * (int64_t)S.nb_cap + 1024 +
                                                                  4 * std::min<int64_t>((int64_t)S.nb_cap * S.nb_cap, int64_t(1) << 21));
    S.cap = (int32_t)arena_cap;
    const int32_t nt = luf_threads();
    const int64_t R = m, NB = S.nb_cap, NB8 = std::max(S.nb_cap, 512), AC = arena_cap;
    // the schedules: one set of work arrays, one image arena, lists and descriptors per schedule (four workgroups build them side by side)
    const int32_t nlev_cap = m + 1;
    S.x_cap = (int32_t)std::min<int64_t>(INT32_MAX / 8, 4 * (int64_t)S.cap / 3 + 2 * (int64_t)m + 64);       // expanded rows of the fused groups
    S.pool_cap = (int32_t)std::min<int64_t>(INT32_MAX / 8, 2 * (int64_t)S.x_cap);
    S.img_cap = 64 + 40 * ((int64_t)S.x_cap + 2 * (int64_t)m + 64) + 16 * ((int64_t)m + 8);
    const int64_t n_words = m / 32 + 3, LV = (int64_t)nlev_cap + 2, XC = S.x_cap, PC = S.pool_cap;
    const bool bits = ft_tier_ >= 2;
    S.M = LufMatrix{}; S.W = LufWork{}; S.O = LufOut{};
    LufMatrix& A = S.M; LufWork& W = S.W; LufOut& O = S.O;
    Carver c(16);                                          // (every piece at least 16 bytes)
    const int64_t o_rptr = c.take(&A.rptr, 4 * (R + 1)), o_rcol = c.take(&A.rcol, 4 * nnz), o_rval = c.take(&A.rval, 8 * nnz),
                  o_art = c.take(&A.art_of_row, 4 * R), o_wr = c.take(&A.wrapped_row, 4 * (int64_t)std::max<int32_t>(lay_.wrapped_na, 1));
    c.take(&W.pos_p, 4 * ((int64_t)nprov + 1)); c.take(&W.pos_a, 4 * ((int64_t)na + 1));
    c.take(&W.wrow_pos, 4 * R); c.take(&W.rcount, 4 * R); c.take(&W.ccount, 4 * R); c.take(&W.claim, 4 * R); c.take(&W.claim2, 4 * R);
    c.take(&W.list, 4 * R); c.take(&W.list2, 4 * R); c.take(&W.piv, 4 * R); c.take(&W.brow, 4 * R); c.take(&W.bcol, 4 * R);
    c.take(&W.lrow, 4 * R); c.take(&W.lcol, 4 * R); c.take(4 * R);      // (+ one spare)
    c.take(&W.part, 4 * ((int64_t)nt + 2));
    c.take(&W.rbeg, 4 * NB); c.take(&W.rlen, 4 * NB); c.take(&W.rcap, 4 * NB); c.take(&W.ract, 4 * NB); c.take(&W.cact, 4 * NB); c.take(&W.bcc, 4 * NB);
    c.take(&W.bstep_row, 4 * NB); c.take(&W.bstep_col, 4 * NB); c.take(&W.cpiv, 4 * NB); c.take(&W.prank, 4 * NB); c.take(&W.acc, 4 * NB);
    // (>= 512 words each: the dense finish keeps 8 x 64 partials there)
    c.take(&W.pval, 8 * NB8); c.take(&W.cmax, 8 * NB8); c.take(&W.rowmark, 8 * NB8); c.take(&W.colbest, 8 * NB8); c.take(&W.cprio, 8 * NB8);
    c.take(&W.ecol, 4 * AC); c.take(&W.eval, 8 * AC);
    c.take(&W.lt_row, 4 * AC); c.take(&W.lt_step, 4 * AC); c.take(&W.lt_val, 8 * AC); c.take(&W.lt_ptr, 4 * (NB + 1)); c.take(&W.lt_ord, 4 * AC);
    c.take(&W.counters, 512); c.take(&W.red, 8 * 8); c.take(&W.scalars, 64);
    c.take(&W.dense, 8 * (int64_t)64 * 64); c.take(&W.dint, 4 * 8 * 64);
    c.take(&W.ut_row, 4 * AC); c.take(&W.ut_col, 4 * AC); c.take(&W.ut_val, 8 * AC); c.take(&W.vw, 4 * (R + 2)); c.take(&W.vtmp, 4 * AC);
    c.take(&O.status, 32); c.take(&O.rowperm, 4 * R); c.take(&O.colperm, 4 * R); c.take(&O.row_step, 4 * R); c.take(&O.col_step, 4 * R);
    c.take(&O.diag, 8 * R);
    for (LufTriangle* t : {&O.Lf, &O.Uf, &O.Ub, &O.Lb}) { c.take(&t->ptr, 4 * (R + 1)); c.take(&t->idx, 4 * (int64_t)S.cap); c.take(&t->val, 8 * (int64_t)S.cap); }
    for (int q = 0; q < 4; ++q) {
        LufSchedWork& w = S.SW[q];
        LufSchedOut& out = S.sout[q];
        w = LufSchedWork{}; out = LufSchedOut{};
        c.take(&w.indeg, 4 * R); c.take(&w.lev, 4 * R); c.take(&w.order, 4 * R); c.take(&w.grp, 4 * R); c.take(&w.xbeg, 4 * R); c.take(&w.xlen, 4 * R);
        c.take(&w.lg, 4 * R); c.take(&w.loff, 4 * R); c.take(&w.rhs_id, 4 * R); c.take(4 * R);      // (+ one spare)
        c.take(&w.lvl_ptr, 4 * LV); c.take(&w.lvl_grp, 4 * LV); c.take(&w.grp_lvl0, 4 * LV); c.take(&w.grp_lane0, 4 * LV); c.take(&w.grp_pass0, 4 * LV);
        c.take(&w.grp_lanes, 4 * LV);
        c.take(&w.bits0, 4 * n_words); c.take(&w.bits1, 4 * n_words);
        c.take(&w.x_src, 4 * XC); c.take(&w.x_coef, 8 * XC); c.take(&w.x_v0, 4 * XC); c.take(&w.x_vn, 4 * XC);
        c.take(&w.pool, 4 * PC);
        c.take(&w.tmp, 4 * (R + 2)); c.take(&w.tmp2, 4 * (R + 2)); c.take(&w.ovf_off, 4 * (R + 1)); c.take(&w.sc, 128);
        c.take(&out.image, S.img_cap); c.take(&out.desc, 4 * LUF_D_WORDS); c.take(&out.triv, 4 * R); c.take(&out.reach, 4 * R); c.take(&out.level_of, 4 * R);
        c.take(&out.via_ptr, 4 * (R + 1)); c.take(&out.via_pos, 4 * PC); c.take(&out.rhs_src, 4 * R);
        c.take(&out.rhs_pos, 4 * R, bits); c.take(&out.triv_bits, 4 * n_words, bits);
        w.x_cap = S.x_cap; w.pool_cap = S.pool_cap; w.nlev_cap = nlev_cap;
        out.image_cap = S.img_cap; out.via_cap = S.pool_cap;
    }
    c.take(&S.pinfo, (int64_t)sizeof(FtPivotInfo) * R);
    HIP_TRY(S.d_buf.alloc_raw((size_t)c.size()));
    HIP_TRY(S.d_buf.zero(S.d_buf.count(), stream_));
    char* const B = S.d_buf;
    c.bind(B);
    HIP_TRY(upload_to(B + o_rptr, rcount.data(), (size_t)m + 1, stream_));
    HIP_TRY(upload_to(B + o_rcol, rcol.data(), (size_t)nnz, stream_));
    HIP_TRY(upload_to(B + o_rval, rval.data(), (size_t)nnz, stream_));
    HIP_TRY(upload_to(B + o_art, art_of_row.data(), (size_t)m, stream_));
    if (lay_.wrapped_na > 0) HIP_TRY(upload_to(B + o_wr, lay_.column_to_row.data(), (size_t)lay_.wrapped_na, stream_));
    A.m = m; A.na = na; A.n_provider = nprov;
    A.csc = csc(); A.ct = table();
    A.wrapped_na = lay_.wrapped_na;
    W.nb_cap = S.nb_cap;
    W.arena_cap = W.lt_cap = W.vtmp_cap = (int32_t)arena_cap;
    W.dense_cap = sw_.luf_dense;                          // RELP_LUF_DENSE: rows of the dense finish (<= 64; 0 = off)
    O.cap = S.cap;
    {
        const bool wide = ft_big_;
        const LufTriangle* tri4[4] = {&O.Lf, &O.Uf, &O.Ub, &O.Lb};
        const LufTriangle* trt4[4] = {&O.Lb, &O.Ub, &O.Uf, &O.Lf};     // the transposed pattern of each
        // (fused schedules read copies of some right-hand sides behind x: ft_rhs_cap_ words of the layout; RELP_FUSE_LANES, read at create)
        const int32_t fuse = ft_rhs_cap_ > 0 ? sw_.fuse_lanes : 0;
        for (int q = 0; q < 4; ++q) {
            const bool maskable = q == 1 || q == 2;
            S.sin[q] = LufSchedIn{m, tri4[q]->ptr, tri4[q]->idx, tri4[q]->val, trt4[q]->ptr, trt4[q]->idx, maskable ? O.diag : nullptr, maskable ? 1 : 0,
                                  wide ? 1 : 0, wide ? 512 : 0x7fffffff, fuse, ft_rhs_cap_, ft_tier_ >= 2 ? 1 : 0};
        }
    }
    S.dirty = false;
    S.key[0] = lay_.m; S.key[1] = lay_.nr_artificial; S.key[2] = phase_; S.key[3] = lay_.wrapped_na;
    return RELP_OK;
}

// P B Q = L U of the basis in d_basis_ by the device kernel.  `resident`: the second kernel also builds the four solve
// schedules on the device and they are installed where they are (persistent pivot kernel only) -- no factor leaves the device;
// otherwise the factors are downloaded and scheduled like lu_factor's (the product-form fallback of very large bases).
// RELP_E_UNSUPPORTED: the bump exceeds the dense working copy, or an arena is too small (the caller factorises on the host).
relp_status_t Engine::lu_factor_on_device(int32_t* device_status) {
    // (the device factorisation packs its images for layouts 0 and 1 and keeps its working sets in one workgroup's LDS:
    // beyond their row range the host factorises)
    if (ft_tier_ >= 2) return RELP_E_UNSUPPORTED;
    if (!luf_ || luf_->dirty || luf_->key[0] != lay_.m || luf_->key[1] != lay_.nr_artificial || luf_->key[2] != phase_ || luf_->key[3] != lay_.wrapped_na) {
        const relp_status_t st = luf_prepare();            // (a row removal or the phase switch renumbers rows / columns)
        if (st) return st;
    }
    LufState& S = *luf_;
    const bool resident = ft_ && !luf_download_;
    const auto t0 = std::chrono::steady_clock::now();
    S.M.csc = csc(); S.M.ct = table();                  // (pointers may have been re-allocated)
    int32_t status[8] = {0}, desc[4][LUF_D_WORDS] = {};
    // (the bump's working set in LDS when it fits, RELP_LUF_LDS=0 keeps it in L2; an arena that overflows in LDS: once more from L2)
    for (int attempt = sw_.luf_lds ? 0 : 1; attempt < 2; ++attempt) {
        launch_lu_factor(S.M, d_basis_, S.W, S.O, stream_, attempt == 0);
        if (resident) launch_lu_schedules(S.sin, S.SW, S.sout, S.O.status, S.pinfo, stream_);
        // the status and the descriptors under one wait: the last copy is the waiting one
        hipError_t got = download_from(status, S.O.status, 8, resident ? enqueue_only(stream_) : On(stream_));
        for (int q = 0; resident && q < 4; ++q)
            got = first_error(got, download_from(desc[q], S.sout[q].desc, LUF_D_WORDS, q < 3 ? enqueue_only(stream_) : On(stream_)));
        HIP_TRY(got);
        if (!(attempt == 0 && status[0] == LUF_NO_ROOM)) break;
        ++luf_lds_retries_;
    }
    luf_kernel_us_ += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    ++luf_runs_;
    if (sw_.debug && luf_runs_ % 200 == 0) {          // phase clocks of the factorisation kernel (relp_lu_factor_core.h: LUF_LAP)
        int32_t cnt[128] = {0};
        HIP_TRY(download_from(cnt, S.W.counters, 128, stream_));
        const unsigned long long* ph = reinterpret_cast<const unsigned long long*>(cnt + 8);
        static const char* nm[11] = {"maps+counts", "peel", "bump setup", "r:column max", "r:proposals", "r:independence+accept", "r:elimination", "r:leave + dense finish",
                                     "triplets", "row views", "column views"};
        std::fprintf(stderr, "[relp] device factorisation, %lld runs (%d with the bump in LDS, %lld of them again in global memory, dense finish on %.1f rows), %.0f us each (host clock, schedules included), last: %d rounds; clocks per run:",
                     (long long)luf_runs_, cnt[3], (long long)luf_lds_retries_, cnt[3] ? (double)cnt[4] / cnt[3] : 0.0, luf_kernel_us_ / luf_runs_, cnt[2]);
        for (int i = 0; i < 11; ++i) std::fprintf(stderr, " %s %.0f", nm[i], (double)ph[i] / luf_runs_);
        std::fprintf(stderr, "\n");
        if (ph[12 + 5]) std::fprintf(stderr, "[relp]   wave 0 of the elimination: rows %llu, hits %llu, pivot entries %llu; clocks: idle/loop %llu, row setup %llu, hit prologue %llu, entries %llu, write-back %llu\n",
                                     ph[17], ph[18], ph[19], ph[12], ph[13], ph[14], ph[15], ph[16]);
        static const char* sn[4] = {"L", "U", "U'", "L'"};
        for (int q = 0; q < 4 && resident; ++q) {
            int32_t sc[32] = {0};
            HIP_TRY(download_from(sc, S.SW[q].sc, 32, stream_));
            const unsigned long long* sp = reinterpret_cast<const unsigned long long*>(sc + 8);
            std::fprintf(stderr, "[relp]   schedule %s clocks per run: levels %.0f, fusion %.0f, classify + offsets %.0f, image %.0f, via %.0f\n", sn[q],
                         (double)sp[0] / luf_runs_, (double)sp[1] / luf_runs_, (double)sp[2] / luf_runs_, (double)sp[3] / luf_runs_, (double)sp[4] / luf_runs_);
        }
    }
    luf_last_bump_ = status[1]; luf_last_peeled_ = status[2];
    if (device_status) *device_status = status[0];
    if (status[0] == LUF_SINGULAR) return fail(RELP_E_SINGULAR, "singular basis (device factorisation)");
    if (status[0] != LUF_OK) return RELP_E_UNSUPPORTED;      // bump too large / no room: not an error, the host takes over
    if (resident) for (int q = 0; q < 4; ++q) if (desc[q][LUF_D_STATUS] != LUF_OK) return RELP_E_UNSUPPORTED;
    const int32_t m = lay_.m, nl = status[3], nu = status[4];
    hlu_ = LUFactors{};
    hlu_.m = m; hlu_.nnz_l = nl; hlu_.nnz_u = (int64_t)nu + m;
    S.resident = resident;
    if (!resident) return luf_download_factors();
    // install the factors where they are
    dlu_ = DeviceLU{};
    dlu_.m = m; dlu_.rowperm = S.O.rowperm; dlu_.colperm = S.O.colperm;
    dlu_.Uf.idx = S.O.Uf.idx; dlu_.Uf.val = S.O.Uf.val; dlu_.Uf.nnz = nu;
    TriangularSchedule* hs[4] = {&hlu_.Lf, &hlu_.Uf, &hlu_.Ub, &hlu_.Lb};
    DeviceSchedule* ds[4] = {&dlu_.Lf, &dlu_.Uf, &dlu_.Ub, &dlu_.Lb};
    fts_.m = m;
    fts_.inv_rowperm = S.O.row_step; fts_.inv_colperm = S.O.col_step; fts_.task_uf = S.O.row_step; fts_.task_ub = S.O.row_step;
    fts_.lev_ub = S.sout[2].level_of; fts_.pinfo = S.pinfo;
    for (int q = 0; q < 4; ++q) {
        const int32_t* d = desc[q];
        EllSchedule& e = fts_.ell[q];
        e = EllSchedule{};
        ell_image_view(S.sout[q].image, EllImageShape{m, d[LUF_D_PASSES], d[LUF_D_LEVELS], d[LUF_D_LANES], d[LUF_D_OVF], ft_big_}, &e);
        const bool maskable = q == 1 || q == 2;
        e.via_ptr = maskable ? S.sout[q].via_ptr : nullptr; e.via_pos = maskable ? S.sout[q].via_pos : nullptr;
        e.rhs_base = d[LUF_D_USES_RHS] ? m + 1 : 0;
        e.n_triv = d[LUF_D_TRIV]; e.triv = S.sout[q].triv; e.reach = S.sout[q].reach; e.rhs_src = S.sout[q].rhs_src;
        e.n_rhs = ft_big_ ? std::max(d[LUF_D_NRHS], 0) : -1;
        e.rhs_pos = S.sout[q].rhs_pos; e.triv_bits = S.sout[q].triv_bits;
        ds[q]->n_levels = d[LUF_D_LEVELS];
        hs[q]->level_ptr.assign((size_t)d[LUF_D_KAHN_LEVELS] + 1, 0);     // (lu_stats reports the level counts)
    }
    ft_plan_staging(fts_);
    return RELP_OK;
}

// the factors of the last device factorisation -> hlu_ with level schedules, like after lu_factor (relp_lu.cpp)
relp_status_t Engine::luf_download_factors() {
    LufState& S = *luf_;
    const int32_t m = lay_.m, nl = (int32_t)hlu_.nnz_l, nu = (int32_t)(hlu_.nnz_u - m);
    hlu_.rowperm.resize(m); hlu_.colperm.resize(m);
    std::vector<double> diag(m), ones(m, 1.0);
    // every piece under one wait: the last copy (the values of L', or its row pointers when it has no entry) is the waiting one
    hipError_t got = download_from(hlu_.rowperm, S.O.rowperm, enqueue_only(stream_));
    got = first_error(got, download_from(hlu_.colperm, S.O.colperm, enqueue_only(stream_)));
    got = first_error(got, download_from(diag, S.O.diag, enqueue_only(stream_)));
    TriangularSchedule* sch[4] = {&hlu_.Lf, &hlu_.Uf, &hlu_.Ub, &hlu_.Lb};
    const LufTriangle* tri[4] = {&S.O.Lf, &S.O.Uf, &S.O.Ub, &S.O.Lb};
    const int32_t cnt[4] = {nl, nu, nu, nl};
    for (int q = 0; q < 4; ++q) {
        sch[q]->ptr.resize(m + 1); sch[q]->idx.resize(cnt[q]); sch[q]->val.resize(cnt[q]);
        const bool last = q == 3;
        got = first_error(got, download_from(sch[q]->ptr, tri[q]->ptr, last && !cnt[q] ? On(stream_) : enqueue_only(stream_)));
        got = first_error(got, download_from(sch[q]->idx, tri[q]->idx, enqueue_only(stream_)));
        got = first_error(got, download_from(sch[q]->val, tri[q]->val, last ? On(stream_) : enqueue_only(stream_)));
    }
    HIP_TRY(got);
    lu_levels_from_rows(m, ones, true, &hlu_.Lf);
    lu_levels_from_rows(m, diag, false, &hlu_.Uf);
    lu_levels_from_rows(m, diag, true, &hlu_.Ub);
    lu_levels_from_rows(m, ones, false, &hlu_.Lb);
    return RELP_OK;
}

// hlu_ as the host needs it for inspection (relp_lu_get_upper, relp_lu_factor_residual): after a device-resident
// factorisation the rows are still on the device
relp_status_t Engine::lu_host_factors() {
    if (luf_ && luf_->resident && hlu_.Lf.ptr.empty()) return luf_download_factors();
    return RELP_OK;
}

bool Engine::luf_is_resident() const { return luf_ && luf_->resident; }

relp_status_t Engine::lu_set_device_factorisation(bool on) {
    if (!lu_) return fail(RELP_E_UNSUPPORTED, "the device factorisation belongs to the LU engine");
    luf_enabled_ = on;
    return RELP_OK;
}

relp_status_t Engine::luf_stats(int64_t* out6) const {
    if (!lu_) return RELP_E_STATE;
    out6[0] = luf_enabled_ ? 1 : 0; out6[1] = luf_runs_; out6[2] = luf_fallbacks_; out6[3] = (int64_t)luf_kernel_us_;
    out6[4] = luf_last_bump_; out6[5] = luf_last_peeled_;
    return RELP_OK;
}

}  // namespace relp

namespace relp {

// max |P B Q - L U| over all entries, for the factors currently installed (whoever computed them) and the basis they were
// computed for; dense arithmetic on the host, so only for m <= 1,024 (tests: the reference's factorisation cases of
// decomposition/mod.rs:301-491 through the ABI).  *out = -1 when m is larger.
relp_status_t Engine::lu_factor_residual(double* out) {
    if (!lu_) return fail(RELP_E_UNSUPPORTED, "the LU engine's factors");
    *out = -1.0;
    const int32_t m = lay_.m;
    if (m > 1024 || hlu_.m != m) return RELP_OK;
    if (ft_) {                                             // updates pending: the factors are those of an earlier basis
        relp_status_t hs = ft_read_hdr();
        if (hs) return hs;
    }
    if (since_flush_ > 0) return RELP_OK;
    relp_status_t st = lu_host_factors();
    if (st) return st;
    if ((st = lu_download_basis())) return st;
    std::vector<std::vector<std::pair<int32_t, double>>> cols;
    if ((st = lu_basis_columns(cols))) return st;
    std::vector<double> a((size_t)m * m, 0.0), L((size_t)m * m, 0.0), U((size_t)m * m, 0.0);
    for (int32_t c = 0; c < m; ++c) for (auto& e : cols[c]) a[(size_t)e.first * m + c] += e.second;
    for (int32_t k = 0; k < m; ++k) {
        L[(size_t)k * m + k] = 1.0; U[(size_t)k * m + k] = hlu_.Uf.diag[k];
        for (int32_t e = hlu_.Lf.ptr[k]; e < hlu_.Lf.ptr[k + 1]; ++e) L[(size_t)k * m + hlu_.Lf.idx[e]] = hlu_.Lf.val[e];
        for (int32_t e = hlu_.Uf.ptr[k]; e < hlu_.Uf.ptr[k + 1]; ++e) U[(size_t)k * m + hlu_.Uf.idx[e]] = hlu_.Uf.val[e];
    }
    double worst = 0.0;
    for (int32_t k = 0; k < m; ++k)
        for (int32_t l = 0; l < m; ++l) {
            double s = 0.0;
            for (int32_t q = 0; q <= std::min(k, l); ++q) s += L[(size_t)k * m + q] * U[(size_t)q * m + l];
            worst = std::max(worst, std::fabs(s - a[(size_t)hlu_.rowperm[k] * m + hlu_.colperm[l]]));
        }
    *out = worst;
    return RELP_OK;
}

}  // namespace relp
