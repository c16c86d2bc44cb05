// The kernel harness of the in-place cut rows (test infrastructure): one extern "C" entry that runs relp::launch_tab_add_cuts of the
// shipped librelp_engine.so once on whole device IMAGES a test constructs (tests/kernel_harness_cuts.py) and hands every image
// back.  `make -C tests/kernels`
//
// The caller owns the layout: it passes the pitches and every buffer as the image the device shall hold (its own sentinels where
// the launch must not write).  This file only checks that nothing the launch may touch lies outside an image -- a refused call
// (negative code) launches nothing -- uploads, launches, synchronises and downloads.  A HIP error is returned as 1000 + code and is
// sticky for the whole library (harness_common.hpp): nothing is launched any more in this process.

#include "harness_common.hpp"

using namespace relp;

extern "C" {

int rkc_cut_tile() { return kTabCutTile; }

// launch_tab_add_cuts on the view (m rows, owned stored columns [c_lo, c_lo + n_owned) = all up to n_store, tableau columns from
// col_off on) with p pending rows of at most kmax.  Images, in and out: T0 (columns ld_t apart, from column c_lo), W (kmax x ld_b),
// R0 ((kmax + 1) x ld_r, from column c_lo), d and cost_store (by storage column from 0), in_basis (by tableau column), idcol / basis /
// pos_of_row (by row), vrow0 / vrow1 / vsign (by virtual column), A (nr_normal x ld_a), rows (entries, ascending in [0, m); the engine's
// lists are strictly ascending, a repeated row is read twice), coef (entries x count), u (count x kmax).
int rkc_tab_add_cuts(int64_t m, int64_t n_owned, int64_t c_lo, int64_t col_off, int64_t p, int64_t kmax, int64_t batch, int64_t count,
                     int64_t entries, int64_t ld_t, int64_t ld_b, int64_t ld_r, int64_t ld_a, int64_t a_row0, int64_t struct_c0,
                     int64_t nr_normal, int64_t first_virtual,
                     double* T0, int64_t T0_len, double* W, int64_t W_len, double* R0, int64_t R0_len, double* d, int64_t d_len,
                     double* cost_store, int64_t cost_store_len, uint8_t* in_basis, int64_t in_basis_len, int32_t* idcol, int64_t idcol_len,
                     int32_t* basis, int64_t basis_len, int32_t* pos_of_row, int64_t pos_of_row_len, int32_t* vrow0, int64_t vrow0_len,
                     int32_t* vrow1, int64_t vrow1_len, int32_t* vsign, int64_t vsign_len, double* A, int64_t A_len, int32_t* rows,
                     int64_t rows_len, double* coef, int64_t coef_len, double* u, int64_t u_len) {
    if (g_sticky) return g_sticky;
    const int64_t cap = 1 << 20;
    REFUSE_IF(m < 1 || m > cap || n_owned < 1 || n_owned > cap || count < 1 || count > 4096 || entries < 0 || entries > cap, kRefusedShape);
    REFUSE_IF(kmax < 1 || kmax > 128 || p < 0 || p > kmax, kRefusedShape);
    REFUSE_IF(batch != 1 && batch != 8 && batch != 16 && batch != 32, kRefusedBatch);
    const int64_t n_all = c_lo + n_owned, n_tab = n_all - col_off;
    REFUSE_IF(c_lo < 0 || c_lo > cap || col_off < 0 || col_off >= n_all, kRefusedIndex);
    REFUSE_IF(ld_t < m + count || ld_b < m + count || ld_r < n_owned + count || ld_t > 2 * cap || ld_b > 2 * cap || ld_r > 2 * cap, kRefusedShape);
    REFUSE_IF(nr_normal < 0 || nr_normal > cap || struct_c0 < 0 || ld_a < 1 || ld_a > 2 * cap || a_row0 < 0 || a_row0 + count > ld_a, kRefusedIndex);
    REFUSE_IF(first_virtual < 0 || first_virtual > cap, kRefusedIndex);
    REFUSE_IF(T0_len != (n_owned + count) * ld_t || W_len != kmax * ld_b || R0_len != (kmax + 1) * ld_r, kRefusedLength);
    REFUSE_IF(d_len != n_all + count || cost_store_len != n_all + count || in_basis_len != n_tab + count, kRefusedLength);
    REFUSE_IF(idcol_len != m + count || basis_len != m + count || pos_of_row_len != m + count, kRefusedLength);
    REFUSE_IF(vrow0_len != first_virtual + count || vrow1_len != vrow0_len || vsign_len != vrow0_len, kRefusedLength);
    REFUSE_IF(A_len != (nr_normal > 0 ? nr_normal : 1) * ld_a || rows_len != entries || coef_len != entries * count || u_len != count * kmax,
              kRefusedLength);
    for (int64_t e = 0; e < entries; ++e) REFUSE_IF(rows[e] < 0 || rows[e] >= m || (e > 0 && rows[e] < rows[e - 1]), kRefusedIndex);
    for (int64_t j = 0; j < in_basis_len; ++j) REFUSE_IF(in_basis[j] > 2, kRefusedIndex);

    Image<double> iT0(T0, T0_len), iW(W, W_len), iR0(R0, R0_len), id(d, d_len), ic(cost_store, cost_store_len), iA(A, A_len), icoef(coef, coef_len),
        iu(u, u_len);
    Image<uint8_t> iflag(in_basis, in_basis_len);
    Image<int32_t> iid(idcol, idcol_len), ibasis(basis, basis_len), ipos(pos_of_row, pos_of_row_len), iv0(vrow0, vrow0_len), iv1(vrow1, vrow1_len),
        ivs(vsign, vsign_len), irows(rows, rows_len);
    HIP_OK(iT0.up()); HIP_OK(iW.up()); HIP_OK(iR0.up()); HIP_OK(id.up()); HIP_OK(ic.up()); HIP_OK(iA.up()); HIP_OK(icoef.up()); HIP_OK(iu.up());
    HIP_OK(iflag.up()); HIP_OK(iid.up()); HIP_OK(ibasis.up()); HIP_OK(ipos.up()); HIP_OK(iv0.up()); HIP_OK(iv1.up()); HIP_OK(ivs.up());
    HIP_OK(irows.up());

    TableauView tv{};
    tv.T0 = iT0.d - c_lo * ld_t; tv.ld_t = ld_t;
    tv.R0 = iR0.d - c_lo; tv.ld_r = ld_r;
    tv.d = id.d; tv.m = (int32_t)m; tv.n_store = (int32_t)n_all; tv.col_off = (int32_t)col_off; tv.n = (int32_t)n_tab;
    tv.c_lo = (int32_t)c_lo; tv.c_hi = (int32_t)n_all;
    DeferredUpdate du{};
    du.W = iW.d; du.ld = ld_b; du.kmax = (int32_t)kmax; du.pos_of_row = ipos.d; du.batch = (int32_t)batch;
    const CutRows cr{irows.d, icoef.d, (int32_t)entries, (int32_t)count, iA.d, ld_a, (int32_t)a_row0, (int32_t)struct_c0, (int32_t)nr_normal};
    const CutTail ct{ic.d, iflag.d, iid.d, ibasis.d, iv0.d, iv1.d, ivs.d, (int32_t)first_virtual, (int32_t)kmax + 1};
    launch_tab_add_cuts(tv, du, cr, iflag.d, (int32_t)p, iu.d, ct, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());

    HIP_OK(iT0.back()); HIP_OK(iW.back()); HIP_OK(iR0.back()); HIP_OK(id.back()); HIP_OK(ic.back()); HIP_OK(iA.back()); HIP_OK(icoef.back());
    HIP_OK(iu.back()); HIP_OK(iflag.back()); HIP_OK(iid.back()); HIP_OK(ibasis.back()); HIP_OK(ipos.back()); HIP_OK(iv0.back()); HIP_OK(iv1.back());
    HIP_OK(ivs.back()); HIP_OK(irows.back());
    return 0;
}

}  // extern "C"
