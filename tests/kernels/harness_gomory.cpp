// The kernel harness of the Gomory cuts (test infrastructure): one extern "C" entry that runs relp::launch_tab_gomory of the shipped
// librelp_engine.so once on whole device IMAGES a test constructs (tests/kernel_harness_gomory.py) and hands every image back.
// `make -C tests/kernels`
//
// The caller owns the layout: it passes the pitches and every buffer as the image the device shall hold (its own sentinels where
// the launch must not write).  This file only checks that nothing the launch may touch lies outside an image -- a refused call
// (negative code) launches nothing -- uploads, launches, synchronises and downloads.  A HIP error is returned as 1000 + code and is
// sticky for the whole library (harness_common.hpp): nothing is launched any more in this process.
#include <cmath>

#include "harness_common.hpp"

using namespace relp;

extern "C" {

int rkg_chunk() { return kTabRatioChunk; }

// launch_tab_gomory on the view (m rows, owned stored columns [c_lo, c_lo + n_owned), tableau columns from col_off >= c_lo on: the
// structural columns are the stored columns col_off .., the virtual ones follow them) with p pending rows of at most kmax.  Images
// in: T0 (n_owned columns ld_t apart), W (kmax x ld_b), R0 ((kmax + 1) x ld_r), in_basis and is_integer (by tableau column;
// has_flags == 0: no integer flags, all integer), vrow0 / vsign (by virtual column), bound_row (by structural column), A (nr_normal
// columns ld_a apart: nr_constraints rows, then nr_cuts cut rows that are the tableau rows cut_row0 ..), rows and f0 (count).
// Images out, each at least as long as the launch writes (the tail is the caller's sentinels): pi (count x n_owned), y (count x m),
// bad (count x ceil(n_owned / 256)), g (count x nr_normal).
int rkg_tab_gomory(int64_t m, int64_t n_owned, int64_t c_lo, int64_t col_off, int64_t p, int64_t kmax, int64_t batch, int64_t count,
                   int64_t kind, int64_t ld_t, int64_t ld_b, int64_t ld_r, int64_t ld_a, int64_t nr_constraints, int64_t nr_cuts,
                   int64_t cut_row0, int64_t nr_normal, int64_t nr_virtual, int64_t has_flags, double tol_zero,
                   double* T0, int64_t T0_len, double* W, int64_t W_len, double* R0, int64_t R0_len, uint8_t* in_basis, int64_t in_basis_len,
                   uint8_t* is_integer, int64_t is_integer_len, int32_t* vrow0, int64_t vrow0_len, int32_t* vsign, int64_t vsign_len,
                   int32_t* bound_row, int64_t bound_row_len, double* A, int64_t A_len, int32_t* rows, int64_t rows_len, double* f0,
                   int64_t f0_len, double* pi, int64_t pi_len, double* y, int64_t y_len, double* bad, int64_t bad_len, double* g,
                   int64_t g_len) {
    if (g_sticky) return g_sticky;
    const int64_t cap = 1 << 20;
    REFUSE_IF(m < 1 || m > cap || n_owned < 1 || n_owned > cap || count < 1 || count > 4096, kRefusedShape);
    REFUSE_IF(kmax < 1 || kmax > 128 || p < 0 || p > kmax || (kind != 0 && kind != 1), kRefusedShape);
    REFUSE_IF(!(tol_zero >= 0.0) || !std::isfinite(tol_zero), kRefusedShape);
    REFUSE_IF(batch != 1 && batch != 8 && batch != 16 && batch != 32, kRefusedBatch);
    const int64_t n_all = c_lo + n_owned, n_tab = n_all - col_off, nbc = (n_owned + 255) / 256;
    REFUSE_IF(c_lo < 0 || c_lo > cap || col_off < c_lo || col_off >= n_all, kRefusedIndex);
    REFUSE_IF(ld_t < m || ld_b < m || ld_r < n_owned || ld_t > 2 * cap || ld_b > 2 * cap || ld_r > 2 * cap, kRefusedShape);
    REFUSE_IF(nr_normal < 0 || nr_virtual < 0 || nr_normal + nr_virtual > n_tab, kRefusedIndex);
    REFUSE_IF(nr_constraints < 0 || nr_cuts < 0 || nr_constraints > m || cut_row0 < 0 || cut_row0 + nr_cuts > m, kRefusedIndex);
    REFUSE_IF(ld_a < 1 || ld_a > 2 * cap || nr_constraints + nr_cuts > ld_a, kRefusedIndex);
    REFUSE_IF(T0_len != n_owned * ld_t || W_len != kmax * ld_b || R0_len != (kmax + 1) * ld_r, kRefusedLength);
    REFUSE_IF(in_basis_len != n_tab || (has_flags && is_integer_len != n_tab), kRefusedLength);
    REFUSE_IF(vrow0_len != nr_virtual || vsign_len != nr_virtual || bound_row_len != nr_normal, kRefusedLength);
    REFUSE_IF(A_len != (nr_normal > 0 ? nr_normal : 1) * ld_a || rows_len != count || f0_len != count, kRefusedLength);
    REFUSE_IF(pi_len < count * n_owned || y_len < count * m || bad_len < count * nbc || g_len < count * nr_normal, kRefusedLength);
    for (int64_t k = 0; k < count; ++k) REFUSE_IF(rows[k] < 0 || rows[k] >= m, kRefusedIndex);
    for (int64_t v = 0; v < nr_virtual; ++v) REFUSE_IF(vrow0[v] < -1 || vrow0[v] >= m || (vsign[v] != 1 && vsign[v] != -1), kRefusedIndex);
    for (int64_t c = 0; c < nr_normal; ++c) REFUSE_IF(bound_row[c] < -1 || bound_row[c] >= m, kRefusedIndex);
    for (int64_t j = 0; j < in_basis_len; ++j) REFUSE_IF(in_basis[j] > 2, kRefusedIndex);

    Image<double> iT0(T0, T0_len), iW(W, W_len), iR0(R0, R0_len), iA(A, A_len), if0(f0, f0_len), ipi(pi, pi_len), iy(y, y_len), ibad(bad, bad_len),
        ig(g, g_len);
    Image<uint8_t> iflag(in_basis, in_basis_len), iint(is_integer, has_flags ? is_integer_len : 0);
    Image<int32_t> iv0(vrow0, vrow0_len), ivs(vsign, vsign_len), ibr(bound_row, bound_row_len), irows(rows, rows_len);
    HIP_OK(iT0.up()); HIP_OK(iW.up()); HIP_OK(iR0.up()); HIP_OK(iA.up()); HIP_OK(if0.up()); HIP_OK(ipi.up()); HIP_OK(iy.up()); HIP_OK(ibad.up());
    HIP_OK(ig.up()); HIP_OK(iflag.up()); HIP_OK(iint.up()); HIP_OK(iv0.up()); HIP_OK(ivs.up()); HIP_OK(ibr.up()); HIP_OK(irows.up());

    TableauView tv{};
    tv.T0 = iT0.d - c_lo * ld_t; tv.ld_t = ld_t;
    tv.R0 = iR0.d - c_lo; tv.ld_r = ld_r;
    tv.m = (int32_t)m; tv.n_store = (int32_t)n_all; tv.col_off = (int32_t)col_off; tv.n = (int32_t)n_tab;
    tv.c_lo = (int32_t)c_lo; tv.c_hi = (int32_t)n_all;
    DeferredUpdate du{};
    du.W = iW.d; du.ld = ld_b; du.kmax = (int32_t)kmax; du.batch = (int32_t)batch;
    ColumnTable ct{};
    ct.nr_artificial = 0; ct.nr_normal = (int32_t)nr_normal; ct.nr_virtual = (int32_t)nr_virtual; ct.nr_constraints = (int32_t)nr_constraints;
    ct.bound_row = ibr.d; ct.vrow0 = iv0.d; ct.vsign = ivs.d; ct.cut_row0 = (int32_t)cut_row0; ct.nr_cuts = (int32_t)nr_cuts;
    Tolerances tol{};
    tol.zero = tol_zero;
    const GomoryCuts gc{irows.d, if0.d, has_flags ? iint.d : nullptr, (int32_t)count, (int32_t)kind, iA.d, ld_a, (int32_t)col_off, (int32_t)nr_normal,
                        ipi.d, iy.d, ibad.d, ig.d};
    launch_tab_gomory(tv, du, ct, iflag.d, tol, gc, (int32_t)p, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());

    HIP_OK(iT0.back()); HIP_OK(iW.back()); HIP_OK(iR0.back()); HIP_OK(iA.back()); HIP_OK(if0.back()); HIP_OK(ipi.back()); HIP_OK(iy.back());
    HIP_OK(ibad.back()); HIP_OK(ig.back()); HIP_OK(iflag.back()); HIP_OK(iint.back()); HIP_OK(iv0.back()); HIP_OK(ivs.back()); HIP_OK(ibr.back());
    HIP_OK(irows.back());
    return 0;
}

}  // extern "C"
