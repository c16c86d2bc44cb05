// The kernel harness of the cut pool (test infrastructure): extern "C" entries that run relp::launch_cutpool_separate and
// relp::launch_cutpool_add_operands of the shipped librelp_engine.so once on whole device IMAGES a test constructs
// (tests/kernel_harness_cutpool.py) and hand every image back.  `make -C tests/kernels`
//
// The caller owns the layout: every buffer is passed as the image the device shall hold (its own sentinels where the launch must
// not write).  This file only checks that nothing the launch may touch lies outside an image -- a refused call (negative code)
// launches nothing -- uploads, launches, synchronises and downloads.  A HIP error is returned as 1000 + code and is sticky for the
// whole library (harness_common.hpp): nothing is launched any more in this process.
#include "harness_common.hpp"

using namespace relp;

namespace {

// the pool and the vertex as images: what both launches read
struct CutPoolArgs {
    int64_t count, m, nr_normal;
    int64_t* slice_ptr; int64_t slice_ptr_len; int32_t* col; int64_t col_len; double* val; int64_t val_len; double* rhs; int64_t rhs_len;
    double* norm; int64_t norm_len; uint8_t* active; int64_t active_len; int32_t* basis; int64_t basis_len;
};
int check_pool(const CutPoolArgs& a) {
    REFUSE_IF(a.count < 0 || a.count > kPoolCap || a.m < 1 || a.m > kPoolCap || a.nr_normal < 1 || a.nr_normal > kPoolCap, kRefusedShape);
    REFUSE_IF(a.norm_len != a.count || a.basis_len != a.m, kRefusedLength);
    if (const int rc = check_sliced_ell(a.count, a.nr_normal, a.slice_ptr, a.slice_ptr_len, a.col, a.col_len, a.val_len, a.rhs_len, a.active_len)) return rc;
    // a structural column is basic in at most one row (the one writer of its word of x and of mark)
    std::vector<uint8_t> basic((size_t)a.nr_normal, 0);
    for (int64_t r = 0; r < a.m; ++r) {
        const int32_t j = a.basis[r];
        if (j < 0 || j >= a.nr_normal) continue;
        REFUSE_IF(basic[j], kRefusedIndex);
        basic[j] = 1;
    }
    return 0;
}

}  // namespace

extern "C" {

int rkcutpool_slice() { return kPoolSlice; }
int rkcutpool_chunk() { return kPoolChunk; }

// launch_cutpool_separate over the pool (count cuts over nr_normal structural columns; the vertex from b and basis over m rows).
// segments == 0: the slacks alone (s_all).  Images, in and out: the pool, b (b_len >= m), basis, x (nr_normal), s_all (count),
// part_d / part_k (segments * chunks), out_k / out_s (segments), found (1, or none with segments == 0).
int rkcutpool_separate(int64_t count, int64_t m, int64_t nr_normal, int64_t segments, int64_t by_efficacy, double tol,
                       int64_t* slice_ptr, int64_t slice_ptr_len, int32_t* col, int64_t col_len, double* val, int64_t val_len, double* rhs,
                       int64_t rhs_len, double* norm, int64_t norm_len, uint8_t* active, int64_t active_len, int32_t* basis, int64_t basis_len,
                       double* b, int64_t b_len, double* x, int64_t x_len, double* s_all, int64_t s_all_len, double* part_d, int64_t part_d_len,
                       int32_t* part_k, int64_t part_k_len, int32_t* out_k, int64_t out_k_len, double* out_s, int64_t out_s_len, int32_t* found,
                       int64_t found_len) {
    if (g_sticky) return g_sticky;
    const CutPoolArgs a{count, m, nr_normal, slice_ptr, slice_ptr_len, col, col_len, val, val_len, rhs, rhs_len, norm, norm_len,
                        active, active_len, basis, basis_len};
    if (const int rc = check_pool(a)) return rc;
    REFUSE_IF(segments < 0 || (segments > 0 && count > 0 && segments > count) || !(tol >= 0.0), kRefusedShape);
    REFUSE_IF(by_efficacy != 0 && by_efficacy != 1, kRefusedShape);
    REFUSE_IF(b_len < m || x_len != nr_normal || s_all_len != count, kRefusedLength);
    const int64_t parts = segments > 0 ? segments * pool_segment_chunks((int32_t)count, (int32_t)segments) : 0;
    REFUSE_IF(part_d_len != parts || part_k_len != parts || out_k_len != segments || out_s_len != segments, kRefusedLength);
    REFUSE_IF(found_len != (segments > 0 ? 1 : 0), kRefusedLength);

    Image<int64_t> isp(slice_ptr, slice_ptr_len);
    Image<int32_t> icol(col, col_len), ibas(basis, basis_len), ipk(part_k, part_k_len), iok(out_k, out_k_len), ifound(found, found_len);
    Image<double> ival(val, val_len), irhs(rhs, rhs_len), inorm(norm, norm_len), ib(b, b_len), ix(x, x_len), iall(s_all, s_all_len),
        ipd(part_d, part_d_len), ios(out_s, out_s_len);
    Image<uint8_t> iact(active, active_len);
    HIP_OK(isp.up()); HIP_OK(icol.up()); HIP_OK(ibas.up()); HIP_OK(ipk.up()); HIP_OK(iok.up()); HIP_OK(ifound.up()); HIP_OK(ival.up());
    HIP_OK(irhs.up()); HIP_OK(inorm.up()); HIP_OK(ib.up()); HIP_OK(ix.up()); HIP_OK(iall.up()); HIP_OK(ipd.up()); HIP_OK(ios.up()); HIP_OK(iact.up());

    const CutPoolView cv{PoolView{isp.d, icol.d, ival.d, irhs.d, iact.d, (int32_t)count}, inorm.d};
    const Vertex vx{ib.d, ibas.d, (int32_t)m, (int32_t)nr_normal, ix.d};
    launch_cutpool_separate(cv, vx, (int32_t)segments, tol, (int32_t)by_efficacy, iall.d, ipd.d, ipk.d, iok.d, ios.d, ifound.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());

    HIP_OK(isp.back()); HIP_OK(icol.back()); HIP_OK(ibas.back()); HIP_OK(ipk.back()); HIP_OK(iok.back()); HIP_OK(ifound.back()); HIP_OK(ival.back());
    HIP_OK(irhs.back()); HIP_OK(inorm.back()); HIP_OK(ib.back()); HIP_OK(ix.back()); HIP_OK(iall.back()); HIP_OK(ipd.back()); HIP_OK(ios.back());
    HIP_OK(iact.back());
    return 0;
}

// launch_cutpool_add_operands for the pool cuts ids[0 .. nids).  `longest` and `room` are what the engine's host side hands the
// launch: the longest chosen cut (checked here from the images) and a bound of the union list (checked here: at least the rows
// whose basic column is structural and touched by a chosen cut).  Images, in and out: the pool, basis (m), b (m + nids: the new
// rows' b behind the old), ids (nids), mark (nr_normal), rows (>= room), entries_out (1), coef (room * nids), A (nr_normal * ld_a,
// the chosen cuts' rows at a_row0 ..).
int rkcutpool_add_operands(int64_t count, int64_t m, int64_t nr_normal, int64_t nids, int64_t longest, int64_t room, int64_t ld_a,
                           int64_t a_row0, int64_t* slice_ptr, int64_t slice_ptr_len, int32_t* col, int64_t col_len, double* val,
                           int64_t val_len, double* rhs, int64_t rhs_len, double* norm, int64_t norm_len, uint8_t* active, int64_t active_len,
                           int32_t* basis, int64_t basis_len, double* b, int64_t b_len, int32_t* ids, int64_t ids_len, int32_t* mark,
                           int64_t mark_len, int32_t* rows, int64_t rows_len, int32_t* entries_out, int64_t entries_out_len, double* coef,
                           int64_t coef_len, double* A, int64_t A_len) {
    if (g_sticky) return g_sticky;
    const CutPoolArgs a{count, m, nr_normal, slice_ptr, slice_ptr_len, col, col_len, val, val_len, rhs, rhs_len, norm, norm_len,
                        active, active_len, basis, basis_len};
    if (const int rc = check_pool(a)) return rc;
    REFUSE_IF(nids < 1 || nids > 4096 || ids_len != nids || a_row0 < 0 || ld_a < a_row0 + nids || ld_a > (1 << 20), kRefusedShape);
    REFUSE_IF(room < 0 || room > m, kRefusedShape);
    REFUSE_IF(b_len != m + nids || mark_len != nr_normal || entries_out_len != 1 || A_len != nr_normal * ld_a, kRefusedLength);
    std::vector<uint8_t> named((size_t)count, 0), touched((size_t)nr_normal, 0);
    int64_t longest_is = 0;
    for (int64_t x = 0; x < nids; ++x) {
        REFUSE_IF(ids[x] < 0 || ids[x] >= count || named[ids[x]], kRefusedIndex);
        named[ids[x]] = 1;
        const int64_t s = ids[x] / kPoolSlice, width = (slice_ptr[s + 1] - slice_ptr[s]) / kPoolSlice;
        int64_t len = 0;
        for (int64_t e = 0; e < width; ++e) {
            const int32_t j = col[slice_ptr[s] + e * kPoolSlice + ids[x] % kPoolSlice];
            if (j < 0) continue;
            len = e + 1;
            touched[j] = 1;
        }
        longest_is = longest_is > len ? longest_is : len;
    }
    int64_t list = 0;
    for (int64_t r = 0; r < m; ++r)
        if (basis[r] >= 0 && basis[r] < nr_normal && touched[basis[r]]) ++list;
    REFUSE_IF(longest != longest_is || room < list, kRefusedShape);
    REFUSE_IF(rows_len < room || coef_len != room * nids, kRefusedLength);

    Image<int64_t> isp(slice_ptr, slice_ptr_len);
    Image<int32_t> icol(col, col_len), ibas(basis, basis_len), iids(ids, ids_len), imark(mark, mark_len), irows(rows, rows_len),
        ient(entries_out, entries_out_len);
    Image<double> ival(val, val_len), irhs(rhs, rhs_len), inorm(norm, norm_len), ib(b, b_len), icoef(coef, coef_len), iA(A, A_len);
    Image<uint8_t> iact(active, active_len);
    HIP_OK(isp.up()); HIP_OK(icol.up()); HIP_OK(ibas.up()); HIP_OK(iids.up()); HIP_OK(imark.up()); HIP_OK(irows.up()); HIP_OK(ient.up());
    HIP_OK(ival.up()); HIP_OK(irhs.up()); HIP_OK(inorm.up()); HIP_OK(ib.up()); HIP_OK(icoef.up()); HIP_OK(iA.up()); HIP_OK(iact.up());

    const CutPoolView cv{PoolView{isp.d, icol.d, ival.d, irhs.d, iact.d, (int32_t)count}, inorm.d};
    const CutPoolAdd ca{iids.d, (int32_t)nids, (int32_t)m, (int32_t)nr_normal, (int32_t)longest, (int32_t)room, ibas.d, ib.d, imark.d, irows.d,
                        ient.d, icoef.d, iA.d, ld_a, (int32_t)a_row0, ib.d + m};
    launch_cutpool_add_operands(cv, ca, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());

    HIP_OK(isp.back()); HIP_OK(icol.back()); HIP_OK(ibas.back()); HIP_OK(iids.back()); HIP_OK(imark.back()); HIP_OK(irows.back()); HIP_OK(ient.back());
    HIP_OK(ival.back()); HIP_OK(irhs.back()); HIP_OK(inorm.back()); HIP_OK(ib.back()); HIP_OK(icoef.back()); HIP_OK(iA.back()); HIP_OK(iact.back());
    return 0;
}

}  // extern "C"
