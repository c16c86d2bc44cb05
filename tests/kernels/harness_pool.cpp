// The kernel harness of the column pool (test infrastructure): extern "C" entries that run relp::launch_pool_price,
// relp::launch_pool_add_operands and relp::launch_pool_set_active of the shipped librelp_engine.so once on whole device IMAGES a test
// constructs (tests/kernel_harness_pool.py) and hand every image back.  `make -C tests/kernels`
//
// The caller owns the layout: every buffer is passed as the image the device shall hold (its own sentinels where the launch must
// not write).  This file only checks that nothing the launch may touch lies outside an image -- a refused call (negative code)
// launches nothing -- uploads, launches, synchronises and downloads.  A HIP error is returned as 1000 + code and is sticky for the
// whole library (harness_common.hpp): nothing is launched any more in this process.
#include "harness_common.hpp"

using namespace relp;

namespace {

// the pool and -pi as images: what both launches read
struct PoolArgs {
    int64_t count, m, n_store;
    int64_t* slice_ptr; int64_t slice_ptr_len; int32_t* row; int64_t row_len; double* val; int64_t val_len; double* cost; int64_t cost_len;
    uint8_t* active; int64_t active_len; double* d; int64_t d_len; double* cost_store; int64_t cost_store_len; int32_t* idcol; int64_t idcol_len;
};
int check_pool(const PoolArgs& a) {
    REFUSE_IF(a.count < 0 || a.count > kPoolCap || a.m < 1 || a.m > kPoolCap || a.n_store < 1 || a.n_store > kPoolCap, kRefusedShape);
    REFUSE_IF(a.d_len != a.n_store || a.cost_store_len != a.n_store || a.idcol_len != a.m, kRefusedLength);
    if (const int rc = check_sliced_ell(a.count, a.m, a.slice_ptr, a.slice_ptr_len, a.row, a.row_len, a.val_len, a.cost_len, a.active_len)) return rc;
    for (int64_t i = 0; i < a.m; ++i) REFUSE_IF(a.idcol[i] < 0 || a.idcol[i] >= a.n_store, kRefusedIndex);
    return 0;
}

}  // namespace

extern "C" {

int rkpool_slice() { return kPoolSlice; }
int rkpool_chunk() { return kPoolChunk; }

// launch_pool_price over the pool (count columns over m rows; -pi from d, cost_store over n_store stored columns and idcol).
// segments == 0: the reduced costs alone (d_all).  Images, in and out: the pool, d / cost_store / idcol and the m words -pi is
// written to (minus_pi), d_all (count words, or none: not written),
// part_d / part_k (segments * chunks), out_k / out_d (segments), found (1).
int rkpool_price(int64_t count, int64_t m, int64_t n_store, int64_t segments, double tol,
                 int64_t* slice_ptr, int64_t slice_ptr_len, int32_t* row, int64_t row_len, double* val, int64_t val_len, double* cost,
                 int64_t cost_len, uint8_t* active, int64_t active_len, double* d, int64_t d_len, double* cost_store, int64_t cost_store_len,
                 int32_t* idcol, int64_t idcol_len, double* minus_pi, int64_t minus_pi_len, double* d_all, int64_t d_all_len, double* part_d,
                 int64_t part_d_len, int32_t* part_k,
                 int64_t part_k_len, int32_t* out_k, int64_t out_k_len, double* out_d, int64_t out_d_len, int32_t* found, int64_t found_len) {
    if (g_sticky) return g_sticky;
    const PoolArgs a{count, m, n_store, slice_ptr, slice_ptr_len, row, row_len, val, val_len, cost, cost_len, active, active_len,
                     d, d_len, cost_store, cost_store_len, idcol, idcol_len};
    if (const int rc = check_pool(a)) return rc;
    REFUSE_IF(segments < 0 || (segments > 0 && count > 0 && segments > count) || !(tol >= 0.0), kRefusedShape);
    REFUSE_IF(minus_pi_len != m || (d_all_len != 0 && d_all_len != count), kRefusedLength);
    REFUSE_IF(segments == 0 && d_all_len != count, kRefusedLength);
    const int64_t parts = segments > 0 ? segments * pool_segment_chunks((int32_t)count, (int32_t)segments) : 0;
    REFUSE_IF(part_d_len != parts || part_k_len != parts || out_k_len != segments || out_d_len != segments, kRefusedLength);
    REFUSE_IF(found_len != (segments > 0 ? 1 : 0), kRefusedLength);

    Image<int64_t> isp(slice_ptr, slice_ptr_len);
    Image<int32_t> irow(row, row_len), iidc(idcol, idcol_len), ipk(part_k, part_k_len), iok(out_k, out_k_len), ifound(found, found_len);
    Image<double> ival(val, val_len), icost(cost, cost_len), id(d, d_len), ics(cost_store, cost_store_len), iall(d_all, d_all_len),
        ipd(part_d, part_d_len), iod(out_d, out_d_len), impi(minus_pi, minus_pi_len);
    Image<uint8_t> iact(active, active_len);
    HIP_OK(isp.up()); HIP_OK(irow.up()); HIP_OK(iidc.up()); HIP_OK(ipk.up()); HIP_OK(iok.up()); HIP_OK(ifound.up()); HIP_OK(ival.up());
    HIP_OK(icost.up()); HIP_OK(id.up()); HIP_OK(ics.up()); HIP_OK(iall.up()); HIP_OK(ipd.up()); HIP_OK(iod.up()); HIP_OK(iact.up()); HIP_OK(impi.up());

    const PoolView pv{isp.d, irow.d, ival.d, icost.d, iact.d, (int32_t)count};
    const MinusPi mp{id.d, ics.d, iidc.d, (int32_t)m, impi.d};
    launch_pool_price(pv, mp, (int32_t)segments, tol, d_all_len ? iall.d : nullptr, ipd.d, ipk.d, iok.d, iod.d, ifound.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());

    HIP_OK(isp.back()); HIP_OK(irow.back()); HIP_OK(iidc.back()); HIP_OK(ipk.back()); HIP_OK(iok.back()); HIP_OK(ifound.back()); HIP_OK(ival.back());
    HIP_OK(icost.back()); HIP_OK(id.back()); HIP_OK(ics.back()); HIP_OK(iall.back()); HIP_OK(ipd.back()); HIP_OK(iod.back()); HIP_OK(iact.back()); HIP_OK(impi.back());
    return 0;
}

// launch_pool_add_operands for the pool columns ids[0 .. nids).  `longest` and `entries` are what the engine's host side hands the
// launch: they must be the longest chosen column and the number of rows the chosen columns touch (checked here from the images:
// the zero fill of coef and the scatter rely on them).  Images, in and out: the pool, -pi, ids (nids), rank (m), cols (>= entries),
// entries_out (1), coef (entries * nids), col_a ((a0 + nids) * ld_c), d_new and cost_new (nids each).
int rkpool_add_operands(int64_t count, int64_t m, int64_t n_store, int64_t nids, int64_t longest, int64_t entries, int64_t ld_c, int64_t a0,
                        int64_t* slice_ptr, int64_t slice_ptr_len, int32_t* row, int64_t row_len, double* val, int64_t val_len, double* cost,
                        int64_t cost_len, uint8_t* active, int64_t active_len, double* d, int64_t d_len, double* cost_store,
                        int64_t cost_store_len, int32_t* idcol, int64_t idcol_len, double* minus_pi, int64_t minus_pi_len, int32_t* ids, int64_t ids_len, int32_t* rank, int64_t rank_len,
                        int32_t* cols, int64_t cols_len, int32_t* entries_out, int64_t entries_out_len, double* coef, int64_t coef_len,
                        double* col_a, int64_t col_a_len, double* d_new, int64_t d_new_len, double* cost_new, int64_t cost_new_len) {
    if (g_sticky) return g_sticky;
    const PoolArgs a{count, m, n_store, slice_ptr, slice_ptr_len, row, row_len, val, val_len, cost, cost_len, active, active_len,
                     d, d_len, cost_store, cost_store_len, idcol, idcol_len};
    if (const int rc = check_pool(a)) return rc;
    REFUSE_IF(nids < 1 || nids > 4096 || ids_len != nids || a0 < 0 || a0 > 4096 || ld_c < m || ld_c > (1 << 23), kRefusedShape);
    REFUSE_IF(minus_pi_len != m || rank_len != m || entries_out_len != 1 || d_new_len != nids || cost_new_len != nids, kRefusedLength);
    REFUSE_IF(col_a_len != (a0 + nids) * ld_c, kRefusedLength);
    std::vector<uint8_t> named((size_t)count, 0), touched((size_t)m, 0);
    int64_t longest_is = 0, entries_are = 0;
    for (int64_t x = 0; x < nids; ++x) {
        REFUSE_IF(ids[x] < 0 || ids[x] >= count || named[ids[x]], kRefusedIndex);
        named[ids[x]] = 1;
        const int64_t s = ids[x] / kPoolSlice, width = (slice_ptr[s + 1] - slice_ptr[s]) / kPoolSlice;
        int64_t len = 0;
        for (int64_t e = 0; e < width; ++e) {
            const int32_t r = row[slice_ptr[s] + e * kPoolSlice + ids[x] % kPoolSlice];
            if (r < 0) continue;
            len = e + 1;
            if (!touched[r]) { touched[r] = 1; ++entries_are; }
        }
        longest_is = longest_is > len ? longest_is : len;
    }
    REFUSE_IF(longest != longest_is || entries != entries_are, kRefusedShape);
    REFUSE_IF(cols_len < entries || coef_len != entries * nids, kRefusedLength);

    Image<int64_t> isp(slice_ptr, slice_ptr_len);
    Image<int32_t> irow(row, row_len), iidc(idcol, idcol_len), iids(ids, ids_len), irank(rank, rank_len), icols(cols, cols_len),
        ient(entries_out, entries_out_len);
    Image<double> ival(val, val_len), icost(cost, cost_len), id(d, d_len), ics(cost_store, cost_store_len), icoef(coef, coef_len),
        ica(col_a, col_a_len), idn(d_new, d_new_len), icn(cost_new, cost_new_len), impi(minus_pi, minus_pi_len);
    Image<uint8_t> iact(active, active_len);
    HIP_OK(isp.up()); HIP_OK(irow.up()); HIP_OK(iidc.up()); HIP_OK(iids.up()); HIP_OK(irank.up()); HIP_OK(icols.up()); HIP_OK(ient.up());
    HIP_OK(ival.up()); HIP_OK(icost.up()); HIP_OK(id.up()); HIP_OK(ics.up()); HIP_OK(icoef.up()); HIP_OK(ica.up()); HIP_OK(idn.up());
    HIP_OK(icn.up()); HIP_OK(iact.up()); HIP_OK(impi.up());

    const PoolView pv{isp.d, irow.d, ival.d, icost.d, iact.d, (int32_t)count};
    const MinusPi mp{id.d, ics.d, iidc.d, (int32_t)m, impi.d};
    const PoolAdd pa{iids.d, (int32_t)nids, (int32_t)m, (int32_t)longest, (int32_t)entries, irank.d, icols.d, ient.d, icoef.d,
                     ica.d, ld_c, (int32_t)a0, idn.d, icn.d};
    launch_pool_add_operands(pv, mp, pa, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());

    HIP_OK(isp.back()); HIP_OK(irow.back()); HIP_OK(iidc.back()); HIP_OK(iids.back()); HIP_OK(irank.back()); HIP_OK(icols.back()); HIP_OK(ient.back());
    HIP_OK(ival.back()); HIP_OK(icost.back()); HIP_OK(id.back()); HIP_OK(ics.back()); HIP_OK(icoef.back()); HIP_OK(ica.back()); HIP_OK(idn.back());
    HIP_OK(icn.back()); HIP_OK(iact.back()); HIP_OK(impi.back());
    return 0;
}

// launch_pool_set_active: active[ids[x]] = flag.  Images, in and out: active (count), ids (nids).
int rkpool_set_active(int64_t count, int64_t nids, int64_t flag, uint8_t* active, int64_t active_len, int32_t* ids, int64_t ids_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(count < 1 || count > (1 << 22) || nids < 1 || nids > count || (flag != 0 && flag != 1), kRefusedShape);
    REFUSE_IF(active_len != count || ids_len != nids, kRefusedLength);
    for (int64_t x = 0; x < nids; ++x) REFUSE_IF(ids[x] < 0 || ids[x] >= count, kRefusedIndex);
    Image<uint8_t> iact(active, active_len);
    Image<int32_t> iids(ids, ids_len);
    HIP_OK(iact.up()); HIP_OK(iids.up());
    const PoolView pv{nullptr, nullptr, nullptr, nullptr, iact.d, (int32_t)count};
    launch_pool_set_active(pv, iids.d, (int32_t)nids, (int32_t)flag, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(iact.back()); HIP_OK(iids.back());
    return 0;
}

}  // extern "C"
