// The kernel harness of the rows and columns removed in place (test infrastructure): one extern "C" entry that runs
// relp::launch_tab_compact of the shipped librelp_engine.so once on a whole device IMAGE a test constructs
// (tests/kernel_harness_remove.py) and hands the image back.  `make -C tests/kernels`
//
// The caller owns the layout: it passes the pitch and the image as the device shall hold it (its own sentinels where the launch must
// not write).  This file only checks that nothing the launch may touch lies outside the image -- a refused call (negative code)
// launches nothing -- uploads, launches, synchronises and downloads.  A HIP error is returned as 1000 + code and is sticky for the
// whole library (harness_common.hpp): nothing is launched any more in this process.

#include "harness_common.hpp"

using namespace relp;

extern "C" {

int rkrm_batch() { return kTabCompactB; }

// launch_tab_compact on the image img (img_len = ld x the columns the image has, at least n): m rows and n columns are live, the
// lists rows (nr) and cols (nc) ascend strictly inside them.  batch: 1, or the shipped kTabCompactB.
int rkrm_tab_compact(int64_t m, int64_t n, int64_t ld, int64_t batch, double* img, int64_t img_len, int32_t* rows, int64_t nr, int32_t* cols,
                     int64_t nc) {
    if (g_sticky) return g_sticky;
    const int64_t cap = 1 << 22;
    REFUSE_IF(m < 1 || m > cap || n < 1 || n > cap || ld < m || ld > 2 * cap, kRefusedShape);
    REFUSE_IF(batch != 1 && batch != kTabCompactB, kRefusedBatch);
    REFUSE_IF(img_len < n * ld || img_len % ld != 0 || img_len > ((int64_t)1 << 28), kRefusedLength);
    REFUSE_IF(nr < 0 || nr > m || nc < 0 || nc > n, kRefusedShape);
    for (int64_t k = 0; k < nr; ++k) REFUSE_IF(rows[k] < 0 || rows[k] >= m || (k > 0 && rows[k] <= rows[k - 1]), kRefusedIndex);
    for (int64_t k = 0; k < nc; ++k) REFUSE_IF(cols[k] < 0 || cols[k] >= n || (k > 0 && cols[k] <= cols[k - 1]), kRefusedIndex);

    Image<double> image(img, img_len);
    Image<int32_t> irows(rows, nr), icols(cols, nc);
    HIP_OK(image.up()); HIP_OK(irows.up()); HIP_OK(icols.up());
    launch_tab_compact(image.d, ld, (int32_t)m, (int32_t)n, irows.d, (int32_t)nr, icols.d, (int32_t)nc, (int32_t)batch, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(image.back());
    return 0;
}

}  // extern "C"
