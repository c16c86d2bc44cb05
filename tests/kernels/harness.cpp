// harness.cpp -- test infrastructure: one extern "C" entry per launcher family of the blocked update (T1 - T4, R1 - R5) and of the
// in-place changes and batched ratio queries of the tableau engine (T5 - T8, at the end of the file), so that a test can
// run a single relp::launch_* of the shipped library on operands it constructs (tests/kernel_harness.py binds it).
//
// Rules of every entry:
//   * host arrays in, host arrays out: the harness allocates, uploads, launches on the null stream, synchronises, downloads
//     and frees.  Every array argument is (pointer, length); callers pass LOGICAL matrices and never a pitch;
//   * pitches and allocation sizes are computed here by the rules of Engine::create: ld_b = round_up(m, 16) for W, Binv and
//     every m-vector, ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2); R0 has kmax + 1 rows, R0c kmax rows, W kmax
//     columns; T0, R0 are pre-shifted by c_lo as in Engine::tview();
//   * fill != 0: pitch padding and stale regions (rows m..ld-1, rows of R0 / columns of W / entries of wr at and beyond p,
//     R0's scratch row, R0c and cols) are filled with the quiet NaN kSentinel before the upload; the WHOLE of every buffer
//     comes back so that the test sees what was written;
//   * refusals (negative return codes) happen before any HIP call; every list index an entry accepts is in range;
//   * the first HIP error is sticky for the whole library (harness_common.hpp): every later entry of every family returns
//     kHipErrorBase + that error without touching the GPU.
//
// Layouts of the logical arrays (C order): T0[c][i] (n_owned x m), W[j][i] (p x m), R0[j][c] (p x n_owned),
// Binv[i][j] (m x m).  Returned device images: T0 n_owned x ld_t, W kmax x ld_b, R0 (kmax + 1) x ld_r, Binv m x ld_b.
//
// A new kernel family gets a harness as one source file harness_<family>.cpp beside this one that includes harness_common.hpp
// (every entry: `if (g_sticky) return g_sticky;`, the REFUSE_* checks, then Image<T> / Dev<T>, the launcher on stream 0, and every
// buffer back), its name in SRCS of the Makefile, and one Python module tests/kernel_harness_<family>.py over tests/kernel_harness.py.
#include <string.h>

#include <algorithm>

#include "harness_common.hpp"

using namespace relp;

namespace {

constexpr uint64_t kSentinelBits = 0x7ff80000c0ffee01ull;
constexpr int32_t kSentinelInt = -0x5a5a5a5b;

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline double sentinel() { double d; memcpy(&d, &kSentinelBits, 8); return d; }

// a device buffer with its host image; freed on scope exit
template <class T>
struct Dev {
    std::vector<T> h;
    T* d = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (d) (void)hipFree(d); }
    void init(int64_t n, T fill) { h.assign((size_t)std::max<int64_t>(n, 1), fill); }
    int upload() {
        HIP_OK(hipMalloc((void**)&d, h.size() * sizeof(T)));
        HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    // the whole buffer back into the caller's array of n entries
    int back(T* out, int64_t n) {
        HIP_OK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost));
        memcpy(out, h.data(), (size_t)n * sizeof(T));
        return 0;
    }
};

// rows x cols logical (row-major, `cols` contiguous) into an image of total_rows x ld, the rest = fill
void pad_rows(std::vector<double>& img, const double* src, int64_t rows, int64_t cols, int64_t ld, int64_t total_rows, double fill) {
    img.assign((size_t)std::max<int64_t>(total_rows * ld, 1), fill);
    for (int64_t r = 0; r < rows; ++r) memcpy(&img[(size_t)(r * ld)], src + r * cols, (size_t)cols * sizeof(double));
}

PivotRecord blank_record() {
    PivotRecord R;
    memset(&R, 0, sizeof R);
    R.outcome = DEV_RUNNING;
    R.last_selected = -1;
    R.phase = 2;
    return R;
}

bool shape_refused(int64_t m, int64_t n_owned, int64_t p, int64_t kmax) {
    return m < 1 || n_owned < 1 || p < 0 || p > kmax || kmax > 128 || kmax < 0;
}

// The tableau operands of one call: T0, W, R0 as the engine lays them out, and the views the launchers take.
struct TabOperands {
    int64_t m, n, p, kmax, c_lo, ld_b, ld_t, ld_r;
    Dev<double> T0, W, R0, wr;
    Dev<int32_t> S, pos;
    Dev<PivotRecord> rec;
    int build(int64_t m_, int64_t n_, int64_t p_, int64_t kmax_, int64_t c_lo_, int fill, const double* t0, const double* w,
              const double* r0, const PivotRecord& R) {
        m = m_; n = n_; p = p_; kmax = kmax_; c_lo = c_lo_;
        ld_b = round_up(m, 16); ld_t = round_up(m, 2); ld_r = round_up(n, 2);
        const double f = fill ? sentinel() : 0.0;
        pad_rows(T0.h, t0, n, m, ld_t, n, f);
        pad_rows(W.h, w, p, m, ld_b, kmax, f);
        pad_rows(R0.h, r0, p, n, ld_r, kmax + 1, f);
        wr.init(kmax, f);
        S.init(kmax, fill ? kSentinelInt : 0);
        pos.init(m, -1);
        rec.init(1, R);
        TRY(T0.upload()); TRY(W.upload()); TRY(R0.upload()); TRY(wr.upload()); TRY(S.upload()); TRY(pos.upload()); TRY(rec.upload());
        return 0;
    }
    TableauView view(double* d) const {
        TableauView tv;
        tv.T0 = T0.d - c_lo * ld_t; tv.ld_t = ld_t;
        tv.R0 = R0.d - c_lo; tv.ld_r = ld_r;
        tv.d = d; tv.m = (int32_t)m; tv.n_store = (int32_t)(c_lo + n); tv.col_off = 0; tv.n = (int32_t)(c_lo + n);
        tv.c_lo = (int32_t)c_lo; tv.c_hi = (int32_t)(c_lo + n);
        return tv;
    }
    DeferredUpdate deferred(int batch) const {
        DeferredUpdate du;
        du.W = W.d; du.ld = ld_b; du.kmax = (int32_t)kmax; du.S = S.d; du.pos_of_row = pos.d; du.wr = wr.d; du.R = nullptr;
        du.batch = batch; du.w_split = 1;
        return du;
    }
};

bool batch_refused(int batch) { return tab_load_batch(batch) != batch; }

// The revised engine's operands: W, S, pos_of_row (from S), wr, and optionally Binv (m x ld_b, padding ZERO as
// launch_set_identity leaves it: the kernels of the revised engine rewrite the padding columns with zeros)
struct RevOperands {
    int64_t m, p, kmax, ld_b;
    Dev<double> W, wr, Binv, R;
    Dev<int32_t> S, pos;
    Dev<PivotRecord> rec;
    int build(int64_t m_, int64_t p_, int64_t kmax_, int fill, const double* w, const int32_t* s, const double* binv, bool with_R,
              const PivotRecord& Rc) {
        m = m_; p = p_; kmax = kmax_;
        ld_b = round_up(m, 16);
        const double f = fill ? sentinel() : 0.0;
        pad_rows(W.h, w, p, m, ld_b, kmax, f);
        wr.init(kmax, f);
        S.init(kmax, fill ? kSentinelInt : 0);
        pos.init(m, -1);
        for (int64_t j = 0; j < p; ++j) { S.h[(size_t)j] = s[j]; pos.h[(size_t)s[j]] = (int32_t)j; }
        rec.init(1, Rc);
        TRY(W.upload()); TRY(wr.upload()); TRY(S.upload()); TRY(pos.upload()); TRY(rec.upload());
        if (binv) { pad_rows(Binv.h, binv, m, m, ld_b, m, 0.0); TRY(Binv.upload()); }
        if (with_R) { R.init(kmax * ld_b, f); TRY(R.upload()); }
        return 0;
    }
    DeferredUpdate deferred() const {
        DeferredUpdate du;
        du.W = W.d; du.ld = ld_b; du.kmax = (int32_t)kmax; du.S = S.d; du.pos_of_row = pos.d; du.wr = wr.d; du.R = R.d;
        du.batch = 0; du.w_split = 1;
        return du;
    }
};

// S must name p distinct rows of [0, m)
bool rows_refused(const int32_t* s, int64_t p, int64_t m) {
    std::vector<char> seen((size_t)m, 0);
    for (int64_t j = 0; j < p; ++j) {
        if (s[j] < 0 || s[j] >= m || seen[(size_t)s[j]]) return true;
        seen[(size_t)s[j]] = 1;
    }
    return false;
}

}  // namespace

extern "C" {

int rkh_sticky_error(void) { return g_sticky; }
uint64_t rkh_sentinel_bits(void) { return kSentinelBits; }
int32_t rkh_sentinel_int(void) { return kSentinelInt; }
int32_t rkh_wrapped_artificial_base(void) { return (int32_t)kWrappedArtificialBase; }

// T1: launch_tab_flush.  listed != 0: FlushList::cols set (mark -> compact -> listed flush on the LDS path).
// stats: {flushes, columns} before the call in, after the call out.
int rkh_tab_flush(int64_t m, int64_t n_owned, int64_t p, int64_t kmax, int64_t c_lo, int listed, int fill,
                  const double* T0, int64_t T0_len, const double* W, int64_t W_len, const double* R0, int64_t R0_len,
                  const uint64_t* stats_in, int64_t stats_in_len,
                  double* T0_out, int64_t T0_out_len, double* W_out, int64_t W_out_len, double* R0_out, int64_t R0_out_len,
                  int32_t* cols_out, int64_t cols_out_len, int32_t* count_out, int64_t count_out_len,
                  double* R0c_out, int64_t R0c_out_len, uint64_t* stats_out, int64_t stats_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, n_owned, p, kmax), kRefusedShape);
    REFUSE_IF(c_lo < 0 || c_lo > (1 << 20), kRefusedIndex);
    const int64_t ld_b = round_up(m, 16), ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2);
    REFUSE_LEN(T0_len, n_owned * m); REFUSE_LEN(W_len, p * m); REFUSE_LEN(R0_len, p * n_owned); REFUSE_LEN(stats_in_len, 2);
    REFUSE_LEN(T0_out_len, n_owned * ld_t); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R0_out_len, (kmax + 1) * ld_r);
    REFUSE_LEN(cols_out_len, n_owned); REFUSE_LEN(count_out_len, 1); REFUSE_LEN(R0c_out_len, kmax * ld_r); REFUSE_LEN(stats_out_len, 2);
    PivotRecord R = blank_record();
    R.n_eta = (int32_t)p; R.n_eta_old = (int32_t)p; R.p_now = (int32_t)p;
    TabOperands op;
    TRY(op.build(m, n_owned, p, kmax, c_lo, fill, T0, W, R0, R));
    Dev<int32_t> cols, count;
    Dev<unsigned long long> mask, stats;
    Dev<double> R0c;
    cols.init(n_owned, kSentinelInt); count.init(1, kSentinelInt); mask.init((n_owned + 63) / 64, 0ull);
    R0c.init(kmax * ld_r, fill ? sentinel() : 0.0);
    stats.init(2, 0ull); stats.h[0] = stats_in[0]; stats.h[1] = stats_in[1];
    TRY(cols.upload()); TRY(count.upload()); TRY(mask.upload()); TRY(R0c.upload()); TRY(stats.upload());
    FlushList fl;
    fl.cols = listed ? cols.d : nullptr; fl.count = count.d; fl.mask = mask.d; fl.R0c = R0c.d; fl.ld = ld_r; fl.stats = stats.d;
    launch_tab_flush(op.view(nullptr), op.deferred(0), op.rec.d, fl, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(op.T0.back(T0_out, T0_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R0.back(R0_out, R0_out_len));
    TRY(cols.back(cols_out, cols_out_len)); TRY(count.back(count_out, 1)); TRY(R0c.back(R0c_out, R0c_out_len));
    unsigned long long st[2];
    TRY(stats.back(st, 2));
    stats_out[0] = st[0]; stats_out[1] = st[1];
    return 0;
}

// T2 (row < 0): launch_tab_column for the owned column q (position from c_lo) into vec_out (ld_b entries).
// T3 (row >= 0): launch_tab_row for that row into vec_out (ld_r entries).
int rkh_tab_vector(int64_t m, int64_t n_owned, int64_t p, int64_t kmax, int64_t c_lo, int batch, int64_t q, int64_t row, int fill,
                   const double* T0, int64_t T0_len, const double* W, int64_t W_len, const double* R0, int64_t R0_len,
                   double* vec_out, int64_t vec_out_len,
                   double* T0_out, int64_t T0_out_len, double* W_out, int64_t W_out_len, double* R0_out, int64_t R0_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, n_owned, p, kmax), kRefusedShape);
    REFUSE_IF(c_lo < 0 || c_lo > (1 << 20), kRefusedIndex);
    const bool is_row = row >= 0;
    REFUSE_IF(is_row ? row >= m : (q < 0 || q >= n_owned), kRefusedIndex);
    REFUSE_IF(batch_refused(batch), kRefusedBatch);
    const int64_t ld_b = round_up(m, 16), ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2);
    REFUSE_LEN(T0_len, n_owned * m); REFUSE_LEN(W_len, p * m); REFUSE_LEN(R0_len, p * n_owned);
    REFUSE_LEN(vec_out_len, is_row ? ld_r : ld_b);
    REFUSE_LEN(T0_out_len, n_owned * ld_t); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R0_out_len, (kmax + 1) * ld_r);
    PivotRecord R = blank_record();
    R.n_eta = (int32_t)p; R.n_eta_old = (int32_t)p; R.p_now = (int32_t)p;
    R.q = is_row ? 0 : (int32_t)(c_lo + q);
    TabOperands op;
    TRY(op.build(m, n_owned, p, kmax, c_lo, fill, T0, W, R0, R));
    Dev<double> vec;
    vec.init(vec_out_len, sentinel());
    TRY(vec.upload());
    if (is_row) launch_tab_row(op.view(nullptr), op.deferred(batch), (int32_t)row, vec.d, op.rec.d, 0);
    else launch_tab_column(op.view(nullptr), op.deferred(batch), vec.d, op.rec.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(vec.back(vec_out, vec_out_len));
    TRY(op.T0.back(T0_out, T0_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R0.back(R0_out, R0_out_len));
    return 0;
}

// T4: launch_tab_update_all for the pivot (row r, owned column q) on a block with p pending rows.  The harness leaves the
// record, wr, S and pos_of_row as ratio_commit_row does: alpha_r = alpha[r], b_r = b[r], d_q = d[q], wr = row r of W,
// n_eta_old = p, eta_target = the slot of r in S or p (then S[p] = r, pos_of_row[r] = p, n_eta = p + 1).
// ipar: {rule, last_selected, leaving, phase, degenerate}; lpar: {iterations, trace_cap}; dpar: {tol_cost, minus_objective}.
// d, in_basis: one entry per owned column.  Out: d (c_lo + n_owned, indexed by storage column), k1 / j (one slot per 256
// owned columns), b (ld_b), basis (m), in_basis (c_lo + n_owned), trace (4 x trace_cap),
// irec {n_eta, eta_target, n_eta_old, degenerate, outcome, q, r, leaving}, lrec {iterations}, drec {minus_objective}.
int rkh_tab_update_all(int64_t m, int64_t n_owned, int64_t p, int64_t kmax, int64_t c_lo, int batch, int64_t r, int64_t q, int fill,
                       const int32_t* ipar, int64_t ipar_len, const int64_t* lpar, int64_t lpar_len, const double* dpar, int64_t dpar_len,
                       const double* T0, int64_t T0_len, const double* W, int64_t W_len, const double* R0, int64_t R0_len,
                       const int32_t* S, int64_t S_len, const double* d, int64_t d_len, const uint8_t* in_basis, int64_t in_basis_len,
                       const double* alpha, int64_t alpha_len, const double* b, int64_t b_len, const int32_t* basis, int64_t basis_len,
                       double* T0_out, int64_t T0_out_len, double* W_out, int64_t W_out_len, double* R0_out, int64_t R0_out_len,
                       double* wr_out, int64_t wr_out_len, int32_t* S_out, int64_t S_out_len, int32_t* pos_out, int64_t pos_out_len,
                       double* d_out, int64_t d_out_len, double* k1_out, int64_t k1_out_len, int32_t* j_out, int64_t j_out_len,
                       double* alpha_out, int64_t alpha_out_len, double* b_out, int64_t b_out_len,
                       int32_t* basis_out, int64_t basis_out_len, uint8_t* in_basis_out, int64_t in_basis_out_len,
                       int32_t* trace_out, int64_t trace_out_len, int32_t* irec, int64_t irec_len, int64_t* lrec, int64_t lrec_len,
                       double* drec, int64_t drec_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, n_owned, p, kmax), kRefusedShape);
    REFUSE_IF(c_lo < 0 || c_lo > (1 << 20), kRefusedIndex);
    REFUSE_IF(r < 0 || r >= m || q < 0 || q >= n_owned, kRefusedIndex);
    REFUSE_IF(batch_refused(batch), kRefusedBatch);
    REFUSE_LEN(ipar_len, 5); REFUSE_LEN(lpar_len, 2); REFUSE_LEN(dpar_len, 2);
    const int64_t ld_b = round_up(m, 16), ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2);
    const int64_t n_all = c_lo + n_owned, nb = tab_scan_blocks((int32_t)n_owned), trace_cap = lpar[1];
    REFUSE_IF(trace_cap < 0 || trace_cap > (1 << 20), kRefusedShape);
    REFUSE_LEN(T0_len, n_owned * m); REFUSE_LEN(W_len, p * m); REFUSE_LEN(R0_len, p * n_owned); REFUSE_LEN(S_len, p);
    REFUSE_LEN(d_len, n_owned); REFUSE_LEN(in_basis_len, n_owned); REFUSE_LEN(alpha_len, m); REFUSE_LEN(b_len, m); REFUSE_LEN(basis_len, m);
    REFUSE_LEN(T0_out_len, n_owned * ld_t); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R0_out_len, (kmax + 1) * ld_r);
    REFUSE_LEN(wr_out_len, kmax); REFUSE_LEN(S_out_len, kmax); REFUSE_LEN(pos_out_len, m);
    REFUSE_LEN(d_out_len, n_all); REFUSE_LEN(k1_out_len, nb); REFUSE_LEN(j_out_len, nb); REFUSE_LEN(alpha_out_len, ld_b); REFUSE_LEN(b_out_len, ld_b);
    REFUSE_LEN(basis_out_len, m); REFUSE_LEN(in_basis_out_len, n_all); REFUSE_LEN(trace_out_len, 4 * trace_cap);
    REFUSE_LEN(irec_len, 8); REFUSE_LEN(lrec_len, 1); REFUSE_LEN(drec_len, 1);
    REFUSE_IF(rows_refused(S, p, m), kRefusedIndex);
    const int32_t leaving = ipar[2];
    REFUSE_IF(leaving < 0 || (leaving < (int32_t)kWrappedArtificialBase && leaving >= n_all), kRefusedIndex);
    REFUSE_IF(ipar[1] < -1 || ipar[1] >= n_all, kRefusedIndex);
    int64_t jt = -1;
    for (int64_t j = 0; j < p; ++j) if (S[j] == r) jt = j;
    REFUSE_IF(jt < 0 && p >= kmax, kRefusedShape);            // a new row needs a free column of W
    const double f = fill ? sentinel() : 0.0;
    PivotRecord R = blank_record();
    R.q = (int32_t)(c_lo + q); R.d_q = d[q]; R.r = (int32_t)r; R.leaving = leaving; R.alpha_r = alpha[r]; R.b_r = b[r];
    R.minus_objective = dpar[1]; R.iterations = lpar[0]; R.last_selected = ipar[1]; R.phase = ipar[3]; R.degenerate = ipar[4];
    R.n_eta_old = (int32_t)p; R.p_now = (int32_t)p; R.eta_target = (int32_t)(jt < 0 ? p : jt); R.n_eta = (int32_t)(jt < 0 ? p + 1 : p);
    TabOperands op;
    {   // as TabOperands::build, with wr, S and pos_of_row filled in
        op.m = m; op.n = n_owned; op.p = p; op.kmax = kmax; op.c_lo = c_lo; op.ld_b = ld_b; op.ld_t = ld_t; op.ld_r = ld_r;
        pad_rows(op.T0.h, T0, n_owned, m, ld_t, n_owned, f);
        pad_rows(op.W.h, W, p, m, ld_b, kmax, f);
        pad_rows(op.R0.h, R0, p, n_owned, ld_r, kmax + 1, f);
        op.wr.init(kmax, f);
        op.S.init(kmax, fill ? kSentinelInt : 0);
        op.pos.init(m, -1);
        for (int64_t j = 0; j < p; ++j) { op.wr.h[(size_t)j] = W[j * m + r]; op.S.h[(size_t)j] = S[j]; op.pos.h[(size_t)S[j]] = (int32_t)j; }
        if (jt < 0) { op.S.h[(size_t)p] = (int32_t)r; op.pos.h[(size_t)r] = (int32_t)p; }
        op.rec.init(1, R);
        TRY(op.T0.upload()); TRY(op.W.upload()); TRY(op.R0.upload()); TRY(op.wr.upload()); TRY(op.S.upload()); TRY(op.pos.upload());
        TRY(op.rec.upload());
    }
    Dev<double> dd, k1, al, bb;
    Dev<int32_t> pj, bas, trace;
    Dev<uint8_t> inb;
    dd.init(n_all, sentinel()); inb.init(n_all, 0);
    for (int64_t c = 0; c < n_owned; ++c) { dd.h[(size_t)(c_lo + c)] = d[c]; inb.h[(size_t)(c_lo + c)] = in_basis[c]; }
    k1.init(nb, sentinel()); pj.init(nb, kSentinelInt);
    al.init(ld_b, f); bb.init(ld_b, f);
    for (int64_t i = 0; i < m; ++i) { al.h[(size_t)i] = alpha[i]; bb.h[(size_t)i] = b[i]; }
    bas.init(m, 0);
    for (int64_t i = 0; i < m; ++i) bas.h[(size_t)i] = basis[i];
    trace.init(4 * trace_cap, kSentinelInt);
    TRY(dd.upload()); TRY(inb.upload()); TRY(k1.upload()); TRY(pj.upload()); TRY(al.upload()); TRY(bb.upload()); TRY(bas.upload());
    TRY(trace.upload());
    SelectPartials sp;
    memset(&sp, 0, sizeof sp);
    sp.k1 = k1.d; sp.j = pj.d; sp.in_basis = inb.d; sp.tol_cost = dpar[0]; sp.rule = ipar[0]; sp.n = (int32_t)n_all; sp.offset = 0;
    sp.nb_struct = 0; sp.tol_tie = 0.0; sp.p_lo = 0; sp.cols_per_slot = 8;
    launch_tab_update_all(op.view(dd.d), op.deferred(batch), sp, (int32_t)m, al.d, bb.d, bas.d, inb.d, trace_cap > 0 ? trace.d : nullptr,
                          trace_cap, op.rec.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(op.T0.back(T0_out, T0_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R0.back(R0_out, R0_out_len));
    TRY(op.wr.back(wr_out, kmax)); TRY(op.S.back(S_out, kmax)); TRY(op.pos.back(pos_out, m));
    TRY(dd.back(d_out, n_all)); TRY(k1.back(k1_out, nb)); TRY(pj.back(j_out, nb)); TRY(al.back(alpha_out, ld_b)); TRY(bb.back(b_out, ld_b));
    TRY(bas.back(basis_out, m)); TRY(inb.back(in_basis_out, n_all)); TRY(trace.back(trace_out, 4 * trace_cap));
    PivotRecord Ro;
    TRY(op.rec.back(&Ro, 1));
    irec[0] = Ro.n_eta; irec[1] = Ro.eta_target; irec[2] = Ro.n_eta_old; irec[3] = Ro.degenerate; irec[4] = Ro.outcome; irec[5] = Ro.q;
    irec[6] = Ro.r; irec[7] = Ro.leaving;
    lrec[0] = Ro.iterations; drec[0] = Ro.minus_objective;
    return 0;
}

// R1: launch_apply_w.  alpha = v + W (S'v); alpha_out has ld_b entries.
int rkh_apply_w(int64_t m, int64_t p, int64_t kmax, int fill, const double* W, int64_t W_len, const int32_t* S, int64_t S_len,
                const double* v, int64_t v_len, double* alpha_out, int64_t alpha_out_len, double* W_out, int64_t W_out_len,
                double* v_out, int64_t v_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, 1, p, kmax), kRefusedShape);
    const int64_t ld_b = round_up(m, 16);
    REFUSE_LEN(W_len, p * m); REFUSE_LEN(S_len, p); REFUSE_LEN(v_len, m);
    REFUSE_LEN(alpha_out_len, ld_b); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(v_out_len, ld_b);
    REFUSE_IF(rows_refused(S, p, m), kRefusedIndex);
    PivotRecord R = blank_record();
    R.n_eta = (int32_t)p;
    RevOperands op;
    TRY(op.build(m, p, kmax, fill, W, S, nullptr, false, R));
    Dev<double> vv, al;
    vv.init(ld_b, fill ? sentinel() : 0.0);
    for (int64_t i = 0; i < m; ++i) vv.h[(size_t)i] = v[i];
    al.init(ld_b, sentinel());
    TRY(vv.upload()); TRY(al.upload());
    launch_apply_w(op.deferred(), (int32_t)m, vv.d, al.d, op.rec.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(al.back(alpha_out, ld_b)); TRY(op.W.back(W_out, W_out_len)); TRY(vv.back(v_out, ld_b));
    return 0;
}

// R2: launch_eta_prepare + launch_update_w for pivot row r with alpha_r = alpha[r].  irec: {n_eta, eta_target, n_eta_old}.
int rkh_eta_update_w(int64_t m, int64_t p, int64_t kmax, int64_t r, int fill, const double* W, int64_t W_len, const int32_t* S,
                     int64_t S_len, const double* alpha, int64_t alpha_len, double* W_out, int64_t W_out_len, double* wr_out,
                     int64_t wr_out_len, int32_t* S_out, int64_t S_out_len, int32_t* pos_out, int64_t pos_out_len, int32_t* irec,
                     int64_t irec_len, double* alpha_out, int64_t alpha_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, 1, p, kmax), kRefusedShape);
    REFUSE_IF(r < 0 || r >= m, kRefusedIndex);
    const int64_t ld_b = round_up(m, 16);
    REFUSE_LEN(W_len, p * m); REFUSE_LEN(S_len, p); REFUSE_LEN(alpha_len, m);
    REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(wr_out_len, kmax); REFUSE_LEN(S_out_len, kmax); REFUSE_LEN(pos_out_len, m);
    REFUSE_LEN(irec_len, 3); REFUSE_LEN(alpha_out_len, ld_b);
    REFUSE_IF(rows_refused(S, p, m), kRefusedIndex);
    bool in_block = false;
    for (int64_t j = 0; j < p; ++j) in_block |= S[j] == r;
    REFUSE_IF(!in_block && p >= kmax, kRefusedShape);
    PivotRecord R = blank_record();
    R.n_eta = (int32_t)p; R.r = (int32_t)r; R.alpha_r = alpha[r];
    RevOperands op;
    TRY(op.build(m, p, kmax, fill, W, S, nullptr, false, R));
    Dev<double> al;
    al.init(ld_b, fill ? sentinel() : 0.0);
    for (int64_t i = 0; i < m; ++i) al.h[(size_t)i] = alpha[i];
    TRY(al.upload());
    launch_eta_prepare(op.deferred(), op.rec.d, 0);
    launch_update_w(op.deferred(), (int32_t)m, al.d, op.rec.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(op.W.back(W_out, W_out_len)); TRY(op.wr.back(wr_out, kmax)); TRY(op.S.back(S_out, kmax)); TRY(op.pos.back(pos_out, m));
    TRY(al.back(alpha_out, ld_b));
    PivotRecord Ro;
    TRY(op.rec.back(&Ro, 1));
    irec[0] = Ro.n_eta; irec[1] = Ro.eta_target; irec[2] = Ro.n_eta_old;
    return 0;
}

// R3: launch_rho_deferred, unsharded.  rho_out: ld_b entries.
int rkh_rho_deferred(int64_t m, int64_t p, int64_t kmax, int64_t r, int fill, const double* W, int64_t W_len, const int32_t* S,
                     int64_t S_len, const double* Binv, int64_t Binv_len, double* rho_out, int64_t rho_out_len, double* W_out,
                     int64_t W_out_len, double* Binv_out, int64_t Binv_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, 1, p, kmax), kRefusedShape);
    REFUSE_IF(r < 0 || r >= m, kRefusedIndex);
    const int64_t ld_b = round_up(m, 16);
    REFUSE_LEN(W_len, p * m); REFUSE_LEN(S_len, p); REFUSE_LEN(Binv_len, m * m);
    REFUSE_LEN(rho_out_len, ld_b); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(Binv_out_len, m * ld_b);
    REFUSE_IF(rows_refused(S, p, m), kRefusedIndex);
    PivotRecord R = blank_record();
    R.n_eta = (int32_t)p; R.r = (int32_t)r;
    RevOperands op;
    TRY(op.build(m, p, kmax, fill, W, S, Binv, false, R));
    Dev<double> rho;
    rho.init(ld_b, sentinel());
    TRY(rho.upload());
    launch_rho_deferred(op.deferred(), op.Binv.d, ld_b, (int32_t)m, 0, (int32_t)m, rho.d, op.rec.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(rho.back(rho_out, ld_b)); TRY(op.W.back(W_out, W_out_len)); TRY(op.Binv.back(Binv_out, Binv_out_len));
    return 0;
}

// R4: launch_flush_snapshot + launch_flush_apply + launch_flush_reset, unsharded.  irec: {n_eta, eta_target, n_eta_old}.
int rkh_flush_revised(int64_t m, int64_t p, int64_t kmax, int fill, const double* W, int64_t W_len, const int32_t* S, int64_t S_len,
                      const double* Binv, int64_t Binv_len, double* Binv_out, int64_t Binv_out_len, double* W_out, int64_t W_out_len,
                      double* R_out, int64_t R_out_len, int32_t* pos_out, int64_t pos_out_len, int32_t* S_out, int64_t S_out_len,
                      int32_t* irec, int64_t irec_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, 1, p, kmax), kRefusedShape);
    const int64_t ld_b = round_up(m, 16);
    REFUSE_LEN(W_len, p * m); REFUSE_LEN(S_len, p); REFUSE_LEN(Binv_len, m * m);
    REFUSE_LEN(Binv_out_len, m * ld_b); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R_out_len, kmax * ld_b);
    REFUSE_LEN(pos_out_len, m); REFUSE_LEN(S_out_len, kmax); REFUSE_LEN(irec_len, 3);
    REFUSE_IF(rows_refused(S, p, m), kRefusedIndex);
    PivotRecord R = blank_record();
    R.n_eta = (int32_t)p; R.n_eta_old = (int32_t)p; R.eta_target = (int32_t)(p > 0 ? p - 1 : 0);
    RevOperands op;
    TRY(op.build(m, p, kmax, fill, W, S, Binv, true, R));
    const DeferredUpdate du = op.deferred();
    if (kmax > 0) launch_flush_snapshot(du, op.Binv.d, ld_b, 0, (int32_t)m, op.rec.d, 0);
    launch_flush_apply(du, op.Binv.d, ld_b, (int32_t)m, 0, (int32_t)m, op.rec.d, 0);
    launch_flush_reset(du, op.rec.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(op.Binv.back(Binv_out, Binv_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R.back(R_out, R_out_len));
    TRY(op.pos.back(pos_out, m)); TRY(op.S.back(S_out, kmax));
    PivotRecord Ro;
    TRY(op.rec.back(&Ro, 1));
    irec[0] = Ro.n_eta; irec[1] = Ro.eta_target; irec[2] = Ro.n_eta_old;
    return 0;
}

// R5: launch_compute_rho + launch_update_inverse, unsharded, for pivot row r with alpha_r = alpha[r].
int rkh_explicit_update(int64_t m, int64_t r, int fill, const double* alpha, int64_t alpha_len, const double* Binv, int64_t Binv_len,
                        double* rho_out, int64_t rho_out_len, double* Binv_out, int64_t Binv_out_len, double* alpha_out,
                        int64_t alpha_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(m < 1, kRefusedShape);
    REFUSE_IF(r < 0 || r >= m, kRefusedIndex);
    const int64_t ld_b = round_up(m, 16);
    REFUSE_LEN(alpha_len, m); REFUSE_LEN(Binv_len, m * m);
    REFUSE_LEN(rho_out_len, ld_b); REFUSE_LEN(Binv_out_len, m * ld_b); REFUSE_LEN(alpha_out_len, ld_b);
    PivotRecord R = blank_record();
    R.r = (int32_t)r; R.alpha_r = alpha[r];
    Dev<double> al, rho, binv;
    Dev<PivotRecord> rec;
    al.init(ld_b, fill ? sentinel() : 0.0);
    for (int64_t i = 0; i < m; ++i) al.h[(size_t)i] = alpha[i];
    rho.init(ld_b, sentinel());
    pad_rows(binv.h, Binv, m, m, ld_b, m, 0.0);
    rec.init(1, R);
    TRY(al.upload()); TRY(rho.upload()); TRY(binv.upload()); TRY(rec.upload());
    launch_compute_rho(binv.d, ld_b, (int32_t)m, 0, (int32_t)m, rho.d, rec.d, 0);
    launch_update_inverse(binv.d, ld_b, (int32_t)m, 0, (int32_t)m, al.d, rho.d, rec.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(rho.back(rho_out, ld_b)); TRY(binv.back(Binv_out, Binv_out_len)); TRY(al.back(alpha_out, ld_b));
    return 0;
}

}  // extern "C"

// ---- T5 - T8: the in-place changes and the batched ratio queries (relp_kernels_tableau.hip: k_tab_rhs_*, k_tab_cost_*,
// k_tab_row_ratios*, k_tab_rhs_ranging*).  These take a view with a column offset: tv.n = n_store - col_off tableau columns,
// in_basis indexed by tableau column.  d_in holds the owned columns' d; the image has n_store entries, sentinel below c_lo.
namespace {

constexpr int64_t kScratchTail = 64;   // sentinel words behind the partial minima of T7 / T8

TableauView view_at(const TabOperands& op, double* d, int64_t col_off) {
    TableauView tv = op.view(d);
    tv.col_off = (int32_t)col_off; tv.n = (int32_t)(op.c_lo + op.n - col_off);
    return tv;
}

PivotRecord pending_record(int64_t p) {
    PivotRecord R = blank_record();
    R.n_eta = (int32_t)p; R.n_eta_old = (int32_t)p; R.p_now = (int32_t)p;
    return R;
}

bool list_refused(const int32_t* list, int64_t count, int64_t lo, int64_t hi, bool ascending) {
    for (int64_t k = 0; k < count; ++k) {
        if (list[k] < lo || list[k] >= hi) return true;
        if (ascending && k > 0 && list[k] <= list[k - 1]) return true;
    }
    return false;
}

bool tol_refused(const double* tol) {   // {pivot, zero, tie}: finite and not negative
    for (int t = 0; t < 3; ++t) if (!(tol[t] >= 0.0) || tol[t] > 1e300) return true;
    return false;
}

Tolerances tolerances(const double* tol) {
    Tolerances t;
    memset(&t, 0, sizeof t);
    t.pivot = tol[0]; t.zero = tol[1]; t.tie = tol[2];
    return t;
}

template <class T>
void fill_from(Dev<T>& dev, int64_t n, T fill, const T* src, int64_t count, int64_t at = 0) {
    dev.init(n, fill);
    for (int64_t k = 0; k < count; ++k) dev.h[(size_t)(at + k)] = src[k];
}

}  // namespace

extern "C" {

// tab_rhs_splits (which = 0, size = m) / tab_cost_splits (which = 1, size = stored columns): host functions, no HIP call
int rkh_tab_splits(int which, int64_t size, int64_t count, int64_t forced, int32_t* out, int64_t out_len) {
    REFUSE_IF(which < 0 || which > 1 || size < 1 || size > (1ll << 30), kRefusedShape);
    REFUSE_IF(count < -(1ll << 30) || count > (1ll << 30) || forced < -(1ll << 30) || forced > (1ll << 30), kRefusedShape);
    REFUSE_LEN(out_len, 1);
    out[0] = which ? tab_cost_splits((int32_t)size, (int32_t)count, (int32_t)forced) : tab_rhs_splits((int32_t)size, (int32_t)count, (int32_t)forced);
    return 0;
}

// T5: launch_tab_rhs_change.  cols: storage columns in [c_lo, c_lo + n_owned), repeats allowed.  Out: b (ld_b), v (kmax),
// partial (splits x ld_b, the engine's ld_partial), the operands and the list.
int rkh_tab_rhs_change(int64_t m, int64_t n_owned, int64_t p, int64_t kmax, int64_t c_lo, int batch, int64_t count, int64_t splits,
                       int fill, const double* T0, int64_t T0_len, const double* W, int64_t W_len, const double* R0, int64_t R0_len,
                       const double* b, int64_t b_len, const int32_t* cols, int64_t cols_len, const double* delta, int64_t delta_len,
                       double* b_out, int64_t b_out_len, double* v_out, int64_t v_out_len, double* partial_out, int64_t partial_out_len,
                       double* T0_out, int64_t T0_out_len, double* W_out, int64_t W_out_len, double* R0_out, int64_t R0_out_len,
                       int32_t* cols_out, int64_t cols_out_len, double* delta_out, int64_t delta_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, n_owned, p, kmax), kRefusedShape);
    REFUSE_IF(c_lo < 0 || c_lo > (1 << 20), kRefusedIndex);
    REFUSE_IF(count < 1 || count > (1 << 20), kRefusedShape);
    REFUSE_IF(splits < 1 || splits > std::min<int64_t>(count, kTabRhsMaxSplits), kRefusedSplits);
    REFUSE_IF(batch_refused(batch), kRefusedBatch);
    const int64_t ld_b = round_up(m, 16), ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2);
    REFUSE_LEN(T0_len, n_owned * m); REFUSE_LEN(W_len, p * m); REFUSE_LEN(R0_len, p * n_owned); REFUSE_LEN(b_len, m);
    REFUSE_LEN(cols_len, count); REFUSE_LEN(delta_len, count);
    REFUSE_LEN(b_out_len, ld_b); REFUSE_LEN(v_out_len, kmax); REFUSE_LEN(partial_out_len, splits * ld_b);
    REFUSE_LEN(T0_out_len, n_owned * ld_t); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R0_out_len, (kmax + 1) * ld_r);
    REFUSE_LEN(cols_out_len, count); REFUSE_LEN(delta_out_len, count);
    REFUSE_IF(list_refused(cols, count, c_lo, c_lo + n_owned, false), kRefusedIndex);
    TabOperands op;
    TRY(op.build(m, n_owned, p, kmax, c_lo, fill, T0, W, R0, pending_record(p)));
    Dev<double> bb, v, partial, dl;
    Dev<int32_t> cl;
    fill_from(bb, ld_b, fill ? sentinel() : 0.0, b, m);
    v.init(kmax, sentinel()); partial.init(splits * ld_b, sentinel());
    fill_from(cl, count, 0, cols, count); fill_from(dl, count, 0.0, delta, count);
    TRY(bb.upload()); TRY(v.upload()); TRY(partial.upload()); TRY(cl.upload()); TRY(dl.upload());
    launch_tab_rhs_change(view_at(op, nullptr, 0), op.deferred(batch), RhsChange{cl.d, dl.d, (int32_t)count}, (int32_t)p, (int32_t)splits,
                          v.d, bb.d, partial.d, ld_b, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(bb.back(b_out, ld_b)); TRY(v.back(v_out, kmax)); TRY(partial.back(partial_out, splits * ld_b));
    TRY(op.T0.back(T0_out, T0_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R0.back(R0_out, R0_out_len));
    TRY(cl.back(cols_out, count)); TRY(dl.back(delta_out, count));
    return 0;
}

// T6: launch_tab_cost_change.  rows: strictly ascending rows of [0, m); ncols: strictly ascending storage columns of
// [c_lo, c_lo + n_owned), none flagged 1; in_basis: n_store - col_off flags (0 / 1 / 2) by tableau column; d: the owned columns.
// count == 0 needs splits == 1 (the launcher forces it).  Out: d (n_store), u (kmax), partial (splits x ld_r, the engine's
// ld_partial; the pointer handed over is shifted by c_lo as T0 and R0 are), the flags, the operands and the lists.
int rkh_tab_cost_change(int64_t m, int64_t n_owned, int64_t p, int64_t kmax, int64_t c_lo, int64_t col_off, int batch, int64_t count,
                        int64_t ncount, int64_t splits, int fill,
                        const double* T0, int64_t T0_len, const double* W, int64_t W_len, const double* R0, int64_t R0_len,
                        const double* d, int64_t d_len, const uint8_t* in_basis, int64_t in_basis_len,
                        const int32_t* rows, int64_t rows_len, const double* delta, int64_t delta_len,
                        const int32_t* ncols, int64_t ncols_len, const double* ndelta, int64_t ndelta_len,
                        double* d_out, int64_t d_out_len, double* u_out, int64_t u_out_len, double* partial_out, int64_t partial_out_len,
                        uint8_t* in_basis_out, int64_t in_basis_out_len,
                        double* T0_out, int64_t T0_out_len, double* W_out, int64_t W_out_len, double* R0_out, int64_t R0_out_len,
                        int32_t* rows_out, int64_t rows_out_len, double* delta_out, int64_t delta_out_len,
                        int32_t* ncols_out, int64_t ncols_out_len, double* ndelta_out, int64_t ndelta_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, n_owned, p, kmax), kRefusedShape);
    REFUSE_IF(c_lo < 0 || c_lo > (1 << 20), kRefusedIndex);
    const int64_t n_all = c_lo + n_owned, n_tab = n_all - col_off;
    REFUSE_IF(col_off < 0 || col_off >= n_all, kRefusedIndex);
    REFUSE_IF(count < 0 || ncount < 0 || count + ncount < 1 || count > (1 << 20) || ncount > (1 << 20), kRefusedShape);
    REFUSE_IF(splits < 1 || splits > std::max<int64_t>(1, std::min<int64_t>(count, kTabCostMaxSplits)), kRefusedSplits);
    REFUSE_IF(batch_refused(batch), kRefusedBatch);
    const int64_t ld_b = round_up(m, 16), ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2);
    REFUSE_LEN(T0_len, n_owned * m); REFUSE_LEN(W_len, p * m); REFUSE_LEN(R0_len, p * n_owned); REFUSE_LEN(d_len, n_owned);
    REFUSE_LEN(in_basis_len, n_tab); REFUSE_LEN(rows_len, count); REFUSE_LEN(delta_len, count); REFUSE_LEN(ncols_len, ncount);
    REFUSE_LEN(ndelta_len, ncount);
    REFUSE_LEN(d_out_len, n_all); REFUSE_LEN(u_out_len, kmax); REFUSE_LEN(partial_out_len, splits * ld_r); REFUSE_LEN(in_basis_out_len, n_tab);
    REFUSE_LEN(T0_out_len, n_owned * ld_t); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R0_out_len, (kmax + 1) * ld_r);
    REFUSE_LEN(rows_out_len, count); REFUSE_LEN(delta_out_len, count); REFUSE_LEN(ncols_out_len, ncount); REFUSE_LEN(ndelta_out_len, ncount);
    REFUSE_IF(list_refused(rows, count, 0, m, false) || list_refused(ncols, ncount, c_lo, n_all, false), kRefusedIndex);
    REFUSE_IF(list_refused(rows, count, 0, m, true) || list_refused(ncols, ncount, c_lo, n_all, true), kRefusedOrder);
    for (int64_t j = 0; j < n_tab; ++j) REFUSE_IF(in_basis[j] > 2, kRefusedIndex);
    for (int64_t k = 0; k < ncount; ++k) REFUSE_IF(ncols[k] >= col_off && in_basis[ncols[k] - col_off] == 1, kRefusedOrder);
    TabOperands op;
    TRY(op.build(m, n_owned, p, kmax, c_lo, fill, T0, W, R0, pending_record(p)));
    Dev<double> dd, u, partial, dl, ndl;
    Dev<int32_t> rw, ncl;
    Dev<uint8_t> inb;
    fill_from(dd, n_all, sentinel(), d, n_owned, c_lo);
    u.init(kmax, sentinel()); partial.init(splits * ld_r, sentinel());
    fill_from(inb, n_tab, (uint8_t)0, in_basis, n_tab);
    fill_from(rw, count, 0, rows, count); fill_from(dl, count, 0.0, delta, count);
    fill_from(ncl, ncount, 0, ncols, ncount); fill_from(ndl, ncount, 0.0, ndelta, ncount);
    TRY(dd.upload()); TRY(u.upload()); TRY(partial.upload()); TRY(inb.upload()); TRY(rw.upload()); TRY(dl.upload()); TRY(ncl.upload());
    TRY(ndl.upload());
    launch_tab_cost_change(view_at(op, dd.d, col_off), op.deferred(batch),
                           CostChange{rw.d, dl.d, (int32_t)count, ncl.d, ndl.d, (int32_t)ncount}, inb.d, (int32_t)p, (int32_t)splits, u.d,
                           partial.d - c_lo, ld_r, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(dd.back(d_out, n_all)); TRY(u.back(u_out, kmax)); TRY(partial.back(partial_out, splits * ld_r)); TRY(inb.back(in_basis_out, n_tab));
    TRY(op.T0.back(T0_out, T0_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R0.back(R0_out, R0_out_len));
    TRY(rw.back(rows_out, count)); TRY(dl.back(delta_out, count)); TRY(ncl.back(ncols_out, ncount)); TRY(ndl.back(ndelta_out, ncount));
    return 0;
}

// T7: launch_tab_row_ratios.  rows: any order, repeats allowed; tol: {pivot, zero, tie}.  Out: ratio / column (2 x count,
// pre-filled with the sentinels), the scratch part_k / part_j (2 x count x scan blocks, then kScratchTail sentinel words), d
// (n_store), the flags, the operands and the list.
int rkh_tab_row_ratios(int64_t m, int64_t n_owned, int64_t p, int64_t kmax, int64_t c_lo, int64_t col_off, int batch, int64_t count,
                       int fill, const double* tol, int64_t tol_len,
                       const double* T0, int64_t T0_len, const double* W, int64_t W_len, const double* R0, int64_t R0_len,
                       const double* d, int64_t d_len, const uint8_t* in_basis, int64_t in_basis_len, const int32_t* rows, int64_t rows_len,
                       double* ratio_out, int64_t ratio_out_len, int32_t* column_out, int64_t column_out_len,
                       double* part_k_out, int64_t part_k_out_len, int32_t* part_j_out, int64_t part_j_out_len,
                       double* d_out, int64_t d_out_len, uint8_t* in_basis_out, int64_t in_basis_out_len,
                       double* T0_out, int64_t T0_out_len, double* W_out, int64_t W_out_len, double* R0_out, int64_t R0_out_len,
                       int32_t* rows_out, int64_t rows_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, n_owned, p, kmax), kRefusedShape);
    REFUSE_IF(c_lo < 0 || c_lo > (1 << 20), kRefusedIndex);
    const int64_t n_all = c_lo + n_owned, n_tab = n_all - col_off;
    REFUSE_IF(col_off < 0 || col_off >= n_all, kRefusedIndex);
    REFUSE_IF(count < 1 || count > (1 << 16), kRefusedShape);
    REFUSE_IF(batch_refused(batch), kRefusedBatch);
    REFUSE_LEN(tol_len, 3);
    REFUSE_IF(tol_refused(tol), kRefusedShape);
    const int64_t ld_b = round_up(m, 16), ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2);
    const int64_t scratch = 2 * count * tab_scan_blocks((int32_t)n_owned) + kScratchTail;
    REFUSE_LEN(T0_len, n_owned * m); REFUSE_LEN(W_len, p * m); REFUSE_LEN(R0_len, p * n_owned); REFUSE_LEN(d_len, n_owned);
    REFUSE_LEN(in_basis_len, n_tab); REFUSE_LEN(rows_len, count);
    REFUSE_LEN(ratio_out_len, 2 * count); REFUSE_LEN(column_out_len, 2 * count); REFUSE_LEN(part_k_out_len, scratch);
    REFUSE_LEN(part_j_out_len, scratch); REFUSE_LEN(d_out_len, n_all); REFUSE_LEN(in_basis_out_len, n_tab);
    REFUSE_LEN(T0_out_len, n_owned * ld_t); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R0_out_len, (kmax + 1) * ld_r);
    REFUSE_LEN(rows_out_len, count);
    REFUSE_IF(list_refused(rows, count, 0, m, false), kRefusedIndex);
    for (int64_t j = 0; j < n_tab; ++j) REFUSE_IF(in_basis[j] > 2, kRefusedIndex);
    TabOperands op;
    TRY(op.build(m, n_owned, p, kmax, c_lo, fill, T0, W, R0, pending_record(p)));
    Dev<double> dd, pk, ratio;
    Dev<int32_t> pj, column, rw;
    Dev<uint8_t> inb;
    fill_from(dd, n_all, sentinel(), d, n_owned, c_lo);
    fill_from(inb, n_tab, (uint8_t)0, in_basis, n_tab);
    fill_from(rw, count, 0, rows, count);
    pk.init(scratch, sentinel()); pj.init(scratch, kSentinelInt); ratio.init(2 * count, sentinel()); column.init(2 * count, kSentinelInt);
    TRY(dd.upload()); TRY(inb.upload()); TRY(rw.upload()); TRY(pk.upload()); TRY(pj.upload()); TRY(ratio.upload()); TRY(column.upload());
    SelectPartials sp;
    memset(&sp, 0, sizeof sp);
    sp.in_basis = inb.d; sp.n = (int32_t)n_tab; sp.cols_per_slot = 8;
    launch_tab_row_ratios(view_at(op, dd.d, col_off), op.deferred(batch), sp, tolerances(tol), rw.d, (int32_t)count, (int32_t)p, pk.d, pj.d,
                          ratio.d, column.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(ratio.back(ratio_out, 2 * count)); TRY(column.back(column_out, 2 * count)); TRY(pk.back(part_k_out, scratch));
    TRY(pj.back(part_j_out, scratch)); TRY(dd.back(d_out, n_all)); TRY(inb.back(in_basis_out, n_tab));
    TRY(op.T0.back(T0_out, T0_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R0.back(R0_out, R0_out_len));
    TRY(rw.back(rows_out, count));
    return 0;
}

// T8: launch_tab_rhs_ranging.  cols: storage columns of [c_lo, c_lo + n_owned), any order, repeats allowed; basis: m distinct
// leaving columns >= 0 (wrapped artificials from kWrappedArtificialBase).  Out: ratio / row (2 x count), the scratch part
// (2 x count x cdiv(m, 256), then kScratchTail sentinel words), b (ld_b), the basis, the operands and the list.
int rkh_tab_rhs_ranging(int64_t m, int64_t n_owned, int64_t p, int64_t kmax, int64_t c_lo, int batch, int64_t count, int fill,
                        const double* tol, int64_t tol_len,
                        const double* T0, int64_t T0_len, const double* W, int64_t W_len, const double* R0, int64_t R0_len,
                        const double* b, int64_t b_len, const int32_t* basis, int64_t basis_len, const int32_t* cols, int64_t cols_len,
                        double* ratio_out, int64_t ratio_out_len, int32_t* row_out, int64_t row_out_len,
                        double* part_out, int64_t part_out_len, double* b_out, int64_t b_out_len, int32_t* basis_out, int64_t basis_out_len,
                        double* T0_out, int64_t T0_out_len, double* W_out, int64_t W_out_len, double* R0_out, int64_t R0_out_len,
                        int32_t* cols_out, int64_t cols_out_len) {
    if (g_sticky) return g_sticky;
    REFUSE_IF(shape_refused(m, n_owned, p, kmax), kRefusedShape);
    REFUSE_IF(c_lo < 0 || c_lo > (1 << 20), kRefusedIndex);
    REFUSE_IF(count < 1 || count > (1 << 16), kRefusedShape);
    REFUSE_IF(batch_refused(batch), kRefusedBatch);
    REFUSE_LEN(tol_len, 3);
    REFUSE_IF(tol_refused(tol), kRefusedShape);
    const int64_t ld_b = round_up(m, 16), ld_t = round_up(m, 2), ld_r = round_up(n_owned, 2);
    const int64_t scratch = 2 * count * ((m + 255) / 256) + kScratchTail;
    REFUSE_LEN(T0_len, n_owned * m); REFUSE_LEN(W_len, p * m); REFUSE_LEN(R0_len, p * n_owned); REFUSE_LEN(b_len, m);
    REFUSE_LEN(basis_len, m); REFUSE_LEN(cols_len, count);
    REFUSE_LEN(ratio_out_len, 2 * count); REFUSE_LEN(row_out_len, 2 * count); REFUSE_LEN(part_out_len, scratch);
    REFUSE_LEN(b_out_len, ld_b); REFUSE_LEN(basis_out_len, m);
    REFUSE_LEN(T0_out_len, n_owned * ld_t); REFUSE_LEN(W_out_len, kmax * ld_b); REFUSE_LEN(R0_out_len, (kmax + 1) * ld_r);
    REFUSE_LEN(cols_out_len, count);
    REFUSE_IF(list_refused(cols, count, c_lo, c_lo + n_owned, false), kRefusedIndex);
    {
        std::vector<int32_t> sorted(basis, basis + m);
        std::sort(sorted.begin(), sorted.end());
        REFUSE_IF(sorted[0] < 0, kRefusedIndex);
        for (int64_t i = 1; i < m; ++i) REFUSE_IF(sorted[(size_t)i] == sorted[(size_t)i - 1], kRefusedOrder);
    }
    TabOperands op;
    TRY(op.build(m, n_owned, p, kmax, c_lo, fill, T0, W, R0, pending_record(p)));
    Dev<double> bb, part, ratio;
    Dev<int32_t> bas, row, cl;
    fill_from(bb, ld_b, fill ? sentinel() : 0.0, b, m);
    fill_from(bas, m, 0, basis, m);
    fill_from(cl, count, 0, cols, count);
    part.init(scratch, sentinel()); ratio.init(2 * count, sentinel()); row.init(2 * count, kSentinelInt);
    TRY(bb.upload()); TRY(bas.upload()); TRY(cl.upload()); TRY(part.upload()); TRY(ratio.upload()); TRY(row.upload());
    launch_tab_rhs_ranging(view_at(op, nullptr, 0), op.deferred(batch), bb.d, bas.d, tolerances(tol), cl.d, (int32_t)count, (int32_t)p, part.d,
                           ratio.d, row.d, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    TRY(ratio.back(ratio_out, 2 * count)); TRY(row.back(row_out, 2 * count)); TRY(part.back(part_out, scratch));
    TRY(bb.back(b_out, ld_b)); TRY(bas.back(basis_out, m));
    TRY(op.T0.back(T0_out, T0_out_len)); TRY(op.W.back(W_out, W_out_len)); TRY(op.R0.back(R0_out, R0_out_len));
    TRY(cl.back(cols_out, count));
    return 0;
}

}  // extern "C"
