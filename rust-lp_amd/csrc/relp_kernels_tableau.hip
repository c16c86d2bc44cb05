// relp_kernels_tableau.hip -- kernels of the dense-tableau engine (RELP_ENGINE_TABLEAU), including the
// f64-MFMA flush T0 += W R0.
#include "relp_device_common.h"
#include <type_traits>

namespace relp {

// ------------------------------------------------------------------------------------------------
// Dense-tableau engine:  T = (I + W S') T0  (see TableauView / DeferredUpdate in relp_kernels.h)
//   PRICE  = one row of T per pivot:   d <- d - (d_q / alpha_r) T[r,:]      (instead of 8 m n_s bytes)
//   FTRAN  = one column of T per pivot: alpha = T0[:,q] + W R0[:,q]        (instead of 8 m^2 bytes)
//   UPDATE = W <- E W per pivot; T0 += W R0 once per K pivots on the f64 matrix cores
// ------------------------------------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));

// The walk over the p pending rows of an update block: use(j, base[j * stride + x]) for j = 0 .. n-1 in ascending order, the
// loads B at a time.  The B elements of a batch are loaded into registers before any of them is used or stored, so the
// loads leave back to back and one descending vmcnt ladder follows: a thread makes ceil(n / B) serial round trips to
// L2 / Infinity Cache instead of n (a store in `use`, or a load the compiler cannot prove independent of it, otherwise
// closes every round trip before the next one opens).  The tail batch is masked: nothing at or past row n is read.
// `use` may store to the element it was given and to nothing else of the walked range (j * stride + x is a different
// address for every j when stride > 0).  B = 1 is the plain loop.
template <int B, class Use>
__device__ __forceinline__ void for_pending(const double* base, int64_t stride, int64_t x, int n, Use&& use) {
    int j0 = 0;
    for (; j0 + B <= n; j0 += B) {
        double v[B];
#pragma unroll
        for (int t = 0; t < B; ++t) v[t] = base[(int64_t)(j0 + t) * stride + x];
#pragma unroll
        for (int t = 0; t < B; ++t) use(j0 + t, v[t]);
    }
    if (B > 1 && j0 < n) {
        double v[B];
#pragma unroll
        for (int t = 0; t < B; ++t) v[t] = j0 + t < n ? base[(int64_t)(j0 + t) * stride + x] : 0.0;
#pragma unroll
        for (int t = 0; t < B; ++t)
            if (j0 + t < n) use(j0 + t, v[t]);
    }
}

// The staged walk over entries [lo, hi) of a list (an index and V coefficients per entry) by a block of 256 threads, each with
// V chains of its own:  acc[v] = fma(coefficient v of entry e, load(index of entry e), acc[v])  for e = lo .. hi-1, ascending.
//   Chunks: 256 entries at a time go into the caller's LDS arrays s_idx / s_coef, entry base + t by thread t through index(e) and
//   coef(e, dst) (dst = the V LDS slots of that entry; coef forms its source address once).  Two barriers per chunk: the first one
//   stands in front of the staging, because until every thread has passed it some may still be reading the previous chunk; the
//   second one publishes the chunk.  Every thread of the block takes part in both, `mine` or not: a thread that is not `mine`
//   stages its entry and loads nothing.  An empty range passes no barrier: a kernel that staged something of its own before the
//   walk publishes it with a barrier of its own after the walk.
//   Batches: the B loads of a batch are issued into registers before any of them is used, as in for_pending, so a thread makes
//   ceil(n / B) round trips per chunk of n entries.  The tail batch is masked: nothing at or past the end of the range is read or
//   used, so neither an index nor a coefficient behind hi is ever touched.  B = 1 is the plain loop.
// The order of every chain is the entry order, whatever B, the chunking and V are.
template <int B, int V, class Index, class Coef, class Load>
__device__ __forceinline__ void for_list(int lo, int hi, int32_t* s_idx, double (*s_coef)[V], Index&& index, Coef&& coef, Load&& load,
                                         bool mine, double (&acc)[V]) {
    for (int base = lo; base < hi; base += kThreads) {
        __syncthreads();                               // (the previous chunk has been read)
        const int n = min(kThreads, hi - base);
        if ((int)threadIdx.x < n) {
            s_idx[threadIdx.x] = index(base + threadIdx.x);
            coef(base + threadIdx.x, s_coef[threadIdx.x]);
        }
        __syncthreads();
        if (!mine) continue;
        int e0 = 0;
        for (; e0 + B <= n; e0 += B) {
            double t[B];
#pragma unroll
            for (int x = 0; x < B; ++x) t[x] = load(s_idx[e0 + x]);
#pragma unroll
            for (int x = 0; x < B; ++x)
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] = fma(s_coef[e0 + x][v], t[x], acc[v]);
        }
        if (e0 < n) {
            double t[B];
#pragma unroll
            for (int x = 0; x < B; ++x) t[x] = e0 + x < n ? load(s_idx[e0 + x]) : 0.0;
#pragma unroll
            for (int x = 0; x < B; ++x)
                if (e0 + x < n) {
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[v] = fma(s_coef[e0 + x][v], t[x], acc[v]);
                }
        }
    }
}

// The list reduction of a block of 256 threads:  sum_k coef(k) * value(k)  over k = 0 .. n-1.  Thread t chains its entries
// k = t, t + 256, ... in ascending order (acc = fma(coef(k), value(k), acc) from 0.0), then a fixed halving tree over the 256
// chains in s_sum: s_sum[t] += s_sum[t + half] for half = 128, 64, .. 1.  Returns s_sum[0]; thread 0 writes it out.  (Not
// block_reduce_value: that one reduces by wave shuffles in another order, and the order is the specification here.)
template <class Coef, class Value>
__device__ __forceinline__ double list_sum(int n, double* s_sum, Coef&& coef, Value&& value) {
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += kThreads) acc = fma(coef(k), value(k), acc);
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_sum[threadIdx.x] += s_sum[threadIdx.x + half];
        __syncthreads();
    }
    return s_sum[0];
}

// The stored column c carries the flag basic (1): the pivot update pins its d at exactly 0.  A barred column (2) and every stored
// column outside [col_off, col_off + n) (the kept artificial block in front of col_off) do not.
__device__ __forceinline__ bool column_flagged_basic(const TableauView& tv, const uint8_t* __restrict__ in_basis, int c) {
    const int j = c - tv.col_off;
    return j >= 0 && j < tv.n && in_basis[j] == 1;
}

// Row r of W (its p pending entries) into s_w, one entry per thread; the caller's next barrier publishes it.
__device__ __forceinline__ void stage_w_row(const DeferredUpdate& du, int r, int p, double* s_w) {
    if ((int)threadIdx.x < p) s_w[threadIdx.x] = du.W[(int64_t)threadIdx.x * du.ld + r];
}

// T[r,c] = base + sum_j W[j][r] R0[j][c] over the p pending rows, ascending j.  s_w = row r of W (stage_w_row); base =
// T0[c * ld_t + r], or row r's slot of R0, loaded by the caller where it wants that load to leave.
template <int B>
__device__ __forceinline__ double tab_row_entry(const TableauView& tv, int c, int p, const double* s_w, double base) {
    for_pending<B>(tv.R0, tv.ld_r, c, p, [&](int j, double r0) { base = fma(s_w[j], r0, base); });
    return base;
}

// alpha_i = t0 + sum_j W[j][i] R0[j][cq] over the p pending rows, ascending j.  s_vs = column cq of R0, staged by the caller;
// t0 = T0[cq * ld_t + i], loaded by the caller where it wants that load to leave.
template <int B>
__device__ __forceinline__ double tab_column_entry(const DeferredUpdate& du, int i, int p, const double* s_vs, double t0) {
    for_pending<B>(du.W, du.ld, i, p, [&](int j, double w) { t0 = fma(w, s_vs[j], t0); });
    return t0;
}

// W <- E W for row i: W[j][i] = fma(u, w_r[j], W[j][i]) for the pending rows j0 <= j < j1, where neither factor is zero
// (fma(u, 0.0, -0.0) is +0.0: an entry a zero factor would leave alone keeps its bits).
template <int B>
__device__ __forceinline__ void tab_update_w_row(const DeferredUpdate& du, int i, double u, const double* s_wr, int j0, int j1) {
    if (u == 0.0 || j1 <= j0) return;
    double* col = du.W + (int64_t)j0 * du.ld;
    for_pending<B>(col, du.ld, i, j1 - j0, [&](int j, double old) {
        const double w = s_wr[j0 + j];
        if (w != 0.0) col[(int64_t)j * du.ld + i] = fma(u, w, old);
    });
}

__global__ void k_tab_build(TableauView tv, const double* __restrict__ A, int64_t ld_a, ColumnTable ct) {
    const int64_t total = (int64_t)tv.m * (tv.c_hi - tv.c_lo);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int c = tv.c_lo + (int)(idx / tv.m), i = (int)(idx % tv.m);
        double v = 0.0;
        if (c < ct.nr_artificial) {
            v = (i == ct.column_to_row[c]) ? 1.0 : 0.0;
        } else {
            const int p = c - ct.nr_artificial;
            if (p < ct.nr_normal) {
                if (i < ct.nr_constraints) v = A[(int64_t)p * ld_a + i];
                else v = (i == ct.bound_row[p]) ? 1.0 : 0.0;
            } else {
                const int vv = p - ct.nr_normal;
                if (i == ct.vrow0[vv]) v = (double)ct.vsign[vv];
                else if (i == ct.vrow1[vv]) v = 1.0;
            }
        }
        tv.T0[(int64_t)c * tv.ld_t + i] = v;
    }
}

// d[c] = cost[c] - w . T0[:,c]   (the PRICE multi-dot over the stored tableau, phase boundaries only)
__global__ __launch_bounds__(kThreads) void k_tab_price_init(TableauView tv, const double* __restrict__ w,
                                                             const double* __restrict__ cost_store) {
    __shared__ double s_partial[4 * kVecPerBlock];
    const int v0 = tv.c_lo + blockIdx.x * kVecPerBlock;
    double dot = 0.0;
    block_multi_dot(tv.T0, tv.ld_t, tv.m, v0, tv.c_hi, w, s_partial, dot);
    const int c = v0 + threadIdx.x;
    if (threadIdx.x < kVecPerBlock && c < tv.c_hi) tv.d[c] = cost_store[c] - dot;
}

// w[i] = cost of the variable that is basic in row i (current phase), for re-pricing d from T0
__global__ void k_tab_basis_costs(const int32_t* __restrict__ basis_indices, const double* __restrict__ cost_store,
                                  int col_off, int n_store, int m, double* __restrict__ w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int j = basis_indices[i];
    const int c = j + col_off;
    w[i] = (j < kWrappedArtificialBase && c >= 0 && c < n_store) ? cost_store[c] : 0.0;
}

// one slot per 256 storage columns
__global__ __launch_bounds__(kThreads) void k_tab_scan(TableauView tv, SelectPartials sp, const PivotRecord* rec) {
    if (rec->outcome != DEV_RUNNING) return;
    const int c = tv.c_lo + blockIdx.x * kThreads + threadIdx.x;
    const int j = c - tv.col_off;
    double key = INFINITY;
    int kj = 0x7fffffff;
    if (c < tv.c_hi && j >= 0 && j < tv.n) {
        const double v = tv.d[c];
        if (!sp.in_basis[j] && v < -sp.tol_cost) { key = select_key(sp.rule, sp.n, rec, j, v); kj = j; }
    }
    block_partial_min(key, kj, sp, blockIdx.x);
}

__global__ __launch_bounds__(kSingleBlock) void k_tab_select(TableauView tv, SelectPartials sp, int count,
                                                             PivotRecord* rec) {
    if (rec->outcome != DEV_RUNNING) return;
    double k1 = INFINITY;
    int bj = 0x7fffffff;
    if ((int)threadIdx.x < count) { k1 = sp.k1[threadIdx.x]; bj = sp.j[threadIdx.x]; }
    tab_select_entering<kSingleBlock>(tv, sp, count, k1, bj);
    if (threadIdx.x == 0) {
        if (bj == 0x7fffffff) {
            rec->outcome = DEV_NO_CANDIDATE;
            if (sp.rule == 1) rec->last_selected = -1;
        } else {
            rec->q = bj;
            rec->d_q = tv.d[bj + tv.col_off];
            rec->key1 = k1;
            if (sp.rule == 1) rec->last_selected = bj;
        }
    }
}

// alpha = T[:,q] = T0[:,q] + W (R0[:,q])
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_column(TableauView tv, DeferredUpdate du, double* __restrict__ alpha,
                                                         const PivotRecord* rec) {
    if (rec->outcome != DEV_RUNNING) return;
    __shared__ double s_vs[kMaxEta];
    const int p = rec->n_eta;
    const int cq = rec->q + tv.col_off;
    if ((int)threadIdx.x < p) s_vs[threadIdx.x] = tv.R0[(int64_t)threadIdx.x * tv.ld_r + cq];
    __syncthreads();
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= tv.m) return;
    alpha[i] = tab_column_entry<B>(du, i, p, s_vs, tv.T0[(int64_t)cq * tv.ld_t + i]);
}

// Row r of T before the pivot, the reduced-cost update and the next PRICE's partial argmin in one
// pass over the stored columns.  When row r is new in the block its T0 row is appended to R0 here.
// `block` = index of this workgroup among the row-update workgroups.
// `R` is the workgroup's snapshot of the PivotRecord (one cache line, fetched once at kernel start: reading
// it field by field between stores costs a dependent memory round trip each time).
// `wr` (shared memory) = row r of W before this pivot; the pivot itself as plain arguments (the fused launch computes them
// per workgroup, the others take them from the record).  `R` is only read for the selection key's rule memory.
template <int B>
__device__ __forceinline__ void tab_row_update_core(const TableauView& tv, const DeferredUpdate& du, const SelectPartials& sp,
                                                    const PivotRecord& R, int block, const double* s_wr, int p_old, int jt, int r,
                                                    int q, int leaving, double d_q, double alpha_r) {
    const PivotRecord* rec = &R;
    const int c = tv.c_lo + block * kThreads + threadIdx.x;
    const double d_old = c < tv.c_hi ? tv.d[c] : 0.0;
    __syncthreads();
    double key = INFINITY;
    int kj = 0x7fffffff;
    if (c < tv.c_hi) {
        double base;
        if (jt < p_old) base = tv.R0[(int64_t)jt * tv.ld_r + c];
        else {
            // row r is new in this block: its row of the tableau the block started from
            base = tv.T0[(int64_t)c * tv.ld_t + r];
            tv.R0[(int64_t)jt * tv.ld_r + c] = base;
        }
        const double row = tab_row_entry<B>(tv, c, p_old, s_wr, base);
        const double theta = d_q / alpha_r;
        const int j = c - tv.col_off;
        double dn = fma(-theta, row, d_old);
        if (j == q) dn = 0.0;
        tv.d[c] = dn;
        if (j >= 0 && j < tv.n) {
            // correct for old AND new flags (the flags may be flipped concurrently by the W/vector part)
            const bool basic = (j == q) || (sp.in_basis[j] && j != leaving);
            if (!basic && dn < -sp.tol_cost) { key = select_key(sp.rule, sp.n, rec, j, dn); kj = j; }
        }
    }
    block_partial_min(key, kj, sp, block);
}

template <int B>
__device__ __forceinline__ void tab_row_update_body(const TableauView& tv, const DeferredUpdate& du,
                                                    const SelectPartials& sp, const PivotRecord& R, int block) {
    __shared__ double s_wr[kMaxEta];
    // fetched without waiting for p_old (entries beyond it are never used)
    if ((int)threadIdx.x < du.kmax) s_wr[threadIdx.x] = du.wr[threadIdx.x];
    tab_row_update_core<B>(tv, du, sp, R, block, s_wr, R.n_eta_old, R.eta_target, R.r, R.q, R.leaving, R.d_q, R.alpha_r);
}

template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_row_update(TableauView tv, DeferredUpdate du, SelectPartials sp,
                                                             PivotRecord* rec) {
    const PivotRecord R = *rec;
    if (R.outcome != DEV_RUNNING) return;
    tab_row_update_body<B>(tv, du, sp, R, blockIdx.x);
}

// W <- E W  and  b, -obj, basis, flags, trace (both walk the m rows)
template <int B>
__device__ __forceinline__ void tab_update_w_vectors_body(const DeferredUpdate& du, int m, const double* __restrict__ alpha,
                                                          double* __restrict__ b, int32_t* __restrict__ basis_indices,
                                                          uint8_t* __restrict__ in_basis, int32_t* __restrict__ trace,
                                                          int64_t trace_cap, const PivotRecord& R, PivotRecord* rec,
                                                          int block) {
    __shared__ double s_wr2[kMaxEta];
    const int p_old = R.n_eta_old, jt = R.eta_target, r = R.r;
    if ((int)threadIdx.x < du.kmax) s_wr2[threadIdx.x] = du.wr[threadIdx.x];
    const int i = block * kThreads + threadIdx.x;
    const double a_i = i < m ? alpha[i] : 0.0;
    const double b_i = i < m ? b[i] : 0.0;
    __syncthreads();
    const double ar = R.alpha_r;
    const double br = R.b_r / ar;
    if (i < m) {
        const double a = a_i;
        const double u = (i == r) ? (1.0 / ar - 1.0) : (-a / ar);
        tab_update_w_row<B>(du, i, u, s_wr2, 0, p_old);
        double* tgt = du.W + (int64_t)jt * du.ld + i;
        if (jt < p_old) *tgt += u; else *tgt = u;
        b[i] = pivot_b(a, b_i, br, i == r);
    }
    if (i == 0) {
        basis_indices[r] = R.q;
        pivot_bookkeeping(R.phase, R.iterations, R.minus_objective, R.d_q, br, R.q, r, R.leaving, in_basis, trace, trace_cap, rec);
    }
}

// Both halves of the update in ONE launch: workgroups [0, nb_row) update the tableau row / reduced
// costs / PRICE partials of their columns, workgroups [nb_row, ..) update W, b and the bookkeeping.
// The halves touch disjoint data; the basis flags flipped by the second half are read by the first
// through an expression that is the same for the old and the new flags.
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_update_all(TableauView tv, DeferredUpdate du, SelectPartials sp,
                                                             int nb_row, int m, const double* __restrict__ alpha,
                                                             double* __restrict__ b, int32_t* __restrict__ basis_indices,
                                                             uint8_t* __restrict__ in_basis, int32_t* __restrict__ trace,
                                                             int64_t trace_cap, PivotRecord* rec) {
    const PivotRecord R = *rec;
    if (R.outcome != DEV_RUNNING) return;
    if ((int)blockIdx.x < nb_row) tab_row_update_body<B>(tv, du, sp, R, blockIdx.x);
    else tab_update_w_vectors_body<B>(du, m, alpha, b, basis_indices, in_basis, trace, trace_cap, R, rec, blockIdx.x - nb_row);
}

// Ratio test + both halves of the update in ONE launch (relp_kernels.h: launch_tab_ratio_update_all).  Workgroups
// [0, nb_row): tableau row / reduced costs / PRICE partials; [nb_row, ..): W, b, basis, bookkeeping.  Every workgroup repeats
// the ratio test (ratio_blocks_pick: same inputs, same code, same row) and fetches row r of W, alpha_r, b_r and the slot of
// row r itself.  Nothing a workgroup reads is rewritten by another one in this launch: b and the basis array go in -> out,
// the new row r of W goes to `shadow`, n_eta is read as p_now; the basis flags are read through the expression that is
// the same for old and new flags; pos_of_row[r] reads as -1 or as the value it is about to get.  Same arithmetic as
// k_ratio_blocks + k_tab_update_all, bit for bit.
// `rmin` holds nblk minima, one per RPB rows (what the column kernel walked per workgroup); the W half keeps blocks of 256 rows,
// nb_w of them (RPB = 256: nblk of them).
// `split` > 1: the W half has split * nb_w workgroups, and workgroup part * nb_w + wblock updates the rows of block wblock in
// its share of the pending columns of W (the m x p entries are independent of each other).  Part 0 alone keeps b, the
// basis array, the shadow row and the record; column jt gets its u from the part that holds it.
template <int B, int RPB>
__global__ __launch_bounds__(kThreads) void k_tab_ratio_update_all(TableauView tv, DeferredUpdate du, SelectPartials sp, int nb_row,
                                                                   int m, const double* alpha,
                                                                   const double* __restrict__ b_in, double* __restrict__ b_out,
                                                                   const int32_t* __restrict__ basis_in,
                                                                   int32_t* __restrict__ basis_out, uint8_t* in_basis,
                                                                   int32_t* __restrict__ trace, int64_t trace_cap, Tolerances tol,
                                                                   const double* rmin, int nblk, int nb_w_other,
                                                                   double* __restrict__ shadow, int32_t* __restrict__ shadow_meta,
                                                                   PivotRecord* rec, const double* __restrict__ msgs, int count,
                                                                   int64_t msg_len, int rule, int split) {
    const double first = (!msgs && (int)threadIdx.x < nblk) ? rmin[threadIdx.x] : INFINITY;      // in flight with the record
    PivotRecord R = *rec;
    const bool w_half = (int)blockIdx.x >= nb_row;
    const int nb_w = RPB == kThreads ? nblk : nb_w_other;
    const int part = w_half ? ((int)blockIdx.x - nb_row) / nb_w : 0;
    const int wblock = (int)blockIdx.x - nb_row - part * nb_w;
    const int i = wblock * kThreads + threadIdx.x;
    // the loop has ended (or ends here): the double buffers still advance, because the host keeps swapping them
    const bool lead = w_half && part == 0;
    const bool mine = lead && i < m;
    if (R.outcome != DEV_RUNNING) {
        if (mine) { b_out[i] = b_in[i]; basis_out[i] = basis_in[i]; }
        return;
    }
    if (msgs) {
        // sharded loop: the entering column is the winner among the gathered candidates [key, j, d_j, alpha (m), block
        // minima of the ratios]; every workgroup picks it with the rules of k_tab_select_candidate_ratio
        int q_win = 0;
        double d_win = 0.0;
        const int win = candidate_winner_staged(msgs, count, msg_len, rule, tol.tie, &q_win, &d_win);
        if (win < 0) {
            if (mine) { b_out[i] = b_in[i]; basis_out[i] = basis_in[i]; }
            if (lead && wblock == 0 && threadIdx.x == 0) record_candidate(rec, rule, -1, 0, 0.0);
            return;
        }
        R.q = q_win;
        R.d_q = d_win;
        if (rule == 1) R.last_selected = R.q;                      // (what the row update's selection keys start from)
        alpha = msgs + win * msg_len + 3;
        rmin = alpha + m;
    }
    int r, leaving;
    ratio_blocks_pick<kThreads>(alpha, b_in, basis_in, m, tol, rmin, nblk, &r, &leaving, first, !msgs, RPB);
    if (r < 0) {
        if (mine) { b_out[i] = b_in[i]; basis_out[i] = basis_in[i]; }
        if (lead && wblock == 0 && threadIdx.x == 0) rec->outcome = DEV_NO_ROW;
        return;
    }
    __shared__ double s_wr[kMaxEta];
    __shared__ double s_ab[2];
    __shared__ int s_jt;
    const int p_old = R.p_now;
    stage_w_row(du, r, p_old, s_wr);
    if (threadIdx.x == 0) {
        s_ab[0] = alpha[r]; s_ab[1] = b_in[r];
        const int slot = du.pos_of_row[r];
        s_jt = slot < 0 ? p_old : slot;
    }
    __syncthreads();
    const double alpha_r = s_ab[0], b_r = s_ab[1];
    const int jt = s_jt, q = R.q;
    if (!w_half) {
        tab_row_update_core<B>(tv, du, sp, R, blockIdx.x, s_wr, p_old, jt, r, q, leaving, R.d_q, alpha_r);
        return;
    }
    const double br = b_r / alpha_r;
    // this part's pending columns [j_lo, j_hi): equal shares, so every part makes the same number of round trips
    const int share = (p_old + split - 1) / split;
    const int j_lo = min(part * share, p_old), j_hi = min(j_lo + share, p_old);
    if (!lead) {
        if (i < m && i != r) {
            const double u = -alpha[i] / alpha_r;
            tab_update_w_row<B>(du, i, u, s_wr, j_lo, j_hi);
            if (jt >= j_lo && jt < j_hi) du.W[(int64_t)jt * du.ld + i] += u;
        }
        return;
    }
    if (i < m) {
        const double a = alpha[i], b_i = b_in[i];
        const double u = (i == r) ? (1.0 / alpha_r - 1.0) : (-a / alpha_r);
        if (i != r) {
            tab_update_w_row<B>(du, i, u, s_wr, j_lo, j_hi);
            double* tgt = du.W + (int64_t)jt * du.ld + i;
            if (jt >= p_old) *tgt = u;
            else if (jt < j_hi) *tgt += u;
        } else {
            // row r itself: other workgroups are reading its old values right now, the new ones go to the shadow row
            for (int j = 0; j < p_old; ++j) {
                const double w = s_wr[j];
                shadow[j] = (u != 0.0 && w != 0.0) ? fma(u, w, w) : w;
            }
            if (jt < p_old) shadow[jt] += u; else shadow[jt] = u;
            shadow_meta[0] = r;
            shadow_meta[1] = jt < p_old ? p_old : p_old + 1;
        }
        b_out[i] = pivot_b(a, b_i, br, i == r);
        basis_out[i] = (i == r) ? q : basis_in[i];
    }
    if (i == 0) {
        if (msgs) record_candidate(rec, rule, 0, q, R.d_q);
        rec->r = r; rec->leaving = leaving; rec->alpha_r = alpha_r; rec->b_r = b_r;
        rec->n_eta_old = p_old; rec->eta_target = jt;
        if (jt >= p_old) { du.S[p_old] = r; du.pos_of_row[r] = p_old; rec->n_eta = p_old + 1; }
        pivot_bookkeeping(R.phase, R.iterations, R.minus_objective, R.d_q, br, q, r, leaving, in_basis, trace, trace_cap, rec);
    }
}

// Folds a pending shadow row (k_tab_ratio_update_all) into W; {row, length} = {-1, 0} afterwards.
__global__ void k_tab_apply_shadow(DeferredUpdate du, double* __restrict__ shadow, int32_t* __restrict__ shadow_meta) {
    const int row = shadow_meta[0], len = shadow_meta[1];
    if (row < 0) return;
    for (int j = threadIdx.x; j < len; j += blockDim.x) du.W[(int64_t)j * du.ld + row] = shadow[j];
    __syncthreads();
    if (threadIdx.x == 0) shadow_meta[0] = -1;
}

// PRICE's final reduction and the tableau column in one launch: every workgroup reduces the (few)
// partials to the same entering column q, then forms alpha = T0[:,q] + W R0[:,q] for its rows.
// `msg` (sharded engines): the candidate message [key, j, d_j, alpha(m)] of this rank is written instead
// of the record; a rank without a candidate sends key = +inf and stays RUNNING (another rank may have one).
// `rmin` (single-GPU loop): the minimum ratio b_i / alpha_i over this workgroup's 256 rows, for
// k_ratio_blocks.
// R = rows per workgroup (256, 128 or 64; tab_column_rows), always 256 threads.  R = 256 is one thread per row walking all p
// pending rows B at a time (tab_column_entry).  R < 256: S = 256 / R slices of R threads stand on the same R rows, thread t on
// row blockIdx.x * R + t % R in slice t / R, and slice s owns the pending rows j in [s * ceil(p / S), (s + 1) * ceil(p / S)),
// cut at p.  Every slice loads its whole share of W into NW registers at once (NW >= ceil(kmax / S), masked by p: nothing at
// or past row p is read), so a row block has S times the loads in flight and a CU pulls 1 / S of the bytes.  The fma chain of a
// row is then handed from slice to slice through s_acc: slice 0 starts from T0[i, q], each slice continues from the value its
// predecessor left, in ascending j -- the operations and the order of tab_column_entry -- and an empty share passes the value
// on untouched.  The last slice writes alpha and forms the ratios; rmin[blockIdx.x] is the minimum over the R rows (exact in
// any order).  B is not used when R < 256.
template <int B, int R, int NW>
__global__ __launch_bounds__(kThreads) void k_tab_select_column(TableauView tv, DeferredUpdate du, SelectPartials sp,
                                                                int count, double* alpha, double* msg,
                                                                const double* b, Tolerances tol,
                                                                double* rmin, PivotRecord* rec,
                                                                const double* shadow, int32_t* shadow_meta) {
    static_assert(R == 64 || R == 128 || R == kThreads, "whole wavefronts per slice");
    constexpr int S = kThreads / R;
    const int outcome = rec->outcome, p = rec->n_eta;          // one round trip for both ...
    // ... and for the shadow row of the previous pivot's fused update: the workgroup that owns the row folds it into W before
    // it reads the row (no other workgroup reads it)
    if (shadow_meta) {
        const int srow = shadow_meta[0], slen = shadow_meta[1];
        if (srow >= 0 && srow / R == (int)blockIdx.x) {
            if ((int)threadIdx.x < slen) du.W[(int64_t)threadIdx.x * du.ld + srow] = shadow[threadIdx.x];
            __syncthreads();
            if (threadIdx.x == 0) shadow_meta[0] = -1;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) rec->p_now = p;
    }
    // ... and for the first PRICE partial and b of this thread's row, which do not depend on the record
    double k1 = INFINITY;
    int bj = 0x7fffffff;
    if ((int)threadIdx.x < count) { k1 = sp.k1[threadIdx.x]; bj = sp.j[threadIdx.x]; }
    const int slice = R == kThreads ? 0 : (int)threadIdx.x / R;
    const int i = blockIdx.x * R + (R == kThreads ? (int)threadIdx.x : (int)threadIdx.x % R);
    const double b_i = (rmin && i < tv.m && slice == S - 1) ? b[i] : 0.0;
    if (outcome != DEV_RUNNING) return;
    __shared__ double s_vs[kMaxEta];
    tab_select_entering<kThreads>(tv, sp, count, k1, bj);
    if (bj == 0x7fffffff) {
        if (msg) {
            if (i < tv.m) alpha[i] = 0.0;
            if (i == 0) { msg[0] = INFINITY; msg[1] = 0.0; msg[2] = 0.0; }
        } else if (blockIdx.x == 0 && threadIdx.x == 0) {
            rec->outcome = DEV_NO_CANDIDATE;
            if (sp.rule == 1) rec->last_selected = -1;
        }
        return;
    }
    const int cq = bj + tv.col_off;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (msg) { msg[0] = k1; msg[1] = (double)bj; msg[2] = tv.d[cq]; }
        else {
            rec->q = bj;
            rec->d_q = tv.d[cq];
            rec->key1 = k1;
            if (sp.rule == 1) rec->last_selected = bj;
        }
    }
    double ratio = INFINITY;
    if constexpr (R == kThreads) {
        if ((int)threadIdx.x < p) s_vs[threadIdx.x] = tv.R0[(int64_t)threadIdx.x * tv.ld_r + cq];
        const double t0 = i < tv.m ? tv.T0[(int64_t)cq * tv.ld_t + i] : 0.0;     // in flight together with the R0 column
        __syncthreads();
        if (i < tv.m) {
            const double a = tab_column_entry<B>(du, i, p, s_vs, t0);
            alpha[i] = a;
            // the same expression as the ratio test's first pass (ratio_body), so min over the block minima is
            // bit for bit the minimum over all rows
            const double bz = b_i <= tol.zero ? 0.0 : b_i;
            if (a > tol.pivot) ratio = bz / a;
        }
    } else {
        // One round trip for the R0 column, T0[i, q] and this slice's whole share of the pending rows: the R0 entry goes to
        // s_vs only after the loads of W have left, so no slice waits for anything before its own loads are on their way.
        const double vq = (int)threadIdx.x < p ? tv.R0[(int64_t)threadIdx.x * tv.ld_r + cq] : 0.0;
        double a = (i < tv.m && slice == 0) ? tv.T0[(int64_t)cq * tv.ld_t + i] : 0.0;
        const int share = (p + S - 1) / S;
        const int j_lo = min(slice * share, p);
        const int cnt = i < tv.m ? min(share, p - j_lo) : 0;
        const double* col = du.W + (int64_t)j_lo * du.ld + i;
        double w[NW];
#pragma unroll
        for (int t = 0; t < NW; ++t) w[t] = t < cnt ? col[(int64_t)t * du.ld] : 0.0;
        if ((int)threadIdx.x < p) s_vs[threadIdx.x] = vq;
        __syncthreads();
        // the share's entries of the R0 column into registers too, ahead of the hand-offs (an entry past the share is read
        // inside s_vs and not used)
        double v[NW];
#pragma unroll
        for (int t = 0; t < NW; ++t) v[t] = s_vs[min(j_lo + t, kMaxEta - 1)];
        __shared__ double s_acc[R];
        const int x = (int)threadIdx.x % R;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s > 0) __syncthreads();                // the value slice s - 1 left in s_acc
            if (slice == s) {
                if (s > 0) a = s_acc[x];
#pragma unroll
                for (int t = 0; t < NW; ++t) a = t < cnt ? fma(w[t], v[t], a) : a;
                if (s < S - 1) s_acc[x] = a;
            }
        }
        if (slice == S - 1 && i < tv.m) {
            alpha[i] = a;
            const double bz = b_i <= tol.zero ? 0.0 : b_i;     // (as above)
            if (a > tol.pivot) ratio = bz / a;
        }
    }
    if (!rmin) return;
    ratio = block_min_value<kThreads>(ratio);
    if (threadIdx.x == 0) rmin[blockIdx.x] = ratio;
}

// Ratio test from the per-block minima of k_tab_select_column (ratio_blocks_body): one workgroup.
__global__ __launch_bounds__(kSingleBlock) void k_ratio_blocks(const double* __restrict__ alpha, const double* __restrict__ b,
                                                               const int32_t* __restrict__ basis_indices, int m,
                                                               Tolerances tol, DeferredUpdate du,
                                                               const double* __restrict__ rmin, int nblk, PivotRecord* rec) {
    const int outcome = rec->outcome, p = rec->n_eta;
    const double first = (int)threadIdx.x < nblk ? rmin[threadIdx.x] : INFINITY;      // same round trip as the record
    if (outcome != DEV_RUNNING) return;
    ratio_blocks_body<kSingleBlock>(alpha, b, basis_indices, m, tol, du, rmin, nblk, p, rec, first, true);
}

// Sharded engines: the winner among the gathered candidates [key, j, d_j, alpha (m), block minima of the
// ratios], its tableau column copied for the update launch, and the ratio test on it from the block minima the
// sender computed -- one single-workgroup launch.  Same choice rules as k_select_candidate.
__global__ __launch_bounds__(kSingleBlock) void k_tab_select_candidate_ratio(const double* __restrict__ msgs, int count,
                                                                             int64_t msg_len, int m, double* __restrict__ alpha,
                                                                             const double* __restrict__ b,
                                                                             const int32_t* __restrict__ basis_indices,
                                                                             int rule, Tolerances tol, DeferredUpdate du,
                                                                             int forced_row, PivotRecord* rec) {
    const int outcome = rec->outcome, p = rec->n_eta;
    if (outcome != DEV_RUNNING) return;
    int q = 0;
    double d_q = 0.0;
    const int win = candidate_winner_staged(msgs, count, msg_len, rule, tol.tie, &q, &d_q);      // all heads in one round trip
    if (threadIdx.x == 0) record_candidate(rec, rule, win, q, d_q);
    if (win < 0) return;
    const double* __restrict__ col = msgs + win * msg_len + 3;
    // the winner's block minima and its column (copied for the update launch) leave in the same round trip; the
    // copy is stored after the ratio test, which reads the column from the message itself
    const int nblk = (m + kThreads - 1) / kThreads;
    if (forced_row >= 0) {
        // zero-level pivot in a given row (phase_one.rs:246-250): no ratio test, the variable basic there leaves
        for (int i = threadIdx.x; i < m; i += kSingleBlock) alpha[i] = col[i];
        ratio_commit_row<kSingleBlock>(forced_row, basis_indices[forced_row], col, b, du, p, rec);
        return;
    }
    const double first = (int)threadIdx.x < nblk ? col[m + threadIdx.x] : INFINITY;
    constexpr int kCopy = 16;
    double cp[kCopy];
#pragma unroll
    for (int u = 0; u < kCopy; ++u) {
        const int i = threadIdx.x + u * kSingleBlock;
        cp[u] = i < m ? col[i] : 0.0;
    }
    ratio_blocks_body<kSingleBlock>(col, b, basis_indices, m, tol, du, col + m, nblk, p, rec, first, true);
#pragma unroll
    for (int u = 0; u < kCopy; ++u) {
        const int i = threadIdx.x + u * kSingleBlock;
        if (i < m) alpha[i] = cp[u];
    }
    for (int i = threadIdx.x + kCopy * kSingleBlock; i < m; i += kSingleBlock) alpha[i] = col[i];
}

__global__ void k_tab_update_vectors(int m, const double* __restrict__ alpha, double* __restrict__ b,
                                     int32_t* __restrict__ basis_indices, uint8_t* __restrict__ in_basis,
                                     int32_t* __restrict__ trace, int64_t trace_cap, PivotRecord* rec) {
    if (rec->outcome != DEV_RUNNING) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = rec->r;
    const double br = rec->b_r / rec->alpha_r;
    if (i < m) b[i] = pivot_b(alpha[i], b[i], br, i == r);
    if (i == 0) {
        basis_indices[r] = rec->q;
        pivot_bookkeeping(rec->phase, rec->iterations, rec->minus_objective, rec->d_q, br, rec->q, r, rec->leaving, in_basis, trace,
                          trace_cap, rec);
    }
}

// Flush: T0 += W R0 on the f64 matrix cores (v_mfma_f64_16x16x4_f64).  The MFMA computes the
// transposed tile (R0' W')  so that the fast lane index of the accumulator runs along the rows of
// T0, which are contiguous (column-major): stores are 128-byte segments.
//   A operand (16 x 4): A[M][k] = R0[k][c0 + M]      lane l: M = l & 15, k = l >> 4
//   B operand (4 x 16): B[k][N] = W[i0 + N][k]       lane l: N = l & 15, k = l >> 4
//   D (16 x 16):        D[M][N] -> T0[i0 + N, c0 + M], lane l holds N = l & 15, M = (l >> 4) + 4 g, g = 0..3
// Wavefront tile 64 columns x 64 rows (4 x 4 MFMA tiles, 8 operand loads per 16 MFMAs), workgroup
// 128 x 128.
template <int MT, int NT>
__global__ __launch_bounds__(kThreads) void k_tab_flush(TableauView tv, DeferredUpdate du, const int32_t* p_dev,
                                                        unsigned long long* stats) {
    constexpr int kFlushMT = MT, kFlushNT = NT;
    const int p = *p_dev;
    if (p == 0) return;
    if (stats && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { stats[0] += 1; stats[1] += tv.c_hi - tv.c_lo; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c_wave = tv.c_lo + blockIdx.x * (2 * 16 * MT) + (wave & 1) * (16 * MT);   // first T0 column of this wavefront
    const int i_wave = blockIdx.y * (2 * 16 * NT) + (wave >> 1) * (16 * NT);            // first T0 row
    if (c_wave >= tv.c_hi || i_wave >= tv.m) return;
    const int lm = lane & 15, lk = lane >> 4;
    // the accumulators start as the T0 tile itself: all of its loads are in flight before the first MFMA
    double4_t acc[kFlushMT][kFlushNT];
#pragma unroll
    for (int a = 0; a < kFlushMT; ++a)
#pragma unroll
        for (int b = 0; b < kFlushNT; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = c_wave + a * 16 + lk + 4 * g;
                const int i = i_wave + b * 16 + lm;
                acc[a][b][g] = (c < tv.c_hi && i < tv.m) ? tv.T0[(int64_t)c * tv.ld_t + i] : 0.0;
            }
    // operand fragments of step k0 + 4 are requested before the MFMAs of step k0 are issued, so their
    // L2 latency (~1-2 us) overlaps the 8 x 64-cycle MFMAs instead of serialising with them
    double af[kFlushMT], bf[kFlushNT], afn[kFlushMT], bfn[kFlushNT];
    auto load_frags = [&](int k0, double* fa, double* fb) {
        const int k = k0 + lk;
        const bool kv = k < p;
#pragma unroll
        for (int a = 0; a < kFlushMT; ++a) {
            const int c = c_wave + a * 16 + lm;
            fa[a] = (kv && c < tv.c_hi) ? tv.R0[(int64_t)k * tv.ld_r + c] : 0.0;
        }
#pragma unroll
        for (int b = 0; b < kFlushNT; ++b) {
            const int i = i_wave + b * 16 + lm;
            fb[b] = (kv && i < tv.m) ? du.W[(int64_t)k * du.ld + i] : 0.0;
        }
    };
    load_frags(0, af, bf);
    for (int k0 = 0; k0 < p; k0 += 4) {
        load_frags(k0 + 4, afn, bfn);                 // k >= p yields zeros, no branch
#pragma unroll
        for (int a = 0; a < kFlushMT; ++a)
#pragma unroll
            for (int b = 0; b < kFlushNT; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < kFlushMT; ++a) af[a] = afn[a];
#pragma unroll
        for (int b = 0; b < kFlushNT; ++b) bf[b] = bfn[b];
    }
#pragma unroll
    for (int a = 0; a < kFlushMT; ++a)
#pragma unroll
        for (int b = 0; b < kFlushNT; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = c_wave + a * 16 + lk + 4 * g;
                const int i = i_wave + b * 16 + lm;
                if (c < tv.c_hi && i < tv.m) tv.T0[(int64_t)c * tv.ld_t + i] = acc[a][b][g];
            }
}

// The same product with the operands staged through LDS.  A workgroup of WC x WR wavefronts owns a
// (WC * 64 columns) x (WR * 32 rows) tile of T0; per chunk of KC pivots of the block it copies the
// R0 rows (KC x TC) and W columns (KC x TR) it needs into LDS once (double-buffered, 16-byte global
// loads issued one chunk ahead) and every wavefront takes its MFMA fragments from there.  Without this
// each wavefront fetches its own operands from L2 / Infinity Cache: 48 KB per 32 KB of T0 traffic
// (4.7 GB per flush at 10k x 20k against 3.2 GB of HBM traffic); with a 256 x 128 tile it is 12 KB.
// Column tiles walk positions x: the owned column c_lo + x (kList = false), or the x-th column of the
// FlushList with its compacted R0 (kList = true; the grid covers every owned column and the tiles past
// the list's count return at once).  Each column gets the same k order, so the same bits, either way.
template <int WC, int WR, int KC, bool kList>
__global__ __launch_bounds__(WC * WR * 64) void k_tab_flush_lds(TableauView tv, DeferredUpdate du, const int32_t* p_dev,
                                                                FlushList fl) {
    constexpr int MT = 4, NT = 2;                     // wavefront tile: 64 columns x 32 rows
    constexpr int TC = WC * 16 * MT, TR = WR * 16 * NT, NTHR = WC * WR * 64;
    constexpr int RA = KC * TC / 2 / NTHR, RB = KC * TR / 2 / NTHR;
    static_assert(RA * NTHR * 2 == KC * TC && RB * NTHR * 2 == KC * TR, "staging must divide evenly");
    const int p = *p_dev;
    const int n_cols = kList ? *fl.count : tv.c_hi - tv.c_lo;
    if (p == 0) return;
    if (kList && (int)blockIdx.y * TC >= n_cols) return;
    if (!kList && fl.stats && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { fl.stats[0] += 1; fl.stats[1] += n_cols; }
    __shared__ __align__(16) double As[2][KC][TC];
    __shared__ __align__(16) double Bs[2][KC][TR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave % WC, wr = wave / WC;
    // consecutive workgroups walk down the rows of the same 256 columns: T0 is column-major, so the
    // workgroups in flight stream whole columns (sequential DRAM pages) and share one R0 chunk in L2
    const int x_blk = blockIdx.y * TC, i_blk = blockIdx.x * TR;
    const int x_wave = x_blk + wc * 16 * MT, i_wave = i_blk + wr * 16 * NT;
    const bool active = x_wave < n_cols && i_wave < tv.m;
    const int lm = lane & 15, lk = lane >> 4;
    // A operand rows: position x at a_src[k * a_ld + x], readable up to the (even) pitch
    const double* a_src = kList ? fl.R0c : tv.R0 + tv.c_lo;
    const int64_t a_ld = kList ? fl.ld : tv.ld_r;
    // kList: lane l holds the storage column at position x_wave + l; accumulator (a, g) belongs to lane a * 16 + lk + 4 g
    const int col_lane = kList && active && x_wave + lane < n_cols ? fl.cols[x_wave + lane] : -1;
    auto column = [&](int a, int g) -> int {           // storage column of accumulator (a, g), -1 past the end
        const int x = a * 16 + lk + 4 * g;
        if (kList) return __shfl(col_lane, x, 64);
        return x_wave + x < n_cols ? tv.c_lo + x_wave + x : -1;
    };
    double2 ra[RA], rb[RB];
    auto gload = [&](int kc) {
#pragma unroll
        for (int u = 0; u < RA; ++u) {
            const int idx = tid + NTHR * u, k = idx / (TC / 2), x = x_blk + 2 * (idx % (TC / 2));
            ra[u] = (kc + k < p && x < a_ld) ? *reinterpret_cast<const double2*>(a_src + (int64_t)(kc + k) * a_ld + x)
                                             : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            const int idx = tid + NTHR * u, k = idx / (TR / 2), i = i_blk + 2 * (idx % (TR / 2));
            rb[u] = (kc + k < p && i < (int)du.ld) ? *reinterpret_cast<const double2*>(du.W + (int64_t)(kc + k) * du.ld + i)
                                                   : make_double2(0.0, 0.0);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int u = 0; u < RA; ++u) {
            const int idx = tid + NTHR * u;
            *reinterpret_cast<double2*>(&As[buf][idx / (TC / 2)][2 * (idx % (TC / 2))]) = ra[u];
        }
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            const int idx = tid + NTHR * u;
            *reinterpret_cast<double2*>(&Bs[buf][idx / (TR / 2)][2 * (idx % (TR / 2))]) = rb[u];
        }
    };
    gload(0);
    // the accumulators start as the T0 tile itself
    double4_t acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = column(a, g);
                const int i = i_wave + b * 16 + lm;
                acc[a][b][g] = (active && c >= 0 && i < tv.m) ? tv.T0[(int64_t)c * tv.ld_t + i] : 0.0;
            }
    lstore(0);
    __syncthreads();
    const int nchunks = (p + KC - 1) / KC;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks) gload((ch + 1) * KC);
        if (active) {
            const int kmax = min(KC, p - ch * KC);
            for (int k0 = 0; k0 < kmax; k0 += 4) {
                double af[MT], bf[NT];
#pragma unroll
                for (int a = 0; a < MT; ++a) af[a] = As[buf][k0 + lk][wc * 16 * MT + a * 16 + lm];
#pragma unroll
                for (int b = 0; b < NT; ++b) bf[b] = Bs[buf][k0 + lk][wr * 16 * NT + b * 16 + lm];
#pragma unroll
                for (int a = 0; a < MT; ++a)
#pragma unroll
                    for (int b = 0; b < NT; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc[a][b], 0, 0, 0);
            }
        }
        if (ch + 1 < nchunks) lstore(buf ^ 1);
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = column(a, g);
                const int i = i_wave + b * 16 + lm;
                if (c >= 0 && i < tv.m) tv.T0[(int64_t)c * tv.ld_t + i] = acc[a][b][g];
            }
}

// The FlushList of a flush, in two launches over groups of 64 owned columns (one workgroup each, its four wavefronts on
// every fourth pending row).  Mark: bit l of mask[b] = column c_lo + 64 b + l has a nonzero R0 entry.
__global__ __launch_bounds__(kThreads) void k_tab_flush_mark(TableauView tv, FlushList fl, const int32_t* p_dev) {
    const int p = *p_dev;
    if (p == 0) return;
    __shared__ unsigned long long s_mask[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = tv.c_lo + blockIdx.x * 64 + lane;
    bool nz = false;
    if (c < tv.c_hi) {
        // eight independent loads in flight per step (p <= kMaxEta: at most four steps)
        for (int j0 = wave; j0 < p; j0 += 4 * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = j0 + 4 * u < p ? tv.R0[(int64_t)(j0 + 4 * u) * tv.ld_r + c] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) nz |= !(v[u] == 0.0);          // NaN != 0
        }
    }
    const unsigned long long m = __ballot(nz);
    if (lane == 0) s_mask[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) fl.mask[blockIdx.x] = s_mask[0] | s_mask[1] | s_mask[2] | s_mask[3];
}

// Compact: group b's marked columns go after those of groups 0 .. b-1 (ascending storage column, the same list every run):
// their indices to cols, their R0 columns to R0c.  The last group stores the count and adds the flush to the statistics.
__global__ __launch_bounds__(kThreads) void k_tab_flush_compact(TableauView tv, FlushList fl, const int32_t* p_dev, int nb) {
    const int p = *p_dev;
    if (p == 0) return;
    __shared__ int s_before[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kThreads) before += __popcll(fl.mask[b]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off, 64);
    if (lane == 0) s_before[wave] = before;
    __syncthreads();
    before = s_before[0] + s_before[1] + s_before[2] + s_before[3];
    const unsigned long long mask = fl.mask[blockIdx.x];
    if ((mask >> lane) & 1ull) {
        const int c = tv.c_lo + blockIdx.x * 64 + lane;
        const int x = before + __popcll(mask & ((1ull << lane) - 1ull));
        if (wave == 0) fl.cols[x] = c;
        for (int j0 = wave; j0 < p; j0 += 4 * 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = j0 + 4 * u < p ? tv.R0[(int64_t)(j0 + 4 * u) * tv.ld_r + c] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + 4 * u < p) fl.R0c[(int64_t)(j0 + 4 * u) * fl.ld + x] = v[u];
        }
    }
    if ((int)blockIdx.x == nb - 1 && threadIdx.x == 0) {
        const int count = before + __popcll(mask);
        *fl.count = count;
        fl.stats[0] += 1;
        fl.stats[1] += count;
    }
}

__global__ void k_tab_gather_columns(TableauView tv, const int32_t* __restrict__ cols, double* __restrict__ out) {
    const int64_t total = (int64_t)tv.m * tv.m;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(idx / tv.m), i = (int)(idx % tv.m);        // consecutive threads walk down a column of T0
        out[(int64_t)i * tv.m + k] = tv.T0[(int64_t)cols[k] * tv.ld_t + i];
    }
}

template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_row(TableauView tv, DeferredUpdate du, int row, double* __restrict__ out,
                                                      const PivotRecord* rec) {
    __shared__ double s_w[kMaxEta];
    const int p = rec->n_eta;
    stage_w_row(du, row, p, s_w);
    __syncthreads();
    const int c = tv.c_lo + blockIdx.x * kThreads + threadIdx.x;
    if (c >= tv.c_hi) return;
    out[c - tv.c_lo] = tab_row_entry<B>(tv, c, p, s_w, tv.T0[(int64_t)c * tv.ld_t + row]);
}

// phase_one.rs:236-244 for the sharded engine: among the owned columns, the candidates to replace a basic
// artificial variable at zero level in tableau row `row` -- non-basic, not artificial, reduced cost 0, tableau
// entry != 0 -- as PRICE partials with key = column index (the first one wins, like FirstProfitable).
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_zero_level_scan(TableauView tv, DeferredUpdate du, SelectPartials sp, int row,
                                                                  int nr_artificial, Tolerances tol, const PivotRecord* rec) {
    const int outcome = rec->outcome, p = rec->n_eta;
    if (outcome != DEV_RUNNING) return;
    __shared__ double s_w[kMaxEta];
    stage_w_row(du, row, p, s_w);
    __syncthreads();
    const int c = tv.c_lo + blockIdx.x * kThreads + threadIdx.x;
    const int j = c - tv.col_off;
    double key = INFINITY;
    int kj = 0x7fffffff;
    if (c < tv.c_hi && j >= nr_artificial && j < tv.n && !sp.in_basis[j] && fabs(tv.d[c]) <= tol.cost) {
        const double v = tab_row_entry<B>(tv, c, p, s_w, tv.T0[(int64_t)c * tv.ld_t + row]);
        if (fabs(v) > tol.pivot) { key = (double)j; kj = j; }
    }
    block_partial_min(key, kj, sp, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Dual simplex on the tableau (relp_run_dual; no counterpart in the reference, whose primal_dual module is empty).  The
// selection is new, the pivot itself is k_tab_update_all:
//   leaving row      the minimum b_i over the infeasible rows (b_i < -tol_feas), ties to the smallest leaving column
//   entering column  over row r of T: the minimum d_j / (-T[r,j]) over the non-basic columns with T[r,j] < -tol_pivot, ties to
//                    the lowest column
// ------------------------------------------------------------------------------------------------
// The minimum b_i over the infeasible rows of every block of 256 rows (+inf: the block has none).
__global__ __launch_bounds__(kThreads) void k_dual_bmin(const double* __restrict__ b, int m, double tol_feas,
                                                        double* __restrict__ bmin, const PivotRecord* rec) {
    if (rec->outcome != DEV_RUNNING) return;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    double v = INFINITY;
    if (i < m) {
        const double bi = b[i];
        if (bi < -tol_feas) v = bi;
    }
    v = block_min_value<kThreads>(v);
    if (threadIdx.x == 0) bmin[blockIdx.x] = v;
}

// The leaving row from the block minima `bmin` (block_minima_pick): Bland on the leaving column among the infeasible rows inside
// the tie band of the minimum.  Every thread returns with (row, leaving column), row = -1 when no row is infeasible; nothing is
// written.
template <int BS>
__device__ __forceinline__ void dual_row_pick(const double* b, const int32_t* basis_indices, int m, double tol_feas, double tol_tie,
                                              const double* bmin, int nblk, int* row_out, int* leave_out) {
    block_minima_pick<BS>(bmin, nblk, kThreads, m, tol_tie, INFINITY, false, false, row_out, leave_out, [&](int i, double bound) {
        const double bi = b[i];
        const int lv = basis_indices[i];
        return (bi < -tol_feas && bi <= bound) ? tie_key(0.0, lv, 0) : kNoTieKey;
    });
}

// The pivot row of a dual kernel: the given one (step-wise call) or the pick from the block minima.
template <int BS>
__device__ __forceinline__ void dual_pivot_row(const double* b, const int32_t* basis_indices, int m, double tol_feas, double tol_tie,
                                               const double* bmin, int nblk, int forced_row, int* r, int* leaving) {
    if (forced_row >= 0) { *r = forced_row; *leaving = basis_indices[forced_row]; return; }
    dual_row_pick<BS>(b, basis_indices, m, tol_feas, tol_tie, bmin, nblk, r, leaving);
}

// d_j / (-row_j) of a candidate of the dual ratio test (row_j < -tol_pivot), with a d_j that rounding left at or below tol_zero
// read as 0: no negative step
__device__ __forceinline__ double dual_ratio(double d_j, double row_j, double tol_zero) {
    const double dz = d_j <= tol_zero ? 0.0 : d_j;
    return dz / (-row_j);
}

// Row r of T over the stored columns, one column per thread, into `row` (indexed from tv.c_lo), and the minimum (ratio, column)
// of the workgroup's 256 columns into partial slot blockIdx.x.  Every workgroup determines the same r.  Reads T0 and R0 only:
// a row that is new in the block is appended to R0 by the update (tab_row_update_core), not here.
template <int B>
__global__ __launch_bounds__(kThreads) void k_dual_row(TableauView tv, DeferredUpdate du, SelectPartials sp,
                                                       const double* __restrict__ b, const int32_t* __restrict__ basis_indices,
                                                       Tolerances tol, double tol_feas, const double* __restrict__ bmin, int nblk,
                                                       int forced_row, double* __restrict__ row, const PivotRecord* rec) {
    const int outcome = rec->outcome, p = rec->n_eta;
    if (outcome != DEV_RUNNING) return;
    int r, leaving;
    dual_pivot_row<kThreads>(b, basis_indices, tv.m, tol_feas, tol.tie, bmin, nblk, forced_row, &r, &leaving);
    if (r < 0) return;                                 // (k_dual_select_column ends the loop)
    __shared__ double s_w[kMaxEta];
    stage_w_row(du, r, p, s_w);
    __syncthreads();
    const int c = tv.c_lo + blockIdx.x * kThreads + threadIdx.x;
    const int j = c - tv.col_off;
    double key = INFINITY;
    int kj = 0x7fffffff;
    if (c < tv.c_hi) {
        const double d_c = tv.d[c];
        const double v = tab_row_entry<B>(tv, c, p, s_w, tv.T0[(int64_t)c * tv.ld_t + r]);
        row[c - tv.c_lo] = v;
        if (j >= 0 && j < tv.n && sp.in_basis[j] == 0 && v < -tol.pivot) { key = dual_ratio(d_c, v, tol.zero); kj = j; }
    }
    block_partial_min(key, kj, sp, blockIdx.x);
}

// Leaving row, entering column and the tableau column alpha = T0[:,q] + W R0[:,q] (the code of k_tab_column) in one launch over
// the rows: every workgroup determines the same r and q, the first one writes them to the record -- or ends the loop: no
// infeasible row is DEV_NO_ROW (the basis is optimal), no candidate in row r is DEV_NO_CANDIDATE (the LP is infeasible).
template <int B>
__global__ __launch_bounds__(kThreads) void k_dual_select_column(TableauView tv, DeferredUpdate du, SelectPartials sp, int count,
                                                                 const double* __restrict__ b,
                                                                 const int32_t* __restrict__ basis_indices, Tolerances tol,
                                                                 double tol_feas, const double* __restrict__ bmin, int nblk,
                                                                 int forced_row, const double* __restrict__ row,
                                                                 double* __restrict__ alpha, PivotRecord* rec) {
    const int outcome = rec->outcome, p = rec->n_eta;
    if (outcome != DEV_RUNNING) return;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    int r, leaving;
    dual_pivot_row<kThreads>(b, basis_indices, tv.m, tol_feas, tol.tie, bmin, nblk, forced_row, &r, &leaving);
    if (r < 0) {
        if (first) rec->outcome = DEV_NO_ROW;
        return;
    }
    // the entering column from the partials of k_dual_row (select_entering): the minimum ratio, then the lowest column with a ratio
    // inside its tie band, from the row k_dual_row left and d
    double k1 = INFINITY;
    int bj = 0x7fffffff;
    select_entering<kThreads>(tv, sp, count, tol.tie, tol.tie > 0.0, false, k1, bj, [&](int c, int j, double bound) {
        const double v = row[c - tv.c_lo];
        const double d_c = tv.d[c];
        return sp.in_basis[j] == 0 && v < -tol.pivot && dual_ratio(d_c, v, tol.zero) <= bound;
    });
    if (bj == 0x7fffffff) {
        if (first) { rec->r = r; rec->leaving = leaving; rec->outcome = DEV_NO_CANDIDATE; }
        return;
    }
    const int cq = bj + tv.col_off;
    if (first) { rec->q = bj; rec->d_q = tv.d[cq]; rec->key1 = k1; rec->r = r; rec->leaving = leaving; }
    __shared__ double s_vs[kMaxEta];
    if ((int)threadIdx.x < p) s_vs[threadIdx.x] = tv.R0[(int64_t)threadIdx.x * tv.ld_r + cq];
    __syncthreads();
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= tv.m) return;
    alpha[i] = tab_column_entry<B>(du, i, p, s_vs, tv.T0[(int64_t)cq * tv.ld_t + i]);
}

// Step-wise call: the leaving row alone, into the record (or DEV_NO_ROW).
__global__ __launch_bounds__(kSingleBlock) void k_dual_select_row(const double* __restrict__ b,
                                                                  const int32_t* __restrict__ basis_indices, int m, double tol_feas,
                                                                  double tol_tie, const double* __restrict__ bmin, int nblk,
                                                                  PivotRecord* rec) {
    if (rec->outcome != DEV_RUNNING) return;
    int r, leaving;
    dual_row_pick<kSingleBlock>(b, basis_indices, m, tol_feas, tol_tie, bmin, nblk, &r, &leaving);
    if (threadIdx.x != 0) return;
    if (r < 0) rec->outcome = DEV_NO_ROW;
    else { rec->r = r; rec->leaving = leaving; }
}

// The pivot (r, q) of k_dual_select_column committed: alpha_r (negative here), b_r and the block bookkeeping of the deferred
// update, as after a ratio test but without its pivot guard.  One workgroup.
__global__ __launch_bounds__(kSingleBlock) void k_dual_commit(const double* __restrict__ alpha, const double* __restrict__ b,
                                                              DeferredUpdate du, PivotRecord* rec) {
    const int outcome = rec->outcome, p = rec->n_eta, r = rec->r, leaving = rec->leaving;
    if (outcome != DEV_RUNNING) return;
    ratio_commit_row<kSingleBlock>(r, leaving, alpha, b, du, p, rec);
}

// ------------------------------------------------------------------------------------------------
// A change of rhs entries in place (relp_change_right_hand_side): b += sum_k delta_k T[:, c_k] over the list (c_k, delta_k) of
// the changed rows' identity columns, with T = T0 + W R0 while an update block is open:
//   b_i += sum_k delta_k T0[i, c_k] + sum_{j<p} W[j][i] v_j,   v_j = sum_k delta_k R0[j][c_k]
// No atomics: every sum has a fixed order, so a given (list, p, splits) gives the same bits every run.
// The two list patterns of this section and of the three after it (cost, cut rows, added columns) are defined once, beside
// for_pending at the top of the file: list_sum (the *_pending kernels) and for_list (the *_apply kernels and k_tab_cut_rows).
// ------------------------------------------------------------------------------------------------
// v_j for pending row j = blockIdx.x: thread t sums its entries k = t, t + 256, ... in ascending order, then a fixed tree over the
// 256 threads (list_sum).  The identity columns of neighbouring rows are mostly neighbouring stored columns: the loads of a
// wavefront coalesce.
__global__ __launch_bounds__(kThreads) void k_tab_rhs_pending(TableauView tv, RhsChange ch, double* __restrict__ v) {
    __shared__ double s_sum[kThreads];
    const double* row = tv.R0 + (int64_t)blockIdx.x * tv.ld_r;
    const double sum = list_sum(ch.count, s_sum, [&](int k) { return ch.delta[k]; }, [&](int k) { return row[ch.cols[k]]; });
    if (threadIdx.x == 0) v[blockIdx.x] = sum;
}

// Row i = blockIdx.x * 256 + threadIdx.x, split blockIdx.y of the list: entries [lo, hi) in ascending k, staged in LDS 256 at a
// time, their T0 loads issued B at a time before any is used (for_list; consecutive threads read consecutive rows of one
// column).  Split 0 then adds the pending rows' share through v (p > 0).  splits == 1: b[i] += acc, else partial[split][i].
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_rhs_apply(TableauView tv, DeferredUpdate du, RhsChange ch, int p,
                                                            const double* __restrict__ v, double* __restrict__ b,
                                                            double* __restrict__ partial, int64_t ld_partial) {
    __shared__ int32_t s_c[kThreads];
    __shared__ double s_delta[kThreads][1];
    __shared__ double s_v[kMaxEta];
    const int splits = gridDim.y, split = blockIdx.y;
    const int share = (ch.count + splits - 1) / splits;
    const int lo = min(split * share, ch.count), hi = min(lo + share, ch.count);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool mine = i < tv.m;
    if (split == 0 && (int)threadIdx.x < p) s_v[threadIdx.x] = v[threadIdx.x];
    double acc[1] = {0.0};
    for_list<B>(lo, hi, s_c, s_delta, [&](int k) { return ch.cols[k]; }, [&](int k, double* dst) { dst[0] = ch.delta[k]; },
                [&](int c) { return tv.T0[(int64_t)c * tv.ld_t + i]; }, mine, acc);
    __syncthreads();                                   // s_v (a split with an empty share never entered the loop)
    if (!mine) return;
    if (split == 0) for_pending<B>(du.W, du.ld, i, p, [&](int j, double w) { acc[0] = fma(w, s_v[j], acc[0]); });
    if (splits == 1) b[i] += acc[0];
    else partial[(int64_t)split * ld_partial + i] = acc[0];
}

// b[i] += partial[0][i] + partial[1][i] + ... in ascending split order
__global__ __launch_bounds__(kThreads) void k_tab_rhs_reduce(int m, int splits, const double* __restrict__ partial, int64_t ld_partial,
                                                             double* __restrict__ b) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    double sum = partial[i];
    for (int s = 1; s < splits; ++s) sum += partial[(int64_t)s * ld_partial + i];
    b[i] += sum;
}

// ------------------------------------------------------------------------------------------------
// A change of cost coefficients in place (relp_change_cost): the mirror image of the rhs change, rows in place of columns and d in
// place of b.  With (r_k, delta_k) the rows of the changed basic columns, ascending r_k, and T = T0 + W R0 while a block is open:
//   d_c -= sum_k delta_k T0[r_k, c] + sum_{j<p} u_j R0[j][c],   u_j = sum_k delta_k W[j][r_k]
// for every stored column not flagged basic; a changed non-basic column also gets d_c += its own delta.
// No atomics: every sum has a fixed order, so a given (list, p, splits) gives the same bits every run.
// ------------------------------------------------------------------------------------------------
// The stored column c is one the change moves: every one the pivot update maintains d for (the kept artificial block in front of
// col_off included), except a column flagged basic, whose d the pivot update pinned at exactly 0.  A barred column moves.
__device__ __forceinline__ bool cost_moves_column(const TableauView& tv, const uint8_t* __restrict__ in_basis, int c) {
    return c < tv.c_hi && !column_flagged_basic(tv, in_basis, c);
}

// u_j for pending row j = blockIdx.x: thread t sums its entries k = t, t + 256, ... in ascending order, then a fixed tree over the
// 256 threads (list_sum).  Column j of W is contiguous and the rows ascend: neighbouring entries share sectors.
__global__ __launch_bounds__(kThreads) void k_tab_cost_pending(DeferredUpdate du, CostChange ch, double* __restrict__ u) {
    __shared__ double s_sum[kThreads];
    const double* col = du.W + (int64_t)blockIdx.x * du.ld;
    const double sum = list_sum(ch.count, s_sum, [&](int k) { return ch.delta[k]; }, [&](int k) { return col[ch.rows[k]]; });
    if (threadIdx.x == 0) u[blockIdx.x] = sum;
}

// Stored column c = c_lo + blockIdx.x * 256 + threadIdx.x, split blockIdx.y of the basic list: entries [lo, hi) in ascending k,
// staged in LDS 256 at a time, their T0 loads issued B at a time before any is used (for_list; a thread walks down its own column:
// eight neighbouring rows are one 64-byte sector).  Split 0 then adds the pending rows' share through u (p > 0, R0 row j is contiguous
// in c) and takes the direct term of a changed non-basic column from the second list (storage columns ascending, binary search).
// splits == 1: d[c] -= acc, else partial[split][c] = acc.
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_cost_apply(TableauView tv, CostChange ch, const uint8_t* __restrict__ in_basis, int p,
                                                             const double* __restrict__ u, double* __restrict__ partial,
                                                             int64_t ld_partial) {
    __shared__ int32_t s_r[kThreads];
    __shared__ double s_delta[kThreads][1];
    __shared__ double s_u[kMaxEta];
    const int splits = gridDim.y, split = blockIdx.y;
    const int share = (ch.count + splits - 1) / splits;
    const int lo = min(split * share, ch.count), hi = min(lo + share, ch.count);
    const int c = tv.c_lo + blockIdx.x * kThreads + threadIdx.x;
    const bool mine = cost_moves_column(tv, in_basis, c);
    const double* col = tv.T0 + (int64_t)(mine ? c : tv.c_lo) * tv.ld_t;
    if (split == 0 && (int)threadIdx.x < p) s_u[threadIdx.x] = u[threadIdx.x];
    double acc[1] = {0.0};
    for_list<B>(lo, hi, s_r, s_delta, [&](int k) { return ch.rows[k]; }, [&](int k, double* dst) { dst[0] = ch.delta[k]; },
                [&](int r) { return col[r]; }, mine, acc);
    __syncthreads();                                   // s_u (a split with an empty share never entered the loop)
    if (!mine) return;
    if (split == 0) {
        for_pending<B>(tv.R0, tv.ld_r, c, p, [&](int j, double r0) { acc[0] = fma(s_u[j], r0, acc[0]); });
        int a = 0, z = ch.ncount;
        while (a < z) {
            const int mid = (a + z) >> 1;
            if (ch.ncols[mid] < c) a = mid + 1;
            else z = mid;
        }
        if (a < ch.ncount && ch.ncols[a] == c) acc[0] -= ch.ndelta[a];
    }
    if (splits == 1) tv.d[c] -= acc[0];
    else partial[(int64_t)split * ld_partial + c] = acc[0];
}

// d[c] -= partial[0][c] + partial[1][c] + ... in ascending split order, for the columns k_tab_cost_apply wrote
__global__ __launch_bounds__(kThreads) void k_tab_cost_reduce(TableauView tv, const uint8_t* __restrict__ in_basis, int splits,
                                                              const double* __restrict__ partial, int64_t ld_partial) {
    const int c = tv.c_lo + blockIdx.x * kThreads + threadIdx.x;
    if (!cost_moves_column(tv, in_basis, c)) return;
    double sum = partial[c];
    for (int s = 1; s < splits; ++s) sum += partial[(int64_t)s * ld_partial + c];
    tv.d[c] -= sum;
}

// ------------------------------------------------------------------------------------------------
// Cut rows added on the current basis (relp_add_cuts): cut k of the call, g_k' x <= beta_k over the structural columns, becomes
// row m + k of the tableau with its new slack basic in it,
//   T[m + k, c] = g_kc - sum_e coef[e][k] T0[r_e, c] - sum_{j<p} u[k][j] R0[j][c],   u[k][j] = sum_e coef[e][k] W[j][r_e]
// over the list of rows r_e (ascending) whose basic column is structural with a nonzero coefficient in some cut of the call;
// coef[e][k] = the coefficient of that basic column in cut k, 0.0 where cut k does not touch it.  The rows are written into T0;
// nothing else of the old rows and columns is.  No atomics: every sum has a fixed order, the same call gives the same bits.
// ------------------------------------------------------------------------------------------------
// u[k][j] for pending row j = blockIdx.x and cut k = blockIdx.y: thread t sums its entries e = t, t + 256, ... in ascending order,
// then a fixed tree over the 256 threads (list_sum; k_tab_cost_pending with a coefficient per (entry, cut)).
__global__ __launch_bounds__(kThreads) void k_tab_cut_pending(DeferredUpdate du, CutRows cr, double* __restrict__ u) {
    __shared__ double s_sum[kThreads];
    const double* col = du.W + (int64_t)blockIdx.x * du.ld;
    const int k = blockIdx.y;
    const double sum = list_sum(cr.entries, s_sum, [&](int e) { return cr.coef[(int64_t)e * cr.count + k]; },
                                [&](int e) { return col[cr.rows[e]]; });
    if (threadIdx.x == 0) u[(int64_t)k * du.kmax + blockIdx.x] = sum;
}

// Old stored column c = c_lo + blockIdx.x * 256 + threadIdx.x, the kTabCutTile cuts from blockIdx.y * kTabCutTile on.  The list is
// staged in LDS 256 entries at a time (rows and the tile's coefficients, 0.0 past the last cut); a thread issues the T0 loads of
// its column B at a time before any is used and feeds every loaded entry into the tile's accumulators, entries ascending
// (for_list): one strided load serves the whole tile.  Then the pending rows' share through u, ascending j, one R0 load for the tile.  Written: T0[m + k, c] = g - acc for
// a structural column (g from the cut rows of A), 0.0 - acc for any other, exactly 0.0 for a column flagged basic.  The tile's
// rows of one column are contiguous.  Nothing else is written; tv describes the tableau before the add.
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_cut_rows(TableauView tv, CutRows cr, const uint8_t* __restrict__ in_basis, int p,
                                                           const double* __restrict__ u, int kmax) {
    __shared__ int32_t s_r[kThreads];
    __shared__ double s_coef[kThreads][kTabCutTile];
    __shared__ double s_u[kTabCutTile][kMaxEta];
    const int k0 = blockIdx.y * kTabCutTile, nv = min(kTabCutTile, cr.count - k0);
    const int c = tv.c_lo + blockIdx.x * kThreads + threadIdx.x;
    const bool mine = c < tv.c_hi;
    const double* col = tv.T0 + (int64_t)(mine ? c : tv.c_lo) * tv.ld_t;
    for (int x = threadIdx.x; x < kTabCutTile * p; x += kThreads) {
        const int v = x / p, j = x - v * p;
        s_u[v][j] = v < nv ? u[(int64_t)(k0 + v) * kmax + j] : 0.0;
    }
    double acc[kTabCutTile];
#pragma unroll
    for (int v = 0; v < kTabCutTile; ++v) acc[v] = 0.0;
    for_list<B>(0, cr.entries, s_r, s_coef, [&](int e) { return cr.rows[e]; },
                [&](int e, double* dst) {
                    const double* g = cr.coef + (int64_t)e * cr.count + k0;
#pragma unroll
                    for (int v = 0; v < kTabCutTile; ++v) dst[v] = v < nv ? g[v] : 0.0;
                },
                [&](int r) { return col[r]; }, mine, acc);
    __syncthreads();                                   // s_u (an empty list never entered the loop)
    if (!mine) return;
    for_pending<B>(tv.R0, tv.ld_r, c, p, [&](int j, double r0) {
#pragma unroll
        for (int v = 0; v < kTabCutTile; ++v) acc[v] = fma(s_u[v][j], r0, acc[v]);
    });
    const bool basic = column_flagged_basic(tv, in_basis, c);
    const int sp = c - cr.struct_c0;
    const double* g = (sp >= 0 && sp < cr.nr_normal) ? cr.A + (int64_t)sp * cr.ld_a + cr.a_row0 + k0 : nullptr;
    double* out = tv.T0 + (int64_t)c * tv.ld_t + tv.m + k0;
#pragma unroll
    for (int v = 0; v < kTabCutTile; ++v)
        if (v < nv && (int64_t)tv.m + k0 + v < tv.ld_t) out[v] = basic ? 0.0 : (g ? g[v] : 0.0) - acc[v];
}

// The rest of an add, for the `count` new rows m .. and new stored columns n_store ..: the new slack columns of T0 are unit columns,
// their entries of R0 (all rows, the scratch row included) and the new rows' entries of W are zero, d and the stored cost of the
// new columns are 0 and their flag is basic, the new rows are identity rows of their slacks and sit in no column of W.
__global__ void k_tab_cut_tail(TableauView tv, DeferredUpdate du, CutTail ct, int count) {
    const int64_t n_t = (int64_t)(tv.m + count) * count, n_r = (int64_t)ct.r0_rows * count, n_w = (int64_t)du.kmax * count;
    const int64_t total = n_t + n_r + n_w + count;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        if (idx < n_t) {
            const int k = (int)(idx / (tv.m + count)), i = (int)(idx % (tv.m + count));
            tv.T0[(int64_t)(tv.n_store + k) * tv.ld_t + i] = i == tv.m + k ? 1.0 : 0.0;
        } else if (idx < n_t + n_r) {
            const int64_t x = idx - n_t;
            tv.R0[(x / count) * tv.ld_r + tv.n_store + (x % count)] = 0.0;
        } else if (idx < n_t + n_r + n_w) {
            const int64_t x = idx - n_t - n_r;
            du.W[(x / count) * du.ld + tv.m + (x % count)] = 0.0;
        } else {
            const int k = (int)(idx - n_t - n_r - n_w);
            const int c = tv.n_store + k, row = tv.m + k, j = tv.n + k;
            tv.d[c] = 0.0;
            ct.cost_store[c] = 0.0;
            ct.in_basis[j] = 1;
            ct.idcol[row] = c;
            ct.basis[row] = j;
            if (du.pos_of_row) du.pos_of_row[row] = -1;
            ct.vrow0[ct.first_virtual + k] = row;
            ct.vrow1[ct.first_virtual + k] = -1;
            ct.vsign[ct.first_virtual + k] = 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Columns added on the current basis (relp_add_columns): the mirror image of the cut rows.  B^-1 sits in the stored columns that
// were the identity at the start, in the form T = (I + W S') T0 like every other column, and that form is linear in T0: the new
// column k of the call is
//   T0[:, n_store + k] = sum_e coef[e][k] T0[:, cols[e]],   R0[j][n_store + k] = T0[S[j], n_store + k]  (so that R0 = S' T0 holds)
// over the list of identity columns cols[e] of the rows (ascending) with a nonzero coefficient in some column of the call, and
// T0 + W R0 of it is B^-1 a_k with the open block left open.  W is not read.  No atomics: one chain per entry, fixed order.
// ------------------------------------------------------------------------------------------------
// Row i = blockIdx.x * 256 + threadIdx.x, the kTabColTile new columns from blockIdx.y * kTabColTile on.  The list is staged in LDS
// 256 entries at a time (identity columns and the tile's coefficients, 0.0 past the last column); a thread issues its T0 loads B at
// a time before any is used (consecutive threads read consecutive rows of one column) and feeds every loaded entry into the tile's
// accumulators, entries ascending (for_list).  Written: T0[i, n_store + k] = acc for i < m.  Nothing else is written; tv describes the tableau before the add.
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_col_apply(TableauView tv, ColumnAdd ca) {
    __shared__ int32_t s_c[kThreads];
    __shared__ double s_coef[kThreads][kTabColTile];
    const int k0 = blockIdx.y * kTabColTile, nv = min(kTabColTile, ca.count - k0);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool mine = i < tv.m;
    double acc[kTabColTile];
#pragma unroll
    for (int v = 0; v < kTabColTile; ++v) acc[v] = 0.0;
    for_list<B>(0, ca.entries, s_c, s_coef, [&](int e) { return ca.cols[e]; },
                [&](int e, double* dst) {
                    const double* a = ca.coef + (int64_t)e * ca.count + k0;
#pragma unroll
                    for (int v = 0; v < kTabColTile; ++v) dst[v] = v < nv ? a[v] : 0.0;
                },
                [&](int c) { return tv.T0[(int64_t)c * tv.ld_t + i]; }, mine, acc);
    if (!mine) return;
#pragma unroll
    for (int v = 0; v < kTabColTile; ++v)
        if (v < nv) tv.T0[(int64_t)(tv.n_store + k0 + v) * tv.ld_t + i] = acc[v];
}

// The rest of an add, for the `count` new stored columns n_store ..: their entries of R0 are the T0 entries k_tab_col_apply wrote at
// the p pending rows S[j] and zero in the other rows of R0 (the scratch row included); d and the stored cost are the caller's,
// the flag is non-basic, the descriptors are those of an empty column.
__global__ void k_tab_col_tail(TableauView tv, DeferredUpdate du, ColumnAdd ca, ColumnTail ct, int p) {
    const int64_t n_r = (int64_t)ct.r0_rows * ca.count, total = n_r + ca.count;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        if (idx < n_r) {
            const int64_t j = idx / ca.count, c = tv.n_store + idx % ca.count;
            tv.R0[j * tv.ld_r + c] = j < p ? tv.T0[c * tv.ld_t + du.S[j]] : 0.0;
        } else {
            const int k = (int)(idx - n_r);
            const int c = tv.n_store + k;
            tv.d[c] = ca.d_new[k];
            ct.cost_store[c] = ca.cost_new[k];
            ct.in_basis[tv.n + k] = 0;
            ct.vrow0[ct.first_virtual + k] = -1;
            ct.vrow1[ct.first_virtual + k] = -1;
            ct.vsign[ct.first_virtual + k] = 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Rows and columns taken out of a column-major image in place (relp_remove_cuts, relp_remove_columns): an order-preserving
// compaction, copies only.  No second image, no atomics, no flags, no communication between workgroups: every element is read before
// it is overwritten by the workgroup (rows) or the thread (columns) that overwrites it, so the order in which workgroups run does
// not matter.
// ------------------------------------------------------------------------------------------------
// Columns c = blockIdx.x, blockIdx.x + gridDim.x, ... belong to this workgroup alone.  Destination rows from the first removed row
// rows[0] on, in chunks of 256 B: thread t owns the rows base + x * 256 + t (x < B; consecutive threads, consecutive rows).  The
// source of destination row dst is dst + #{k : rows[k] - k <= dst} >= dst (rows[k] - k ascends: an upper bound by bisection), the
// same in every column, so a chunk's B sources are found once and serve all the workgroup's columns.  Per (chunk, column): B loads,
// the wait for them, __syncthreads(), B stores.  Within a chunk every load precedes every store; chunk k stores below base + 256 B,
// chunk k + 1 loads at or above it.  Destination rows [m - nr, m) get 0.0, the value of the room rows; rows above rows[0] are not
// touched.
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_drop_rows(double* img, int64_t ld, int m, int n, const int32_t* __restrict__ rows,
                                                            int nr) {
    const int m_new = m - nr;
    for (int base = rows[0]; base < m; base += kThreads * B) {
        int src[B];
#pragma unroll
        for (int x = 0; x < B; ++x) {
            const int dst = base + x * kThreads + (int)threadIdx.x;
            int lo = 0, hi = nr;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rows[mid] - mid <= dst) lo = mid + 1; else hi = mid;
            }
            src[x] = dst < m_new ? dst + lo : -1;
        }
        for (int c = blockIdx.x; c < n; c += gridDim.x) {
            double* col = img + (int64_t)c * ld;
            double t[B];
#pragma unroll
            for (int x = 0; x < B; ++x) t[x] = src[x] >= 0 ? col[src[x]] : 0.0;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the loads have returned before any thread of the chunk stores
            __syncthreads();
#pragma unroll
            for (int x = 0; x < B; ++x) {
                const int dst = base + x * kThreads + (int)threadIdx.x;
                if (dst < m) col[dst] = t[x];
            }
        }
    }
}

// Row i = blockIdx.x * 64 + threadIdx.x of the image belongs to this thread alone (consecutive threads, consecutive rows of one
// column: the access pattern of k_tab_col_apply; 64 threads per workgroup so that 10,000 rows are 157 workgroups).  Destination
// columns ascending from the first removed column cols[0], B at a time: the B loads, then the B stores.  The source of dst is
// dst + #{removed columns <= source}, found by walking the list along (the same in every thread: scalar work); it lies at or right
// of dst, and right of every column the thread has written.  Destination columns [n - nc, n) get 0.0; columns left of cols[0] are
// not touched.
template <int B>
__global__ __launch_bounds__(64) void k_tab_drop_columns(double* img, int64_t ld, int m, int n, const int32_t* __restrict__ cols,
                                                         int nc) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= m) return;
    const int n_new = n - nc;
    double* row = img + i;
    int k = 0;                                         // removed columns left of the next source
    for (int dst = cols[0]; dst < n; dst += B) {
        double t[B];
#pragma unroll
        for (int x = 0; x < B; ++x) {
            t[x] = 0.0;
            if (dst + x < n_new) {
                int src = dst + x + k;
                while (k < nc && cols[k] <= src) { ++k; ++src; }
                t[x] = row[(int64_t)src * ld];
            }
        }
#pragma unroll
        for (int x = 0; x < B; ++x)
            if (dst + x < n) row[(int64_t)(dst + x) * ld] = t[x];
    }
}

// ------------------------------------------------------------------------------------------------
// Batched ratio tests over the tableau as it stands (relp_row_ratios, relp_rhs_ranging): read-only streams over T0 (+ W R0 while
// an update block is open, p = its pending rows).  Two launches each: [the minimum of every (list entry, block of 256 columns or
// rows) into scratch] -> [one workgroup per list entry: the minimum of its blocks, then the tie band from the blocks whose own
// minimum is inside it, their entries recomputed by the same fma chain].  Minima of (ratio, index) pairs and of keys only: no
// sums, no global atomics, the same call on the same state gives the same bits.
// ------------------------------------------------------------------------------------------------
// Rows rows[k0 .. k0 + RB) of T (k0 = blockIdx.x * RB) over the 256 stored columns of block blockIdx.y, one column per thread:
// d_c, the flag and the p entries of column c of R0 are loaded once and serve all RB rows; a sorted chunk's T0 entries of one
// column share a 64-byte sector.  Entry (u, c) = T0[rows[u], c], then fma over the pending rows in ascending j (tab_row_entry).
// part_k / part_j[(dir * count + k) * gridDim.y + blockIdx.y] = the block's minimum (ratio, column) of list entry k, dir 0 = down
// (entry < -tol_pivot, ratio d / -entry), 1 = up (entry > tol_pivot, ratio d / entry): dual_ratio on the entry with its sign turned.
template <int B, int RB>
__global__ __launch_bounds__(kThreads) void k_tab_row_ratios(TableauView tv, DeferredUpdate du, const uint8_t* __restrict__ in_basis,
                                                             Tolerances tol, const int32_t* __restrict__ rows, int count, int p,
                                                             double* __restrict__ part_k, int32_t* __restrict__ part_j) {
    __shared__ double s_w[RB * kMaxEta];
    __shared__ int s_rows[RB];
    __shared__ double s_k[2 * RB][kThreads / 64];
    __shared__ int s_j[2 * RB][kThreads / 64];
    const int k0 = blockIdx.x * RB, nk = min(RB, count - k0);
    if ((int)threadIdx.x < RB) s_rows[threadIdx.x] = rows[k0 + min((int)threadIdx.x, nk - 1)];     // (a short chunk repeats its last row)
    __syncthreads();
    for (int idx = threadIdx.x; idx < RB * p; idx += kThreads) {
        const int u = idx / p, j = idx - u * p;
        s_w[u * kMaxEta + j] = du.W[(int64_t)j * du.ld + s_rows[u]];
    }
    const int c = tv.c_lo + blockIdx.y * kThreads + threadIdx.x;
    const int j = c - tv.col_off;
    const bool live = c < tv.c_hi;
    double acc[RB];
    double d_c = 0.0;
    bool cand = false;
#pragma unroll
    for (int u = 0; u < RB; ++u) acc[u] = 0.0;
    if (live) {
        d_c = tv.d[c];
        cand = j >= 0 && j < tv.n && in_basis[j] == 0;
        const double* col = tv.T0 + (int64_t)c * tv.ld_t;
#pragma unroll
        for (int u = 0; u < RB; ++u) acc[u] = col[s_rows[u]];
    }
    __syncthreads();
    if (live) {
        for_pending<B>(tv.R0, tv.ld_r, c, p, [&](int jj, double r0) {
#pragma unroll
            for (int u = 0; u < RB; ++u) acc[u] = fma(s_w[u * kMaxEta + jj], r0, acc[u]);
        });
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < RB; ++u) {
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            double key = INFINITY;
            int kj = 0x7fffffff;
            const double v = dir ? -acc[u] : acc[u];
            if (cand && v < -tol.pivot) { key = dual_ratio(d_c, v, tol.zero); kj = j; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ok = __shfl_down(key, off, 64);
                const int oj = __shfl_down(kj, off, 64);
                if (ok < key || (ok == key && oj < kj)) { key = ok; kj = oj; }
            }
            if (lane == 0) { s_k[dir * RB + u][wave] = key; s_j[dir * RB + u][wave] = kj; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * RB) {
        const int dir = threadIdx.x / RB, u = threadIdx.x % RB;
        if (u < nk) {
            double key = s_k[threadIdx.x][0];
            int kj = s_j[threadIdx.x][0];
#pragma unroll
            for (int w = 1; w < kThreads / 64; ++w)
                if (s_k[threadIdx.x][w] < key || (s_k[threadIdx.x][w] == key && s_j[threadIdx.x][w] < kj)) {
                    key = s_k[threadIdx.x][w]; kj = s_j[threadIdx.x][w];
                }
            const int64_t slot = ((int64_t)dir * count + k0 + u) * gridDim.y + blockIdx.y;
            part_k[slot] = key;
            part_j[slot] = kj;
        }
    }
}

// List entry k = blockIdx.x, row r = rows[k]: per direction the entering rule of k_dual_select_column on the entry's nbc partials
// (select_entering: the minimum ratio, then the lowest column inside its tie band, from the entries recomputed by tab_row_entry).
// ratio / column[dir * count + k] = (the minimum, that column), (+inf, -1) without a candidate.
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_row_ratios_pick(TableauView tv, DeferredUpdate du, SelectPartials sp, Tolerances tol,
                                                                  const int32_t* __restrict__ rows, int count, int p, int nbc,
                                                                  double* part_k, int32_t* part_j, double* __restrict__ ratio,
                                                                  int32_t* __restrict__ column) {
    __shared__ double s_w[kMaxEta];
    const int k = blockIdx.x, r = rows[k];
    stage_w_row(du, r, p, s_w);
    __syncthreads();
    for (int dir = 0; dir < 2; ++dir) {
        SelectPartials spd = sp;
        spd.k1 = part_k + ((int64_t)dir * count + k) * nbc;
        spd.j = part_j + ((int64_t)dir * count + k) * nbc;
        double k1 = INFINITY;
        int bj = 0x7fffffff;
        select_entering<kThreads>(tv, spd, nbc, tol.tie, tol.tie > 0.0, false, k1, bj, [&](int c, int j, double bound) {
            if (sp.in_basis[j] != 0) return false;
            const double d_c = tv.d[c];
            const double e = tab_row_entry<B>(tv, c, p, s_w, tv.T0[(int64_t)c * tv.ld_t + r]);
            const double v = dir ? -e : e;
            return v < -tol.pivot && dual_ratio(d_c, v, tol.zero) <= bound;
        });
        if (threadIdx.x == 0) {
            const bool none = bj == 0x7fffffff;
            ratio[(int64_t)dir * count + k] = none ? INFINITY : k1;
            column[(int64_t)dir * count + k] = none ? -1 : bj;
        }
        __syncthreads();                               // (select_entering's LDS words before the other direction reuses them)
    }
}

// Stored columns cols[k0 .. k0 + CB) of T (k0 = blockIdx.x * CB) over the 256 rows of block blockIdx.y, one row per thread: b_i
// and the p entries of row i of W are loaded once and serve all CB columns, whose R0 columns are staged in LDS.  Entry (i, u) =
// T0[i, cols[u]], then fma over the pending rows in ascending j (tab_column_entry).  part[(dir * count + k) * gridDim.y +
// blockIdx.y] = the block's minimum ratio of list entry k, dir 0 = decrease (row_ratio on the entry), 1 = increase (on its negative).
template <int B, int CB>
__global__ __launch_bounds__(kThreads) void k_tab_rhs_ranging(TableauView tv, DeferredUpdate du, const double* __restrict__ b,
                                                              Tolerances tol, const int32_t* __restrict__ cols, int count, int p,
                                                              double* __restrict__ part) {
    __shared__ double s_r0[CB * kMaxEta];
    __shared__ int s_cols[CB];
    __shared__ double s_m[2 * CB][kThreads / 64];
    const int k0 = blockIdx.x * CB, nk = min(CB, count - k0);
    if ((int)threadIdx.x < CB) s_cols[threadIdx.x] = cols[k0 + min((int)threadIdx.x, nk - 1)];     // (a short chunk repeats its last column)
    __syncthreads();
    for (int idx = threadIdx.x; idx < CB * p; idx += kThreads) {
        const int u = idx / p, j = idx - u * p;
        s_r0[u * kMaxEta + j] = tv.R0[(int64_t)j * tv.ld_r + s_cols[u]];
    }
    const int i = blockIdx.y * kThreads + threadIdx.x;
    const bool live = i < tv.m;
    double acc[CB];
    double b_i = 0.0;
#pragma unroll
    for (int u = 0; u < CB; ++u) acc[u] = 0.0;
    if (live) {
        b_i = b[i];
#pragma unroll
        for (int u = 0; u < CB; ++u) acc[u] = tv.T0[(int64_t)s_cols[u] * tv.ld_t + i];
    }
    __syncthreads();
    if (live) {
        for_pending<B>(du.W, du.ld, i, p, [&](int jj, double w) {
#pragma unroll
            for (int u = 0; u < CB; ++u) acc[u] = fma(w, s_r0[u * kMaxEta + jj], acc[u]);
        });
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < CB; ++u) {
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            double ratio = live ? row_ratio(dir ? -acc[u] : acc[u], b_i, tol) : INFINITY;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) ratio = fmin(ratio, __shfl_down(ratio, off, 64));
            if (lane == 0) s_m[dir * CB + u][wave] = ratio;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * CB) {
        const int dir = threadIdx.x / CB, u = threadIdx.x % CB;
        if (u < nk) {
            double ratio = s_m[threadIdx.x][0];
#pragma unroll
            for (int w = 1; w < kThreads / 64; ++w) ratio = fmin(ratio, s_m[threadIdx.x][w]);
            part[((int64_t)dir * count + k0 + u) * gridDim.y + blockIdx.y] = ratio;
        }
    }
}

// List entry k = blockIdx.x, column c = cols[k]: per direction the reference ratio test on the entry's nbr block minima
// (block_minima_pick: the minimum ratio, then the smallest leaving column among the rows inside its tie band, their entries
// recomputed by tab_column_entry).  ratio / row[dir * count + k] = (the minimum, that row), (+inf, -1) without a candidate.
template <int B>
__global__ __launch_bounds__(kThreads) void k_tab_rhs_ranging_pick(TableauView tv, DeferredUpdate du, const double* __restrict__ b,
                                                                   const int32_t* __restrict__ basis_indices, Tolerances tol,
                                                                   const int32_t* __restrict__ cols, int count, int p, int nbr,
                                                                   const double* part, double* __restrict__ ratio,
                                                                   int32_t* __restrict__ row) {
    __shared__ double s_vs[kMaxEta];
    const int k = blockIdx.x, c = cols[k];
    if ((int)threadIdx.x < p) s_vs[threadIdx.x] = tv.R0[(int64_t)threadIdx.x * tv.ld_r + c];
    __syncthreads();
    for (int dir = 0; dir < 2; ++dir) {
        const double* minima = part + ((int64_t)dir * count + k) * nbr;
        double mn = INFINITY;
        for (int t = threadIdx.x; t < nbr; t += kThreads) mn = fmin(mn, minima[t]);
        const double gmin = block_min_value<kThreads>(mn);
        __syncthreads();                               // (block_minima_pick makes the same reduction)
        int r, leaving;
        block_minima_pick<kThreads>(minima, nbr, kThreads, tv.m, tol.tie, INFINITY, false, false, &r, &leaving, [&](int i, double bound) {
            const double a = tab_column_entry<B>(du, i, p, s_vs, tv.T0[(int64_t)c * tv.ld_t + i]);
            const double bi = b[i];
            const int lv = basis_indices[i];
            return row_ratio(dir ? -a : a, bi, tol) <= bound ? tie_key(0.0, lv, 0) : kNoTieKey;
        });
        if (threadIdx.x == 0) {
            ratio[(int64_t)dir * count + k] = gmin;    // (+inf when no row qualifies)
            row[(int64_t)dir * count + k] = r;         // (-1 then)
        }
        __syncthreads();                               // (the pick's LDS words before the other direction reuses them)
    }
}

// ------------------------------------------------------------------------------------------------
// Gomory cuts from rows of the tableau as it stands (relp_gomory_cuts): the row stream of k_tab_row_ratios with the rounding rule
// on every entry, then the virtual columns substituted out through their rows over the dense A.  Read-only on the tableau; every
// sum has a fixed order, no atomics: the same call on the same state gives the same bits.
// ------------------------------------------------------------------------------------------------
// The coefficient pi_j of a non-basic column from its entry a of the row, the row's fraction f0 and the column's flag (kind 0 =
// fractional, 1 = mixed).  Every difference, product and quotient is rounded once, in the order written, nothing is contracted.
// *bad: a continuous column with |a| > tol_zero in a fractional cut (the entry is skipped by the host).
__device__ __forceinline__ double gomory_pi(double a, double f0, bool integer, int kind, double tol_zero, bool* bad) {
#pragma clang fp contract(off)
    if (fabs(a) <= tol_zero) return 0.0;
    if (integer) {
        const double f = a - floor(a);
        if (f <= tol_zero || f >= 1.0 - tol_zero) return 0.0;
        if (kind == 0 || f <= f0) return f;
        const double num = f0 * (1.0 - f);
        return num / (1.0 - f0);
    }
    if (kind == 0) { *bad = true; return 0.0; }
    if (a > 0.0) return a;
    const double num = f0 * (-a);
    return num / (1.0 - f0);
}

// Rows rows[k0 .. k0 + RB) of T (k0 = blockIdx.x * RB) over the 256 stored columns of block blockIdx.y, one column per thread, the
// entries formed as in k_tab_row_ratios: one T0 load per row, the R0 column shared by all RB, fma over the pending rows in
// ascending j (tab_row_entry).  Written per entry k of the chunk: pi[k][c - c_lo] = gomory_pi of the entry for a non-basic
// tableau column (flag != 1: a barred column counts), exactly 0.0 for a basic one, for the kept artificial block in front of
// col_off and for a skipped entry (f0 < 0); y[k][vrow0[v]] = vsign[v] * pi where c is the virtual column v with a row;
// bad[k * gridDim.y + blockIdx.y] = 1.0 if any column of the block was bad for entry k, else 0.0.
template <int B, int RB>
__global__ __launch_bounds__(kThreads) void k_tab_gomory_rows(TableauView tv, DeferredUpdate du, ColumnTable ct,
                                                              const uint8_t* __restrict__ in_basis, double tol_zero, GomoryCuts gc, int p) {
    __shared__ double s_w[RB * kMaxEta];
    __shared__ int s_rows[RB];
    __shared__ double s_f0[RB];
    const int k0 = blockIdx.x * RB, nk = min(RB, gc.count - k0);
    if ((int)threadIdx.x < RB) {
        const int k = k0 + min((int)threadIdx.x, nk - 1);  // (a short chunk repeats its last row)
        s_rows[threadIdx.x] = gc.rows[k];
        s_f0[threadIdx.x] = gc.f0[k];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < RB * p; idx += kThreads) {
        const int u = idx / p, j = idx - u * p;
        s_w[u * kMaxEta + j] = du.W[(int64_t)j * du.ld + s_rows[u]];
    }
    const int c = tv.c_lo + blockIdx.y * kThreads + threadIdx.x;
    const int j = c - tv.col_off;
    const bool live = c < tv.c_hi;
    double acc[RB];
    bool cand = false, integer = true;
#pragma unroll
    for (int u = 0; u < RB; ++u) acc[u] = 0.0;
    if (live) {
        cand = j >= 0 && j < tv.n && in_basis[j] != 1;
        if (cand && gc.is_integer) integer = gc.is_integer[j] != 0;
        const double* col = tv.T0 + (int64_t)c * tv.ld_t;
#pragma unroll
        for (int u = 0; u < RB; ++u) acc[u] = col[s_rows[u]];
    }
    __syncthreads();
    if (live && cand) {
        for_pending<B>(tv.R0, tv.ld_r, c, p, [&](int jj, double r0) {
#pragma unroll
            for (int u = 0; u < RB; ++u) acc[u] = fma(s_w[u * kMaxEta + jj], r0, acc[u]);
        });
    }
    // the row of the virtual column's slack and its sign (0: c is no virtual column with a row)
    int y_row = -1, y_sign = 0;
    if (live && j >= ct.nr_artificial + ct.nr_normal) {
        const int v = j - ct.nr_artificial - ct.nr_normal;
        if (v < ct.nr_virtual && ct.vrow0[v] >= 0 && ct.vrow0[v] < tv.m) { y_row = ct.vrow0[v]; y_sign = ct.vsign[v]; }
    }
    const int n_st = tv.c_hi - tv.c_lo;
#pragma unroll
    for (int u = 0; u < RB; ++u) {
        bool bad = false;
        const double f0 = s_f0[u];
        const double v = (cand && f0 >= 0.0) ? gomory_pi(acc[u], f0, integer, gc.kind, tol_zero, &bad) : 0.0;
        if (live && u < nk) {
            gc.pi[(int64_t)(k0 + u) * n_st + (c - tv.c_lo)] = v;
            if (y_row >= 0) gc.y[(int64_t)(k0 + u) * tv.m + y_row] = y_sign < 0 ? -v : v;
        }
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (threadIdx.x == 0 && u < nk) gc.bad[(int64_t)(k0 + u) * gridDim.y + blockIdx.y] = any ? 1.0 : 0.0;
    }
}

// Structural column sp = blockIdx.x, the RB cuts from k0 = blockIdx.y * RB on together; lanes run along the rows of the column of A
// (coalesced), and every load of A serves the chunk.  Thread t chains  acc[u] = fma(y[k0 + u][row(i)], A[i, sp], acc[u])  over the
// rows i = t, t + 256, .. of A in ascending order from 0.0, the loads of A min(B, 16) at a time (for_pending); row(i) = i for a constraint
// row, cut_row0 + (i - nr_constraints) for a cut row.  Then the fixed halving tree of list_sum over the 256 chains of every cut,
// and g[k][sp] = (sum - pi[k][sp]) + y[k][bound_row(sp)], the last term only where sp has a bound row.
template <int B, int RB>
__global__ __launch_bounds__(kThreads) void k_tab_gomory_structural(TableauView tv, ColumnTable ct, GomoryCuts gc) {
    __shared__ double s_sum[RB][kThreads];
    const int sp = blockIdx.x;
    const int k0 = blockIdx.y * RB, nk = min(RB, gc.count - k0);
    const int n_a = ct.nr_constraints + ct.nr_cuts;
    const int t = threadIdx.x;
    const double* y[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) y[u] = gc.y + (int64_t)(k0 + min(u, nk - 1)) * tv.m;     // (a short chunk repeats its last cut)
    double acc[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) acc[u] = 0.0;
    constexpr int BA = B > 16 ? 16 : B;                // (32 loads in flight beside 8 chains and 8 row pointers spill scalar registers)
    for_pending<BA>(gc.A + (int64_t)sp * gc.ld_a, kThreads, t, t < n_a ? (n_a - t + kThreads - 1) / kThreads : 0, [&](int jj, double a) {
        const int i = jj * kThreads + t;
        const int row = i < ct.nr_constraints ? i : ct.cut_row0 + (i - ct.nr_constraints);
#pragma unroll
        for (int u = 0; u < RB; ++u) acc[u] = fma(y[u][row], a, acc[u]);
    });
#pragma unroll
    for (int u = 0; u < RB; ++u) s_sum[u][t] = acc[u];
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int u = 0; u < RB; ++u) s_sum[u][t] += s_sum[u][t + half];
        }
        __syncthreads();
    }
    if (t < nk) {
        const int c = gc.struct_c0 + sp;
        double v = s_sum[t][0] - gc.pi[(int64_t)(k0 + t) * (tv.c_hi - tv.c_lo) + (c - tv.c_lo)];
        const int br = ct.bound_row[sp];
        if (br >= 0 && br < tv.m) v = v + gc.y[(int64_t)(k0 + t) * tv.m + br];
        gc.g[(int64_t)(k0 + t) * gc.nr_normal + sp] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// The snapshot of a trial (relp_trial_begin / relp_trial_end): up to kTrialMaxSegments copies src -> dst in ONE launch, the table
// passed by value (relp_trial.hpp: the planner).  The grid strides over the 16-byte units of all segments together: unit u belongs
// to the segment s with unit_end[s - 1] <= u < unit_end[s], found by a walk over the table that is the same for every lane (the
// table is read through scalar loads, never indexed by a lane).  Per stride iteration a thread owns kTrialB units a grid stride
// apart: their loads are all issued before the first store, as in k_tab_drop_rows.  The bytes % 16 bytes behind the last unit of
// a segment are copied bytewise by the first lanes of workgroup 0.  Sources and destinations never overlap (live arrays against
// the snapshot buffer).  Copies only: no atomics, no LDS, no communication between workgroups.
// ------------------------------------------------------------------------------------------------
static constexpr int kTrialB = 4;
// unit u of the table: its source and destination, nullptr past the last unit (the walk is the same for every lane)
__device__ __forceinline__ void trial_locate(const TrialTable& t, int64_t u, const uint4*& src, uint4*& dst) {
    src = nullptr; dst = nullptr;
    int64_t begin = 0;
    for (int s = 0; s < t.count; ++s) {
        const int64_t end = t.unit_end[s];
        if (u >= begin && u < end) {
            src = static_cast<const uint4*>(t.seg[s].src) + (u - begin);
            dst = static_cast<uint4*>(t.seg[s].dst) + (u - begin);
        }
        begin = end;
    }
}

__global__ __launch_bounds__(kThreads) void k_tab_trial_copy(TrialTable t) {
    static_assert(kTrialB == 4, "the four units of a stride iteration are written out below");
    const int64_t total = t.count > 0 ? t.unit_end[t.count - 1] : 0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int64_t base = first; base < total; base += stride * kTrialB) {
        const uint4 *s0, *s1, *s2, *s3;
        uint4 *d0, *d1, *d2, *d3;
        trial_locate(t, base, s0, d0);
        trial_locate(t, base + stride, s1, d1);
        trial_locate(t, base + 2 * stride, s2, d2);
        trial_locate(t, base + 3 * stride, s3, d3);
        uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0, v2 = v0, v3 = v0;
        if (s0) v0 = *s0;
        if (s1) v1 = *s1;
        if (s2) v2 = *s2;
        if (s3) v3 = *s3;
        if (s0) *d0 = v0;
        if (s1) *d1 = v1;
        if (s2) *d2 = v2;
        if (s3) *d3 = v3;
    }
    if (blockIdx.x == 0 && threadIdx.x < kTrialUnit) {
        for (int s = 0; s < t.count; ++s) {
            const int64_t bytes = t.seg[s].bytes, whole = bytes / kTrialUnit * kTrialUnit;
            if (whole + (int64_t)threadIdx.x < bytes)
                static_cast<uint8_t*>(t.seg[s].dst)[whole + threadIdx.x] = static_cast<const uint8_t*>(t.seg[s].src)[whole + threadIdx.x];
        }
    }
}

int32_t tab_scan_blocks(int32_t n_owned_columns) { return cdiv(n_owned_columns, kThreads); }

// The batch sizes of for_pending the kernels are instantiated for (DeferredUpdate::batch, RELP_TAB_LOAD_BATCH).  1 is the
// serial loop, the control; the default measured best on dense10k (profiles/r06_tab_load_batch.md).
int32_t tab_load_batch(int32_t wanted) {
    return (wanted == 1 || wanted == 8 || wanted == 16 || wanted == 32) ? wanted : kTabLoadBatchDefault;
}

// RELP_TAB_COLUMN_ROWS / DeferredUpdate::col_rows: 256, 128 and 64 are themselves; anything else is the smallest of them that
// keeps the column kernel within one workgroup per CU (kTabSplitCUs).
int32_t tab_column_rows(int32_t wanted, int32_t m) {
    if (wanted == 64 || wanted == 128 || wanted == kThreads) return wanted;
    for (int32_t rows : {64, 128})
        if (cdiv(m, rows) <= kTabSplitCUs) return rows;
    return kThreads;
}

// Rows per workgroup of k_tab_select_column and per minimum in rmin for this DeferredUpdate: 256 unless the caller asked for
// 128 or 64.
static int column_rows_of(const DeferredUpdate& du) { return du.col_rows == 64 || du.col_rows == 128 ? du.col_rows : kThreads; }

// launch(std::integral_constant<int, B>) for B = tab_load_batch(batch)
template <class Launch>
static void with_load_batch(int32_t batch, Launch&& launch) {
    switch (tab_load_batch(batch)) {
    case 1:  launch(std::integral_constant<int, 1>{}); break;
    case 16: launch(std::integral_constant<int, 16>{}); break;
    case 32: launch(std::integral_constant<int, 32>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
    }
    static_assert(kTabLoadBatchDefault == 8, "the default of tab_load_batch is the switch's default case");
}

void launch_tab_build(const TableauView& tv, const double* A, int64_t ld_a, const ColumnTable& ct, hipStream_t s) {
    const int64_t total = (int64_t)tv.m * (tv.c_hi - tv.c_lo);
    if (total <= 0) return;
    hipLaunchKernelGGL(k_tab_build, dim3(element_blocks(total)), dim3(256), 0, s, tv, A, ld_a, ct);
}

void launch_tab_price_init(const TableauView& tv, const double* w, const double* cost_store, hipStream_t s) {
    if (tv.c_hi <= tv.c_lo) return;
    hipLaunchKernelGGL(k_tab_price_init, dim3(cdiv(tv.c_hi - tv.c_lo, kVecPerBlock)), dim3(kThreads), 0, s, tv, w,
                       cost_store);
}

void launch_tab_basis_costs(const TableauView& tv, const int32_t* basis_indices, const double* cost_store, double* w,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_tab_basis_costs, dim3(cdiv(tv.m, 256)), dim3(256), 0, s, basis_indices, cost_store, tv.col_off,
                       tv.n_store, tv.m, w);
}

void launch_tab_scan(const TableauView& tv, SelectPartials sp, const PivotRecord* rec, hipStream_t s) {
    if (tv.c_hi <= tv.c_lo) return;
    hipLaunchKernelGGL(k_tab_scan, dim3(tab_scan_blocks(tv.c_hi - tv.c_lo)), dim3(kThreads), 0, s, tv, sp, rec);
}

void launch_tab_select(const TableauView& tv, SelectPartials sp, int32_t count, PivotRecord* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_tab_select, dim3(1), dim3(kSingleBlock), 0, s, tv, sp, count, rec);
}

void launch_tab_column(const TableauView& tv, const DeferredUpdate& du, double* alpha, const PivotRecord* rec,
                       hipStream_t s) {
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_column<decltype(B)::value>), dim3(cdiv(tv.m, kThreads)), dim3(kThreads), 0, s, tv, du, alpha, rec);
    });
}

void launch_tab_row_update(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, PivotRecord* rec,
                           hipStream_t s) {
    if (tv.c_hi <= tv.c_lo) return;
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_row_update<decltype(B)::value>), dim3(tab_scan_blocks(tv.c_hi - tv.c_lo)), dim3(kThreads), 0, s, tv, du, sp,
                           rec);
    });
}

void launch_tab_update_vectors(int32_t m, const double* alpha, double* b, int32_t* basis_indices, uint8_t* in_basis,
                               int32_t* trace, int64_t trace_cap, PivotRecord* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_tab_update_vectors, dim3(cdiv(m, 256)), dim3(256), 0, s, m, alpha, b, basis_indices, in_basis,
                       trace, trace_cap, rec);
}

void launch_tab_select_column_rmin(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t count,
                                   double* alpha, const double* b, Tolerances tol, double* rmin, PivotRecord* rec,
                                   hipStream_t s, const double* shadow, int32_t* shadow_meta) {
    const int rows = column_rows_of(du);
    if (rows == kThreads) {
        with_load_batch(du.batch, [&](auto B) {
            hipLaunchKernelGGL((k_tab_select_column<decltype(B)::value, kThreads, 1>), dim3(cdiv(tv.m, kThreads)), dim3(kThreads), 0, s, tv, du, sp,
                               count, alpha, (double*)nullptr, b, tol, rmin, rec, shadow, shadow_meta);
        });
        return;
    }
    // the registers of a slice hold its whole share of the pending rows: the smallest array that takes ceil(kmax / S)
    const int need = cdiv(du.kmax, kThreads / rows);
    static_assert(kMaxEta <= 2 * 64, "the largest array takes half of the pending rows");
    auto launch = [&](auto R, auto NW) {
        hipLaunchKernelGGL((k_tab_select_column<kTabLoadBatchDefault, decltype(R)::value, decltype(NW)::value>), dim3(cdiv(tv.m, rows)),
                           dim3(kThreads), 0, s, tv, du, sp, count, alpha, (double*)nullptr, b, tol, rmin, rec, shadow, shadow_meta);
    };
    static_assert(kMaxEta <= 4 * 32, "32 registers take a quarter of the pending rows");
    if (need <= 16) {
        if (rows == 128) launch(std::integral_constant<int, 128>{}, std::integral_constant<int, 16>{});
        else launch(std::integral_constant<int, 64>{}, std::integral_constant<int, 16>{});
    } else if (need <= 32) {
        if (rows == 128) launch(std::integral_constant<int, 128>{}, std::integral_constant<int, 32>{});
        else launch(std::integral_constant<int, 64>{}, std::integral_constant<int, 32>{});
    } else {
        launch(std::integral_constant<int, 128>{}, std::integral_constant<int, 64>{});       // (two slices only)
    }
}

void launch_tab_ratio_update_all(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t m,
                                 const double* alpha, const double* b_in, double* b_out, const int32_t* basis_in,
                                 int32_t* basis_out, uint8_t* in_basis, int32_t* trace, int64_t trace_cap, Tolerances tol,
                                 const double* rmin, double* shadow, int32_t* shadow_meta, PivotRecord* rec, hipStream_t s,
                                 const double* msgs, int32_t count, int64_t msg_len, int32_t rule) {
    const int nb_row = tv.c_hi > tv.c_lo ? tab_scan_blocks(tv.c_hi - tv.c_lo) : 0;
    const int nb_w = cdiv(m, kThreads);
    // the minima the column kernel left: one per 256 rows in a message, else one per column_rows_of(du) rows
    const int rpb = msgs ? kThreads : column_rows_of(du);
    // the W half over `split` workgroups per 256 rows, as far as the whole grid still fits one workgroup per CU (past that
    // the extra workgroups queue behind the others and only repeat the ratio test); never under batch 1, the control
    int split = tab_load_batch(du.batch) == 1 ? 1 : std::max(1, std::min({(int)du.w_split, (int)du.kmax, (kTabSplitCUs - nb_row) / nb_w}));
    auto launch = [&](auto B, auto RPB) {
        hipLaunchKernelGGL((k_tab_ratio_update_all<decltype(B)::value, decltype(RPB)::value>), dim3(nb_row + split * nb_w), dim3(kThreads), 0, s,
                           tv, du, sp, nb_row, m, alpha, b_in, b_out, basis_in, basis_out, in_basis, trace, trace_cap, tol, rmin,
                           cdiv(m, rpb), nb_w, shadow, shadow_meta, rec, msgs, (int)count, msg_len, (int)rule, split);
    };
    with_load_batch(du.batch, [&](auto B) {
        if (rpb == 64) launch(B, std::integral_constant<int, 64>{});
        else if (rpb == 128) launch(B, std::integral_constant<int, 128>{});
        else launch(B, std::integral_constant<int, kThreads>{});
    });
}

void launch_tab_apply_shadow(const DeferredUpdate& du, double* shadow, int32_t* shadow_meta, hipStream_t s) {
    hipLaunchKernelGGL(k_tab_apply_shadow, dim3(1), dim3(128), 0, s, du, shadow, shadow_meta);
}

void launch_ratio_blocks(const double* alpha, const double* b, const int32_t* basis_indices, int32_t m, Tolerances tol,
                         const DeferredUpdate& du, const double* rmin, PivotRecord* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_ratio_blocks, dim3(1), dim3(kSingleBlock), 0, s, alpha, b, basis_indices, m, tol, du, rmin,
                       cdiv(m, kThreads), rec);
}

void launch_tab_select_column_msg(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t count,
                                  double* msg, const double* b, Tolerances tol, PivotRecord* rec, hipStream_t s,
                                  const double* shadow, int32_t* shadow_meta) {
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_select_column<decltype(B)::value, kThreads, 1>), dim3(cdiv(tv.m, kThreads)), dim3(kThreads), 0, s, tv, du, sp, count, msg + 3,
                           msg, b, tol, msg + 3 + tv.m, rec, shadow, shadow_meta);
    });
}

void launch_tab_select_candidate_ratio(const double* msgs, int32_t count, int64_t msg_len, int32_t m, double* alpha,
                                       const double* b, const int32_t* basis_indices, int32_t rule, Tolerances tol,
                                       const DeferredUpdate& du, int32_t forced_row, PivotRecord* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_tab_select_candidate_ratio, dim3(1), dim3(kSingleBlock), 0, s, msgs, count, msg_len, m, alpha, b,
                       basis_indices, rule, tol, du, forced_row, rec);
}

void launch_tab_zero_level_scan(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t row,
                                int32_t nr_artificial, Tolerances tol, const PivotRecord* rec, hipStream_t s) {
    if (tv.c_hi <= tv.c_lo) return;
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_zero_level_scan<decltype(B)::value>), dim3(tab_scan_blocks(tv.c_hi - tv.c_lo)), dim3(kThreads), 0, s, tv, du, sp,
                           row, nr_artificial, tol, rec);
    });
}

void launch_tab_update_all(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t m,
                           const double* alpha, double* b, int32_t* basis_indices, uint8_t* in_basis, int32_t* trace,
                           int64_t trace_cap, PivotRecord* rec, hipStream_t s) {
    const int nb_row = tv.c_hi > tv.c_lo ? tab_scan_blocks(tv.c_hi - tv.c_lo) : 0;
    const int nb_w = cdiv(m, kThreads);
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_update_all<decltype(B)::value>), dim3(nb_row + nb_w), dim3(kThreads), 0, s, tv, du, sp, nb_row, m, alpha, b,
                           basis_indices, in_basis, trace, trace_cap, rec);
    });
}

void launch_tab_flush(const TableauView& tv, const DeferredUpdate& du, const PivotRecord* rec, const FlushList& fl,
                      hipStream_t s) {
    if (tv.c_hi <= tv.c_lo) return;
    const int ncols = tv.c_hi - tv.c_lo;
    const int32_t* p_dev = &rec->n_eta;
    if ((int64_t)ncols * tv.m >= (1 << 16)) {
        // LDS-staged operands: 8 wavefronts, 128 columns x 128 rows per workgroup, chunks of 16 pivots
        // (64 KB of LDS, <= 128 VGPRs: two workgroups per CU, so one streams its T0 tile while the
        // other one is in its MFMA loop)
        constexpr int WC = 2, WR = 4, KC = 16;
        dim3 grid(cdiv(tv.m, WR * 32), cdiv(ncols, WC * 64));
        if (fl.cols) {
            // only the listed columns; the host reads nothing back, the grid stays sized for all of them
            const int nb = cdiv(ncols, 64);
            hipLaunchKernelGGL(k_tab_flush_mark, dim3(nb), dim3(kThreads), 0, s, tv, fl, p_dev);
            hipLaunchKernelGGL(k_tab_flush_compact, dim3(nb), dim3(kThreads), 0, s, tv, fl, p_dev, nb);
            hipLaunchKernelGGL((k_tab_flush_lds<WC, WR, KC, true>), grid, dim3(WC * WR * 64), 0, s, tv, du, p_dev, fl);
        } else {
            hipLaunchKernelGGL((k_tab_flush_lds<WC, WR, KC, false>), grid, dim3(WC * WR * 64), 0, s, tv, du, p_dev, fl);
        }
        return;
    }
    constexpr int MT = 4, NT = 2;      // wavefront tile 64 columns x 32 rows, workgroup 128 x 64 (every owned column)
    dim3 grid(cdiv(ncols, 2 * 16 * MT), cdiv(tv.m, 2 * 16 * NT));
    hipLaunchKernelGGL((k_tab_flush<MT, NT>), grid, dim3(kThreads), 0, s, tv, du, p_dev, fl.stats);
}

void launch_tab_gather_columns(const TableauView& tv, const int32_t* cols, double* out, hipStream_t s) {
    const int64_t total = (int64_t)tv.m * tv.m;
    hipLaunchKernelGGL(k_tab_gather_columns, dim3(element_blocks(total)), dim3(256), 0, s, tv, cols, out);
}

void launch_tab_row(const TableauView& tv, const DeferredUpdate& du, int32_t row, double* out, const PivotRecord* rec,
                    hipStream_t s) {
    if (tv.c_hi <= tv.c_lo) return;
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_row<decltype(B)::value>), dim3(tab_scan_blocks(tv.c_hi - tv.c_lo)), dim3(kThreads), 0, s, tv, du, row, out, rec);
    });
}

void launch_dual_bmin(const double* b, int32_t m, double tol_feas, double* bmin, const PivotRecord* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_dual_bmin, dim3(cdiv(m, kThreads)), dim3(kThreads), 0, s, b, m, tol_feas, bmin, rec);
}

void launch_dual_select_row(const double* b, const int32_t* basis_indices, int32_t m, double tol_feas, double tol_tie,
                            const double* bmin, PivotRecord* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_dual_select_row, dim3(1), dim3(kSingleBlock), 0, s, b, basis_indices, m, tol_feas, tol_tie, bmin,
                       cdiv(m, kThreads), rec);
}

void launch_dual_row(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, const double* b,
                     const int32_t* basis_indices, Tolerances tol, double tol_feas, const double* bmin, int32_t forced_row,
                     double* row, const PivotRecord* rec, hipStream_t s) {
    if (tv.c_hi <= tv.c_lo) return;
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_dual_row<decltype(B)::value>), dim3(tab_scan_blocks(tv.c_hi - tv.c_lo)), dim3(kThreads), 0, s, tv, du, sp, b,
                           basis_indices, tol, tol_feas, bmin, cdiv(tv.m, kThreads), (int)forced_row, row, rec);
    });
}

void launch_dual_select_column(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, const double* b,
                               const int32_t* basis_indices, Tolerances tol, double tol_feas, const double* bmin,
                               int32_t forced_row, const double* row, double* alpha, PivotRecord* rec, hipStream_t s) {
    const int count = tv.c_hi > tv.c_lo ? tab_scan_blocks(tv.c_hi - tv.c_lo) : 0;
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_dual_select_column<decltype(B)::value>), dim3(cdiv(tv.m, kThreads)), dim3(kThreads), 0, s, tv, du, sp, count, b,
                           basis_indices, tol, tol_feas, bmin, cdiv(tv.m, kThreads), (int)forced_row, row, alpha, rec);
    });
}

void launch_dual_commit(const double* alpha, const double* b, const DeferredUpdate& du, PivotRecord* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_dual_commit, dim3(1), dim3(kSingleBlock), 0, s, alpha, b, du, rec);
}

int32_t tab_rhs_splits(int32_t m, int32_t count, int32_t forced) {
    if (count < 1) return 1;
    if (forced >= 1) return std::min({forced, count, kTabRhsMaxSplits});
    const int32_t fill = kTabRhsGrid / cdiv(m, kThreads);              // splits until the grid covers the device ...
    return std::max(1, std::min({fill, count / kThreads, kTabRhsMaxSplits}));   // ... each with a full LDS chunk of the list
}

void launch_tab_rhs_change(const TableauView& tv, const DeferredUpdate& du, const RhsChange& ch, int32_t p, int32_t splits,
                           double* v, double* b, double* partial, int64_t ld_partial, hipStream_t s) {
    if (ch.count < 1) return;
    if (p > 0) hipLaunchKernelGGL(k_tab_rhs_pending, dim3(p), dim3(kThreads), 0, s, tv, ch, v);
    const int nb = cdiv(tv.m, kThreads);
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_rhs_apply<decltype(B)::value>), dim3(nb, splits), dim3(kThreads), 0, s, tv, du, ch, (int)p, v, b, partial,
                           ld_partial);
    });
    if (splits > 1) hipLaunchKernelGGL(k_tab_rhs_reduce, dim3(nb), dim3(kThreads), 0, s, (int)tv.m, (int)splits, partial, ld_partial, b);
}

int32_t tab_cost_splits(int32_t n_columns, int32_t count, int32_t forced) {
    if (count < 1) return 1;
    if (forced >= 1) return std::min({forced, count, kTabCostMaxSplits});
    const int32_t fill = kTabCostGrid / cdiv(n_columns, kThreads);     // splits until the grid covers the device five times ...
    return std::max(1, std::min({fill, count / kTabCostShareMin, kTabCostMaxSplits}));  // ... each with three load batches of the list
}

void launch_tab_cost_change(const TableauView& tv, const DeferredUpdate& du, const CostChange& ch, const uint8_t* in_basis, int32_t p,
                            int32_t splits, double* u, double* partial, int64_t ld_partial, hipStream_t s) {
    if ((ch.count < 1 && ch.ncount < 1) || tv.c_hi <= tv.c_lo) return;
    if (ch.count < 1) { p = 0; splits = 1; }           // only direct terms: no row of the tableau is read
    if (p > 0) hipLaunchKernelGGL(k_tab_cost_pending, dim3(p), dim3(kThreads), 0, s, du, ch, u);
    const int nb = tab_scan_blocks(tv.c_hi - tv.c_lo);
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_cost_apply<decltype(B)::value>), dim3(nb, splits), dim3(kThreads), 0, s, tv, ch, in_basis, (int)p, u, partial,
                           ld_partial);
    });
    if (splits > 1) hipLaunchKernelGGL(k_tab_cost_reduce, dim3(nb), dim3(kThreads), 0, s, tv, in_basis, (int)splits, partial, ld_partial);
}

void launch_tab_add_cuts(const TableauView& tv, const DeferredUpdate& du, const CutRows& cr, const uint8_t* in_basis, int32_t p, double* u,
                         const CutTail& ct, hipStream_t s) {
    if (cr.count < 1) return;
    if (cr.entries < 1) p = 0;                         // no row of the tableau is read: every u would be 0
    if (p > 0) hipLaunchKernelGGL(k_tab_cut_pending, dim3(p, cr.count), dim3(kThreads), 0, s, du, cr, u);
    if (tv.c_hi > tv.c_lo)
        with_load_batch(du.batch, [&](auto B) {
            hipLaunchKernelGGL((k_tab_cut_rows<decltype(B)::value>), dim3(tab_scan_blocks(tv.c_hi - tv.c_lo), cdiv(cr.count, kTabCutTile)),
                               dim3(kThreads), 0, s, tv, cr, in_basis, (int)p, u, (int)du.kmax);
        });
    const int64_t total = (int64_t)(tv.m + cr.count + ct.r0_rows + du.kmax + 1) * cr.count;
    hipLaunchKernelGGL(k_tab_cut_tail, dim3(element_blocks(total)), dim3(256), 0, s, tv, du, ct, (int)cr.count);
}

void launch_tab_add_columns(const TableauView& tv, const DeferredUpdate& du, const ColumnAdd& ca, int32_t p, const ColumnTail& ct,
                            hipStream_t s) {
    if (ca.count < 1) return;
    if (tv.m > 0)
        with_load_batch(du.batch, [&](auto B) {
            hipLaunchKernelGGL((k_tab_col_apply<decltype(B)::value>), dim3(cdiv(tv.m, kThreads), cdiv(ca.count, kTabColTile)), dim3(kThreads), 0,
                               s, tv, ca);
        });
    const int64_t total = (int64_t)(ct.r0_rows + 1) * ca.count;
    hipLaunchKernelGGL(k_tab_col_tail, dim3(element_blocks(total)), dim3(256), 0, s, tv, du, ca, ct, (int)p);
}

void launch_tab_compact(double* img, int64_t ld, int32_t m, int32_t n, const int32_t* rows, int32_t nr, const int32_t* cols, int32_t nc,
                        int32_t batch, hipStream_t s) {
    if (m < 1 || n < 1 || nr < 0 || nc < 0 || nr > m || nc > n) return;
    auto with_batch = [&](auto&& launch) {
        if (batch == 1) launch(std::integral_constant<int, 1>{}); else launch(std::integral_constant<int, kTabCompactB>{});
    };
    if (nr > 0)                                        // (all n columns: the vacated rows of a column that goes are cleared too)
        with_batch([&](auto B) {
            hipLaunchKernelGGL((k_tab_drop_rows<decltype(B)::value>), dim3(std::min(n, kTabCompactGrid)), dim3(kThreads), 0, s, img, ld, (int)m, (int)n,
                               rows, (int)nr);
        });
    if (nc > 0 && m - nr > 0)
        with_batch([&](auto B) {
            hipLaunchKernelGGL((k_tab_drop_columns<decltype(B)::value>), dim3(cdiv(m - nr, 64)), dim3(64), 0, s, img, ld, (int)(m - nr), (int)n, cols,
                               (int)nc);
        });
}

void launch_tab_row_ratios(const TableauView& tv, const DeferredUpdate& du, const SelectPartials& sp, Tolerances tol,
                           const int32_t* rows, int32_t count, int32_t p, double* part_k, int32_t* part_j, double* ratio,
                           int32_t* column, hipStream_t s) {
    if (count < 1 || tv.c_hi <= tv.c_lo) return;
    const int nbc = tab_scan_blocks(tv.c_hi - tv.c_lo);
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_row_ratios<decltype(B)::value, kTabRatioChunk>), dim3(cdiv(count, kTabRatioChunk), nbc), dim3(kThreads), 0,
                           s, tv, du, sp.in_basis, tol, rows, (int)count, (int)p, part_k, part_j);
        hipLaunchKernelGGL((k_tab_row_ratios_pick<decltype(B)::value>), dim3(count), dim3(kThreads), 0, s, tv, du, sp, tol, rows, (int)count,
                           (int)p, nbc, part_k, part_j, ratio, column);
    });
}

void launch_tab_rhs_ranging(const TableauView& tv, const DeferredUpdate& du, const double* b, const int32_t* basis_indices,
                            Tolerances tol, const int32_t* cols, int32_t count, int32_t p, double* part, double* ratio, int32_t* row,
                            hipStream_t s) {
    if (count < 1) return;
    const int nbr = cdiv(tv.m, kThreads);
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_rhs_ranging<decltype(B)::value, kTabRatioChunk>), dim3(cdiv(count, kTabRatioChunk), nbr), dim3(kThreads), 0,
                           s, tv, du, b, tol, cols, (int)count, (int)p, part);
        hipLaunchKernelGGL((k_tab_rhs_ranging_pick<decltype(B)::value>), dim3(count), dim3(kThreads), 0, s, tv, du, b, basis_indices, tol,
                           cols, (int)count, (int)p, nbr, part, ratio, row);
    });
}

void launch_tab_gomory(const TableauView& tv, const DeferredUpdate& du, const ColumnTable& ct, const uint8_t* in_basis, Tolerances tol,
                       const GomoryCuts& gc, int32_t p, hipStream_t s) {
    if (gc.count < 1 || tv.c_hi <= tv.c_lo || tv.m < 1) return;
    const int chunks = cdiv(gc.count, kTabRatioChunk);
    (void)hipMemsetAsync(gc.y, 0, sizeof(double) * (size_t)gc.count * (size_t)tv.m, s);
    with_load_batch(du.batch, [&](auto B) {
        hipLaunchKernelGGL((k_tab_gomory_rows<decltype(B)::value, kTabRatioChunk>), dim3(chunks, tab_scan_blocks(tv.c_hi - tv.c_lo)),
                           dim3(kThreads), 0, s, tv, du, ct, in_basis, tol.zero, gc, (int)p);
        if (gc.nr_normal > 0)
            hipLaunchKernelGGL((k_tab_gomory_structural<decltype(B)::value, kTabRatioChunk>), dim3(gc.nr_normal, chunks), dim3(kThreads), 0, s,
                               tv, ct, gc);
    });
}

void launch_tab_trial_copy(const TrialTable& t, hipStream_t s) {
    if (t.count < 1 || t.count > kTrialMaxSegments) return;
    const int64_t units = t.unit_end[t.count - 1];
    // one workgroup per 256 units up to the device's share (kTabTrialGrid); a table of tails alone still needs workgroup 0
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((units + kThreads - 1) / kThreads, kTabTrialGrid));
    hipLaunchKernelGGL(k_tab_trial_copy, dim3(grid), dim3(kThreads), 0, s, t);
}

// ------------------------------------------------------------------------------------------------
// The pools (relp_pool_*, relp_cutpool_*): sliced ELL, one item -- a pool column, or a cut -- per lane (PoolView).  An item's value
// (the reduced cost, or the slack) is one sequential fma chain, so the parallelism is across items, never inside one.
// ------------------------------------------------------------------------------------------------
// -pi as a vector of its own, once per launch sequence: vec[i] = d[idcol[i]] - cost_store[idcol[i]], one rounding, what
// relp_get_minus_pi forms on the host.  The chains then make two dependent loads per entry (row, vec[row]) instead of three
// (row, idcol[row], d and cost_store of it), and 8 m bytes that stay in cache instead of three scattered arrays.
__global__ void k_pool_minus_pi(MinusPi mp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < mp.m) { const int c = mp.idcol[i]; mp.vec[i] = mp.d[c] - mp.cost_store[c]; }
}

// Where item k of a pool lives: its entry e has its index at idx[e * kPoolSlice] and its value at val[e * kPoolSlice], e < width.
struct PoolLane {
    const int32_t* __restrict__ idx;
    const double* __restrict__ val;
    int64_t width;
    __device__ __forceinline__ PoolLane(const PoolView& pv, int k) {
        const int s = k / kPoolSlice;
        const int64_t base = pv.slice_ptr[s];
        width = (pv.slice_ptr[s + 1] - base) / kPoolSlice;
        idx = pv.idx + base + k % kPoolSlice;
        val = pv.val + base + k % kPoolSlice;
    }
};

// acc0 + sum vec[index] * value over the entries of a lane in stored order: one chain from acc0.  The loads do not depend on the
// chain, so they are issued kPoolBatch entries at a time before any is used, as in for_pending: indices and values first
// (consecutive lanes, consecutive addresses), then the gathers from vec; a thread makes two round trips per batch instead of two
// per entry.  A padded entry (index < 0) gathers and adds nothing, and with BOUNDED neither does an entry whose index is not below
// `bound`.  The order of the chain is the stored order whatever the batch is.
static constexpr int kPoolBatch = 16;
template <bool BOUNDED>
__device__ __forceinline__ double pool_chain(const PoolLane& ln, const double* __restrict__ vec, int bound, double acc0) {
    const auto live = [&](int i) { return i >= 0 && (!BOUNDED || i < bound); };
    double acc = acc0;
    int64_t e = 0;
    for (; e + kPoolBatch <= ln.width; e += kPoolBatch) {
        int i[kPoolBatch];
        double v[kPoolBatch], g[kPoolBatch];
#pragma unroll
        for (int t = 0; t < kPoolBatch; ++t) { i[t] = ln.idx[(e + t) * kPoolSlice]; v[t] = ln.val[(e + t) * kPoolSlice]; }
#pragma unroll
        for (int t = 0; t < kPoolBatch; ++t) g[t] = live(i[t]) ? vec[i[t]] : 0.0;
#pragma unroll
        for (int t = 0; t < kPoolBatch; ++t)
            if (live(i[t])) acc = fma(g[t], v[t], acc);
    }
    for (; e < ln.width; ++e) {
        const int i = ln.idx[e * kPoolSlice];
        if (live(i)) acc = fma(vec[i], ln.val[e * kPoolSlice], acc);
    }
    return acc;
}

// What a sweep asks of item k: its value and, from the value, the key its winners are ranked by; kAlwaysAll: the vector of every
// item's value is always written (the kernel then does not test the pointer).
// The reduced cost of a pool column: the chain from its cost over -pi; the key is the value.
struct ReducedCost {
    static constexpr bool kAlwaysAll = false;
    PoolView pv; const double* minus_pi;
    __device__ __forceinline__ double value(int k) const { return pool_chain<false>(PoolLane(pv, k), minus_pi, 0, pv.scalar[k]); }
    __device__ __forceinline__ double key(int, double d) const { return d; }
};
// The slack of a cut at the vertex x: its right-hand side minus the chain from 0.0 over x; the key is the slack or the efficacy.
struct Slack {
    static constexpr bool kAlwaysAll = true;
    PoolView pv; const double* norm; const double* x; int nr_normal, by_efficacy;
    __device__ __forceinline__ double value(int k) const {
        const double acc = pool_chain<true>(PoolLane(pv, k), x, nr_normal, 0.0);
        return pv.scalar[k] - acc;
    }
    __device__ __forceinline__ double key(int k, double sl) const {
        if (!by_efficacy) return sl;
        const double nk = norm[k];
        return sl / (nk == 0.0 ? 1.0 : nk);
    }
};

// Chunk blockIdx.x % chunks of segment blockIdx.x / chunks (relp_kernels.h: the sweep).  segments < 1: one share, no partials.
template <class Scorer>
__global__ __launch_bounds__(kThreads) void k_pool_sweep(Scorer sc, int seg_size, int chunks, double tol, double* all, double* part_d,
                                                         int32_t* part_k) {
    const int seg = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int64_t lo = (int64_t)seg * seg_size + (int64_t)chunk * kPoolChunk;
    const int hi = (int)min(min(lo + kPoolChunk, (int64_t)(seg + 1) * seg_size), (int64_t)sc.pv.count);
    double best = INFINITY;
    int best_k = INT32_MAX;
    for (int64_t k64 = lo + threadIdx.x; k64 < hi; k64 += kThreads) {
        const int k = (int)k64;
        const double v = sc.value(k);
        if (Scorer::kAlwaysAll || all) all[k] = v;
        const double key = sc.key(k, v);
        if (sc.pv.active[k] && v < -tol && key < best) { best = key; best_k = k; }     // (ascending k: the first of equal keys stays)
    }
    if (!part_d) return;
    block_min_key<kThreads>(best, best_k);
    if (threadIdx.x == 0) {
        part_d[blockIdx.x] = best_k == INT32_MAX ? INFINITY : best;
        part_k[blockIdx.x] = best_k == INT32_MAX ? -1 : best_k;
    }
}

// The exclusive prefix sum of one flag per thread over the workgroup's 256 threads, in thread order; *total = the sum.  Inside a
// wave by ballot and population count, across the four waves through LDS: two barriers, callable in a loop (the first barrier
// stands in front of the write: the previous call's words have been read).
__device__ __forceinline__ int block_flag_scan(int flag, int* s_scan, int* total) {
    const unsigned long long votes = __ballot(flag != 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int below = __popcll(votes & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_scan[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const int c = s_scan[w];
        before += w < wave ? c : 0;
        all += c;
    }
    *total = all;
    return before + below;
}

// The chunks of share blockIdx.x folded into its first slot: thread t takes the chunks t, t + 256, ... in ascending order, then the
// workgroup minimum in the same total order.  Every read of the share's partials precedes the barrier inside block_min_key, the
// one write follows it.  Launched only when a share has more than one chunk.
__global__ __launch_bounds__(kThreads) void k_pool_fold(int chunks, double* part_d, int32_t* part_k) {
    const int64_t first = (int64_t)blockIdx.x * chunks;
    double best = INFINITY;
    int best_k = INT32_MAX;
    for (int c = threadIdx.x; c < chunks; c += kThreads) {
        const double d = part_d[first + c];
        const int k = part_k[first + c];
        if (k >= 0 && (d < best || (d == best && k < best_k))) { best = d; best_k = k; }
    }
    block_min_key<kThreads>(best, best_k);
    if (threadIdx.x == 0) {
        part_d[first] = best_k == INT32_MAX ? INFINITY : best;
        part_k[first] = best_k == INT32_MAX ? -1 : best_k;
    }
}

// One workgroup: the winners of the shares (the first slot of each share's partials), compacted in ascending share order with their
// keys or, where `values` is given, with values[winner] (the cut pool: the slack, not the efficacy).
__global__ __launch_bounds__(kThreads) void k_pool_winners(int segments, int chunks, const double* __restrict__ part_d,
                                                           const int32_t* __restrict__ part_k, const double* __restrict__ values, int count,
                                                           int32_t* out_k, double* out, int32_t* found) {
    __shared__ int s_scan[kThreads / 64];
    int placed = 0;
    for (int base = 0; base < segments; base += kThreads) {
        const int seg = base + threadIdx.x;
        int best_k = seg < segments ? part_k[(int64_t)seg * chunks] : -1;
        if (best_k >= count) best_k = -1;
        int total;
        const int at = placed + block_flag_scan(best_k >= 0 ? 1 : 0, s_scan, &total);
        if (best_k >= 0) { out_k[at] = best_k; out[at] = values ? values[best_k] : part_d[(int64_t)seg * chunks]; }
        placed += total;
    }
    if (threadIdx.x == 0) *found = placed;
}

// The front of both entries kernels.  Entries 256 at a time: with C = ceil(longest / 256), workgroup b has the entries
// (b % C) * 256 + threadIdx.x of the chosen item x = b / C.  i: the entry's index, -1 where the thread has nothing to do (behind the
// item's slice width, padding, an index not below `bound`); v: where its value stands.
struct PoolEntry { int x, i; const double* v; };
__device__ __forceinline__ PoolEntry pool_entry(const PoolView& pv, const int32_t* __restrict__ ids, int longest, int bound) {
    const int per_item = (longest + kThreads - 1) / kThreads;
    const int x = blockIdx.x / per_item;
    const PoolLane ln(pv, ids[x]);
    const int64_t e = (int64_t)(blockIdx.x % per_item) * kThreads + threadIdx.x;
    if (e >= ln.width) return PoolEntry{x, -1, nullptr};
    const int i = ln.idx[e * kPoolSlice];
    return PoolEntry{x, i < bound ? i : -1, ln.val + e * kPoolSlice};
}

// One entry of a chosen column per thread (pool_entry; relp_kernels.h: launch_pool_add_operands).  SCATTER == false: the row is
// marked.  true: the value goes to its place in coef and in the column's row-space vector.
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void k_pool_entries(PoolView pv, PoolAdd pa) {
    const PoolEntry en = pool_entry(pv, pa.ids, pa.longest, pa.m);
    const int x = en.x, r = en.i;
    if (r < 0) return;
    if (!SCATTER) { pa.rank[r] = 1; return; }
    const double v = *en.v;
    if (pa.rank[r] < 0 || pa.rank[r] >= pa.entries) return;      // (a list longer than the caller sized coef for: reported through *entries_out)
    pa.coef[(int64_t)pa.rank[r] * pa.count + x] = v;
    pa.col_a[(int64_t)(pa.a0 + x) * pa.ld_c + r] = v;
}

// One workgroup: the marks become places, the marked rows' identity columns the union list, ascending.
__global__ __launch_bounds__(kThreads) void k_pool_union(PoolAdd pa, const int32_t* __restrict__ idcol) {
    __shared__ int s_scan[kThreads / 64];
    int placed = 0;
    for (int base = 0; base < pa.m; base += kThreads) {
        const int i = base + threadIdx.x;
        const int flag = i < pa.m && pa.rank[i] != 0 ? 1 : 0;
        int total;
        const int at = placed + block_flag_scan(flag, s_scan, &total);
        if (i < pa.m) pa.rank[i] = flag ? at : -1;
        if (flag && at < pa.entries) pa.cols[at] = idcol[i];
        placed += total;
    }
    if (threadIdx.x == 0) *pa.entries_out = placed;
}

// d, cost of the chosen column blockIdx.x; its activity flag cleared.  One chain, so one thread adds; but its operands do not depend
// on it, so the workgroup fetches them 256 entries at a time into LDS (row, value, -pi of the row: one entry per thread, three
// round trips per 256 entries instead of two per batch of one thread) and thread 0 chains them from there in stored order.
__global__ __launch_bounds__(kThreads) void k_pool_chosen(PoolView pv, MinusPi mp, PoolAdd pa) {
    __shared__ double s_p[kThreads], s_v[kThreads];
    __shared__ int s_r[kThreads];
    const int x = blockIdx.x, k = pa.ids[x];
    const PoolLane ln(pv, k);
    const int64_t width = ln.width;
    double acc = pv.scalar[k];
    for (int64_t e0 = 0; e0 < width; e0 += kThreads) {
        __syncthreads();                               // (thread 0 has read the previous 256)
        const int64_t e = e0 + threadIdx.x;
        int r = -1;
        double v = 0.0, p = 0.0;
        if (e < width) {
            r = ln.idx[e * kPoolSlice];
            if (r >= 0) { v = ln.val[e * kPoolSlice]; p = mp.vec[r]; }
        }
        s_r[threadIdx.x] = r; s_v[threadIdx.x] = v; s_p[threadIdx.x] = p;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = (int)min((int64_t)kThreads, width - e0);
#pragma unroll 8
            for (int j = 0; j < n; ++j) {              // (a select, not a branch: the LDS reads of the unrolled entries leave together)
                const double next = fma(s_p[j], s_v[j], acc);
                acc = s_r[j] >= 0 ? next : acc;
            }
        }
    }
    if (threadIdx.x == 0) {
        pa.d_new[x] = acc;
        pa.cost_new[x] = pv.scalar[k];
        pv.active[k] = 0;
    }
}

__global__ void k_pool_set_active(PoolView pv, const int32_t* __restrict__ ids, int count, int flag) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < count) pv.active[ids[x]] = (uint8_t)flag;
}

// The launches of a sweep behind its prologue (relp_kernels.h).  values: what the winners come back with in place of their keys.
template <class Scorer>
static void launch_pool_sweep(const Scorer& sc, int32_t segments, double tol, double* all, double* part_d, int32_t* part_k,
                              const double* values, int32_t* out_k, double* out, int32_t* found, hipStream_t s) {
    const int32_t count = sc.pv.count;
    if (segments < 1) {
        if (count > 0 && all)
            hipLaunchKernelGGL(k_pool_sweep<Scorer>, dim3(cdiv(count, kPoolChunk)), dim3(kThreads), 0, s, sc, (int)count, cdiv(count, kPoolChunk), tol,
                               all, (double*)nullptr, (int32_t*)nullptr);
        return;
    }
    const int chunks = pool_segment_chunks(count, segments);
    if (count > 0)
        hipLaunchKernelGGL(k_pool_sweep<Scorer>, dim3((unsigned)((int64_t)segments * chunks)), dim3(kThreads), 0, s, sc,
                           (int)pool_segment_size(count, segments), chunks, tol, all, part_d, part_k);
    if (count > 0 && chunks > 1) hipLaunchKernelGGL(k_pool_fold, dim3(segments), dim3(kThreads), 0, s, chunks, part_d, part_k);
    hipLaunchKernelGGL(k_pool_winners, dim3(1), dim3(kThreads), 0, s, count > 0 ? (int)segments : 0, chunks, part_d, part_k, values, (int)count,
                       out_k, out, found);
}

void launch_pool_price(const PoolView& pv, const MinusPi& mp, int32_t segments, double tol, double* d_all, double* part_d, int32_t* part_k,
                       int32_t* out_k, double* out_d, int32_t* found, hipStream_t s) {
    if (pv.count > 0 && mp.m > 0) hipLaunchKernelGGL(k_pool_minus_pi, dim3(cdiv(mp.m, 256)), dim3(256), 0, s, mp);
    launch_pool_sweep(ReducedCost{pv, mp.vec}, segments, tol, d_all, part_d, part_k, nullptr, out_k, out_d, found, s);
}

void launch_pool_add_operands(const PoolView& pv, const MinusPi& mp, const PoolAdd& pa, hipStream_t s) {
    if (pa.count < 1 || pa.m < 1) return;
    const dim3 grid((unsigned)((int64_t)cdiv(std::max(pa.longest, 1), kThreads) * pa.count));
    (void)hipMemsetAsync(pa.rank, 0, sizeof(int32_t) * (size_t)pa.m, s);
    if (pa.longest > 0) hipLaunchKernelGGL(k_pool_entries<false>, grid, dim3(kThreads), 0, s, pv, pa);
    hipLaunchKernelGGL(k_pool_union, dim3(1), dim3(kThreads), 0, s, pa, mp.idcol);
    hipLaunchKernelGGL(k_pool_minus_pi, dim3(cdiv(mp.m, 256)), dim3(256), 0, s, mp);
    if (pa.entries > 0) (void)hipMemsetAsync(pa.coef, 0, sizeof(double) * (size_t)pa.entries * (size_t)pa.count, s);
    (void)hipMemset2DAsync(pa.col_a + (int64_t)pa.a0 * pa.ld_c, sizeof(double) * (size_t)pa.ld_c, 0, sizeof(double) * (size_t)pa.m, (size_t)pa.count, s);
    if (pa.longest > 0) hipLaunchKernelGGL(k_pool_entries<true>, grid, dim3(kThreads), 0, s, pv, pa);
    hipLaunchKernelGGL(k_pool_chosen, dim3(pa.count), dim3(kThreads), 0, s, pv, mp, pa);
}

void launch_pool_set_active(const PoolView& pv, const int32_t* ids, int32_t count, int32_t flag, hipStream_t s) {
    if (count < 1) return;
    hipLaunchKernelGGL(k_pool_set_active, dim3(cdiv(count, 256)), dim3(256), 0, s, pv, ids, (int)count, (int)flag);
}

// ------------------------------------------------------------------------------------------------
// The cut pool's own (relp_cutpool_slacks, relp_cutpool_separate, relp_cutpool_add): the items are cuts, pv.idx holds structural
// columns, pv.scalar the right-hand sides (CutPoolView).  The sweep is k_pool_sweep<Slack> above.
// ------------------------------------------------------------------------------------------------
// The vertex over the structural columns, after x was cleared to +0.0: row r hands b[r] to its basic column where that is structural.
__global__ void k_cutpool_x(Vertex vx) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= vx.m) return;
    const int j = vx.basis[r];
    if (j >= 0 && j < vx.nr_normal) vx.x[j] = vx.b[r];
}

// One entry of a chosen cut per thread (pool_entry).  SCATTER == false: the column is marked.  true: the value goes to its place in
// the cut's row of A, and into coef where the column is in the union list.
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void k_cutpool_entries(PoolView pv, CutPoolAdd ca) {
    const PoolEntry en = pool_entry(pv, ca.ids, ca.longest, ca.nr_normal);
    const int x = en.x, j = en.i;
    if (j < 0) return;
    if (!SCATTER) { ca.mark[j] = 1; return; }
    const double v = *en.v;
    ca.A[(int64_t)j * ca.ld_a + ca.a_row0 + x] = v;
    const int place = ca.mark[j] - 2;
    if (place >= 0 && place < ca.room) ca.coef[(int64_t)place * ca.count + x] = v;
}

// One workgroup: row r joins the union list iff its basic column is structural and marked; the list ascends in r.
__global__ __launch_bounds__(kThreads) void k_cutpool_union(CutPoolAdd ca) {
    __shared__ int s_scan[kThreads / 64];
    int placed = 0;
    for (int base = 0; base < ca.m; base += kThreads) {
        const int r = base + threadIdx.x;
        int j = -1;
        if (r < ca.m) { j = ca.basis[r]; if (j < 0 || j >= ca.nr_normal || ca.mark[j] == 0) j = -1; }
        int total;
        const int at = placed + block_flag_scan(j >= 0 ? 1 : 0, s_scan, &total);
        if (j >= 0) {
            ca.mark[j] = 2 + at;                       // (basic in this row alone: the word's one writer)
            if (at < ca.room) ca.rows[at] = r;
        }
        placed += total;
    }
    if (threadIdx.x == 0) *ca.entries_out = placed;
}

// b of the new row of the chosen cut blockIdx.x; its activity flag cleared.  One chain over the whole union list, zeros included, so
// one thread adds; the workgroup fetches its operands 256 entries at a time into LDS (coef[e][x] and b[rows[e]]) and thread 0 chains
// them from there in ascending e, as k_pool_chosen does.
__global__ __launch_bounds__(kThreads) void k_cutpool_chosen(PoolView pv, CutPoolAdd ca) {
    __shared__ double s_g[kThreads], s_b[kThreads];
    const int x = blockIdx.x, k = ca.ids[x];
    const int entries = min(*ca.entries_out, ca.room);
    double acc = 0.0;
    for (int e0 = 0; e0 < entries; e0 += kThreads) {
        __syncthreads();                               // (thread 0 has read the previous 256)
        const int e = e0 + threadIdx.x;
        double g = 0.0, bv = 0.0;
        if (e < entries) { g = ca.coef[(int64_t)e * ca.count + x]; bv = ca.b[ca.rows[e]]; }
        s_g[threadIdx.x] = g; s_b[threadIdx.x] = bv;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = min((int)kThreads, entries - e0);
#pragma unroll 8
            for (int j = 0; j < n; ++j) acc = fma(s_g[j], s_b[j], acc);
        }
    }
    if (threadIdx.x == 0) {
        ca.b_new[x] = pv.scalar[k] - acc;
        pv.active[k] = 0;
    }
}

void launch_cutpool_x(const Vertex& vx, hipStream_t s) {
    if (vx.nr_normal > 0) (void)hipMemsetAsync(vx.x, 0, sizeof(double) * (size_t)vx.nr_normal, s);
    if (vx.m > 0 && vx.nr_normal > 0) hipLaunchKernelGGL(k_cutpool_x, dim3(cdiv(vx.m, 256)), dim3(256), 0, s, vx);
}

void launch_cutpool_separate(const CutPoolView& cv, const Vertex& vx, int32_t segments, double tol, int32_t by_efficacy, double* s_all,
                             double* part_d, int32_t* part_k, int32_t* out_k, double* out_s, int32_t* found, hipStream_t s) {
    if (cv.pv.count > 0) launch_cutpool_x(vx, s);
    launch_pool_sweep(Slack{cv.pv, cv.norm, vx.x, vx.nr_normal, (int)by_efficacy}, segments, tol, s_all, part_d, part_k, s_all, out_k, out_s,
                      found, s);
}

void launch_cutpool_add_operands(const CutPoolView& cv, const CutPoolAdd& ca, hipStream_t s) {
    if (ca.count < 1 || ca.nr_normal < 1) return;      // (an LP has structural columns: Layout)
    const dim3 grid((unsigned)((int64_t)cdiv(std::max(ca.longest, 1), kThreads) * ca.count));
    (void)hipMemsetAsync(ca.mark, 0, sizeof(int32_t) * (size_t)ca.nr_normal, s);
    if (ca.longest > 0) hipLaunchKernelGGL(k_cutpool_entries<false>, grid, dim3(kThreads), 0, s, cv.pv, ca);
    hipLaunchKernelGGL(k_cutpool_union, dim3(1), dim3(kThreads), 0, s, ca);
    if (ca.room > 0) (void)hipMemsetAsync(ca.coef, 0, sizeof(double) * (size_t)ca.room * (size_t)ca.count, s);
    (void)hipMemset2DAsync(ca.A + ca.a_row0, sizeof(double) * (size_t)ca.ld_a, 0, sizeof(double) * (size_t)ca.count, (size_t)ca.nr_normal, s);
    if (ca.longest > 0) hipLaunchKernelGGL(k_cutpool_entries<true>, grid, dim3(kThreads), 0, s, cv.pv, ca);
    hipLaunchKernelGGL(k_cutpool_chosen, dim3(ca.count), dim3(kThreads), 0, s, cv.pv, ca);
}

}  // namespace relp
