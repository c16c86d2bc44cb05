// relp_device_common.h -- device helpers shared by the three kernel files (constants, wavefront and
// workgroup reductions, and the steps of a pivot every engine's kernels share: the PRICE key and (key, column) minimum, the
// entering-column choice, the winner among shard candidates, the ratio test, the bookkeeping of a completed pivot).
// Included by relp_kernels_*.hip only.
#pragma once
#include <algorithm>
#include "relp_kernels.h"

#include <math.h>

namespace relp {

static constexpr int kThreads = 256;     // 4 wavefronts
static constexpr int kVecPerBlock = 8;   // vectors (columns of A / rows of B^-1) per workgroup
static constexpr int kSingleBlock = 1024;

// ------------------------------------------------------------------------------------------------
// Wavefront (64 lanes) and workgroup reductions
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Workgroup minimum (block_max_value: maximum) of one value per thread over BS threads, result in every thread.  One barrier;
// every thread finishes from the BS / 64 LDS words itself, in ascending order.  Exact, so the result does not depend on how the
// values are spread over the threads.  One set of LDS words per (BS, type, min or max): a kernel that makes the same call twice
// puts a barrier between the calls.
struct MinOp {
    __device__ double operator()(double a, double b) const { return fmin(a, b); }
    __device__ int operator()(int a, int b) const { return min(a, b); }
};
struct MaxOp {
    __device__ double operator()(double a, double b) const { return fmax(a, b); }
};
template <int BS, class T, class Op>
__device__ __forceinline__ T block_reduce_value(T v, Op op) {
    __shared__ T s_v[BS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, 64));
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
    __syncthreads();
    v = s_v[0];
#pragma unroll
    for (int w = 1; w < BS / 64; ++w) v = op(v, s_v[w]);
    return v;
}
template <int BS, class T>
__device__ __forceinline__ T block_min_value(T v) { return block_reduce_value<BS>(v, MinOp{}); }
template <int BS>
__device__ __forceinline__ double block_max_value(double v) { return block_reduce_value<BS>(v, MaxOp{}); }

// Dot products of kVecPerBlock contiguous vectors (stride ld) with one shared vector x.
// Thread t streams 16-byte pairs k = 2t, 2t + 512, ...; all 8 loads of one step are independent.
// Vectors beyond `v_hi` are clamped (duplicate loads, results discarded) so there is no branch in
// the stream.  result[v] is valid for threads < kVecPerBlock after the call.
__device__ __forceinline__ void block_multi_dot(const double* __restrict__ M, int64_t ld, int len,
                                                int v0, int v_hi, const double* __restrict__ x,
                                                double* s_partial /* [4][kVecPerBlock] */,
                                                double& result) {
    const int t = threadIdx.x;
    double acc[kVecPerBlock];
    const double* base[kVecPerBlock];
#pragma unroll
    for (int v = 0; v < kVecPerBlock; ++v) {
        acc[v] = 0.0;
        int vi = v0 + v;
        if (vi >= v_hi) vi = v_hi - 1;
        base[v] = M + (int64_t)vi * ld;
    }
    const int len2 = len & ~1;
    for (int k = 2 * t; k < len2; k += 2 * kThreads) {
        const double2 xv = *reinterpret_cast<const double2*>(x + k);
#pragma unroll
        for (int v = 0; v < kVecPerBlock; ++v) {
            const double2 a = *reinterpret_cast<const double2*>(base[v] + k);
            acc[v] = fma(a.x, xv.x, acc[v]);
            acc[v] = fma(a.y, xv.y, acc[v]);
        }
    }
    if ((len & 1) && t == 0) {
        const double xl = x[len - 1];
#pragma unroll
        for (int v = 0; v < kVecPerBlock; ++v) acc[v] = fma(base[v][len - 1], xl, acc[v]);
    }
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int v = 0; v < kVecPerBlock; ++v) {
        const double w = wave_sum(acc[v]);
        if (lane == 0) s_partial[wave * kVecPerBlock + v] = w;
    }
    __syncthreads();
    if (t < kVecPerBlock) {
        result = (s_partial[0 * kVecPerBlock + t] + s_partial[1 * kVecPerBlock + t]) +
                 (s_partial[2 * kVecPerBlock + t] + s_partial[3 * kVecPerBlock + t]);
    }
}

// Selection key of a candidate column (smaller wins, ties by smaller j):
//   SteepestDescent: d_j (pivot_rule.rs:118); FirstProfitable[WithMemory]: position in the search order (:88)
__device__ __forceinline__ double select_key(int rule, int n, const PivotRecord* rec, int j, double d_j) {
    if (rule == 2) return d_j;
    const int last = (rule == 1 && rec) ? rec->last_selected : -1;
    if (last >= 0) return (double)(j >= last ? j - last : j - last + n);
    return (double)j;
}

// ------------------------------------------------------------------------------------------------
// PRICE
// Workgroup minimum of (key, column) over BS threads, result in every thread: smaller key wins, ties go to the lower column.
// One barrier; every thread finishes from the BS / 64 LDS words itself.  The order is total, so the result does not depend
// on how the candidates are spread over the threads.  A kernel that calls it twice puts a barrier between the calls.
template <int BS>
__device__ __forceinline__ void block_min_key(double& key, int& kj) {
    __shared__ double s_k[BS / 64];
    __shared__ int s_j[BS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ok = __shfl_down(key, off, 64);
        const int oj = __shfl_down(kj, off, 64);
        if (ok < key || (ok == key && oj < kj)) { key = ok; kj = oj; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_k[wave] = key; s_j[wave] = kj; }
    __syncthreads();
    key = s_k[0]; kj = s_j[0];
#pragma unroll
    for (int w = 1; w < BS / 64; ++w)
        if (s_k[w] < key || (s_k[w] == key && s_j[w] < kj)) { key = s_k[w]; kj = s_j[w]; }
}

// Workgroup-level (key, j) minimum of one candidate per thread -> partial slot `slot`.
__device__ __forceinline__ void block_partial_min(double key, int kj, SelectPartials sp, int slot) {
    block_min_key<kThreads>(key, kj);
    if (threadIdx.x == 0) { sp.k1[slot] = key; sp.j[slot] = kj; }
}

// PRICE of 256 virtual columns (artificial, slack, bound slack; no matrix data: d_j = cost + (+-)(-pi)_row) and their
// partial argmin; `block` = index of the workgroup among the virtual-column workgroups.
__device__ __forceinline__ void price_virtual_body(const ColumnTable& ct, const double* __restrict__ minus_pi,
                                                   double* __restrict__ d, int cost_mode, const SelectPartials& sp,
                                                   const PivotRecord* rec, int block) {
    const int t = block * kThreads + threadIdx.x;
    int j = -1;
    double val = 0.0;
    if (t < ct.nr_artificial) {
        j = t;
        val = (cost_mode == 1 ? 1.0 : 0.0) + minus_pi[ct.column_to_row[t]];   // Cost::One + (-pi)_row
    } else {
        const int v = t - ct.nr_artificial;
        if (v < ct.nr_virtual) {
            // a slack whose row was removed as redundant (RemoveRows) is an empty column: vrow0 = -1
            const int r0 = ct.vrow0[v];
            double s = r0 >= 0 ? (double)ct.vsign[v] * minus_pi[r0] : 0.0;
            const int r1 = ct.vrow1[v];
            if (r1 >= 0) s += minus_pi[r1];
            j = ct.nr_artificial + ct.nr_normal + v;              // slack cost is None (zero)
            val = s;
        }
    }
    if (j >= 0) d[j] = val;
    if (!sp.k1) return;
    double key = INFINITY;
    int kj = 0x7fffffff;
    if (j >= 0 && !sp.in_basis[j] && val < -sp.tol_cost) { key = select_key(sp.rule, sp.n, rec, j, val); kj = j; }
    block_partial_min(key, kj, sp, sp.offset + block);
}

// The slots t < count whose own minimum is inside a tie band (minima[t] <= bound), listed in s_list by a workgroup of BS threads;
// returns their number in every thread (one barrier).  More than kListMax: the list is incomplete and the caller walks all
// slots instead.  One thread of the caller sets s_cnt = 0 ahead of a barrier the caller already has.
template <int BS, int kListMax>
__device__ __forceinline__ int band_slots(const double* minima, int count, double bound, int* s_list, int& s_cnt) {
    for (int t = threadIdx.x; t < count; t += BS) {
        if (!(minima[t] <= bound)) continue;
        const int pos = atomicAdd(&s_cnt, 1);
        if (pos < kListMax) s_list[pos] = t;
    }
    __syncthreads();
    return s_cnt;
}

// Entering column of the tableau engine from the `count` partials of a PRICE (slot t = the kThreads storage columns from
// tv.c_lo + t * kThreads), by a workgroup of BS threads.  On entry (k1, bj) is the thread's first partial -- slot threadIdx.x,
// (+inf, 0x7fffffff) past the end -- when the caller loaded it together with whatever else it has to wait for (have_first),
// (+inf, 0x7fffffff) otherwise; on return every thread holds the winner's key and column, bj = 0x7fffffff when there is none.
// Ties (band_on): the lowest index among the columns inside the band k1 + tol_tie * max(1, |k1|), in_band(c, j, bound) = storage
// column c (index j) is a candidate inside it.  Only a slot whose own minimum is inside the band can hold such a column: those
// slots (normally one or two) are listed first, then re-read one column per thread, so the scan does not walk all `count`
// slots one dependent load after the other.
template <int BS, class InBand>
__device__ __forceinline__ void select_entering(const TableauView& tv, const SelectPartials& sp, int count, double tol_tie,
                                                bool band_on, bool have_first, double& k1, int& bj, InBand&& in_band) {
    constexpr int kListMax = 32, kGroups = BS / kThreads;
    __shared__ int s_list[kListMax];
    __shared__ int s_cnt;
    for (int t = threadIdx.x + (have_first ? BS : 0); t < count; t += BS) {
        const double key = sp.k1[t];
        const int j = sp.j[t];
        if (key < k1 || (key == k1 && j < bj)) { k1 = key; bj = j; }
    }
    if (threadIdx.x == 0) s_cnt = 0;                   // (visible after the barrier of the reduction)
    block_min_key<BS>(k1, bj);
    if (bj == 0x7fffffff || !band_on) return;
    const double bound = k1 + tol_tie * fmax(1.0, fabs(k1));
    const int listed = band_slots<BS, kListMax>(sp.k1, count, bound, s_list, s_cnt);
    // kGroups groups of kThreads threads, each on every kGroups-th slot
    const int grp = threadIdx.x / kThreads, u = threadIdx.x % kThreads;
    int lowest = 0x7fffffff;
    auto scan_slot = [&](int t) {
        const int c = tv.c_lo + t * kThreads + u;
        const int j = c - tv.col_off;
        if (c < tv.c_hi && j >= 0 && j < tv.n && in_band(c, j, bound) && j < lowest) lowest = j;
    };
    if (listed <= kListMax) {
        for (int i = grp; i < listed; i += kGroups) scan_slot(s_list[i]);
    } else {
        for (int t = grp; t < count; t += kGroups)
            if (sp.k1[t] <= bound) scan_slot(t);
    }
    bj = block_min_value<BS>(lowest);                  // the minimum itself is inside the band: there is one
}

// The primal pick: Dantzig ties (pivot_rule.rs:118), the lowest index with d_j <= k1 + tol_tie * max(1, |k1|).  (k1, bj) = the
// thread's first partial, loaded by the caller.
template <int BS>
__device__ __forceinline__ void tab_select_entering(const TableauView& tv, const SelectPartials& sp, int count, double& k1,
                                                    int& bj) {
    select_entering<BS>(tv, sp, count, sp.tol_tie, sp.rule == 2 && sp.tol_tie > 0.0, true, k1, bj, [&](int c, int j, double bound) {
        const double v = tv.d[c];
        const bool basic = sp.in_basis[j];             // with d: one round trip, not two (no short circuit between the loads)
        return !basic & (v < -sp.tol_cost && v <= bound);
    });
}

// Sharded PRICE: the winner among `count` gathered candidates, candidate g with key key[g * stride] (+inf = the rank has
// none) and column idx[g * stride] -- the heads of the messages themselves or a copy of them in LDS.  Smallest key, ties to
// the lower column; Dantzig ties across ranks: every rank sent (its minimum, its lowest index within the band of that
// minimum), and the lowest index among the ranks inside the global band wins.  Returns the rank, -1 when no rank has a
// candidate.  Serial: for ONE thread, which hands the answer to the others.
__device__ __forceinline__ int candidate_winner(const double* key, const double* idx, int64_t stride, int count, int rule,
                                                double tol_tie) {
    int win = -1; double k1 = INFINITY; double kj = 0.0;
    for (int g = 0; g < count; ++g) {
        const double a = key[g * stride], j = idx[g * stride];
        if (a < k1 || (a == k1 && win >= 0 && j < kj)) { k1 = a; kj = j; win = g; }
    }
    if (win >= 0 && rule == 2 && tol_tie > 0.0) {
        const double bound = k1 + tol_tie * fmax(1.0, fabs(k1));
        for (int g = 0; g < count; ++g)
            if (key[g * stride] <= bound && idx[g * stride] < kj) { kj = idx[g * stride]; win = g; }
    }
    return win;
}

// The same for a whole workgroup (of blockDim.x threads) with the heads [key, j, d_j] of the messages staged in LDS, so that
// they arrive in one round trip: the winner's rank in every thread, with its column and reduced cost.
static constexpr int kMaxRanks = 64;
__device__ __forceinline__ int candidate_winner_staged(const double* __restrict__ msgs, int count, int64_t msg_len, int rule,
                                                       double tol_tie, int* q, double* d_q) {
    __shared__ double s_key[kMaxRanks], s_idx[kMaxRanks], s_dq[kMaxRanks];
    __shared__ int s_win;
    for (int g = threadIdx.x; g < count && g < kMaxRanks; g += blockDim.x) {
        s_key[g] = msgs[g * msg_len + 0]; s_idx[g] = msgs[g * msg_len + 1]; s_dq[g] = msgs[g * msg_len + 2];
    }
    __syncthreads();
    if (threadIdx.x == 0) s_win = candidate_winner(s_key, s_idx, 1, count, rule, tol_tie);
    __syncthreads();
    const int win = s_win;
    if (win >= 0) { *q = (int)s_idx[win]; *d_q = s_dq[win]; }
    return win;
}

// What the sharded PRICE leaves in the record, by one thread: the entering column, or the end of the loop (win < 0)
__device__ __forceinline__ void record_candidate(PivotRecord* rec, int rule, int win, int q, double d_q) {
    if (win < 0) {
        rec->outcome = DEV_NO_CANDIDATE;
        if (rule == 1) rec->last_selected = -1;
    } else {
        rec->q = q;
        rec->d_q = d_q;
        if (rule == 1) rec->last_selected = q;
    }
}

// ------------------------------------------------------------------------------------------------
// UPDATE: what every engine does to b and to the scalars of a completed pivot (carry/mod.rs:283-333, tableau/mod.rs:72-84)
// ------------------------------------------------------------------------------------------------
// b_i after the pivot, br = b_r / alpha_r: row r gets br, a row with alpha_i = 0 keeps its bits
__device__ __forceinline__ double pivot_b(double a, double b_i, double br, bool is_r) {
    return is_r ? br : (a != 0.0 ? fma(-a, br, b_i) : b_i);
}

// -obj, the basis flags, the trace row, the degenerate and the iteration counter, by ONE thread.  The pivot comes by value, so
// from the record and from a register snapshot of it alike; basis_indices[r] = q stays with the caller (the fused launch writes
// it to its output copy of the array).
__device__ __forceinline__ void pivot_bookkeeping(int phase, long long iterations, double minus_objective, double d_q, double br,
                                                  int q, int r, int leaving, uint8_t* in_basis, int32_t* trace, int64_t trace_cap,
                                                  PivotRecord* rec) {
    rec->minus_objective = fma(-d_q, br, minus_objective);
    if (leaving < kWrappedArtificialBase) in_basis[leaving] = 0;   // a wrapped artificial has no flag
    in_basis[q] = 1;
    if (trace && iterations < trace_cap) {
        trace[0 * trace_cap + iterations] = phase;
        trace[1 * trace_cap + iterations] = q;
        trace[2 * trace_cap + iterations] = r;
        trace[3 * trace_cap + iterations] = leaving;
    }
    if (br == 0.0) rec->degenerate += 1;               // ratio 0: the basis changes, the vertex does not
    rec->iterations = iterations + 1;
}

static constexpr int kMaxEta = 128;

// ------------------------------------------------------------------------------------------------
// RATIO TEST (single workgroup; two passes: strict minimum, then Bland tie-break on the leaving
// column among rows within the tie band -- identical to tableau/mod.rs:221-247 for zero tolerances)
// ------------------------------------------------------------------------------------------------
// Tie-break key of a row inside the tie band (smaller wins).  ratio_rule 0 = the reference: the leaving column
// (tableau/mod.rs:229-239).  ratio_rule 1 (an f64 safeguard, relp_engine.h: RELP_RATIO_LARGEST_PIVOT): the pivot element's
// size first -- at float precision, larger = smaller key -- then the leaving column.  Order-independent either way.
typedef unsigned long long tie_key_t;
static constexpr tie_key_t kNoTieKey = ~0ull;
__device__ __forceinline__ tie_key_t tie_key(double a, int leave, int ratio_rule) {
    const unsigned size = ratio_rule ? 0x7fffffffu - __float_as_uint((float)a) : 0u;      // (a > tol.pivot > 0)
    return ((tie_key_t)size << 32) | (unsigned)leave;
}
__device__ __forceinline__ int tie_key_leaving(tie_key_t k) { return (int)(unsigned)(k & 0xffffffffull); }

// Workgroup minimum of (key, row) over BS threads, result in every thread; s_k / s_r: BS / 64 words of LDS each.  `wide`
// (uniform) = the keys use their upper half; otherwise the reduction runs on the 32-bit leaving columns as it always did.
template <int BS>
__device__ __forceinline__ void tie_reduce(tie_key_t& key, int& row, tie_key_t* s_k, int* s_r, bool wide) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wide) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const tie_key_t ok = __shfl_down(key, off, 64);
            const int orow = __shfl_down(row, off, 64);
            if (ok < key) { key = ok; row = orow; }
        }
    } else {
        int lv = (int)(unsigned)key;                   // (kNoTieKey -> -1: mapped to INT_MAX below)
        if (key == kNoTieKey) lv = 0x7fffffff;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int ol = __shfl_down(lv, off, 64);
            const int orow = __shfl_down(row, off, 64);
            if (ol < lv) { lv = ol; row = orow; }
        }
        key = (unsigned)lv;
    }
    if (lane == 0) { s_k[wave] = key; s_r[wave] = row; }
    __syncthreads();
    // every thread finishes the reduction itself (BS / 64 LDS words): no second barrier
    key = s_k[0]; row = s_r[0];
#pragma unroll
    for (int w = 1; w < BS / 64; ++w)
        if (s_k[w] < key) { key = s_k[w]; row = s_r[w]; }
}

// Last step of the ratio test, once the workgroup agrees on the pivot row r and its leaving column (tie_reduce: Bland on the
// leaving column among the rows inside the tie band, tableau/mod.rs:229-239): the pivot guard, then the record is written and
// the block bookkeeping of the deferred update (row r of W saved, slot of W chosen) is done.
// (everything this reads from memory -- alpha_r, b_r, row r of W, the slot of row r -- goes out in ONE round trip)
template <int BS>
__device__ __forceinline__ void ratio_commit_row(int r, int leaving, const double* alpha, const double* b, const DeferredUpdate& du,
                                                 int p, PivotRecord* rec, int guard_m = 0, double guard_rel = 0.0) {
    if (guard_m > 0) {
        // Tolerances::pivot_guard: the chosen element against the largest |entry| of the column (one pass of the workgroup
        // over alpha; nothing has been written yet)
        double mx = 0.0;
        for (int i = threadIdx.x; i < guard_m; i += BS) mx = fmax(mx, fabs(alpha[i]));
        if (alpha[r] < guard_rel * block_max_value<BS>(mx)) {
            if (threadIdx.x == 0) rec->outcome = DEV_NO_ROW;
            return;
        }
    }
    const bool deferred = du.kmax > 0;
    double a_r = 0.0, b_r = 0.0;
    int jt = 0;
    if (threadIdx.x == 0) {
        a_r = alpha[r];
        b_r = b[r];
        if (deferred) jt = du.pos_of_row[r];
    }
    // deferred update bookkeeping (k_eta_prepare): save row r of W, choose the column that receives u
    if (deferred)
        for (int j = threadIdx.x; j < p; j += BS) du.wr[j] = du.W[(int64_t)j * du.ld + r];
    if (threadIdx.x == 0) {
        rec->r = r;
        rec->leaving = leaving;
        rec->alpha_r = a_r;
        rec->b_r = b_r;
        if (deferred) {
            rec->n_eta_old = p;
            if (jt < 0) { jt = p; du.S[p] = r; du.pos_of_row[r] = p; rec->n_eta = p + 1; }
            rec->eta_target = jt;
        }
    }
}

// Body of the ratio test for a workgroup of BS threads that keeps up to ITEMS rows per thread in
// registers.  `p` = rec->n_eta read by the caller together with the outcome.  Ends with the block
// bookkeeping of the deferred update.
template <int BS, int ITEMS>
__device__ __forceinline__ void ratio_body(const double* alpha, const double* b, const int32_t* basis_indices, int m,
                                           const Tolerances& tol, const DeferredUpdate& du, int p, PivotRecord* rec) {
    // Each thread keeps its rows' ratios and leaving columns in registers (all loads issued at once, one
    // memory round trip); both passes then run out of registers.  m > 16 * 1024 falls back to re-reading.
    constexpr int kItems = ITEMS;
    const bool cached = m <= kItems * BS;
    double ratio_r[kItems], alpha_r[kItems];
    int leave_r[kItems];
    double mn = INFINITY;
    if (cached) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int i = threadIdx.x + k * BS;
            const bool in = i < m;
            const double a = in ? alpha[i] : 0.0;
            double bi = in ? b[i] : 0.0;
            leave_r[k] = in ? basis_indices[i] : 0x7fffffff;
            alpha_r[k] = a;
            if (bi <= tol.zero) bi = 0.0;   // also clamps a b_i that rounding pushed below 0: no negative step
            ratio_r[k] = (in && a > tol.pivot) ? bi / a : INFINITY;
            mn = fmin(mn, ratio_r[k]);
        }
    } else {
#pragma unroll 4
        for (int i = threadIdx.x; i < m; i += BS) {
            const double a = alpha[i];
            double bi = b[i];
            if (bi <= tol.zero) bi = 0.0;   // also clamps a b_i that rounding pushed below 0: no negative step
            const double ratio = (a > tol.pivot) ? bi / a : INFINITY;
            mn = fmin(mn, ratio);
        }
    }
    const double gmin = block_min_value<BS>(mn);
    if (gmin == INFINITY) {
        if (threadIdx.x == 0) rec->outcome = DEV_NO_ROW;
        return;
    }
    const double bound = gmin + tol.tie * fmax(1.0, fabs(gmin));
    tie_key_t best_key = kNoTieKey;
    int best_row = -1;
    if (cached) {
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            // ratio_r is +inf for rows that do not take part, so `<= bound` excludes them
            if (ratio_r[k] <= bound) {
                const tie_key_t key = tie_key(alpha_r[k], leave_r[k], tol.ratio_rule);
                if (key < best_key) { best_key = key; best_row = threadIdx.x + k * BS; }
            }
        }
    } else {
#pragma unroll 4
        for (int i = threadIdx.x; i < m; i += BS) {
            const double a = alpha[i];
            double bi = b[i];
            const int lv = basis_indices[i];
            if (bi <= tol.zero) bi = 0.0;   // also clamps a b_i that rounding pushed below 0: no negative step
            if (a > tol.pivot && bi / a <= bound) {
                const tie_key_t key = tie_key(a, lv, tol.ratio_rule);
                if (key < best_key) { best_key = key; best_row = i; }
            }
        }
    }
    __shared__ tie_key_t s_cl[BS / 64];
    __shared__ int s_cr[BS / 64];
    tie_reduce<BS>(best_key, best_row, s_cl, s_cr, tol.ratio_rule != 0);
    ratio_commit_row<BS>(best_row, tie_key_leaving(best_key), alpha, b, du, p, rec, tol.pivot_guard ? m : 0, tol.guard_rel);
}

// b_i / alpha_i as the ratio test's first pass forms it (ratio_body), +inf when the row does not qualify
__device__ __forceinline__ double row_ratio(double a, double bi, const Tolerances& tol) {
    if (bi <= tol.zero) bi = 0.0;   // also clamps a b_i that rounding pushed below 0: no negative step
    return a > tol.pivot ? bi / a : INFINITY;
}

// The pivot row from the minimum of every block of `rpb` rows (`minima`, nblk entries, written by the kernel that walked the
// rows), by a workgroup of BS threads: the global minimum is the minimum of the block minima, and a row inside the tie band
// lives in a block whose own minimum is inside the band, so only those blocks' rows (usually one or two blocks) are read
// again.  key_of_row(i, bound) = the tie-break key of row i (tie_key), kNoTieKey when the row does not qualify or lies outside
// the band; the smallest key wins (tie_reduce, `wide` = the keys use their upper half).  Every thread of the workgroup returns
// with (row, leaving column), row = -1 when no row qualifies; nothing is written.
// `first` = minima[threadIdx.x] when the caller loaded it together with the record (have_first)
template <int BS, class KeyOfRow>
__device__ __forceinline__ void block_minima_pick(const double* minima, int nblk, int rpb, int m, double tol_tie, double first,
                                                  bool have_first, bool wide, int* row_out, int* leave_out, KeyOfRow&& key_of_row) {
    constexpr int kListMax = 64;
    __shared__ int s_list[kListMax];
    __shared__ int s_cnt;
    __shared__ tie_key_t s_cl[BS / 64];
    __shared__ int s_cr[BS / 64];
    double mn = have_first ? first : INFINITY;
    for (int t = threadIdx.x + (have_first ? BS : 0); t < nblk; t += BS) mn = fmin(mn, minima[t]);
    if (threadIdx.x == 0) s_cnt = 0;                   // (visible after the barrier of the reduction)
    const double gmin = block_min_value<BS>(mn);
    if (gmin == INFINITY) { *row_out = -1; *leave_out = 0x7fffffff; return; }
    const double bound = gmin + tol_tie * fmax(1.0, fabs(gmin));
    const int listed = band_slots<BS, kListMax>(minima, nblk, bound, s_list, s_cnt);
    const bool use_list = listed <= kListMax;
    const int total = (use_list ? listed : nblk) * rpb;
    tie_key_t best_key = kNoTieKey;
    int best_row = -1;
    for (int idx = threadIdx.x; idx < total; idx += BS) {
        const int t = use_list ? s_list[idx / rpb] : idx / rpb;
        const int i = t * rpb + idx % rpb;
        if (i >= m) continue;
        const tie_key_t key = key_of_row(i, bound);
        if (key < best_key) { best_key = key; best_row = i; }
    }
    tie_reduce<BS>(best_key, best_row, s_cl, s_cr, wide);
    *row_out = best_row; *leave_out = tie_key_leaving(best_key);
}

// Ratio test from the minimum ratio of every block of `rpb` rows (`rmin`, written by the kernel that formed alpha).  Same choice
// as ratio_body.
template <int BS>
__device__ __forceinline__ void ratio_blocks_pick(const double* alpha, const double* b, const int32_t* basis_indices, int m,
                                                  const Tolerances& tol, const double* rmin, int nblk, int* row_out, int* leave_out,
                                                  double first = INFINITY, bool have_first = false, int rpb = kThreads) {
    block_minima_pick<BS>(rmin, nblk, rpb, m, tol.tie, first, have_first, tol.ratio_rule != 0, row_out, leave_out,
                          [&](int i, double bound) {
        const double a = alpha[i];
        double bi = b[i];
        int lv = basis_indices[i];                     // with alpha and b: one round trip, not two
        asm volatile("" : "+v"(lv));
        if (bi <= tol.zero) bi = 0.0;   // also clamps a b_i that rounding pushed below 0: no negative step
        return (a > tol.pivot && bi / a <= bound) ? tie_key(a, lv, tol.ratio_rule) : kNoTieKey;
    });
}

// The same as one whole step of a single-workgroup launch: the choice, then "no row" or the record and the block bookkeeping.
// `p` = rec->n_eta read by the caller.
template <int BS>
__device__ __forceinline__ void ratio_blocks_body(const double* alpha, const double* b, const int32_t* basis_indices, int m,
                                                  const Tolerances& tol, const DeferredUpdate& du, const double* rmin, int nblk,
                                                  int p, PivotRecord* rec, double first = INFINITY, bool have_first = false,
                                                  int rpb = kThreads) {
    int r, leaving;
    ratio_blocks_pick<BS>(alpha, b, basis_indices, m, tol, rmin, nblk, &r, &leaving, first, have_first, rpb);
    if (r < 0) {
        if (threadIdx.x == 0) rec->outcome = DEV_NO_ROW;
        return;
    }
    ratio_commit_row<BS>(r, leaving, alpha, b, du, p, rec, tol.pivot_guard ? m : 0, tol.guard_rel);
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// Blocks of 256 threads for a grid-stride loop over `total` elements.  (A HIP launch takes at most 2^32 - 1 threads: a tableau
// of 64,000 x 256,000 has four times as many elements, and a launch beyond the limit fails without running.)
static inline int element_blocks(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, int64_t(1) << 22); }

}  // namespace relp
