// relp_kernels.h -- device-side state and kernel launchers of the explicit-inverse pivot engine.
//
// Layout in HBM (all f64 unless noted):
//   A        dense column-major  nr_constraints x nr_normal (ld_a even, column j contiguous)
//   Binv     dense row-major     m x m (ld_b multiple of 16, row i contiguous) = `BasisInverseRows`
//   minus_pi, b, alpha, aq, rho  dense m-vectors (`Carry`, carry/mod.rs:45-65)
//   d        reduced costs, one per tableau column
//   basis_indices (i32, m), in_basis (u8, n_tableau), virtual-column descriptors (i32)
//   PivotRecord: the per-pivot scalars every kernel reads instead of the host (no sync in the loop)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "relp_layout.hpp"   // kWrappedArtificialBase
#include "relp_pool.hpp"     // kPoolSlice, kPoolChunk, pool_segment_size
#include "relp_trial.hpp"    // TrialTable

namespace relp {

enum DeviceOutcome : int32_t { DEV_RUNNING = 0, DEV_NO_CANDIDATE = 1, DEV_NO_ROW = 2 };

struct PivotRecord {
    int32_t outcome;        // DeviceOutcome; once != RUNNING every loop kernel is a no-op
    int32_t q;              // entering column (tableau index)
    double  d_q;            // its reduced cost
    int32_t r;              // pivot row
    int32_t leaving;        // basis_indices[r] before the update
    double  alpha_r;        // pivot element
    double  b_r;            // b[r] before the update
    double  minus_objective;
    long long iterations;   // basis changes so far (all phases)
    int32_t last_selected;  // FirstProfitableWithMemory state, -1 = None (pivot_rule.rs:62-64)
    int32_t phase;          // 1 or 2
    int32_t owner_has_row;  // sharded: 1 iff this rank owns row r
    int32_t pad_;
    double  key1;           // selection key of q (d_q, or its position in the search order)
    int32_t n_eta;          // deferred update: columns of W in use (distinct pivot rows since the last flush)
    int32_t eta_target;     // deferred update: column of W that receives this pivot's u
    int32_t n_eta_old;      // deferred update: n_eta before this pivot
    int32_t degenerate;     // pivots so far whose ratio b_r / alpha_r was exactly 0 (reported for config C5)
    int32_t p_now;          // n_eta as the column kernel of this pivot saw it (the fused ratio + update launch reads this copy:
                            // its first workgroup rewrites n_eta while later ones may not have started)
    int32_t pad2_;
};

// Deferred (blocked) update of the explicit inverse:  B^-1 = (I + W S') B0inv, where B0inv is the
// dense inverse at the last flush, S = [e_s1 .. e_sp] selects the distinct pivot rows since then and
// W (m x p, column-major) accumulates the elementary matrices E_k = I + u_k e_rk'.  A flush folds the
// p pivots into B0inv with one m x p x m GEMM (B0inv += W (S' B0inv)), so the 16 m^2 bytes of
// basis_inverse_rows.rs:63-83 are paid once per K pivots instead of once per pivot.
struct DeferredUpdate {
    double*  W;             // m x kmax, column j contiguous with pitch ld
    int64_t  ld;
    int32_t  kmax;
    int32_t* S;             // column j of W belongs to pivot row S[j]            (kmax)
    int32_t* pos_of_row;    // row -> column of W, or -1                          (m)
    double*  wr;            // row r of W before this pivot's update              (kmax)
    double*  R;             // flush snapshot S' B0inv, kmax x ld (row j contiguous)
    int32_t  batch;         // tableau kernels: pending rows loaded per round trip (tab_load_batch; 0 = the default)
    int32_t  w_split;       // tableau fused update: workgroups per 256 rows of W <- E W, at most (0 or 1 = one)
    int32_t  col_rows = 0;  // tableau column kernel with block minima: rows per workgroup and per minimum, 128 or 64 (else 256)
};

// Read-only description of the tableau's columns (Kind + MatrixData, partially.rs:72-80,
// matrix_data.rs:308-348).  Tableau column j: j < nr_artificial -> artificial unit column,
// else provider column p = j - nr_artificial; p < nr_normal structural, else virtual.
struct ColumnTable {
    int32_t nr_artificial;
    int32_t nr_normal;
    int32_t nr_virtual;           // provider columns that are slack / bound slack
    int32_t nr_constraints;       // rows of A
    const int32_t* column_to_row; // artificial k -> row                      (nr_artificial)
    const int32_t* bound_row;     // structural p -> bound row or -1          (nr_normal)
    const int32_t* vrow0;         // virtual v -> first row                   (nr_virtual)
    const int32_t* vrow1;         // virtual v -> second row or -1 (range slack)
    const int32_t* vsign;         // virtual v -> +1 / -1 on vrow0
    const double*  cost;          // structural p -> phase-2 cost             (nr_normal)
    // cut rows (relp_add_cuts): rows [cut_row0, cut_row0 + nr_cuts) of a structural column p are A[p * ld_a + nr_constraints + k]
    int32_t cut_row0 = 0;
    int32_t nr_cuts = 0;
};

// ratio_rule: relp_ratio_rule_t.  pivot_guard (relp_config_t.pivot_rescue): a pivot row whose element is below `pivot` times the
// largest |entry| of the entering column ends the loop as "no row" -- the host looks at the column and pivots with a tolerance
// relative to it or bars the column (Engine::run) -- instead of being pivoted on
struct Tolerances { double cost, pivot, zero, tie; int32_t ratio_rule, pivot_guard; double guard_rel; };

// PRICE -> entering-column choice without a second pass over d: every PRICE workgroup leaves the
// best (key, j) of its own columns here (key as in k_select_column), k_select_partials reduces them.
struct SelectPartials {
    double*        k1;        // per workgroup: best key (+inf = none)
    int32_t*       j;         // per workgroup: its column
    const uint8_t* in_basis;
    double         tol_cost;
    int32_t        rule;      // relp_pivot_rule_t
    int32_t        n;         // tableau columns (search-order wrap for FirstProfitableWithMemory)
    int32_t        offset;    // first slot this launch may use
    int32_t        nb_struct; // slots [0, nb_struct) belong to structural workgroups of 8 columns from p_lo
    double         tol_tie;   // SteepestDescent: columns within tol_tie*max(1,|min|) of the minimum tie
    int32_t        p_lo;      // first structural column priced by this rank
    int32_t        cols_per_slot;  // structural columns behind one slot (8 dense PRICE, 256 CSC PRICE)
};

// ---- sparse LU engine (device side of relp_lu.hpp) ------------------------------------------------
// One row of a triangular factor in solve order (rows of a level are contiguous): unknown k becomes
// (x[k] - sum_{e in [e0, e1)} val[e] x[idx[e]]) * diag, diag = 1 / (diagonal entry).
struct LuRow { int32_t k, e0, e1, pad_; double diag; };
struct DeviceSchedule {
    const LuRow* rows;          // m rows, level by level
    const int32_t* idx; const double* val;
    const int32_t* level_ptr;   // n_levels + 1 offsets into rows
    int32_t n_levels; int32_t nnz;
    // runs of levels (begin, end, solo) from level 1 on: solo = 1 when every level of the run has at most 8 rows, so that
    // ONE wavefront walks the run without workgroup barriers (relp_lu_device.h: levels_pipelined)
    const int32_t* seg; int32_t n_seg; int32_t pad_;
};
struct DeviceLU {
    int32_t m; int32_t pad_;
    const int32_t* rowperm;   // pivot step -> original row
    const int32_t* colperm;   // pivot step -> basis position
    DeviceSchedule Lf, Uf, Ub, Lb;
};
// The same solve packed "ELL by pass" for the persistent pivot kernel (relp_lu.hpp: ell_pack; relp_lu_device.h: ell_solve):
// one image per schedule, contiguous in device memory in the order of the members below, every array padded to 16 bytes.
static constexpr int kEllLg = 13;                       // sidx = index | lg << kEllLg (relp_lu.hpp: kEllLgShift)
static constexpr int kEllLgWide = 24;                   // the same in the 32-bit images of large bases (FtState::big)
static constexpr int kEllPadHeaders = 4;                // empty pass headers behind the last one: the solves read ahead unchecked
struct EllPass { int32_t lane0, lanes, info, level; };     // info: max lg | last-of-level << 8 | overflow << 9
struct EllSchedule {
    const EllPass*  passes;      // n_passes (+ 3 empty headers)
    const int32_t*  lvl_pass;    // n_levels + 1: first pass of a level (= group of fused levels, relp_lu.hpp: fuse_levels)
    double*         rdiag;       // m + 1: 1 / diagonal by pivot; 0 = row masked by a Forrest-Tomlin update
    double*         sval;        // n_lanes; an update zeroes the entries whose substitution path runs through the masked pivot
    const double*   oval;        // n_ovf: entries beyond the 63rd of a row
    const int32_t*  rovf;        // 2 m (or nothing when n_ovf = 0): overflow range by pivot
    const uint16_t* sidx;        // n_lanes: index | lg << 13; index >= rhs_base: the copy of the right-hand side behind x
    const uint16_t* oidx;        // n_ovf
    const int32_t*  via_ptr;     // m + 1 (U, U' only, else null): positions in sval to zero when a pivot is masked ...
    const int32_t*  via_pos;     // ... (not part of the staged image)
    int32_t n_passes, n_levels, m, n_lanes, n_ovf;
    int32_t bytes;               // size of the image
    int32_t rhs_base;            // m + 1 when some entry reads the right-hand-side copy, else 0 (no copy is made)
    int32_t n_triv;              // rows without entries of U / U' (relp_lu.hpp: EllPacked::triv): x[k] *= rdiag[k] before the passes
    const int32_t* triv;         // n_triv pivots (global, not part of the staged image)
    const int32_t* reach;        // m: first group in which x[p] matters (EllPacked::reach) -> where a sweep may start
    const int32_t* rhs_src;      // n_rhs: slot index rhs_base + i reads the right-hand side of pivot rhs_src[i] (EllPacked::rhs_src)
    int32_t n_rhs, pad_;
    // layout 2 of the persistent kernel (x as a sparse vector: relp_kernels_ft.hip, "hs_"), else null:
    const int32_t* rhs_pos;      // m: i with rhs_src[i] == pivot, or -1 (the inverse of rhs_src)
    const uint32_t* triv_bits;   // m bits: pivot is in `triv`
};

struct DeviceCSC { const int64_t* col_ptr; const int32_t* row_idx; const double* values; };

// ---- sparse LU engine with the Forrest-Tomlin update on the device (relp_kernels_ft.hip) -------------------------
// lower_upper/mod.rs:92-155 keeps `updates: Vec<(EtaFile, RotateToBack)>` and rewrites U at every basis change.  Here L and
// U0 of the last refactorisation are never modified (their level schedules stay valid).  A "pivot" is a step k of the
// factorisation P B Q = L U0; the reference's position of a pivot in U is its rank in the order
// [pivots never updated, ascending k | updated pivots, by the time of their last update], so its rotate-to-back needs no
// data movement.  Update number s ("slot" s, pivot p):
//   * row p and column p of U0 are masked (the pull rows of p get 1/diag = 0, x[p] reads as 0 in the U0 sweeps),
//   * the row eta r = u_bar U^-1 (R = I - e_p r', eta_file.rs:10-18): sparse part over never-updated pivots in the eta
//     pool, part over updated pivots in row s of TC (below the diagonal),
//   * the spike L^-1 a_q (after the earlier etas) becomes the last column of U: sparse part over never-updated pivots in
//     the spike pool, part over updated pivots in column s of TC (on and above the diagonal; TC[s][s] = new diagonal).
// A pivot updated again gets a new slot; its old slot is dead (row / column of TC zeroed, diagonal 1).
static constexpr int kFtThreads = 512;                 // the persistent pivot workgroup: 8 wavefronts
static constexpr int kFtWaves = kFtThreads / 64;       // sparse lists are bucketed by (pivot % kFtWaves): one wavefront per bucket
static constexpr int kFtMaxSlots = 64;                 // one lane of a wavefront per slot in the chains over TC
static constexpr int kFtMaxRows = 1 << 20;             // (layout 2 keeps no per-row array in LDS; the spike pool is tcap x m pairs)
static constexpr int kFtLdsBudget = 156 * 1024;        // of the CU's 160 KB
// Layout 2 keeps "may be non-zero" bitmaps of x (with its right-hand-side copies) and of the spike in LDS, one bit per 2^shift
// entries: the smallest shift with which both fit kFtBitmapBytes.
static constexpr int kFtBitmapBytes = 40 * 1024;
static inline __host__ __device__ int ft_bitmap_shift(int m, int rhs_cap) {
    int s = 0;
    while (((((long long)m + 1 + rhs_cap) >> s) + 64 + (((long long)m) >> s) + 64) / 8 > kFtBitmapBytes) ++s;
    return s;
}
// Everything the Forrest-Tomlin update needs to know about the leaving pivot p, together in one cache line segment (it was
// five dependent global round trips: task -> row header -> entries, via_ptr -> via_pos, twice).
struct FtPivotInfo {
    int32_t u_e0, u_e1;          // row p of U right of the diagonal: entries [u_e0, u_e1) of DeviceLU::Uf idx / val
    int32_t via_u0, via_u1;      // EllSchedule::via_pos range of p in the U image ...
    int32_t via_t0, via_t1;      // ... and in the U' image
    int32_t lev_ub, pad_;
};
struct FtState {
    int32_t  m, tcap, ldt, eta_cap;
    int32_t* hdr;            // [0] updates since the refactorisation (t), [1] eta pool entries in use, [2] refactor requested
    int32_t* slot_pivot;     // tcap
    int32_t* slot_prev;      // tcap: earlier slot of the same pivot or -1
    int32_t* slot_live;      // tcap
    int32_t* tslot;          // m: live slot of a pivot, -1 = never updated
    double*  TC;             // tcap x ldt
    int32_t* eta_off;        // tcap x (kFtWaves + 1): bucket offsets into the eta pool (absolute)
    int32_t* eta_idx; double* eta_val;     // eta_cap
    int32_t* spk_off;        // tcap x (kFtWaves + 1): bucket offsets relative to the slot's region s * m
    int32_t* spk_idx; double* spk_val;     // tcap * m
    const int32_t* inv_rowperm;            // original row -> pivot
    const int32_t* inv_colperm;            // basis position -> pivot
    const int32_t* task_uf;                // pivot -> index of its row in the U (FTRAN) schedule
    const int32_t* task_ub;                // pivot -> index of its row in the U' (BTRAN) schedule
    EllSchedule ell[4];                    // L, U, U', L' packed for the persistent kernel
    const int32_t* lev_ub;                 // pivot -> level of its row in the U' schedule (a solve with e_p or u_bar starts there)
    const struct FtPivotInfo* pinfo;       // per pivot: what an update of that pivot needs, one 32-byte load
    int32_t* journal;                      // (basis position, entering column) of every basis change of the last k_ft_run
                                           // launch, hdr[3] of them: what k_ft_replay applies to freshly computed factors
    double*  spike;          // m: the spike of the last FTRAN (step-wise API: consumed by the next update)
    double*  sp_work;        // m: the spike inside the kernels when it does not live in LDS (big)
    int32_t  hyper;          // bit k: sweep k (L, U, U', L') starts at the first group its right-hand side reaches (RELP_FT_HYPER)
    int32_t  pad2_;
    double*  x_work;         // m + 1 + rhs_cap: the work vector inside the kernels when it does not live in LDS (layout 2)
    unsigned long long* chunk_mask;    // ceil(m / 64) words of scratch (layout 2: ft_compact)
    int32_t* nz_idx; double* nz_val;   // m each (layout 2): the non-zeros of the entering column as (row, alpha), RATIO and the update of b
    int32_t* rho_idx;                  // m (layout 2): the rows where the last pivot row rho is not zero
    int32_t* nzc;                      // [0] entries of nz_idx that describe pb.alpha, [1] of rho_idx / pb.rho (-1: unknown, the
                                       // vectors are rewritten densely), [2] bits_save holds the bitmaps of x and the spike
    uint32_t* bits_save;               // the two LDS bitmaps between launches
    int32_t  big;            // layout (relp_kernels_ft.hip: ft_layout).  0: everything in LDS.  1: spike, permutations and eta pool in
                             // global memory (L2), 32-bit slot indices.  2: x, -pi and the pivot -> slot table there as well (no per-row
                             // array in LDS: any m), 32-bit row indices in the PRICE copy
    int32_t  rhs_cap;        // words behind x[m] for the right-hand-side copies of the fused schedules (0: levels are not fused)
    int32_t  stage[4];       // which of the four schedules (L, U, U', L') fit the LDS staging area
    int32_t  stage_bytes;
    int32_t  lds_bytes;      // dynamic LDS of every FT kernel
    int32_t  max_updates;    // refactor when this many updates are pending (<= tcap)
    int32_t  pad_;
    long long* prof;         // 16 phase accumulators of the persistent kernel (shader clocks, thread 0) or nullptr
};
// PRICE copy of the structural columns for the persistent kernel, k-major ("ELL"): slot k of column p at [k * n + p], so
// that a thread pricing column p issues all its loads at once, coalesced, with no column offsets and no entry loop.
// Tier A: the first kPriceSlots entries of EVERY column (bit 15 of slot 0's index marks a column that has more).  Tier B:
// the long columns once more, complete (up to kPriceLongSlots entries, k-major over n_long), with their column number, so a
// long column is priced by one thread in the column's own order from loads that do not depend on each other.  Columns
// beyond kPriceLongSlots entries (`very_long`) are priced from the CSC arrays.  Padding slots are (0, 0.0).
static constexpr int kPriceSlots = 8;
static constexpr int kPriceLongSlots = 24;
static constexpr int kPriceLongFlag = 0x8000;
static constexpr uint32_t kPriceLongFlag32 = 0x80000000u;
struct PriceEll {
    const uint16_t* idx; const double* val;            // kPriceSlots x nr_normal
    const uint16_t* lidx; const double* lval;          // kPriceLongSlots x n_long
    const uint32_t* idx32; const uint32_t* lidx32;     // the two index arrays 32 bits wide (FtState::big == 2: rows beyond 32,767), else null
    const int32_t* long_cols;                          // n_long
    const int32_t* very_long;                          // n_very_long
    const uint16_t* long_of;                           // nr_normal: index of a column in tier B, 0xFFFF = not there
    int32_t n_long, n_very_long;
};
// What the host wants to know when the pivot kernel returns, written by the kernel itself into pinned, device-mapped host
// memory: after the stream is synchronised it is simply there (no copies, no second synchronisation): the record, the
// header of the update file and the basis (the snapshot a look-ahead refactorisation factorises).
struct FtMirror {
    PivotRecord rec;
    int32_t hdr[4];
    int32_t walked[4], whole[4]; // this launch: passes walked / passes of the whole schedule, summed over its sweeps of L, U, U', L'
    int32_t sweeps[4];           // (the host switches the hyper-sparse start of a schedule off while it saves less than it costs)
    int32_t basis[1];            // m entries
};
struct FtProblem {           // what the persistent kernel needs besides the factors
    DeviceCSC csc; ColumnTable ct; PriceEll pe;
    double *minus_pi, *b, *alpha, *rho, *d;
    int32_t* basis; uint8_t* in_basis; int32_t* trace; int64_t trace_cap;
    PivotRecord* rec;
    FtMirror* mirror;        // or null
    Tolerances tol;
    int32_t rule, n, phase;
    int32_t external_price;  // 1: PRICE ran as a grid launch (k_price_csc + k_select_partials): the entering column is in the record
};

// ---- launchers (all asynchronous on `s`) -------------------------------------------------------
// cost_mode: 0 = no cost term (tableau row), 1 = phase-1 costs (artificial: 1), 2 = phase-2 costs
// PRICE, structural part: d[na + p] = c_p + (-pi[0:mc]) . A[:,p] (+ -pi[bound_row]) for p in [p_lo, p_hi)
void launch_price_structural(const double* A, int64_t ld_a, const ColumnTable& ct, const double* minus_pi,
                             double* d, int32_t p_lo, int32_t p_hi, int32_t cost_mode, const PivotRecord* rec,
                             hipStream_t s);
// structural columns outside [p_lo, p_hi) get +inf (sharded pricing)
void launch_price_mask_unowned(const ColumnTable& ct, double* d, int32_t p_lo, int32_t p_hi,
                               const PivotRecord* rec, hipStream_t s);
// fused PRICE + partial selection (hot loop): same results as the two-kernel form
void launch_price_structural_sel(const double* A, int64_t ld_a, const ColumnTable& ct, const double* minus_pi,
                                 double* d, int32_t p_lo, int32_t p_hi, int32_t cost_mode, SelectPartials sp,
                                 const PivotRecord* rec, hipStream_t s);
void launch_price_virtual_sel(const ColumnTable& ct, const double* minus_pi, double* d, int32_t cost_mode,
                              SelectPartials sp, const PivotRecord* rec, hipStream_t s);
// both of the above in one launch (unsharded loop): structural workgroups first, then the virtual ones
void launch_price_all_sel(const double* A, int64_t ld_a, const ColumnTable& ct, const double* minus_pi, double* d,
                          int32_t p_lo, int32_t p_hi, int32_t cost_mode, SelectPartials sp, const PivotRecord* rec,
                          hipStream_t s);
int32_t price_structural_blocks(int32_t p_lo, int32_t p_hi);
int32_t price_virtual_blocks(const ColumnTable& ct);
// reduce `count` partials, record q / d_q, and build aq (= k_select_column + k_build_column)
void launch_select_partials(SelectPartials sp, int32_t count, const double* d, const double* A, int64_t ld_a,
                            const ColumnTable& ct, int32_t m, double* aq, PivotRecord* rec, hipStream_t s);
// PRICE, artificial + virtual columns
void launch_price_virtual(const ColumnTable& ct, const double* minus_pi, double* d, int32_t cost_mode,
                          const PivotRecord* rec, hipStream_t s);
// entering-column choice over d (masked by in_basis), rule = relp_pivot_rule_t
void launch_select_column(const double* d, const uint8_t* in_basis, int32_t n, int32_t rule, double tol_cost,
                          double tol_tie, PivotRecord* rec, hipStream_t s);
// aq := dense column rec->q in tableau row space (m entries)
void launch_build_column(const double* A, int64_t ld_a, const ColumnTable& ct, int32_t m, double* aq,
                         const PivotRecord* rec, hipStream_t s);
// FTRAN: alpha[i] = Binv[i,:] . aq for i in [row_lo, row_hi); out[i - out_offset]
void launch_ftran(const double* Binv, int64_t ld_b, int32_t m, int32_t row_lo, int32_t row_hi,
                  const double* aq, double* out, int32_t out_offset, const PivotRecord* rec, hipStream_t s);
// RATIO TEST over alpha/b/basis_indices (two-pass tie rule)
void launch_ratio(const double* alpha, const double* b, const int32_t* basis_indices, int32_t m,
                  Tolerances tol, PivotRecord* rec, hipStream_t s);
// rho = Binv[r,:] / alpha_r if row r in [row_lo,row_hi) else 0   (ld_b entries, padding zero)
void launch_compute_rho(const double* Binv, int64_t ld_b, int32_t m, int32_t row_lo, int32_t row_hi,
                        double* rho, PivotRecord* rec, hipStream_t s);
// b, -pi, -obj, basis_indices, in_basis, trace, iteration counter
void launch_update_vectors(int32_t m, const double* alpha, const double* rho, double* b, double* minus_pi,
                           int32_t* basis_indices, uint8_t* in_basis, int32_t* trace, int64_t trace_cap,
                           PivotRecord* rec, hipStream_t s);
// rank-1 update of rows [row_lo,row_hi) of Binv: row_r = rho; row_i -= alpha_i * rho
void launch_update_inverse(double* Binv, int64_t ld_b, int32_t m, int32_t row_lo, int32_t row_hi,
                           const double* alpha, const double* rho, const PivotRecord* rec, hipStream_t s);
// launch_update_vectors + launch_update_inverse in one launch (unsharded explicit path)
void launch_update_inverse_vectors(double* Binv, int64_t ld_b, int32_t m, const double* alpha, const double* rho, double* b,
                                   double* minus_pi, int32_t* basis_indices, uint8_t* in_basis, int32_t* trace,
                                   int64_t trace_cap, PivotRecord* rec, hipStream_t s);

// phase switch: minus_pi[j] = -sum_i w[i] * Binv[i,j]  (w = cost of basis column of row i)
void launch_weighted_column_sums(const double* Binv, int64_t ld_b, int32_t m, const double* w,
                                 double* minus_pi, hipStream_t s);
void launch_set_identity(double* Binv_local, int64_t ld_b, int32_t row_lo, int32_t row_hi, hipStream_t s);
void launch_fill_dense(double* A, int64_t ld, int32_t m, int32_t n, uint64_t seed, int64_t first_column,
                       hipStream_t s);
// A (zeroed, column-major, ld) := the n_cols CSC columns whose pointers start at col_ptr[0] (row_idx / values hold their entries only)
void launch_csc_to_dense(const int64_t* col_ptr, const int32_t* row_idx, const double* values, int32_t n_cols, double* A,
                         int64_t ld, hipStream_t s);

// deferred update (see DeferredUpdate)
// alpha[i] = v[i] + sum_j W[i,j] v[S[j]] for every row
void launch_apply_w(const DeferredUpdate& du, int32_t m, const double* v, double* alpha, const PivotRecord* rec,
                    hipStream_t s);
// FTRAN / alpha = v + W (S'v) that also leave the minimum ratio b_i / alpha_i of every block of rows (8 rows per
// k_ftran workgroup, 256 per k_apply_w workgroup), and the ratio test that starts from those minima (same result
// as launch_ratio, followed by the bookkeeping of launch_eta_prepare when du.kmax > 0; re-reads only the blocks inside the tie
// band).  Unsharded engines.
int32_t ftran_rows_per_block();
void launch_ftran_rmin(const double* Binv, int64_t ld_b, int32_t m, const double* aq, double* out, const double* b,
                       Tolerances tol, double* rmin, const PivotRecord* rec, hipStream_t s);
void launch_apply_w_rmin(const DeferredUpdate& du, int32_t m, const double* v, double* alpha, const double* b, Tolerances tol,
                         double* rmin, const PivotRecord* rec, hipStream_t s);
void launch_ratio_rows(const double* alpha, const double* b, const int32_t* basis_indices, int32_t m, Tolerances tol,
                       const DeferredUpdate& du, const double* rmin, int32_t rows_per_block, PivotRecord* rec, hipStream_t s);
// wr = W[r,:], pick the target column (existing column of row r or a new one), book-keeping
void launch_eta_prepare(const DeferredUpdate& du, PivotRecord* rec, hipStream_t s);
// W <- W + u W[r,:], then column target += / = u, with u = eta - e_r built from alpha
void launch_update_w(const DeferredUpdate& du, int32_t m, const double* alpha, const PivotRecord* rec, hipStream_t s);
// rho = sum over owned rows in {r} U S of coefficient * B0inv[row,:]  (coefficient 1 for r, W[r,j] for S[j])
void launch_rho_deferred(const DeferredUpdate& du, const double* Binv, int64_t ld_b, int32_t m, int32_t row_lo,
                         int32_t row_hi, double* rho, PivotRecord* rec, hipStream_t s);
// B0inv[rows] += W[rows,:] (S' B0inv); the snapshot R must hold S' B0inv of ALL ranks' rows
void launch_flush_snapshot(const DeferredUpdate& du, const double* Binv, int64_t ld_b, int32_t row_lo, int32_t row_hi,
                           const PivotRecord* rec, hipStream_t s);
void launch_flush_apply(const DeferredUpdate& du, double* Binv, int64_t ld_b, int32_t m, int32_t row_lo,
                        int32_t row_hi, const PivotRecord* rec, hipStream_t s);
void launch_flush_reset(const DeferredUpdate& du, PivotRecord* rec, hipStream_t s);

// ---- dense-tableau engine ------------------------------------------------------------------------
// T = B^-1 [all columns] is kept as T = (I + W S') T0 with T0 dense column-major (m x n_store, column
// pitch ld_t) and R0 = S' T0 (the rows of T0 at the distinct pivot rows of the block, row pitch ld_r).
// Storage column = tableau column + col_off (phase 2 skips the artificial block).
struct TableauView {
    double*  T0;      int64_t ld_t;
    double*  R0;      int64_t ld_r;
    double*  d;       // reduced cost per storage column, maintained incrementally
    int32_t  m;
    int32_t  n_store; // stored columns (artificial block + provider columns)
    int32_t  col_off; // first storage column of the current phase's tableau
    int32_t  n;       // tableau columns of the current phase
    int32_t  c_lo, c_hi;  // storage columns owned by this rank (T0, R0 hold only these; pointers are
                          // pre-shifted so that kernels index by global storage column)
};
// T0 := original matrix in row space (artificial unit columns | A + bound rows | virtual unit columns)
void launch_tab_build(const TableauView& tv, const double* A, int64_t ld_a, const ColumnTable& ct, hipStream_t s);
// d[c] = cost[c] - w . T0[:,c] for every stored column (w = cost of the basic variable of each row)
void launch_tab_price_init(const TableauView& tv, const double* w, const double* cost_store, hipStream_t s);
// partial argmin over d (one slot per 256 columns) -- used when the loop is (re)entered
// w[i] = cost of the basic variable of row i; with launch_tab_price_init it recomputes d from T0
void launch_tab_basis_costs(const TableauView& tv, const int32_t* basis_indices, const double* cost_store, double* w,
                            hipStream_t s);
void launch_tab_scan(const TableauView& tv, SelectPartials sp, const PivotRecord* rec, hipStream_t s);
int32_t tab_scan_blocks(int32_t n_owned_columns);
// The two batch solves (launch_lu_ftran_cols, launch_lu_btran_rows) keep the work vector x in LDS, one workgroup per
// right-hand side, while lu_batch_fits_lds(m) (m <= 9,984).  Beyond that -- or when the caller asks for it -- `groups`
// workgroups each own a slab of `ld` doubles (ld >= m, even) in `x` (groups * ld doubles) and walk the right-hand sides in
// a grid-stride loop.  groups == 0: the LDS path.
struct LuSlabs { double* x; int64_t ld; int32_t groups; };
bool lu_batch_fits_lds(int32_t m);
// re-tabulation: T0[:, c] = (LU)^-1 a_c for the stored columns [c_first, c_first + c_count) in one launch (a_c as in
// launch_tab_build)
void launch_lu_ftran_cols(const DeviceLU& lu, const TableauView& tv, const double* A, int64_t ld_a, const ColumnTable& ct,
                          int32_t c_first, int32_t c_count, const LuSlabs& slabs, hipStream_t s);
// entering column from the partials (no column build: the tableau column is read directly)
void launch_tab_select(const TableauView& tv, SelectPartials sp, int32_t count, PivotRecord* rec, hipStream_t s);
// alpha = T[:,q] = T0[:,q] + W R0[:,q]
void launch_tab_column(const TableauView& tv, const DeferredUpdate& du, double* alpha, const PivotRecord* rec,
                       hipStream_t s);
// row r of T (appending T0[r,:] to R0 when r is new in the block), d -= (d_q/alpha_r) row, partial argmin
void launch_tab_row_update(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, PivotRecord* rec,
                           hipStream_t s);
// b, -obj, basis_indices, in_basis, trace, iteration counter (no -pi: it is read off d)
void launch_tab_update_vectors(int32_t m, const double* alpha, double* b, int32_t* basis_indices, uint8_t* in_basis,
                               int32_t* trace, int64_t trace_cap, PivotRecord* rec, hipStream_t s);
// launch_tab_select + launch_tab_column in one launch (every workgroup reduces the partials itself) that also leaves the
// minimum ratio of every block of 256 rows in `rmin` (single-GPU loop), and the ratio test that starts from those minima
// (re-reads only the row blocks inside the tie band)
void launch_tab_select_column_rmin(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t count,
                                   double* alpha, const double* b, Tolerances tol, double* rmin, PivotRecord* rec,
                                   hipStream_t s, const double* shadow = nullptr, int32_t* shadow_meta = nullptr);
void launch_ratio_blocks(const double* alpha, const double* b, const int32_t* basis_indices, int32_t m, Tolerances tol,
                         const DeferredUpdate& du, const double* rmin, PivotRecord* rec, hipStream_t s);
// sharded engines: the same launch with this rank's candidate message [key, j, d_j, alpha (m), minimum ratio per block of
// 256 rows (cdiv(m, 256))] written instead of the record, and the choice among the gathered messages + ratio test from the
// winner's block minima + block bookkeeping in one launch
void launch_tab_select_column_msg(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t count,
                                  double* msg, const double* b, Tolerances tol, PivotRecord* rec, hipStream_t s,
                                  const double* shadow = nullptr, int32_t* shadow_meta = nullptr);
// forced_row >= 0: the winner enters in that row at zero level (no ratio test), phase_one.rs:246-250
void launch_tab_select_candidate_ratio(const double* msgs, int32_t count, int64_t msg_len, int32_t m, double* alpha,
                                       const double* b, const int32_t* basis_indices, int32_t rule, Tolerances tol,
                                       const DeferredUpdate& du, int32_t forced_row, PivotRecord* rec, hipStream_t s);
// sharded removal of basic artificial variables: PRICE partials (key = column index) of the owned columns that may
// replace the variable basic in `row` at zero level
void launch_tab_zero_level_scan(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t row,
                                int32_t nr_artificial, Tolerances tol, const PivotRecord* rec, hipStream_t s);
// launch_tab_row_update, and launch_update_w + launch_tab_update_vectors for the rows, in one launch (disjoint workgroup ranges)
void launch_tab_update_all(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t m,
                           const double* alpha, double* b, int32_t* basis_indices, uint8_t* in_basis, int32_t* trace,
                           int64_t trace_cap, PivotRecord* rec, hipStream_t s);
// Columns of a flush.  Column c of T0 + W R0 differs from T0 only if R0[j][c] != 0 for a pending row j < p (a NaN counts
// as nonzero): for every other column the flush adds sum 0 * w.  With `cols` set the flush first lists those columns and
// copies their R0 columns, then rewrites only them; `cols` = nullptr: every owned column (RELP_TAB_FLUSH_ALL=1).
struct FlushList {
    int32_t*            cols;    // storage columns to flush, ascending (n_owned)
    int32_t*            count;   // how many (one device int)
    unsigned long long* mask;    // per 64 owned columns from c_lo: which of them have a nonzero R0 entry
    double*             R0c;     // R0[:, cols]: kmax rows, position x at R0c[j * ld + x]
    int64_t             ld;      // even, >= n_owned
    unsigned long long* stats;   // {flushes with p > 0, columns rewritten} since create
};
// RELP_TAB_LOAD_BATCH: the tableau kernels walk the p pending rows of W and R0 `batch` loads at a time.  tab_load_batch maps
// a wanted value to one the kernels are instantiated for: 1 (one load per round trip, the control), 8, 16, 32; anything else
// to the default.  kTabSplitDefault / kTabSplitCUs: see launch_tab_ratio_update_all.
static constexpr int32_t kTabLoadBatchDefault = 8;
static constexpr int32_t kTabSplitDefault = 2;
static constexpr int32_t kTabSplitCUs = 256;
int32_t tab_load_batch(int32_t wanted);
// RELP_TAB_COLUMN_ROWS: the rows a workgroup of the column kernel walks in the fused single-GPU loop (DeferredUpdate::col_rows;
// launch_tab_select_column_rmin and launch_tab_ratio_update_all read it, every other launch keeps 256).  256 (the control), 128
// and 64 are themselves; anything else is the default for m rows.
int32_t tab_column_rows(int32_t wanted, int32_t m);
// flush: T0 += W R0 with v_mfma_f64_16x16x4_f64 tiles
void launch_tab_flush(const TableauView& tv, const DeferredUpdate& du, const PivotRecord* rec, const FlushList& fl,
                      hipStream_t s);
// Ratio test + update in ONE launch (single-GPU loop): every workgroup repeats the ratio test from the block minima the column
// kernel left (same code, same answer), then does its share of the update.  What one workgroup rewrites while another may
// still read it is double-buffered: b and the basis array (in -> out, the caller swaps them), row r of W (its new values go
// to `shadow`, {row, length} to `shadow_meta`; the next column kernel or launch_tab_apply_shadow folds them into W), n_eta
// (read as PivotRecord::p_now).  With du.batch > 1 the rows of W get up to du.w_split workgroups per 256 rows, each with an
// equal share of the p pending columns of W <- E W (one of them keeps b, the basis, the shadow row and the record), as long as
// the grid stays within one workgroup per CU (kTabSplitCUs); under batch 1 the grid is the unsplit one.
void launch_tab_ratio_update_all(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, int32_t m,
                                 const double* alpha, const double* b_in, double* b_out, const int32_t* basis_in,
                                 int32_t* basis_out, uint8_t* in_basis, int32_t* trace, int64_t trace_cap, Tolerances tol,
                                 const double* rmin, double* shadow, int32_t* shadow_meta, PivotRecord* rec, hipStream_t s,
                                 const double* msgs = nullptr, int32_t count = 0, int64_t msg_len = 0, int32_t rule = 0);
// (msgs: sharded loop -- the gathered candidate messages; the winner's column and block minima are taken from there and
// `alpha` / `rmin` are ignored)
void launch_tab_apply_shadow(const DeferredUpdate& du, double* shadow, int32_t* shadow_meta, hipStream_t s);
// out[i, k] = T0[i, cols[k]] (row-major m x m): B^-1 from the identity columns
void launch_tab_gather_columns(const TableauView& tv, const int32_t* cols, double* out, hipStream_t s);
// tableau row `row` of the CURRENT T into out[0..n_store) (remove_artificial_basis_variables)
void launch_tab_row(const TableauView& tv, const DeferredUpdate& du, int32_t row, double* out, const PivotRecord* rec,
                    hipStream_t s);
// Dual simplex on the tableau (relp_run_dual; the reference has no dual loop).  One pivot: launch_dual_bmin, launch_dual_row,
// launch_dual_select_column, launch_dual_commit, launch_tab_update_all -- the update takes the pivot from the record and does
// not care that alpha_r and b_r are negative.  `tol`: pivot, zero and tie are read (ratio_rule and the pivot guard are not).
// bmin[k] = the minimum b_i over the rows of block k (256 rows) with b_i < -tol_feas, +inf when there is none
void launch_dual_bmin(const double* b, int32_t m, double tol_feas, double* bmin, const PivotRecord* rec, hipStream_t s);
// step-wise call: the leaving row from the block minima into the record (DEV_NO_ROW: no row is infeasible)
void launch_dual_select_row(const double* b, const int32_t* basis_indices, int32_t m, double tol_feas, double tol_tie,
                            const double* bmin, PivotRecord* rec, hipStream_t s);
// row r of T over the owned stored columns into `row` (indexed from tv.c_lo) and the partial (ratio, column) minima of the dual
// ratio test, one slot per 256 columns; r = forced_row, or the leaving row picked from bmin (forced_row < 0)
void launch_dual_row(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, const double* b,
                     const int32_t* basis_indices, Tolerances tol, double tol_feas, const double* bmin, int32_t forced_row,
                     double* row, const PivotRecord* rec, hipStream_t s);
// q from those partials, (q, d_q, r, leaving) into the record and alpha = T[:,q]; DEV_NO_ROW: the basis is optimal,
// DEV_NO_CANDIDATE: row r has no entry to pivot on (the LP is infeasible)
void launch_dual_select_column(const TableauView& tv, const DeferredUpdate& du, SelectPartials sp, const double* b,
                               const int32_t* basis_indices, Tolerances tol, double tol_feas, const double* bmin,
                               int32_t forced_row, const double* row, double* alpha, PivotRecord* rec, hipStream_t s);
// alpha_r, b_r and the block bookkeeping of the deferred update for the (r, leaving) of the record: ratio_commit_row, no guard
void launch_dual_commit(const double* alpha, const double* b, const DeferredUpdate& du, PivotRecord* rec, hipStream_t s);
// The four in-place changes below (rhs, cost, cut rows, added columns) are built from two device helpers of
// relp_kernels_tableau.hip, which state their summation orders once: for_list<B, V>, a thread's walk over a list staged in LDS 256
// entries at a time with the loads B at a time and V fma chains in ascending entry order (the *_apply kernels and k_tab_cut_rows),
// and list_sum, a workgroup's sum over a list by thread chains and a fixed halving tree (the *_pending kernels).
// A change of rhs entries on the current basis (relp_change_right_hand_side): b += sum_k delta[k] T[:, cols[k]] with T = T0 + W R0
// over the p pending rows, nothing else touched.  cols[k] = the stored column that was the identity column of the k-th changed row
// (entries with delta 0 left out), ascending k as the caller gave them.
struct RhsChange { const int32_t* cols; const double* delta; int32_t count; };
// The list is cut into `splits` equal shares of ceil(count / splits) entries, one grid row of workgroups each.  tab_rhs_splits:
// forced >= 1 (RELP_TAB_RHS_SPLITS) clamped to [1, min(count, kTabRhsMaxSplits)]; else as many as bring the grid of cdiv(m, 256)
// workgroups per split up to kTabRhsGrid workgroups, as long as every split keeps a full LDS chunk (256 entries) of the list.
static constexpr int32_t kTabRhsGrid = 512;
static constexpr int32_t kTabRhsMaxSplits = 256;
int32_t tab_rhs_splits(int32_t m, int32_t count, int32_t forced);
// [k_tab_rhs_pending: v_j = sum_k delta_k R0[j][c_k], p > 0 only] -> [k_tab_rhs_apply: the T0 columns + W v per row; b += or
// partial[split]] -> [k_tab_rhs_reduce: b += the partials in split order, splits > 1 only].  v: du.kmax doubles; partial:
// splits * ld_partial doubles (unused when splits == 1).  No atomics: the same (list, p, splits) gives the same bits.
void launch_tab_rhs_change(const TableauView& tv, const DeferredUpdate& du, const RhsChange& ch, int32_t p, int32_t splits,
                           double* v, double* b, double* partial, int64_t ld_partial, hipStream_t s);
// A change of cost coefficients on the current basis (relp_change_cost): d_c -= sum_k delta[k] T[rows[k], c] with T = T0 + W R0
// over the p pending rows, for every stored column c that is not flagged basic (in_basis == 1 keeps its d to the bit; the kept
// artificial block and barred columns move).  rows[k] = the row in which the k-th changed basic column is basic, ascending (the
// summation order, whatever order the caller named the columns in).  ncols / ndelta: the changed non-basic columns as storage
// columns, ascending, each of which also gets d_c += ndelta.  Entries with delta 0 are in neither list.
struct CostChange { const int32_t* rows; const double* delta; int32_t count; const int32_t* ncols; const double* ndelta; int32_t ncount; };
// The basic list is cut into `splits` equal shares of ceil(count / splits) entries, one grid row of workgroups each.
// tab_cost_splits: forced >= 1 (RELP_TAB_COST_SPLITS) clamped to [1, min(count, kTabCostMaxSplits)]; else as many as bring the grid
// of cdiv(n_columns, 256) workgroups per split up to kTabCostGrid workgroups (five per CU), as long as every split keeps
// kTabCostShareMin entries (three load batches of 8).  A thread's walk down its column is a chain of strided round trips, so
// shares pay long before a share fills an LDS chunk: measured at 10,000 x 10,000, 408 entries take 0.31 ms in one
// share and 0.18 ms in 16, 64 entries 0.124 ms in one and 0.116 ms in 2.
static constexpr int32_t kTabCostGrid = 1280;
static constexpr int32_t kTabCostShareMin = 24;
static constexpr int32_t kTabCostMaxSplits = 256;
int32_t tab_cost_splits(int32_t n_columns, int32_t count, int32_t forced);
// [k_tab_cost_pending: u_j = sum_k delta_k W[j][rows[k]], p > 0 only] -> [k_tab_cost_apply: the T0 rows + u R0 and the direct term
// per stored column; d -= or partial[split]] -> [k_tab_cost_reduce: d -= the partials in split order, splits > 1 only].  u: du.kmax
// doubles; partial: splits * ld_partial doubles, ld_partial >= n_store (unused when splits == 1).  count == 0 with ncount > 0 is one
// launch that reads no tableau entry.  No atomics: the same (lists, p, splits) gives the same bits.
void launch_tab_cost_change(const TableauView& tv, const DeferredUpdate& du, const CostChange& ch, const uint8_t* in_basis, int32_t p,
                            int32_t splits, double* u, double* partial, int64_t ld_partial, hipStream_t s);
// Cut rows added on the current basis (relp_add_cuts).  `count` cuts over the structural columns become the rows tv.m .. tv.m + count
// - 1 of the tableau, their slacks the stored columns tv.n_store .. (tableau columns tv.n ..), basic in their rows; tv is the view
// BEFORE the add, and every buffer has room for the new rows and columns behind it.  Row of cut k in the current basis:
// T[m + k, c] = g_kc - sum_e coef[e][k] T[rows[e], c], T = T0 + W R0 over the p pending rows.  rows: the rows whose basic column is
// structural with a nonzero coefficient in some cut of the call, ascending (the summation order); coef[e * count + k] = that
// column's coefficient in cut k, 0.0 where cut k does not touch it.  A: the engine's matrix, whose rows a_row0 .. a_row0 + count - 1
// of structural column sp (stored column struct_c0 + sp) hold the cuts' coefficients g.
struct CutRows {
    const int32_t* rows; const double* coef; int32_t entries, count;
    const double* A; int64_t ld_a; int32_t a_row0, struct_c0, nr_normal;
};
// What the add sets for the new rows and columns besides T0, R0, W and d: stored cost 0, flag basic (1), identity column and basis
// entry of the new rows, the descriptors of the new virtual columns (first_virtual: the first one's index).  r0_rows: rows of R0
// to clear in the new columns (du.kmax + the scratch row).
struct CutTail {
    double* cost_store; uint8_t* in_basis; int32_t* idcol; int32_t* basis; int32_t *vrow0, *vrow1, *vsign;
    int32_t first_virtual, r0_rows;
};
static constexpr int32_t kTabCutTile = 8;              // cuts per workgroup: eight rows of one column are one 64-byte run of T0
// [k_tab_cut_pending: u[k][j] = sum_e coef[e][k] W[j][rows[e]], grid (p, count), p > 0 only] -> [k_tab_cut_rows: one old stored column
// per thread, kTabCutTile cuts per workgroup, the list walked by for_list, every T0 and R0 load shared by the tile;
// writes T0[m + k, c]: g - acc for a structural column, 0.0 - acc for any other, exactly 0.0 for a column flagged basic (in_basis == 1)]
// -> [k_tab_cut_tail: unit columns of the new slacks in T0, zeros in their R0 entries and in the new rows of W, d = cost = 0 and flag 1
// for the new columns, idcol / basis / pos_of_row (-1) of the new rows, the new virtual descriptors].  b of the new rows is the
// caller's.  The list is not cut into shares.  u: count * du.kmax doubles.  No atomics, fixed summation orders: the same call on the
// same state gives the same bits.
void launch_tab_add_cuts(const TableauView& tv, const DeferredUpdate& du, const CutRows& cr, const uint8_t* in_basis, int32_t p, double* u,
                         const CutTail& ct, hipStream_t s);
// Columns added on the current basis (relp_add_columns).  `count` columns from outside become the stored columns tv.n_store ..
// tv.n_store + count - 1 (tableau columns tv.n ..), non-basic; tv is the view BEFORE the add, and every buffer has room for the
// new columns behind it.  T = (I + W S') T0 is linear in T0 and the stored columns that were the identity at the start are B^-1
// in that form, so the new column k needs no read of W:
//   T0[:, n_store + k] = sum_e coef[e][k] T0[:, cols[e]]        R0[j][n_store + k] = T0[S[j], n_store + k]   (j < p)
// cols: the identity columns (storage columns, inside [tv.c_lo, tv.c_hi)) of the rows with a nonzero coefficient in some column
// of the call, rows ascending (the summation order); coef[e * count + k] = the coefficient of column k in that row, 0.0 where
// column k does not touch it.  d_new / cost_new: reduced cost and cost of the new columns (count each; the host forms d from -pi).
struct ColumnAdd {
    const int32_t* cols; const double* coef; int32_t entries, count;
    const double* d_new; const double* cost_new;
};
// What the add sets for the new columns besides T0 and R0: d, the stored cost, flag non-basic (0) and the empty descriptors
// (vrow0 = vrow1 = -1, vsign = 1) of the new virtual columns (first_virtual: the first one's index).  r0_rows: rows of R0 the new
// columns have (du.kmax + the scratch row); the ones from p on are cleared.
struct ColumnTail {
    double* cost_store; uint8_t* in_basis; int32_t *vrow0, *vrow1, *vsign;
    int32_t first_virtual, r0_rows;
};
static constexpr int32_t kTabColTile = 8;              // new columns per workgroup: every T0 load feeds eight accumulators
// [k_tab_col_apply: one row per thread, 256 rows and kTabColTile new columns per workgroup, the list walked by for_list, every
// (coalesced) T0 load shared by the tile, one fma chain per new column from 0.0 in ascending list order; writes
// T0[i, n_store + k] for i < m] -> [k_tab_col_tail: R0[j][n_store + k] = the T0 entry just written at row du.S[j] for j < p and
// 0.0 for the other rows of R0, d, stored cost, flag 0 and the descriptors of the new columns].  The list is not cut into shares.
// No atomics, fixed summation orders: the same call on the same state gives the same bits.
void launch_tab_add_columns(const TableauView& tv, const DeferredUpdate& du, const ColumnAdd& ca, int32_t p, const ColumnTail& ct,
                            hipStream_t s);
// Rows and columns taken out of a column-major image in place, order preserved (relp_remove_cuts, relp_remove_columns): img holds m
// rows and n columns, column c at c * ld; rows (nr, ascending, distinct, inside [0, m)) and cols (nc, ascending, distinct, inside
// [0, n)) are device lists.  Afterwards the m - nr surviving rows of the n - nc surviving columns stand in rows [0, m - nr) of columns
// [0, n - nc) in their old order with their old bits, and rows [m - nr, m) of every column and rows [0, m) of columns [n - nc, n) are
// 0.0 (what room rows and room columns hold); rows from m on and columns from n on are not touched, nor are the rows above rows[0]
// in the columns left of cols[0].  Copies only: nothing is recomputed.
// [k_tab_drop_rows<B>, if nr > 0: a workgroup owns whole columns (grid min(n, kTabCompactGrid), columns strided over it) and walks
// them from rows[0] down in chunks of 256 B destination rows -- B coalesced loads per thread, their wait, __syncthreads(), B coalesced
// stores; chunk k stores only below where chunk k + 1 loads] -> [k_tab_drop_columns<B>, if nc > 0: one row per thread over the
// m - nr rows, 64 threads per workgroup, destination columns ascending from cols[0], B loads before their B stores; sources lie
// right of everything the thread has written].  B = kTabCompactB; batch == 1: B = 1, one by one (the control).  No atomics, no
// flags, no communication between workgroups; the result does not depend on the order in which workgroups run.
static constexpr int32_t kTabCompactB = 4;
static constexpr int32_t kTabCompactGrid = 2048;        // 256 CUs x 8 workgroups of 256 threads
void launch_tab_compact(double* img, int64_t ld, int32_t m, int32_t n, const int32_t* rows, int32_t nr, const int32_t* cols, int32_t nc,
                        int32_t batch, hipStream_t s);
// Batched ratio tests over the tableau as it stands, T = T0 + W R0 over the p pending rows, read-only (relp_row_ratios,
// relp_rhs_ranging).  The list is taken kTabRatioChunk entries per workgroup (a fixed size, not a rule: eight rows of one column are
// one 64-byte sector of T0), grid = chunks x blocks of 256 columns (rows); the second launch has one workgroup per list entry.
// No sums, no global atomics: minima of (ratio, index) and tie keys in total orders, the same bits every run.
static constexpr int32_t kTabRatioChunk = 8;
// Rows rows[k] of T, k < count (device list, any order, repeats allowed): per direction (0 = down: entries < -tol.pivot, ratio
// dz_j / -entry; 1 = up: entries > tol.pivot, ratio dz_j / entry) over the non-basic columns (sp.in_basis[j] == 0) the entering
// rule of launch_dual_select_column -- minimum ratio, lowest column inside its tie band.  ratio / column[dir * count + k], (+inf,
// -1) without a candidate.  part_k / part_j: 2 * count * tab_scan_blocks(owned columns) entries of scratch.
void launch_tab_row_ratios(const TableauView& tv, const DeferredUpdate& du, const SelectPartials& sp, Tolerances tol,
                           const int32_t* rows, int32_t count, int32_t p, double* part_k, int32_t* part_j, double* ratio,
                           int32_t* column, hipStream_t s);
// Stored columns cols[k] of T, k < count: per direction (0 = decrease: entries a_i > tol.pivot, ratio bz_i / a_i; 1 = increase:
// a_i < -tol.pivot, bz_i / -a_i) the reference ratio test -- minimum ratio, smallest leaving column inside its tie band, whatever
// tol.ratio_rule says.  ratio / row[dir * count + k], (+inf, -1) without a candidate.  part: 2 * count * cdiv(m, 256) doubles.
void launch_tab_rhs_ranging(const TableauView& tv, const DeferredUpdate& du, const double* b, const int32_t* basis_indices,
                            Tolerances tol, const int32_t* cols, int32_t count, int32_t p, double* part, double* ratio, int32_t* row,
                            hipStream_t s);
// Gomory cuts from rows of the tableau as it stands, in structural space (relp_gomory_cuts), read-only like the ratio queries.
// Entry k < count: row rows[k] with fraction f0[k] of its b (f0[k] < 0: the entry is skipped, every pi of it is 0.0).  is_integer:
// one flag per tableau column (tv.n), nullptr = all integer.  kind: 0 fractional, 1 mixed.  A: the engine's matrix with the cut rows
// behind the ct.nr_constraints constraint rows (ct.nr_cuts of them, tableau rows ct.cut_row0 ..), structural column sp the stored
// column struct_c0 + sp.  Scratch, all written by the launch: pi count x (tv.c_hi - tv.c_lo), y count x tv.m (both row-major by
// entry), bad count x tab_scan_blocks(stored columns) (1.0: a continuous column with |entry| > tol.zero in a fractional cut), g
// count x nr_normal.
struct GomoryCuts {
    const int32_t* rows; const double* f0; const uint8_t* is_integer;
    int32_t count, kind;
    const double* A; int64_t ld_a; int32_t struct_c0, nr_normal;
    double *pi, *y, *bad, *g;
};
// [y = 0] -> [k_tab_gomory_rows<B, 8>: grid chunks of kTabRatioChunk entries x blocks of 256 stored columns, one column per thread,
// the entry of k_tab_row_ratios (T0, then one fma per pending row in ascending j), the rule of relp_gomory_cuts on it; writes pi,
// exactly 0.0 for a basic column and for the kept artificial block, y[k][vrow0[v]] = vsign[v] * pi for the virtual column v, and bad]
// -> [k_tab_gomory_structural<B, 8>: one structural column per workgroup, the chunk's eight cuts together, lanes along the rows of
// A: thread t chains  acc = fma(y_i, A[i, c], acc)  over the rows t, t + 256, .. of A ascending from 0.0 (every row of A: y is 0.0
// where a row has no slack or pi is 0.0), the halving tree of list_sum, then  (sum - pi_c) + y[bound_row(c)]  (the last term only
// where c has a bound row); writes g].  No atomics, fixed orders: the same call on the same state gives the same bits.
void launch_tab_gomory(const TableauView& tv, const DeferredUpdate& du, const ColumnTable& ct, const uint8_t* in_basis, Tolerances tol,
                       const GomoryCuts& gc, int32_t p, hipStream_t s);
// The snapshot of a trial (relp_trial_begin / relp_trial_end), either direction: the segments of `t` (relp_trial.hpp: at most
// kTrialMaxSegments, every src, dst 16-byte aligned, no overlap) copied src -> dst in one launch of k_tab_trial_copy.  The grid
// strides over the 16-byte units of all segments together -- 16-byte loads and stores, kTrialB units per thread and stride
// iteration with every load issued before the first store --, one workgroup per 256 units up to kTabTrialGrid (the device's share:
// 256 CUs x 8 workgroups of 256 threads); each segment's tail of bytes % 16 bytes goes bytewise.  No atomics, no LDS.
static constexpr int32_t kTabTrialGrid = 2048;
void launch_tab_trial_copy(const TrialTable& t, hipStream_t s);
// A pool on the device, the column pool (relp_pool_create .. relp_pool_add) or, inside a CutPoolView, the cut pool: read-only to
// every launch below but for the activity flags.  Sliced ELL as relp_pool.hpp packs it: item k (a pool column, or a cut) is lane
// k % 64 of slice k / 64, entry e of it stands at slice_ptr[k / 64] + e * 64 + k % 64 and slice s is
// (slice_ptr[s + 1] - slice_ptr[s]) / 64 entries wide; the indices (rows, or structural columns) ascend inside an item, padding has
// index -1 and is skipped by its index (it reaches no fma).  scalar (the cost, or the right-hand side), active: one per item.
struct PoolView {
    const int64_t* slice_ptr; const int32_t* idx; const double* val; const double* scalar; uint8_t* active;
    int32_t count;
};
// The sweep both pools share (k_pool_sweep).  An item's value is one fma chain over its entries in stored (ascending index) order,
// acc = fma(vec[index], value, acc), every operand rounded once; the loads of a chain are issued sixteen entries at a time
// (kPoolBatch: indices and values first, then the gathers from vec), and the order of the chain does not depend on it.  The pool
// indices are cut into `segments` shares of S = ceil(count / segments) items and every share into chunks of kPoolChunk items:
// [k_pool_sweep, grid segments x chunks (one dimension), 256 threads: thread t of chunk (s, c) has the item
// s * S + c * kPoolChunk + t where that lies below the end of the share and of the pool -- consecutive lanes, consecutive items, so
// a wave reads consecutive entries of a slice; all[k] = the value when `all` is given; an item is a candidate when it is active and
// its value < -tol; the chunk's minimum in the total order (key, pool index) by block_min_key -> part_d / part_k[s * chunks + c],
// (+inf, -1) without a candidate] -> [k_pool_fold, only when chunks > 1, one workgroup per share: the share's chunks folded in the
// same order into its first slot part_d / part_k[s * chunks]] -> [k_pool_winners, one workgroup of 256 threads, shares 256 at a
// time: an ordered scan over the 256 flags "has a winner" gives every winner its place; out_k / out[0 .. *found) = the winners in
// ascending share order, out = the winner's key or, where the launch says so, its value].  No atomics; minima in a total order and
// one fma chain per item: the same launch on the same state gives the same bits.  segments < 1: only `all` is written (no partials,
// no further launch).  part_d / part_k: segments * pool_segment_chunks(count, segments) entries; out_k / out: segments entries;
// found: one.
//
// -pi as relp_get_minus_pi reads it off the tableau: (-pi)_i = d[idcol[i]] - cost_store[idcol[i]], rounded once, over the m engine
// rows.  vec: m doubles of scratch; every launch below first writes -pi there (k_pool_minus_pi, one row per thread) and its chains
// read it from there.
struct MinusPi { const double* d; const double* cost_store; const int32_t* idcol; int32_t m; double* vec; };
// Multiple pricing (relp_pool_price, relp_pool_reduced_costs): [k_pool_minus_pi] -> the sweep with the reduced cost as value and
// as key -- the chain from cost[k] over -pi, the one Engine::add_columns forms for d_new, to the bit; out_d = the key.
void launch_pool_price(const PoolView& pv, const MinusPi& mp, int32_t segments, double tol, double* d_all, double* part_d, int32_t* part_k,
                       int32_t* out_k, double* out_d, int32_t* found, hipStream_t s);
// The operands of launch_tab_add_columns for the pool columns ids[0 .. count) (device list, distinct), formed on the device
// (relp_pool_add).  m: the engine rows; longest: the longest chosen column (entries, the second grid dimension's reach).
//   rank     m words of scratch: afterwards rank[i] = the place of row i in the union list, -1 for a row no chosen column touches
//   cols     the union list: idcol[i] of the touched rows i, ascending; *entries = its length
//   coef     coef[e * count + x] = the coefficient of column ids[x] in the row of list entry e, 0.0 elsewhere (`entries` x count;
//            the caller knows `entries` from its host copy -- it sizes the buffer and the zero fill)
//   col_a    the dense row-space block of added columns: column a0 + x at (a0 + x) * ld_c gets the m-vector of column ids[x]
//   d_new, cost_new   the chain above and the cost of column ids[x];  the activity flags of the chosen columns are cleared
// [rank = 0] -> [k_pool_entries<false>, one workgroup per 256 entries of a chosen column: rank[row] = 1; many writers, one value] ->
// [k_pool_union, one workgroup, rows 256 at a time, an ordered scan over the marks: rank, cols, *entries] -> [k_pool_minus_pi] -> [coef = 0, the new
// columns of col_a = 0] -> [k_pool_entries<true>, the same grid: one entry per thread into coef and col_a] -> [k_pool_chosen, one
// workgroup per chosen column, the operands staged in LDS 256 entries at a time, thread 0 chains: d_new, cost_new, active = 0].  No atomics; every output word has one writer or one value.
struct PoolAdd {
    const int32_t* ids; int32_t count, m, longest, entries;
    int32_t* rank; int32_t* cols; int32_t* entries_out; double* coef;
    double* col_a; int64_t ld_c; int32_t a0;
    double* d_new; double* cost_new;
};
void launch_pool_add_operands(const PoolView& pv, const MinusPi& mp, const PoolAdd& pa, hipStream_t s);
// active[ids[x]] = flag for x < count (relp_pool_set_active); ids: device list
void launch_pool_set_active(const PoolView& pv, const int32_t* ids, int32_t count, int32_t flag, hipStream_t s);
// A cut pool on the device (relp_cutpool_create .. relp_cutpool_add): a PoolView whose items are cuts over the structural columns
// with their right-hand sides (relp_cutpool.hpp), and the norms, one per cut.
struct CutPoolView { PoolView pv; const double* norm; };
// The current vertex over the structural columns: x[j] = b[r] where structural column j is basic in row r (basis[r] == j), +0.0
// elsewhere.  x: nr_normal doubles of scratch; every launch sequence below first writes it ([x = +0.0, a memset] -> [k_cutpool_x, one
// row per thread; a column is basic in at most one row, so no two threads write one word]) and its chains read it from there.
struct Vertex { const double* b; const int32_t* basis; int32_t m, nr_normal; double* x; };
void launch_cutpool_x(const Vertex& vx, hipStream_t s);
// Separation (relp_cutpool_separate, relp_cutpool_slacks): [x] -> the sweep with the slack as value -- s_k = rhs_k - acc, acc the
// chain from 0.0 over x, an entry on a column >= nr_normal skipped like padding -- and as key s_k or, with by_efficacy,
// s_k / norm_k (norm 0 counts as 1); out_s[i] = s_all[out_k[i]], the slack, not the key.  s_all: count doubles (always needed).
void launch_cutpool_separate(const CutPoolView& cv, const Vertex& vx, int32_t segments, double tol, int32_t by_efficacy, double* s_all,
                             double* part_d, int32_t* part_k, int32_t* out_k, double* out_s, int32_t* found, hipStream_t s);
// The operands of launch_tab_add_cuts for the pool cuts ids[0 .. count) (device list, distinct), formed on the device
// (relp_cutpool_add) as Engine::add_cuts forms them on the host.  longest: the longest chosen cut (entries); room: the entries the
// caller sized rows and coef for (the structural columns the chosen cuts touch bound the list).
//   mark     nr_normal words of scratch: 0 for a column no chosen cut touches, 1 for a touched one that is not basic, 2 + the place
//            in the union list for a touched one that is
//   rows     the union list: the rows r, ascending, whose basic column is structural and touched; *entries_out = its length
//   coef     coef[e * count + x] = the coefficient of the basic column of list entry e in cut ids[x], 0.0 elsewhere (room x count)
//   A        rows a_row0 + x of the structural columns of the engine's matrix = the coefficients of cut ids[x], 0.0 elsewhere
//   b_new    b_new[x] = rhs - acc, acc = fma(coef[e][x], b[rows[e]], acc) from 0.0 over the WHOLE list in ascending e, zeros
//            included: the loop of Engine::add_cuts.  (The caller points it at b[m_old].)  The chosen cuts' flags are cleared.
// [mark = 0] -> [k_cutpool_entries<false>, one workgroup per 256 entries of a chosen cut: mark[column] = 1; many writers, one
// value] -> [k_cutpool_union, one workgroup, rows 256 at a time, an ordered scan over the flags: mark, rows, *entries_out] ->
// [coef = 0, the new rows of A = 0] -> [k_cutpool_entries<true>, the same grid: one entry per thread into A, and into coef where
// its column is in the list] -> [k_cutpool_chosen, one workgroup per chosen cut, the operands staged in LDS 256 entries at a
// time, thread 0 chains: b_new, active = 0].  No atomics; every output word has one writer or one value.
struct CutPoolAdd {
    const int32_t* ids; int32_t count, m, nr_normal, longest, room;
    const int32_t* basis; const double* b;
    int32_t* mark; int32_t* rows; int32_t* entries_out; double* coef;
    double* A; int64_t ld_a; int32_t a_row0;
    double* b_new;
};
void launch_cutpool_add_operands(const CutPoolView& cv, const CutPoolAdd& ca, hipStream_t s);

// ---- sparse LU engine ------------------------------------------------------------------------------
// PRICE over CSC columns (thread per column), partial argmin per 256 columns
void launch_price_csc(const DeviceCSC& csc, const ColumnTable& ct, const double* vec, double* d, int32_t p_lo,
                      int32_t p_hi, int32_t cost_mode, SelectPartials sp, const PivotRecord* rec, hipStream_t s);
// the same plus the virtual columns (launch_price_virtual_sel) in one launch
void launch_price_csc_all(const DeviceCSC& csc, const ColumnTable& ct, const double* vec, double* d, int32_t nr_normal,
                          int32_t cost_mode, SelectPartials sp, int32_t nb_virtual, const PivotRecord* rec, hipStream_t s);
int32_t price_csc_blocks(int32_t p_lo, int32_t p_hi);
// k_select_partials with the entering column scattered from CSC instead of copied from dense A
void launch_select_partials_csc(SelectPartials sp, int32_t count, const double* d, const DeviceCSC& csc,
                                const ColumnTable& ct, int32_t m, double* aq, PivotRecord* rec, hipStream_t s);
void launch_build_column_csc(const DeviceCSC& csc, const ColumnTable& ct, int32_t m, double* aq, const PivotRecord* rec,
                             hipStream_t s);
// FTRAN: v = (LU)^-1 aq  (one persistent workgroup, level-scheduled pull solves, work vector in LDS)
void launch_lu_ftran(const DeviceLU& lu, const double* aq, double* v, double* scratch, const PivotRecord* rec,
                     hipStream_t s);
// BTRAN: rho' = z' (LU)^-1 with z = e_r + sum_j W[r,j] e_S[j] (rhs == nullptr, r from rec or `row` >= 0)
//        or z = rhs (dense, indexed by basis position)
void launch_lu_btran(const DeviceLU& lu, const DeferredUpdate& du, const double* rhs, int32_t row, double* rho,
                     double* scratch, const PivotRecord* rec, hipStream_t s);
// every row of B^-1 = (LU)^-1 in one launch (workgroup i: e_i' B^-1 -> out + i * ld); `none`: a DeferredUpdate with kmax = 0
void launch_lu_btran_rows(const DeviceLU& lu, const DeferredUpdate& none, double* out, int64_t ld, const LuSlabs& slabs,
                          hipStream_t s);

// ---- Forrest-Tomlin engine (relp_kernels_ft.hip) ---------------------------------------------------------------
// bytes of dynamic LDS the FT kernels need besides the staging area
size_t ft_lds_base_bytes(int32_t m, int32_t tcap, int32_t eta_cap, int32_t tier, int32_t rhs_cap);
// LDS bytes a schedule needs to be staged (relp_lu_device.h: schedule_lds_bytes)
int64_t ft_schedule_stage_bytes(int32_t m, int64_t nnz, int32_t n_levels, int32_t n_seg);
// up to `max_pivots` whole pivots (PRICE -> FTRAN -> RATIO -> FT update -> BTRAN -> b, -pi, basis) in ONE launch of one
// workgroup; stops early when the outcome is decided or a refactorisation is due (hdr[2] = 1)
void launch_ft_run(const DeviceLU& lu, const FtState& st, const FtProblem& pb, int64_t max_pivots, hipStream_t s);
// alpha = B^-1 a for tableau column `column` (>= 0; -2: rec->q) or the dense right-hand side `rhs` (indexed by original
// row); leaves the spike in st.spike
void launch_ft_ftran(const DeviceLU& lu, const FtState& st, const FtProblem& pb, int32_t column, const double* rhs, double* alpha,
                     hipStream_t s);
// rho' = c' B^-1 with c = e_row (row >= 0; -2: rec->r) or the dense `rhs` (indexed by basis position)
void launch_ft_btran(const DeviceLU& lu, const FtState& st, const FtProblem& pb, int32_t row, const double* rhs, double* rho,
                     hipStream_t s);
// the Forrest-Tomlin update for the basis change in position rec->r with the spike in st.spike
void launch_ft_update(const DeviceLU& lu, const FtState& st, const FtProblem& pb, hipStream_t s);
// the first `count` basis changes of the journal as Forrest-Tomlin updates of the (fresh) factors; hdr[2] = 2 when one fails
void launch_ft_replay(const DeviceLU& lu, const FtState& st, const FtProblem& pb, int32_t count, hipStream_t s);

// sharded helpers
void launch_pack_candidate(const double* aq, int32_t m, double* msg, PivotRecord* rec, hipStream_t s);
void launch_select_candidate(const double* msgs, int32_t count, int64_t msg_len, int32_t m, double* aq,
                             int32_t rule, double tol_tie, PivotRecord* rec, hipStream_t s);
void launch_gather_alpha(const double* slices, int32_t count, int32_t stride, int32_t m, double* alpha,
                         const PivotRecord* rec, hipStream_t s);
void launch_pad_slice(double* slice, int32_t valid, int32_t stride, hipStream_t s);

}  // namespace relp
