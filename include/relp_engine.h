/*
 * relp_engine.h -- C ABI of the MI355X-native revised-simplex pivot engine.
 *
 * This is the drop-in boundary for RELP's hot path (vandenheuvel/rust-lp, `relp` 0.0.5).  The
 * reference has no FFI; the unit replaced is `Tableau<Carry<F, BI>, K>` + `PivotRule` driven by
 * `phase_one::primal` / `phase_two::primal`.  Each entry point names the reference interface it
 * replaces (file:line under /root/reference/src/algorithm/two_phase/).  A Rust maintainer binds
 * these with `extern "C"` and implements `InverseMaintener` / `PivotRule` on top.
 *
 * Conventions
 *   - plain C types only; every function returns a relp_status_t (0 = ok, < 0 = error); no panics
 *     or aborts cross the boundary (the reference panics on a zero pivot, carry/mod.rs:291).
 *   - a handle is not thread-safe: one host thread per handle; each handle owns one HIP stream
 *     (relp_set_stream lets the caller supply its own, e.g. the stream RCCL collectives run on).
 *   - the problem is copied at create time (the reference borrows the provider, `&'a MP`); all
 *     getters copy into caller-provided host buffers.
 *   - field = f64 (the reference has no float field, README.md:27: this is the build's extension);
 *     comparisons use the tolerances of relp_config_t, all-zero tolerances = the reference's exact
 *     `<`, `>`, `==`.
 *   - column indices are tableau indices: in phase 1 the `nr_artificial` artificial columns come
 *     first (kind/artificial/partially.rs:72-80), in phase 2 they are provider indices.
 */
#ifndef RELP_ENGINE_H
#define RELP_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct relp_engine relp_engine_t;

typedef enum {
    RELP_OK = 0,
    RELP_E_ARG = -1,          /* bad argument */
    RELP_E_HIP = -2,          /* HIP runtime error (relp_last_error gives the text) */
    RELP_E_ZERO_PIVOT = -3,   /* "Pivot value can't be zero." carry/mod.rs:291, basis_inverse_rows.rs:47 */
    RELP_E_SINGULAR = -4,     /* basis could not be inverted (from_basis) */
    RELP_E_STATE = -5,        /* call not valid in the current phase / state */
    RELP_E_UNSUPPORTED = -6,
    RELP_E_ALLOC = -7
} relp_status_t;

/* Outcome of a loop (algorithm/mod.rs:46-50 `OptimizationResult`, phase_one.rs:177-194). */
typedef enum {
    RELP_RUNNING = 0,          /* iteration limit hit, more pivots possible */
    RELP_OPTIMAL = 1,          /* phase 2: no candidate column (FiniteOptimum) */
    RELP_UNBOUNDED = 2,        /* phase 2: no pivot row (Unbounded) */
    RELP_INFEASIBLE = 3,       /* phase 1 ended with objective != 0 */
    RELP_PHASE_ONE_DONE = 4,   /* phase 1 ended feasible; the tableau is now NonArtificial */
    RELP_NO_ROW_PHASE_ONE = 5  /* "Artificial cost can not be unbounded." phase_one.rs:143 */
} relp_outcome_t;

/* strategy/pivot_rule.rs:38,62,97 */
typedef enum {
    RELP_RULE_FIRST_PROFITABLE = 0,
    RELP_RULE_FIRST_PROFITABLE_WITH_MEMORY = 1,   /* phase-1 default, phase_one.rs:55,97 */
    RELP_RULE_STEEPEST_DESCENT = 2                /* = most negative d_j; phase-2 default, two_phase/mod.rs:44 */
} relp_pivot_rule_t;

typedef enum { RELP_FORMAT_CSC = 0, RELP_FORMAT_DENSE = 1 } relp_format_t;
typedef enum { RELP_MEM_HOST = 0, RELP_MEM_DEVICE = 1 } relp_memory_t;

/* matrix_provider/matrix_data.rs:54-90.  Constraint rows are ordered [== | range | <= | >=]; the
 * slack, bound-slack columns and bound rows are virtual (matrix_data.rs:37-52, 308-348). */
typedef struct {
    int32_t nr_normal;                        /* structural columns */
    int32_t nr_eq, nr_range, nr_le, nr_ge;    /* constraint rows */
    int32_t format;                           /* relp_format_t */
    int32_t matrix_memory;                    /* relp_memory_t: where col_ptr/row_idx/values/dense live */
    const int64_t *col_ptr;                   /* CSC: nr_normal + 1 */
    const int32_t *row_idx;                   /* CSC: sorted inside a column */
    const double  *values;                    /* CSC */
    const double  *dense;                     /* DENSE: column-major nr_constraints x nr_normal */
    int64_t        dense_ld;                  /* DENSE: leading dimension (>= nr_constraints) */
    const double  *b;                         /* host, nr_constraints (all >= 0, general_form/mod.rs:574) */
    const double  *ranges;                    /* host, nr_range */
    const double  *cost;                      /* host, nr_normal */
    const double  *upper_bound;               /* host, nr_normal; +inf = none (lower bounds are 0) */
} relp_matrix_data_t;

typedef struct {
    int32_t device;               /* HIP device ordinal, -1 = current */
    int32_t phase_one_rule;       /* relp_pivot_rule_t */
    int32_t phase_two_rule;
    double  tol_cost;             /* candidate iff d_j < -tol_cost          (pivot_rule.rs:56,81,117) */
    double  tol_pivot;            /* ratio test iff alpha_i > tol_pivot      (tableau/mod.rs:227).  Defaults:
                                   * tol_cost = tol_feas = 1e-7, tol_pivot = 1e-5, tol_tie = 1e-9, tol_zero = 1e-11.
                                   * tol_pivot is larger than the others because an alpha_i that is exactly 0 in the
                                   * reference's rational field carries the rounding noise of B^-1 in f64 (1e-7 .. 1e-6 on
                                   * unscaled Netlib data such as 25FV47, whose entries span 1e-3 .. 1e4): a pivot on
                                   * such an element destroys the basis inverse */
    double  tol_zero;             /* |b_i| <= tol_zero reads as 0 in the ratio */
    double  tol_tie;              /* ratio ties: <= min + tol_tie*max(1,|min|), smallest leaving column wins
                                     (tableau/mod.rs:229-239) */
    double  tol_feas;             /* phase 1 feasible iff |obj| <= tol_feas*max(1, initial obj) (phase_one.rs:146) */
    int32_t poll_interval;        /* relp_run: iterations enqueued between host polls of the outcome */
    int32_t trace_capacity;       /* pivots recorded on the device (0 = no trace) */
    /* column / row sharding for multi-GPU pricing; 0,1 = everything local */
    int32_t shard_rank, shard_count;
    /* basis-inverse maintenance: 0 = rank-1 update of the explicit inverse at every pivot
     * (basis_inverse_rows.rs:131-142 literally); K > 0 = deferred: the explicit inverse is kept as
     * (I + W S') B0inv and the K most recent pivots are folded in by one m x K x m GEMM ("flush");
     * -1 = automatic (64 when m >= 4096, else 0; the dense tableau engine, which always works in blocks: 64, and 96 for
     * tableaus of 40,000 columns or more with m >= 4096).  Results are the same up to f64 rounding. */
    int32_t update_block;
    /* relp_engine_kind_t: which device representation maintains the basis inverse */
    int32_t engine;
    /* ---- f64 safeguards the exact reference has no need for; 0 (relp_default_config) = the reference's rule ----
     * relp_ratio_rule_t.  RELP_RATIO_LARGEST_PIVOT: among the rows inside the tie band of the minimum ratio the largest pivot
     * element wins (compared at float precision), then the lowest leaving column; tableau/mod.rs:229-239 has only the latter.
     * On degenerate LPs with badly scaled columns (Netlib GREENBEA / GREENBEB, which the reference `#[ignore]`s) the
     * reference's choice among dozens of ratio-0 rows regularly lands on a pivot of 1e-4 beside candidates of 1e+2; exact
     * arithmetic does not care, an f64 basis inverse is destroyed within ~1,000 pivots. */
    int32_t ratio_rule;
    /* relp_artificial_removal_t.  RELP_ARTIFICIAL_TEXTBOOK: at the end of phase 1 a basic artificial variable is pivoted out
     * in the row it is basic in (phase_one.rs:236 takes the row it started in: an artificial that re-entered the basis in
     * another row survives into phase 2 as a free column on that row -- Netlib GREENBEA ends 73,482 below its optimum that
     * way), on the first non-basic column with a non-zero element in that row, whatever that column's reduced cost (the
     * pivot is at zero level either way; phase_one.rs:239-244 only tries columns whose reduced cost is exactly zero), and
     * where there is no such column the artificial's OWN constraint is removed together with the basis position it sits in
     * (the two positions are exchanged first -- rows of B^-1 / of the tableau, b, the basis array -- so that one index names
     * both: that pair always leaves a basis of the filtered problem; phase_one.rs:252 pushes the artificial's INDEX, which
     * names another row as soon as `<=` rows lie in front of the artificial's row: the reference then deletes a
     * non-redundant row and optimises a relaxation -- Netlib 80BAU3B ends at 964,593.50 instead of 987,224.19 that way). */
    int32_t artificial_removal;
    /* RELP_PIVOT_RESCUE (1): a pivot loop that ends without a pivot row is looked at before it is believed.  The reference
     * takes every alpha_i > 0 (tableau/mod.rs:227); f64 needs `tol_pivot`, and an ABSOLUTE one is wrong both ways on unscaled
     * data: Netlib SIERRA (entries up to 1e5) has legitimate columns whose largest entry is 1e-5 -- all of it below the
     * tolerance, phase 1 "unbounded" after 620 pivots on every engine -- while SCSD6 prices a column whose reduced cost
     * (-2.2e-7) and positive entries (2.2e-7 beside entries of -5) are both artefacts of its six-digit data.  With the
     * rescue the engine reads alpha back: positive entries of at least tol_pivot * max|alpha| are pivoted on (one step with the
     * tolerance lowered to that), otherwise the column is barred from pricing until the basis has changed, and an outcome
     * reached with barred columns is confirmed once more without them.  Rare events, handled on the host. */
    int32_t pivot_rescue;
    /* 1: the explicit inverse / the tableau is rebuilt from the basis columns at an interval the engine adapts itself -- halved
     * (down to 32 pivots) when a rebuild moves b by more than 1e-7 relative, doubled (up to 1,024) when by less than 1e-10 --
     * instead of the hand-set relp_set_reinversion_interval (the LU engine refactorises every update_block pivots anyway). */
    int32_t auto_reinversion;
} relp_config_t;

typedef enum { RELP_RATIO_REFERENCE = 0, RELP_RATIO_LARGEST_PIVOT = 1 } relp_ratio_rule_t;
typedef enum { RELP_ARTIFICIAL_REFERENCE = 0, RELP_ARTIFICIAL_TEXTBOOK = 1 } relp_artificial_removal_t;

typedef enum {
    /* revised simplex with the explicit dense inverse (`Carry<_, BasisInverseRows<_>>`): PRICE and FTRAN
     * are HBM streams over A and B^-1 at every pivot */
    RELP_ENGINE_REVISED = 0,
    /* dense tableau T = B^-1 [A | slacks] kept as (I + W S') T0: PRICE is one tableau row, FTRAN one
     * tableau column per pivot, and T0 is updated by an m x K x n GEMM on the f64 matrix cores every
     * update_block pivots (needs 8 m n bytes; same pivots as the revised engine up to f64 rounding).
     * relp_from_basis re-tabulates T0 = B^-1 [A | I] from a factorisation of the given basis.  Column-sharded across GPUs
     * through relp_shard_* / relp_shard_run: both
     * phases, artificial removal and redundant-row removal included (the revised engine shards only LPs with a full
     * slack basis). */
    RELP_ENGINE_TABLEAU = 1,
    RELP_ENGINE_LU = 2,       /* sparse LU of the basis + pending updates (Carry<_, LUDecomposition<_>>) */
    /* resolved at create (relp_engine_kind tells which): the dense tableau while it fits comfortably -- 8 m n <= 64 GB and
     * m <= 50,000 rows, where it is the fastest engine on every file of the reference -- the LU engine beyond,
     * where its O(nnz) memory and the persistent kernel's third layout win (5.3b) */
    RELP_ENGINE_AUTO = 3
} relp_engine_kind_t;

/* relp_default_config: the reference's rules literally (every safeguard 0, engine RELP_ENGINE_REVISED).
 * relp_robust_config: what an f64 caller who wants the optimum rather than the reference's pivot sequence should take --
 * ratio_rule = RELP_RATIO_LARGEST_PIVOT, artificial_removal = RELP_ARTIFICIAL_TEXTBOOK, pivot_rescue, auto_reinversion,
 * engine = RELP_ENGINE_AUTO; no per-file knobs (tests/test_gpu_big_pins.py, tests/test_gpu_corpus.py). */
void relp_default_config(relp_config_t *cfg);
void relp_robust_config(relp_config_t *cfg);
/* the engine in use (RELP_ENGINE_AUTO resolved) */
int32_t relp_engine_kind(const relp_engine_t *h);
/* RELP_PIVOT_RESCUE / auto_reinversion at work: out[4] = { pivots made with a lowered tolerance, columns barred, outcomes
 * confirmed without barred columns, the re-inversion interval in effect } */
relp_status_t relp_robust_stats(const relp_engine_t *h, int64_t *out4);
const char *relp_last_error(const relp_engine_t *h);
const char *relp_version(void);

/* ---- construction ----------------------------------------------------------------------------
 * Tableau::<_, Partially<_>>::new (kind/artificial/partially.rs:125-206) +
 * InverseMaintener::create_for_partially_artificial (carry/mod.rs:381-426): B^-1 = I, b = rhs,
 * -pi_i = -1 on artificial rows, -obj = -sum of b over artificial rows. */
relp_status_t relp_engine_create(const relp_matrix_data_t *md, const relp_config_t *cfg, relp_engine_t **out);
void          relp_engine_destroy(relp_engine_t *h);
relp_status_t relp_set_stream(relp_engine_t *h, void *hip_stream);

/* ---- one pivot, step by step (the body of phase_one.rs:135-146 / phase_two.rs:32-50) ---------- */
/* PivotRule::select_primal_pivot_column (strategy/pivot_rule.rs:25-33): full PRICE on the device. */
relp_status_t relp_select_primal_pivot_column(relp_engine_t *h, int32_t rule, int32_t *found,
                                              int32_t *column, double *relative_cost);
/* Tableau::relative_cost (tableau/mod.rs:102-108) for every column (basic columns included). */
relp_status_t relp_relative_costs(relp_engine_t *h, double *out_n);
/* Tableau::generate_column (tableau/mod.rs:122-126) = BasisInverse::generate_column
 * (basis_inverse_rows.rs:144-155): FTRAN; result stays on the device until the next call;
 * `out_m` (may be NULL) receives the dense column. */
relp_status_t relp_generate_column(relp_engine_t *h, int32_t column, double *out_m);
/* Tableau::generate_element (tableau/mod.rs:129-134). */
relp_status_t relp_generate_element(relp_engine_t *h, int32_t row, int32_t column, double *out);
/* Tableau::select_primal_pivot_row (tableau/mod.rs:221-247) on the last generated column. */
relp_status_t relp_select_primal_pivot_row(relp_engine_t *h, int32_t *found, int32_t *row);
/* The same ratio test on a column the caller supplies (dense, m entries, host memory), the reference's signature
 * `select_primal_pivot_row(&self, column: &SparseVector)`; leaves the last generated column untouched. */
relp_status_t relp_select_primal_pivot_row_of(relp_engine_t *h, const double *column_m, int32_t *found, int32_t *row);
/* Tableau::bring_into_basis (tableau/mod.rs:47-60) -> Carry::change_basis (carry/mod.rs:549-570):
 * consumes the last generated column; returns the leaving column. */
relp_status_t relp_bring_into_basis(relp_engine_t *h, int32_t column, int32_t row, double relative_cost,
                                    int32_t *leaving_column);

/* ---- whole loops on the device ------------------------------------------------------------------
 * relp_run: up to max_iters basis changes of the current phase with no per-pivot host sync.
 * phase_one::primal (phase_one.rs:125-170) / phase_two::primal (phase_two.rs:22-51). */
relp_status_t relp_run(relp_engine_t *h, int64_t max_iters, int64_t *iterations_done, int32_t *outcome);
/* SolveRelaxation::solve_relaxation (two_phase/mod.rs:30-76): phase 1, artificial removal
 * (phase_one.rs:223-260), phase switch (kind/non_artificial.rs:151-220), phase 2. */
relp_status_t relp_solve_relaxation(relp_engine_t *h, int64_t max_iters, int32_t *outcome);
/* ---- dual simplex (RELP_ENGINE_TABLEAU, unsharded, phase 2) --------------------------------------------------------
 * No counterpart in the reference: its `primal_dual` and `criss_cross` modules are empty placeholders.  Like the f64 field this
 * is the build's extension, for the bases the primal loops cannot use: reduced costs d >= 0 but b = B^-1 rhs with negative
 * entries -- the all-surplus basis of a covering LP (min c'x, A x >= b, c > 0) after relp_from_basis, or an optimal basis
 * after relp_set_right_hand_side.  Rules, with the absolute tolerances of relp_config_t:
 *   leaving row      row i is infeasible iff b_i < -tol_feas; the minimum b_i over the infeasible rows; among the infeasible
 *                    rows with b_i <= min + tol_tie*max(1,|min|) the smallest leaving column wins (the tie order of the primal
 *                    ratio test); no infeasible row: the basis is optimal
 *   entering column  over tableau row r, the non-basic columns j (a column barred by the pivot rescue is not one) with
 *                    T[r,j] < -tol_pivot; ratio dz_j / (-T[r,j]) with dz_j = 0 when d_j <= tol_zero, else d_j; the minimum
 *                    ratio; among ratios <= min + tol_tie*max(1,|min|) the lowest j wins; no candidate: the LP is infeasible
 *   pivot            on T[r,q] < 0, by the update of the primal loop
 * relp_config_t.ratio_rule and pivot_rescue are IGNORED by the dual loop (no largest-pivot tie-break, no rescue of a small
 * pivot); update_block and the flush schedule, relp_set_reinversion_interval, auto_reinversion, trace_capacity (phase field 2)
 * and poll_interval are honoured exactly as by relp_run.
 * relp_run_dual: up to max_iters dual pivots with no per-pivot host sync.  *outcome: RELP_OPTIMAL, RELP_INFEASIBLE, or
 * RELP_RUNNING at the iteration limit.  RELP_E_UNSUPPORTED on another engine or a sharded one; RELP_E_STATE in phase 1, and when
 * the basis is not dual feasible (a non-basic column with d_j < -tol_cost: relp_last_error names it) -- the handle stays usable,
 * and relp_run may follow on it in every case. */
relp_status_t relp_run_dual(relp_engine_t *h, int64_t max_iters, int64_t *iterations_done, int32_t *outcome);
/* The two selections of one dual pivot, step by step like relp_select_primal_pivot_row (no counterpart in the reference): the
 * leaving row by the rule above (*found = 0: no row is infeasible), and the entering column for tableau row `row` (*found = 0:
 * no candidate).  One pivot is then relp_select_dual_pivot_row, relp_select_dual_pivot_column, relp_generate_column(column),
 * relp_bring_into_basis(column, row, d_column). */
relp_status_t relp_select_dual_pivot_row(relp_engine_t *h, int32_t *found, int32_t *row);
relp_status_t relp_select_dual_pivot_column(relp_engine_t *h, int32_t row, int32_t *found, int32_t *column);
/* A new right-hand side for the current basis (no counterpart in the reference, which borrows an immutable provider):
 * `rhs_m` has relp_nr_rows entries in the engine's current row order (b, upper bounds, ranges), of any sign.  The tableau is
 * re-tabulated on the current basis -- b = B^-1 rhs, the reduced costs, -obj -- at the cost of relp_from_basis.  The reduced
 * costs do not depend on rhs: an optimal basis stays dual feasible, and relp_run_dual re-solves from it.  The rebuild counts in
 * relp_reinversions but does not adapt the auto_reinversion interval (b moved with rhs, not by drift).  RELP_ENGINE_TABLEAU,
 * unsharded, phase 2. */
relp_status_t relp_set_right_hand_side(relp_engine_t *h, const double *rhs_m);
/* Single rhs entries moved on the current basis WITHOUT a re-tabulation (no counterpart in the reference): what a branch-and-bound
 * or cutting-plane driver does at every node before relp_run_dual.  rhs[rows[k]] = values[k] for k < count; `rows` are engine rows
 * in the current order (the indexing of relp_set_right_hand_side), values of any sign.  Nothing is rebuilt: B^-1 is in the tableau
 * (the stored columns that were the identity at the start), so with delta_k = values[k] - rhs[rows[k]] and c_k the identity column
 * of row rows[k]
 *     b_i += sum_k delta_k * (T0[i,c_k] + sum_{j<p} W[j][i] * R0[j][c_k])          (p = pending rows of the open update block)
 * in fixed summation orders (no atomics: the same call on the same state gives the same bits).  Entries with delta_k == 0 are dropped
 * before anything is uploaded.  -obj is re-formed from the new b as a re-tabulation forms it, and the call synchronises.  The
 * reduced costs, the basis, the pending update block (no flush happens) and relp_reinversions are untouched; every later
 * re-tabulation (re-inversion interval, auto_reinversion, relp_from_basis, relp_set_right_hand_side) builds on the new values.
 * RELP_E_ARG with nothing changed: a row out of range, a row named twice, a value that is not finite, count < 0.  count == 0 is a
 * no-op.  The list is processed in `splits` shares: chosen so that the launch covers the device while every share keeps at least 256
 * entries, or RELP_TAB_RHS_SPLITS=n at create (clamped to [1, min(entries, 256)]).  Measured at 10,000 x 10,000
 * (profiles/r13_rhs_in_place.md): 0.08 ms for 1 or 64 entries and 0.24 ms for all 10,000 (0.28 ms with an update
 * block open) against 517 ms of relp_set_right_hand_side -- the every-entry change beats the rebuild too.
 * RELP_ENGINE_TABLEAU, unsharded, phase 2: RELP_E_UNSUPPORTED on another or a sharded engine, RELP_E_STATE in phase 1 (all four
 * calls). */
relp_status_t relp_change_right_hand_side(relp_engine_t *h, const int32_t *rows, const double *values, int32_t count);
/* The upper bound of structural (provider) column `column`: relp_change_right_hand_side on its bound row with count = 1 ("tighten
 * x_j <= floor(x_j), relp_run_dual").  RELP_E_ARG when the column is not structural, when its bound was +inf at create (it has no
 * bound row, and none can be added or dropped here) or when `value` is not finite.  A value below 0 is accepted: relp_run_dual then
 * reports RELP_INFEASIBLE.
 * A lower bound l on x_j is not built; a caller gets it with what exists by substituting x_j = l + x'_j: rhs_i -= l * A_ij over the
 * constraint rows (one relp_change_right_hand_side), the bound row becomes u - l, and the constant c_j * l goes on the objective. */
relp_status_t relp_set_upper_bound(relp_engine_t *h, int32_t column, double value);
/* The rhs in effect (b, upper bounds, ranges): relp_nr_rows entries in the engine's current row order. */
relp_status_t relp_get_right_hand_side(relp_engine_t *h, double *out_m);
/* out4 = { in-place changes so far, columns of B^-1 they read (entries with a nonzero delta), pending rows p of the update block
 * at the last change, shares (k-splits) of its last launch }. */
relp_status_t relp_rhs_stats(const relp_engine_t *h, int64_t *out4);
/* Cost coefficients moved on the current basis WITHOUT a flush or a re-tabulation (no counterpart in the reference): what a
 * parametric objective, a feasibility pump or a Lagrangian loop does between re-solves, and the call that moves a cost as far as
 * Tableau.cost_ranging says it may go.  cost[columns[k]] = values[k] for k < count; `columns` are structural provider columns,
 * 0 <= column < nr_normal (virtual columns have cost 0 and keep it), values of any sign.  b does not depend on the cost: the basis
 * stays primal feasible and relp_run continues from it; neither primal nor dual feasibility is required.  Nothing is rebuilt: with
 * delta_k = values[k] - cost[columns[k]], r_k the row in which a changed BASIC column is basic and the basic entries sorted by r_k
 * ascending (the summation order: the order of the caller's list cannot change a bit),
 *     d_c -= sum_k delta_k * (T0[r_k,c] + sum_{j<p} W[j][r_k] * R0[j][c])          (p = pending rows of the open update block)
 * for every stored column c the pivot update maintains d for, the kept artificial block (relp_get_minus_pi reads it) and barred
 * columns included; a changed NON-BASIC column also gets d_c += its delta.  A column flagged basic keeps its d to the bit (the
 * pivot update pinned it at exactly 0).  Fixed summation orders, no atomics: the same call on the same state gives the same bits.
 * Entries with delta_k == 0 are dropped before anything is uploaded; a call whose deltas are all zero leaves d bit-identical.
 * -obj is re-formed from b with the new costs, and the call synchronises.  b, the basis, the flags, the pending update block (no
 * flush happens), the trace, relp_reinversions and relp_tab_flush_stats are untouched; every later reprice and re-tabulation
 * (re-inversion interval, relp_from_basis, relp_set_right_hand_side) builds on the new costs.
 * RELP_E_ARG with nothing changed: a column out of range, a column named twice, a value that is not finite, count < 0, a missing
 * list.  count == 0 is a no-op.  The basic list is processed in `splits` shares: the rule of DESIGN.md 10, or
 * RELP_TAB_COST_SPLITS=n at create (clamped to [1, min(basic entries, 256)]).
 * RELP_ENGINE_TABLEAU, unsharded, phase 2: RELP_E_UNSUPPORTED on another or a sharded engine, RELP_E_STATE in phase 1 (all four
 * calls). */
relp_status_t relp_change_cost(relp_engine_t *h, const int32_t *columns, const double *values, int32_t count);
/* All nr_normal structural costs at once by the route the engine has: an open update block is flushed (it counts in
 * relp_tab_flush_stats), the costs are replaced, d = c - c_B' T0 in one coalesced pass over T0 and -obj = -c_B' b.  No LU, no
 * re-tabulation, relp_reinversions unchanged.  The yardstick of relp_change_cost, and the call to make when most costs move: the
 * in-place walk reads T0 by rows (strided), this one by columns (DESIGN.md 10 has the crossover).  RELP_E_ARG with nothing
 * changed when a value is not finite. */
relp_status_t relp_set_cost(relp_engine_t *h, const double *cost_n);
/* The structural costs in effect, nr_normal entries. */
relp_status_t relp_get_cost(relp_engine_t *h, double *out_n);
/* out4 = { in-place changes so far, tableau rows they read (basic entries with a nonzero delta), pending rows p of the update block
 * at the last change, shares (k-splits) of its last launch }.  Refused calls and calls with count == 0 are not counted; a call
 * whose deltas are all zero counts as a change that read 0 rows. */
relp_status_t relp_cost_stats(const relp_engine_t *h, int64_t *out4);
/* Cut rows added to the tableau on the current basis WITHOUT a flush or a re-tabulation (no counterpart in the reference): what a
 * cutting-plane or branch-and-cut driver does between re-solves.  `count` cuts
 *     sum_e values[e] * x[col_idx[e]] <= rhs[k]        (e in [row_ptr[k], row_ptr[k + 1]))
 * in CSR over the structural provider columns, 0 <= col_idx[e] < nr_normal.
 * Where a cut goes: cut k of the call becomes engine row relp_nr_rows() + k, behind every existing row (bound and range-bound rows
 * included); its slack becomes provider column relp_nr_columns() + k, behind every existing column.  No existing row or column
 * index moves.
 * The new slack is basic in its row, with cost 0 and sign +1, and behaves like a <= slack everywhere: relp_get_basis_indices,
 * relp_current_bfs, relp_get_trace and relp_from_basis name it by that index; relp_change_right_hand_side, relp_rhs_ranging and
 * relp_row_ratios take the cut row by its row index; relp_get_right_hand_side, relp_set_right_hand_side, relp_get_b and
 * relp_get_minus_pi have the new length.
 * Other cut forms: rhs may have any sign, a >= cut is passed negated, an equality is two cuts.  A coefficient on a virtual column
 * is not accepted; the caller substitutes it.
 * What the call changes: nothing is flushed or re-tabulated.  With B(r) the basic column of row r, the row of cut k in the current
 * basis is
 *     T[new,c] = g_c - sum_r g_B(r) * (T0[r,c] + sum_{j<p} W[j][r] * R0[j][c])      b_new = rhs[k] - sum_r g_B(r) * b_r
 * over the rows r whose basic column is structural with a nonzero coefficient (p = pending rows of the open update block), written
 * into T0.  The bits of d over the old columns, the bits of b over the old rows, -obj, the basis entries of the old rows, the
 * flags of the old columns, W, R0 and T0 over the old rows and old columns, the trace, relp_reinversions and relp_tab_flush_stats
 * stay exactly as they were.  A violated cut shows as b_new < 0: the state relp_run_dual starts from.
 * Pinned values: new-row entries of stored columns flagged basic are exactly 0.0; the new slack columns are exactly unit columns
 * and their d is exactly 0.0.  A barred column and the kept artificial block are computed like every other column.
 * After the call the PRICE partials are invalid and the record is re-armed; relp_run_dual or relp_run may follow.  The call
 * synchronises.  Every later rebuild (re-inversion interval, auto_reinversion, relp_from_basis, relp_set_right_hand_side)
 * includes the cuts.
 * Deterministic: the rows r are walked in ascending order whatever the order of the entries inside the caller's CSR, no atomics;
 * the same call on the same state gives the same bits.
 * RELP_E_ARG with nothing changed: count < 0, a missing array, a row_ptr that does not ascend from 0, a column outside
 * [0, nr_normal), a column named twice in one cut, a coefficient or rhs that is not finite.  count == 0 is a no-op.
 * RELP_ENGINE_TABLEAU, unsharded, phase 2: RELP_E_UNSUPPORTED on another or a sharded engine, RELP_E_STATE in phase 1 (all three
 * calls).  RELP_E_ALLOC when growing fails: every new buffer is allocated before an old one is released, so the handle is then as
 * it was.
 * Capacity: relp_reserve_cuts(rows) makes room for `rows` cut rows in all (a no-op when there is room already; it never shrinks,
 * adds nothing and changes no getter).  relp_add_cuts grows by itself when room lacks, to max(cuts then in the tableau, 2 x the
 * room so far, 16).  Growing re-allocates and copies the tableau: old and new T0 live side by side for a moment, so a driver
 * that knows its cut budget reserves it once, while memory is plentiful.
 * A cut is taken back with relp_remove_cuts (below) once its slack is basic; a tight cut can be relaxed instead,
 * relp_change_right_hand_side(cut row, a value it cannot bind at). */
relp_status_t relp_add_cuts(relp_engine_t *h, int32_t count, const int64_t *row_ptr, const int32_t *col_idx, const double *values,
                            const double *rhs);
relp_status_t relp_reserve_cuts(relp_engine_t *h, int32_t rows);
/* out4 = { cuts in the tableau, cut rows there is room for, tableau rows the last relp_add_cuts read (the rows r above, over all
 * cuts of the call), pending rows p of the update block at that call }. */
relp_status_t relp_cut_stats(const relp_engine_t *h, int64_t *out4);
/* Columns added to the tableau on the current basis WITHOUT a flush or a re-tabulation (no counterpart in the reference): what
 * column generation (cutting stock, Dantzig-Wolfe, branch-and-price) does between re-solves -- take relp_get_minus_pi, price columns
 * outside the LP, add the ones with a negative reduced cost, relp_run.  `count` columns in CSC over the engine rows in their current
 * order, the indexing of relp_change_right_hand_side (cut rows and bound rows included): column k has the coefficients values[e] in
 * the rows row_idx[e], e in [col_ptr[k], col_ptr[k + 1]), 0 <= row_idx[e] < relp_nr_rows().
 * Where a column goes: column k of the call becomes provider column relp_nr_columns() + k as it is at the call, behind every
 * existing column (cut slacks and earlier added columns included).  No existing row or column index moves.
 * What the variable is: x >= 0 without an upper bound, cost cost[k], non-basic (flag 0).  relp_get_basis_indices, relp_current_bfs,
 * relp_get_trace, relp_from_basis, relp_generate_column and relp_relative_costs name it by that index.
 * What the call changes: nothing is flushed or re-tabulated.  The stored columns that were the identity at the start are B^-1, in
 * the update-block form T = (I + W S') T0, which is linear in T0, so with idcol(i) the identity column of row i
 *     T0[:, new_k] = sum_e a_k[rows_e] * T0[:, idcol(rows_e)]      (rows_e ascending, an fma chain from 0.0)
 *     R0[j][new_k] = T0[S[j], new_k]  for the p pending rows        (R0 = S' T0 still holds; W is not read)
 *     d[new_k]     = c_k + sum_i (-pi)_i * a_k[i]                   (i ascending over the column's nonzero entries, an fma chain from
 *                                                                    c_k, -pi as relp_get_minus_pi gives it at the call)
 * and T0 + W R0 of the new column is B^-1 a_k with the open block left open.  The new columns' stored cost and flag are written.
 * b, -obj, the basis, T0 / R0 / W and d over the old columns, the flags of the old columns, the trace, relp_reinversions,
 * relp_tab_flush_stats, relp_cut_stats and relp_nr_rows stay exactly as they were, to the bit.  After the call the PRICE partials
 * are invalid and the record is re-armed; relp_run or relp_run_dual may follow.  The call synchronises.
 * Deterministic: the rows are walked in ascending order whatever the order of the entries inside the caller's CSC, no atomics, the
 * list is not cut into shares; the same call on the same state gives the same bits.  An explicit zero coefficient is dropped
 * before anything is uploaded.
 * Every later rebuild (re-inversion interval, auto_reinversion, relp_from_basis, relp_set_right_hand_side) includes the columns:
 * the host LU sees them when they are basic, the re-tabulation recomputes their stored columns, the objective uses their costs.
 * relp_set_cost replaces the nr_normal structural costs only: the added columns keep theirs, and their d is recomputed with the
 * rest.  relp_change_cost, relp_get_cost, relp_set_upper_bound and the col_idx of relp_add_cuts keep refusing an index >= nr_normal:
 * a cut added later has coefficient 0 on every added column; changing the cost of an added column and cuts over added columns
 * are not built.  relp_add_cuts after relp_add_columns works, and so do columns with entries in cut rows.
 * RELP_E_ARG with nothing changed: count < 0, a missing array, a col_ptr that does not ascend from 0, a row outside
 * [0, relp_nr_rows()), a row named twice in one column, a coefficient or cost that is not finite, more than 524,280 columns in one
 * call.  count == 0 is a no-op.  A column without entries is accepted: T0 = 0, d = cost.
 * RELP_ENGINE_TABLEAU, unsharded, phase 2: RELP_E_UNSUPPORTED on another or a sharded engine, RELP_E_STATE in phase 1 (all three
 * calls).  RELP_E_ALLOC when growing fails: every new buffer is allocated before an old one is released, so the handle is then as
 * it was.
 * Capacity: relp_reserve_columns(columns) makes room for `columns` added columns in all (a no-op when there is room already; it
 * never shrinks, adds nothing and changes no getter).  relp_add_columns grows by itself when room lacks, to max(added columns then
 * in the tableau, 2 x the room so far, 16).  The room for cuts and the room for columns are independent: relp_reserve_cuts and
 * relp_cut_stats report exactly what they report without added columns.  Growing re-allocates and copies the tableau, as for cuts;
 * room for columns alone leaves the row-sized buffers and the matrix where they are (a caller's device matrix stays adopted).
 * A column nobody wants any more is taken back with relp_remove_columns (below) while it is non-basic. */
relp_status_t relp_add_columns(relp_engine_t *h, int32_t count, const int64_t *col_ptr, const int32_t *row_idx, const double *values,
                               const double *cost);
relp_status_t relp_reserve_columns(relp_engine_t *h, int32_t columns);
/* out4 = { added columns in the tableau, columns there is room for, identity columns the last relp_add_columns read (the rows with
 * a nonzero coefficient in some column of the call), pending rows p of the update block at that call }.  Refused calls and calls
 * with count == 0 are not counted. */
relp_status_t relp_column_stats(const relp_engine_t *h, int64_t *out4);
/* Cut rows and added columns taken out of the tableau IN PLACE (no counterpart in the reference): what a branch-and-cut or
 * column-generation driver does when it purges -- cuts whose slack has gone basic after a round, columns whose reduced cost stays
 * positive after pricing, everything a node added when branch-and-bound backtracks.  Both are exact deletions, without arithmetic
 * and without a re-tabulation; nothing is re-allocated or shrunk, and the freed room is what the next relp_add_cuts /
 * relp_add_columns uses (relp_cut_stats and relp_column_stats report fewer cuts or columns and the same room).
 * relp_remove_cuts: `rows` are `count` engine rows of cut rows, the indexing of relp_change_right_hand_side (with cuts in the
 * tableau these are the last rows: [relp_nr_rows() - cuts, relp_nr_rows())), each at most once, in any order.  With i the row of a
 * cut and s its slack, s must be basic, in whichever tableau row r that is (after pivots r need not be i: read
 * relp_get_basis_indices).  Constraint i leaves everything indexed by constraint (the right-hand side, relp_get_minus_pi, the cut
 * rows of the matrix, the entries added columns hold in it), tableau row r everything indexed by basis position (the rows of the
 * tableau, relp_get_b, relp_get_basis_indices), column s everything indexed by column (relp_relative_costs, relp_generate_column, the
 * flags, the costs).  Both index spaces close up in order: a surviving row or column keeps its place relative to every other
 * survivor, so an index above a removed one drops by the number of removed ones below it -- the column indices inside
 * relp_get_basis_indices and relp_current_bfs too.  relp_nr_rows and relp_nr_columns drop by count.
 * relp_remove_columns: `columns` are `count` provider columns added by relp_add_columns, each at most once, in any order, each
 * NON-basic.  The column, its reduced cost, cost and flag go; the columns behind it (cut slacks and later added columns) close up in
 * order.  relp_nr_columns drops by count, no row moves.
 * The flush: both calls first settle and flush the open update block exactly as relp_flush does (a removed row that is pending
 * would leave the block without its row), so relp_tab_flush_stats may move; relp_reinversions, relp_retab_stats and the trace do
 * not.  Trace entries recorded before the call keep the row and column indices of their time.
 * The bit contract: after the call every surviving entry of the tableau -- every column over the surviving rows, d over the
 * surviving columns, b over the surviving rows, -obj, the flags and the costs -- has exactly the bits it has on a handle that went
 * through the same calls and called relp_flush instead; relp_get_minus_pi loses entry i and keeps the other bits.  The PRICE partials
 * are invalid and the record is re-armed; relp_run and relp_run_dual may follow.  The call synchronises.  Every later rebuild
 * (re-inversion interval, auto_reinversion, relp_from_basis, relp_set_right_hand_side) works on the smaller LP.
 * Refusals leave the handle untouched and do not flush.  RELP_E_ARG: count < 0, a missing array, an index that is no cut row (no
 * added column), an index named twice.  RELP_E_STATE: a cut whose slack is not basic (a tight cut: relax it, or pivot), an added
 * column that is basic, phase 1.  RELP_E_UNSUPPORTED: another or a sharded engine.  count == 0 is a no-op (no flush either). */
relp_status_t relp_remove_cuts(relp_engine_t *h, const int32_t *rows, int32_t count);
relp_status_t relp_remove_columns(relp_engine_t *h, const int32_t *columns, int32_t count);
/* out4 = { cuts removed so far, added columns removed so far, (stored column x row) entries of the tableau the last removal moved
 * (rows: every stored column from the first removed tableau row down; columns: every row of the columns behind the first removed
 * one), pending rows p of the update block the last removal flushed }.  Refused calls and calls with count == 0 are not counted. */
relp_status_t relp_removal_stats(const relp_engine_t *h, int64_t *out4);
/* Batched ratio tests over the tableau as it stands (no counterpart in the reference): what a branch-and-bound driver asks at a
 * node ("which fractional row is the dearest to branch on?") and a solve asks at its end (the ranging report).  Both are read-only:
 * nothing is flushed or re-tabulated, and T0, R0, W, d, b, the basis, the flags, the PRICE partials, the record, the trace and
 * relp_reinversions stay as they are; while an update block is open the entries are T0 + W R0 over its p pending rows, formed in the
 * order of relp_generate_column and relp_select_dual_pivot_column.  Deterministic: minima in total orders, no atomics on results,
 * the same call on the same state gives the same bits.  `rows` are engine rows in the current order (the indexing of
 * relp_change_right_hand_side), in any order, a row may be named twice; outputs are per list entry and any of them may be NULL.
 * RELP_E_ARG with nothing written: a row out of range, count < 0.  count == 0 is a no-op.  Two launches and one download per call,
 * the list in chunks of 8 entries per workgroup (a fixed size).  RELP_ENGINE_TABLEAU, unsharded, phase 2: RELP_E_UNSUPPORTED on
 * another or a sharded engine, RELP_E_STATE in phase 1 (all three calls).
 *
 * relp_row_ratios, entry k with r = rows[k], over the non-basic columns 0 <= j < n (a barred column is excluded as in the dual loop):
 *   down_ratio[k]  = min d'_j / (-T[r,j]) over T[r,j] < -tol_pivot, d'_j = 0 when d_j <= tol_zero, else d_j
 *   up_ratio[k]    = min d'_j /   T[r,j]  over T[r,j] >  tol_pivot
 *   *_column[k]    = the lowest j among the ratios <= min + tol_tie * max(1, |min|); (+inf, -1) without a candidate
 * down is literally the entering rule of relp_select_dual_pivot_column(r): the same bits and the same column.  Dual feasibility is
 * not required.  Two readings, x_B the basic variable of row r and c its cost:
 *   penalty     the objective degrades by down_ratio per unit x_B is pushed down (the dual pivot that removes b_r < 0 enters
 *               down_column), by up_ratio per unit it is pushed up: the Driebeek/Tomlin penalties of branching on x_B
 *   cost range  the basis stays optimal while the cost of x_B stays within [c - down_ratio, c + up_ratio]
 *
 * relp_rhs_ranging, entry k with row rows[k] and a = T[:, idcol] = B^-1 e_row, bz_i = 0 when b_i <= tol_zero, else b_i:
 *   decrease[k]    = min bz_i /   a_i  over a_i >  tol_pivot
 *   increase[k]    = min bz_i / (-a_i) over a_i < -tol_pivot
 *   *_row[k]       = among the ratios inside the tie band the row with the smallest leaving column; (+inf, -1) without a candidate
 * The basis stays primal feasible while rhs[row] stays within [rhs - decrease, rhs + increase]; *_row is the row that blocks.
 * decrease is the reference ratio test (RELP_RATIO_REFERENCE) of relp_select_primal_pivot_row on that column, whatever ratio_rule is
 * configured.  Measured at 10,000 x 10,000: profiles/r14_ranging.md, DESIGN.md 10. */
relp_status_t relp_row_ratios(relp_engine_t *h, const int32_t *rows, int32_t count, double *down_ratio, int32_t *down_column,
                              double *up_ratio, int32_t *up_column);
relp_status_t relp_rhs_ranging(relp_engine_t *h, const int32_t *rows, int32_t count, double *decrease, int32_t *decrease_row,
                               double *increase, int32_t *increase_row);
/* out4 = { relp_row_ratios calls so far, rows they covered, relp_rhs_ranging calls so far, pending rows p of the update block at
 * the last call of either }.  (Calls with count == 0 and refused calls are not counted.) */
relp_status_t relp_ranging_stats(const relp_engine_t *h, int64_t *out4);
/* Gomory cuts from rows of the tableau as it stands, in structural space, in the form relp_add_cuts takes (no counterpart in the
 * reference): relp_gomory_cuts -> relp_add_cuts -> relp_run_dual is one round of a cutting-plane loop.  Read-only and deterministic
 * like relp_row_ratios: nothing is flushed or re-tabulated, T0, R0, W, d, b, the basis, the flags, the PRICE partials, the record,
 * the trace, relp_reinversions and relp_tab_flush_stats keep their bits; no atomics, the same call on the same state gives the same
 * bits.  `rows` as in relp_row_ratios: engine rows in the current order, in any order, a row may be named twice.
 *
 * Entry k, r = rows[k], f0 = b_r - floor(b_r).  Over the non-basic provider columns j (flag != basic; a barred column counts like
 * any other; the kept artificial block is left out: those variables are 0 in every feasible point) the cut in provider space is
 * sum_j pi_j x_j >= f0, pi_j from the entry a = T[r,j] (T0 + W R0 over the pending rows, formed in the order of relp_row_ratios):
 *   |a| <= tol_zero                                    pi_j = 0
 *   integer column, f = a - floor(a)                   f <= tol_zero or f >= 1 - tol_zero: pi_j = 0
 *       RELP_GOMORY_FRACTIONAL                         pi_j = f
 *       RELP_GOMORY_MIXED                              pi_j = f if f <= f0, else (f0 (1 - f)) / (1 - f0)
 *   continuous column, RELP_GOMORY_MIXED               pi_j = a if a > 0, else (f0 (-a)) / (1 - f0)
 *   continuous column, RELP_GOMORY_FRACTIONAL          the entry is skipped (status 4)
 * every difference, product and quotient rounded once in the order written.  The virtual columns go out through their rows: with
 * row i written as (A x)_i [+ x_c in the bound row of c] + sigma_i s_i = rhs_i and y_i = sigma_i pi_{s_i},
 *   g_c  = -pi_c + sum_i y_i A[i,c] + y_{bound_row(c)}     i over the constraint rows and the cut rows already added
 *   beta = -f0 + sum_i y_i rhs_i                           i ascending over the rows with y_i != 0, one fma each from -f0
 * (the order of the sum in g_c: DESIGN.md 10).  coefficients[k,:] = g (count x structural columns, row-major), rhs[k] = beta:
 * the cut g'x <= beta, violated by the current vertex by f0.  fraction[k] = f0 (may be NULL).  is_integer: one flag per provider
 * column (relp_nr_columns() of them), NULL = all integer.  status[k]:
 *   0  a cut was made
 *   1  the basic column of row r is not flagged integer
 *   2  f0 < away or f0 > 1 - away                        (0 <= away < 0.5)
 *   3  the basic column of row r is a kept artificial
 *   4  a continuous column with |a| > tol_zero in a fractional cut
 * decided in the order 3, 1, 2, 4.  A skipped entry gets an all-zero coefficient row, rhs = 0 and fraction = f0.
 * Refusals leave nothing written.  RELP_E_ARG: a row out of range, count < 0, rows / coefficients / rhs / status missing, a kind
 * other than the two, away outside [0, 0.5) or not finite.  RELP_E_UNSUPPORTED: another or a sharded engine, an LP with range rows
 * (their virtual columns have two rows).  RELP_E_STATE: phase 1; added columns in the tableau (relp_add_cuts cannot hold a
 * coefficient on one).  count == 0 is a no-op.  Two launches, one download per call; f0 and the statuses 1 - 3 are decided on the
 * host from b and the basis.  Out of scope: range rows, cuts while added columns are present, sharded engines, lifting or
 * strengthening of the cuts, and any choice of which rows to cut (engine.gomory_rounds in Python has a simple rule). */
enum { RELP_GOMORY_FRACTIONAL = 0, RELP_GOMORY_MIXED = 1 };
relp_status_t relp_gomory_cuts(relp_engine_t *h, const int32_t *rows, int32_t count, const uint8_t *is_integer, int32_t kind,
                               double away, double *coefficients, double *rhs, double *fraction, int32_t *status);
/* out4 = { relp_gomory_cuts calls so far, list entries they covered, cuts made (status 0), pending rows p of the update block at
 * the last call }.  (Calls with count == 0 and refused calls are not counted.) */
relp_status_t relp_gomory_stats(const relp_engine_t *h, int64_t *out4);
/* A trial scope on the unsharded tableau engine in phase 2 (no counterpart in the reference): try something on the current basis,
 * look at the result, and come back.  Between two flushes the tableau is T = (I + W S') T0 and nothing a trial may call writes T0
 * over the rows and columns that exist, or a pending row of R0; so the way back is a copy of a few arrays of length m or n, the
 * pending columns of W and the record, not of the tableau (DESIGN.md 10 lists every array and why it is or is not saved).
 *
 * relp_trial_begin settles the fused update's shadow row, does NOT flush, and saves what a trial can change: on the device in one
 * launch of k_tab_trial_copy (RELP_TRIAL_MEMCPY=1 at create: the same copies as a chain of hipMemcpyAsync, the control), on the
 * host the layout (rhs, costs, cuts) and every counter.  Trials do not nest (RELP_E_STATE).
 * Inside a trial these work as usual: every getter but relp_get_basis_inverse (it flushes), the read-only queries (relp_row_ratios,
 * relp_rhs_ranging, relp_gomory_cuts, relp_generate_column, relp_relative_costs, relp_check_basis, ...), relp_change_right_hand_side,
 * relp_set_upper_bound, relp_change_cost, relp_add_cuts within the room that exists, relp_run_dual and relp_select_dual_pivot_row /
 * _column.  These return RELP_E_STATE with nothing changed -- they flush, rebuild, re-allocate or compact --: relp_flush,
 * relp_set_cost, relp_set_right_hand_side, relp_from_basis, relp_get_basis_inverse, relp_remove_cuts, relp_remove_columns,
 * relp_reserve_cuts, relp_reserve_columns, a relp_add_cuts that would have to grow, relp_add_columns,
 * relp_set_reinversion_interval, and relp_run, relp_solve_relaxation, relp_bring_into_basis (the primal loop's rescue and barring
 * state is not part of the snapshot).  relp_engine_destroy inside a trial is fine.
 * relp_run_dual inside a trial never flushes and never re-inverts (the interval and auto_reinversion are suspended; their counters
 * are part of the saved state): it pivots only while since_flush + 1 < update_block, since_flush counted in pivots made, so the
 * block is never left full.  When that room is used up the loop returns RELP_RUNNING with *iterations_done = the pivots made, and
 * relp_trial_stats reports 0 pivots of room.
 *
 * relp_trial_end(h, 0) restores the handle to the bit: every getter and every *_stats call returns exactly what it returned before
 * relp_trial_begin -- b, d, -obj, -pi, the basis, the flags, rhs, the costs, relp_nr_rows / relp_nr_columns, the trace with its
 * count, the iterations, the degenerate pivots, relp_cut_stats, relp_rhs_stats, relp_cost_stats, relp_ranging_stats,
 * relp_gomory_stats, relp_tab_flush_stats, relp_reinversions -- and every later call gives the bits it gives on a handle that never
 * opened the trial.  Only relp_trial_stats and the profile timers move.  The PRICE partials are marked invalid and the record is
 * re-armed, as the in-place calls do; the call synchronises.  What a cut added inside the trial left behind the old rows and
 * columns is unreachable once the counts are back; the room stays.
 * relp_trial_end(h, 1) drops the snapshot and leaves the state as it is; a pending re-inversion or a due flush happens at the next
 * loop, as usual.  RELP_E_STATE without an open trial; RELP_E_ARG for a keep other than 0 and 1.
 * All three: RELP_E_UNSUPPORTED on another or a sharded engine, RELP_E_STATE in phase 1.  Out of scope: trials on sharded or other
 * engines, the primal loop or relp_add_columns inside a trial, nested trials. */
relp_status_t relp_trial_begin(relp_engine_t *h);
relp_status_t relp_trial_end(relp_engine_t *h, int32_t keep);   /* 0: roll back, 1: keep */
/* out4 = { trials begun, trials rolled back, bytes the last snapshot held on the device, pivots the last trial could still have
 * made when it ended (0: relp_run_dual stopped, or would have stopped, for want of room) }. */
relp_status_t relp_trial_stats(const relp_engine_t *h, int64_t *out4);
/* Strong branching over the trial scope, host code over relp_trial_begin, relp_add_cuts, relp_run_dual and relp_trial_end: no kernel
 * of its own.  Entry k, r = rows[k], j = the basic column of row r, f0 = b_r - floor(b_r).  status[k], decided on the host from b
 * and the basis:
 *   0  evaluated
 *   1  j is not a structural column (j >= the structural columns, or a kept artificial)
 *   2  f0 < away or f0 > 1 - away                        (0 <= away < 0.5)
 * A skipped entry gets objective = NaN, outcome = -1, pivots = 0 in both slots.  An evaluated entry takes slot 2k for down and
 * 2k + 1 for up; each side is one trial: relp_trial_begin, relp_add_cuts of the single cut (down: x_j <= floor(b_r); up:
 * -x_j <= -ceil(b_r)), relp_run_dual(max_pivots), the objective exactly as relp_get_objective returns it, relp_trial_end(0).
 * outcome is RELP_OPTIMAL, RELP_INFEASIBLE (objective +inf) or RELP_RUNNING (the iteration limit); the dual objective is monotone,
 * so the objective of a RELP_RUNNING slot is still a valid bound on the child.  pivots = the dual pivots made.
 * Before the first trial, outside any trial, and only when some entry is evaluated: without room for one more cut the room is grown
 * as relp_add_cuts itself would grow it (to max(cuts + 1, twice the room, 16): relp_reserve_cuts); and if since_flush + max_pivots
 * + 1 > update_block (since_flush: the iterations the host has enqueued since the last flush) the open block is flushed once,
 * exactly as relp_flush does.  The call is otherwise read-only in the sense of relp_row_ratios: b, d, the basis, the flags, the
 * trace, every count and every *_stats but relp_trial_stats (two trials per evaluated entry) keep their bits.
 * Refusals leave nothing written.  RELP_E_ARG: a row out of range, count < 0, a missing array, max_pivots < 1 or
 * > update_block - 1, away outside [0, 0.5).  RELP_E_STATE: phase 1, an open trial, a basis that is not dual feasible (as
 * relp_run_dual).  RELP_E_UNSUPPORTED: another or a sharded engine.  count == 0 is a no-op.  Out of scope: a branch-and-bound
 * driver, and any choice of which rows to branch on. */
relp_status_t relp_strong_branch(relp_engine_t *h, const int32_t *rows, int32_t count, int32_t max_pivots, double away,
                                 double *objective /* 2*count */, int32_t *outcome /* 2*count */,
                                 int32_t *pivots /* 2*count */, int32_t *status /* count */);
/* A pool of candidate columns kept ON THE DEVICE, priced and added in place (no counterpart in the reference): the master problem
 * of a column-generation scheme (cutting stock, crew pairing, Dantzig-Wolfe) holds many candidate columns, prices all of them
 * every round and adds a handful.  The loop: relp_run, relp_pool_price, relp_pool_add of the winners, until nothing prices out.
 * Pricing needs no download of d and no host loop, and the add does not send the coefficients through the host again.
 * relp_pool_create: `count` columns x >= 0 in CSC over the engine rows in their current order, exactly the argument of
 * relp_add_columns, with its checks and refusals (RELP_E_ARG, no pool: count < 0, a missing array, a col_ptr that does not ascend
 * from 0, a row outside [0, relp_nr_rows()), a row named twice in one column, a coefficient or cost that is not finite).  Explicit
 * zeros are dropped, a column without entries is accepted, count == 0 gives an empty pool.  The pool is copied to the device as
 * sliced ELL -- 64 columns per slice, entry-major inside a slice, rows ascending inside a column, every slice padded to its longest
 * column -- and a host copy is kept for the layout and the later rebuilds.  The pool belongs to the handle: relp_pool_destroy frees
 * it, relp_engine_destroy frees the pools still alive; a handle may hold several.  A fresh pool has every column active.
 * Rows: the pool remembers rows_at_create = relp_nr_rows().  Cut rows added later (relp_add_cuts) have coefficient 0 in every pool
 * column, and removing such rows again (relp_remove_cuts of rows >= rows_at_create) leaves the pool valid.  A relp_remove_cuts that
 * takes out an engine row below rows_at_create makes the pool STALE: relp_pool_price, relp_pool_reduced_costs and relp_pool_add
 * then return RELP_E_STATE with nothing written (relp_last_error says why); destroy it and create a new one.  The rollback of a
 * trial takes rows out too: relp_trial_end(h, 0) takes back the cut rows added inside the trial, so a pool created INSIDE that trial
 * after such a cut (rows_at_create above the rows the rollback leaves) is stale from the rollback on, for good -- a cut added later
 * in the same place is another row.  Pools created before the trial, or inside it before its cuts, and every pool of a trial that is
 * kept (relp_trial_end(h, 1)) stay valid.  Pools are no part of a trial's snapshot: a pool created or destroyed inside a trial stays
 * created or destroyed, and activity flags set inside a trial (relp_pool_set_active) survive the rollback.
 * relp_pool_reduced_costs: out[k], for every pool column k, active or not,
 *     d_k = c_k + sum_i (-pi)_i * a_k[i]        (i ascending over the column's nonzero entries, ONE fma chain from c_k,
 *                                                (-pi)_i = d[idcol(i)] - cost_store[idcol(i)] rounded once: relp_get_minus_pi)
 * which is the arithmetic relp_add_columns uses for d[new_k]: d_k has the bits the column's reduced cost would have after
 * relp_add_columns at this moment.  Read-only in the sense of relp_row_ratios: nothing is flushed, and T0, R0, W, d, b, the basis,
 * the flags, the PRICE partials, the record, the trace and every other *_stats keep their bits.  Neither dual nor primal
 * feasibility is required; allowed inside a trial.  No atomics: the same call on the same state gives the same bits.
 * relp_pool_price: multiple pricing.  The pool indices [0, count) are cut into `segments` equal shares of ceil(count / segments)
 * columns (the last shares may be short or empty; 1 <= segments <= count).  The winner of a share is its ACTIVE column with the
 * smallest d_k among those with d_k < -tol (tol >= 0, finite; d_k == -tol is no candidate), the lowest pool index among equal
 * d_k.  ids_out and d_out (room for `segments` entries each) receive the winners in ascending share order, compacted; *found is
 * their number.  segments = 1: the most negative column; segments = count: every candidate.  The d are the bits of
 * relp_pool_reduced_costs.  The winners are picked on the device and come down in one copy (beyond 4,096 segments: their number
 * first, then the winners alone); the d vector never crosses the bus.  Read-only as above, allowed inside a trial.  RELP_E_ARG with
 * nothing written: segments out of range, a tol that is negative or not finite, a missing array.  A pool without columns gives
 * *found = 0 for any segments >= 1.  Priced in chunks of 256 columns per workgroup and share: meant for shares of hundreds of
 * columns or more (segments = count works and launches a workgroup per column).
 * relp_pool_set_active: the activity flag (0 or 1) of the listed pool columns, on the device.  RELP_E_ARG: an index outside the
 * pool, an index named twice, another flag value, count < 0, a missing list.  Works on a stale pool too.
 * relp_pool_add: the pool columns ids[0 .. count) (each once, any order) join the tableau exactly as relp_add_columns would add the
 * same columns in the same order: column k becomes provider column relp_nr_columns() + k, non-basic, with the growth rule, the
 * flags, the relp_column_stats bookkeeping and the inclusion in later rebuilds of relp_add_columns, and RELP_E_STATE inside a
 * trial.  The activity flags of the added columns are cleared.  The bit contract: after the call every getter and every *_stats
 * but relp_pool_stats returns exactly what it returns on a twin handle that called relp_add_columns with the host data of the same
 * columns.  The operands of the add -- the ascending union list of identity columns of the touched rows, coef[entry][column],
 * d[new], the costs and the columns' rows of the re-tabulation block -- are formed on the device from the device copy; the
 * coefficient values are not uploaded again.  RELP_POOL_HOST_ADD=1 at relp_engine_create routes the call through relp_add_columns
 * with the host copy (the control: the same bits).  RELP_E_ARG with nothing changed: an index outside the pool or named twice,
 * count < 0, a missing list, more than 524,280 columns in one call.  count == 0 is a no-op.  RELP_E_HIP from this call means, as
 * after a failed launch of a pivot, that the device may hold columns the layout does not: the handle is unusable (this includes the
 * call's own cross-check of the device's union list against the host's, which cannot fail while the device copy is intact).  relp_remove_columns does not know the
 * pool: a caller who takes an added column out again re-activates it with relp_pool_set_active.
 * relp_pool_stats: out4 = { pool columns, nonzeros held (explicit zeros dropped), entries stored on the device (padding included),
 * relp_pool_price calls so far (calls that returned RELP_OK; refused and failed ones are not counted) }.
 * All seven: RELP_ENGINE_TABLEAU, unsharded, phase 2 -- RELP_E_UNSUPPORTED on another or a sharded engine, RELP_E_STATE in
 * phase 1 -- and RELP_E_ARG for a pool that is not one of this handle's.  Out of scope: pools on sharded or other engines, pricing
 * in phase 1, pools whose row space follows row removals, automatic re-activation on relp_remove_columns, changing the cost of a
 * pool column. */
typedef struct relp_pool relp_pool_t;
relp_status_t relp_pool_create(relp_engine_t *h, int32_t count, const int64_t *col_ptr, const int32_t *row_idx, const double *values,
                               const double *cost, relp_pool_t **pool);
relp_status_t relp_pool_destroy(relp_engine_t *h, relp_pool_t *pool);
relp_status_t relp_pool_set_active(relp_engine_t *h, relp_pool_t *pool, const int32_t *ids, int32_t count, int32_t flag);
relp_status_t relp_pool_reduced_costs(relp_engine_t *h, relp_pool_t *pool, double *out_count);
relp_status_t relp_pool_price(relp_engine_t *h, relp_pool_t *pool, int32_t segments, double tol, int32_t *ids_out /* segments */,
                              double *d_out /* segments */, int32_t *found);
relp_status_t relp_pool_add(relp_engine_t *h, relp_pool_t *pool, const int32_t *ids, int32_t count);
relp_status_t relp_pool_stats(const relp_engine_t *h, const relp_pool_t *pool, int64_t *out4);
/* A pool of candidate CUTS kept ON THE DEVICE, separated and added in place (no counterpart in the reference): the mirror image of
 * the column pool above, for row generation -- lazy constraints, a model with far more rows than are ever binding, cuts kept from
 * earlier rounds or nodes, Gomory cuts set aside.  The loop: relp_run_dual, relp_cutpool_separate, relp_cutpool_add of the winners,
 * until nothing is violated.  Separation needs no download of b and the basis and no host loop, and the add does not send the
 * coefficients through the host again.
 * relp_cutpool_create: `count` cuts g_k' x <= rhs_k in CSR over the structural columns [0, nr_normal), exactly the argument of
 * relp_add_cuts, with its checks and refusals (RELP_E_ARG, no pool: count < 0, a missing array, a row_ptr that does not ascend from
 * 0, a column that is not structural, a column named twice in one cut, a coefficient or right-hand side that is not finite).
 * Explicit zeros are dropped, a cut without entries is accepted, count == 0 gives an empty pool.  The pool is copied to the device
 * as sliced ELL -- 64 cuts per slice, entry-major inside a slice, columns ascending inside a cut, every slice padded to its longest
 * cut with (column -1, value 0.0), skipped by its column -- with rhs_k and norm_k per cut; norm_k is the square root of ONE fma chain
 * of squares from 0.0 over the stored entries in ascending column order, computed on the host at the create.  A host copy is kept
 * for the layout and the later rebuilds.  The pool belongs to the handle: relp_cutpool_destroy frees it, relp_engine_destroy frees
 * the pools still alive; a handle may hold several, next to column pools.  A fresh pool has every cut active.  There is NO stale
 * rule: the structural columns never move -- added columns (relp_add_columns) lie behind them, and cuts with coefficients on added
 * columns are out of scope -- so a cut pool stays valid through every add and removal of rows and columns.
 * relp_cutpool_slacks: out[k], for every pool cut k, active or not,
 *     s_k = rhs_k - acc,   acc = fma(g_kj, x_j, acc) from 0.0 over the cut's stored entries, j ascending, every operand rounded once,
 *     x_j = b[r] if structural column j is basic in row r, else +0.0:
 * the slack the cut would have at the current vertex; s_k < 0 means the cut is violated.  This is the call's own fixed arithmetic.
 * It equals the b of the new row that relp_add_cuts would produce at this moment UP TO SUMMATION ORDER -- relp_add_cuts walks the
 * tableau rows ascending, this call the columns -- and equals it to the bit whenever ascending columns and ascending rows give the
 * cut's entries the same order.  Read-only in the sense of relp_pool_reduced_costs: nothing is flushed or re-armed, the record is
 * not downloaded, and T0, R0, W, d, b, the basis, the flags, the record, the trace and every other *_stats keep their bits.
 * Neither primal nor dual feasibility is required; allowed inside a trial.  No atomics: the same call on the same state gives the
 * same bits.
 * relp_cutpool_separate: the pool indices [0, count) are cut into `segments` equal shares of ceil(count / segments) cuts (the last
 * shares may be short or empty; 1 <= segments <= count).  The winner of a share is its ACTIVE cut with the smallest key among those
 * with s_k < -tol (tol >= 0, finite; s_k == -tol is no candidate).  The key is s_k when by_efficacy is 0 and s_k / norm_k when it
 * is 1 (a cut with norm_k == 0 ranks with norm 1); the lowest pool index wins among equal keys.  ids_out and slack_out (room for
 * `segments` entries each) receive the winners in ascending share order, compacted; *found is their number; slack_out[i] has the
 * bits of relp_cutpool_slacks()[ids_out[i]].  The winners are picked on the device and come down in one copy (beyond 4,096
 * segments: their number first, then the winners alone).  Read-only as above, allowed inside a trial.  RELP_E_ARG with nothing
 * written: segments out of range, a tol that is negative or not finite, by_efficacy outside {0, 1}, a missing array.  A pool
 * without cuts gives *found = 0 for any segments >= 1.
 * relp_cutpool_set_active: the activity flag (0 or 1) of the listed pool cuts, on the device.  RELP_E_ARG: an index outside the
 * pool, an index named twice, another flag value, count < 0, a missing list.
 * relp_cutpool_add: the pool cuts ids[0 .. count) (each once, any order) join the tableau exactly as relp_add_cuts would add the
 * same cuts in the same order: cut k becomes row relp_nr_rows() + k with its slack basic in it, with the growth rule, the room
 * rule inside a trial (allowed within the reserved room, RELP_E_STATE when the tableau would have to grow), the relp_cut_stats
 * bookkeeping and the inclusion in later rebuilds of relp_add_cuts.  The activity flags of the added cuts are cleared.  The bit
 * contract: after the call every getter and every *_stats but relp_cutpool_stats returns exactly what it returns on a twin handle
 * that called relp_add_cuts with the host data of the same cuts.  The operands of the add -- the ascending union list of rows
 * whose basic column is structural and touched by a chosen cut, coef[entry][cut], the cut rows of the engine's matrix and b of the
 * new rows -- are formed on the device from the device copy; the coefficient values, b and the basis do not cross the bus.  Four
 * bytes do: the length of the union list comes down between the operands and the row kernels, because which touched columns are
 * basic only the device knows; it is checked there against the host's bound, before the tableau is written.
 * RELP_CUTPOOL_HOST_ADD=1 at relp_engine_create routes the call through relp_add_cuts with the host copy (the control: the same
 * bits).  RELP_E_ARG with nothing changed: an index outside the pool or named twice, count < 0, a missing list.  count == 0 is a
 * no-op.  Pools are no part of a trial's snapshot: a pool created or destroyed inside a trial stays created or destroyed, and the
 * flags cleared by an add inside a trial STAY cleared after relp_trial_end(h, 0), although the rows are gone -- the caller
 * re-activates them with relp_cutpool_set_active.  relp_remove_cuts does not know the pool either.
 * relp_cutpool_stats: out4 = { pool cuts, nonzeros held (explicit zeros dropped), entries stored on the device (padding included),
 * relp_cutpool_separate calls so far (calls that returned RELP_OK; refused and failed ones are not counted) }.
 * All seven: RELP_ENGINE_TABLEAU, unsharded, phase 2 -- RELP_E_UNSUPPORTED on another or a sharded engine, RELP_E_STATE in
 * phase 1 -- and RELP_E_ARG for a pool that is not one of this handle's.  Out of scope: pools on sharded or other engines or in
 * phase 1, cuts with coefficients on added or virtual columns, moving slack-basic pool cuts back into the pool, restoring the
 * flags at a rollback, parallelism and orthogonality filtering between chosen cuts. */
typedef struct relp_cutpool relp_cutpool_t;
relp_status_t relp_cutpool_create(relp_engine_t *h, int32_t count, const int64_t *row_ptr, const int32_t *col_idx, const double *values,
                                  const double *rhs, relp_cutpool_t **pool);
relp_status_t relp_cutpool_destroy(relp_engine_t *h, relp_cutpool_t *pool);
relp_status_t relp_cutpool_set_active(relp_engine_t *h, relp_cutpool_t *pool, const int32_t *ids, int32_t count, int32_t flag);
relp_status_t relp_cutpool_slacks(relp_engine_t *h, relp_cutpool_t *pool, double *out_count);
relp_status_t relp_cutpool_separate(relp_engine_t *h, relp_cutpool_t *pool, int32_t segments, double tol, int32_t by_efficacy,
                                    int32_t *ids_out /* segments */, double *slack_out /* segments */, int32_t *found);
relp_status_t relp_cutpool_add(relp_engine_t *h, relp_cutpool_t *pool, const int32_t *ids, int32_t count);
relp_status_t relp_cutpool_stats(const relp_engine_t *h, const relp_cutpool_t *pool, int64_t *out4);
/* InverseMaintener::from_basis (carry/mod.rs:428-463): warm start from provider column indices,
 * one per row; switches to phase 2.  RELP_ENGINE_LU: any basis (factorise, b = FTRAN(rhs), -pi = BTRAN(-c_B));
 * RELP_ENGINE_REVISED: any basis (basis_inverse_rows.rs:103-129: LU - factorised on the host like every
 * refactorisation - then m unit solves, b and -pi on the device; slack bases are a signed permutation and take a
 * shortcut); RELP_ENGINE_TABLEAU (unsharded): any basis -- the tableau B^-1 [A | I] is re-tabulated column by column from the
 * factors, then b, the reduced costs and -obj (tests/cpp/test_tableau.cpp, tests/test_gpu_parity.py::test_from_basis_*).
 * "Any basis" holds at any m on both dense engines: the m unit solves / the solves of the stored columns keep their work
 * vector in LDS up to m = 9,984 and in a slab of global memory per workgroup beyond (relp_retab_stats;
 * tests/test_gpu_retab_any_m.py).  RELP_E_SINGULAR: a column twice, or a basis the factorisation declines. */
relp_status_t relp_from_basis(relp_engine_t *h, const int32_t *basis_columns_m);
/* RELP_ENGINE_REVISED and RELP_ENGINE_TABLEAU (unsharded), an f64 matter (the exact reference never needs it,
 * `should_refactor() = false`, basis_inverse_rows.rs:175-179): every `pivots` basis changes inside relp_run the state is
 * rebuilt from the columns of the current basis -- host LU, then on the device B^-1 row by row (revised) or the tableau
 * B^-1 [A | I] column by column (tableau), b = B^-1 rhs, -pi / the reduced costs and -obj -- which bounds the error of a
 * representation that is otherwise only ever updated.  Default: 1,000 for sparse input (CSC, at most 10 % nonzeros)
 * with at most 4,096 rows -- where the host factorisation of a basis is cheap -- else 0 = never.  An interval set by hand
 * (and relp_config_t.auto_reinversion) works at any m: beyond m = 9,984 the solves of a rebuild keep their work vector in
 * global memory instead of LDS (relp_retab_stats).
 * relp_reinversions: how many have been done. */
relp_status_t relp_set_reinversion_interval(relp_engine_t *h, int64_t pivots);
int64_t       relp_reinversions(const relp_engine_t *h);
/* Fold every pending deferred update into the stored representation: B0^-1 += W (S' B0^-1) (revised), T0 += W R0
 * (tableau), refactorisation (LU).  No-op when update_block = 0. */
relp_status_t relp_flush(relp_engine_t *h);
/* Tableau engine: out2 = { flushes that folded pending pivots, columns they rewrote } since create.  A flush rewrites the
 * owned columns with a nonzero entry among the pending rows R0 (the others have T0 + W R0 = T0), or every owned column
 * when RELP_TAB_FLUSH_ALL=1 was set at create.  Other engines: { 0, 0 }. */
relp_status_t relp_tab_flush_stats(relp_engine_t *h, int64_t *out2);
/* Revised and tableau engines: the batch solves of the rebuilds so far (relp_from_basis, re-inversion, re-tabulation: all m
 * rows of B^-1, or every stored column of the tableau, in one launch).  out4 = { batch solves with the work vector in LDS (one
 * workgroup per right-hand side, m <= 9,984), batch solves with it in a slab of global memory per workgroup (larger m, or
 * RELP_RETAB_GLOBAL=1 at create), workgroups of the last launch of the second kind (at most two per CU, at most 256 MiB of
 * slabs, at most RELP_RETAB_GROUPS when that was set at create), bytes of the slab buffer }.  Other engines: zeros. */
relp_status_t relp_retab_stats(const relp_engine_t *h, int64_t *out4);
/* Tableau engine: how many of the p pending rows of an update block the per-pivot kernels load per memory round trip:
 * RELP_TAB_LOAD_BATCH at create if it was 1 (one by one), 8, 16 or 32, else the default.  Other engines: 0. */
int32_t       relp_tab_load_batch(const relp_engine_t *h);
/* Tableau engine: the rows one workgroup of the column kernel walks in the fused single-GPU loop (every other path: 256):
 * RELP_TAB_COLUMN_ROWS at create if it was 256 (the control), 128 or 64; else 256 when the update block is above 64 pivots, and
 * relp_tab_column_rows_for(0, m) for the m rows the tableau has at the call.  Other engines: 0. */
int32_t       relp_tab_column_rows(const relp_engine_t *h);
/* The choice itself (host code, no device): `wanted` if it is 256, 128 or 64, else the smallest of them with at most 256
 * workgroups over m rows. */
int32_t       relp_tab_column_rows_for(int32_t wanted, int32_t m);
/* The block size K in effect (0 = explicit rank-1 updates; LU engine: pivots between refactorisations). */
int32_t       relp_update_block(const relp_engine_t *h);
/* RELP_ENGINE_LU only: statistics of the current factorisation, out[8] = { refactorisations so far, m,
 * nnz(L) (off-diagonal), nnz(U) (with diagonal), levels of the four solve schedules L, U (FTRAN) and
 * U', L' (BTRAN) }.  Levels bound the length of the dependent chain of a triangular solve. */
relp_status_t relp_lu_stats(const relp_engine_t *h, int64_t *out8);
/* RELP_ENGINE_LU: the look-ahead refactorisation (a refactorisation prepared on the host while the pivot kernel keeps
 * going on the old factors; carry/mod.rs:602-614 refactorises synchronously): out[4] = { look-ahead factorisations
 * installed, basis changes replayed onto them, the look-ahead length in effect (RELP_LU_LOOKAHEAD, 0 = off), the lane
 * budget of a fused group of levels (RELP_FUSE_LANES) }; both switches are read when the engine is created. */
relp_status_t relp_lu_lookahead_stats(const relp_engine_t *h, int64_t *out4);
/* RELP_ENGINE_LU: how the pivot loop runs.  out[4] = { persistent pivot kernel in use (0: the product-form fallback, one launch
 * per step), its layout (0: work vectors, eta file and permutations in one CU's LDS; 1: x, -pi and the slot tables in LDS, the
 * rest in L2; 2: nothing per row in LDS, any m), slots of the dense tail of U (= the longest refactorisation interval), PRICE as
 * a grid launch per pivot (Dantzig's rule over >= 32,768 columns in layout 2; RELP_FT_GRID_PRICE) }.  RELP_FT_BIG = 0 / 1 / 2
 * forces that layout at create: when the forced layout does not fit, no other layout is tried and the engine runs the
 * product-form fallback (out[0] = 0) -- bench.py's `lu_product_form_fallback` leg relies on exactly that. */
relp_status_t relp_lu_kernel_layout(const relp_engine_t *h, int32_t *out4);
/* RELP_ENGINE_LU: refactorise ON THE DEVICE (LUDecomposition::invert -> decomposition/mod.rs:27-138 with the Markowitz
 * pivoting of decomposition/pivoting.rs:45-81): singleton rows / columns peeled in parallel rounds, the bump eliminated on
 * a dense working copy by one workgroup, L and U read off afterwards -- no basis download, no search on the host.  Off by
 * default (the host factorisation behind the look-ahead is faster at Netlib sizes); RELP_LU_DEVICE_FACTOR=1
 * switches it on at create.  A bump beyond the working copy (RELP_LUF_BUMP_CAP, 2,048) is factorised on the host.
 * stats: out[6] = { enabled, device factorisations, fallbacks to the host, microseconds spent in the kernel so far,
 * bump size and number of peeled singleton pivots of the last factorisation }. */
relp_status_t relp_lu_set_device_factorisation(relp_engine_t *h, int32_t on);
relp_status_t relp_lu_device_factorisation_stats(const relp_engine_t *h, int64_t *out6);
/* max |P B Q - L U| over all entries for the factors in use and the current basis (decomposition/mod.rs:301-491 asserts
 * the factors themselves; pivot orders differ, the identity is what they have in common).  Dense arithmetic on the host:
 * m <= 1,024, else *out = -1.  The factors describe the basis of the last refactorisation: with Forrest-Tomlin updates
 * pending the comparison would be against another basis, and *out = -1 as well (call it right after relp_from_basis /
 * a refactorisation). */
relp_status_t relp_lu_factor_residual(relp_engine_t *h, double *out);

/* RELP_ENGINE_LU in Forrest-Tomlin mode: shader clocks spent per phase of the pivot inside the persistent kernel since create
 * (thread 0): out[16] = { PRICE, entering-column scatter, L solve, eta file forward, spike push, U solve, ratio test, b update,
 * u_bar extraction, U' solve for r, compaction of r and the spike, eta file backward, L' solve, -pi / basis, state load + store,
 * 0 }.  Measurement aid for profiles/ and DESIGN.md. */
relp_status_t relp_lu_phase_cycles(relp_engine_t *h, int64_t *out16);

/* ---- the `BasisInverse` surface (carry/mod.rs:68-157) beside the tableau-level calls above ------------------------
 * BasisInverse::basis_inverse_row(row) (carry/mod.rs:145-150): row `row` of B^-1, dense, m entries.  LU engine: one BTRAN
 * of e_row (lower_upper/mod.rs:204-222); revised engine: a copy of the stored row (basis_inverse_rows.rs:181-183);
 * tableau engine: row `row` of the tableau over the columns that were the identity. */
relp_status_t relp_basis_inverse_row(relp_engine_t *h, int32_t row, double *out_m);
/* BasisInverse::should_refactor (carry/mod.rs:138-143).  LU engine: 1 when as many updates are pending as
 * relp_config_t.update_block allows (lower_upper/mod.rs:199-202 refactors when updates.len() > 10: update_block = 11) or the
 * eta pool is exhausted; relp_run / relp_bring_into_basis refactor by themselves (Carry::after_basis_change,
 * carry/mod.rs:602-614).  Revised and tableau engine: always 0 (basis_inverse_rows.rs:175-179). */
relp_status_t relp_should_refactor(relp_engine_t *h, int32_t *out);
/* BasisInverse::generate_column(original_column) (carry/mod.rs:108-118) for a column the caller supplies as sorted
 * (row, value) pairs over the m tableau rows -- the reference's signature, where relp_generate_column takes a column
 * index of the provider.  The result also becomes the "last generated column" (relp_select_primal_pivot_row,
 * relp_lu_change_basis).  Tableau engine: computed on the host from B^-1 read off the tableau. */
relp_status_t relp_generate_column_of(relp_engine_t *h, const int32_t *row_idx, const double *values, int32_t nnz, double *out_m);
/* InverseMaintener::cost_difference(column) (carry/mod.rs:572-577): (-pi) . column */
relp_status_t relp_cost_difference_of(relp_engine_t *h, const int32_t *row_idx, const double *values, int32_t nnz, double *out);
/* BasisInverse::change_basis(pivot_row_index, column) on the inverse alone (lower_upper/mod.rs:92-155): the Forrest-Tomlin
 * update with the column (and spike, mod.rs:378-381) of the last relp_generate_column / relp_generate_column_of.  b, -pi and
 * the basis indices are NOT touched (that is Carry::change_basis = relp_bring_into_basis).  LU engine only. */
relp_status_t relp_lu_change_basis(relp_engine_t *h, int32_t pivot_row_index);
/* `LUDecomposition { row_permutation: identity, column_permutation: identity, lower_triangular, upper_triangular, updates: [] }`
 * given literally (lower_upper/mod.rs:33-57), the way the reference's tests construct their starting points: L column-major
 * with the unit diagonal implied, U column-major with its diagonal; CSC arrays of m columns each. */
relp_status_t relp_lu_set_factors(relp_engine_t *h, const int64_t *l_col_ptr, const int32_t *l_row_idx, const double *l_values,
                                  const int64_t *u_col_ptr, const int32_t *u_row_idx, const double *u_values);
/* The update file in the reference's coordinates: `updates.len()`; `updates[k]` = (EtaFile { values, pivot, len },
 * RotateToBack { index: pivot }) with positions as they were before that rotation (eta_file.rs:14-18, mod.rs:56);
 * `upper_triangular` after every update so far: column-major, rows sorted, diagonal last in its column (mod.rs:48-52). */
relp_status_t relp_lu_updates(relp_engine_t *h, int32_t *count);
relp_status_t relp_lu_get_update(relp_engine_t *h, int32_t k, int32_t *pivot, int32_t *idx, double *values, int32_t cap, int32_t *nnz);
relp_status_t relp_lu_get_upper(relp_engine_t *h, int64_t *col_ptr_m1, int32_t *row_idx, double *values, int64_t cap, int64_t *nnz);

/* ---- state getters (InverseMaintener accessors, inverse_maintenance/mod.rs:200-266) ----------- */
int32_t relp_nr_rows(const relp_engine_t *h);
int32_t relp_nr_columns(const relp_engine_t *h);
int32_t relp_phase(const relp_engine_t *h);                 /* 1 or 2 */
int32_t relp_nr_artificial(const relp_engine_t *h);
relp_status_t relp_get_objective(relp_engine_t *h, double *out);        /* get_objective_function_value */
relp_status_t relp_get_b(relp_engine_t *h, double *out_m);              /* b() */
relp_status_t relp_get_minus_pi(relp_engine_t *h, double *out_m);
relp_status_t relp_get_basis_indices(relp_engine_t *h, int32_t *out_m); /* basis_column_index_for_row */
relp_status_t relp_get_basis_inverse(relp_engine_t *h, double *out_mm); /* dense row-major B^-1 */
/* current_bfs (carry/mod.rs:616-625): (column, value) pairs sorted by column, zeros dropped. */
relp_status_t relp_current_bfs(relp_engine_t *h, int32_t *cols, double *vals, int32_t cap, int32_t *count);
relp_status_t relp_get_iterations(relp_engine_t *h, int64_t *out);
/* how many of those pivots were degenerate: ratio b_r / alpha_r exactly 0, the basis changed but b did not */
relp_status_t relp_get_degenerate_pivots(relp_engine_t *h, int64_t *out);
/* recorded pivots: phase, entering, row, leaving (each `cap` long); count = pivots so far */
relp_status_t relp_get_trace(relp_engine_t *h, int32_t *phase, int32_t *entering, int32_t *row,
                             int32_t *leaving, int64_t cap, int64_t *count);
/* Debug invariant checker (tableau/mod.rs:253-289): max |B^-1 B - I|, max |d_basic|, min b. */
relp_status_t relp_check_basis(relp_engine_t *h, double *max_identity_error, double *max_basic_cost,
                               double *min_b);

/* ---- per-kernel timing (bench.py roofline) ------------------------------------------------------ */
typedef enum {
    RELP_K_PRICE = 0, RELP_K_SELECT_COLUMN = 1, RELP_K_BUILD_COLUMN = 2, RELP_K_FTRAN = 3,
    RELP_K_RATIO = 4, RELP_K_UPDATE_VECTORS = 5, RELP_K_UPDATE_INVERSE = 6,
    RELP_K_APPLY_W = 7,          /* deferred update: alpha = v + W (S'v) */
    RELP_K_UPDATE_W = 8,         /* deferred update: W <- E W, pivot row rho */
    RELP_K_FLUSH = 9,            /* deferred update: B0inv += W (S' B0inv); LU engine: refactorisation */
    RELP_K_FT_RUN = 10,          /* LU engine: the persistent pivot kernel (many pivots per launch) */
    RELP_K_COUNT = 11
} relp_kernel_id_t;
/* When enabled, the kernel classes of every `sample_every`-th pivot inside relp_run are bracketed by
 * HIP events on the engine's stream (an event pair costs ~4 us of stream time, so bracketing every
 * launch would slow a 330 us pivot by 15 %); relp_profile_read sums them (this synchronises). */
relp_status_t relp_profile_enable(relp_engine_t *h, int32_t enable, int64_t max_launches, int32_t sample_every);
relp_status_t relp_profile_read(relp_engine_t *h, int32_t kernel_id, int64_t *launches, double *total_ms);

/* ---- synthetic workloads (bench / tests; rust-lp_amd/synthetic.py defines the numbers) ----------
 * Fills a column-major m x n matrix on the device with A[i,j] = (1 + x(0, j*m+i) % 999) / 1000. */
relp_status_t relp_synth_fill_dense(double *device_a, int64_t ld, int32_t m, int32_t n, uint64_t seed,
                                    int64_t first_column, void *hip_stream);
relp_status_t relp_device_alloc(void **out, int64_t bytes);
relp_status_t relp_device_free(void *p);

/* ---- multi-GPU shards: structural columns [col_lo, col_hi) and rows
 * [row_lo, row_hi) of B^-1 live on this rank; b, -pi, basis are replicated.  Buffers are device
 * pointers the caller exchanges with RCCL on the engine's stream; no host sync inside. ----------- */
relp_status_t relp_shard_ranges(const relp_engine_t *h, int32_t *col_lo, int32_t *col_hi,
                                int32_t *row_lo, int32_t *row_hi, int32_t *row_slice_stride);
/* columns [lo, hi) of the structural block owned by `rank` of `count` (what relp_engine_create
 * expects in `dense` when cfg.shard_count > 1) */
void          relp_shard_column_range(int32_t nr_normal, int32_t rank, int32_t count, int32_t *lo, int32_t *hi);
/* message length in doubles of one PRICE candidate: [key, j, d_j, a_j (m entries, tableau row space)]; the
 * tableau engine appends the minimum ratio b_i / alpha_i of every block of 256 rows (the receiver's ratio test
 * starts from those) */
int64_t       relp_shard_candidate_len(const relp_engine_t *h);
/* length in doubles of the rho buffer (m rounded up to the B^-1 row pitch) */
int64_t       relp_shard_rho_len(const relp_engine_t *h);
/* local PRICE over the owned columns (+ every virtual column) -> candidate message */
relp_status_t relp_shard_price(relp_engine_t *h, double *dev_candidate);
/* choose the global entering column from `count` gathered candidates (min d, then min j) */
relp_status_t relp_shard_select_column(relp_engine_t *h, const double *dev_candidates, int32_t count);
/* FTRAN slice: alpha[row_lo:row_hi) into dev_alpha_slice (row_slice_stride entries, zero padded) */
relp_status_t relp_shard_ftran(relp_engine_t *h, double *dev_alpha_slice);
/* ratio test on the gathered alpha (count slices of row_slice_stride); the owner of the pivot row
 * writes rho = row_r(B^-1)/alpha_r into dev_rho (m entries), every other rank writes zeros, so a
 * SUM all-reduce of dev_rho is the broadcast */
relp_status_t relp_shard_ratio(relp_engine_t *h, const double *dev_alpha_slices, int32_t count, double *dev_rho);
/* rank-1 update of the owned rows + replicated b, -pi, obj, basis */
relp_status_t relp_shard_update(relp_engine_t *h, const double *dev_rho);
/* structural columns [lo, hi) that rank cfg->shard_rank must supply in `dense` for this problem and
 * engine kind (only the counts and upper bounds of `md` are read).  The revised engine splits the
 * structural columns; the tableau engine splits its stored columns [artificial | structural | virtual]. */
relp_status_t relp_shard_plan(const relp_matrix_data_t *md, const relp_config_t *cfg, int32_t *col_lo, int32_t *col_hi);
/* Tableau engine only: the whole pivot after relp_shard_select_column (ratio test, row update of the
 * owned columns, W / b / basis update, local flush when due).  One all-gather per pivot in total. */
relp_status_t relp_shard_pivot(relp_engine_t *h);
/* deferred update in sharded mode, every relp_update_block() pivots: `begin` snapshots the rows
 * S' B0inv this rank owns (zeros elsewhere) and returns the buffer to SUM all-reduce in place
 * (*len_doubles = 0: nothing pending); `end` applies W (S' B0inv) to the owned rows. */
relp_status_t relp_shard_flush_begin(relp_engine_t *h, double **dev_snapshot, int64_t *len_doubles);
relp_status_t relp_shard_flush_end(relp_engine_t *h);
/* outcome poll (one small device->host copy) */
relp_status_t relp_poll(relp_engine_t *h, int32_t *outcome, int64_t *iterations);

/* ---- native multi-GPU loop: the same per-pivot sequence as above, enqueued by the library itself with the
 * collectives called through two hooks between its kernels, on the engine's stream (no Python and no host
 * sync inside a pivot; the host polls the outcome every cfg.poll_interval pivots like relp_run).  The hooks
 * return 0 on success. */
typedef int (*relp_allgather_fn)(void *ctx, const void *dev_send, void *dev_recv, int64_t bytes_per_rank, void *hip_stream);
typedef int (*relp_allreduce_sum_fn)(void *ctx, double *dev_buf, int64_t count, void *hip_stream);
relp_status_t relp_shard_set_collectives(relp_engine_t *h, relp_allgather_fn allgather, relp_allreduce_sum_fn allreduce_sum,
                                         void *ctx);
/* phase_one::primal / phase_two::primal across ranks: up to max_iters basis changes of the current phase.  Every
 * rank must call it with the same arguments; every rank takes the same decisions from the same gathered data,
 * so *done and *outcome agree on all ranks. */
relp_status_t relp_shard_run(relp_engine_t *h, int64_t max_iters, int64_t *done, int32_t *outcome);
/* Failure agreement: a rank whose step fails locally (anything but a collective) keeps the collectives of the current chunk
 * going and reports at the next poll, where one 16-byte all-gather of the statuses makes every rank return the same error:
 * nobody is left waiting inside a collective.  relp_shard_inject_failure is the test hook for exactly that: this engine's
 * relp_shard_run fails locally after `after_pivots` further pivots. */
relp_status_t relp_shard_inject_failure(relp_engine_t *h, int64_t after_pivots);
/* RCCL as the collectives: rank 0 makes a unique id (ncclGetUniqueId, 128 bytes), the caller hands it to every
 * rank (any channel; bench.py broadcasts it with torch.distributed), and each rank attaches a communicator of
 * cfg.shard_count ranks on the engine's device (ncclCommInitRank), which installs ncclAllGather / ncclAllReduce
 * as the hooks.  librccl.so.1 is taken from the process if already loaded (PyTorch ships one), else dlopen'ed.
 * RELP_E_UNSUPPORTED when no RCCL library can be loaded. */
#define RELP_RCCL_ID_BYTES 128
relp_status_t relp_rccl_unique_id(uint8_t id[RELP_RCCL_ID_BYTES]);
relp_status_t relp_rccl_attach(relp_engine_t *h, const uint8_t id[RELP_RCCL_ID_BYTES]);

#ifdef __cplusplus
}
#endif
#endif /* RELP_ENGINE_H */
