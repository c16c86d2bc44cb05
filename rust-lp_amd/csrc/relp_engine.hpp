// relp_engine.hpp -- host driver of the three pivot engines: revised (explicit B^-1, deferred updates), dense tableau
// (T = B^-1 [A | I] in blocks) and sparse LU (product form, or Forrest-Tomlin in one persistent workgroup).
//
// `Engine` plays the role of the reference's `Tableau<Carry<f64, BasisInverseRows<f64>>, K>` plus
// the `PivotRule` state and the `MatrixData` provider (file:line under
// /root/reference/src/algorithm/two_phase/):
//   MatrixData columns/rows          matrix_provider/matrix_data.rs:198-268, 308-371, 432-452
//   Partially / NonArtificial kinds  tableau/kind/artificial/partially.rs:125-206, kind/non_artificial.rs:151-220
//   Carry constructors / updates     tableau/inverse_maintenance/carry/mod.rs:214-271, 283-333, 381-426, 484-570
//   phase loops                      phase_one.rs:125-170, 223-260; phase_two.rs:22-51; two_phase/mod.rs:30-76
// All numeric state lives in HBM; the host only sequences launches and handles the rare
// phase-boundary work.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/relp_engine.h"
#include "relp_buffers.hpp"
#include "relp_kernels.h"
#include "relp_layout.hpp"
#include "relp_cutpool.hpp"
#include "relp_lu.hpp"
#include "relp_pack.hpp"

namespace relp {
// What a column pool and a cut pool of a handle share (relp_engine_pool.cpp).  The host copy (relp_pool.hpp) is what
// Layout::add_columns / add_cuts and the rebuilds are given; the device copy is what the sweep and the add read.
struct DevicePool {
    PoolImage image;
    DeviceBuf<int64_t> d_slice_ptr;
    DeviceBuf<int32_t> d_idx, d_part_k;
    DeviceBuf<double> d_val, d_scalar, d_all, d_part_d;   // (d_all, d_part_*, d_out: scratch of a sweep, allocated at the first one)
    DeviceBuf<uint8_t> d_active;
    DeviceBuf<char> d_out;                                // what a sweep downloads: the winners' values, their pool indices, their number
    int64_t sweep_calls = 0;                              // relp_pool_price / relp_cutpool_separate calls that succeeded
};
}  // namespace relp

// A column pool of a handle (relp_pool_create .. relp_pool_stats).  Owned by its Engine.
struct relp_pool : relp::DevicePool {
    bool stale = false;                                   // an engine row below image.bound went (relp_remove_cuts, the rollback of a trial)
};

// A cut pool of a handle (relp_cutpool_create .. relp_cutpool_stats).  Owned by its Engine.
struct relp_cutpool : relp::DevicePool {
    std::vector<double> norm;                             // relp_cutpool.hpp: CutPoolImage
    relp::DeviceBuf<double> d_norm;
};

namespace relp {

// two helper threads for the host side of a refactorisation (created at first use, joined with their owner)
struct HostPool {
    struct Slot { std::thread th; std::mutex mu; std::condition_variable cv; std::function<void()> job; bool busy = false, stop = false; };
    Slot slot[2];
    void run(int i, std::function<void()> f) {
        Slot& s = slot[i];
        if (!s.th.joinable())
            s.th = std::thread([&s] {
                std::unique_lock<std::mutex> lk(s.mu);
                for (;;) {
                    s.cv.wait(lk, [&s] { return s.busy || s.stop; });
                    if (s.stop) return;
                    lk.unlock(); s.job(); lk.lock();
                    s.busy = false;
                    s.cv.notify_all();
                }
            });
        { std::lock_guard<std::mutex> lk(s.mu); s.job = std::move(f); s.busy = true; }
        s.cv.notify_all();
    }
    void wait() {
        for (Slot& s : slot) { std::unique_lock<std::mutex> lk(s.mu); s.cv.wait(lk, [&s] { return !s.busy; }); }
    }
    ~HostPool() {
        for (Slot& s : slot) {
            if (!s.th.joinable()) continue;
            { std::lock_guard<std::mutex> lk(s.mu); s.stop = true; }
            s.cv.notify_all();
            s.th.join();
        }
    }
};

// The environment switches, read once per engine in Engine::create.  `*_set`: the variable was given.
struct Switches {
    bool debug = false;                                   // RELP_DEBUG
    bool pivot_guard_set = false; double pivot_guard = 0.0;   // RELP_PIVOT_GUARD
    bool tab_flush_all = false;                           // RELP_TAB_FLUSH_ALL
    int tab_load_batch = 0, tab_w_split = 0;              // RELP_TAB_LOAD_BATCH, RELP_TAB_W_SPLIT (0: the default)
    int tab_column_rows = 0;                              // RELP_TAB_COLUMN_ROWS (0: the default)
    bool fused_update = true;                             // RELP_FUSED_UPDATE
    bool lu_lookahead_set = false; int lu_lookahead = 8;  // RELP_LU_LOOKAHEAD
    int fuse_lanes = 256;                                 // RELP_FUSE_LANES
    int lu_device_factor = 0;                             // RELP_LU_DEVICE_FACTOR
    bool lu_pipeline_short = false;                       // RELP_LU_PIPELINE_SHORT
    int ft_big = -1;                                      // RELP_FT_BIG (-1: not given)
    bool ft_hyper_set = false; int ft_hyper = 0x9;        // RELP_FT_HYPER
    int ft_grid_price = -1;                               // RELP_FT_GRID_PRICE (-1: not given)
    int luf_bump_cap = INT32_MAX;                         // RELP_LUF_BUMP_CAP (at least 16 when given)
    int luf_dense = 64;                                   // RELP_LUF_DENSE
    bool luf_lds = true;                                  // RELP_LUF_LDS
    bool lu_peel_stacks = false;                          // RELP_LU_PEEL_STACKS
    bool dump_basis_set = false; std::string dump_basis;  // RELP_DUMP_BASIS
    bool retab_global = false;                            // RELP_RETAB_GLOBAL
    int retab_groups = 0;                                 // RELP_RETAB_GROUPS (0: not given)
    int tab_rhs_splits = 0;                               // RELP_TAB_RHS_SPLITS (0: the rule of tab_rhs_splits)
    int tab_cost_splits = 0;                              // RELP_TAB_COST_SPLITS (0: the rule of tab_cost_splits)
    bool trial_memcpy = false;                            // RELP_TRIAL_MEMCPY
    bool pool_host_add = false;                           // RELP_POOL_HOST_ADD
    bool cutpool_host_add = false;                        // RELP_CUTPOOL_HOST_ADD
    static Switches read();
};

// The stream and the profiling events.  A base of Engine: destroyed after every member, i.e. after all memory is freed.
struct EngineQueue {
    hipStream_t stream_ = nullptr; bool owns_stream_ = false;
    std::vector<hipEvent_t> prof_ev_;
    ~EngineQueue() {
        for (auto e : prof_ev_) (void)hipEventDestroy(e);
        if (owns_stream_ && stream_) (void)hipStreamDestroy(stream_);
    }
};

class Engine : private EngineQueue {
  public:
    Engine() = default;
    ~Engine();                                            // rccl_release() first, then the members, then EngineQueue

    relp_status_t create(const relp_matrix_data_t& md, const relp_config_t& cfg);
    relp_status_t set_stream(hipStream_t s);

    // step-wise pivot
    relp_status_t select_primal_pivot_column(int rule, int32_t* found, int32_t* column, double* cost);
    relp_status_t relative_costs(double* out_n);
    relp_status_t generate_column(int32_t column, double* out_m);
    relp_status_t generate_element(int32_t row, int32_t column, double* out);
    relp_status_t select_primal_pivot_row(int32_t* found, int32_t* row);
    relp_status_t select_primal_pivot_row_of(const double* column, int32_t* found, int32_t* row);
    relp_status_t bring_into_basis(int32_t column, int32_t row, double cost, int32_t* leaving);

    // loops
    relp_status_t run(int64_t max_iters, int64_t* done, int32_t* outcome);
    // dual simplex on the unsharded tableau engine (no counterpart in the reference): the loop, its two step-wise selectors and
    // a new right-hand side for the current basis
    relp_status_t run_dual(int64_t max_iters, int64_t* done, int32_t* outcome);
    relp_status_t select_dual_pivot_row(int32_t* found, int32_t* row);
    relp_status_t select_dual_pivot_column(int32_t row, int32_t* found, int32_t* column);
    relp_status_t set_right_hand_side(const double* rhs_m);
    // the same without a re-tabulation: single rhs entries (an upper bound is the rhs of its bound row) moved on the current basis
    relp_status_t change_right_hand_side(const int32_t* rows, const double* values, int32_t count);
    relp_status_t set_upper_bound(int32_t column, double value);
    relp_status_t get_right_hand_side(double* out_m);
    relp_status_t rhs_stats(int64_t* out4) const;
    // the objective's side of it: structural costs moved on the current basis in place, or all of them by a reprice of the
    // flushed tableau (no re-tabulation either way); relp_run continues from there
    relp_status_t change_cost(const int32_t* columns, const double* values, int32_t count);
    relp_status_t set_cost(const double* cost_n);
    relp_status_t get_cost(double* out_n);
    relp_status_t cost_stats(int64_t* out4) const;
    // cut rows g'x <= beta over the structural columns added behind every row, their slacks behind every column, in place on the
    // current basis (no flush, no re-tabulation); relp_run_dual continues from there.  reserve_cuts makes room without adding.
    relp_status_t add_cuts(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs);
    relp_status_t reserve_cuts(int32_t rows);
    relp_status_t cut_stats(int64_t* out4) const;
    // columns x >= 0 from outside (CSC over the engine rows) added behind every column, non-basic, in place on the current basis
    // (no flush, no re-tabulation); relp_run continues from there.  reserve_columns makes room without adding.
    relp_status_t add_columns(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost);
    relp_status_t reserve_columns(int32_t columns);
    relp_status_t column_stats(int64_t* out4) const;
    // the way back: cut rows whose slack is basic and non-basic added columns leave the tableau in place (a flush, then an
    // order-preserving compaction: no arithmetic, no re-tabulation, nothing re-allocated); relp_run / relp_run_dual continue
    relp_status_t remove_cuts(const int32_t* rows, int32_t count);
    relp_status_t remove_columns(const int32_t* columns, int32_t count);
    relp_status_t removal_stats(int64_t* out4) const;
    // batched ratio tests over the tableau as it stands, read-only: rows of T against d (penalties, cost ranges), identity columns
    // against b (rhs ranges)
    relp_status_t row_ratios(const int32_t* rows, int32_t count, double* down_ratio, int32_t* down_column, double* up_ratio,
                             int32_t* up_column);
    relp_status_t rhs_ranging(const int32_t* rows, int32_t count, double* decrease, int32_t* decrease_row, double* increase,
                              int32_t* increase_row);
    relp_status_t ranging_stats(int64_t* out4) const;
    // Gomory cuts from rows of the tableau as it stands, in structural space (the form add_cuts takes), read-only
    relp_status_t gomory_cuts(const int32_t* rows, int32_t count, const uint8_t* is_integer, int32_t kind, double away, double* coefficients,
                              double* rhs, double* fraction, int32_t* status);
    relp_status_t gomory_stats(int64_t* out4) const;
    // a trial scope: everything a trial can change between two flushes is saved on the device (one launch) and on the host, and
    // trial_end(0) puts it back to the bit; strong_branch is host code over it, relp_add_cuts and relp_run_dual
    relp_status_t trial_begin();
    relp_status_t trial_end(int32_t keep);
    relp_status_t trial_stats(int64_t* out4) const;
    relp_status_t strong_branch(const int32_t* rows, int32_t count, int32_t max_pivots, double away, double* objective, int32_t* outcome,
                                int32_t* pivots, int32_t* status);
    // a pool of candidate columns kept on the device (relp_engine_pool.cpp): priced there against -pi as it stands (read-only), its
    // winners picked there, the chosen columns added as add_columns adds them, their coefficients never uploaded again
    relp_status_t pool_create(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost,
                              relp_pool** out);
    relp_status_t pool_destroy(relp_pool* pool);
    relp_status_t pool_set_active(relp_pool* pool, const int32_t* ids, int32_t count, int32_t flag);
    relp_status_t pool_reduced_costs(relp_pool* pool, double* out_count);
    relp_status_t pool_price(relp_pool* pool, int32_t segments, double tol, int32_t* ids_out, double* d_out, int32_t* found);
    relp_status_t pool_add(relp_pool* pool, const int32_t* ids, int32_t count);
    relp_status_t pool_stats(const relp_pool* pool, int64_t* out4) const;
    // a pool of candidate cuts kept on the device (relp_engine_pool.cpp), the column pool with the roles transposed: separated there
    // against the vertex as it stands (read-only), its winners picked there, the chosen cuts added as add_cuts adds them, their
    // coefficients, b and the basis never crossing the bus
    relp_status_t cutpool_create(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs,
                                 relp_cutpool** out);
    relp_status_t cutpool_destroy(relp_cutpool* pool);
    relp_status_t cutpool_set_active(relp_cutpool* pool, const int32_t* ids, int32_t count, int32_t flag);
    relp_status_t cutpool_slacks(relp_cutpool* pool, double* out_count);
    relp_status_t cutpool_separate(relp_cutpool* pool, int32_t segments, double tol, int32_t by_efficacy, int32_t* ids_out, double* slack_out,
                                   int32_t* found);
    relp_status_t cutpool_add(relp_cutpool* pool, const int32_t* ids, int32_t count);
    relp_status_t cutpool_stats(const relp_cutpool* pool, int64_t* out4) const;
    int32_t engine_kind() const { return lay_.engine; }
    relp_status_t robust_stats(int64_t* out4) const;
    relp_status_t solve_relaxation(int64_t max_iters, int32_t* outcome);
    relp_status_t from_basis(const int32_t* basis_columns);
    relp_status_t set_reinversion_interval(int64_t pivots);
    int64_t reinversions() const { return reinversions_; }
    relp_status_t flush();
    int32_t update_block() const { return block_; }
    relp_status_t lu_stats(int64_t* out8) const;
    relp_status_t lu_lookahead_stats(int64_t* out4) const;
    relp_status_t lu_kernel_layout(int32_t* out4) const;
    relp_status_t luf_stats(int64_t* out6) const;
    relp_status_t lu_set_device_factorisation(bool on);
    relp_status_t lu_factor_residual(double* out);
    relp_status_t lu_basis_columns(std::vector<std::vector<std::pair<int32_t, double>>>& cols);
    relp_status_t lu_basis_flat(std::vector<int64_t>& ptr, std::vector<int32_t>& idx, std::vector<double>& val);
    relp_status_t lu_phase_cycles(int64_t* out16);
    relp_status_t lu_download_basis();
    relp_status_t lu_factor_downloaded_basis();
    relp_status_t lu_refactor_lookahead(int rule, int64_t budget, bool have_basis);
    relp_status_t ft_read_report(bool* have_basis);
    void lu_refactor_clock(std::chrono::steady_clock::time_point tb, std::chrono::steady_clock::time_point t0,
                           std::chrono::steady_clock::time_point t1, std::chrono::steady_clock::time_point t2);
    // BasisInverse surface of the LU engine (carry/mod.rs:68-157, lower_upper/mod.rs:199-222)
    relp_status_t basis_inverse_row(int32_t row, double* out_m);
    relp_status_t should_refactor(int32_t* out);
    relp_status_t generate_column_of(const int32_t* idx, const double* val, int32_t nnz, double* out_m);
    relp_status_t cost_difference_of(const int32_t* idx, const double* val, int32_t nnz, double* out);
    relp_status_t lu_change_basis(int32_t row);
    relp_status_t lu_updates(int32_t* count);
    relp_status_t lu_get_update(int32_t k, int32_t* pivot, int32_t* idx, double* val, int32_t cap, int32_t* nnz);
    relp_status_t lu_get_upper(int64_t* col_ptr, int32_t* row_idx, double* values, int64_t cap, int64_t* nnz);
    relp_status_t lu_set_factors(const int64_t* l_ptr, const int32_t* l_idx, const double* l_val, const int64_t* u_ptr,
                                 const int32_t* u_idx, const double* u_val);
    relp_status_t shard_flush_begin(double** dev_snapshot, int64_t* len);
    relp_status_t shard_flush_end();

    // getters
    int32_t nr_rows() const { return lay_.m; }
    int32_t nr_columns() const { return lay_.nr_columns(); }
    int32_t phase() const { return phase_; }
    int32_t nr_artificial() const { return lay_.nr_artificial; }
    relp_status_t get_objective(double* out);
    relp_status_t get_vector(int which, double* out);  // 0 b, 1 minus_pi, 2 alpha
    relp_status_t get_basis_indices(int32_t* out);
    relp_status_t get_basis_inverse(double* out);
    relp_status_t current_bfs(int32_t* cols, double* vals, int32_t cap, int32_t* count);
    relp_status_t get_iterations(int64_t* out);
    relp_status_t get_degenerate_pivots(int64_t* out);
    relp_status_t tab_flush_stats(int64_t* out2);
    relp_status_t retab_stats(int64_t* out4) const;
    int32_t tab_load_batch_size() const { return tableau_ ? load_batch_ : 0; }
    // for the rows the tableau has now (cut rows come and go); blocks above 64 pivots keep 256 unless a value was asked for:
    // their shares need the larger register arrays, which nobody has measured
    int32_t tab_column_rows_size() const {
        if (!tableau_) return 0;
        const bool asked = col_rows_wanted_ == 64 || col_rows_wanted_ == 128 || col_rows_wanted_ == 256;
        return !asked && block_ > 64 ? 256 : tab_column_rows(col_rows_wanted_, lay_.m);
    }
    relp_status_t get_trace(int32_t* phase, int32_t* entering, int32_t* row, int32_t* leaving, int64_t cap,
                            int64_t* count);
    relp_status_t check_basis(double* max_identity_error, double* max_basic_cost, double* min_b);

    relp_status_t profile_enable(bool enable, int64_t max_launches, int32_t sample_every);
    relp_status_t profile_read(int kernel_id, int64_t* launches, double* total_ms);

    // shards
    void shard_ranges(int32_t* col_lo, int32_t* col_hi, int32_t* row_lo, int32_t* row_hi, int32_t* stride) const;
    int64_t candidate_len() const { return lay_.candidate_len; }
    int64_t rho_len() const { return ld_b_; }
    relp_status_t shard_price(double* dev_candidate);
    relp_status_t shard_select_column(const double* dev_candidates, int32_t count);
    relp_status_t shard_ftran(double* dev_alpha_slice);
    relp_status_t shard_ratio(const double* dev_alpha_slices, int32_t count, double* dev_rho);
    relp_status_t shard_update(const double* dev_rho);
    relp_status_t shard_pivot();
    relp_status_t shard_set_collectives(relp_allgather_fn ag, relp_allreduce_sum_fn ar, void* ctx);
    relp_status_t shard_run(int64_t max_iters, int64_t* done, int32_t* outcome);
    void shard_inject_failure(int64_t after_pivots) { inject_failure_after_ = after_pivots; }
    relp_status_t rccl_attach(const uint8_t* id);
    relp_status_t poll(int32_t* outcome, int64_t* iterations);

    const char* last_error() const { return err_.c_str(); }

  private:
    // ---- MatrixData + Kind (host side: rows, columns, artificial columns, shards) ----
    Layout lay_;
    relp_config_t cfg_{};
    int32_t phase_ = 1;

    // ---- device state ----
    Switches sw_;
    DeviceBuf<double> dA_; int64_t ld_a_ = 0;             // (a view when the caller's device matrix was adopted)
    DeviceBuf<double> dBinv_; int64_t ld_b_ = 0;
    DeviceBuf<double> d_minus_pi_, d_b_, d_alpha_, d_aq_, d_rho_, d_d_, d_w_, d_cost_;
    DeviceBuf<int32_t> d_basis_, d_column_to_row_, d_bound_row_, d_vrow0_, d_vrow1_, d_vsign_, d_trace_;
    DeviceBuf<uint8_t> d_in_basis_;
    DeviceBuf<PivotRecord> d_rec_;
    PinnedBuf<PivotRecord> h_rec_;
    int64_t trace_cap_ = 0;
    // deferred update (B^-1 = (I + W S') B0inv), see relp_kernels.h
    int32_t block_ = 0;            // K, 0 = explicit rank-1 updates
    int64_t since_flush_ = 0;      // pivots enqueued since the last flush
    DeviceBuf<double> d_v_;        // B0inv a_q before the W correction
    DeviceBuf<double> d_W_, d_wr_, d_R_;
    DeviceBuf<int32_t> d_S_, d_pos_of_row_;
    DeviceBuf<double> d_part_k1_;  // PRICE workgroups' partial argmin (SelectPartials)
    DeviceBuf<int32_t> d_part_j_;
    // dense-tableau engine (cfg.engine == RELP_ENGINE_TABLEAU)
    bool tableau_ = false;
    DeviceBuf<double> dT0_; int64_t ld_t_ = 0;
    DeviceBuf<double> dR0_; int64_t ld_r_ = 0;
    // flush over the columns with a nonzero R0 entry (relp_kernels.h: FlushList); RELP_TAB_FLUSH_ALL=1: every owned column
    bool flush_all_ = false;
    DeviceBuf<int32_t> d_fcols_, d_fcount_;
    DeviceBuf<unsigned long long> d_fmask_, d_fstats_;              // d_fstats_: {flushes, columns flushed} since create
    DeviceBuf<double> d_R0c_;
    FlushList flush_list() const;
    // RELP_TAB_LOAD_BATCH / RELP_TAB_W_SPLIT (relp_kernels.h: tab_load_batch, launch_tab_ratio_update_all)
    int32_t load_batch_ = 0, w_split_ = 0;
    int32_t col_rows_wanted_ = 0;        // RELP_TAB_COLUMN_ROWS (tab_column_rows): the fused single-GPU loop's column kernel
    DeviceBuf<double> d_cost_store_;     // cost per stored column in the current phase
    DeviceBuf<int32_t> d_idcol_;         // stored column that was e_k originally, per row k
    // Ratio test + update in one launch (single-GPU loop, relp_kernels.h: launch_tab_ratio_update_all): the second copies of b
    // and the basis array it writes (swapped with d_b_ / d_basis_ after every pivot), the shadow row of W and its {row, length}
    bool fused_update_ = false, shadow_pending_ = false;
    DeviceBuf<double> d_b_alt_, d_shadow_;
    DeviceBuf<int32_t> d_basis_alt_, d_shadow_meta_;
    DeviceBuf<double> d_rmin_;           // minimum ratio per block of 256 (128, 64) rows (k_tab_select_column -> k_ratio_blocks)
    int32_t n_store_ = 0;                // stored columns = original artificials + provider columns
    int32_t tab_na_ = 0;                 // original number of artificial columns (their block is kept)
    bool tab_partials_valid_ = false;    // the PRICE partials describe the current d
    static constexpr int kRepriceEveryFlushes = 8;
    int32_t flushes_since_reprice_ = 0;
    std::vector<int32_t> idcol_h_;
    std::vector<double> cost_store_h_;
    bool in_loop_ = false;               // inside relp_run / relp_shard_run (the two-launch pivot keeps a shadow row pending)
    void tab_settle();                   // fold the fused update's shadow row into W
    struct LoopScope {                   // marks the pivot loops; settles on every way out
        Engine& e;
        explicit LoopScope(Engine& en) : e(en) { e.in_loop_ = true; }
        ~LoopScope() { e.in_loop_ = false; e.tab_settle(); }
    };
    struct SettledScope {                // work that reads or rebuilds the tableau from inside a pivot loop (re-tabulation)
        Engine& e; bool was;
        explicit SettledScope(Engine& en) : e(en), was(en.in_loop_) { e.in_loop_ = false; e.tab_settle(); }
        ~SettledScope() { e.in_loop_ = was; }
    };
    TableauView tview() const;
    double* d_aq_big() { return dR0_ + (int64_t)block_ * ld_r_; }         // scratch row behind R0 (owned columns)
    SelectPartials tab_partials(int rule) const;
    SelectPartials lu_partials(int rule) const;
    void enqueue_iteration_tableau(int rule);
    void enqueue_iteration_dual();
    relp_status_t dual_ready(const char* what);        // phase 2 on the unsharded tableau engine, or the error
    // what the in-place functions below share: their front (settle, download the record, *p = the open block's pending rows), the
    // guard and the four counters of their *_stats, and the validation of a named list (index in [0, bound), named once, finite)
    relp_status_t settled_pending(int32_t* p);
    relp_status_t in_place_stats(int64_t* out4, int64_t s0, int64_t s1, int64_t s2, int64_t s3) const;
    relp_status_t check_named_list(const char* what, const int32_t* index, const double* values, int32_t count, int32_t bound,
                                   const char* noun, const char* outside);
    void tableau_reprice();
    // relp_change_right_hand_side: the compacted list (identity column, delta) of a change, v = the pending rows' share and the
    // per-split partial sums (relp_kernels.h: launch_tab_rhs_change); what relp_rhs_stats reports
    DeviceBuf<int32_t> d_rhs_cols_;
    DeviceBuf<double> d_rhs_delta_, d_rhs_v_, d_rhs_partial_;      // (d_rhs_partial_: allocated at the first split launch, grown on demand)
    int64_t rhs_changes_ = 0, rhs_columns_ = 0;
    int32_t rhs_last_p_ = 0, rhs_last_splits_ = 0;
    // relp_change_cost: the two compacted lists of a change -- (row, delta) of the basic columns, (storage column, delta) of the
    // non-basic ones --, u = the pending rows' share and the per-split partial sums (relp_kernels.h: launch_tab_cost_change);
    // what relp_cost_stats reports
    DeviceBuf<int32_t> d_cost_rows_, d_cost_ncols_;
    DeviceBuf<double> d_cost_delta_, d_cost_ndelta_, d_cost_u_, d_cost_partial_;
    int64_t cost_changes_ = 0, cost_rows_ = 0;
    int32_t cost_last_p_ = 0, cost_last_splits_ = 0;
    relp_status_t store_costs(int32_t lo, int32_t hi);  // d_cost_, cost_store_h_, d_cost_store_ <- lay_.cost[lo, hi)
    // relp_add_cuts: cut_room_ = the cut rows (and slack columns) every buffer of the tableau path has room for; grow_for_cuts
    // takes them to a larger room (the only function that does).  The list of a call (rows, coef[entry][cut]) and u[cut][pending row]
    // (relp_kernels.h: launch_tab_add_cuts) are grown on demand; what relp_cut_stats reports
    int32_t cut_room_ = 0;
    relp_status_t grow_for_cuts(int32_t room) { return grow_tableau(room, col_room_); }
    // The one growth function of the tableau engine, for both kinds of room (cut rows with their slacks; added columns): never shrinks
    relp_status_t grow_tableau(int32_t cut_room, int32_t col_room);
    DeviceBuf<int32_t> d_cut_rows_;
    DeviceBuf<double> d_cut_coef_, d_cut_u_, d_cut_g_;   // (d_cut_g_: the cuts of a call by structural column, on their way into A)
    int32_t cut_last_rows_ = 0, cut_last_p_ = 0;
    // relp_add_columns: col_room_ = the added columns every per-column buffer has room for, independent of cut_room_.  d_col_a_:
    // the added columns as a dense block in row space, column a at a * ld_c_ (ld_c_ >= the row capacity), what a re-tabulation
    // solves them from (retabulate).  The list of a call (identity columns, coef[entry][column]), d and cost of the new columns
    // (relp_kernels.h: launch_tab_add_columns) are grown on demand; what relp_column_stats reports
    int32_t col_room_ = 0;
    int64_t ld_c_ = 0;
    DeviceBuf<double> d_col_a_;
    DeviceBuf<int32_t> d_col_cols_;
    DeviceBuf<double> d_col_coef_, d_col_d_, d_col_cost_;
    int32_t col_last_cols_ = 0, col_last_p_ = 0;
    relp_status_t room_for_columns(const char* what, int32_t count);      // the growth rule of relp_add_columns
    // the layout, the host mirrors and the record after the launches of an add (the columns have passed Layout::check_columns)
    relp_status_t columns_added(int32_t count, const int64_t* col_ptr, const int32_t* row_idx, const double* values, const double* cost,
                                int32_t entries, int32_t p);
    // relp_pool_*: the pools of this handle (freed with it), the chosen ids and the places of the rows of an add on the device
    // (relp_kernels.h: launch_pool_add_operands), grown on demand
    std::vector<std::unique_ptr<relp_pool>> pools_;
    DeviceBuf<int32_t> d_pool_ids_, d_pool_rank_, d_pool_entries_;
    DeviceBuf<double> d_pool_minus_pi_;                   // -pi as a vector: scratch of every price and add (relp_kernels.h: MinusPi)
    relp_status_t pool_ready(const char* what, const relp_pool* pool, bool fresh);
    void pools_mark_stale(const int32_t* rows, int32_t count);             // engine rows went: the listed ones, or (nullptr) those from lay_.m on
    MinusPi minus_pi_view() const { return MinusPi{d_d_, d_cost_store_, d_idcol_, lay_.m, d_pool_minus_pi_}; }
    relp_status_t pool_launch_price(relp_pool& pool, int32_t segments, double tol, bool all);
    // what the column pools and the cut pools do alike, each written once (`list`: pools_ or cutpools_; `w`: the words of the kind).
    // The three member templates are defined in relp_engine_pool.cpp and used there alone: a use from another translation unit
    // would not link.
    template <class List> relp_status_t pool_mine(const char* what, const PoolWords& w, const List& list, const DevicePool* pool);
    template <class List> relp_status_t pool_drop(const char* what, const PoolWords& w, List& list, const DevicePool* pool);
    template <class List> relp_status_t pool_stats_in(const List& list, const DevicePool* pool, int64_t* out4) const;
    relp_status_t pool_upload(DevicePool& dp, const std::vector<double>* norm, DeviceBuf<double>* d_norm);
    PoolView pool_view(const DevicePool& dp) const;
    relp_status_t pool_flags(const DevicePool& dp, const int32_t* ids, int32_t count, int32_t flag);
    relp_status_t pool_flags_checked(const char* what, const PoolWords& w, const DevicePool& dp, const int32_t* ids, int32_t count, int32_t flag);
    relp_status_t pool_sweep_scratch(DevicePool& dp, int32_t segments, bool all);
    relp_status_t pool_winners(const char* what, DevicePool& dp, int32_t segments, int32_t* ids_out, double* out, int32_t* found);
    void rename_prefix(const char* from, const char* to);                  // err_ said `from`, the call the checks were borrowed from
    // relp_cutpool_*: the cut pools of this handle (freed with it), the vertex over the structural columns and the marks of an add on
    // the device (relp_kernels.h: Vertex, launch_cutpool_add_operands), grown on demand; d_pool_ids_ and d_pool_entries_ are shared
    // with the column pools
    std::vector<std::unique_ptr<relp_cutpool>> cutpools_;
    DeviceBuf<double> d_cutpool_x_;
    DeviceBuf<int32_t> d_cutpool_mark_;
    CutPoolView cutpool_view(const relp_cutpool& pool) const { return CutPoolView{pool_view(pool), pool.d_norm}; }
    Vertex vertex_view() const { return Vertex{d_b_, d_basis_, lay_.m, lay_.nr_normal, d_cutpool_x_}; }
    relp_status_t cutpool_launch_separate(relp_cutpool& pool, int32_t segments, double tol, int32_t by_efficacy);
    relp_status_t room_for_cuts(const char* what, int32_t count);         // the growth rule of relp_add_cuts, its room rule inside a trial
    // the layout, the host mirrors and the record after the launches of an add (the cuts have passed Layout::check_cuts)
    relp_status_t cuts_added(int32_t count, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* rhs,
                             int32_t entries, int32_t p);
    // relp_remove_cuts / relp_remove_columns: the lists of a call on the device (relp_kernels.h: launch_tab_compact), grown on demand;
    // what relp_removal_stats reports.  The rooms stay: the next add reuses what a removal freed.
    DeviceBuf<int32_t> d_rm_lists_;
    int64_t rm_cuts_ = 0, rm_columns_ = 0, rm_last_moved_ = 0;
    int32_t rm_last_p_ = 0;
    relp_status_t flush_for_removal();
    relp_status_t compact_tableau(const std::vector<int32_t>& rows_t, const std::vector<int32_t>& rows_c, const std::vector<int32_t>& cols_p,
                                  const std::vector<int32_t>& basis);
    relp_status_t finish_removal();
    // relp_row_ratios / relp_rhs_ranging: the uploaded list (rows, or their identity columns), the per-(direction, entry, block)
    // minima and the results [direction][entry] (relp_kernels.h: launch_tab_row_ratios, launch_tab_rhs_ranging); allocated at the
    // first query, grown on demand; what relp_ranging_stats reports
    relp_status_t ranging_query(bool columns, const char* what, const int32_t* rows, int32_t count, double* ratio0, int32_t* index0,
                                double* ratio1, int32_t* index1);
    DeviceBuf<int32_t> d_rng_list_, d_rng_part_j_, d_rng_index_;
    DeviceBuf<double> d_rng_part_k_, d_rng_ratio_;
    int64_t rng_ratio_calls_ = 0, rng_ratio_rows_ = 0, rng_ranging_calls_ = 0;
    int32_t rng_last_p_ = 0;
    // relp_gomory_cuts: the uploaded list (rows, f0, the integer flags) and the scratch of launch_tab_gomory -- [g | y | bad], one
    // download, then pi -- allocated at the first call, grown on demand; what relp_gomory_stats reports
    DeviceBuf<int32_t> d_gom_rows_;
    DeviceBuf<double> d_gom_f0_, d_gom_out_;
    DeviceBuf<uint8_t> d_gom_int_;
    int64_t gom_calls_ = 0, gom_entries_ = 0, gom_cuts_ = 0;
    int32_t gom_last_p_ = 0;
    // relp_trial_begin / relp_trial_end (relp_engine_trial.cpp): the plan of the open trial's snapshot (relp_trial.hpp) over
    // d_trial_ -- one device buffer, allocated at the first begin, grown on demand --, the host side of the snapshot, and what
    // relp_trial_stats reports.  in_trial(what): RELP_E_STATE for a call that flushes, rebuilds, re-allocates or compacts.
    struct TrialExtents { int32_t m = 0, n_store = 0, n = 0, nr_normal = 0, p = 0; };   // rows, stored / tableau / structural columns, pending rows at the begin
    struct TrialHost {
        TrialExtents extents;
        Layout lay;
        int32_t n_store = 0, n_alloc = 0;
        std::vector<int32_t> idcol_h;
        std::vector<double> cost_store_h;
        int64_t since_flush = 0, since_reinvert = 0, reinvert_interval = 0, reinversions = 0;
        int32_t flushes_since_reprice = 0;
        double last_reinvert_drift = -1.0;
        bool retab_done = false;
        int64_t rhs_changes = 0, rhs_columns = 0, cost_changes = 0, cost_rows = 0, rm_cuts = 0, rm_columns = 0, rm_last_moved = 0;
        int64_t rng_ratio_calls = 0, rng_ratio_rows = 0, rng_ranging_calls = 0, gom_calls = 0, gom_entries = 0, gom_cuts = 0;
        int32_t rhs_last_p = 0, rhs_last_splits = 0, cost_last_p = 0, cost_last_splits = 0, cut_last_rows = 0, cut_last_p = 0;
        int32_t col_last_cols = 0, col_last_p = 0, rm_last_p = 0, rng_last_p = 0, gom_last_p = 0;
    };
    bool trial_open_ = false;
    TrialPlan trial_plan_;
    DeviceBuf<char> d_trial_;
    TrialHost trial_host_;
    int64_t trials_begun_ = 0, trials_rolled_back_ = 0, trial_last_bytes_ = 0, trial_last_room_ = 0;
    relp_status_t in_trial(const char* what);
    TrialPlan trial_layout(const TrialExtents& x, bool* ok);
    relp_status_t trial_copy(bool save);
    void trial_host_save();
    void trial_host_restore();
    relp_status_t check_dual_feasible(const char* what);   // the front of relp_run_dual: PRICE finds no candidate, or RELP_E_STATE
    // sparse LU engine (cfg.engine == RELP_ENGINE_LU): B^-1 = (I + W S') (L U)^-1, refactor every block_ pivots
    bool lu_ = false;
    std::vector<int64_t> hc_ptr_; std::vector<int32_t> hc_idx_; std::vector<double> hc_val_;   // host CSC of A
    DeviceBuf<int64_t> d_cptr_; DeviceBuf<int32_t> d_cidx_; DeviceBuf<double> d_cval_;         // device CSC of A
    LUFactors hlu_;
    DeviceBuf<char> d_lu_buf_;                           // packed factors (permutations, rows, entries, levels)
    std::vector<std::vector<std::pair<int32_t, double>>> basis_cols_;      // the basis columns handed to lu_factor
    std::vector<int64_t> basis_ptr_; std::vector<int32_t> basis_idx_; std::vector<double> basis_val_;   // ... as one flat copy (lu_factor_csc)
    HostPool host_pool_;                                  // the host side of a refactorisation (created at first use, joined with the engine)
    PinnedBuf<char> h_lu_buf_;                            // the same, assembled in pinned host memory
    DeviceBuf<char> d_lu_buf_alt_;                        // second device buffer: the factors the host prepares while the kernel runs
    PinnedBuf<int32_t> h_basis_;                          // the basis a refactorisation downloads
    PinnedBuf<FtMirror> h_mirror_;                        // mapped: what k_ft_run reports (relp_kernels.h); .device() is its address there
    DeviceBuf<double> d_lu_scratch_;
    relp_status_t ensure_lu_scratch();
    // the batch solves of a rebuild (re-inversion, re-tabulation, warm start) with x in global memory (relp_kernels.h: LuSlabs):
    // one slab of ld_b_ doubles per workgroup, allocated at first use and kept; what relp_retab_stats reports
    DeviceBuf<double> d_lu_slabs_;
    int64_t batch_solves_lds_ = 0, batch_solves_slab_ = 0;
    int32_t slab_groups_last_ = 0;
    relp_status_t batch_solve_slabs(int32_t rhs_count, LuSlabs* slabs);
    DeviceLU dlu_{};
    relp_status_t lu_status_ = RELP_OK;                   // a failed refactorisation inside the loop
    int64_t lu_refactors_ = 0;
    int64_t lu_lookahead_installs_ = 0, lu_replayed_changes_ = 0;     // look-ahead refactorisations installed, journal entries replayed
    int32_t lu_pipeline_cap_ = 0;                        // RELP_LU_PIPELINE_SHORT: the update file's cap while the host factorises (run_ft)
    double refactor_us_[3] = {0.0, 0.0, 0.0};            // host time: basis + columns, factorisation, schedules + upload
    // revised engine: B^-1 is re-inverted from the basis columns every `reinvert_interval_` pivots (0 = never)
    int64_t reinvert_interval_ = 0, since_reinvert_ = 0, reinversions_ = 0;
    DeviceCSC csc() const { return DeviceCSC{d_cptr_, d_cidx_, d_cval_}; }
    // structural column p of the host CSC for Layout::for_each_entry
    auto csc_column() const {
        return [this](int32_t p, auto&& put) { for (int64_t e = hc_ptr_[p]; e < hc_ptr_[p + 1]; ++e) put(hc_idx_[e], hc_val_[e]); };
    }
    relp_status_t lu_load_matrix(const relp_matrix_data_t& md);
    relp_status_t lu_refactor();
    relp_status_t lu_upload_factors();
    // its steps, in the order of the pieces in the buffer (relp_engine_lu.cpp); LuUpload is what one step hands to the next
    struct LuUpload;
    void lu_pack_permutations(LuUpload& u);
    relp_status_t lu_pack_images(LuUpload& u);
    void lu_pack_pivot_info(LuUpload& u);
    void lu_pack_row_schedules(LuUpload& u);
    relp_status_t lu_copy_to_device(LuUpload& u);
    relp_status_t lu_install(LuUpload& u);
    int64_t ft_plan_staging(FtState& f) const;            // stage_bytes, stage[], lds_bytes from the four images; returns the LDS base
    relp_status_t reinvert();
    relp_status_t retabulate(bool adapt_interval = true);   // false: b moves because rhs did (relp_set_right_hand_side), not by drift
    bool retab_done_ = false;                             // the last retabulate() rebuilt the tableau (it keeps the old one otherwise)
    relp_status_t build_basis_columns(const std::vector<int32_t>& basis, std::vector<std::vector<std::pair<int32_t, double>>>* cols);
    void enqueue_iteration_lu(int rule);
    // Forrest-Tomlin mode of the LU engine (relp_kernels_ft.hip): whole pivots in one persistent workgroup; chosen at
    // create when the work vectors, the eta pool and the dense tail of U fit one CU's LDS (m <= kFtMaxRows)
    bool ft_ = false;
    FtState fts_{};
    DeviceBuf<char> d_ft_buf_;
    PinnedBuf<int32_t> h_ft_hdr_;                         // copy of fts_.hdr
    int32_t ft_tcap_ = 0, ft_eta_cap_ = 0;
    // the refactorisation on the device (relp_engine_luf.cpp, relp_lu_factor_core.h): RELP_LU_DEVICE_FACTOR=1 or
    // relp_lu_set_device_factorisation; a bump beyond the dense working copy falls back to lu_factor on the host
    struct LufState;
    LufState* luf_ = nullptr;
    bool luf_enabled_ = false;
    int64_t luf_runs_ = 0, luf_fallbacks_ = 0, luf_lds_retries_ = 0; double luf_kernel_us_ = 0.0; int32_t luf_last_bump_ = 0, luf_last_peeled_ = 0;
    relp_status_t luf_prepare();
    relp_status_t lu_factor_on_device(int32_t* device_status);
    relp_status_t luf_download_factors();
    relp_status_t lu_host_factors();
    bool luf_is_resident() const;
    bool luf_download_ = false;                          // RELP_LU_DEVICE_FACTOR=2: download the factors, schedule on the host
    void luf_release();
    bool hyper_forced_ = false; int32_t hyper_probe_in_[4] = {0, 0, 0, 0};    // adaptive hyper-sparse starts (ft_read_report)
    bool ft_big_ = false; int32_t ft_rhs_cap_ = 0;        // layout of the persistent kernel (relp_kernels_ft.hip: ft_layout)
    bool ft_grid_price_ = false;                          // Dantzig PRICE as a grid launch per pivot (run_ft): layout 2 with very many columns
    int32_t ft_tier_ = 0;                                 // 0 all in LDS, 1 big (ft_big_), 2 no per-row array in LDS (ft_big_ too)
    int64_t ft_zero_bytes_ = 0, ft_ones_bytes_ = 0;       // the two regions of the state buffer a refactorisation resets
    bool ft_need_refactor_ = false;
    relp_status_t ft_plan_and_alloc();
    relp_status_t ft_reset();
    relp_status_t ft_read_hdr(bool with_record = false);
    FtProblem ft_problem(int rule) const;
    void ft_enqueue_pivots(const FtState& go, int rule, int64_t left);
    DeviceBuf<char> d_pe_buf_; PriceEll pe_{};            // PRICE copy of the structural columns (relp_kernels.h: PriceEll)
    relp_status_t ft_build_price_ell();
    relp_status_t run_ft(int64_t max_iters, int64_t* done, int32_t* outcome);
    DeferredUpdate deferred() const;
    void enqueue_flush();
    int32_t n_alloc_ = 0;     // allocated tableau columns (artificial + provider)

    // ---- shards ----
    // native multi-GPU loop: collective hooks and the message buffers they exchange
    relp_allgather_fn coll_allgather_ = nullptr;
    relp_allreduce_sum_fn coll_allreduce_ = nullptr;
    void* coll_ctx_ = nullptr;
    void* rccl_comm_ = nullptr;          // ncclComm_t owned by this engine (relp_rccl_attach)
    DeviceBuf<double> d_msg_cand_, d_msg_cands_;                 // this rank's candidate / all ranks' candidates
    DeviceBuf<double> d_msg_slice_, d_msg_slices_, d_msg_rho_;   // revised engine: alpha slice / all slices, rho
    relp_status_t shard_iteration();
    relp_status_t shard_iteration_comm_only(int from_step);
    int coll_step_ = 0;                  // collectives of the current pivot already done (a failed pivot is completed from here)
    int64_t shadow_flush_ = 0;           // pivots since the last flush as every rank counts them
    relp_status_t shard_agree_on_status(relp_status_t local);
    DeviceBuf<double> d_msg_status_, d_msg_statuses_;   // this rank's status / all ranks' statuses (agreed on at every poll of relp_shard_run)
    int64_t inject_failure_after_ = -1;  // test hook (relp_shard_inject_failure)
    bool coll_broken_ = false;           // a collective hook itself failed: nothing can be agreed on any more
    relp_status_t remove_artificial_basis_variables_sharded(std::vector<int32_t>& rows_to_remove);
    void rccl_release();

    // ---- profiling ----
    bool prof_on_ = false;
    std::vector<int> prof_kid_;
    bool prof_open_ = false;
    int32_t prof_stride_ = 1;      // bracket the kernels of every prof_stride_-th pivot only
    int64_t prof_tick_ = 0;

    std::string err_;

    // helpers
    ColumnTable table() const;
    Tolerances tolerances() const;
    bool hip_ok(hipError_t e, const char* what);
    relp_status_t fail(relp_status_t code, const std::string& msg) { err_ = msg; return code; }
    relp_status_t fetch(void* dst, const void* src, size_t bytes);
    relp_status_t download_rec();
    relp_status_t upload_rec();
    // re-arm the pivot record: download it, outcome = DEV_RUNNING, whatever else `f` sets, upload it
    template <class F> relp_status_t edit_rec(F&& f) {
        const relp_status_t st = download_rec();
        if (st) return st;
        h_rec_->outcome = DEV_RUNNING;
        f(*h_rec_);
        return upload_rec();
    }
    relp_status_t edit_rec() { return edit_rec([](PivotRecord&) {}); }
    int current_rule() const { return phase_ == 1 ? cfg_.phase_one_rule : cfg_.phase_two_rule; }
    // dA_ / dBinv_ hold the owned columns / rows only: shifted so that kernels index globally
    double* A_base() const { return dA_ - (int64_t)lay_.col_lo * ld_a_; }
    double* Binv_base() const { return dBinv_ - (int64_t)lay_.row_lo * ld_b_; }
    relp_status_t take_lu_status() { const relp_status_t e = lu_status_; lu_status_ = RELP_OK; return e; }   // a refactorisation that failed inside a launch sequence
    // LU engine, Forrest-Tomlin or product form: row `row` of B^-1 (rhs null) or rhs' B^-1 (row -1); B^-1 rhs
    void lu_btran(int32_t row, const double* rhs, double* out);
    void lu_ftran(const double* rhs, double* out, const PivotRecord* rec);
    relp_status_t read_pivot_row(int32_t* found, int32_t* row);
    std::vector<double> basic_costs(const std::vector<int32_t>& basis, int phase, double sign) const;
    double objective_of(const std::vector<int32_t>& basis, const std::vector<double>& b) const;
    relp_status_t check_basis_columns(const std::vector<int32_t>& basis, std::vector<uint8_t>* flags);
    relp_status_t refactor_current_basis(std::vector<int32_t>* basis, std::vector<double>* b_before, bool* factored);
    relp_status_t inverse_from_factors(const std::vector<double>& w, bool rearm, std::vector<double>* b);
    relp_status_t basic_artificials(std::vector<int32_t>* basis, std::vector<int32_t>* arts);
    void keep_artificial_row(int32_t a, std::vector<int32_t>& rows_to_remove);
    void prof_begin(int kid, hipStream_t on = nullptr);
    void prof_end(hipStream_t on = nullptr);
    void enqueue_price(int cost_mode, const double* vec, const PivotRecord* rec, int32_t p_lo, int32_t p_hi);
    void enqueue_iteration(int rule);
    relp_status_t finish_phase_one(int32_t* outcome);
    relp_status_t remove_artificial_basis_variables(std::vector<int32_t>& rows_to_remove);
    relp_status_t switch_to_phase_two(const std::vector<int32_t>& rows_to_remove);
    // RELP_ARTIFICIAL_TEXTBOOK: artificial variables no zero-level pivot could remove; remove_rows exchanges the basis position
    // each one sits in with its own row before both go (the pair (own constraint, position) always leaves a basis)
    std::vector<int32_t> stuck_artificials_;
    // relp_config_t.pivot_rescue (relp_engine.h): the loop of run_loop() behind a look at every exit without a pivot row
    relp_status_t run_loop(int64_t max_iters, int64_t* done, int32_t* outcome);
    relp_status_t outcome_of_record(int32_t* oc);
    relp_status_t rescue_unbar_all();
    void auto_reinversion_adapt(const std::vector<double>& before, const std::vector<double>& after);
    std::vector<int32_t> barred_;                  // columns barred from pricing (in_basis flag 2) until the basis changes
    // RELP_PIVOT_GUARD: a pivot element below this fraction of the column's largest |entry| ends the loop for a rescue.  0 = off,
    // the default: measured on 16 files of the corpus (profiles/r04_guard_sweep.md), 1e-5 / 1e-7 / 1e-9 fire on most pivots of the
    // ill-conditioned files and the ratio test without the small rows overshoots them -- wrong `infeasible` outcomes on four files
    double guard_rel_ = 0.0;
    bool pivot_guard_on_ = false;                  // Tolerances::pivot_guard of the launches (on inside the rescued loop only)
    bool hold_phase_end_ = false;                  // run_loop returns kHeldNoCandidate instead of ending the phase
    int64_t rescue_small_pivots_ = 0, rescue_barred_ = 0, rescue_confirmations_ = 0;
    double last_reinvert_drift_ = -1.0;            // relp_config_t.auto_reinversion: what the last rebuild moved b by (relative)
    relp_status_t remove_rows(const std::vector<int32_t>& rows);
};

}  // namespace relp
