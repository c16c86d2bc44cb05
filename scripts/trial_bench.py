"""Cost of the trial scope (relp_trial_begin / relp_trial_end) and of relp_strong_branch beside the only way back there was before
them: relp_from_basis on the same handle (a re-tabulation of the whole tableau for the basis the trial started from).

The LP is the dense `<=` LP of scripts/cuts_bench.py (bench.py's dense10k: A generated in HBM by relp_synth_fill_dense) on the
tableau engine at the default update_block, solved to optimality.  Timed, host clock around calls (relp_trial_end and everything
that returns a value synchronise; relp_trial_begin only enqueues, so it is timed together with the relp_trial_end(0) that follows it
and once more alone with a device synchronisation of its own through relp_get_objective):
  rollback   relp_trial_begin + relp_trial_end(0) with nothing in between: five warm-up pairs, then the median / min / max of --reps
             pairs, with the update block open (a second engine taken through exactly the pivots of the first,
             scripts/rhs_bench.py says why) and flushed (p = 0), on an engine created with the one-launch copy (k_tab_trial_copy) and
             on one created under RELP_TRIAL_MEMCPY=1 (the same copies as a chain of hipMemcpyAsync)
  branch     relp_strong_branch over the first 1 / 8 / 64 rows whose basic column is structural and whose fraction lies in [0.001,
             0.999], at max_pivots 1 / 16 / 63: one warm-up call, then the median of 3; per child = per call / (2 rows)
  child      one child by hand, median over the first 8 rows, both sides: relp_trial_begin, relp_add_cuts, relp_run_dual(max_pivots),
             relp_get_objective, relp_trial_end(0), each timed (the split of a child into add-cut, pivots and rollback)
  yardstick  relp_from_basis with the optimal basis on the same handle, median of 3
One JSON line; `--out` also writes it to a file.

    python scripts/trial_bench.py [--m 10000 --n 10000 --seed 20250002] [--rows 1,8,64] [--pivots 1,16,63] [--reps 20] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rust_lp_amd  # noqa: E402,F401
from rust_lp_amd import MatrixData, engine, synthetic  # noqa: E402


def dense_le_md(m, n, seed):
    b = n * (1000 + (synthetic.splitmix64(seed, 1, np.arange(m, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    c = -(1000 + (synthetic.splitmix64(seed, 2, np.arange(n, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    return MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=b.astype(np.float64) / 4000.0, cost=c.astype(np.float64) / 1000.0,
                      upper_bound=np.full(n, np.inf))


def summary(seconds, scale=1e3, unit="ms"):
    return {f"median_{unit}": scale * statistics.median(seconds), f"min_{unit}": scale * min(seconds), f"max_{unit}": scale * max(seconds),
            "calls": len(seconds)}


def timed(call, warm, reps):
    for _ in range(warm):
        call()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


def rollback_times(h, reps):
    def pair():
        h.trial_begin()
        h.trial_end(False)

    pairs = timed(pair, 5, reps)
    begins, ends = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        h.trial_begin()
        h.objective_function_value()                   # (a download: waits for the snapshot)
        t1 = time.perf_counter()
        h.trial_end(False)
        t2 = time.perf_counter()
        begins.append(t1 - t0)
        ends.append(t2 - t1)
    h.change_right_hand_side([0], h.right_hand_side()[:1])      # (changes nothing; relp_rhs_stats then reports the pending rows)
    return {"pending_rows": h.rhs_stats()[2], "snapshot_bytes": h.trial_stats()[2], "begin_end_pair": summary(pairs, 1e6, "us"),
            "begin_and_wait": summary(begins, 1e6, "us"), "end": summary(ends, 1e6, "us")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="1,8,64")
    ap.add_argument("--pivots", default="1,16,63")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    sizes = [int(v) for v in args.rows.split(",") if v.strip()]
    limits = [int(v) for v in args.pivots.split(",") if v.strip()]
    lib = engine.load_library()
    md = dense_le_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"

    def solved(pivots=None):
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)
        if pivots is None:
            oc = t.solve_relaxation()
            assert oc == engine.OPTIMAL, engine.OUTCOME_NAMES.get(oc, oc)
        else:
            assert t.run(1 << 40) == (0, engine.PHASE_ONE_DONE)
            assert t.run(pivots)[0] == pivots
        return t

    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau", "reps": args.reps}
    try:
        os.environ.pop("RELP_TRIAL_MEMCPY", None)
        t = solved()
        pivots = t.iterations()
        result.update(update_block=t.update_block(), primal_pivots=pivots, objective=t.objective_function_value())
        t.close()
        # ---- the rollback, both copies, block open and flushed ----
        result["rollback"] = {}
        for path in ("kernel", "memcpy"):
            if path == "memcpy":
                os.environ["RELP_TRIAL_MEMCPY"] = "1"
            h = solved(pivots)                          # the block is open: no flush since the last full block
            entry = {"open_block": rollback_times(h, args.reps)}
            h.flush()
            entry["flushed"] = rollback_times(h, args.reps)
            result["rollback"][path] = entry
            print(json.dumps({"progress": "rollback", "path": path, "row": entry}), flush=True)
            os.environ.pop("RELP_TRIAL_MEMCPY", None)
            if path == "memcpy":
                h.close()
            else:
                keep = h
        h = keep                                       # the kernel path, flushed
        # ---- strong branching ----
        b, basis = h.b(), h.basis_indices()
        fraction = b - np.floor(b)
        pool = np.flatnonzero((basis < n) & (fraction >= 1e-3) & (fraction <= 1 - 1e-3)).astype(np.int32)
        assert pool.size >= max(sizes), "too few fractional structural rows"
        result["strong_branch"] = []
        for k in sizes:
            for limit in limits:
                rows = pool[:k]
                seconds = timed(lambda: h.strong_branch(rows, limit, away=1e-3), 1, 3)
                objective, outcome, made, status = h.strong_branch(rows, limit, away=1e-3)
                assert (status == engine.BRANCH_EVALUATED).all()
                entry = {"rows": k, "max_pivots": limit, "call": summary(seconds), "per_child_ms": 1e3 * statistics.median(seconds) / (2 * k),
                         "pivots_made": int(made.sum()), "outcomes": {engine.OUTCOME_NAMES[int(o)]: int((outcome == o).sum()) for o in np.unique(outcome)}}
                result["strong_branch"].append(entry)
                print(json.dumps({"progress": "strong_branch", "row": entry}), flush=True)
        # ---- one child by hand: add-cut, pivots, rollback ----
        result["child"] = []
        h.strong_branch(pool[:1], max(limits), away=1e-3)      # (the room and the flush a call makes before its first trial)
        for limit in limits:
            parts = {"begin": [], "add_cut": [], "pivots": [], "objective": [], "rollback": []}
            made = 0
            for r in pool[:8]:
                for side in (0, 1):
                    g = np.zeros((1, n))
                    g[0, basis[r]] = 1.0 if side == 0 else -1.0
                    beta = [np.floor(b[r]) if side == 0 else -np.ceil(b[r])]
                    t0 = time.perf_counter(); h.trial_begin()
                    t1 = time.perf_counter(); h.add_cuts((np.array([0, 1]), np.array([basis[r]]), g[0, basis[r]:basis[r] + 1]), beta)
                    t2 = time.perf_counter(); made += h.run_dual(limit)[0]
                    t3 = time.perf_counter(); h.objective_function_value()
                    t4 = time.perf_counter(); h.trial_end(False)
                    t5 = time.perf_counter()
                    for name, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                        parts[name].append(dt)
            entry = {"max_pivots": limit, "children": 16, "pivots_made": made, **{name: summary(v, 1e6, "us") for name, v in parts.items()}}
            result["child"].append(entry)
            print(json.dumps({"progress": "child", "row": entry}), flush=True)
        # ---- the yardstick: the parent commit's only way back ----
        start = basis.copy()
        seconds = timed(lambda: h.from_basis(start), 1, 3)
        result["from_basis"] = summary(seconds)
        h.close()
    finally:
        lib.relp_device_free(A)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
