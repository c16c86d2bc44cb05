"""Cost of moving the right-hand side of a solved LP: relp_change_right_hand_side (in place) beside relp_set_right_hand_side (the full
re-tabulation), and the relp_run_dual that follows a one-entry change.

The LP is the dense `<=` LP of bench.py's dense10k (A generated in HBM by relp_synth_fill_dense, b = n (1000 + r) / 4000,
c = -(1000 + r) / 1000) on the tableau engine at the default update_block, solved to optimality once per engine.  Timed, host
clock around calls that synchronise, after warm-up calls, median / min / max over the repetitions:
  change   relp_change_right_hand_side with 1, 64 and m entries (every entry moves: the values alternate between b_i and b_i / 2),
           with an open update block (p pending rows) and after relp_flush (p = 0).  A loop that runs to its own end leaves the
           block flushed (it enqueues up to its next poll, and the host counts enqueued iterations towards the flush), so the open
           block comes from a second engine taken through exactly the N pivots the first one needed: N mod update_block are pending
  rebuild  relp_set_right_hand_side with the same alternating vectors
  resolve  a one-entry change of a tight row (its slack is non-basic; to 0.99 b_i, back, to b_i / 2, back) and the relp_run_dual
           that restores optimality each time
`--splits 0,1,6,...` repeats the m-entry change on a fresh engine per value with RELP_TAB_RHS_SPLITS set (0 = the rule of
tab_rhs_splits), which is how the rule was chosen.  One JSON line; `--out` also writes it to a file.

    python scripts/rhs_bench.py [--m 10000 --n 10000 --seed 20250002] [--splits 0,1,3,6,12,25,39] [--out FILE]
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
    return MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=b.astype(np.float64) / 4000.0,
                      cost=c.astype(np.float64) / 1000.0, upper_bound=np.full(n, np.inf))


def summary(seconds):
    return {"median_ms": 1e3 * statistics.median(seconds), "min_ms": 1e3 * min(seconds), "max_ms": 1e3 * max(seconds),
            "calls": len(seconds)}


def alternate(call, values, warmup, reps):
    """call(values[k % 2]) for warmup + reps calls (both even, so the state ends where it began); the seconds of the last reps."""
    seconds = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        call(values[(k + 1) % 2])
        if k >= warmup:
            seconds.append(time.perf_counter() - t0)
    return seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rebuild-reps", type=int, default=4)
    ap.add_argument("--rebuild-seconds", type=float, default=120.0, help="no further rebuild is started after this many seconds of them")
    ap.add_argument("--splits", default="", help="comma-separated RELP_TAB_RHS_SPLITS values for the m-entry change (0 = the rule)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    lib = engine.load_library()
    md = dense_le_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"
    b = np.asarray(md.b, dtype=np.float64)
    half = 0.5 * b

    def solved(pivots=None):
        """A handle at the optimum: by solve_relaxation, or (pivots given) by exactly that many phase-2 pivots, block left open."""
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)
        t0 = time.perf_counter()
        if pivots is None:
            oc = t.solve_relaxation()
            assert oc == engine.OPTIMAL, engine.OUTCOME_NAMES.get(oc, oc)
        else:
            assert t.run(1 << 40) == (0, engine.PHASE_ONE_DONE)
            assert t.run(pivots)[0] == pivots
        return t, time.perf_counter() - t0

    def change_times(t, rows, reps):
        rows = np.asarray(rows, dtype=np.int32)
        seconds = alternate(lambda v: t.change_right_hand_side(rows, v[rows]), (b, half), 2, reps)
        stats = t.rhs_stats()
        out = summary(seconds)
        out.update(entries=len(rows), pending_rows=stats[2], splits=stats[3])
        return out

    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau"}
    try:
        os.environ.pop("RELP_TAB_RHS_SPLITS", None)
        t, solve_s = solved()
        result.update(update_block=t.update_block(), solve_s=solve_s, primal_pivots=t.iterations(),
                      objective=t.objective_function_value())
        print(json.dumps({"progress": "solved", "solve_s": solve_s, "pivots": t.iterations()}), flush=True)
        sizes = sorted({1, min(64, m), m})
        pick = {k: np.arange(m) if k == m else np.linspace(0, m - 1, k).astype(np.int32) for k in sizes}
        pivots, objective = t.iterations(), t.objective_function_value()
        t_open, _ = solved(pivots)
        assert abs(t_open.objective_function_value() - objective) <= 1e-9 * max(1.0, abs(objective))
        result["change_open_block"] = [change_times(t_open, pick[k], args.reps if k < m else max(2, args.reps // 2)) for k in sizes]
        assert t_open.run(1 << 40) == (0, engine.OPTIMAL)
        t_open.close()
        print(json.dumps({"progress": "open block", "change": result["change_open_block"]}), flush=True)

        # the re-solve after a one-entry change: tight rows (slack non-basic), each tightened to 0.99 b_i and to b_i / 2, re-solved,
        # restored, re-solved
        basis = set(t.basis_indices().tolist())
        tight = [i for i in range(m) if n + i not in basis][:2]
        resolves = []
        for row in tight:
            for factor in (0.99, 1.0, 0.5, 1.0):
                t0 = time.perf_counter()
                t.change_right_hand_side([row], [factor * b[row]])
                t1 = time.perf_counter()
                dual_pivots, oc = t.run_dual(1 << 40)
                t2 = time.perf_counter()
                resolves.append({"row": row, "factor": factor, "change_ms": 1e3 * (t1 - t0), "run_dual_ms": 1e3 * (t2 - t1),
                                 "pivots": dual_pivots, "us_per_pivot": 1e6 * (t2 - t1) / max(dual_pivots, 1),
                                 "outcome": engine.OUTCOME_NAMES.get(oc, oc)})
        result["resolve_after_one_entry"] = resolves
        print(json.dumps({"progress": "resolve", "resolves": resolves}), flush=True)

        t.flush()
        result["change_flushed"] = [change_times(t, pick[k], args.reps if k < m else max(2, args.reps // 2)) for k in sizes]
        print(json.dumps({"progress": "flushed", "change": result["change_flushed"]}), flush=True)

        # the full rebuild, last: its host factorisation is the long part
        seconds, spent = [], 0.0
        for k in range(2 + args.rebuild_reps):
            if spent > args.rebuild_seconds:
                break
            t0 = time.perf_counter()
            t.set_right_hand_side((b, half)[(k + 1) % 2])
            dt = time.perf_counter() - t0
            spent += dt
            print(json.dumps({"progress": "rebuild", "call": k, "seconds": dt}), flush=True)
            if k >= 1:
                seconds.append(dt)                          # (the first call is the warm-up)
        result["rebuild"] = summary(seconds) if seconds else None
        result["retab_stats"] = t.retab_stats()
        t.close()

        sweep = []
        for value in [int(v) for v in args.splits.split(",") if v.strip() != ""]:
            if value > 0:
                os.environ["RELP_TAB_RHS_SPLITS"] = str(value)
            else:
                os.environ.pop("RELP_TAB_RHS_SPLITS", None)
            t, _ = solved(pivots)
            row = {"RELP_TAB_RHS_SPLITS": value, "open_block": change_times(t, pick[m], max(2, args.reps // 2))}
            t.flush()
            row["flushed"] = change_times(t, pick[m], max(2, args.reps // 2))
            t.close()
            sweep.append(row)
            print(json.dumps({"progress": "splits", "row": row}), flush=True)
        os.environ.pop("RELP_TAB_RHS_SPLITS", None)
        if sweep:
            result["splits_sweep"] = sweep
    finally:
        lib.relp_device_free(A)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
