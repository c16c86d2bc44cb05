"""Cost of moving the objective of a solved LP: relp_change_cost (in place) beside relp_set_cost (flush + reprice) and a fresh engine
with relp_from_basis (the only route before these calls).

The LP is the dense `<=` LP of scripts/rhs_bench.py (bench.py's dense10k: A generated in HBM by relp_synth_fill_dense,
b = n (1000 + r) / 4000, c = -(1000 + r) / 1000) on the tableau engine at the default update_block, solved to optimality once per
engine.  Timed, host clock around calls that synchronise, after warm-up calls, median / min / max over the repetitions:
  change   relp_change_cost with 1, 64, 1,000 and all basic structural columns (evenly spaced picks of the basic structural columns in
           row order; every entry moves: the values alternate between c_j and c_j / 2), with an open update block (p pending rows)
           and after relp_flush (p = 0).  The open block comes from a second engine taken through exactly the N pivots the first one
           needed (scripts/rhs_bench.py says why)
  set      relp_set_cost with the same alternating vectors on the flushed handle (no flush inside), and alternating between c and c
           reversed with three pivots run between the calls, so that every call flushes a block of at most three rows first
  rebuild  a fresh engine with the new costs + relp_from_basis on the same basis
`--splits 0,1,2,...` repeats the changes on a fresh engine per value with RELP_TAB_COST_SPLITS set (0 = the rule of tab_cost_splits),
which is how the rule was chosen.  One JSON line; `--out` also writes it to a file.

    python scripts/cost_bench.py [--m 10000 --n 10000 --seed 20250002] [--splits 0,1,2,4,8,16] [--out FILE]
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


def dense_le_md(m, n, seed, cost=None):
    b = n * (1000 + (synthetic.splitmix64(seed, 1, np.arange(m, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    c = -(1000 + (synthetic.splitmix64(seed, 2, np.arange(n, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    return MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=b.astype(np.float64) / 4000.0,
                      cost=c.astype(np.float64) / 1000.0 if cost is None else np.asarray(cost, dtype=np.float64),
                      upper_bound=np.full(n, np.inf))


def summary(seconds):
    return {"median_ms": 1e3 * statistics.median(seconds), "min_ms": 1e3 * min(seconds), "max_ms": 1e3 * max(seconds),
            "calls": len(seconds)}


def alternate(call, values, warmup, reps, between=None):
    """call(values[k % 2]) for warmup + reps calls (both even, so the costs end where they began); the seconds of the last reps."""
    seconds = []
    for k in range(warmup + reps):
        if between:
            between()
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
    ap.add_argument("--rebuild-reps", type=int, default=2)
    ap.add_argument("--splits", default="", help="comma-separated RELP_TAB_COST_SPLITS values (0 = the rule)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    lib = engine.load_library()
    md = dense_le_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"
    c = np.asarray(md.cost, dtype=np.float64)
    half = 0.5 * c

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

    def change_times(t, cols, reps):
        cols = np.asarray(cols, dtype=np.int32)
        d0 = t.relative_costs()
        seconds = alternate(lambda v: t.change_cost(cols, v[cols]), (c, half), 2, reps)
        stats = t.cost_stats()
        out = summary(seconds)
        out.update(entries=len(cols), pending_rows=stats[2], splits=stats[3],
                   drift_after_the_round_trips=float(np.abs(t.relative_costs() - d0).max()))
        return out

    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau"}
    try:
        os.environ.pop("RELP_TAB_COST_SPLITS", None)
        t, solve_s = solved()
        pivots, objective = t.iterations(), t.objective_function_value()
        basis = t.basis_indices()
        basic = basis[basis < n]                            # the basic structural columns, in row order
        result.update(update_block=t.update_block(), solve_s=solve_s, primal_pivots=pivots, objective=objective,
                      basic_structural=len(basic), stored_columns=t.nr_columns())
        print(json.dumps({"progress": "solved", "solve_s": solve_s, "pivots": pivots, "basic_structural": len(basic)}), flush=True)
        sizes = sorted({1, min(64, len(basic)), min(1000, len(basic)), len(basic)})
        pick = {k: basic if k == len(basic) else basic[np.linspace(0, len(basic) - 1, k).astype(np.int64)] for k in sizes}

        def reps_of(k):
            return args.reps if k < 1000 else max(2, args.reps // 2)

        def both_states(splits_value):
            """The changes on a fresh pair of states: block open (a handle taken through the same pivots), then flushed."""
            h, _ = solved(pivots)
            assert abs(h.objective_function_value() - objective) <= 1e-9 * max(1.0, abs(objective))
            row = {"RELP_TAB_COST_SPLITS": splits_value, "open_block": [change_times(h, pick[k], reps_of(k)) for k in sizes]}
            h.flush()
            row["flushed"] = [change_times(h, pick[k], reps_of(k)) for k in sizes]
            row["run_after"] = list(h.run(1 << 40))            # (pivots, outcome): the costs are back where they began
            h.close()
            return row

        row = both_states(0)
        result["change_open_block"], result["change_flushed"] = row["open_block"], row["flushed"]
        print(json.dumps({"progress": "change", "row": row}), flush=True)

        # relp_set_cost: on the flushed handle, then with three pivots between the calls (every call flushes them first)
        t.flush()
        result["set_cost_flushed"] = summary(alternate(t.set_cost, (c, half), 2, reps_of(n)))
        assert t.run(1 << 40) == (0, engine.OPTIMAL)
        before = t.flush_stats()[0]
        rev = np.ascontiguousarray(c[::-1])                 # (c / 2 has the optimum of c: no pivot would follow it)
        result["set_cost_with_flush"] = summary(alternate(t.set_cost, (c, rev), 2, reps_of(n), between=lambda: t.run(3)))
        result["set_cost_with_flush"]["flushes"] = t.flush_stats()[0] - before
        t.set_cost(c)
        assert t.run(1 << 40)[1] == engine.OPTIMAL
        print(json.dumps({"progress": "set_cost", "flushed": result["set_cost_flushed"], "with_flush": result["set_cost_with_flush"]}),
              flush=True)
        basis = t.basis_indices()
        t.close()

        # the only route before: a fresh engine with the new costs, warm-started on the basis (host LU + one FTRAN per stored column)
        seconds = []
        for k in range(1 + args.rebuild_reps):
            t0 = time.perf_counter()
            h = engine.Tableau(dense_le_md(m, n, seed, cost=(half, c)[k % 2]), engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value,
                               device_dense_ld=m)
            h.from_basis(basis)
            dt = time.perf_counter() - t0
            h.close()
            print(json.dumps({"progress": "rebuild", "call": k, "seconds": dt}), flush=True)
            if k >= 1:
                seconds.append(dt)                          # (the first call is the warm-up)
        result["fresh_engine_from_basis"] = summary(seconds) if seconds else None

        sweep = []
        for value in [int(v) for v in args.splits.split(",") if v.strip() != ""]:
            if value > 0:
                os.environ["RELP_TAB_COST_SPLITS"] = str(value)
            else:
                os.environ.pop("RELP_TAB_COST_SPLITS", None)
            row = both_states(value)
            sweep.append(row)
            print(json.dumps({"progress": "splits", "row": row}), flush=True)
        os.environ.pop("RELP_TAB_COST_SPLITS", None)
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
