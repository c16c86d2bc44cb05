"""Cost of the batched ratio queries of the tableau engine -- relp_row_ratios and relp_rhs_ranging -- beside the only device route
there was before them, in the same process and binary:
  row ratios   a loop of relp_select_dual_pivot_column(row): the down direction alone, two launches, a record download and upload per row
  ranging      relp_generate_column(idcol) + relp_select_primal_pivot_row per row: the decrease direction alone

The LP is the dense `<=` LP of bench.py's dense10k (scripts/rhs_bench.py: A generated in HBM, solved to optimality once per engine) on
the tableau engine at the default update_block.  Timed, host clock around calls that synchronise, two warm-up calls, median / min / max
of the repetitions, for lists of 1, 64, 1,000 and m rows (evenly spread, ascending; m = every row), once with an update block open
(p pending rows: a second engine taken through exactly the pivots the first one needed) and once just flushed (p = 0).  The loops over
1,000 and m rows are repeated `--loop-reps` times after one warm-up pass (a pass over m rows takes seconds).

Byte model of a batched call (what has to cross the memory system at least once; 8-byte entries, 64-byte sectors, chunks of 8 list
entries per workgroup, n_store stored columns, nbc / nbr blocks of 256 columns / rows):
  row ratios   T0: the distinct sectors (row // 8) of every chunk x n_store x 64;  R0: chunks x p x n_store x 8;  d: chunks x n_store x 8
  ranging      T0: entries x m x 8;  W: chunks x p x m x 8;  b: chunks x m x 8
The achieved bytes / s is that model over the median time.  One JSON line; `--out` also writes it to a file.

    python scripts/ranging_bench.py [--m 10000 --n 10000 --seed 20250002] [--out FILE]
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
from rust_lp_amd import engine  # noqa: E402
from scripts.rhs_bench import dense_le_md, summary  # noqa: E402

CHUNK = 8


def timed(call, warmup, reps):
    seconds = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if k >= warmup:
            seconds.append(time.perf_counter() - t0)
    return seconds


def ratio_bytes(rows, p, n_store):
    chunks = [rows[k:k + CHUNK] for k in range(0, len(rows), CHUNK)]
    sectors = sum(len({int(r) // 8 for r in ch}) for ch in chunks)
    return 64 * sectors * n_store + 8 * len(chunks) * (p + 1) * n_store


def ranging_bytes(rows, p, m):
    chunks = (len(rows) + CHUNK - 1) // CHUNK
    return 8 * len(rows) * m + 8 * chunks * (p + 1) * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    lib = engine.load_library()
    md = dense_le_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"

    def solved(pivots=None):
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)
        t0 = time.perf_counter()
        if pivots is None:
            oc = t.solve_relaxation()
            assert oc == engine.OPTIMAL, engine.OUTCOME_NAMES.get(oc, oc)
        else:
            assert t.run(1 << 40) == (0, engine.PHASE_ONE_DONE)
            assert t.run(pivots)[0] == pivots
        return t, time.perf_counter() - t0

    sizes = sorted({1, min(64, m), min(1000, m), m})
    lists = {k: np.arange(m, dtype=np.int32) if k == m else np.linspace(0, m - 1, k).astype(np.int32) for k in sizes}
    n_store = n + m

    def measure(t):
        rows_out = []
        for k in sizes:
            rows = lists[k]
            reps = args.reps if k <= 64 else args.loop_reps
            batched = summary(timed(lambda: t.row_ratios(rows), 2, args.reps))
            p = t.ranging_stats()[3]
            down, down_col, _, _ = t.row_ratios(rows)
            loop = summary(timed(lambda: [t.select_dual_pivot_column(int(r)) for r in rows], 2 if k <= 64 else 1, reps))
            assert [(-1 if c is None else c) for c in (t.select_dual_pivot_column(int(r)) for r in rows[:64])] == down_col[:64].tolist()
            model = ratio_bytes(rows, p, n_store)
            entry = {"rows": k, "pending_rows": p, "row_ratios": batched, "select_dual_pivot_column_loop": loop,
                     "speedup": loop["median_ms"] / batched["median_ms"], "model_bytes": model,
                     "row_ratios_GBps": model / (1e6 * batched["median_ms"])}
            ranged = summary(timed(lambda: t.rhs_ranging(rows), 2, args.reps))

            def stepwise():
                out = []
                for r in rows:
                    t.generate_column(n + int(r))
                    out.append(t.select_primal_pivot_row())
                return out

            loop2 = summary(timed(stepwise, 2 if k <= 64 else 1, reps))
            model2 = ranging_bytes(rows, p, m)
            entry.update({"rhs_ranging": ranged, "generate_column_select_row_loop": loop2,
                          "ranging_speedup": loop2["median_ms"] / ranged["median_ms"], "ranging_model_bytes": model2,
                          "rhs_ranging_GBps": model2 / (1e6 * ranged["median_ms"])})
            rows_out.append(entry)
            print(json.dumps({"progress": entry}), flush=True)
        return rows_out

    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau", "stored_columns": n_store, "chunk": CHUNK}
    try:
        t, solve_s = solved()
        pivots = t.iterations()
        result.update(update_block=t.update_block(), solve_s=solve_s, primal_pivots=pivots, objective=t.objective_function_value())
        print(json.dumps({"progress": "solved", "solve_s": solve_s, "pivots": pivots}), flush=True)
        t.flush()
        result["flushed"] = measure(t)
        t.close()
        t_open, _ = solved(pivots)
        result["open_block"] = measure(t_open)
        assert t_open.run(1 << 40) == (0, engine.OPTIMAL)
        t_open.close()
    finally:
        lib.relp_device_free(A)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
