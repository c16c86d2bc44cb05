"""Cost of taking cut rows and added columns out of a solved LP in place (relp_remove_cuts, relp_remove_columns), and the only route
before these calls -- a fresh engine on the smaller LP with relp_from_basis -- in the same run.

The LP is the dense `<=` LP of scripts/cuts_bench.py (bench.py's dense10k: A generated in HBM by relp_synth_fill_dense) on the tableau
engine at the default update_block, solved to optimality.  Host clock around calls that synchronise; per series two warm-up
repetitions, then the median / min / max of the repetitions; what was removed is added again between repetitions (the room is
reserved once: nothing grows).
  cuts_back  k = 1, 8, 64 loose cuts (G = default_rng(1000 * seed + k).integers(0, 8, (k, n)), beta = 1.5 G x* + 1) added on the flushed
             tableau and removed: their slacks are basic in their own rows, the last k rows and columns -- the short move
  cuts_row0  the same cuts with their slacks pivoted into the tableau rows 0 .. k-1 first (two forced pivots per cut through
             relp_bring_into_basis: a non-basic structural column into the cut's row, the slack into row c; the basis need not stay
             feasible for a timing): the first removed tableau row is 0, so every stored column moves from the top -- the long move.
             The forced pivots leave an update block open, which the removal flushes (`pending_rows`)
  columns    k = 1, 8, 64 added columns (uniform (0, 1) entries, cost +1: they never price out) removed again; the cut slacks of the
             series above are gone, so the columns behind the first removed one are the added columns alone
  rebuild    a fresh engine on the LP (the matrix is already on the device: the cheapest form of this route) and relp_from_basis on
             the optimal basis: create and from_basis timed apart
`entries_moved` is relp_removal_stats()[2]; 16 bytes per entry (one read, one write) is the byte model of DESIGN.md 10.
One JSON line; `--out` also writes it to a file.

    python scripts/remove_bench.py [--m 10000 --n 10000 --seed 20250002] [--sizes 1,8,64] [--reps 20] [--out FILE]
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


def summary(seconds):
    return {"median_ms": 1e3 * statistics.median(seconds), "min_ms": 1e3 * min(seconds), "max_ms": 1e3 * max(seconds), "calls": len(seconds)}


def timed(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    sizes = [int(v) for v in args.sizes.split(",") if v.strip()]
    lib = engine.load_library()
    md = dense_le_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"
    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau"}
    try:
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)
        oc = t.solve_relaxation()
        assert oc == engine.OPTIMAL, engine.OUTCOME_NAMES.get(oc, oc)
        t.flush()
        basis = t.basis_indices()
        x = np.zeros(n)
        for j, v in t.current_bfs():
            if j < n:
                x[j] = v
        result.update(update_block=t.update_block(), primal_pivots=t.iterations(), objective=t.objective_function_value(),
                      stored_columns=t.nr_columns())
        print(json.dumps({"progress": "solved", "pivots": t.iterations()}), flush=True)
        t.reserve_cuts(max(sizes))
        t.reserve_columns(max(sizes))
        cuts = {}
        for k in sizes:
            G = np.random.default_rng(1000 * seed + k).integers(0, 8, (k, n)).astype(float)
            cuts[k] = (G, 1.5 * (G @ x) + 1.0)

        def row(seconds, k, **more):
            stats = t.removal_stats()
            out = summary(seconds[2:])
            out.update(count=k, entries_moved=stats[2], pending_rows=stats[3], model_gb_per_s=16e-9 * stats[2] / statistics.median(seconds[2:]), **more)
            return out

        # ---- cuts at the back, in their own rows ----
        series = []
        for k in sizes:
            seconds = []
            for _ in range(2 + args.reps):
                t.add_cuts(*cuts[k])
                seconds.append(timed(lambda: t.remove_cuts(np.arange(m, m + k, dtype=np.int32))))
            series.append(row(seconds, k))
        result["cuts_back"] = series
        print(json.dumps({"progress": "cuts at the back", "rows": series}), flush=True)

        # ---- columns ----
        series = []
        for k in sizes:
            cols = np.random.default_rng(5000 * seed + k).random((m, k))
            seconds = []
            for _ in range(2 + args.reps):
                first = t.nr_columns()
                t.add_columns(cols, np.ones(k))
                seconds.append(timed(lambda: t.remove_columns(np.arange(first, first + k, dtype=np.int32))))
            series.append(row(seconds, k))
        result["columns"] = series
        print(json.dumps({"progress": "columns", "rows": series}), flush=True)

        # ---- cuts whose slacks sit in the tableau rows 0 .. k-1 ----
        def force(column, r, also=None):
            """pivot `column` into row r if its entry there (and in row `also`) is not tiny"""
            cost = t.relative_cost(column)
            alpha = t.generate_column(column)
            if abs(alpha[r]) < 1e-6 or (also is not None and abs(alpha[also]) < 1e-6):
                return False
            t.bring_into_basis(column, r, cost)
            return True

        series = []
        for k in sizes:
            reps = args.reps if k <= 8 else max(3, args.reps // 4)
            seconds, forced = [], 0
            for _ in range(2 + reps):
                t.add_cuts(*cuts[k])
                in_basis = set(int(j) for j in t.basis_indices())
                free = (j for j in range(n) if j not in in_basis)
                for c in range(k):
                    while not force(next(free), m + c, also=c):   # a non-basic structural column takes the cut's row: the slack leaves
                        pass
                    assert force(n + m + c, c), "the slack has no entry in the row it should enter"
                    forced += 2
                assert t.basis_indices()[:k].tolist() == list(range(n + m, n + m + k))
                seconds.append(timed(lambda: t.remove_cuts(np.arange(m, m + k, dtype=np.int32))))
            series.append(row(seconds, k, forced_pivots=forced))
        result["cuts_row0"] = series
        print(json.dumps({"progress": "cuts in rows 0 ..", "rows": series}), flush=True)
        t.close()

        # ---- the route without these calls: a fresh engine on the smaller LP, warm-started ----
        rebuilds = []
        for _ in range(3):
            t0 = time.perf_counter()
            h = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)
            t1 = time.perf_counter()
            h.from_basis(basis)
            t2 = time.perf_counter()
            rebuilds.append({"create_ms": 1e3 * (t1 - t0), "from_basis_ms": 1e3 * (t2 - t1), "objective": h.objective_function_value()})
            h.close()
        result["fresh_engine_from_basis"] = rebuilds
        fastest = min(r["create_ms"] + r["from_basis_ms"] for r in rebuilds)
        result["rebuild_over_removal"] = {name: [fastest / r["median_ms"] for r in result[name]] for name in ("cuts_back", "cuts_row0", "columns")}
    finally:
        lib.relp_device_free(A)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
