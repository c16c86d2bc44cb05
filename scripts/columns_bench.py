"""Cost of adding columns to a solved LP: relp_add_columns (in place) with and without room reserved, the growth itself
(relp_reserve_columns), the relp_run that follows, and the two routes before these calls -- a fresh engine on the wider LP with
relp_from_basis, and relp_generate_column_of per column (B^-1 a alone, nothing added).

The LP is the dense `<=` LP of scripts/cuts_bench.py (bench.py's dense10k: A generated in HBM by relp_synth_fill_dense,
b = n (1000 + r) / 4000, c = -(1000 + r) / 1000) on the tableau engine at the default update_block, solved to optimality.  The new
columns have the statistics of the LP's own: coefficients (1 + r) / 1000, r < 999, cost -(1000 + r) / 1000, from
default_rng(1000 * seed + k); dense (m entries) or sparse (8 entries in random rows).  Timed, host clock around calls that
synchronise, the CSC prepared by the caller:
  add        relp_add_columns of k = 1, 8, 64 columns, dense and sparse, with the room for every repetition reserved beforehand: two
             warm-up calls, then the median / min / max of the repetitions.  The columns stay (scripts/remove_bench.py times taking
             them back): the repetitions stack the same k columns again on the same handle (the basis stays: nothing is run in between); with the update block flushed
             (p = 0) and open (a second engine taken through exactly the pivots of the first)
  growth     relp_reserve_columns on the tableau as created, and the first relp_add_columns of a handle without room (growth + add);
             a rebuild (relp_set_right_hand_side with the rhs in effect) without and with the k columns present
  run        a fresh handle: add (room reserved), then relp_run to the optimum: pivots, seconds, objective
  rebuild    (--rebuild K) the wide LP built on the host, a fresh engine on it and relp_from_basis on the old basis: create (with the
             upload of the matrix) and from_basis timed apart; its relp_run must reach the same optimum
  column_of  relp_generate_column_of of one dense column, per call
One JSON line; `--out` also writes it to a file.

    python scripts/columns_bench.py [--m 10000 --n 10000 --seed 20250002] [--columns 1,8,64] [--rebuild 8] [--out FILE]
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


def new_columns(m, k, seed, entries):
    """(CSC triple, cost, dense m x k) of k new columns with `entries` nonzeros each (entries == m: dense)."""
    rng = np.random.default_rng(1000 * seed + k + (0 if entries == m else 7))
    dense = np.zeros((m, k))
    for c in range(k):
        rows = np.arange(m) if entries >= m else np.sort(rng.choice(m, size=entries, replace=False))
        dense[rows, c] = (1 + rng.integers(0, 999, rows.size)) / 1000.0
    cost = -(1000 + rng.integers(0, 1000, k)) / 1000.0
    cols, rows = np.nonzero(dense.T)
    ptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=k)))).astype(np.int64)
    return (ptr, rows.astype(np.int32), np.ascontiguousarray(dense[rows, cols])), cost, dense


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
    ap.add_argument("--columns", default="1,8,64")
    ap.add_argument("--sparse-entries", type=int, default=8)
    ap.add_argument("--rebuild", type=int, default=8, help="columns of the fresh-engine comparison (0: leave it out)")
    ap.add_argument("--adds-only", action="store_true", help="solve, reserve, three adds per size (a profiler's run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    sizes = [int(v) for v in args.columns.split(",") if v.strip()]
    lib = engine.load_library()
    md = dense_le_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"

    def solved(pivots=None):
        """A handle at the optimum: by solve_relaxation, or (pivots given) by exactly that many phase-2 pivots, block left open."""
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)
        if pivots is None:
            oc = t.solve_relaxation()
            assert oc == engine.OPTIMAL, engine.OUTCOME_NAMES.get(oc, oc)
        else:
            assert t.run(1 << 40) == (0, engine.PHASE_ONE_DONE)
            assert t.run(pivots)[0] == pivots
        return t

    kinds = {"dense": m, "sparse": args.sparse_entries}
    columns = {(name, k): new_columns(m, k, seed, entries) for name, entries in kinds.items() for k in sizes}
    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau"}
    try:
        t = solved()
        pivots, objective, basis = t.iterations(), t.objective_function_value(), t.basis_indices()
        result.update(update_block=t.update_block(), primal_pivots=pivots, objective=objective, stored_columns=t.nr_columns())
        print(json.dumps({"progress": "solved", "pivots": pivots}), flush=True)

        def add_series(h, name, k, reps):
            """2 + reps stacked adds of the same k columns with all their room reserved beforehand."""
            csc, cost, _ = columns[(name, k)]
            h.reserve_columns(h.column_stats()[0] + (2 + reps) * k)
            first = h.nr_columns()
            seconds = [timed(lambda: h.add_columns(csc, cost)) for _ in range(2 + reps)][2:]
            stats = h.column_stats()
            out = summary(seconds)
            out.update(kind=name, columns=k, identity_columns_read=stats[2], pending_rows=stats[3], columns_first=first, columns_last=h.nr_columns(),
                       tile_bytes_read=8 * m * stats[2])
            return out

        if args.adds_only:
            t.flush()
            result["adds"] = [add_series(t, "dense", k, 1) for k in sizes]
            t.close()
            print(json.dumps(result))
            return

        # the adds, block open (a handle taken through the same pivots) and flushed
        h = solved(pivots)
        assert abs(h.objective_function_value() - objective) <= 1e-9 * max(1.0, abs(objective))
        result["add_open_block"] = [add_series(h, name, k, args.reps) for name in kinds for k in sizes]
        h.close()
        print(json.dumps({"progress": "add, block open", "rows": result["add_open_block"]}), flush=True)
        t.flush()
        result["add_flushed"] = [add_series(t, name, k, args.reps) for name in kinds for k in sizes]
        # B^-1 a alone by the route that existed: relp_generate_column_of (downloads B^-1, multiplies on the host)
        dense1 = columns[("dense", sizes[0])][2][:, 0]
        entries = [(int(i), float(dense1[i])) for i in range(m)]
        seconds = [timed(lambda: t.generate_column_of(entries)) for _ in range(3)][1:]
        result["generate_column_of"] = summary(seconds)
        t.close()
        print(json.dumps({"progress": "add, flushed", "rows": result["add_flushed"], "generate_column_of": result["generate_column_of"]}), flush=True)

        # the growth itself, the first add of a handle without room, and the re-solve
        growth = []
        for k in sizes:
            csc, cost, _ = columns[("dense", k)]
            h = solved()
            row = {"columns": k, "reserve_ms": 1e3 * timed(lambda: h.reserve_columns(k)), "room": h.column_stats()[1]}
            row["rebuild_without_columns_ms"] = 1e3 * timed(lambda: h.set_right_hand_side(h.right_hand_side()))
            h.close()
            h = solved()
            row["add_without_room_ms"] = 1e3 * timed(lambda: h.add_columns(csc, cost))
            row["room_after"] = h.column_stats()[1]
            d_new = h.relative_costs()[n + m:]
            t0 = time.perf_counter()
            done, oc = h.run(1 << 40)
            row.update(negative_d=int((d_new < -1e-9).sum()), run_ms=1e3 * (time.perf_counter() - t0), run_pivots=done,
                       outcome=engine.OUTCOME_NAMES.get(oc, oc), objective=h.objective_function_value(), min_b=float(h.b().min()),
                       reinversions=h.reinversions())
            # a rebuild with the k columns present (relp_set_right_hand_side with the rhs in effect: host LU + re-tabulation)
            row["rebuild_with_columns_ms"] = 1e3 * timed(lambda: h.set_right_hand_side(h.right_hand_side()))
            h.close()
            growth.append(row)
            print(json.dumps({"progress": "growth and re-solve", "row": row}), flush=True)
        result["growth_and_resolve"] = growth

        if args.rebuild > 0:
            k = args.rebuild
            _, cost, dense = columns[("dense", k)] if ("dense", k) in columns else new_columns(m, k, seed, m)
            lp = synthetic.dense_lp(m, n, seed)
            wide = MatrixData.from_dense_le(np.asfortranarray(np.hstack([lp["A"], dense])), lp["b"], np.concatenate([lp["c"], cost]))
            basis2 = np.where(basis < n, basis, basis + k).astype(np.int32)
            t0 = time.perf_counter()
            h = engine.Tableau(wide, engine=engine.ENGINE_TABLEAU)
            t1 = time.perf_counter()
            h.from_basis(basis2)
            t2 = time.perf_counter()
            done, oc = h.run(1 << 40)
            row = {"columns": k, "create_with_upload_ms": 1e3 * (t1 - t0), "from_basis_ms": 1e3 * (t2 - t1), "run_pivots": done,
                   "outcome": engine.OUTCOME_NAMES.get(oc, oc), "objective": h.objective_function_value()}
            h.close()
            result["fresh_engine_from_basis"] = row
            print(json.dumps({"progress": "rebuild", "row": row}), flush=True)
    finally:
        lib.relp_device_free(A)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
