"""Cost of adding cut rows to a solved LP: relp_add_cuts (in place) with and without room reserved, the growth itself
(relp_reserve_cuts), the relp_run_dual that follows, and the only route before these calls -- a fresh engine on the longer LP with
relp_from_basis.

The LP is the dense `<=` LP of scripts/cost_bench.py (bench.py's dense10k: A generated in HBM by relp_synth_fill_dense,
b = n (1000 + r) / 4000, c = -(1000 + r) / 1000) on the tableau engine at the default update_block, solved to optimality.  The cuts are
those of tests/test_gpu_cuts_in_place.py: G = default_rng(1000 * seed + k).integers(0, 8, (k, n)), beta = 0.9 G x*; G >= 0 and
b >= 0, so x = 0 satisfies every cut and the stacked LP stays feasible for any k.  Timed, host clock around calls that synchronise:
  add        relp_add_cuts of k = 1, 8, 64, 256 cuts with the room for every repetition reserved beforehand: two warm-up calls, then
             the median / min / max of the repetitions.  The cuts stay (scripts/remove_bench.py times taking them back): the
             repetitions stack the same k cuts again on the same handle: the basis and the list (the basic structural rows G touches) stay, the tableau is k rows and columns
             longer per call (`rows_first`, `rows_last`); with the update block flushed (p = 0) and open (a second engine taken through
             exactly the pivots of the first, scripts/rhs_bench.py says why)
  growth     relp_reserve_cuts on the tableau as created, for every k: one call each on a fresh room (the re-allocation and the
             copies of every buffer), and the first relp_add_cuts of a handle without room (growth + add)
  run_dual   a fresh handle per k: add (room reserved), then relp_run_dual to the optimum: pivots, seconds, objective
  rebuild    (--rebuild K) the stacked LP built on the host, a fresh engine on it and relp_from_basis on the old basis plus the K new
             slacks: create (with the upload of the matrix) and from_basis timed apart; its relp_run_dual must reach the same optimum
One JSON line; `--out` also writes it to a file.

    python scripts/cuts_bench.py [--m 10000 --n 10000 --seed 20250002] [--cuts 1,8,64,256] [--rebuild 8] [--out FILE]
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
    ap.add_argument("--cuts", default="1,8,64,256")
    ap.add_argument("--rebuild", type=int, default=8, help="cuts of the fresh-engine comparison (0: leave it out)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    sizes = [int(v) for v in args.cuts.split(",") if v.strip()]
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

    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau"}
    try:
        t = solved()
        pivots, objective, basis = t.iterations(), t.objective_function_value(), t.basis_indices()
        x = np.zeros(n)
        for j, v in t.current_bfs():
            if j < n:
                x[j] = v
        cuts = {}
        for k in sizes:
            G = np.random.default_rng(1000 * seed + k).integers(0, 8, (k, n)).astype(float)
            cuts[k] = (G, 0.9 * (G @ x))
            assert (G @ x > cuts[k][1]).all()
        result.update(update_block=t.update_block(), primal_pivots=pivots, objective=objective, basic_structural=int((basis < n).sum()),
                      stored_columns=t.nr_columns())
        print(json.dumps({"progress": "solved", "pivots": pivots, "basic_structural": result["basic_structural"]}), flush=True)

        def add_series(h, k, reps):
            """2 + reps stacked adds of the same k cuts with all their room reserved beforehand."""
            G, beta = cuts[k]
            h.reserve_cuts(h.cut_stats()[0] + (2 + reps) * k)
            first = h.nr_rows()
            seconds = [timed(lambda: h.add_cuts(G, beta)) for _ in range(2 + reps)][2:]
            stats = h.cut_stats()
            out = summary(seconds)
            out.update(cuts=k, rows_read=stats[2], pending_rows=stats[3], rows_first=first, rows_last=h.nr_rows())
            return out

        def reps_of(k):
            return args.reps if k <= 64 else max(4, args.reps // 4)

        # the adds, block open (a handle taken through the same pivots) and flushed
        h = solved(pivots)
        assert abs(h.objective_function_value() - objective) <= 1e-9 * max(1.0, abs(objective))
        result["add_open_block"] = [add_series(h, k, reps_of(k)) for k in sizes[:-1]]
        h.close()
        h = solved(pivots)
        result["add_open_block"].append(add_series(h, sizes[-1], reps_of(sizes[-1])))
        h.flush()
        h.close()
        print(json.dumps({"progress": "add, block open", "rows": result["add_open_block"]}), flush=True)
        t.flush()
        result["add_flushed"] = [add_series(t, k, reps_of(k)) for k in sizes[:-1]]
        t.close()
        t = solved()
        t.flush()
        result["add_flushed"].append(add_series(t, sizes[-1], reps_of(sizes[-1])))
        t.close()
        print(json.dumps({"progress": "add, flushed", "rows": result["add_flushed"]}), flush=True)

        # the growth itself, and the first add of a handle without room
        growth = []
        for k in sizes:
            h = solved()
            G, beta = cuts[k]
            row = {"cuts": k, "reserve_ms": 1e3 * timed(lambda: h.reserve_cuts(k)), "room": h.cut_stats()[1]}
            h.close()
            h = solved()
            row["add_without_room_ms"] = 1e3 * timed(lambda: h.add_cuts(G, beta))
            row["room_after"] = h.cut_stats()[1]
            # ... and the re-solve from there
            t0 = time.perf_counter()
            done, oc = h.run_dual(1 << 40)
            row.update(run_dual_ms=1e3 * (time.perf_counter() - t0), run_dual_pivots=done, outcome=engine.OUTCOME_NAMES.get(oc, oc),
                       objective=h.objective_function_value(), min_b=float(h.b().min()), reinversions=h.reinversions())
            h.close()
            growth.append(row)
            print(json.dumps({"progress": "growth and re-solve", "row": row}), flush=True)
        result["growth_and_resolve"] = growth

        if args.rebuild > 0:
            k = args.rebuild
            G = np.random.default_rng(1000 * seed + k).integers(0, 8, (k, n)).astype(float)
            beta = 0.9 * (G @ x)
            lp = synthetic.dense_lp(m, n, seed)
            stacked = MatrixData.from_dense_le(np.asfortranarray(np.vstack([lp["A"], G])), np.concatenate([lp["b"], beta]), lp["c"])
            basis2 = np.concatenate([basis, np.arange(n + m, n + m + k, dtype=np.int32)])
            t0 = time.perf_counter()
            h = engine.Tableau(stacked, engine=engine.ENGINE_TABLEAU)
            t1 = time.perf_counter()
            h.from_basis(basis2)
            t2 = time.perf_counter()
            done, oc = h.run_dual(1 << 40)
            row = {"cuts": k, "create_with_upload_ms": 1e3 * (t1 - t0), "from_basis_ms": 1e3 * (t2 - t1), "run_dual_pivots": done,
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
