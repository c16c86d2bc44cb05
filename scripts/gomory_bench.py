"""Cost of relp_gomory_cuts beside the only route there was before it: relp_generate_column of every non-basic column (the rows of T
read off the downloaded columns) plus the rule and the substitution of the slacks on the host in numpy.

The LP is the dense `<=` LP of scripts/cuts_bench.py (bench.py's dense10k: A generated in HBM by relp_synth_fill_dense) on the
tableau engine at the default update_block, solved to optimality.  The rows: the first k rows of the optimum whose fraction lies in
[0.001, 0.999], k = 1, 8, 64; all columns count as integer (the data is not: the cuts are timed, not used).  Timed, host clock around
calls that synchronise:
  batched    relp_gomory_cuts: two warm-up calls, then the median / min / max of --reps calls, with the update block flushed (p = 0)
             and open (a second engine taken through exactly the pivots of the first, scripts/rhs_bench.py says why)
  host       once per block state: relp_generate_column of every non-basic column (timed as one loop), then per k the numpy
             rule and substitution (median of 3); the host's A comes from synthetic.dense_lp (the same numbers)
The largest difference between the two routes' coefficients is reported per k.  --calls-only leaves the host route out (the run
under a kernel trace).  One JSON line; `--out` also writes it to a file.

    python scripts/gomory_bench.py [--m 10000 --n 10000 --seed 20250002] [--rows 1,8,64] [--reps 10] [--calls-only] [--out FILE]
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

TOL_ZERO = 1e-11


def dense_le_md(m, n, seed):
    b = n * (1000 + (synthetic.splitmix64(seed, 1, np.arange(m, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    c = -(1000 + (synthetic.splitmix64(seed, 2, np.arange(n, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    return MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=b.astype(np.float64) / 4000.0, cost=c.astype(np.float64) / 1000.0,
                      upper_bound=np.full(n, np.inf))


def summary(seconds):
    return {"median_ms": 1e3 * statistics.median(seconds), "min_ms": 1e3 * min(seconds), "max_ms": 1e3 * max(seconds), "calls": len(seconds)}


def timed(call, warm, reps):
    for _ in range(warm):
        call()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


def host_cuts(E, f0, nonbasic, A, b, n, m):
    """The fractional rule on the entries E (k x non-basic columns) and the substitution of the <= slacks: g = -pi_x + A' y,
    beta = -f0 + y' b (plain numpy sums)."""
    f = E - np.floor(E)
    pi = np.where((np.abs(E) <= TOL_ZERO) | (f <= TOL_ZERO) | (f >= 1.0 - TOL_ZERO), 0.0, f)
    full = np.zeros((E.shape[0], n + m))
    full[:, nonbasic] = pi
    y = full[:, n:]
    return y @ A - full[:, :n], y @ b - f0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rows", default="1,8,64")
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    sizes = [int(v) for v in args.rows.split(",") if v.strip()]
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
        t = solved()
        pivots = t.iterations()
        lp = None if args.calls_only else synthetic.dense_lp(m, n, seed)
        result.update(update_block=t.update_block(), primal_pivots=pivots, objective=t.objective_function_value())
        for label in ("flushed", "open_block"):
            if label == "flushed":
                h = t
                h.flush()
            else:
                h = solved(pivots)
            b, basis = h.b(), h.basis_indices()
            fraction = b - np.floor(b)
            pool = np.flatnonzero((fraction >= 1e-3) & (fraction <= 1 - 1e-3)).astype(np.int32)
            assert pool.size >= max(sizes), "too few fractional rows"
            rows_out = []
            columns = None
            if not args.calls_only:
                in_basis = np.zeros(n + m, dtype=bool)
                in_basis[basis[basis < n + m]] = True
                nonbasic = np.flatnonzero(~in_basis)
                t0 = time.perf_counter()
                columns = np.stack([h.generate_column(int(j)) for j in nonbasic], axis=1)      # m x non-basic columns
                generate_s = time.perf_counter() - t0
            for k in sizes:
                rows = pool[:k]
                batched = summary(timed(lambda: h.gomory_cuts(rows, away=1e-3), 2, args.reps))
                G, rhs, f0, status = h.gomory_cuts(rows, away=1e-3)
                assert (status == engine.GOMORY_CUT).all()
                entry = {"rows": k, "pending_rows": h.gomory_stats()[3], "gomory_cuts": batched}
                if columns is not None:
                    E = columns[rows]
                    host = summary(timed(lambda: host_cuts(E, f0, nonbasic, lp["A"], lp["b"], n, m), 0, 3))
                    Gh, rh = host_cuts(E, f0, nonbasic, lp["A"], lp["b"], n, m)
                    entry.update(generate_columns_ms=1e3 * generate_s, columns_generated=int(nonbasic.size), host_substitution=host,
                                 host_route_ms=1e3 * generate_s + host["median_ms"],
                                 speedup=(1e3 * generate_s + host["median_ms"]) / batched["median_ms"],
                                 max_abs_coefficient_difference=float(np.abs(G - Gh).max()), max_abs_rhs_difference=float(np.abs(rhs - rh).max()))
                rows_out.append(entry)
                print(json.dumps({"progress": label, "row": entry}), flush=True)
            result[label] = rows_out
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
