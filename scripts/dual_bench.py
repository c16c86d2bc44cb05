"""Time to optimum of the dual simplex loop against the two-phase primal on one covering LP (min c'x, A x >= b, c > 0).

The LP has the numbers of `synthetic.dense_numerators(m, n, seed)`: A = A_num / 1000 (generated in HBM by relp_synth_fill_dense),
b = b_num / 4000, c = -c_num / 1000, all rows `>=`.  On the tableau engine at the default update_block, after a warm-up engine,
in one process:
  dual    relp_from_basis(surplus slacks) + relp_run_dual to the optimum
  primal  relp_solve_relaxation from a fresh engine (phase 1 over m artificial variables, phase 2)
and one JSON line with pivots, wall time, iterations/s and both objectives.  `--legs dual` runs the dual leg alone (for a kernel
trace of its own: rocprofv3 --kernel-trace --stats -- python scripts/dual_bench.py --legs dual).  `--primal-seconds` caps the primal
leg: a leg that hits it is reported with "finished": false and the pivots it made.

    python scripts/dual_bench.py [--m 10000 --n 10000 --seed 20250002] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rust_lp_amd  # noqa: E402,F401
from rust_lp_amd import MatrixData, engine, synthetic  # noqa: E402


def covering_md(m, n, seed):
    b = n * (1000 + (synthetic.splitmix64(seed, 1, np.arange(m, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    c = 1000 + (synthetic.splitmix64(seed, 2, np.arange(n, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64)
    return MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=0, nr_ge=m, b=b.astype(np.float64) / 4000.0,
                      cost=c.astype(np.float64) / 1000.0, upper_bound=np.full(n, np.inf))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--legs", default="dual,primal")
    ap.add_argument("--primal-seconds", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=256, help="pivots of the warm-up engine per leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    legs = args.legs.split(",")
    lib = engine.load_library()
    md = covering_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"
    slacks = np.arange(n, n + m, dtype=np.int32)

    def fresh():
        return engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)

    result = {"workload": f"covering {m} x {n}, seed {seed}", "engine": "tableau"}
    try:
        # warm-up engine: code objects loaded, allocator warm, both loops entered once
        t = fresh()
        result["update_block"] = t.update_block()
        if "primal" in legs:
            t.run(args.warmup)
        t.from_basis(slacks)
        t.run_dual(args.warmup)
        t.close()

        if "dual" in legs:
            t = fresh()
            t0 = time.perf_counter()
            t.from_basis(slacks)
            t1 = time.perf_counter()
            pivots, oc = t.run_dual(1 << 40)
            t2 = time.perf_counter()
            result["dual"] = {"outcome": engine.OUTCOME_NAMES.get(oc, oc), "finished": oc == engine.OPTIMAL, "pivots": pivots,
                              "from_basis_s": t1 - t0, "run_dual_s": t2 - t1, "wall_s": t2 - t0,
                              "iterations_per_s": pivots / max(t2 - t1, 1e-12), "objective": t.objective_function_value(),
                              "min_b": float(t.b().min())}
            t.close()

        if "primal" in legs:
            t = fresh()
            t0 = time.perf_counter()
            pivots, oc, phase_one = 0, engine.RUNNING, None
            while time.perf_counter() - t0 < args.primal_seconds:
                done, oc = t.run(20000)
                pivots += done
                if oc == engine.PHASE_ONE_DONE:
                    phase_one = {"pivots": pivots, "s": time.perf_counter() - t0}
                elif oc != engine.RUNNING:
                    break
            t1 = time.perf_counter()
            result["primal"] = {"outcome": engine.OUTCOME_NAMES.get(oc, oc), "finished": oc == engine.OPTIMAL, "pivots": pivots,
                                "phase_one": phase_one, "wall_s": t1 - t0, "iterations_per_s": pivots / max(t1 - t0, 1e-12),
                                "objective": t.objective_function_value() if t.phase == 2 else None}
            t.close()
        if "dual" in result and "primal" in result and result["primal"]["finished"] and result["dual"]["finished"]:
            result["primal_over_dual_wall"] = result["primal"]["wall_s"] / result["dual"]["wall_s"]
            ref = result["primal"]["objective"]
            result["objective_relative_difference"] = abs(result["dual"]["objective"] - ref) / max(1.0, abs(ref))
    finally:
        lib.relp_device_free(A)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
