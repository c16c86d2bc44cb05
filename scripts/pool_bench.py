"""Cost of pricing and adding columns from a device-resident pool (relp_pool_price, relp_pool_add) against what a caller can do
without it: relp_get_minus_pi, a numpy product over the same CSC on the host, and relp_add_columns of the winners.

The LP is the dense `<=` LP of scripts/columns_bench.py (bench.py's dense10k) on the tableau engine at the default update_block,
solved to optimality and flushed.  Pool columns have the statistics of the LP's own (scripts/columns_bench.py: coefficients
(1 + r) / 1000, cost -(1000 + r) / 1000): sparse ones with 8 coefficients, one row from each eighth of the rows, dense ones with m.
Timed, host clock around calls that synchronise, two warm-up calls, then the median / min / max of the repetitions:
  price      relp_pool_price at segments 1 and 64 over pools of 10^4, 10^5, 10^6 sparse and 10^3 dense columns; the bytes the call must
             read (12 per stored entry, 9 per column) over the call's time is the CALL's rate, not the kernel's, and cache-warm for a
             pool below the 256 MiB of the Infinity Cache (the repetitions re-read it back to back); next to it the host
             route: relp_get_minus_pi, d = c + A' (-pi) by numpy over the CSC, the minimum per share
  add        relp_pool_add of k = 1, 8, 64 pool columns, dense and sparse, room reserved, stacked like scripts/columns_bench.py (the same
             ids again: an add does not mind an inactive column); relp_add_columns of the same columns on the same handle in the same
             run; and relp_pool_add on a handle created under RELP_POOL_HOST_ADD=1 (the control)
  --trace    pricing only, a few calls per pool (a kernel trace's run)
One JSON line; `--out` also writes it to a file, `--md` writes the report.

    python scripts/pool_bench.py [--m 10000 --n 10000 --seed 20250002] [--out FILE] [--md FILE]
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
from scripts.columns_bench import dense_le_md  # noqa: E402

HBM_PEAK = 8.0e12             # bytes per second, the data sheet's figure
HBM_MEASURED = 6.29e12        # what a float4 copy reaches


def pool_columns(m, count, entries, seed):
    """(col_ptr, row_idx, values), cost of `count` columns with `entries` nonzeros each (entries == m: dense)."""
    rng = np.random.default_rng(1000 * seed + count + entries)
    if entries >= m:
        rows = np.tile(np.arange(m, dtype=np.int32), count)
        entries = m
    else:
        stride = m // entries                              # one row from each stratum: distinct and ascending
        rows = (np.arange(entries, dtype=np.int32) * stride + rng.integers(0, stride, (count, entries), dtype=np.int32)).reshape(-1)
    values = (1 + rng.integers(0, 999, rows.size)) / 1000.0
    cost = -(1000 + rng.integers(0, 1000, count)) / 1000.0
    return (np.arange(count + 1, dtype=np.int64) * entries, rows, values), cost


def summary(seconds):
    return {"median_ms": 1e3 * statistics.median(seconds), "min_ms": 1e3 * min(seconds), "max_ms": 1e3 * max(seconds), "calls": len(seconds)}


def timed(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def series(call, reps):
    return summary([timed(call) for _ in range(2 + reps)][2:])


def host_price(t, csc, cost, entries, segments):
    """The route without a pool: -pi from the engine, the product on the host, the minimum of every share."""
    mpi = t.minus_pi()
    ptr, rows, values = csc
    d = cost + (mpi[rows] * values).reshape(-1, entries).sum(axis=1)
    size = (d.size + segments - 1) // segments
    return [int(lo + np.argmin(d[lo:lo + size])) for lo in range(0, d.size, size)]


def fmt(row):
    return f"{row['median_ms']:.3f} ms ({row['min_ms']:.3f} – {row['max_ms']:.3f})"


def report(result):
    lines = ["# Column pool priced and added in place", "",
             f"`scripts/pool_bench.py` (the JSON line is `r23_pool.json`), MI355X, one run.  {result['workload']}, tableau engine, `update_block` "
             f"{result['update_block']}, {result['primal_pivots']:,} primal pivots to the optimum {result['objective']!r}, flushed.  Host clock "
             "around the Python calls, which synchronise; two warm-up calls, then median (min – max) of "
             f"{result['reps']}.  The rate is the bytes a price must read (12 per stored entry, 9 per pool column) over the CALL's time "
             f"-- launches, the wait and the download included, not the kernel's time -- against the {HBM_PEAK / 1e12:.1f} TB/s of the data "
             f"sheet ({HBM_MEASURED / 1e12:.2f} TB/s is what a copy reaches).  The repetitions price the same pool back to back, so a pool below the "
             "256 MiB of the Infinity Cache is read from that cache, not from HBM: its rate is a cache-warm one.  Per-kernel times: **not measured** here (no kernel trace in this run).", "",
             "## Pricing", "",
             "| pool | stored entries | segments | `relp_pool_price` | call rate | share of 8 TB/s | host route (`relp_get_minus_pi` + numpy) | winners |",
             "|---|---|---|---|---|---|---|---|"]
    for r in result["price"]:
        lines.append(f"| {r['columns']:,} x {r['entries']} | {r['stored']:,} | {r['segments']} | {fmt(r['pool'])} | {r['rate_gbs']:.0f} GB/s | "
                     f"{100 * r['rate_gbs'] * 1e9 / HBM_PEAK:.1f} % | {fmt(r['host'])} | {r['found']} |")
    lines += ["", "## Adding", "",
              "| columns | kind | `relp_pool_add` | `relp_add_columns` (same columns, same handle) | `relp_pool_add` under `RELP_POOL_HOST_ADD=1` |",
              "|---|---|---|---|---|"]
    for r in result["add"]:
        lines.append(f"| {r['columns']} | {r['kind']} | {fmt(r['pool_add'])} | {fmt(r['add_columns'])} | {fmt(r['pool_add_host'])} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sparse", default="10000,100000,1000000")
    ap.add_argument("--dense", type=int, default=1000)
    ap.add_argument("--columns", default="1,8,64")
    ap.add_argument("--trace", action="store_true", help="pricing only, three calls per pool and segment count")
    ap.add_argument("--price-only", action="store_true", help="the pricing section alone (a pool beyond the Infinity Cache: --sparse 4000000 --dense 0)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    sizes = [int(v) for v in args.columns.split(",") if v.strip()]
    lib = engine.load_library()
    md = dense_le_md(m, n, seed)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0, "device allocation failed"
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0, "synthetic fill failed"

    def solved():
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, device_dense_ptr=A.value, device_dense_ld=m)
        oc = t.solve_relaxation()
        assert oc == engine.OPTIMAL, engine.OUTCOME_NAMES.get(oc, oc)
        t.flush()
        return t

    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau", "reps": args.reps}
    try:
        t = solved()
        result.update(update_block=t.update_block(), primal_pivots=t.iterations(), objective=t.objective_function_value())
        print(json.dumps({"progress": "solved", "pivots": result["primal_pivots"]}), flush=True)

        shapes = [(int(v), 8) for v in args.sparse.split(",") if v.strip()] + ([(args.dense, m)] if args.dense > 0 else [])
        result["price"] = []
        for count, entries in shapes:
            csc, cost = pool_columns(m, count, entries, seed)
            t0 = time.perf_counter()
            pool = t.pool(csc, cost)
            create = time.perf_counter() - t0
            stats = pool.stats()
            d = pool.reduced_costs()
            for segments in (1, 64):
                ids, dw = pool.price(segments, 1e-7)
                want = host_price(t, csc, cost, min(entries, m), segments)
                want = [k for k in want if d[k] < -1e-7]
                agree = ids.tolist() == want                 # (numpy sums in another order: a near-tie may pick a neighbour)
                reps = 3 if args.trace else args.reps
                row = {"columns": count, "entries": min(entries, m), "stored": stats[2], "nonzeros": stats[1], "segments": segments, "found": int(ids.size), "winners_agree_with_host": agree,
                       "create_ms": 1e3 * create, "pool": series(lambda: pool.price(segments, 1e-7), reps)}
                row["bytes"] = 12 * stats[2] + 9 * count
                row["rate_gbs"] = row["bytes"] / (1e-3 * row["pool"]["median_ms"]) / 1e9
                if not args.trace:
                    row["host"] = series(lambda: host_price(t, csc, cost, min(entries, m), segments), max(3, args.reps // 4))
                result["price"].append(row)
                print(json.dumps({"progress": "price", "row": row}), flush=True)
            pool.close()
            del csc, cost
        if args.trace or args.price_only:
            t.close()
            print(json.dumps(result))
            if args.out:
                with open(args.out, "w") as f:
                    f.write(json.dumps(result) + "\n")
            return

        # the adds: a handle as created and a handle created under RELP_POOL_HOST_ADD=1, the same pools on both
        os.environ["RELP_POOL_HOST_ADD"] = "1"
        try:
            th = solved()
        finally:
            os.environ.pop("RELP_POOL_HOST_ADD", None)
        result["add"] = []
        for kind, entries in (("dense", m), ("sparse", 8)):
            csc, cost = pool_columns(m, 64, entries, seed + 1)
            pools = {h: h.pool(csc, cost) for h in (t, th)}
            ptr, rows, values = csc
            for k in sizes:
                ids = np.arange(k, dtype=np.int32)
                head = (ptr[:k + 1].copy(), rows[:ptr[k]].copy(), values[:ptr[k]].copy())
                for h in (t, th):
                    h.reserve_columns(h.column_stats()[0] + 2 * (2 + args.reps) * k)
                row = {"columns": k, "kind": kind,
                       "pool_add": series(lambda: pools[t].add(ids), args.reps),
                       "add_columns": series(lambda: t.add_columns(head, cost[:k]), args.reps),
                       "pool_add_host": series(lambda: pools[th].add(ids), args.reps)}
                row["identity_columns_read"] = t.column_stats()[2]
                result["add"].append(row)
                print(json.dumps({"progress": "add", "row": row}), flush=True)
            for p in pools.values():
                p.close()
        t.close()
        th.close()
    finally:
        lib.relp_device_free(A)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write(report(result))


if __name__ == "__main__":
    main()
