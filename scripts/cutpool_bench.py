"""Cost of separating and adding cuts from a device-resident pool (relp_cutpool_separate, relp_cutpool_add) against what a caller
can do without it: relp_get_b and relp_get_basis_indices, a numpy product over the same CSR on the host, and relp_add_cuts of the
winners.

The LP is the dense `<=` LP of scripts/cuts_bench.py (bench.py's dense10k) on the tableau engine at the default update_block, solved
to optimality and flushed.  Pool cuts: sparse ones with 8 coefficients, one column from each eighth of the structural columns,
dense ones with n; coefficients (1 + r) / 1000; the right-hand side 0.9 g'x* for every other cut (violated at the optimum x*) and
1.1 g'x* + 1 for the rest.  Timed, host clock around calls that synchronise, two warm-up calls, then the median / min / max of
the repetitions:
  separate   relp_cutpool_separate at segments 1 and 64, by slack and by efficacy, over pools of 10^4, 10^5, 10^6 sparse and 10^3
             dense cuts; the bytes the call must read (12 per stored entry, 17 per cut, 8 per structural column, 12 per row) over
             the call's time is the CALL's rate, not the kernel's, and cache-warm for a pool below the 256 MiB of the Infinity Cache
             (the repetitions re-read it back to back); next to it the host route: relp_get_b, relp_get_basis_indices,
             s = rhs - G x by numpy over the CSR, the minimum per share
  add        relp_cutpool_add of k = 1, 8, 64 pool cuts, dense and sparse, room reserved, stacked like scripts/cuts_bench.py (the same
             ids again: an add does not mind an inactive cut); relp_add_cuts of the same cuts on the same handle in the same run; and
             relp_cutpool_add on a handle created under RELP_CUTPOOL_HOST_ADD=1 (the control)
One JSON line; `--out` also writes it to a file, `--md` writes the report.

    python scripts/cutpool_bench.py [--m 10000 --n 10000 --seed 20250002] [--out FILE] [--md FILE]
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


def vertex(t, n):
    b, basis = t.b(), t.basis_indices()
    x = np.zeros(n)
    mask = (basis >= 0) & (basis < n)
    x[basis[mask]] = b[mask]
    return x


def pool_cuts(n, count, entries, seed, x):
    """(row_ptr, col_idx, values), rhs of `count` cuts with `entries` nonzeros each (entries == n: dense)."""
    rng = np.random.default_rng(1000 * seed + count + entries)
    if entries >= n:
        cols = np.tile(np.arange(n, dtype=np.int32), count)
        entries = n
    else:
        stride = n // entries                              # one column from each stratum: distinct and ascending
        cols = (np.arange(entries, dtype=np.int32) * stride + rng.integers(0, stride, (count, entries), dtype=np.int32)).reshape(-1)
    values = (1 + rng.integers(0, 999, cols.size)) / 1000.0
    gx = (values * x[cols]).reshape(count, entries).sum(axis=1)
    rhs = np.where(np.arange(count) % 2 == 0, 0.9 * gx, 1.1 * gx + 1.0)
    return (np.arange(count + 1, dtype=np.int64) * entries, cols, values), rhs


def summary(seconds):
    return {"median_ms": 1e3 * statistics.median(seconds), "min_ms": 1e3 * min(seconds), "max_ms": 1e3 * max(seconds), "calls": len(seconds)}


def timed(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def series(call, reps):
    return summary([timed(call) for _ in range(2 + reps)][2:])


def host_separate(t, n, csr, rhs, entries, segments, tol):
    """The route without a pool: b and the basis from the engine, the product on the host, the minimum of every share."""
    x = vertex(t, n)
    ptr, cols, values = csr
    s = rhs - (values * x[cols]).reshape(-1, entries).sum(axis=1)
    size = (s.size + segments - 1) // segments
    out = []
    for lo in range(0, s.size, size):
        k = int(lo + np.argmin(s[lo:lo + size]))
        if s[k] < -tol:
            out.append(k)
    return out


def fmt(row):
    return f"{row['median_ms']:.3f} ms ({row['min_ms']:.3f} – {row['max_ms']:.3f})"


def report(result):
    lines = ["# Cut pool separated and added in place", "",
             f"`scripts/cutpool_bench.py` (the JSON line is `r24_cutpool.json`), MI355X, one run.  {result['workload']}, tableau engine, "
             f"`update_block` {result['update_block']}, {result['primal_pivots']:,} primal pivots to the optimum {result['objective']!r}, "
             f"{result['basic_structural']:,} structural columns basic, flushed.  Host clock around the Python calls, which synchronise; two "
             f"warm-up calls, then median (min – max) of {result['reps']}.  The rate is the bytes a separation must read (12 per stored "
             "entry, 17 per pool cut, 8 per structural column and 12 per row for the vertex) over the CALL's time -- launches, the wait and "
             f"the download included, not the kernel's time -- against the {HBM_PEAK / 1e12:.1f} TB/s of the data sheet "
             f"({HBM_MEASURED / 1e12:.2f} TB/s is what a copy reaches).  The repetitions separate the same pool back to back, so a pool below "
             "the 256 MiB of the Infinity Cache is read from that cache, not from HBM: its rate is a cache-warm one.  Per-kernel times: "
             "**not measured** here (no kernel trace in this run).", "",
             "## Separation", "",
             "| pool | stored entries | segments | key | `relp_cutpool_separate` | call rate | share of 8 TB/s | host route (`relp_get_b` + "
             "`relp_get_basis_indices` + numpy) | winners |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in result["separate"]:
        host = fmt(r["host"]) if "host" in r else "(as by slack)"
        lines.append(f"| {r['cuts']:,} x {r['entries']} | {r['stored']:,} | {r['segments']} | {'efficacy' if r['by_efficacy'] else 'slack'} | "
                     f"{fmt(r['pool'])} | {r['rate_gbs']:.0f} GB/s | {100 * r['rate_gbs'] * 1e9 / HBM_PEAK:.1f} % | {host} | {r['found']} |")
    lines += ["", "## Adding", "",
              "| cuts | kind | `relp_cutpool_add` | `relp_add_cuts` (same cuts, same handle) | `relp_cutpool_add` under `RELP_CUTPOOL_HOST_ADD=1` | "
              "rows in the union list |",
              "|---|---|---|---|---|---|"]
    for r in result.get("add", []):
        lines.append(f"| {r['cuts']} | {r['kind']} | {fmt(r['pool_add'])} | {fmt(r['add_cuts'])} | {fmt(r['pool_add_host'])} | {r['rows_read']:,} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sparse", default="10000,100000,1000000")
    ap.add_argument("--dense", type=int, default=1000)
    ap.add_argument("--cuts", default="1,8,64")
    ap.add_argument("--separate-only", action="store_true", help="the separation section alone")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    sizes = [int(v) for v in args.cuts.split(",") if v.strip()]
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

    def write(result):
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        if args.md:
            with open(args.md, "w") as f:
                f.write(report(result))

    result = {"workload": f"dense <= {m} x {n}, seed {seed}", "engine": "tableau", "reps": args.reps}
    try:
        t = solved()
        x = vertex(t, n)
        result.update(update_block=t.update_block(), primal_pivots=t.iterations(), objective=t.objective_function_value(),
                      basic_structural=int((t.basis_indices() < n).sum()))
        print(json.dumps({"progress": "solved", "pivots": result["primal_pivots"]}), flush=True)

        shapes = [(int(v), 8) for v in args.sparse.split(",") if v.strip()] + ([(args.dense, n)] if args.dense > 0 else [])
        result["separate"] = []
        for count, entries in shapes:
            csr, rhs = pool_cuts(n, count, entries, seed, x)
            entries = min(entries, n)
            t0 = time.perf_counter()
            pool = t.cut_pool(csr, rhs)
            create = time.perf_counter() - t0
            stats = pool.stats()
            for segments in (1, 64):
                for eff in (False, True):
                    ids, sw = pool.separate(segments, 1e-7, eff)
                    row = {"cuts": count, "entries": entries, "stored": stats[2], "nonzeros": stats[1], "segments": segments, "by_efficacy": eff,
                           "found": int(ids.size), "create_ms": 1e3 * create, "pool": series(lambda: pool.separate(segments, 1e-7, eff), args.reps)}
                    if not eff:                              # (numpy sums in another order: a near-tie may pick a neighbour)
                        row["winners_agree_with_host"] = ids.tolist() == host_separate(t, n, csr, rhs, entries, segments, 1e-7)
                        row["host"] = series(lambda: host_separate(t, n, csr, rhs, entries, segments, 1e-7), max(3, args.reps // 4))
                    row["bytes"] = 12 * stats[2] + 17 * count + 8 * n + 12 * m
                    row["rate_gbs"] = row["bytes"] / (1e-3 * row["pool"]["median_ms"]) / 1e9
                    result["separate"].append(row)
                    print(json.dumps({"progress": "separate", "row": row}), flush=True)
            pool.close()
            del csr, rhs
            write(result)
        if args.separate_only:
            t.close()
            return

        # the adds: a handle as created and a handle created under RELP_CUTPOOL_HOST_ADD=1, the same pools on both
        os.environ["RELP_CUTPOOL_HOST_ADD"] = "1"
        try:
            th = solved()
        finally:
            os.environ.pop("RELP_CUTPOOL_HOST_ADD", None)
        result["add"] = []
        total = 2 * (2 + args.reps) * sum(sizes)             # both kinds
        t.reserve_cuts(2 * total)                            # relp_cutpool_add and relp_add_cuts on this handle
        th.reserve_cuts(total)
        for kind, entries in (("dense", n), ("sparse", 8)):
            csr, rhs = pool_cuts(n, 64, entries, seed + 1, x)
            pools = {h: h.cut_pool(csr, rhs) for h in (t, th)}
            ptr, cols, values = csr
            for k in sizes:
                ids = np.arange(k, dtype=np.int32)
                head = (ptr[:k + 1].copy(), cols[:ptr[k]].copy(), values[:ptr[k]].copy())
                row = {"cuts": k, "kind": kind,
                       "pool_add": series(lambda: pools[t].add(ids), args.reps),
                       "add_cuts": series(lambda: t.add_cuts(head, rhs[:k]), args.reps),
                       "pool_add_host": series(lambda: pools[th].add(ids), args.reps)}
                row["rows_read"] = t.cut_stats()[2]
                result["add"].append(row)
                print(json.dumps({"progress": "add", "row": row}), flush=True)
                write(result)
            for p in pools.values():
                p.close()
        t.close()
        th.close()
    finally:
        lib.relp_device_free(A)
    write(result)


if __name__ == "__main__":
    main()
