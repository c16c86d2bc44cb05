"""Fraction of the stored columns each tableau flush skips, over one whole solve of bench.py's dense10k LP.

A flush rewrites only the columns with a nonzero entry among its pending rows R0 (relp_kernels.h: FlushList); the
others are skipped.  This drives the headline's solve (tableau engine, K = 64, the same seeded LP generated in HBM)
K pivots at a time and reads relp_tab_flush_stats after every call.  Writes a markdown report to --out.

    python scripts/flush_skip_profile.py --out profiles/r05_flush_skip_dense10k.md
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rust_lp_amd  # noqa: E402,F401
from rust_lp_amd import MatrixData, engine, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=20250002)
    ap.add_argument("--max-pivots", type=int, default=1 << 20)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    m, n, seed = args.m, args.n, args.seed
    lib = engine.load_library()
    # the host side of bench.py's synthetic LP; A is generated in HBM
    nums_b = n * (1000 + (synthetic.splitmix64(seed, 1, np.arange(m, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    nums_c = -(1000 + (synthetic.splitmix64(seed, 2, np.arange(n, dtype=np.uint64)) % np.uint64(1000)).astype(np.int64))
    md = MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=nums_b / 4000.0, cost=nums_c / 1000.0,
                    upper_bound=np.full(n, np.inf))
    cfg = engine.default_config(poll_interval=1 << 20, engine=engine.ENGINE_TABLEAU)
    A = C.c_void_p()
    assert lib.relp_device_alloc(C.byref(A), 8 * m * n) == 0
    assert lib.relp_synth_fill_dense(A, m, m, n, seed, 0, None) == 0
    t = engine.Tableau(md, config=cfg, device_dense_ptr=A.value, device_dense_ld=m)
    block = t.update_block()
    assert t.run(1)[1] == engine.PHASE_ONE_DONE
    rows, total, last = [], 0, (0, 0)
    t0 = time.perf_counter()
    while total < args.max_pivots:
        done, oc = t.run(block)
        total += done
        st = t.flush_stats()
        if st[0] > last[0]:
            rows.append((total, st[0] - last[0], st[1] - last[1]))
        last = st
        if oc != engine.RUNNING or done == 0:
            break
    dt = time.perf_counter() - t0
    outcome = engine.OUTCOME_NAMES.get(oc, oc)
    t.close()
    lib.relp_device_free(A)

    n_store = m + n
    # flushes whose pending pivots were folded between two reads (one per K pivots in the loop)
    frac = [1.0 - cols / (fl * n_store) for _, fl, cols in rows]
    flushes = sum(fl for _, fl, _ in rows)
    cols = sum(c for _, _, c in rows)
    lines = [f"# Columns skipped by the tableau flush over one dense{m // 1000}k solve", "",
             f"`scripts/flush_skip_profile.py`: bench.py's synthetic LP ({m:,} x {n:,}, seed {seed}, {n_store:,} stored columns), "
             f"tableau engine, K = {block}, from the slack basis to `{outcome}` after {total:,} pivots ({dt:.1f} s with a read "
             f"of the counter every K pivots).  A column is skipped when all of its R0 entries of the block are 0.", "",
             f"* flushes: {flushes:,}; columns rewritten: {cols:,} of {flushes * n_store:,} "
             f"(skipped overall: {1.0 - cols / max(flushes * n_store, 1):.3f})"]
    if frac:
        lines.append(f"* skipped at the first flush {frac[0]:.3f}, at the last {frac[-1]:.3f}")
    lines += ["", "| pivots | flushes | skipped (mean) | skipped (min) | skipped (max) |", "|---:|---:|---:|---:|---:|"]
    step = 2000
    for lo in range(0, total, step):
        sel = [f for (p, _, _), f in zip(rows, frac) if lo < p <= lo + step]
        if sel:
            lines.append(f"| {lo + 1:,}–{min(lo + step, total):,} | {len(sel)} | {np.mean(sel):.3f} | {min(sel):.3f} | {max(sel):.3f} |")
    lines += ["", "Every flush, in order (pivots after it: skipped fraction):", "", "```"]
    per_line = 8
    for k in range(0, len(rows), per_line):
        lines.append("  ".join(f"{p:>6}:{f:.3f}" for (p, _, _), f in zip(rows[k:k + per_line], frac[k:k + per_line])))
    lines.append("```")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"{total} pivots, {flushes} flushes, skipped {1.0 - cols / max(flushes * n_store, 1):.3f}, {dt:.1f} s")


if __name__ == "__main__":
    main()
