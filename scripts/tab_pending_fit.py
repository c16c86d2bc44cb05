"""Duration of the tableau engine's two per-pivot launches against p, the number of pending rows of the update block.

Reads the kernel trace of a `bench.py` run on dense10k (K = 64):

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o NAME -- python bench.py [--steps 2000]
    python scripts/tab_pending_fit.py DIR/NAME_kernel_trace.csv

The launches of `k_tab_ratio_update_all` and `k_tab_select_column` are, in order: one of the empty phase 1, the warm-up
pivots (p = 0 .. warmup-1, then a flush), the timed pivots in blocks of K (p = 0 .. K-1), and one launch that finds the
loop ended.  Per p the median over the whole blocks of the run, then a least-squares line: intercept (the cost at p = 0)
and slope (ns per pending row).  profiles/r06_tab_load_batch.md quotes these fits."""
import argparse
import csv

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", nargs="+")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--series", action="store_true", help="print the median duration for every p")
    args = ap.parse_args()
    K = args.block
    for path in args.trace:
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        print(path)
        for kernel in ("k_tab_ratio_update_all", "k_tab_select_column"):
            d = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]], float)
            first = 1 + args.warmup
            blocks = (len(d) - first - 1) // K
            timed = d[first:first + K * blocks].reshape(blocks, K)
            med = np.median(timed, axis=0)
            A = np.vstack([np.ones(K), np.arange(K)]).T
            (c0, c1), *_ = np.linalg.lstsq(A, med, rcond=None)
            print(f"  {kernel:24s} {len(d)} launches, {blocks} blocks: {c0 / 1000:.2f} us + {c1:.0f} ns * p;  p = 0: {med[0] / 1000:.2f} us,"
                  f"  p = {K - 1}: {med[-1] / 1000:.2f} us,  mean {timed.mean() / 1000:.2f} us")
            if args.series:
                print("   ", " ".join(f"{x / 1000:.1f}" for x in med))


if __name__ == "__main__":
    main()
