"""The case table of launch_tab_gomory (not collected by pytest): tests/test_kernel_models_gomory.py holds the f64 model of every case
to the Fraction model on the CPU, tests/test_gpu_kernels_gomory.py runs the cases on the GPU.  The smallest shapes at which the two
kernels can still go wrong: stored columns 1 / 255 / 256 / 257 (one block, its edge, a second block), list lengths 1 / 7 / 8 / 9
(a chunk, its edge, a second chunk) with a repeated row and descending rows, pending rows 0 / 1 / 8 / 9 / kmax, every load batch, a
kept artificial block in front, basic and barred columns, the special entries of Case (0.0, -0.0, integers, f == f0, f within
tol_zero of 0 and of 1), 0 / 1 / 255 / 256 / 257 / 513 rows of A with a non-basic slack, 1 and 257 structural columns, a bound row,
cut rows, both kinds with continuous columns of either sign."""
import numpy as np

from kernel_harness_gomory import Case


def some_continuous(n):
    flags = np.ones(n, dtype=np.uint8)
    flags[1::3] = 0
    return flags


def columns(n_owned, **kw):
    """20 rows of A (19 slacks): n_owned stored columns."""
    return Case(20, n_owned - 19, [7], 0, **kw)


def slack_rows(k, **kw):
    """520 rows of A, k of them with a non-basic slack; 3 structural columns; two list entries."""
    return Case(520, 3, [400, 17], 0, y_rows=range(1, 1 + k), special=False, **kw)


CASES = {
    "one stored column": lambda: Case(3, 1, [1], 0, mc=0),
    "255 stored columns": lambda: columns(255),
    "256 stored columns": lambda: columns(256),
    "257 stored columns": lambda: columns(257, seed=1),
    "list of 7, descending": lambda: Case(12, 5, [11, 9, 8, 6, 4, 3, 0], 0, seed=2),
    "list of 8, a row twice": lambda: Case(12, 5, [0, 5, 3, 5, 11, 2, 7, 1], 1, seed=3),
    "list of 9": lambda: Case(12, 5, [3, 0, 5, 9, 11, 2, 7, 1, 3], 8, kmax=12, seed=4),
    "p = 9": lambda: Case(12, 5, [4, 10], 9, kmax=12, seed=5),
    "p = kmax": lambda: Case(12, 5, [4, 10, 2], 16, kmax=16, seed=6),
    "artificial block in front": lambda: Case(12, 5, [6, 1], 0, art=3, c_lo=2, seed=7),
    "artificial block, pending rows": lambda: Case(12, 5, [6, 1], 3, art=3, c_lo=2, seed=8),
    "basic and barred columns": lambda: Case(12, 5, [6, 1], 0, basic=(1, 8), barred=(2, 9), seed=9),
    "no row of A with y": lambda: slack_rows(0),
    "1 row of A with y": lambda: slack_rows(1),
    "255 rows of A with y": lambda: slack_rows(255),
    "256 rows of A with y": lambda: slack_rows(256),
    "257 rows of A with y": lambda: slack_rows(257),
    "513 rows of A with y": lambda: slack_rows(513),
    "257 structural columns": lambda: Case(8, 257, [5, 2], 2, seed=10),
    "a bound row": lambda: Case(12, 5, [6, 10], 0, bound_rows=((0, 9), (3, 10)), cuts=1, seed=11),
    "cut rows in A": lambda: Case(12, 5, [6, 11, 10], 1, cuts=2, seed=12),
    "mixed, continuous columns": lambda: Case(12, 5, [6, 1, 3], 0, kind=1, flags=some_continuous, seed=13),
    "mixed, pending rows, bound and cut rows": lambda: Case(14, 6, [6, 1, 13], 4, kind=1, flags=some_continuous, bound_rows=((2, 10),), cuts=3, seed=14),
    "fractional, a continuous column": lambda: Case(12, 5, [6, 1, 3], 0, kind=0, flags=some_continuous, seed=15),
}
BATCH_CASES = {
    "p = 33": lambda batch: Case(12, 5, [4, 10, 2], 33, kmax=40, batch=batch, seed=16),
    "600 rows of A": lambda batch: Case(600, 2, [1], 0, special=False, batch=batch, seed=17),
}
