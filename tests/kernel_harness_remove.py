"""Helper module of the kernel tests of the rows and columns removed in place (not collected by pytest): the calls of
tests/kernels/harness_remove.cpp (through tests/kernel_harness.py) (one launch_tab_compact on an image the test constructs) and the list of cases the
CPU model test and the GPU test share.  The reference and the in-place model are in tests/remove_reference.py.

A case is (m, n, rows, cols): m x n live entries in an image with 3 room rows (pitch rounded up to even) and 2 room columns, all
sentinels.  "moved" below = the surviving rows below the first removed one, the rows k_tab_drop_rows copies: the chunk of a launch
is 256 B of them, B = 4 as shipped or 1."""
from __future__ import annotations

import numpy as np

import kernel_harness as kh
import remove_reference as rr

BATCHES = (rr.SHIPPED_B, 1)


def _one_row(moved, above=3):
    """one removed row with `above` rows over it and `moved` rows under it"""
    return dict(m=above + 1 + moved, n=5, rows=[above], cols=[])


CASES = {f"{moved} moved rows": _one_row(moved) for moved in (1, 255, 256, 257, 515, 1023, 1025, 2051)}
CASES.update({
    "the first row": dict(m=300, n=4, rows=[0], cols=[]),
    "the last row": dict(m=300, n=4, rows=[299], cols=[]),
    "two adjacent rows": dict(m=1100, n=3, rows=[40, 41], cols=[]),
    "every other row of the last 9": dict(m=530, n=3, rows=[521, 523, 525, 527, 529], cols=[]),
    "70 scattered rows": dict(m=1400, n=3, rows=sorted(set(range(5, 1400, 20))), cols=[]),
    "every row": dict(m=9, n=3, rows=list(range(9)), cols=[]),
    "more columns than workgroups": dict(m=40, n=2100, rows=[7, 30], cols=[]),
    "the first column of the tail, 63 rows": dict(m=63, n=30, rows=[], cols=[20]),
    "the last column, 64 rows": dict(m=64, n=30, rows=[], cols=[29]),
    "adjacent columns, 65 rows": dict(m=65, n=30, rows=[], cols=[21, 22]),
    "one column, 257 rows": dict(m=257, n=40, rows=[], cols=[31]),
    "8 columns at once": dict(m=65, n=40, rows=[], cols=[20, 22, 23, 27, 30, 31, 32, 39]),
    "9 columns at once": dict(m=257, n=40, rows=[], cols=[0, 20, 22, 23, 27, 30, 31, 32, 38]),
    "every column": dict(m=10, n=6, rows=[], cols=list(range(6))),
    "rows and columns together": dict(m=1290, n=37, rows=[2, 3, 700, 1289], cols=[5, 30, 31, 36]),
    "a cut at the back: its row and its slack": dict(m=65, n=131, rows=[64], cols=[130]),
    "nothing": dict(m=20, n=6, rows=[], cols=[]),
})


def image_of(case, seed=0):
    m, n = case["m"], case["n"]
    return rr.sentinel_image(np.random.default_rng(seed), m, n, kh.round_up(m + 3, 2), n + 2, kh.SENTINEL)


def launch(img, m, n, rows, cols, batch=rr.SHIPPED_B):
    """The image after rkrm_tab_compact (a copy; img stays)."""
    assert kh.load().rkrm_batch() == rr.SHIPPED_B
    out = np.ascontiguousarray(np.array(img, dtype=np.float64, copy=True))
    r, c = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    kh._call("rkrm_tab_compact", [m, n, out.shape[1], batch], [out, r, c])
    return out


def diff_bits(got, want, limit=5):
    g, w = kh.bits(got).reshape(-1), kh.bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    if not bad.size:
        return ""
    ld = want.shape[1]
    shown = ", ".join(f"[column {int(x) // ld}, row {int(x) % ld}] {got.reshape(-1)[x]!r} != {want.reshape(-1)[x]!r}" for x in bad[:limit])
    return f"{bad.size} words differ: {shown}"
