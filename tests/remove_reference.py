"""Helper module of the tests of the rows and columns removed in place (not collected by pytest): the plain reference of
launch_tab_compact (np.delete on the live part of an image), a numpy model that walks the image IN PLACE in the order the two
kernels state in relp_kernels.h, and the index maps a removal leaves behind.

Layout: an image is a C-ordered array img[c][i] (columns x ld): column c of the device image at c * ld, as in kernel_harness.
m rows and n columns of it are live; the rest (pitch padding, room rows, room columns) must come back untouched.

The model's order (one step = every load of the step, then every store of the step, all on the same array):
  k_tab_drop_rows<B>     per column: chunks of 256 B destination rows from rows[0] down; source of dst = dst + #{k: rows[k] - k <= dst};
                         destination rows [m - nr, m) get 0.0
  k_tab_drop_columns<B>  per row (of the m - nr rows): destination columns from cols[0] on, B at a time; source = dst + removed
                         columns at or left of the source; destination columns [n - nc, n) get 0.0
A model that read after an overwrite would differ from np.delete: tests/test_kernel_models_remove.py holds the two together."""
from __future__ import annotations

import numpy as np

THREADS = 256
SHIPPED_B = 4


def expected(img, m, n, rows, cols):
    """The image after launch_tab_compact by its contract: the survivors closed up in order, 0.0 in the vacated rows and columns of
    the live part, everything else as it was."""
    out = np.array(img, copy=True)
    live = np.delete(np.delete(out[:n, :m], np.asarray(cols, dtype=np.int64), axis=0), np.asarray(rows, dtype=np.int64), axis=1)
    if len(rows) or len(cols):
        out[:n, :m] = 0.0
        out[:live.shape[0], :live.shape[1]] = live
    return out


def row_sources(m, rows, dst):
    """source row of every destination row in dst (all < m - len(rows)), as k_tab_drop_rows finds it"""
    rows = np.asarray(rows, dtype=np.int64)
    adj = rows - np.arange(rows.size)
    return dst + np.searchsorted(adj, dst, side="right")


def model_drop_rows(img, m, n, rows, B=SHIPPED_B):
    """k_tab_drop_rows<B> in place on img (modified and returned)."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0:
        return img
    m_new = m - rows.size
    for base in range(int(rows[0]), m, THREADS * B):
        dst = np.arange(base, min(base + THREADS * B, m))
        moved = dst[dst < m_new]
        src = row_sources(m, rows, moved)
        assert np.all(src >= moved) and np.all(src < m)
        for c in range(n):
            loaded = np.zeros(dst.size)
            loaded[:moved.size] = img[c, src]          # every load of the chunk ...
            img[c, dst] = loaded                       # ... then every store
    return img


def model_drop_columns(img, m, n, cols, B=SHIPPED_B):
    """k_tab_drop_columns<B> in place on rows [0, m) of img (modified and returned); every row walks the same way."""
    cols = [int(c) for c in cols]
    if not cols:
        return img
    n_new, k = n - len(cols), 0
    for dst0 in range(cols[0], n, B):
        loaded = []
        for dst in range(dst0, min(dst0 + B, n)):
            if dst < n_new:
                src = dst + k
                while k < len(cols) and cols[k] <= src:
                    k += 1
                    src += 1
                assert dst <= src < n
                loaded.append(img[src, :m].copy())
            else:
                loaded.append(np.zeros(m))
        for x, dst in enumerate(range(dst0, min(dst0 + B, n))):
            img[dst, :m] = loaded[x]
    return img


def model_compact(img, m, n, rows, cols, B=SHIPPED_B):
    """launch_tab_compact: the row kernel over all n columns, then the column kernel over the m - nr rows."""
    out = np.array(img, copy=True)
    model_drop_rows(out, m, n, rows, B)
    model_drop_columns(out, m - len(rows), n, cols, B)
    return out


def index_map(size, gone):
    """old index -> new index after the entries `gone` left (-1 for those)"""
    keep = np.ones(size, dtype=bool)
    keep[np.asarray(gone, dtype=np.int64)] = False
    out = np.full(size, -1, dtype=np.int64)
    out[keep] = np.arange(int(keep.sum()))
    return out


def sentinel_image(rng, m, n, ld, n_alloc, sentinel):
    """An image of n_alloc columns with pitch ld: distinct finite values (signed zeros among them) in the live m x n part, the
    sentinel everywhere else."""
    img = np.full((n_alloc, ld), sentinel)
    live = rng.standard_normal((n, m)) * np.exp(rng.uniform(-20, 20, (n, m)))
    live[rng.random((n, m)) < 0.05] = 0.0
    live[rng.random((n, m)) < 0.03] = -0.0
    img[:n, :m] = live
    return img
