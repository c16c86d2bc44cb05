"""What relp_add_columns must leave in the engine (include/relp_engine.h), as a test reference over numpy f64: the
wide LP with the new columns behind the structural ones, and T = B^-1 [A | I], b, d, -pi and B^-1 of a basis of it from
`cut_reference.Tableau`, re-ordered into the engine's column order.

TEST INFRASTRUCTURE ONLY; the row kinds of dual_reference (no variable bounds, no range rows).

Column orders for a dense <= LP with m rows, n structural columns and k added ones:
    engine  [ n structural | m slacks | k added ]          (relp_add_columns puts a column behind every existing one)
    wide    [ n structural | k added | m slacks ]          (the LP a fresh engine is created on)
`to_wide` / `to_engine` map single indices, `wide_order` is the permutation that re-orders a wide vector into the engine's.

The LPs of the tests: lp = synthetic.dense_lp(m, n + k, seed); the engine gets A[:, :n], b, c[:n], the new columns are A[:, n:]
with the costs c[n:]."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from rust_lp_amd import MatrixData

import cut_reference as cutref


def narrow(lp, n: int) -> MatrixData:
    """The LP the engine starts from: the first n columns."""
    return MatrixData.from_dense_le(np.asfortranarray(np.asarray(lp["A"])[:, :n]), np.array(lp["b"]), np.array(lp["c"])[:n])


def new_columns(lp, n: int, sparse: bool = False):
    """(A_new, cost): the columns held back.  sparse: column k keeps only its rows i % 4 == k % 4."""
    A = np.array(np.asarray(lp["A"])[:, n:], dtype=np.float64)
    if sparse:
        i, k = np.indices(A.shape)
        A[(i % 4) != (k % 4)] = 0.0
    return A, np.array(lp["c"], dtype=np.float64)[n:]


def wide(lp, n: int, A_new=None, cost=None, b=None) -> MatrixData:
    """The LP with the new columns as further structural columns."""
    A = np.asarray(lp["A"], dtype=np.float64)
    if A_new is not None:
        A = np.hstack([A[:, :n], np.asarray(A_new, dtype=np.float64).reshape(A.shape[0], -1)])
    c = np.array(lp["c"], dtype=np.float64)[:A.shape[1]].copy()
    if cost is not None:
        c[:len(cost)] = cost
    return MatrixData.from_dense_le(np.asfortranarray(A), np.array(lp["b"] if b is None else b, dtype=np.float64), c)


def to_wide(j, m: int, n: int, k: int):
    j = np.asarray(j)
    return np.where(j < n, j, np.where(j < n + m, j + k, j - m)).astype(np.int32)


def to_engine(j, m: int, n: int, k: int):
    j = np.asarray(j)
    return np.where(j < n, j, np.where(j < n + k, j + m, j - k)).astype(np.int32)


def wide_order(m: int, n: int, k: int) -> np.ndarray:
    """order[engine index] = wide index."""
    return to_wide(np.arange(n + m + k), m, n, k)


class Tableau:
    """T, b, d, -pi, B^-1 and the objective of the engine-indexed `basis` of the wide LP, columns in the engine's order."""

    def __init__(self, md_wide: MatrixData, basis: Sequence[int], m: int, n: int, k: int):
        ref = cutref.Tableau(md_wide, to_wide(np.asarray(basis), m, n, k))
        order = wide_order(m, n, k)
        self.T, self.d = ref.T[:, order], ref.d[order]
        self.b, self.binv, self.minus_pi, self.objective = ref.b, ref.binv, ref.minus_pi, ref.objective
