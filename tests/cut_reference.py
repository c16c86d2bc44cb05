"""What relp_add_cuts must leave in the engine (include/relp_engine.h), as a test reference over numpy f64: the LP with
the cuts stacked under A as <= rows, and T = B^-1 [A | I], b, d, -pi and B^-1 of a basis of it from `dual_reference.standard_form`
and `np.linalg.solve`.

TEST INFRASTRUCTURE ONLY; the row kinds of dual_reference (no variable bounds, no range rows).  For a dense <= LP the stacked LP has
the engine's row and column indices exactly: cut k is row m + k, its slack column n + m + k.

The cuts of the tests: G = default_rng(1000 * seed + k).integers(0, 8, (k, n)), beta = 0.9 * G x* with x* the optimum of the LP."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from rust_lp_amd import MatrixData

import dual_reference as dr


def optimum_x(lp, basis: Sequence[int]) -> np.ndarray:
    """The structural part of the basic solution of `basis` of the dense <= LP `lp`."""
    md = MatrixData.from_dense_le(lp["A"], np.array(lp["b"]), np.array(lp["c"]))
    full, rhs, _ = dr.standard_form(md)
    basis = [int(j) for j in basis]
    x = np.zeros(full.shape[1])
    x[basis] = np.linalg.solve(full[:, basis], rhs)
    return x[: md.nr_normal]


def cuts(lp, basis: Sequence[int], k: int, seed: int):
    """(G, beta): k cuts G x <= beta, each violated at the optimum x* of `basis`."""
    n = lp["A"].shape[1]
    G = np.random.default_rng(1000 * seed + k).integers(0, 8, (k, n)).astype(float)
    beta = 0.9 * (G @ optimum_x(lp, basis))
    return G, beta


def stacked(lp, G, beta, cost=None, b=None) -> MatrixData:
    """The LP with the cuts as further <= rows."""
    A = np.vstack([np.asarray(lp["A"]), np.asarray(G, dtype=np.float64).reshape(-1, lp["A"].shape[1])])
    rhs = np.concatenate([np.asarray(lp["b"] if b is None else b, dtype=np.float64), np.atleast_1d(beta)])
    return MatrixData.from_dense_le(A, rhs, np.array(lp["c"] if cost is None else cost, dtype=np.float64))


def extended_basis(basis: Sequence[int], m: int, n: int, k: int) -> np.ndarray:
    """The old basis with the k cut slacks basic in the cut rows."""
    return np.concatenate([np.asarray(basis, dtype=np.int32), np.arange(n + m, n + m + k, dtype=np.int32)])


class Tableau:
    """T = B^-1 [A | I], b, d, -pi, B^-1 and the objective of `basis` of `md` (numpy solve)."""

    def __init__(self, md: MatrixData, basis: Sequence[int]):
        full, rhs, c = dr.standard_form(md)
        basis = [int(j) for j in basis]
        B = full[:, basis]
        self.T = np.linalg.solve(B, full)
        self.b = np.linalg.solve(B, rhs)
        self.binv = np.linalg.inv(B)
        pi = np.linalg.solve(B.T, c[basis])
        self.d = c - pi @ full
        self.minus_pi = -pi
        self.objective = float(c[basis] @ self.b)
