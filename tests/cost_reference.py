"""The reduced costs of a basis under a given cost vector -- what relp_change_cost and relp_set_cost must leave in the engine
(include/relp_engine.h) -- as a test reference over numpy f64: d = c - c_B' B^-1 [A | I] and -pi = -(c_B' B^-1) from
`dual_reference.standard_form` and `np.linalg.solve`, plus a textbook primal simplex that only serves to choose test inputs on the
CPU (how many pivots a re-solve needs, roughly; it is not the engine's pivot rule).

TEST INFRASTRUCTURE ONLY; the row kinds of dual_reference (no variable bounds, no range rows).  With <= rows only, engine row k has
the identity column n + k, so -pi_k = d[n + k]."""
from __future__ import annotations

from typing import Sequence

import numpy as np

import dual_reference as dr


def with_cost(md, cost):
    """(full, rhs, cost over all columns) of `md` with the structural costs replaced by `cost`."""
    full, rhs, c = dr.standard_form(md)
    c[: md.nr_normal] = np.asarray(cost, dtype=np.float64)
    return full, rhs, c


def reduced_costs(md, basis: Sequence[int], cost):
    """(d over the columns of standard_form, -pi, objective) of `basis` under the structural costs `cost`."""
    full, rhs, c = with_cost(md, cost)
    basis = [int(j) for j in basis]
    B = full[:, basis]
    pi = np.linalg.solve(B.T, c[basis])
    d = c - pi @ full
    return d, -pi, float(c[basis] @ np.linalg.solve(B, rhs))


def tableau_row(md, basis: Sequence[int], row: int):
    """Row `row` of T = B^-1 [A | I]."""
    full, _, _ = dr.standard_form(md)
    basis = [int(j) for j in basis]
    e = np.zeros(len(basis))
    e[int(row)] = 1.0
    return np.linalg.solve(full[:, basis].T, e) @ full


def primal_pivots(md, basis: Sequence[int], cost, tol_cost: float = 1e-7, tol_pivot: float = 1e-5, max_iters: int = 10000):
    """Pivots a most-negative-d, minimum-ratio primal simplex needs from the primal feasible `basis` to the optimum under `cost`,
    by Gauss-Jordan on the dense tableau; None when it does not end `optimal` within max_iters."""
    full, rhs, c = with_cost(md, cost)
    basis = [int(j) for j in basis]
    B = full[:, basis]
    T = np.linalg.solve(B, full)
    b = np.linalg.solve(B, rhs)
    d = c - c[basis] @ T
    for it in range(max_iters):
        free = np.ones(T.shape[1], dtype=bool)
        free[basis] = False
        cand = np.flatnonzero(free & (d < -tol_cost))
        if cand.size == 0:
            return it
        q = int(cand[np.argmin(d[cand])])
        rows = np.flatnonzero(T[:, q] > tol_pivot)
        if rows.size == 0:
            return None
        r = int(rows[np.argmin(np.maximum(b[rows], 0.0) / T[rows, q])])
        piv = T[r, q]
        T[r] /= piv
        b[r] /= piv
        for i in range(T.shape[0]):
            if i != r and T[i, q] != 0.0:
                f = T[i, q]
                T[i] -= f * T[r]
                b[i] -= f * b[r]
        d -= d[q] * T[r]
        basis[r] = q
    return None
