"""Dense-tableau dual simplex with the rules of `relp_run_dual` (include/relp_engine.h), as a test reference: once
over `fractions.Fraction`, once over numpy f64.  It starts from a given basis of [A | slacks] of a `MatrixData` and keeps the whole
tableau T = B^-1 [A | slacks], b = B^-1 rhs and d = c - c_B' T, pivoting by Gauss-Jordan elimination.

TEST INFRASTRUCTURE ONLY.  Supported row kinds: ==, <= and >= without variable bounds or range rows (columns: structural | <= slacks
(+1) | >= slacks (-1), the order of matrix_data.rs:403-409).

Rules (absolute tolerances of relp_config_t):
  leaving row      row i is infeasible iff b_i < -tol_feas; the minimum b_i over the infeasible rows; among the infeasible rows with
                   b_i <= min + tol_tie * max(1, |min|) the smallest leaving column basis[i] wins; no infeasible row = optimal
  entering column  candidates are the non-basic columns j with T[r, j] < -tol_pivot; ratio dz_j / (-T[r, j]) with dz_j = 0 when
                   d_j <= tol_zero, else d_j; the minimum ratio; among ratios <= min + tol_tie * max(1, |min|) the lowest j wins;
                   no candidate = primal infeasible
"""
from __future__ import annotations

from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

import numpy as np

from rust_lp_amd import MatrixData, synthetic

TOLERANCES = dict(tol_cost=1e-7, tol_pivot=1e-5, tol_zero=1e-11, tol_tie=1e-9, tol_feas=1e-7)   # relp_default_config


def covering_lp(m: int, n: int, seed: int):
    """min c'x, A x >= b, x >= 0 with c > 0 from `synthetic.dense_numerators`: A = A_num / 1000, b = b_num / 4000, c = -c_num / 1000.
    Returns (MatrixData, exact) with exact = (A, b, c) as object arrays of Fractions."""
    nums = synthetic.dense_numerators(m, n, seed)
    md = MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=0, nr_ge=m, b=nums["b_num"].astype(np.float64) / 4000.0,
                    cost=-nums["c_num"].astype(np.float64) / 1000.0, upper_bound=np.full(n, np.inf),
                    dense=np.asfortranarray(nums["A_num"].astype(np.float64) / 1000.0))
    A = np.empty((m, n), dtype=object)
    for i in range(m):
        for j in range(n):
            A[i, j] = Fraction(int(nums["A_num"][i, j]), 1000)
    b = np.array([Fraction(int(v), 4000) for v in nums["b_num"]], dtype=object)
    c = np.array([Fraction(-int(v), 1000) for v in nums["c_num"]], dtype=object)
    return md, (A, b, c)


def infeasible_pair() -> MatrixData:
    """x1 + x2 <= 2, x1 + x2 >= 4, c = (1, 1): primal infeasible; the slack basis [2, 3] is dual feasible."""
    return MatrixData(nr_normal=2, nr_eq=0, nr_range=0, nr_le=1, nr_ge=1, b=np.array([2.0, 4.0]), cost=np.array([1.0, 1.0]),
                      upper_bound=np.full(2, np.inf), dense=np.asfortranarray(np.ones((2, 2))))


def exact_of(md: MatrixData):
    """(A, b, c) of `md` as object arrays of Fractions (every f64 is a rational)."""
    A = np.asarray(md.ensure_dense().dense)
    out = np.empty(A.shape, dtype=object)
    for i in range(A.shape[0]):
        for j in range(A.shape[1]):
            out[i, j] = Fraction(float(A[i, j]))
    return (out, np.array([Fraction(float(v)) for v in md.b], dtype=object),
            np.array([Fraction(float(v)) for v in md.cost], dtype=object))


def surplus_basis(m: int, n: int) -> np.ndarray:
    """The all-slack basis n .. n + m - 1."""
    return np.arange(n, n + m, dtype=np.int32)


def standard_form(md: MatrixData, exact=None):
    """[A | slacks] (m x (n + nr_le + nr_ge)), rhs, cost over all columns: float64 arrays, or object arrays of Fractions when
    `exact` = (A, b, c) is given."""
    if md.nr_range or np.isfinite(np.asarray(md.upper_bound)).any():
        raise ValueError("dual_reference: no range rows, no variable bounds")
    m, n = md.nr_constraints, md.nr_normal
    ns = md.nr_le + md.nr_ge
    if exact is None:
        full = np.zeros((m, n + ns))
        full[:, :n] = np.asarray(md.ensure_dense().dense, dtype=np.float64)
        rhs = np.asarray(md.b, dtype=np.float64).copy()
        cost = np.concatenate([np.asarray(md.cost, dtype=np.float64), np.zeros(ns)])
        one = 1.0
    else:
        full = np.empty((m, n + ns), dtype=object)
        full[:, :] = Fraction(0)
        full[:, :n] = exact[0]
        rhs = exact[1].copy()
        cost = np.concatenate([exact[2], np.array([Fraction(0)] * ns, dtype=object)])
        one = Fraction(1)
    for k in range(ns):
        row = md.nr_eq + k
        full[row, n + k] = one if k < md.nr_le else -one
    return full, rhs, cost


def select_dual_pivot_row(b: Sequence, basis: Sequence[int], tol_feas, tol_tie) -> Optional[int]:
    """The leaving row, None when no row is infeasible."""
    infeasible = [i for i in range(len(b)) if b[i] < -tol_feas]
    if not infeasible:
        return None
    mn = min(b[i] for i in infeasible)
    bound = mn + tol_tie * max(1, abs(mn))
    return min((int(basis[i]), i) for i in infeasible if b[i] <= bound)[1]


def select_dual_pivot_column(d: Sequence, row: Sequence, in_basis: Sequence, tol_pivot, tol_zero, tol_tie) -> Optional[int]:
    """The entering column for tableau row `row` over the columns 0 .. len(row) - 1, None when there is no candidate."""
    cand = []
    for j in range(len(row)):
        if in_basis[j] or not row[j] < -tol_pivot:
            continue
        dz = d[j] if d[j] > tol_zero else d[j] * 0
        cand.append((dz / (-row[j]), j))
    if not cand:
        return None
    mn = min(cand)[0]
    bound = mn + tol_tie * max(1, abs(mn))
    return min(j for ratio, j in cand if ratio <= bound)


class DualResult:
    def __init__(self, outcome, trace, objective, basis, b, max_band):
        self.outcome = outcome              # "optimal", "infeasible", "running"
        self.trace = trace                  # [(q, r, leaving)]
        self.objective = objective
        self.basis = basis
        self.b = b
        self.max_band = max_band            # the most rows / columns any tie band held


def dual_simplex(md: MatrixData, basis: Sequence[int], exact=None, max_iters: int = 1 << 30, **tolerances) -> DualResult:
    tol = dict(TOLERANCES)
    tol.update(tolerances)
    if exact is not None:
        tol = {k: Fraction(v) for k, v in tol.items()}
    full, rhs, cost = standard_form(md, exact)
    m, ncol = full.shape
    basis = [int(j) for j in basis]
    B = full[:, basis]
    if exact is None:
        T = np.linalg.solve(B, full)
        b = np.linalg.solve(B, rhs)
    else:
        T, b = _solve_exact(B, full, rhs)
    cb = cost[basis]
    d = cost - cb @ T
    in_basis = [False] * ncol
    for j in basis:
        in_basis[j] = True
    trace: List[Tuple[int, int, int]] = []
    outcome = "running"
    max_band = 0
    for _ in range(max_iters):
        r = select_dual_pivot_row(b, basis, tol["tol_feas"], tol["tol_tie"])
        if r is None:
            outcome = "optimal"
            break
        mn = min(b)
        max_band = max(max_band, sum(1 for v in b if v < -tol["tol_feas"] and v <= mn + tol["tol_tie"] * max(1, abs(mn))))
        q = select_dual_pivot_column(d, T[r], in_basis, tol["tol_pivot"], tol["tol_zero"], tol["tol_tie"])
        if q is None:
            outcome = "infeasible"
            break
        ratios = [(d[j] if d[j] > tol["tol_zero"] else d[j] * 0) / (-T[r, j]) for j in range(ncol)
                  if not in_basis[j] and T[r, j] < -tol["tol_pivot"]]
        lo = min(ratios)
        max_band = max(max_band, sum(1 for v in ratios if v <= lo + tol["tol_tie"] * max(1, abs(lo))))
        leaving = basis[r]
        trace.append((q, r, leaving))
        alpha = T[:, q].copy()
        T[r] = T[r] / alpha[r]
        b[r] = b[r] / alpha[r]
        for i in range(m):
            if i != r and alpha[i] != 0:
                T[i] = T[i] - alpha[i] * T[r]
                b[i] = b[i] - alpha[i] * b[r]
        d = d - d[q] * T[r]
        d[q] = d[q] * 0
        basis[r] = q
        in_basis[leaving] = False
        in_basis[q] = True
    objective = sum(cost[basis[i]] * b[i] for i in range(m))
    return DualResult(outcome, trace, objective, basis, b, max_band)


def _solve_exact(B, full, rhs):
    """B^-1 [full | rhs] by Gauss-Jordan elimination over Fractions (any non-singular B)."""
    m = B.shape[0]
    aug = np.concatenate([B.copy(), full.copy(), rhs.reshape(m, 1).copy()], axis=1)
    for k in range(m):
        p = next(i for i in range(k, m) if aug[i, k] != 0)
        if p != k:
            aug[[k, p]] = aug[[p, k]]
        aug[k] = aug[k] / aug[k, k]
        for i in range(m):
            if i != k and aug[i, k] != 0:
                aug[i] = aug[i] - aug[i, k] * aug[k]
    return aug[:, m:-1].copy(), aug[:, -1].copy()
