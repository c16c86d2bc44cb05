"""What relp_gomory_cuts must return (include/relp_engine.h) and the rounds of engine.gomory_rounds, as a test reference:
once over `fractions.Fraction`, once over numpy f64.

TEST INFRASTRUCTURE ONLY.  The LP is kept in the engine's standard form with the engine's indices:
  rows     == | <= | >= | one bound row per bounded column (x_c + s = u_c) | the cut rows, in the order they were added
  columns  structural | <= slacks (+1) | >= slacks (-1) | bound slacks (+1) | cut slacks (+1)
(no range rows).  The engine minimises: `max c'x` is the cost -c.

The rule.  f0 = b_r - floor(b_r); over the non-basic columns j with a = T[r, j]:
  |a| <= tol_zero                          pi_j = 0
  integer column, f = a - floor(a)         f <= tol_zero or f >= 1 - tol_zero: pi_j = 0
      fractional                           pi_j = f
      mixed                                pi_j = f if f <= f0 else (f0 * (1 - f)) / (1 - f0)
  continuous column, mixed                 pi_j = a if a > 0 else (f0 * (-a)) / (1 - f0)
  continuous column, fractional            the entry is skipped (status 4)
Every product, difference and quotient is rounded once, in the order written, with no contraction (numpy f64 scalars do exactly
that; over Fractions nothing is rounded).

The substitution.  Row i reads (A x)_i [+ x_c in the bound row of c] + sigma_i s_i = rhs_i; y_i = sigma_i * pi_{s_i}:
  g_c  = -pi_c + sum_i y_i A[i, c] + y_{bound_row(c)}        beta = -f0 + sum_i y_i rhs_i
The order of the sum in g_c on the device: thread t of 256 chains the rows t, t + 256, .. of A (the constraint rows, then the cut
rows; every row: y_i is 0 where a row has no slack or pi is 0) by fma in ascending order from 0.0, then the fixed halving tree over
the 256 chains (kernel_harness.model_pending(order="tree")), then (sum - pi_c) + y_{bound_row(c)}, the last term only where c has a
bound row.  beta is one fma per row with y_i != 0 in ascending i from -f0.  `structural_f64` below restates exactly that; `cut` uses
plain sums (the ABI tests compare within a rounding bound, the kernel tests bit for bit against structural_f64)."""
from __future__ import annotations

import itertools
import math
from fractions import Fraction
from typing import List, Optional, Sequence

import numpy as np

import dual_reference as dr
import kernel_harness as kh

FRACTIONAL, MIXED = 0, 1
CUT, NOT_INTEGER, FRACTION, ARTIFICIAL, CONTINUOUS = range(5)
TOL_ZERO = dr.TOLERANCES["tol_zero"]


def pi_of(a, f0, integer: bool, kind: int, tol_zero):
    """(pi_j, bad) of one entry; bad: a continuous column in a fractional cut."""
    zero = abs(a * 0)                                  # (+0.0 whatever the sign of a)
    if abs(a) <= tol_zero:
        return zero, False
    if integer:
        f = a - math.floor(a)
        if f <= tol_zero or f >= 1 - tol_zero:
            return zero, False
        if kind == FRACTIONAL or f <= f0:
            return f, False
        num = f0 * (1 - f)
        return num / (1 - f0), False
    if kind == FRACTIONAL:
        return zero, True
    if a > 0:
        return a, False
    num = f0 * (-a)
    return num / (1 - f0), False


class LP:
    """The standard form above, over float64 (exact=False) or Fractions.  A: rows == | <= | >=; upper: per column, inf = none."""

    def __init__(self, A, b, cost, nr_eq, nr_le, nr_ge, upper=None, exact=False):
        conv = (lambda v: Fraction(v)) if exact else float
        A = [[conv(v) for v in row] for row in A]
        self.exact, self.n = exact, len(cost)
        self.mc = nr_eq + nr_le + nr_ge
        assert len(A) == self.mc
        upper = [math.inf] * self.n if upper is None else list(upper)
        bounded = [c for c in range(self.n) if math.isfinite(upper[c])]
        self.bound_row = [-1] * self.n
        m, ncol = self.mc + len(bounded), self.n + nr_le + nr_ge + len(bounded)
        zero = conv(0)
        self.full = [[zero] * ncol for _ in range(m)]
        self.rhs = [conv(v) for v in b] + [conv(upper[c]) for c in bounded]
        self.cost = [conv(v) for v in cost] + [zero] * (ncol - self.n)
        self.slack = [None] * m                       # per row: (column, sign)
        for i in range(self.mc):
            self.full[i][: self.n] = A[i]
        for k in range(nr_le + nr_ge):
            sign = 1 if k < nr_le else -1
            self.full[nr_eq + k][self.n + k] = conv(sign)
            self.slack[nr_eq + k] = (self.n + k, sign)
        for k, c in enumerate(bounded):
            row, col = self.mc + k, self.n + nr_le + nr_ge + k
            self.bound_row[c] = row
            self.full[row][c] = conv(1)
            self.full[row][col] = conv(1)
            self.slack[row] = (col, 1)
        self.nr_cuts = 0

    @property
    def m(self): return len(self.full)

    @property
    def ncol(self): return len(self.cost)

    def add_cuts(self, G, beta):
        zero, one = self.cost[0] * 0, self.cost[0] * 0 + 1
        for g, bk in zip(G, beta):
            for row in self.full:
                row.append(zero)
            self.full.append(list(g) + [zero] * (self.ncol - self.n) + [one])
            self.slack.append((self.ncol, 1))
            self.cost.append(zero)
            self.rhs.append(bk)
            self.nr_cuts += 1

    def arrays(self):
        dt = object if self.exact else np.float64
        return np.array(self.full, dtype=dt), np.array(self.rhs, dtype=dt), np.array(self.cost, dtype=dt)

    def tableau(self, basis: Sequence[int]):
        """(T, b, d) of `basis`: Gauss-Jordan over Fractions, numpy solve over f64."""
        full, rhs, cost = self.arrays()
        basis = [int(j) for j in basis]
        B = full[:, basis]
        if self.exact:
            T, b = dr._solve_exact(B, full, rhs)
        else:
            T, b = np.linalg.solve(B, full), np.linalg.solve(B, rhs)
        return T, b, cost - cost[basis] @ T

    def objective(self, basis, b):
        return sum(self.cost[int(basis[i])] * b[i] for i in range(self.m))


def cut(lp: LP, row, b_r, basic: int, in_basis, is_integer=None, kind=FRACTIONAL, away=1e-6, tol_zero=TOL_ZERO, detail=None):
    """(g over the structural columns, beta, f0, status) of the tableau row `row` (all columns of lp) with basic column `basic`.
    detail: a dict that receives pi (per column) and y (per row) of a cut that was made."""
    zero = lp.cost[0] * 0
    if lp.exact:
        away, tol_zero = Fraction(away), Fraction(tol_zero)
    f0 = b_r - math.floor(b_r)
    skipped = [zero] * lp.n, zero, f0
    if is_integer is not None and not is_integer[basic]:
        return (*skipped, NOT_INTEGER)
    if f0 < away or f0 > 1 - away:
        return (*skipped, FRACTION)
    pi = [zero] * lp.ncol
    for j in range(lp.ncol):
        if in_basis[j]:
            continue
        pi[j], bad = pi_of(row[j], f0, True if is_integer is None else bool(is_integer[j]), kind, tol_zero)
        if bad:
            return (*skipped, CONTINUOUS)
    y = [zero if s is None else s[1] * pi[s[0]] for s in lp.slack]
    if detail is not None:
        detail.update(pi=pi, y=y)
    g = []
    for c in range(lp.n):
        acc = zero
        for i in range(lp.m):
            if lp.bound_row[c] != i:
                acc = acc + y[i] * lp.full[i][c]
        acc = acc - pi[c]
        if lp.bound_row[c] >= 0:
            acc = acc + y[lp.bound_row[c]]
        g.append(acc)
    beta = -f0
    for i in range(lp.m):
        if y[i] != 0:
            beta = beta + y[i] * lp.rhs[i]
    return g, beta, f0, CUT


def pick_rows(b, basis, flags, away, cuts_per_round):
    """The driver's rule: the first rows whose basic column is flagged integer and whose fraction lies inside [away, 1 - away]."""
    rows = []
    for i in range(len(b)):
        f = b[i] - math.floor(b[i])
        if flags[int(basis[i])] and away <= f <= 1 - away:
            rows.append(i)
    return rows[:cuts_per_round]


def dual_simplex(lp: LP, basis, max_iters=10_000):
    """dual_reference.dual_simplex on the standard form of `lp`: ("optimal" | "infeasible" | "running", basis, b, T, d)."""
    tol = {k: (Fraction(v) if lp.exact else v) for k, v in dr.TOLERANCES.items()}
    T, b, d = lp.tableau(basis)
    basis = [int(j) for j in basis]
    in_basis = [False] * lp.ncol
    for j in basis:
        in_basis[j] = True
    outcome = "running"
    for _ in range(max_iters):
        r = dr.select_dual_pivot_row(b, basis, tol["tol_feas"], tol["tol_tie"])
        if r is None:
            outcome = "optimal"
            break
        q = dr.select_dual_pivot_column(d, T[r], in_basis, tol["tol_pivot"], tol["tol_zero"], tol["tol_tie"])
        if q is None:
            outcome = "infeasible"
            break
        alpha = T[:, q].copy()
        T[r] = T[r] / alpha[r]
        b[r] = b[r] / alpha[r]
        for i in range(lp.m):
            if i != r and alpha[i] != 0:
                T[i] = T[i] - alpha[i] * T[r]
                b[i] = b[i] - alpha[i] * b[r]
        d = d - d[q] * T[r]
        d[q] = d[q] * 0
        in_basis[basis[r]] = False
        in_basis[q] = True
        basis[r] = q
    return outcome, basis, b, T, d


class Round:
    def __init__(self, rows, cuts, vertex, objective, basis):
        self.rows, self.cuts, self.vertex, self.objective, self.basis = rows, cuts, vertex, objective, basis


def vertex_of(lp: LP, basis, b):
    x = [lp.cost[0] * 0] * lp.n
    for i, j in enumerate(basis):
        if int(j) < lp.n:
            x[int(j)] = b[i]
    return x


def rounds(lp: LP, basis, is_integer=None, max_rounds=20, cuts_per_round=3, kind=FRACTIONAL, away=1e-6) -> List[Round]:
    """engine.gomory_rounds on `lp` from the optimal basis `basis`; lp grows by the cuts.  Round.cuts: [(g, beta, f0)], Round.vertex:
    the structural part of the vertex the cuts were made at; objective and basis after the round's dual simplex (None, None when
    the LP became infeasible)."""
    out = []
    basis = [int(j) for j in basis]
    away_c = Fraction(away) if lp.exact else away
    for _ in range(max_rounds):
        T, b, _ = lp.tableau(basis)
        flags = [True] * lp.ncol
        if is_integer is not None:
            flags[: len(is_integer)] = [bool(v) for v in is_integer][: lp.ncol]
        picked = pick_rows(b, basis, flags, away_c, cuts_per_round)
        if not picked:
            break
        in_basis = [False] * lp.ncol
        for j in basis:
            in_basis[j] = True
        made = []
        for r in picked:
            g, beta, f0, status = cut(lp, T[r], b[r], basis[r], in_basis, flags, kind, away)
            if status == CUT:
                made.append((g, beta, f0))
        if not made:
            break
        vertex = vertex_of(lp, basis, b)
        first_slack = lp.ncol
        lp.add_cuts([g for g, _, _ in made], [beta for _, beta, _ in made])
        basis = basis + list(range(first_slack, first_slack + len(made)))
        outcome, basis, b, _, _ = dual_simplex(lp, basis)
        if outcome != "optimal":
            out.append(Round(picked, made, vertex, None, None))
            break
        out.append(Round(picked, made, vertex, lp.objective(basis, b), list(basis)))
    return out


def optimal_basis(lp: LP):
    """An optimal basis of the (small) LP by enumeration over Fractions: the first basis in lexicographic order that is primal and
    dual feasible.  None when there is none."""
    assert lp.exact
    full, rhs, cost = lp.arrays()
    for basis in itertools.combinations(range(lp.ncol), lp.m):
        B = full[:, list(basis)]
        try:
            T, b = dr._solve_exact(B, full, rhs)
        except StopIteration:                          # singular
            continue
        if min(b) < 0:
            continue
        d = cost - cost[list(basis)] @ T
        if min(d) >= 0:
            return list(basis)
    return None


def integer_points(A, b, nr_eq, nr_le, nr_ge, upper, box: int):
    """Every integer x in [0, box]^n (and under its upper bounds) with A x (== | <= | >=) b, as an int64 array, one point per row."""
    A = np.asarray(A, dtype=np.int64)
    n = A.shape[1]
    hi = [box if upper is None or not math.isfinite(upper[c]) else min(box, int(math.floor(upper[c]))) for c in range(n)]
    grid = np.stack(np.meshgrid(*[np.arange(h + 1) for h in hi], indexing="ij"), axis=-1).reshape(-1, n)
    v = grid @ A.T
    bb = np.asarray(b, dtype=np.int64)
    ok = np.ones(grid.shape[0], dtype=bool)
    for i in range(A.shape[0]):
        if i < nr_eq:
            ok &= v[:, i] == bb[i]
        elif i < nr_eq + nr_le:
            ok &= v[:, i] <= bb[i]
        else:
            ok &= v[:, i] >= bb[i]
    return grid[ok]


# ---- the device's orders, bit for bit (tests of launch_tab_gomory) ------------------------------------------------------------
def pi_f64(E, f0, cand, integer, kind, tol_zero):
    """pi[k][c] of the entries E (count x stored columns): gomory_pi in f64; cand / integer per stored column; f0[k] < 0: skipped.
    Returns (pi, bad[k][c])."""
    count, n = E.shape
    pi = np.zeros((count, n))
    bad = np.zeros((count, n), dtype=bool)
    for k in range(count):
        if f0[k] < 0:
            continue
        for c in range(n):
            if cand[c]:
                v, bad[k, c] = pi_of(np.float64(E[k, c]), np.float64(f0[k]), bool(integer[c]), kind, np.float64(tol_zero))
                pi[k, c] = v
    return pi, bad


def structural_f64(pi_struct, y, A, a_rows, bound_row):
    """g[k][c] = (tree sum over the rows of A of y[k][a_rows[i]] * A[i, c]  -  pi_struct[k][c])  +  y[k][bound_row[c]] (where c has
    a bound row).  A: rows of A x structural columns; a_rows: the tableau row of every row of A."""
    count, nn = pi_struct.shape
    g = np.zeros((count, nn))
    a_rows = np.asarray(a_rows, dtype=np.int64)
    for k in range(count):
        s = kh.model_pending(np.asarray(y[k][a_rows], dtype=np.float64), np.ascontiguousarray(A.T)) if A.shape[0] else np.zeros(nn)
        v = s - pi_struct[k]
        for c in range(nn):
            if bound_row[c] >= 0:
                v[c] = v[c] + y[k][bound_row[c]]
        g[k] = v
    return g


def beta_f64(f0, y, rhs):
    beta = -float(f0)
    for i in range(len(rhs)):
        if y[i] != 0.0:
            beta = kh.fma_exact(float(y[i]), float(rhs[i]), beta)
    return beta
