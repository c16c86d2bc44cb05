"""What relp_pool_reduced_costs, relp_pool_price and the column-generation loop must give (include/relp_engine.h), as
a test reference (not collected by pytest).

The price: `kernel_harness.fma_exact` chains -- d_k = cost_k, then fma((-pi)_row, value, d_k) over the column's nonzero entries by
ascending row -- and the winners in the total order (d, pool index) per share of ceil(count / segments) pool indices.

The column-generation instance: a small cutting-stock problem.  Rolls of length ROLL are cut into pieces of the widths WIDTHS to
meet DEMAND; a pattern says how many pieces of each width one roll gives, and it is maximal when the rest of the roll is shorter
than the shortest width.  The master LP is  min sum_p x_p,  sum_p a_ip x_p >= demand_i,  x >= 0.  The pool holds all 35 maximal
patterns; the initial LP has one pattern per width, floor(ROLL / width) pieces of that width alone (feasible by itself).  The loop
over Fractions here solves every master exactly with oracle/relp_exact.py, prices the pool with the exact duals and adds the winner
of every share; FULL_OPTIMUM is the exact optimum of the LP over all patterns, carried here because a GPU test cannot solve it.

The round cap.  The exact loop ends after EXACT_ROUNDS[segments] rounds that add columns (7 at one share, 2 at four;
tests/test_pool_reference.py runs it and holds these numbers to it).  The f64 engine follows the same rule with tol = 1e-7, but a
master LP of this kind is dual degenerate: another optimal basis has other duals, prices another winner and may need further
rounds.  round_cap(segments) = 2 * EXACT_ROUNDS[segments] leaves each exact round one round of detour; it is far below the trivial
bound len(pool) = 35 (every round adds a column never added before), so that it says something about the loop under test."""
from fractions import Fraction

import numpy as np

import kernel_harness as kh
from oracle import relp_exact as rx

ROLL = 60
WIDTHS = (25, 21, 17, 11, 7)
DEMAND = (30, 45, 60, 35, 50)
FULL_OPTIMUM = Fraction(985, 17)


# ------------------------------------------------------------------------------------------------------------------------
# the price
# ------------------------------------------------------------------------------------------------------------------------
def reduced_cost(cost, rows, values, minus_pi):
    """One fma chain from the cost over the nonzero entries, rows ascending."""
    acc = float(cost)
    for e in np.argsort(np.asarray(rows), kind="stable"):
        if values[e] != 0.0:
            acc = kh.fma_exact(float(minus_pi[rows[e]]), float(values[e]), acc)
    return acc


def reduced_costs(A, cost, minus_pi):
    """d of every column of the dense block A (rows x count)."""
    A = np.asarray(A, dtype=np.float64)
    return np.array([reduced_cost(cost[k], np.flatnonzero(A[:, k]), A[np.flatnonzero(A[:, k]), k], minus_pi) for k in range(A.shape[1])])


def winners(d, active, segments, tol):
    """(ids, d) of the winners of relp_pool_price, ascending share order."""
    count = len(d)
    size = (count + segments - 1) // segments
    ids = []
    for s in range(segments):
        best = -1
        for k in range(min(count, s * size), min(count, (s + 1) * size)):
            if active[k] and d[k] < -tol and (best < 0 or d[k] < d[best]):
                best = k
        if best >= 0:
            ids.append(best)
    return np.array(ids, dtype=np.int32), np.array([d[k] for k in ids], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# the cutting-stock instance
# ------------------------------------------------------------------------------------------------------------------------
def maximal_patterns():
    """Every maximal pattern, in descending lexicographic order of (pieces of WIDTHS[0], pieces of WIDTHS[1], ...)."""
    out = []

    def extend(i, left, pattern):
        if i == len(WIDTHS):
            if left < min(WIDTHS):
                out.append(tuple(pattern))
            return
        for pieces in range(left // WIDTHS[i], -1, -1):
            extend(i + 1, left - pieces * WIDTHS[i], pattern + [pieces])

    extend(0, ROLL, [])
    return out


def initial_patterns():
    return [tuple(ROLL // w if i == j else 0 for j in range(len(WIDTHS))) for i, w in enumerate(WIDTHS)]


def block(patterns):
    """The patterns as a dense rows x count block."""
    return np.array(patterns, dtype=np.float64).T.reshape(len(WIDTHS), len(patterns))


def exact_master(patterns):
    """The master LP over `patterns`, solved exactly: (objective, -pi)."""
    columns = [[(i, Fraction(a)) for i, a in enumerate(p) if a] for p in patterns]
    md = rx.MatrixData(columns, [Fraction(v) for v in DEMAND], [], 0, 0, 0, len(WIDTHS), [Fraction(1)] * len(patterns), [None] * len(patterns))
    result = rx.solve_relaxation(md)
    assert result["status"] == "optimal"
    minus_pi = result["tableau"].im.minus_pi
    assert len(minus_pi) == len(WIDTHS)                    # no row was removed: -pi is indexed by the demand rows
    return result["objective"], list(minus_pi)


def exact_column_generation(segments, max_rounds):
    """The loop of engine.column_generation over Fractions (tol = 0).  Returns (rounds that added columns, pool columns added in
    order, the final objective, whether the last pricing found nothing)."""
    pool = maximal_patterns()
    master, active, added, rounds = initial_patterns(), [True] * len(pool), [], 0
    size = (len(pool) + segments - 1) // segments
    while True:
        objective, minus_pi = exact_master(master)
        d = [1 + sum(minus_pi[i] * a for i, a in enumerate(p)) for p in pool]
        ids = []
        for s in range(segments):
            share = [k for k in range(s * size, min(len(pool), (s + 1) * size)) if active[k] and d[k] < 0]
            if share:
                ids.append(min(share, key=lambda k: (d[k], k)))
        if not ids:
            return rounds, added, objective, True
        if rounds >= max_rounds:
            return rounds, added, objective, False
        for k in ids:
            master.append(pool[k])
            active[k] = False
            added.append(k)
        rounds += 1


EXACT_ROUNDS = {1: 7, 4: 2}


def round_cap(segments):
    return 2 * EXACT_ROUNDS[segments]
