"""What relp_cutpool_slacks, relp_cutpool_separate and the row-generation loop must give (include/relp_engine.h), as a
test reference (not collected by pytest).

The separation: `kernel_harness.fma_exact` chains -- x_j = b[r] where structural column j is basic in row r, else +0.0;
acc = 0.0, then fma(g_kj, x_j, acc) over the cut's nonzero entries by ascending column; s_k = rhs_k - acc -- the norms as one fma
chain of squares and a square root, and the winners in the total order (key, pool index) per share of ceil(count / segments) pool
indices, key = s_k or s_k / norm_k (norm 0 counts as 1), candidates s_k < -tol.

The row-generation instance: tangent half-planes of a ball around a box-bounded LP.  min c'x over the box 0 <= x <= SIDE in DIM
dimensions (the box as DIM rows x_j <= SIDE of the initial LP) and over CUTS half-planes a_k'x <= a_k'p + RADIUS |a_k| tangent to
the ball of radius RADIUS around the centre p of the box, a_k integer directions from a fixed linear congruential sequence.  The
ball cuts the corners of the box off, and c points into a corner, so the optimum lies on tangent planes and the box alone is far
from it.  The right-hand sides are rounded to f64 once, here; the LP "over all cuts" is the LP with exactly these f64 data, which
is what the engine is given too.  The loop over Fractions solves every LP exactly with oracle/relp_exact.py, separates the pool at
its exact vertex (tol = 0) and adds the winner of every share; when nothing is violated the vertex is feasible for the LP over
all cuts and optimal for a relaxation of it, hence optimal for it: FULL_OPTIMUM is that objective, carried here because a GPU test
cannot run the exact loop (tests/test_cutpool_reference.py runs it and holds the constant to it).

The round cap.  The exact loop ends after EXACT_ROUNDS[(per_round, by_efficacy)] rounds that add cuts.  The f64 engine follows the
same rule with tol = 1e-7 from vertices that differ from the exact ones in the last bits, so a cut violated by less than that is
not added and a near-tie between two cuts may go the other way, after which the paths differ.  round_cap = 2 * EXACT_ROUNDS + 2
leaves every exact round one round of detour; it is far below the trivial bound CUTS (every round adds a cut never added before),
so that it says something about the loop under test."""
from fractions import Fraction

import numpy as np

import kernel_harness as kh
from oracle import relp_exact as rx

DIM, SIDE, RADIUS, CUTS = 6, 10.0, 6.0, 300
COST = (-5.0, -4.0, -6.0, -3.0, -5.5, -4.5)


# ------------------------------------------------------------------------------------------------------------------------
# the separation
# ------------------------------------------------------------------------------------------------------------------------
def vertex(b, basis, nr_normal):
    x = np.zeros(nr_normal)
    for r, j in enumerate(basis):
        if 0 <= j < nr_normal:
            x[j] = b[r]
    return x


def slack(rhs, cols, values, x):
    """rhs - (one fma chain from 0.0 over the nonzero entries, columns ascending)."""
    acc = 0.0
    for e in np.argsort(np.asarray(cols), kind="stable"):
        if values[e] != 0.0:
            acc = kh.fma_exact(float(values[e]), float(x[cols[e]]), acc)
    return float(rhs) - acc


def slacks(G, rhs, x):
    """s of every cut of the dense block G (count x nr_normal) at x."""
    G = np.asarray(G, dtype=np.float64)
    return np.array([slack(rhs[k], np.flatnonzero(G[k]), G[k, np.flatnonzero(G[k])], x) for k in range(G.shape[0])])


def norms(G):
    out = []
    for row in np.asarray(G, dtype=np.float64):
        acc = 0.0
        for v in row[np.flatnonzero(row)]:
            acc = kh.fma_exact(float(v), float(v), acc)
        out.append(float(np.sqrt(acc)))
    return np.array(out)


def winners(s, norm, active, segments, tol, by_efficacy=False):
    """(ids, slacks) of the winners of relp_cutpool_separate, ascending share order."""
    count = len(s)
    key = [float(s[k]) / (1.0 if norm[k] == 0.0 else float(norm[k])) if by_efficacy else float(s[k]) for k in range(count)]
    size = (count + segments - 1) // segments
    ids = []
    for sg in range(segments):
        best = -1
        for k in range(min(count, sg * size), min(count, (sg + 1) * size)):
            if active[k] and s[k] < -tol and (best < 0 or key[k] < key[best]):
                best = k
        if best >= 0:
            ids.append(best)
    return np.array(ids, dtype=np.int32), np.array([s[k] for k in ids], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# the row-generation instance
# ------------------------------------------------------------------------------------------------------------------------
def instance():
    """(G, rhs): the CUTS tangent half-planes as a dense CUTS x DIM block of integer directions and their f64 right-hand sides."""
    state, G = 12345, np.zeros((CUTS, DIM))
    for k in range(CUTS):
        while True:
            row = []
            for _ in range(DIM):
                state = (state * 1103515245 + 12345) % (1 << 31)
                row.append(float((state >> 16) % 19 - 9))
            if any(row):
                break
        G[k] = row
    centre = SIDE / 2
    rhs = np.array([float(G[k].sum() * centre + RADIUS * np.sqrt(float((G[k] * G[k]).sum()))) for k in range(CUTS)])
    return G, rhs


def exact_lp(G, rhs, rows):
    """min COST'x over the box and the cuts `rows`, solved exactly: (objective, x)."""
    columns = []
    for j in range(DIM):
        columns.append([(j, Fraction(1))] + [(DIM + i, Fraction(G[k, j])) for i, k in enumerate(rows) if G[k, j] != 0.0])
    b = [Fraction(SIDE)] * DIM + [Fraction(float(rhs[k])) for k in rows]
    md = rx.MatrixData(columns, b, [], 0, 0, DIM + len(rows), 0, [Fraction(c) for c in COST], [None] * DIM)
    result = rx.solve_relaxation(md)
    assert result["status"] == "optimal"
    x = [Fraction(0)] * DIM
    for j, v in result["bfs"]:
        if j < DIM:
            x[j] = v
    return result["objective"], x


def exact_row_generation(per_round, max_rounds, by_efficacy=False):
    """The loop of engine.row_generation over Fractions (tol = 0).  Returns (rounds that added cuts, pool cuts added in order, the
    final objective, the final x, whether the last separation found nothing).  By efficacy the candidates (s < 0) are ranked by
    -s^2 / |a|^2, the order of s / |a| without the square root."""
    G, rhs = instance()
    active, added, rounds = [True] * CUTS, [], 0
    norm2 = [sum(Fraction(v) ** 2 for v in G[k]) for k in range(CUTS)]
    size = (CUTS + per_round - 1) // per_round
    while True:
        objective, x = exact_lp(G, rhs, added)
        s = [Fraction(float(rhs[k])) - sum(Fraction(G[k, j]) * x[j] for j in range(DIM)) for k in range(CUTS)]
        key = [-(s[k] * s[k]) / norm2[k] if by_efficacy else s[k] for k in range(CUTS)]
        ids = []
        for sg in range(per_round):
            share = [k for k in range(sg * size, min(CUTS, (sg + 1) * size)) if active[k] and s[k] < 0]
            if share:
                ids.append(min(share, key=lambda k: (key[k], k)))
        if not ids:
            return rounds, added, objective, x, True
        if rounds >= max_rounds:
            return rounds, added, objective, x, False
        for k in ids:
            active[k] = False
            added.append(k)
        rounds += 1


EXACT_ROUNDS = {(1, False): 9, (1, True): 8, (8, False): 4, (8, True): 4}
FULL_OPTIMUM = Fraction(-226065260124238400703, 1023407830947856384)          # -220.89459674630595; the box alone gives -280


def round_cap(per_round, by_efficacy=False):
    return 2 * EXACT_ROUNDS[(per_round, bool(by_efficacy))] + 2
