"""relp_add_cuts / relp_reserve_cuts / relp_cut_stats of the tableau engine: cut rows added on the current basis without a flush or
a re-tabulation, through the ctypes binding, against a twin handle created on the LP with the cuts stacked under A and warm-started
by relp_from_basis on the old basis plus the new slacks (only code that existed before these calls), the numpy solve of
tests/cut_reference.py and the committed f64 oracle's fresh two-phase optimum of the stacked LP.

LPs: `MatrixData.from_dense_le(**synthetic.dense_lp(m, n, seed))` at (24, 32, 1), (40, 300, 4: more than 256 stored columns), (300,
40, 5: more than 256 rows), (257, 8, 2), (255, 8, 3) and (250, 12, 6) -- 255 + 3 and 250 + 9 cross the 256-row block of the ratio
minima --, solved to the optimum with poll_interval = 1 and update_block 3 (a flush every third enqueued iteration) and -1 (64: the
block stays open, the add reads T0 + W R0).  Cuts: G = default_rng(1000 * seed + k).integers(0, 8, (k, n)), beta = 0.9 G x*, k in
{1, 3, 9}: every cut is violated at x*.  For these LPs (no bounds) the stacked LP has the engine's row and column indices exactly.

One LP has `==` rows, some redundant: its stored columns keep the artificial block in front, and the phase switch removes rows
before any cut is added (equality_lp).

Tolerances: the project's 1e-9 relative on objectives (OBJ_RTOL) and 1e-9 * max(1, max|expected|) on vectors and matrices.  The
pending rows p that relp_cut_stats reports are the DISTINCT pivot rows since the last flush, computed here from the trace
(tests/test_gpu_cost_in_place.py)."""
import functools
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic
from oracle import relp_f64

import cut_reference as cutref

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-9
TOL_FEAS = 1e-7
E_ARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
SHAPES = [(24, 32, 1), (40, 300, 4), (300, 40, 5), (257, 8, 2), (255, 8, 3), (250, 12, 6)]
CUTS = [1, 3, 9]


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    """A, b, c of the dense <= LP (computed once, read only)."""
    lp = synthetic.dense_lp(m, n, seed)
    for v in lp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lp


def le_md(lp):
    return MatrixData.from_dense_le(lp["A"], np.array(lp["b"]), np.array(lp["c"]))


@functools.lru_cache(maxsize=None)
def oracle_optimum(m, n, seed, k):
    """The f64 oracle's fresh two-phase optimum of the LP with the k cuts stacked under A (the basis of the cuts' x* is the oracle's)."""
    lp = dense_lp(m, n, seed)
    plain = relp_f64.OracleF64(le_md(lp).ensure_csc())
    assert plain.run() == "optimal"
    G, beta = cutref.cuts(lp, plain.basis(), k, seed)
    oracle = relp_f64.OracleF64(cutref.stacked(lp, G, beta).ensure_csc())
    assert oracle.run() == "optimal"
    return oracle.objective, plain.objective


def status_of(err):
    return int(re.search(r"\((-?\d+)\)", str(err.value)).group(1))


def close_to(value, expected):
    return abs(value - expected) <= OBJ_RTOL * max(1.0, abs(expected))


def bound_of(expected):
    return 1e-9 * max(1.0, float(np.abs(expected).max()))


def near(value, expected, what=""):
    err = float(np.abs(np.asarray(value) - np.asarray(expected)).max())
    print(f"   {what}: max error {err:.3e}, bound {bound_of(expected):.3e}")
    return err <= bound_of(expected)


def solved(m, n, seed, **config):
    lp = dense_lp(m, n, seed)
    t = engine.Tableau(le_md(lp), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    return lp, t


def twin_of(md, basis, **config):
    """A handle created on `md` and warm-started on `basis`: a re-tabulation, no code of the in-place add."""
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    t.from_basis(basis)
    return t


def pending_rows(t):
    """The distinct pivot rows since the last flush, from the trace of a handle of `solved()` that has only run its primal solve."""
    rows = [r for _, _, r, _ in t.trace()]
    flushed = t.update_block() * ((len(rows) + 1) // t.update_block())
    return len(set(rows[flushed:]))


def getters(t):
    """Everything a caller can read that an add or a reserve must or must not move, as bytes."""
    return dict(d=t.relative_costs().tobytes(), b=t.b().tobytes(), pi=t.minus_pi().tobytes(), basis=t.basis_indices().tobytes(),
                objective=t.objective_function_value(), trace=t.trace(), reinversions=t.reinversions(), flushes=t.flush_stats(),
                rhs=t.right_hand_side().tobytes(), rows=t.nr_rows(), columns=t.nr_columns())


def compare_with(a, other, name, columns, cut_row):
    """b, d, -pi, B^-1, three generated columns, a row of B^-1 and the objective of `a` against `other` (a handle or cutref.Tableau)."""
    print(f"  against {name}:")
    if isinstance(other, cutref.Tableau):
        b, d, pi, binv, objective = other.b, other.d, other.minus_pi, other.binv, other.objective
        column, binv_row = (lambda j: other.T[:, j]), (lambda r: other.binv[r])
    else:
        b, d, pi, binv, objective = other.b(), other.relative_costs(), other.minus_pi(), other.basis_inverse(), other.objective_function_value()
        column, binv_row = other.generate_column, other.basis_inverse_row
    assert near(a.b(), b, "b")
    assert near(a.relative_costs(), d, "d")
    assert near(a.minus_pi(), pi, "-pi")
    assert near(a.basis_inverse(), binv, "B^-1")
    for j in columns:
        assert near(a.generate_column(j), column(j), f"column {j}")
    assert near(a.basis_inverse_row(cut_row), binv_row(cut_row), f"row {cut_row} of B^-1")
    assert close_to(a.objective_function_value(), objective)


def three_columns(basis, m, n):
    """One basic structural, one non-basic structural (at (255, 8, 3) all eight are basic: the first non-basic slack then) and the
    first cut slack column."""
    in_basis = set(int(x) for x in basis)
    basic = next(int(j) for j in basis if j < n)
    nonbasic = next(j for j in range(n + m) if j not in in_basis)
    return [basic, nonbasic, n + m]


# ---- (a) against the rebuilds, (b) what must not move, (c) the re-solve -------------------------------------------------------
def check_add(m, n, seed, k, update_block, flush):
    lp, a = solved(m, n, seed, update_block=update_block)
    p = pending_rows(a)
    if update_block == -1:
        assert p >= 1                                      # no flush has happened: every pivot row is pending
    if flush:
        a.flush()
        p = 0
    basis = a.basis_indices()
    G, beta = cutref.cuts(lp, basis, k, seed)
    assert (G @ cutref.optimum_x(lp, basis) > beta).all()      # every cut is violated at x*
    touched = sorted(r for r in range(m) if basis[r] < n and G[:, basis[r]].any())
    assert 4 <= len(touched)
    before = getters(a)
    assert a.cut_stats() == (0, 0, 0, 0)
    a.add_cuts(G, beta)
    print(f"({m}, {n}, {seed}) k {k} block {update_block} p {p}: {len(touched)} rows read")
    assert a.cut_stats() == (k, max(k, 16), len(touched), p)
    assert a.nr_rows() == m + k and a.nr_columns() == n + m + k
    # (b) bit for bit
    after = getters(a)
    assert after["d"][: 8 * (n + m)] == before["d"] and after["b"][: 8 * m] == before["b"]
    assert after["objective"] == before["objective"] and after["basis"][: 4 * m] == before["basis"]
    assert after["trace"] == before["trace"] and after["reinversions"] == before["reinversions"] and after["flushes"] == before["flushes"]
    assert a.basis_indices()[m:].tolist() == list(range(n + m, n + m + k))
    assert (a.relative_costs()[n + m:] == 0.0).all() and (a.minus_pi()[m:] == 0.0).all()
    assert np.array_equal(a.right_hand_side(), np.concatenate([lp["b"], beta]))
    for j in [int(x) for x in basis]:
        assert (a.generate_column(j)[m:] == 0.0).all()         # new-row entries of the columns flagged basic
    for c in range(k):
        unit = np.zeros(m + k)
        unit[m + c] = 1.0
        assert np.array_equal(a.generate_column(n + m + c), unit)
    assert (a.b()[m:] < -TOL_FEAS).all()                       # violated cuts: the state run_dual starts from
    # (a) the twin on the stacked LP and numpy
    md2 = cutref.stacked(lp, G, beta)
    basis2 = cutref.extended_basis(basis, m, n, k)
    twin = twin_of(md2, basis2, update_block=update_block)
    columns = three_columns(basis, m, n)
    compare_with(a, twin, "the twin", columns, m + k - 1)
    compare_with(a, cutref.Tableau(md2, basis2), "numpy", columns, m + k - 1)
    # (c) the re-solve
    pivots, outcome = a.run_dual(1 << 20)
    optimum, plain = oracle_optimum(m, n, seed, k)
    print(f"   run_dual: {pivots} pivots, objective {a.objective_function_value():.12f}, oracle {optimum:.12f} (without cuts {plain:.12f})")
    assert outcome == engine.OPTIMAL and pivots >= 1
    assert close_to(a.objective_function_value(), optimum)
    ident, basic, min_b = a.check_basis()
    print(f"   check_basis: identity {ident:.3e}, basic costs {basic:.3e}, min b {min_b:.3e}")
    assert min_b >= -TOL_FEAS                                  # (the bound of tests/test_gpu_dual.py)
    if update_block == -1:                                     # the pivots ran on W and R0 as grown: a flush changes nothing beyond rounding
        b_open, d_open = a.b(), a.relative_costs()
        a.flush()
        assert near(a.b(), b_open, "b after the flush") and near(a.relative_costs(), d_open, "d after the flush")
        assert close_to(a.objective_function_value(), optimum)
    assert twin.run_dual(1 << 20)[1] == engine.OPTIMAL and close_to(twin.objective_function_value(), optimum)
    for t in (a, twin):
        t.close()


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("k", CUTS)
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_add_against_the_rebuilds(m, n, seed, k, update_block):
    check_add(m, n, seed, k, update_block, flush=False)


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("k", CUTS)
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_add_against_the_rebuilds_after_a_flush(m, n, seed, k, update_block):
    check_add(m, n, seed, k, update_block, flush=True)


def test_the_order_inside_the_csr_cannot_change_a_bit():
    m, n, seed, k = 40, 300, 4, 3
    lp, a = solved(m, n, seed)
    _, c = solved(m, n, seed)
    G, beta = cutref.cuts(lp, a.basis_indices(), k, seed)
    a.add_cuts(G, beta)
    ptr, idx, val = [0], [], []
    for row in G:                                              # the same cuts with every row's entries reversed, zeros included
        cols = np.arange(n)[::-1]
        idx += cols.tolist()
        val += row[cols].tolist()
        ptr.append(len(idx))
    c.add_cuts((ptr, idx, val), beta)
    assert getters(a) == getters(c)
    for j in (0, n - 1, n + m + k - 1):
        assert a.generate_column(j).tobytes() == c.generate_column(j).tobytes()
    assert a.basis_inverse().tobytes() == c.basis_inverse().tobytes()
    a.close()
    c.close()


# ---- (d) growth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (300, 40, 5)])
def test_growth_with_a_cut_present_and_a_block_open(m, n, seed):
    lp, step = solved(m, n, seed)
    _, step2 = solved(m, n, seed)
    _, once = solved(m, n, seed)
    _, reserved = solved(m, n, seed)
    assert pending_rows(step) >= 1
    basis = step.basis_indices()
    G, beta = cutref.cuts(lp, basis, 9, seed)
    before = getters(step)
    step.reserve_cuts(1)
    assert step.cut_stats() == (0, 1, 0, 0) and getters(step) == before        # reserve alone: every getter bit-identical
    for j in (0, n, n + m - 1):
        assert step.generate_column(j).tobytes() == once.generate_column(j).tobytes()
    step.reserve_cuts(0)
    step.reserve_cuts(1)
    assert step.cut_stats() == (0, 1, 0, 0)                                    # never shrinks, no-op when there is room
    step2.reserve_cuts(1)
    for t in (step, step2):
        t.add_cuts(G[:1], beta[:1])
        assert t.cut_stats()[:2] == (1, 1)
        t.add_cuts(G[1:], beta[1:])                                            # forces growth with a cut present and the block open
        assert t.cut_stats()[:2] == (9, 16)
    once.add_cuts(G, beta)
    reserved.reserve_cuts(9)
    assert reserved.cut_stats() == (0, 9, 0, 0)
    reserved.add_cuts(G, beta)
    assert reserved.cut_stats()[:2] == (9, 9)
    assert getters(step) == getters(step2)                                     # the same calls: the same bits
    assert getters(once) == getters(reserved)                                  # room reserved or grown inside the add: the same bits
    for j in (0, n, n + m + 8):
        assert step.generate_column(j).tobytes() == step2.generate_column(j).tobytes()
        assert once.generate_column(j).tobytes() == reserved.generate_column(j).tobytes()
    md2 = cutref.stacked(lp, G, beta)
    basis2 = cutref.extended_basis(basis, m, n, 9)
    twin = twin_of(md2, basis2)
    columns = three_columns(basis, m, n)
    for name, t in (("1 + 8", step), ("9 at once", once), ("reserved", reserved)):
        print(name)
        compare_with(t, twin, "the twin", columns, m + 8)
    optimum = oracle_optimum(m, n, seed, 9)[0]
    for t in (step, once, reserved):
        assert t.run_dual(1 << 20)[1] == engine.OPTIMAL and close_to(t.objective_function_value(), optimum)
    for t in (step, step2, once, reserved, twin):
        t.close()


# ---- (e) the neighbours on the grown engine -----------------------------------------------------------------------------------
def grown_pair(m, n, seed, k, **config):
    lp, a = solved(m, n, seed, **config)
    basis = a.basis_indices()
    G, beta = cutref.cuts(lp, basis, k, seed)
    a.add_cuts(G, beta)
    md2 = cutref.stacked(lp, G, beta)
    return lp, a, twin_of(md2, cutref.extended_basis(basis, m, n, k), **config), md2, G, beta


@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (255, 8, 3)])
def test_rhs_change_and_ranging_on_cut_rows(m, n, seed):
    k = 3
    lp, a, twin, md2, G, beta = grown_pair(m, n, seed, k)
    rows = np.array([m, m + 2, 0], dtype=np.int32)
    for name in ("rhs_ranging", "row_ratios"):
        got, want = getattr(a, name)(rows), getattr(twin, name)(rows)
        for g, w in zip(got, want):
            if g.dtype == np.int32:
                assert g.tolist() == w.tolist(), name
            else:
                assert np.array_equal(np.isinf(g), np.isinf(w)), name
                finite = ~np.isinf(w)
                assert near(g[finite], w[finite], name) if finite.any() else True
    values = np.array([beta[0] * 1.05, beta[2] * 0.97])
    for t in (a, twin):
        t.change_right_hand_side(rows[:2], values)
    assert near(a.b(), twin.b(), "b after the rhs change")
    assert np.array_equal(a.right_hand_side(), twin.right_hand_side())
    for t in (a, twin):
        assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), twin.objective_function_value())
    a.close()
    twin.close()


@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (40, 300, 4)])
def test_cost_change_and_full_rhs_on_the_grown_engine(m, n, seed):
    k = 3
    lp, a, twin, md2, G, beta = grown_pair(m, n, seed, k)
    cols = np.arange(0, n, 3)
    c2 = lp["c"].copy()
    c2[cols] = 0.5 * c2[cols] - 0.125
    for t in (a, twin):
        t.change_cost(cols, c2[cols])
    assert near(a.relative_costs(), twin.relative_costs(), "d after the cost change")
    assert near(a.minus_pi(), twin.minus_pi(), "-pi after the cost change")
    assert close_to(a.objective_function_value(), twin.objective_function_value())
    rhs = np.concatenate([lp["b"] * 1.01, beta * 1.02])
    reinversions = a.reinversions()
    for t in (a, twin):
        t.set_right_hand_side(rhs)                             # a rebuild: it includes the cuts
    assert a.reinversions() == reinversions + 1
    assert near(a.b(), twin.b(), "b after set_right_hand_side") and near(a.relative_costs(), twin.relative_costs(), "d")
    assert near(a.basis_inverse(), twin.basis_inverse(), "B^-1 after the rebuild")
    assert near(a.generate_column(0), twin.generate_column(0), "column 0 after the rebuild")
    a.close()
    twin.close()


@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (300, 40, 5)])
def test_reinversion_interval_one_rebuilds_with_the_cuts(m, n, seed):
    k = 9
    lp, a, twin, md2, G, beta = grown_pair(m, n, seed, k)
    a.set_reinversion_interval(1)
    reinversions = a.reinversions()
    pivots, outcome = a.run_dual(1)
    assert pivots == 1 and a.reinversions() == reinversions + 1
    ref = cutref.Tableau(md2, a.basis_indices())
    assert near(a.b(), ref.b, "b after one pivot and a rebuild") and near(a.relative_costs(), ref.d, "d")
    assert near(a.basis_inverse(), ref.binv, "B^-1")
    a.set_reinversion_interval(0)
    assert a.run_dual(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), oracle_optimum(m, n, seed, k)[0])
    a.close()
    twin.close()


def test_from_basis_names_the_cut_slacks():
    m, n, seed, k = 24, 32, 1, 3
    lp, a, twin, md2, G, beta = grown_pair(m, n, seed, k)
    assert a.run_dual(1 << 20)[1] == engine.OPTIMAL
    optimum = a.objective_function_value()
    start = cutref.extended_basis(np.arange(n, n + m), m, n, k)           # the all-slack basis of the grown LP
    a.from_basis(start)
    ref = cutref.Tableau(md2, start)
    assert near(a.b(), ref.b, "b of the slack basis") and near(a.relative_costs(), ref.d, "d of the slack basis")
    assert a.run(1 << 20)[1] == engine.OPTIMAL and close_to(a.objective_function_value(), optimum)
    a.close()
    twin.close()


# ---- (f) bound rows between the constraints and the cuts ----------------------------------------------------------------------
def test_bound_rows_between_the_constraints_and_the_cuts():
    """(24, 32, 1) with finite upper bounds, loose enough to stay inactive at x*, on three structural columns, one of them basic.
    Engine rows: 24 constraints | 3 bound rows | k cuts; columns: 32 structural | 24 slacks | 3 bound slacks | k cut slacks.  The
    twin states the bounds as <= rows e_j' x <= u_j in front of the cuts: its rows are the engine's, its columns too (the bound
    rows' slacks follow the constraint slacks in both)."""
    m, n, seed, k = 24, 32, 1, 3
    lp = dense_lp(m, n, seed)
    _, plain = solved(m, n, seed)
    basis0 = plain.basis_indices()
    plain.close()
    x = cutref.optimum_x(lp, basis0)
    basic = next(int(j) for j in basis0 if j < n and x[j] > 0)
    others = [j for j in range(n) if j not in set(int(v) for v in basis0)][:2]
    bounded = sorted([basic] + others)
    upper = np.full(n, np.inf)
    upper[bounded] = x[bounded] + 10.0
    md = MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=np.array(lp["b"]), cost=np.array(lp["c"]), upper_bound=upper,
                    dense=np.asfortranarray(lp["A"]))
    a = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1)
    assert a.solve_relaxation() == engine.OPTIMAL and a.nr_rows() == m + 3 and a.nr_columns() == n + m + 3
    basis = a.basis_indices()
    G, beta = cutref.cuts(lp, basis0, k, seed)
    E = np.zeros((3, n))
    E[np.arange(3), bounded] = 1.0
    before = getters(a)
    a.add_cuts(G, beta)
    assert a.nr_rows() == m + 3 + k and a.nr_columns() == n + m + 3 + k and a.cut_stats()[:2] == (k, 16)
    after = getters(a)
    assert after["d"][: 8 * (n + m + 3)] == before["d"] and after["b"][: 8 * (m + 3)] == before["b"] and after["objective"] == before["objective"]
    lp2 = dict(A=np.vstack([lp["A"], E]), b=np.concatenate([lp["b"], upper[bounded]]), c=lp["c"])
    md2 = cutref.stacked(lp2, G, beta)
    basis2 = cutref.extended_basis(basis, m + 3, n, k)
    twin = twin_of(md2, basis2)
    compare_with(a, twin, "the twin", three_columns(basis, m + 3, n), m + 3 + k - 1)
    compare_with(a, cutref.Tableau(md2, basis2), "numpy", three_columns(basis, m + 3, n), m + 3 + k - 1)
    oracle = relp_f64.OracleF64(md2.ensure_csc())
    assert oracle.run() == "optimal"
    assert a.run_dual(1 << 20)[1] == engine.OPTIMAL and close_to(a.objective_function_value(), oracle.objective)
    a.set_upper_bound(bounded[0], float(upper[bounded[0]]) + 1.0)          # the bound rows keep their indices
    assert a.right_hand_side()[m] == upper[bounded[0]] + 1.0
    a.close()
    twin.close()


# ---- equality rows, rows removed at the phase switch, the kept artificial block ------------------------------------------------
def equality_lp(dup, G=None, beta=None):
    """(24, 32, 1) with 4 independent == rows in front and `dup` more that are integer combinations of them (redundant: phase 1
    ends with `dup` artificial variables basic at zero and the phase switch removes their rows), optionally with cuts stacked as
    further <= rows.  The == rows hold at x_f = x* / 2 rounded down to 64ths, so every rhs is exact and x_f satisfies the <= rows."""
    lp = dense_lp(24, 32, 1)
    n = 32
    rng = np.random.default_rng(424242)
    oracle = relp_f64.OracleF64(le_md(lp).ensure_csc())
    assert oracle.run() == "optimal"
    x_f = np.floor(32.0 * cutref.optimum_x(lp, oracle.basis())) / 64.0
    R = rng.integers(0, 4, (4, n)).astype(float)
    C = rng.integers(0, 3, (dup, 4)).astype(float)
    C[C.sum(axis=1) == 0, 0] = 1.0
    E = np.vstack([R, C @ R])
    rows = [E, lp["A"]] + ([np.asarray(G, dtype=float)] if G is not None else [])
    b = [E @ x_f, lp["b"]] + ([np.asarray(beta, dtype=float)] if G is not None else [])
    k = 0 if G is None else len(beta)
    return MatrixData(nr_normal=n, nr_eq=4 + dup, nr_range=0, nr_le=24 + k, nr_ge=0, b=np.concatenate(b), cost=np.array(lp["c"]),
                      upper_bound=np.full(n, np.inf), dense=np.asfortranarray(np.vstack(rows)))


@pytest.mark.parametrize("dup,reserve", [(3, 1), (20, None), (20, 40)])
def test_cuts_after_the_phase_switch_removed_rows(dup, reserve):
    """More rows removed than the room adds (3 and reserve_cuts(1); 20 and the first add's room of 16): the growth must keep the
    pitches create() chose.  The LP has == rows, so the stored columns keep the artificial block in front (col_off > 0) and
    B^-1 is read off it.  References: the new rows formed in numpy from the engine's own tableau before the add, the same handle
    after a rebuild (relp_set_right_hand_side with the rhs in effect: host LU + re-tabulation with the cuts), and the f64 oracle's
    fresh solve of the LP with the cuts stacked."""
    n, k = 32, 3
    t = engine.Tableau(equality_lp(dup), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, update_block=-1)
    assert t.phase == 1 and t.nr_artificial_variables() == 4 + dup
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    m = t.nr_rows()
    assert m == 4 + 24                                          # the `dup` redundant rows are gone
    ncol = t.nr_columns()
    basis = t.basis_indices()
    T = np.stack([t.generate_column(j) for j in range(ncol)], axis=1)
    binv = np.stack([t.basis_inverse_row(r) for r in range(m)])           # (no flush: the block stays open)
    b0 = t.b()
    x = np.zeros(n)
    for j, v in t.current_bfs():
        if j < n:
            x[j] = v
    G = np.random.default_rng(99 + dup).integers(0, 8, (k, n)).astype(float)
    beta = 0.9 * (G @ x)
    before = getters(t)
    if reserve is not None:
        t.reserve_cuts(reserve)
        assert t.cut_stats() == (0, reserve, 0, 0) and getters(t) == before
        for j in (0, n, ncol - 1):
            assert t.generate_column(j).tobytes() == T[:, j].tobytes()
    t.add_cuts(G, beta)
    room = 16 if reserve in (None, 1) else reserve
    touched = [r for r in range(m) if basis[r] < n and G[:, basis[r]].any()]
    assert t.cut_stats()[:3] == (k, room, len(touched)) and t.nr_rows() == m + k and t.nr_columns() == ncol + k
    after = getters(t)
    assert after["d"][: 8 * ncol] == before["d"] and after["b"][: 8 * m] == before["b"] and after["objective"] == before["objective"]
    assert after["trace"] == before["trace"] and after["reinversions"] == before["reinversions"] and after["flushes"] == before["flushes"]
    GB = np.zeros((k, m))
    GB[:, touched] = G[:, basis[touched]]
    g_full = np.zeros((k, ncol))
    g_full[:, :n] = G
    want_rows = g_full - GB @ T
    got_rows = np.stack([t.generate_column(j)[m:] for j in range(ncol)], axis=1)
    assert near(got_rows, want_rows, "the new rows against numpy on the tableau before")
    assert near(t.b()[m:], beta - GB @ b0, "b of the new rows")
    for j in range(ncol):
        assert t.generate_column(j)[:m].tobytes() == T[:, j].tobytes()    # the old rows of the old columns
    for j in [int(v) for v in basis if v < ncol]:
        assert (got_rows[:, j] == 0.0).all()
    binv2 = np.stack([t.basis_inverse_row(r) for r in range(m + k)])
    want_binv = np.zeros((m + k, m + k))
    want_binv[:m, :m] = binv
    want_binv[m:, :m] = -GB @ binv
    want_binv[m:, m:] = np.eye(k)
    assert near(binv2, want_binv, "B^-1 read off the artificial block and the slacks")
    assert binv2[:m, :m].tobytes() == binv.tobytes()
    # the same handle rebuilt from its basis: the cut rows of A, the host LU with the cuts, the stored columns re-tabulated
    state = dict(b=t.b(), d=t.relative_costs(), pi=t.minus_pi(), cols=[t.generate_column(j) for j in (0, n, ncol, ncol + k - 1)])
    reinversions = t.reinversions()
    t.set_right_hand_side(t.right_hand_side())
    assert t.reinversions() == reinversions + 1
    assert near(t.b(), state["b"], "b after the rebuild") and near(t.relative_costs(), state["d"], "d after the rebuild")
    assert near(t.minus_pi(), state["pi"], "-pi after the rebuild")
    for j, col in zip((0, n, ncol, ncol + k - 1), state["cols"]):
        assert near(t.generate_column(j), col, f"column {j} after the rebuild")
    # the re-solve
    oracle = relp_f64.OracleF64(equality_lp(dup, G, beta).ensure_csc())
    assert oracle.run() == "optimal"
    pivots, outcome = t.run_dual(1 << 20)
    print(f"   run_dual: {pivots} pivots, objective {t.objective_function_value():.12f}, oracle {oracle.objective:.12f}")
    assert outcome == engine.OPTIMAL and pivots >= 1 and close_to(t.objective_function_value(), oracle.objective)
    assert t.check_basis()[2] >= -TOL_FEAS
    t.close()


@pytest.mark.parametrize("update_block", [3, -1])
def test_primal_run_on_the_grown_tableau(update_block):
    """relp_run directly on the tableau as grown in place (no re-tabulation in between): the cuts added, the dual re-solve, then a
    cost change and the primal loop -- whose fused update swaps the second copies of b and the basis per pivot -- to the optimum of
    the stacked LP under the new costs."""
    m, n, seed, k = 40, 300, 4, 9
    lp, t = solved(m, n, seed, update_block=update_block)
    G, beta = cutref.cuts(lp, t.basis_indices(), k, seed)
    t.add_cuts(G, beta)
    assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    c2 = lp["c"].copy()
    c2[::3] = 0.5 * c2[::3] - 0.125
    t.change_cost(np.arange(0, n, 3), c2[::3])
    pivots, outcome = t.run(1 << 20)
    oracle = relp_f64.OracleF64(cutref.stacked(lp, G, beta, cost=c2).ensure_csc())
    assert oracle.run() == "optimal"
    print(f"   run: {pivots} pivots, objective {t.objective_function_value():.12f}, oracle {oracle.objective:.12f}")
    assert outcome == engine.OPTIMAL and pivots >= 1 and t.reinversions() == 0
    assert close_to(t.objective_function_value(), oracle.objective)
    ref = cutref.Tableau(cutref.stacked(lp, G, beta, cost=c2), t.basis_indices())
    assert near(t.b(), ref.b, "b at the optimum") and near(t.relative_costs(), ref.d, "d at the optimum")
    ident, basic, min_b = t.check_basis()
    assert min_b >= -TOL_FEAS
    t.close()


# ---- (g) refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    m, n, seed = 24, 32, 1
    lp, a = solved(m, n, seed)
    G, beta = cutref.cuts(lp, a.basis_indices(), 3, seed)
    a.add_cuts(G[:1], beta[:1])
    before, stats = getters(a), a.cut_stats()
    lib, h = a._lib, a._h

    def raw(count, ptr, idx, val, rhs):
        arrays = [None if x is None else np.ascontiguousarray(x, dtype=t) for x, t in
                  ((ptr, np.int64), (idx, np.int32), (val, np.float64), (rhs, np.float64))]
        return lib.relp_add_cuts(h, count, *[None if x is None else x.ctypes.data for x in arrays])

    good = ([0, 2], [0, 1], [1.0, 2.0], [5.0])
    cases = {
        "count < 0": (-1, *good),
        "row_ptr missing": (1, None, *good[1:]),
        "rhs missing": (1, *good[:3], None),
        "col_idx missing": (1, good[0], None, good[2], good[3]),
        "values missing": (1, good[0], good[1], None, good[3]),
        "row_ptr not from 0": (1, [1, 2], *good[1:]),
        "row_ptr descends": (2, [0, 2, 1], [0, 1], [1.0, 2.0], [5.0, 5.0]),
        "column below 0": (1, good[0], [-1, 1], *good[2:]),
        "a virtual column": (1, good[0], [0, n], *good[2:]),
        "column named twice": (1, good[0], [1, 1], *good[2:]),
        "coefficient nan": (1, good[0], good[1], [1.0, np.nan], good[3]),
        "coefficient inf": (1, good[0], good[1], [np.inf, 1.0], good[3]),
        "rhs inf": (1, *good[:3], [np.inf]),
    }
    for name, args in cases.items():
        assert raw(*args) == E_ARG, name
        assert a.cut_stats() == stats and getters(a) == before, name
    assert lib.relp_reserve_cuts(h, -1) == E_ARG
    assert raw(0, None, None, None, None) == 0                 # count == 0: a no-op
    a.add_cuts(np.zeros((0, n)), np.zeros(0))
    assert a.cut_stats() == stats and getters(a) == before
    assert raw(*((1,) + good)) == 0                            # ... and the good call is taken
    assert a.cut_stats()[0] == 2
    a.close()


def test_refused_in_phase_one_and_on_the_other_engines():
    lp = dense_lp(24, 32, 1)
    G, beta = np.ones((1, 32)), np.array([1.0])
    cover, _ = __import__("dual_reference").covering_lp(6, 5, 3)          # >= rows: the engine starts in phase 1
    t = engine.Tableau(cover, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (lambda: t.add_cuts(np.ones((1, 5)), [1.0]), lambda: t.reserve_cuts(4), t.cut_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    t.close()
    for kind in (engine.ENGINE_REVISED, engine.ENGINE_LU):
        t = engine.Tableau(le_md(lp), engine=kind)
        assert t.solve_relaxation() == engine.OPTIMAL
        objective = t.objective_function_value()
        for call in (lambda: t.add_cuts(G, beta), lambda: t.reserve_cuts(4), t.cut_stats):
            with pytest.raises(engine.RelpError) as err:
                call()
            assert status_of(err) == E_UNSUPPORTED
        assert t.nr_rows() == 24 and t.objective_function_value() == objective
        t.close()
