"""relp_add_columns / relp_reserve_columns / relp_column_stats of the tableau engine: columns added on the current basis without a
flush or a re-tabulation, through the ctypes binding, against a twin handle created on the wide LP and warm-started by
relp_from_basis on the mapped basis (only code that existed before these calls), the numpy solve of tests/column_reference.py and
the committed f64 oracle's fresh two-phase optimum of the wide LP.

LPs: lp = synthetic.dense_lp(m, n + k, seed); the engine gets A[:, :n], b, c[:n] (positive data: every LP here is bounded), the new
columns are A[:, n:] with the costs c[n:].  Shapes (24, 32, 1), (40, 300, 4: more than 256 stored columns), (300, 40, 5: more than
256 rows, a second chunk of the list), (257, 8, 2), (255, 8, 3) and (250, 12, 6); k in {1, 3, 9, 17} (a second and a third tile);
solved to the optimum with poll_interval = 1 and update_block 3 (a flush every third enqueued iteration) and -1 (64: the block stays
open, the add writes R0 too), with and without a flush before the add.  One sparse variant: column k keeps its rows i % 4 == k % 4.

By the f64 oracle: at every (shape, k) except (40, 300, 4) with k <= 9 at least one new column has d < -0.04 at the old optimum; at
(40, 300, 4) with k <= 9 all new columns have d > 0.2 -- the cases in which relp_run must make 0 pivots.

Column orders (tests/column_reference.py): engine [n | m slacks | k added], wide LP [n | k added | m slacks].

Tolerances: the project's 1e-9 relative on objectives (OBJ_RTOL) and 1e-9 * max(1, max|expected|) on vectors and matrices.  The
pending rows p that relp_column_stats reports are the DISTINCT pivot rows since the last flush, computed here from the trace."""
import functools
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic
from oracle import relp_f64

import column_reference as colref
import cut_reference as cutref

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-9
TOL_FEAS = 1e-7
IDENT_TOL = 1e-6              # check_basis: |B^-1 B - I| and |d_B|, the bound of tests/test_gpu_big_pins.py and test_gpu_lu_device.py
E_ARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
SHAPES = [(24, 32, 1), (40, 300, 4), (300, 40, 5), (257, 8, 2), (255, 8, 3), (250, 12, 6)]
COLUMNS = [1, 3, 9, 17]


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    """A, b, c of the dense <= LP (computed once, read only)."""
    lp = synthetic.dense_lp(m, n, seed)
    for v in lp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lp


@functools.lru_cache(maxsize=None)
def oracle_optimum(m, n, seed, k, sparse=False):
    """The f64 oracle's fresh two-phase optimum of the wide LP."""
    lp = dense_lp(m, n + k, seed)
    A_new, cost = colref.new_columns(lp, n, sparse)
    oracle = relp_f64.OracleF64(colref.wide(lp, n, A_new).ensure_csc())
    assert oracle.run() == "optimal"
    return oracle.objective


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


def solved(m, n, k, seed, **config):
    """(lp of n + k columns, a handle on its first n columns at the optimum)."""
    lp = dense_lp(m, n + k, seed)
    t = engine.Tableau(colref.narrow(lp, n), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
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


def assert_basis_state(t):
    ident, basic, min_b = t.check_basis()
    print(f"   check_basis: identity {ident:.3e}, basic costs {basic:.3e}, min b {min_b:.3e}")
    assert min_b >= -TOL_FEAS and ident <= IDENT_TOL and basic <= IDENT_TOL


def getters(t):
    """Everything a caller can read that an add or a reserve must or must not move, as bytes."""
    return dict(d=t.relative_costs().tobytes(), b=t.b().tobytes(), pi=t.minus_pi().tobytes(), basis=t.basis_indices().tobytes(),
                objective=t.objective_function_value(), trace=t.trace(), reinversions=t.reinversions(), flushes=t.flush_stats(),
                rhs=t.right_hand_side().tobytes(), rows=t.nr_rows(), columns=t.nr_columns(), cuts=t.cut_stats())


def old_part(g, n_old):
    """getters() restricted to what exists before an add of columns: d over the old columns, everything else whole."""
    return dict(g, d=g["d"][: 8 * n_old], columns=n_old)


def entries_of(column):
    return [(int(i), float(column[i])) for i in np.flatnonzero(column)]


def three_old_columns(basis, m, n):
    """One basic structural, one non-basic column and the last slack."""
    in_basis = set(int(x) for x in basis)
    basic = next(int(j) for j in basis if j < n)
    nonbasic = next(j for j in range(n + m) if j not in in_basis)
    return [basic, nonbasic, n + m - 1]


def compare_with(a, other, name, columns, m, n, k):
    """b, d, -pi, B^-1, generated columns and the objective of `a` (engine order) against `other`: a twin handle on the wide LP
    (wide order) or colref.Tableau (engine order)."""
    print(f"  against {name}:")
    if isinstance(other, colref.Tableau):
        b, d, pi, binv, objective = other.b, other.d, other.minus_pi, other.binv, other.objective
        column = lambda j: other.T[:, j]   # noqa: E731
    else:
        order = colref.wide_order(m, n, k)
        b, d, pi, binv, objective = other.b(), other.relative_costs()[order], other.minus_pi(), other.basis_inverse(), other.objective_function_value()
        column = lambda j: other.generate_column(int(order[j]))   # noqa: E731
    assert near(a.b(), b, "b")
    assert near(a.relative_costs(), d, "d")
    assert near(a.minus_pi(), pi, "-pi")
    assert near(a.basis_inverse(), binv, "B^-1")
    for j in columns:
        assert near(a.generate_column(j), column(j), f"column {j}")
    assert close_to(a.objective_function_value(), objective)


# ---- (a) against the rebuilds, (b) what must not move, (c) the re-solve -------------------------------------------------------
def check_add(m, n, seed, k, update_block, flush, sparse=False):
    lp, a = solved(m, n, k, seed, update_block=update_block)
    _, same = solved(m, n, k, seed, update_block=update_block)     # the same state (same bits): asked what would flush `a`
    p = pending_rows(a)
    if update_block == -1:
        assert p >= 1                                      # no flush has happened: every pivot row is pending
    if flush:
        a.flush()
        p = 0
    basis = a.basis_indices()
    A_new, cost = colref.new_columns(lp, n, sparse)
    touched = int(np.count_nonzero(np.abs(A_new).sum(axis=1)))
    old_columns = three_old_columns(basis, m, n)
    before = getters(a)
    old_generated = [a.generate_column(j).tobytes() for j in old_columns]
    assert a.column_stats() == (0, 0, 0, 0)
    a.add_columns(A_new, cost)
    print(f"({m}, {n}, {seed}) k {k} block {update_block} p {p}: {touched} identity columns read")
    assert a.column_stats() == (k, max(k, 16), touched, p)
    assert a.nr_rows() == m and a.nr_columns() == n + m + k
    # (b) bit for bit
    after = getters(a)
    assert old_part(after, n + m) == before
    assert [a.generate_column(j).tobytes() for j in old_columns] == old_generated
    d_new = a.relative_costs()[n + m:]
    for c in range(k):
        assert near(d_new[c], cost[c] + same.cost_difference_of(entries_of(A_new[:, c])), f"d of new column {c}")
    # (a) the twin on the wide LP and numpy; generate_column_of on the handle that was not touched
    md2 = colref.wide(lp, n, A_new)
    twin = twin_of(md2, colref.to_wide(basis, m, n, k), update_block=update_block)
    new_columns = [n + m + c for c in range(k)]                # every new column, against all three references
    for j in new_columns:
        assert near(a.generate_column(j), same.generate_column_of(entries_of(A_new[:, j - n - m])), f"column {j} against generate_column_of")
    compare_with(a, twin, "the twin", old_columns + new_columns, m, n, k)
    compare_with(a, colref.Tableau(md2, basis, m, n, k), "numpy", old_columns + new_columns, m, n, k)
    # (c) the re-solve
    tol_cost = float(a.config.tol_cost)
    expect_pivots = bool((d_new < -tol_cost).any())
    if not sparse:
        assert expect_pivots == (not ((m, n, seed) == (40, 300, 4) and k <= 9))     # what the f64 oracle found for these LPs
        assert (d_new.min() < -0.04) if expect_pivots else (d_new.min() > 0.2)
    pivots, outcome = a.run(1 << 20)
    optimum = oracle_optimum(m, n, seed, k, sparse)
    print(f"   run: {pivots} pivots, objective {a.objective_function_value():.12f}, oracle {optimum:.12f}")
    assert outcome == engine.OPTIMAL and (pivots >= 1) == expect_pivots
    assert close_to(a.objective_function_value(), optimum)
    ident, basic, min_b = a.check_basis()
    print(f"   check_basis: identity {ident:.3e}, basic costs {basic:.3e}, min b {min_b:.3e}")
    assert min_b >= -TOL_FEAS and ident <= IDENT_TOL and basic <= IDENT_TOL
    if update_block == -1:                                     # the pivots ran on W and R0 as widened: a flush changes nothing beyond rounding
        b_open, d_open = a.b(), a.relative_costs()
        a.flush()
        assert near(a.b(), b_open, "b after the flush") and near(a.relative_costs(), d_open, "d after the flush")
    assert twin.run(1 << 20)[1] == engine.OPTIMAL and close_to(twin.objective_function_value(), optimum)
    entered = any(e >= n + m for _, e, _, _ in a.trace()[len(before["trace"]):])
    for t in (a, twin, same):
        t.close()
    return entered


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("k", COLUMNS)
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_add_against_the_rebuilds(m, n, seed, k, update_block):
    entered = check_add(m, n, seed, k, update_block, flush=False)
    if (m, n, seed) == (24, 32, 1):
        assert entered                                         # a new column enters the basis (from the trace)


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("k", COLUMNS)
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_add_against_the_rebuilds_after_a_flush(m, n, seed, k, update_block):
    check_add(m, n, seed, k, update_block, flush=True)


@pytest.mark.parametrize("update_block", [3, -1])
def test_sparse_columns(update_block):
    check_add(300, 40, 5, 9, update_block, flush=False, sparse=True)


def test_the_order_inside_the_csc_cannot_change_a_bit():
    m, n, seed, k = 40, 300, 4, 3
    lp, a = solved(m, n, k, seed)
    _, c = solved(m, n, k, seed)
    A_new, cost = colref.new_columns(lp, n)
    a.add_columns(A_new, cost)
    ptr, idx, val = [0], [], []
    for col in A_new.T:                                        # the same columns with every column's entries reversed
        rows = np.arange(m)[::-1]
        idx += rows.tolist()
        val += col[rows].tolist()
        ptr.append(len(idx))
    c.add_columns((ptr, idx, val), cost)
    assert getters(a) == getters(c) and a.column_stats() == c.column_stats()
    for j in (0, n - 1, n + m, n + m + k - 1):
        assert a.generate_column(j).tobytes() == c.generate_column(j).tobytes()
    a.close()
    c.close()


def test_a_column_without_entries_and_explicit_zeros():
    m, n, seed, k = 24, 32, 1, 3
    lp, a = solved(m, n, k, seed)
    before = getters(a)
    a.add_columns(([0, 0, 2], [3, 5], [0.0, 0.0]), [1.5, -2.5])        # no entries; explicit zeros only
    assert a.column_stats()[:3] == (2, 16, 0) and old_part(getters(a), n + m) == before
    assert a.relative_costs()[n + m:].tolist() == [1.5, -2.5]
    assert not a.generate_column(n + m).any() and not a.generate_column(n + m + 1).any()
    pivots, outcome = a.run(1 << 20)                           # an empty column of negative cost: the LP is unbounded
    assert outcome == engine.UNBOUNDED
    a.close()


# ---- (d) growth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (300, 40, 5)])
def test_growth_with_a_column_present_and_a_block_open(m, n, seed):
    k = 17
    lp, step = solved(m, n, k, seed)
    _, step2 = solved(m, n, k, seed)
    _, once = solved(m, n, k, seed)
    _, reserved = solved(m, n, k, seed)
    assert pending_rows(step) >= 1
    basis = step.basis_indices()
    A_new, cost = colref.new_columns(lp, n)
    before = getters(step)
    step.reserve_columns(1)
    assert step.column_stats() == (0, 1, 0, 0) and getters(step) == before     # reserve alone: every getter bit-identical
    for j in (0, n, n + m - 1):
        assert step.generate_column(j).tobytes() == once.generate_column(j).tobytes()
    step.reserve_columns(0)
    step.reserve_columns(1)
    assert step.column_stats() == (0, 1, 0, 0) and step.cut_stats() == (0, 0, 0, 0)      # never shrinks; the rooms are independent
    step2.reserve_columns(1)
    for t in (step, step2):
        t.add_columns(A_new[:, :1], cost[:1])
        assert t.column_stats()[:2] == (1, 1)
        t.add_columns(A_new[:, 1:], cost[1:])                  # forces growth with a column present and the block open
        assert t.column_stats()[:2] == (17, 17)
    once.add_columns(A_new, cost)
    assert once.column_stats()[:2] == (17, 17)
    reserved.reserve_columns(40)
    assert reserved.column_stats() == (0, 40, 0, 0)
    reserved.add_columns(A_new, cost)
    assert reserved.column_stats()[:2] == (17, 40)
    assert getters(step) == getters(step2)                                     # the same calls: the same bits
    assert getters(once) == getters(reserved)                                  # room reserved or grown inside the add: the same bits
    assert getters(once) == getters(step)                                      # a column does not depend on the ones added with it
    for j in (0, n, n + m, n + m + 16):
        assert step.generate_column(j).tobytes() == step2.generate_column(j).tobytes()
        assert once.generate_column(j).tobytes() == reserved.generate_column(j).tobytes()
        assert once.generate_column(j).tobytes() == step.generate_column(j).tobytes()
    twin = twin_of(colref.wide(lp, n, A_new), colref.to_wide(basis, m, n, k))
    columns = three_old_columns(basis, m, n) + [n + m, n + m + 16]
    for name, t in (("1 + 16", step), ("17 at once", once), ("reserved", reserved)):
        print(name)
        compare_with(t, twin, "the twin", columns, m, n, k)
    optimum = oracle_optimum(m, n, seed, k)
    for t in (step, once, reserved):
        assert t.run(1 << 20)[1] == engine.OPTIMAL and close_to(t.objective_function_value(), optimum)
    for t in (step, step2, once, reserved, twin):
        t.close()


# ---- (e) the neighbours on the widened engine ---------------------------------------------------------------------------------
def widened_pair(m, n, seed, k, **config):
    lp, a = solved(m, n, k, seed, **config)
    basis = a.basis_indices()
    A_new, cost = colref.new_columns(lp, n)
    a.add_columns(A_new, cost)
    md2 = colref.wide(lp, n, A_new)
    return lp, a, twin_of(md2, colref.to_wide(basis, m, n, k), **config), md2, A_new, cost


@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (255, 8, 3)])
def test_rhs_change_ranging_and_ratios_on_the_widened_engine(m, n, seed):
    k = 3
    lp, a, twin, md2, A_new, cost = widened_pair(m, n, seed, k)
    order = colref.wide_order(m, n, k)
    rows = np.array([0, m // 2, m - 1], dtype=np.int32)
    for name in ("rhs_ranging", "row_ratios"):
        got, want = getattr(a, name)(rows), getattr(twin, name)(rows)
        for g, w in zip(got, want):
            if g.dtype == np.int32:
                if name == "row_ratios":                       # columns: the twin's index in the engine's order
                    w = np.array([-1 if x < 0 else int(colref.to_engine(x, m, n, k)) for x in w])
                assert g.tolist() == w.tolist(), name
            else:
                assert np.array_equal(np.isinf(g), np.isinf(w)), name
                finite = ~np.isinf(w)
                assert near(g[finite], w[finite], name) if finite.any() else True
    assert a.run(1 << 20)[1] == engine.OPTIMAL                # to the optimum of the wide LP: dual feasible, the state of an rhs change
    twin.from_basis(colref.to_wide(a.basis_indices(), m, n, k))
    values = np.array([lp["b"][0] * 0.9, lp["b"][m // 2] * 1.05])
    for t in (a, twin):
        t.change_right_hand_side(rows[:2], values)
    assert near(a.b(), twin.b(), "b after the rhs change")
    for t in (a, twin):
        assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), twin.objective_function_value())
    if colref.to_wide(a.basis_indices(), m, n, k).tolist() == twin.basis_indices().tolist():
        assert near(a.relative_costs(), twin.relative_costs()[order], "d at the new optimum")
    a.close()
    twin.close()


@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (40, 300, 4)])
def test_cost_calls_and_full_rhs_on_the_widened_engine(m, n, seed):
    k = 3
    lp, a, twin, md2, A_new, cost = widened_pair(m, n, seed, k)
    order = colref.wide_order(m, n, k)
    cols = np.arange(0, n, 3)
    c2 = np.array(lp["c"][:n])
    c2[cols] = 0.5 * c2[cols] - 0.125
    for t in (a, twin):
        t.change_cost(cols, c2[cols])
    assert near(a.relative_costs(), twin.relative_costs()[order], "d after the cost change")
    assert near(a.minus_pi(), twin.minus_pi(), "-pi after the cost change")
    assert close_to(a.objective_function_value(), twin.objective_function_value())
    for bad in (n, n + m, n + m + k - 1):                      # an added column is no structural column to these calls
        with pytest.raises(engine.RelpError) as err:
            a.change_cost([bad], [1.0])
        assert status_of(err) == E_ARG
        with pytest.raises(engine.RelpError) as err:
            a.set_upper_bound(bad, 1.0)
        assert status_of(err) == E_ARG
    assert a.cost().shape == (n,)
    c3 = 0.75 * c2 - 0.0625
    a.set_cost(c3)                                             # the added costs are kept
    twin.set_cost(np.concatenate([c3, cost]))
    assert near(a.relative_costs(), twin.relative_costs()[order], "d after set_cost")
    assert close_to(a.objective_function_value(), twin.objective_function_value())
    rhs = np.array(lp["b"]) * 1.01
    reinversions = a.reinversions()
    for t in (a, twin):
        t.set_right_hand_side(rhs)                             # a rebuild: it includes the columns
    assert a.reinversions() == reinversions + 1
    assert near(a.b(), twin.b(), "b after set_right_hand_side") and near(a.relative_costs(), twin.relative_costs()[order], "d")
    assert near(a.basis_inverse(), twin.basis_inverse(), "B^-1 after the rebuild")
    for j in (0, n + m, n + m + k - 1):
        assert near(a.generate_column(j), twin.generate_column(int(order[j])), f"column {j} after the rebuild")
    if a.b().min() >= -TOL_FEAS:                               # still primal feasible under the larger rhs: the primal loop goes on
        for t in (a, twin):
            assert t.run(1 << 20)[1] == engine.OPTIMAL
        assert close_to(a.objective_function_value(), twin.objective_function_value())
    a.close()
    twin.close()


@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (300, 40, 5)])
def test_rebuilds_with_an_added_column_basic(m, n, seed):
    k = 9
    lp, a, twin, md2, A_new, cost = widened_pair(m, n, seed, k)
    a.set_reinversion_interval(1)
    reinversions = a.reinversions()
    pivots, outcome = a.run(1)
    assert pivots == 1 and a.reinversions() == reinversions + 1
    assert (a.basis_indices() >= n + m).any()                  # the entering column is an added one: the host LU factorises it
    ref = colref.Tableau(md2, a.basis_indices(), m, n, k)
    assert near(a.b(), ref.b, "b after one pivot and a rebuild") and near(a.relative_costs(), ref.d, "d")
    assert near(a.basis_inverse(), ref.binv, "B^-1") and close_to(a.objective_function_value(), ref.objective)
    for j in (0, n + m, n + m + k - 1):
        assert near(a.generate_column(j), ref.T[:, j], f"column {j} after the rebuild")
    a.set_reinversion_interval(0)
    assert a.run(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), oracle_optimum(m, n, seed, k))
    basis = a.basis_indices()
    assert (basis >= n + m).any()
    rhs = np.array(lp["b"]) * 0.99                             # set_right_hand_side with added columns basic
    a.set_right_hand_side(rhs)
    ref = colref.Tableau(colref.wide(lp, n, A_new, b=rhs), basis, m, n, k)
    assert near(a.b(), ref.b, "b after set_right_hand_side") and near(a.relative_costs(), ref.d, "d")
    assert close_to(a.objective_function_value(), ref.objective)
    a.close()
    twin.close()


def test_from_basis_names_an_added_column():
    m, n, seed, k = 24, 32, 1, 3
    lp, a, twin, md2, A_new, cost = widened_pair(m, n, seed, k)
    assert a.run(1 << 20)[1] == engine.OPTIMAL
    optimum = a.objective_function_value()
    start = np.arange(n, n + m, dtype=np.int32)                # the all-slack basis with the first added column in row 0's place
    start[0] = n + m
    a.from_basis(start)
    ref = colref.Tableau(md2, start, m, n, k)
    assert near(a.b(), ref.b, "b of the named basis") and near(a.relative_costs(), ref.d, "d of the named basis")
    assert close_to(a.objective_function_value(), ref.objective)
    if ref.b.min() >= 0:
        assert a.run(1 << 20)[1] == engine.OPTIMAL and close_to(a.objective_function_value(), optimum)
    with pytest.raises(engine.RelpError):
        a.from_basis(np.concatenate([start[:-1], [n + m + k]]))    # behind the last column
    a.close()
    twin.close()


# ---- (f) interleaving with cuts -----------------------------------------------------------------------------------------------
def stacked_and_widened(A, b, c, n, blocks, nr_eq=0):
    """The LP a fresh engine gets for a sequence of adds, and engine index -> its index.  blocks: ("columns", A_new over the rows then
    present, cost) or ("cuts", G over the n structural columns, beta).  Its rows are the engine's (the first nr_eq of them == rows,
    which have no slack); its columns are [n | every added column | one slack per <= row]."""
    A, b, c = np.array(A, dtype=np.float64), np.array(b, dtype=np.float64), np.array(c, dtype=np.float64)
    m0 = A.shape[0]
    engine_columns = [("s", j) for j in range(n)] + [("r", i - nr_eq) for i in range(nr_eq, m0)]
    added = 0
    for kind, X, v in blocks:
        if kind == "columns":
            A = np.hstack([A, np.asarray(X, dtype=np.float64).reshape(A.shape[0], -1)])
            c = np.concatenate([c, np.atleast_1d(v)])
            engine_columns += [("a", added + x) for x in range(len(np.atleast_1d(v)))]
            added += len(np.atleast_1d(v))
        else:
            G = np.zeros((len(v), A.shape[1]))
            G[:, :n] = X
            engine_columns += [("r", A.shape[0] - nr_eq + x) for x in range(len(v))]
            A = np.vstack([A, G])
            b = np.concatenate([b, v])
    index = {"s": lambda j: j, "a": lambda x: n + x, "r": lambda i: n + added + i}
    to_twin = np.array([index[kind](x) for kind, x in engine_columns], dtype=np.int32)
    if nr_eq == 0:
        return MatrixData.from_dense_le(np.asfortranarray(A), b, c), to_twin
    md = MatrixData(nr_normal=A.shape[1], nr_eq=nr_eq, nr_range=0, nr_le=A.shape[0] - nr_eq, nr_ge=0, b=b, cost=c,
                    upper_bound=np.full(A.shape[1], np.inf), dense=np.asfortranarray(A))
    return md, to_twin


def structural_x(t, n):
    x = np.zeros(n)
    for j, v in t.current_bfs():
        if j < n:
            x[j] = v
    return x


def compare_interleaved(a, md2, to_twin, columns, **config):
    """`a` against a twin of the stacked and widened LP on a's basis (a re-tabulation), in the engine's order."""
    twin = twin_of(md2, to_twin[a.basis_indices()], **config)
    assert near(a.b(), twin.b(), "b") and near(a.relative_costs(), twin.relative_costs()[to_twin], "d")
    assert near(a.minus_pi(), twin.minus_pi(), "-pi") and near(a.basis_inverse(), twin.basis_inverse(), "B^-1")
    for j in columns:
        assert near(a.generate_column(j), twin.generate_column(int(to_twin[j])), f"column {j}")
    assert close_to(a.objective_function_value(), twin.objective_function_value())
    twin.close()


def oracle_of(md):
    oracle = relp_f64.OracleF64(md.ensure_csc())
    assert oracle.run() == "optimal"
    return oracle.objective


@pytest.mark.parametrize("bounds", [False, True])
@pytest.mark.parametrize("first", ["columns", "cuts"])
@pytest.mark.parametrize("update_block", [3, -1])
def test_columns_and_cuts_interleaved(first, update_block, bounds):
    """columns, run, cuts, run_dual, columns with entries in the cut rows, run -- and cuts, run_dual, columns, run: after each add
    against the twin of the stacked and widened LP on the same basis, after each solve against the oracle's optimum of that LP.
    bounds: three structural columns have loose upper bounds, stated to the twin as <= rows e_j' x <= u_j behind the constraints, so
    the engine has bound rows (and their slacks) between the constraints and whatever is added."""
    m0, n, seed, k = 24, 32, 1, 6
    lp = dense_lp(m0, n + k, seed)
    A0, b0, c0 = np.asarray(lp["A"])[:, :n], np.array(lp["b"]), np.array(lp["c"])[:n]
    A_new, cost = colref.new_columns(lp, n)
    config = dict(update_block=update_block)
    if bounds:
        bounded = [1, 7, 20]
        upper = np.full(n, np.inf)
        upper[bounded] = b0.max() * 1000.0                     # x_j <= b_i / a_ij <= 1000 b_i: the bounds never bind
        md = MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m0, nr_ge=0, b=b0, cost=c0, upper_bound=upper, dense=np.asfortranarray(A0))
        E = np.zeros((3, n))
        E[np.arange(3), bounded] = 1.0
        A0, b0 = np.vstack([A0, E]), np.concatenate([b0, upper[bounded]])
        A_new = np.vstack([A_new, np.zeros((3, k))])           # a new variable has no entry in a bound row of another variable
    else:
        md = MatrixData.from_dense_le(np.asfortranarray(A0), b0, c0)
    m = A0.shape[0]
    a = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    assert a.solve_relaxation() == engine.OPTIMAL and a.nr_rows() == m and a.nr_columns() == n + m
    rng = np.random.default_rng(17)
    blocks = []

    def add(kind, X, v, solve):
        before = getters(a)
        n_before, m_before = a.nr_columns(), a.nr_rows()
        blocks.append((kind, X, v))
        if kind == "columns":
            a.add_columns(X, v)
        else:
            a.add_cuts(X, v)
        after = getters(a)
        assert after["d"][: 8 * n_before] == before["d"] and after["b"][: 8 * m_before] == before["b"]
        assert after["objective"] == before["objective"] and after["trace"] == before["trace"] and after["reinversions"] == before["reinversions"]
        md2, to_twin = stacked_and_widened(A0, b0, c0, n, blocks)
        assert a.nr_columns() == len(to_twin)
        compare_interleaved(a, md2, to_twin, (0, n, n_before - 1, a.nr_columns() - 1), **config)
        pivots, outcome = getattr(a, solve)(1 << 20)
        optimum = oracle_of(md2)
        print(f"   {kind}, {solve}: {pivots} pivots, objective {a.objective_function_value():.12f}, oracle {optimum:.12f}")
        assert outcome == engine.OPTIMAL and close_to(a.objective_function_value(), optimum)
        assert_basis_state(a)
        compare_interleaved(a, md2, to_twin, (0, a.nr_columns() - 1), **config)

    def cuts():
        G = rng.integers(0, 8, (3, n)).astype(float)
        return G, 0.9 * (G @ structural_x(a, n))

    if first == "columns":
        add("columns", A_new[:, :3], cost[:3], "run")
        add("cuts", *cuts(), "run_dual")
        add("columns", np.vstack([A_new[:, 3:], rng.integers(1, 4, (3, 3)).astype(float)]), cost[3:], "run")
        assert a.column_stats()[:2] == (6, 16) and a.cut_stats()[:2] == (3, 16)
    else:
        add("cuts", *cuts(), "run_dual")
        add("columns", np.vstack([A_new, rng.integers(0, 3, (3, k)).astype(float)]), cost, "run")
        add("cuts", *cuts(), "run_dual")                       # and cuts behind the columns: coefficient 0 on every added column
        assert a.column_stats()[:2] == (6, 16) and a.cut_stats()[:2] == (6, 16)
    a.close()


def test_columns_on_the_equality_lp_of_the_cut_tests():
    """The LP of tests/test_gpu_cuts_in_place.py with == rows, some redundant: the phase switch removes rows before anything is added,
    and the stored columns keep the artificial block in front (col_off > 0), off which B^-1 is read.  Cuts, then columns with entries
    in every row, cut rows included.  References: the new columns formed in numpy from the engine's own B^-1 before the add, the same
    handle after a rebuild, and the f64 oracle's fresh solve of the LP with everything stacked (the coefficients of a new column in
    a redundant == row are the same combination of its coefficients in the independent ones)."""
    import test_gpu_cuts_in_place as cut_tests
    n, dup, k = 32, 3, 5
    base = cut_tests.equality_lp(dup)
    t = engine.Tableau(base, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, update_block=-1)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    m = t.nr_rows()
    assert m == 4 + 24
    G = np.random.default_rng(99).integers(0, 8, (3, n)).astype(float)
    beta = 0.9 * (G @ structural_x(t, n))
    t.add_cuts(G, beta)
    assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    m, ncol = t.nr_rows(), t.nr_columns()
    # the engine's == rows among the 4 + dup of the LP, by their rhs (exact values, distinct)
    dense = np.asarray(base.dense)
    E, bE = dense[: 4 + dup, :], np.asarray(base.b)[: 4 + dup]
    kept = [int(np.flatnonzero(bE == v)[0]) for v in t.right_hand_side()[:4]]
    assert len(set(kept)) == 4 and np.linalg.matrix_rank(E[kept]) == 4
    coefs = np.linalg.lstsq(E[kept].T, E.T, rcond=None)[0].T               # every == row as a combination of the kept ones
    assert np.allclose(coefs @ E[kept], E, atol=1e-9)
    rng = np.random.default_rng(7)
    a_eq = rng.integers(0, 3, (4, k)).astype(float)                        # new coefficients in the kept == rows, the <= rows, the cut rows
    a_le = rng.integers(0, 5, (24, k)).astype(float) / 4.0 + 0.25
    a_cut = rng.integers(0, 3, (3, k)).astype(float)
    cost = -rng.integers(1, 9, k).astype(float) / 4.0
    A_new = np.vstack([a_eq, a_le, a_cut])
    binv = np.stack([t.basis_inverse_row(r) for r in range(m)])            # (no flush: the block stays open)
    before = getters(t)
    old = [t.generate_column(j).tobytes() for j in (0, n, ncol - 1)]
    minus_pi = t.minus_pi()
    t.add_columns(A_new, cost)
    after = getters(t)
    assert old_part(after, ncol) == before and t.column_stats()[:2] == (k, 16) and t.nr_columns() == ncol + k
    assert [t.generate_column(j).tobytes() for j in (0, n, ncol - 1)] == old
    got = np.stack([t.generate_column(ncol + c) for c in range(k)], axis=1)
    assert near(got, binv @ A_new, "the new columns against numpy on B^-1 before")
    assert near(t.relative_costs()[ncol:], cost + minus_pi @ A_new, "d of the new columns")
    state = dict(b=t.b(), d=t.relative_costs(), pi=t.minus_pi(), cols=[t.generate_column(j) for j in (0, n, ncol, ncol + k - 1)])
    reinversions = t.reinversions()
    t.set_right_hand_side(t.right_hand_side())                             # the same handle rebuilt from its basis
    assert t.reinversions() == reinversions + 1
    assert near(t.b(), state["b"], "b after the rebuild") and near(t.relative_costs(), state["d"], "d after the rebuild")
    assert near(t.minus_pi(), state["pi"], "-pi after the rebuild")
    for j, col in zip((0, n, ncol, ncol + k - 1), state["cols"]):
        assert near(t.generate_column(j), col, f"column {j} after the rebuild")
    pivots, outcome = t.run(1 << 20)
    # the whole LP afresh: == rows (all of them), <= rows, cut rows; structural columns, then the new ones
    rows = np.vstack([np.hstack([E, coefs @ a_eq]), np.hstack([dense[4 + dup:], a_le]), np.hstack([G, a_cut])])
    whole = MatrixData(nr_normal=n + k, nr_eq=4 + dup, nr_range=0, nr_le=24 + 3, nr_ge=0, b=np.concatenate([np.asarray(base.b), beta]),
                       cost=np.concatenate([np.asarray(base.cost), cost]), upper_bound=np.full(n + k, np.inf), dense=np.asfortranarray(rows))
    optimum = oracle_of(whole)
    print(f"   run: {pivots} pivots, objective {t.objective_function_value():.12f}, oracle {optimum:.12f}")
    assert outcome == engine.OPTIMAL and close_to(t.objective_function_value(), optimum)
    assert_basis_state(t)
    t.close()


@pytest.mark.parametrize("first", ["columns", "cuts"])
def test_both_sequences_on_the_equality_lp_against_a_twin(first):
    """The two sequences of test_columns_and_cuts_interleaved on the equality LP of the cut tests: rows removed at the phase switch,
    the artificial block kept in front of the stored columns (col_off > 0), the update block open.  The twin is a fresh engine on
    the LP with the == rows the engine kept (found by their rhs), everything added so far stacked and widened, warm-started by
    relp_from_basis; the oracle solves that LP afresh.  Room for one cut is reserved before the three cuts, so relp_add_cuts grows
    the tableau -- and re-pitches the added columns' row-space block -- while columns are present ("columns" first)."""
    import test_gpu_cuts_in_place as cut_tests
    n, dup, k = 32, 3, 6
    base = cut_tests.equality_lp(dup)
    config = dict(update_block=-1)
    a = engine.Tableau(base, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    assert a.solve_relaxation() == engine.OPTIMAL and a.phase == 2 and a.nr_rows() == 4 + 24 and a.nr_columns() == n + 24
    dense, b_all = np.asarray(base.dense), np.asarray(base.b)
    kept = [int(np.flatnonzero(b_all[: 4 + dup] == v)[0]) for v in a.right_hand_side()[:4]]
    assert len(set(kept)) == 4
    A0 = np.vstack([dense[kept], dense[4 + dup:]])             # the engine's rows: the kept == rows, the <= rows
    b0, c0 = np.concatenate([b_all[kept], b_all[4 + dup:]]), np.asarray(base.cost)
    assert np.array_equal(a.right_hand_side(), b0)
    rng = np.random.default_rng(23)
    blocks = []

    def columns(count, rows):
        A_new = np.vstack([rng.integers(0, 3, (4, count)), rng.integers(1, 6, (24, count)) / 4.0, rng.integers(0, 3, (rows - 28, count))]).astype(float)
        return A_new, -rng.integers(1, 9, count).astype(float) / 4.0

    def add(kind, X, v, solve):
        before = getters(a)
        n_before, m_before = a.nr_columns(), a.nr_rows()
        old = [a.generate_column(j).tobytes() for j in (0, n, n_before - 1)]
        blocks.append((kind, X, v))
        if kind == "columns":
            a.add_columns(X, v)
            assert [a.generate_column(j).tobytes() for j in (0, n, n_before - 1)] == old
        else:
            a.add_cuts(X, v)
            assert [a.generate_column(j)[:m_before].tobytes() for j in (0, n, n_before - 1)] == [o[: 8 * m_before] for o in old]
        after = getters(a)
        assert after["d"][: 8 * n_before] == before["d"] and after["b"][: 8 * m_before] == before["b"]
        assert after["objective"] == before["objective"] and after["trace"] == before["trace"] and after["reinversions"] == before["reinversions"]
        md2, to_twin = stacked_and_widened(A0, b0, c0, n, blocks, nr_eq=4)
        assert a.nr_columns() == len(to_twin) and a.nr_rows() == md2.nr_eq + md2.nr_le
        compare_interleaved(a, md2, to_twin, range(a.nr_columns()), **config)      # every column of the tableau
        pivots, outcome = getattr(a, solve)(1 << 20)
        optimum = oracle_of(md2)
        print(f"   {kind}, {solve}: {pivots} pivots, objective {a.objective_function_value():.12f}, oracle {optimum:.12f}")
        assert outcome == engine.OPTIMAL and close_to(a.objective_function_value(), optimum)
        assert_basis_state(a)
        compare_interleaved(a, md2, to_twin, (0, n, a.nr_columns() - 1), **config)

    def cuts():
        G = rng.integers(0, 8, (3, n)).astype(float)
        return G, 0.9 * (G @ structural_x(a, n))

    if first == "columns":
        add("columns", *columns(3, 28), "run")
        a.reserve_cuts(1)
        assert a.cut_stats()[:2] == (0, 1) and a.column_stats()[:2] == (3, 16)
        add("cuts", *cuts(), "run_dual")                       # grows with columns present
        assert a.cut_stats()[:2] == (3, 16)
        add("columns", *columns(3, 31), "run")                 # entries in the cut rows
        assert a.column_stats()[:2] == (6, 16)
    else:
        add("cuts", *cuts(), "run_dual")
        add("columns", *columns(k, 31), "run")
        add("cuts", *cuts(), "run_dual")
        assert a.cut_stats()[:2] == (6, 16) and a.column_stats()[:2] == (6, 16)
    # and a rebuild of the whole thing from its basis: nothing moves beyond rounding
    state = dict(b=a.b(), d=a.relative_costs(), cols=[a.generate_column(j) for j in range(a.nr_columns())])
    a.set_right_hand_side(a.right_hand_side())
    assert near(a.b(), state["b"], "b after the rebuild") and near(a.relative_costs(), state["d"], "d after the rebuild")
    for j, col in enumerate(state["cols"]):
        assert near(a.generate_column(j), col, f"column {j} after the rebuild")
    a.close()


# ---- (g) refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    m, n, seed, k = 24, 32, 1, 3
    lp, a = solved(m, n, k, seed)
    A_new, cost = colref.new_columns(lp, n)
    a.add_columns(A_new[:, :1], cost[:1])
    before, stats = getters(a), a.column_stats()
    lib, h = a._lib, a._h

    def raw(count, ptr, idx, val, c):
        arrays = [None if x is None else np.ascontiguousarray(x, dtype=t) for x, t in
                  ((ptr, np.int64), (idx, np.int32), (val, np.float64), (c, np.float64))]
        return lib.relp_add_columns(h, count, *[None if x is None else x.ctypes.data for x in arrays])

    good = ([0, 2], [0, 1], [1.0, 2.0], [5.0])
    cases = {
        "count < 0": (-1, *good),
        "col_ptr missing": (1, None, *good[1:]),
        "cost missing": (1, *good[:3], None),
        "row_idx missing": (1, good[0], None, good[2], good[3]),
        "values missing": (1, good[0], good[1], None, good[3]),
        "col_ptr not from 0": (1, [1, 2], *good[1:]),
        "col_ptr descends": (2, [0, 2, 1], [0, 1], [1.0, 2.0], [5.0, 5.0]),
        "row below 0": (1, good[0], [-1, 1], *good[2:]),
        "row behind the last": (1, good[0], [0, m], *good[2:]),
        "row named twice": (1, good[0], [1, 1], *good[2:]),
        "coefficient nan": (1, good[0], good[1], [1.0, np.nan], good[3]),
        "coefficient inf": (1, good[0], good[1], [np.inf, 1.0], good[3]),
        "cost inf": (1, *good[:3], [np.inf]),
        "cost nan": (1, *good[:3], [np.nan]),
        "more columns than one launch takes": (8 * 65535 + 1, None, None, None, None),
    }
    for name, args in cases.items():
        assert raw(*args) == E_ARG, name
        assert a.column_stats() == stats and getters(a) == before, name
    assert lib.relp_reserve_columns(h, -1) == E_ARG
    assert raw(0, None, None, None, None) == 0                 # count == 0: a no-op, not counted
    a.add_columns(np.zeros((m, 0)), np.zeros(0))
    assert a.column_stats() == stats and getters(a) == before
    assert raw(*((1,) + good)) == 0                            # ... and the good call is taken
    assert a.column_stats()[0] == 2 and a.column_stats()[2] == 2
    a.close()


def test_refused_in_phase_one_and_on_the_other_engines():
    lp = dense_lp(24, 32, 1)
    cover, _ = __import__("dual_reference").covering_lp(6, 5, 3)          # >= rows: the engine starts in phase 1
    t = engine.Tableau(cover, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (lambda: t.add_columns(np.ones((t.nr_rows(), 1)), [1.0]), lambda: t.reserve_columns(4), t.column_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    t.close()
    md = MatrixData.from_dense_le(lp["A"], np.array(lp["b"]), np.array(lp["c"]))
    for kind in (engine.ENGINE_REVISED, engine.ENGINE_LU):
        t = engine.Tableau(md, engine=kind)
        assert t.solve_relaxation() == engine.OPTIMAL
        objective = t.objective_function_value()
        for call in (lambda: t.add_columns(np.ones((24, 1)), [1.0]), lambda: t.reserve_columns(4), t.column_stats):
            with pytest.raises(engine.RelpError) as err:
                call()
            assert status_of(err) == E_UNSUPPORTED
        assert t.nr_columns() == 32 + 24 and t.objective_function_value() == objective
        t.close()
