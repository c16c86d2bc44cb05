"""relp_row_ratios / relp_rhs_ranging / relp_ranging_stats of the tableau engine: the batched ratio tests over rows of T (branching
penalties, cost ranges) and over the identity columns (rhs ranges), through the ctypes binding, against the engine's own step-wise
calls (bit level), the numpy reference tests/ranging_reference.py (started from the engine's basis at test time) and the merged rhs
calls (a move past a reported bound makes the reported row the dual loop's first pivot row).

LPs and handles are those of tests/test_gpu_rhs_in_place.py (`solved`: poll_interval = 1, trace_capacity = 4096): dense <= LPs at
(24, 32, 1), (40, 300, 4: 340 stored columns, two column blocks), (300, 40, 5: two row blocks) and (257, 8, 2: the second row block
holds one row), each with update_block 3 (flushed often) and -1 (64: the block is open, the queries read T0 + W R0); the pending rows
p come from the trace as in that file.  Engine row k has the identity column n + k (its slack).

At the optimal bases of all four LPs every tie band of the reference holds one entry and the smallest relative gap to a runner-up is
4.7e-6 (row ratios) and 9.5e-4 (ranging); every row has candidates in both directions of relp_row_ratios and a decrease bound, and 16 /
20 / 277 / 251 rows (the basic slacks, whose column of B^-1 is a unit vector) have no increase bound.  `reference()` asserts band == 1
and gap > 1e-7 for every entry, so no entry is left out of any comparison."""
import functools

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine

import dual_reference as dr
import ranging_reference as rr
from test_gpu_rhs_in_place import (E_ARG, E_STATE, E_UNSUPPORTED, PRIMAL_PIVOTS, TOL_FEAS, close_to, dense_lp, dual_trace, le_lp,
                                   pending_rows, solved, status_of)

pytestmark = pytest.mark.gpu

LPS = [(24, 32, 1), (40, 300, 4), (300, 40, 5), (257, 8, 2)]
NO_INCREASE = {(24, 32, 1): 16, (40, 300, 4): 20, (300, 40, 5): 277, (257, 8, 2): 251}
FINITE_MOVES = {(24, 32, 1): 32, (40, 300, 4): 60, (300, 40, 5): 323, (257, 8, 2): 263}
QUOTIENT_RTOL = 8 * 2.0 ** -52                   # two IEEE quotients of the same bits
TOL_ZERO = dr.TOLERANCES["tol_zero"]


def pending(t, key, update_block):
    """The pending rows p of a handle of `solved()`, from its trace (pending_rows of tests/test_gpu_rhs_in_place.py).  8 pivots with
    update_block 3 are 2 past a multiple of 3: the one no-op iteration after the last pivot completes the block, which is flushed."""
    if update_block == 3 and PRIMAL_PIVOTS[key] % 3 == 2:
        return 0
    p = pending_rows(t)
    if update_block == 3:
        assert p == PRIMAL_PIVOTS[key] % 3
    else:
        assert 1 <= p <= PRIMAL_PIVOTS[key]                   # no flush has happened: every pivot row is pending
    return p


@functools.lru_cache(maxsize=None)
def reference(m, n, seed, basis):
    """(T, b, d, in_basis, [(down, up)], [(decrease, increase)]) of the reference at `basis` (a tuple), every row; computed once per
    basis and read only.  Asserts what the module docstring states."""
    lp = dense_lp(m, n, seed)
    T, b, d, in_basis = rr.tableau(le_lp(lp, lp["b"]), basis)
    ratios = rr.row_ratios(T, d, in_basis, range(m))
    ranging = rr.rhs_ranging(T, b, basis, np.arange(n, n + m), range(m))
    for pick in [p for pair in ratios for p in pair] + [dec for dec, _ in ranging]:
        assert pick.band == 1 and pick.gap > 1e-7
    for _, inc in ranging:
        assert inc.band in (0, 1) and (inc.band == 0 or inc.gap > 1e-7)
    assert sum(1 for _, inc in ranging if inc.index < 0) == NO_INCREASE[(m, n, seed)]
    for a in (T, b, d):
        a.setflags(write=False)
    return T, b, d, in_basis, ratios, ranging


def reference_of(t, key):
    return reference(*key, tuple(int(j) for j in t.basis_indices()))


def dz(v):
    return 0.0 if v <= TOL_ZERO else v


def same_quotient(value, expected):
    return abs(value - expected) <= QUOTIENT_RTOL * abs(expected)


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", LPS)
def test_equal_to_the_step_wise_calls(m, n, seed, update_block):
    lp, t = solved(m, n, seed, update_block=update_block)
    p = pending(t, (m, n, seed), update_block)
    rows = np.arange(m)
    assert t.ranging_stats() == (0, 0, 0, 0)
    down, down_col, up, up_col = t.row_ratios(rows)
    dec, dec_row, inc, inc_row = t.rhs_ranging(rows)
    assert t.ranging_stats() == (1, m, 1, p)
    d, b = t.relative_costs(), t.b()
    columns = {}

    def column(j):
        if j not in columns:
            columns[j] = t.generate_column(int(j))
        return columns[j]

    for r in range(m):
        stepwise = t.select_dual_pivot_column(r)
        assert down_col[r] == (-1 if stepwise is None else stepwise)
        assert down_col[r] >= 0 and up_col[r] >= 0            # every row has candidates in both directions here
        assert same_quotient(down[r], dz(d[down_col[r]]) / -column(down_col[r])[r])
        assert same_quotient(up[r], dz(d[up_col[r]]) / column(up_col[r])[r])
    for k in range(m):
        col = t.generate_column(n + k)
        stepwise = t.select_primal_pivot_row()
        assert dec_row[k] == (-1 if stepwise is None else stepwise) and dec_row[k] >= 0
        assert same_quotient(dec[k], dz(b[dec_row[k]]) / col[dec_row[k]])
        if inc_row[k] >= 0:
            assert same_quotient(inc[k], dz(b[inc_row[k]]) / -col[inc_row[k]])
        else:
            assert inc[k] == np.inf and not (col < -dr.TOLERANCES["tol_pivot"]).any()
    t.close()


def seventeen_rows(m):
    """17 rows in no order, one of them twice."""
    rows = (np.arange(17) * 7 + 3) % m
    rows = rows[[11, 2, 16, 0, 7, 13, 4, 9, 1, 15, 6, 10, 3, 14, 8, 12, 5]]
    rows[9] = rows[2]
    return rows.astype(np.int32)


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", LPS)
def test_equal_to_the_numpy_reference(m, n, seed, update_block):
    lp, t = solved(m, n, seed, update_block=update_block)
    p = pending(t, (m, n, seed), update_block)
    _, _, _, _, ratios, ranging = reference_of(t, (m, n, seed))
    lists = [np.arange(m, dtype=np.int32), np.array([m // 2], dtype=np.int32), seventeen_rows(m)]
    for rows in lists:
        down, down_col, up, up_col = t.row_ratios(rows)
        dec, dec_row, inc, inc_row = t.rhs_ranging(rows)
        assert down_col.tolist() == [ratios[r][0].index for r in rows] and up_col.tolist() == [ratios[r][1].index for r in rows]
        assert dec_row.tolist() == [ranging[r][0].index for r in rows] and inc_row.tolist() == [ranging[r][1].index for r in rows]
        for got, which in ((down, lambda r: ratios[r][0]), (up, lambda r: ratios[r][1]), (dec, lambda r: ranging[r][0]),
                           (inc, lambda r: ranging[r][1])):
            assert [bool(np.isinf(v)) for v in got] == [which(r).index < 0 for r in rows]
        worst = max(abs(v - ranging[r][0].ratio) / max(1.0, abs(v)) for v, r in zip(dec, rows))
        print(f"{len(rows)} rows, p = {p}: max relative |decrease - reference| = {worst:.3e}")
    assert t.ranging_stats() == (3, m + 1 + 17, 3, p)
    t.close()


def test_slack_basis_the_full_tie_band_and_the_empty_directions():
    """T = [A | I] with A > 0 and d = c < 0: no down candidate anywhere; every up ratio is exactly 0 (d_j <= tol_zero reads as 0) with
    all 300 structural columns of both column blocks in the band, so column 0 wins; B^-1 = I, so nothing bounds an increase and row k
    itself bounds the decrease at rhs_k."""
    m, n, seed = 40, 300, 4
    lp = dense_lp(m, n, seed)
    assert (lp["A"] > 0).all() and (lp["c"] < 0).all()
    t = engine.Tableau(le_lp(lp, lp["b"]), engine=engine.ENGINE_TABLEAU)
    t.from_basis(dr.surplus_basis(m, n))
    rows = np.arange(m)
    down, down_col, up, up_col = t.row_ratios(rows)
    assert np.isinf(down).all() and (down > 0).all() and (down_col == -1).all()
    assert (up == 0.0).all() and (up_col == 0).all()
    dec, dec_row, inc, inc_row = t.rhs_ranging(rows)
    assert np.isinf(inc).all() and (inc_row == -1).all()
    assert np.array_equal(dec, lp["b"]) and np.array_equal(dec_row, rows)
    for r in (0, m - 1):
        assert t.select_dual_pivot_column(r) is None
    t.close()


def a_minimiser_column():
    """A structural column below 290 that is non-basic at the optimum of (40, 300, 4) and the minimiser of the most (row, direction)
    pairs there, from the reference at the engine's optimal basis."""
    m, n, seed = 40, 300, 4
    _, t = solved(m, n, seed)
    _, _, _, in_basis, ratios, _ = reference_of(t, (m, n, seed))
    t.close()
    counts = np.bincount([pick.index for pair in ratios for pick in pair if 0 <= pick.index < 290], minlength=290)
    source = int(np.argmax(counts))
    assert counts[source] > 0 and not in_basis[source]
    return source


@pytest.mark.parametrize("source", [3, None])
def test_duplicated_column_ties_go_to_the_lower_index(source):
    """Column 290 is a copy of column `source` (same cost): their tableau columns and reduced costs carry the same bits on the device,
    the two ratios tie exactly, and wherever they are the minimum the lower index is reported.  source 3 is minimiser of no row at
    this optimum (the step-wise call still has to agree on every row); `a_minimiser_column()` is one of several, by construction."""
    m, n, seed = 40, 300, 4
    must_hit = source is None
    if source is None:
        source = a_minimiser_column()
    lp = dense_lp(m, n, seed)
    A, c = lp["A"].copy(), lp["c"].copy()
    A[:, 290], c[290] = A[:, source], c[source]
    md = MatrixData.from_dense_le(A, lp["b"].copy(), c)
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, poll_interval=1)
    assert t.solve_relaxation() == engine.OPTIMAL
    basis = [int(j) for j in t.basis_indices()]
    T, _, d, in_basis = rr.tableau(md, basis)
    ratios = rr.row_ratios(T, d, in_basis, range(m))
    down, down_col, up, up_col = t.row_ratios(np.arange(m))
    both_free = not in_basis[source] and not in_basis[290]
    hits = 0
    for r in range(m):
        stepwise = t.select_dual_pivot_column(r)
        assert down_col[r] == (-1 if stepwise is None else stepwise)
        for pick, got in ((ratios[r][0], down_col[r]), (ratios[r][1], up_col[r])):
            if both_free and pick.index in (source, 290):
                assert pick.band == 2 and got == source
                hits += 1
    print(f"columns {source} and 290 both non-basic: {both_free}; minimiser of {hits} (row, direction) pairs")
    assert hits > 0 or not must_hit
    t.close()


def finite_moves(ranging):
    """[(k, sign, pick)] of every (row, direction) with a finite bound: sign -1 = decrease."""
    return [(k, sign, pick) for k, pair in enumerate(ranging) for sign, pick in zip((-1.0, 1.0), pair) if pick.index >= 0]


def past_the_bound(pick):
    """The midpoint of the first and the second blocking ratio; a direction that a single row bounds (a basic slack's own row: its
    column of B^-1 is a unit vector) has its second blocking ratio at infinity, and 1.5 x the bound is past the first alone too."""
    return 0.5 * (pick.ratio + pick.runner_up) if np.isfinite(pick.runner_up) else 1.5 * pick.ratio


@pytest.mark.parametrize("m,n,seed", LPS)
def test_a_move_past_the_bound_makes_the_reported_row_the_dual_pivot(m, n, seed):
    lp, t = solved(m, n, seed, update_block=-1)
    key = (m, n, seed)
    basis = t.basis_indices()
    T, b_ref, _, _, _, ranging = reference_of(t, key)
    moves = finite_moves(ranging)
    assert len(moves) == FINITE_MOVES[key]
    for k, sign, pick in moves:                                # on the CPU: every move leaves the blocking row alone infeasible
        assert pick.ratio > 0
        after = b_ref + sign * past_the_bound(pick) * T[:, n + k]
        assert np.flatnonzero(after < -10 * TOL_FEAS).tolist() == [pick.index]
    if len(moves) > 60:                                        # a fixed sample of 24 for time: up to 8 increases, the rest decreases spread over the rows
        increases = [mv for mv in moves if mv[1] > 0][:8]
        decreases = [mv for mv in moves if mv[1] < 0]
        spread = np.linspace(0, len(decreases) - 1, 24 - len(increases)).astype(int)
        moves = increases + [decreases[i] for i in spread]
        assert len(moves) == 24
    rows = np.arange(m)
    down, down_col, _, _ = t.row_ratios(rows)
    dec, dec_row, inc, inc_row = t.rhs_ranging(rows)
    optimum = t.objective_function_value()
    for k, sign, pick in moves:
        bound, blocking = (dec[k], dec_row[k]) if sign < 0 else (inc[k], inc_row[k])
        assert blocking == pick.index
        # half way to the bound: still optimal
        t.change_right_hand_side([k], [lp["b"][k] + sign * 0.5 * bound])
        assert t.run_dual(1 << 20) == (0, engine.OPTIMAL)
        # past it: the blocking row leaves, the column reported for it enters, the objective moves by ratio * |b_r|
        t.change_right_hand_side([k], [lp["b"][k] + sign * past_the_bound(pick)])
        b_moved, before = t.b(), t.objective_function_value()
        assert int(np.argmin(b_moved)) == blocking and b_moved[blocking] < -TOL_FEAS
        done, _ = t.run_dual(1)
        assert done == 1
        q, r, _ = dual_trace(t)[-1]
        assert (r, q) == (blocking, down_col[blocking])
        step = t.objective_function_value() - before
        assert close_to(step, down[blocking] * abs(b_moved[blocking]))
        # back to the optimal basis of the original rhs
        t.change_right_hand_side([k], [lp["b"][k]])
        t.from_basis(basis)
        assert close_to(t.objective_function_value(), optimum)
    t.close()


def snapshot(t):
    return (t.b().tobytes(), t.relative_costs().tobytes(), t.basis_indices().tobytes(), t.objective_function_value(), len(t.trace()),
            t.reinversions(), t.flush_stats())


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", [(40, 300, 4), (300, 40, 5)])
def test_the_queries_change_nothing(m, n, seed, update_block):
    lp, t = solved(m, n, seed, update_block=update_block)
    _, twin = solved(m, n, seed, update_block=update_block)
    before = snapshot(t)
    assert before == snapshot(twin)
    rows = np.arange(m)
    first = t.row_ratios(rows) + t.rhs_ranging(rows)
    assert snapshot(t) == before
    again = t.row_ratios(rows) + t.rhs_ranging(rows)          # the same call on the same state: the same bits
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    assert snapshot(t) == before
    assert pending_rows(t) == t.ranging_stats()[3]
    # the handle that was queried and the one that was not walk the same dual pivots to the same b
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    for handle in (t, twin):
        handle.change_right_hand_side(np.arange(0, m, 3), b2[::3])
    result = t.run_dual(1 << 20)
    assert result[1] == engine.OPTIMAL and result == twin.run_dual(1 << 20)
    assert t.trace() == twin.trace() and t.b().tobytes() == twin.b().tobytes()
    assert t.run(1 << 20) == (0, engine.OPTIMAL)
    t.close()
    twin.close()


def test_cost_ranging_of_structural_columns():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed)
    basis, d = t.basis_indices().tolist(), t.relative_costs()
    down, _, up, _ = t.row_ratios(np.arange(m))
    dec, inc = t.cost_ranging(np.arange(n))
    assert any(j in basis for j in range(n)) and any(j not in basis for j in range(n))
    for j in range(n):
        if j in basis:
            assert (dec[j], inc[j]) == (down[basis.index(j)], up[basis.index(j)])
        else:
            assert (dec[j], inc[j]) == (d[j], np.inf)
    t.close()


def raw_query(lib, name, t, rows, count, fill=-7.0):
    ratio0, ratio1 = np.full(4, fill), np.full(4, fill)
    index0, index1 = np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
    r = np.array(rows, dtype=np.int32)
    st = getattr(lib, name)(t.handle, r.ctypes.data, count, ratio0.ctypes.data, index0.ctypes.data, ratio1.ctypes.data,
                            index1.ctypes.data)
    untouched = (ratio0 == fill).all() and (ratio1 == fill).all() and (index0 == -7).all() and (index1 == -7).all()
    return st, untouched


def test_argument_errors_write_nothing():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed)
    lib = engine.load_library()
    before = snapshot(t)
    for name in ("relp_row_ratios", "relp_rhs_ranging"):
        for rows, count in (([0, m], 2), ([-1], 1), ([0, 1, 2, m + 5], 4), ([0], -1)):
            assert raw_query(lib, name, t, rows, count) == (E_ARG, True)
        assert raw_query(lib, name, t, [0], 0) == (0, True)                        # count == 0: a no-op
        assert getattr(lib, name)(t.handle, None, 0, None, None, None, None) == 0
        three = np.array([5, 0, 5], dtype=np.int32)
        assert getattr(lib, name)(t.handle, three.ctypes.data, 3, None, None, None, None) == 0     # NULL outputs are accepted
    with pytest.raises(engine.RelpError) as err:
        t.row_ratios([m])
    assert status_of(err) == E_ARG
    assert t.ranging_stats() == (1, 3, 1, pending_rows(t)) and snapshot(t) == before
    ratio_only = np.zeros(3)
    assert lib.relp_row_ratios(t.handle, three.ctypes.data, 3, ratio_only.ctypes.data, None, None, None) == 0
    assert ratio_only[0] == ratio_only[2] == t.row_ratios([5])[0][0]
    t.close()


def test_refused_in_phase_one():
    md, _ = dr.covering_lp(24, 32, 1)
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (lambda: t.row_ratios([0]), lambda: t.rhs_ranging([0]), t.ranging_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    assert t.solve_relaxation() == engine.OPTIMAL
    assert t.ranging_stats() == (0, 0, 0, 0)
    t.close()


@pytest.mark.parametrize("kind", [engine.ENGINE_REVISED, engine.ENGINE_LU])
def test_refused_on_the_other_engines(kind):
    lp = dense_lp(24, 32, 1)
    t = engine.Tableau(le_lp(lp, lp["b"]), engine=kind)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    objective = t.objective_function_value()
    for call in (lambda: t.row_ratios([0]), lambda: t.rhs_ranging([0]), t.ranging_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_UNSUPPORTED
    assert t.run(1 << 20) == (0, engine.OPTIMAL) and t.objective_function_value() == objective
    t.close()
