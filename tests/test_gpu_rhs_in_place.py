"""relp_change_right_hand_side / relp_set_upper_bound / relp_get_right_hand_side / relp_rhs_stats of the tableau engine: rhs entries
moved on the current basis without a re-tabulation, through the ctypes binding, against relp_set_right_hand_side (the full rebuild),
a dense solve of B x = rhs, the test reference tests/dual_reference.py (same rules as relp_run_dual, numpy f64, started from the
engine's own basis at test time) and the committed f64 oracle's fresh two-phase optimum.

LPs: `MatrixData.from_dense_le(**synthetic.dense_lp(m, n, seed))` at (24, 32, 1), (40, 300, 4: more than 256 stored columns), (300, 40,
5: more than 256 rows) and (257, 8, 2: the second block of 256 rows holds one row, and a change of every row spans two LDS chunks of
the list), with update_block 3 (flushes every third pivot) and -1 (64: the block stays open, the change reads T0 + W R0).  No tie band
of the reference ever holds two entries on these inputs (`max_band == 1` is asserted), so the device must walk the reference's
pivots one for one.  Tolerances: the project's 1e-9 relative on objectives (OBJ_RTOL), tol_feas = 1e-7 on b, and 1e-9 * max(1, max|b|)
between the b of the in-place change, of the rebuild and of the dense solve.

The pending rows p that relp_rhs_stats reports are the DISTINCT pivot rows since the last flush (PivotRecord::n_eta), computed here
from the engine's trace: with update_block 3 that is 0 / 1 / 1 after 18 / 49 / 43 primal pivots, with 64 it is the number of
distinct rows among all of them (at most the pivot count; 49 pivots on 40 rows cannot all be distinct).  The host counts the
iterations it ENQUEUES towards the next flush, and a loop that polls every 64 iterations (the default) enqueues no-op iterations past
the optimum up to its next poll, so it leaves with the block just flushed; the handles of `solved()` poll after every iteration
(poll_interval = 1: one no-op iteration, the one that finds no candidate), which is what leaves the block open here."""
import functools
import math
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic
from oracle import relp_f64

import dual_reference as dr

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-9
TOL_FEAS = 1e-7
E_ARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
PRIMAL_PIVOTS = {(24, 32, 1): 18, (40, 300, 4): 49, (300, 40, 5): 43, (257, 8, 2): 8}
# dual pivots of the four chained changes, and the optima where they are pinned
CHAIN_PIVOTS = {(24, 32, 1): [16, 5, 8, 5], (40, 300, 4): [32, 12, 23, 36], (300, 40, 5): [105, 20, 71, 37]}
CHAIN_OBJECTIVES = {(24, 32, 1): [-24.711272676, -22.164031227, -17.147584449, -21.040055671]}


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    """A, b, c of the dense <= LP (computed once, read only: every test copies what it changes)."""
    lp = synthetic.dense_lp(m, n, seed)
    for v in lp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lp


def le_lp(lp, b):
    return MatrixData.from_dense_le(lp["A"], np.array(b, dtype=np.float64), lp["c"])


@functools.lru_cache(maxsize=None)
def oracle_optimum(m, n, seed, b_bytes):
    oracle = relp_f64.OracleF64(le_lp(dense_lp(m, n, seed), np.frombuffer(b_bytes)).ensure_csc())
    assert oracle.run() == "optimal"
    return oracle.objective


def status_of(err):
    return int(re.search(r"\((-?\d+)\)", str(err.value)).group(1))


def dual_trace(t, skip=0):
    rows = t.trace()[skip:]
    assert all(phase == 2 for phase, _, _, _ in rows)
    return [(q, r, leaving) for _, q, r, leaving in rows]


def close_to(value, expected):
    return abs(value - expected) <= OBJ_RTOL * max(1.0, abs(expected))


def solved(m, n, seed, **config):
    lp = dense_lp(m, n, seed)
    t = engine.Tableau(le_lp(lp, lp["b"]), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    assert t.iterations() == PRIMAL_PIVOTS[(m, n, seed)]
    return lp, t


def pending_rows(t):
    """The distinct pivot rows since the last flush, from the trace of a handle of `solved()` that has only run its primal solve: a
    flush follows every update_block-th enqueued iteration, and the one no-op iteration after the last pivot completes no block
    here (18, 49 and 43 pivots are 0, 1 and 1 past a multiple of 3, 8 and all of them are below 63)."""
    rows = [r for _, _, r, _ in t.trace()]
    tail = len(rows) % t.update_block()
    assert tail + 1 < t.update_block()
    return len(set(rows[len(rows) - tail:]))


def b_bound(b):
    return 1e-9 * max(1.0, float(np.abs(b).max()))


def dense_b(lp, rhs, basis):
    full, _, _ = dr.standard_form(le_lp(lp, rhs))
    return np.linalg.solve(full[:, basis], rhs)


def check_equal_to_a_rebuild(m, n, seed, negative_rows, update_block, flush):
    lp, a = solved(m, n, seed, update_block=update_block)
    _, rebuilt = solved(m, n, seed, update_block=update_block)
    assert a.update_block() == (3 if update_block == 3 else 64)
    p = pending_rows(a)
    if update_block == 3:
        assert p == PRIMAL_PIVOTS[(m, n, seed)] % 3 == {(24, 32, 1): 0, (40, 300, 4): 1, (300, 40, 5): 1}[(m, n, seed)]
    else:
        assert 1 <= p <= PRIMAL_PIVOTS[(m, n, seed)]           # no flush has happened: every pivot row is pending
    if flush:
        a.flush()
        p = 0
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    rows = np.arange(0, m, 3)
    basis, d_before, reinversions = a.basis_indices(), a.relative_costs(), a.reinversions()
    assert a.rhs_stats() == (0, 0, 0, 0)
    assert np.array_equal(a.right_hand_side(), lp["b"])
    a.change_right_hand_side(rows, b2[::3])
    rebuilt.set_right_hand_side(b2)
    assert a.rhs_stats() == (1, len(rows), p, 1)
    assert a.basis_indices().tolist() == rebuilt.basis_indices().tolist() == basis.tolist()
    b_a, b_r = a.b(), rebuilt.b()
    print(f"max|b_A - b_B| = {np.abs(b_a - b_r).max():.3e}, against the dense solve {np.abs(b_a - dense_b(lp, b2, basis)).max():.3e}, "
          f"bound {b_bound(b_r):.3e}, p = {p}")
    assert np.abs(b_a - b_r).max() <= b_bound(b_r)
    assert np.abs(b_a - dense_b(lp, b2, basis)).max() <= b_bound(b_r)
    assert close_to(a.objective_function_value(), rebuilt.objective_function_value())
    assert a.relative_costs().tobytes() == d_before.tobytes()
    assert a.reinversions() == reinversions
    assert np.array_equal(a.right_hand_side(), b2)
    assert int((b_a < -TOL_FEAS).sum()) == negative_rows
    a.close()
    rebuilt.close()


SHAPES = [(24, 32, 1, 10), (40, 300, 4, 17), (300, 40, 5, 70)]


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed,negative_rows", SHAPES)
def test_equal_to_a_rebuild(m, n, seed, negative_rows, update_block):
    check_equal_to_a_rebuild(m, n, seed, negative_rows, update_block, flush=False)


@pytest.mark.parametrize("m,n,seed,negative_rows", SHAPES)
def test_equal_to_a_rebuild_after_a_flush(m, n, seed, negative_rows):
    check_equal_to_a_rebuild(m, n, seed, negative_rows, -1, flush=True)


def chain_steps(m):
    """(rows, factor) of the four changes; each factor multiplies the rhs current at that point."""
    return [(np.arange(0, m, 3), 0.5), (np.array([1]), 0.25), (np.arange(2, m, 5), 0.5), (np.arange(0, m, 3), 2.0)]


def walk_the_chain(m, n, seed, t, lp):
    b = lp["b"].copy()
    key = (m, n, seed)
    for step, (rows, factor) in enumerate(chain_steps(m)):
        b[rows] *= factor
        basis_before, done_before = t.basis_indices(), t.iterations()
        ref = dr.dual_simplex(le_lp(lp, b), basis_before)
        assert ref.outcome == "optimal" and ref.max_band == 1 and len(ref.trace) == CHAIN_PIVOTS[key][step]
        optimum = oracle_optimum(m, n, seed, b.tobytes())
        if key in CHAIN_OBJECTIVES:
            assert abs(optimum - CHAIN_OBJECTIVES[key][step]) <= 1e-8
        t.change_right_hand_side(rows, b[rows])
        assert np.array_equal(t.right_hand_side(), b)
        assert t.run_dual(1 << 20) == (len(ref.trace), engine.OPTIMAL)
        assert dual_trace(t, skip=done_before) == ref.trace
        print(f"step {step}: objective {t.objective_function_value():.12f}, oracle {optimum:.12f}")
        assert close_to(t.objective_function_value(), optimum)
        assert t.check_basis()[2] >= -TOL_FEAS
        assert t.run(1 << 20) == (0, engine.OPTIMAL)
    assert t.rhs_stats()[0] == 4


@pytest.mark.parametrize("m,n,seed,update_block", [(24, 32, 1, -1), (24, 32, 1, 3), (40, 300, 4, -1), (300, 40, 5, -1)])
def test_chained_resolves_walk_the_reference_pivots(m, n, seed, update_block):
    lp, t = solved(m, n, seed, update_block=update_block)
    walk_the_chain(m, n, seed, t, lp)
    assert t.reinversions() == 0
    t.close()


@pytest.mark.parametrize("forced", [3, None])
def test_every_row_at_once_over_the_split_path(forced, monkeypatch):
    """257 rows, all of them changed: the list spans two LDS chunks; RELP_TAB_RHS_SPLITS=3 cuts it into 86 / 86 / 85 entries with
    partial sums and the reduction kernel, and the second block of 256 rows holds row 256 alone."""
    if forced:
        monkeypatch.setenv("RELP_TAB_RHS_SPLITS", str(forced))
    else:
        monkeypatch.delenv("RELP_TAB_RHS_SPLITS", raising=False)
    m, n, seed = 257, 8, 2
    lp, t = solved(m, n, seed)
    _, rebuilt = solved(m, n, seed)
    b2 = lp["b"] * (0.5 + (np.arange(m) % 7) / 7)
    assert (b2 != lp["b"]).all()
    basis, done_before = t.basis_indices(), t.iterations()
    ref = dr.dual_simplex(le_lp(lp, b2), basis)
    assert ref.outcome == "optimal" and ref.max_band == 1 and len(ref.trace) == 10
    optimum = oracle_optimum(m, n, seed, b2.tobytes())
    assert abs(optimum - -2.8122547088) <= 1e-9
    p = pending_rows(t)
    assert 1 <= p <= 8
    t.change_right_hand_side(np.arange(m), b2)
    rebuilt.set_right_hand_side(b2)
    stats = t.rhs_stats()
    assert stats[:3] == (1, m, p)
    assert stats[3] == 3 if forced else stats[3] >= 1
    b_t, b_r = t.b(), rebuilt.b()
    print(f"splits {stats[3]}: max|b_A - b_B| = {np.abs(b_t - b_r).max():.3e}, bound {b_bound(b_r):.3e}")
    assert np.abs(b_t - b_r).max() <= b_bound(b_r)
    assert np.abs(b_t - dense_b(lp, b2, basis)).max() <= b_bound(b_r)
    assert t.run_dual(1 << 20) == (10, engine.OPTIMAL)
    assert dual_trace(t, skip=done_before) == ref.trace
    assert close_to(t.objective_function_value(), optimum)
    t.close()
    rebuilt.close()


@functools.lru_cache(maxsize=None)
def bounded_case():
    """(24, 32, 1) with upper bounds 4 * max(1, ceil(max x*)) on every second structural column, x* the optimum without bounds:
    16 bound rows, 40 rows and 72 columns in all."""
    m, n, seed = 24, 32, 1
    lp = dense_lp(m, n, seed)
    oracle = relp_f64.OracleF64(le_lp(lp, lp["b"]).ensure_csc())
    assert oracle.run() == "optimal"
    x_max = max(v for j, v in zip(oracle.basis(), oracle.b()) if j < n)
    ub = np.full(n, np.inf)
    ub[::2] = 4.0 * max(1.0, math.ceil(x_max))
    ub.setflags(write=False)
    return lp, ub


def bounded_md(lp, ub):
    m, n = lp["A"].shape
    return MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=lp["b"].copy(), cost=lp["c"].copy(),
                      upper_bound=np.array(ub), dense=np.asfortranarray(lp["A"]))


def explicit_bounds_md(lp, ub):
    """The same LP with the bounds as <= rows appended after A: rows and columns coincide with the engine's (bound rows follow the
    constraints and bound slacks follow the <= slacks, both in column order)."""
    bounded = np.flatnonzero(np.isfinite(ub))
    unit = np.zeros((len(bounded), lp["A"].shape[1]))
    unit[np.arange(len(bounded)), bounded] = 1.0
    return MatrixData.from_dense_le(np.vstack([lp["A"], unit]), np.concatenate([lp["b"], ub[bounded]]), lp["c"])


def bounded_optimum(lp, ub):
    oracle = relp_f64.OracleF64(bounded_md(lp, ub).ensure_csc())
    assert oracle.run() == "optimal"
    return oracle.objective


def test_upper_bounds_branch_and_bound_style():
    lp, ub0 = bounded_case()
    m, n = lp["A"].shape
    ub = np.array(ub0)
    t = engine.Tableau(bounded_md(lp, ub), engine=engine.ENGINE_TABLEAU, trace_capacity=4096)
    assert t.solve_relaxation() == engine.OPTIMAL
    assert (t.nr_rows(), t.nr_columns()) == (40, 72)
    assert abs(bounded_optimum(lp, ub) - -36.595873601) <= 1e-8 and close_to(t.objective_function_value(), bounded_optimum(lp, ub))
    expected = [(20, 1.0, 1, -36.508420869), (22, 1.0, 3, -36.262669135), (20, 0.0, 1, -36.113006086), (30, 7.0, 1, -36.067483642)]
    for column, bound, pivots, objective in expected:
        basis, values, done_before, read_before = t.basis_indices(), t.b(), t.iterations(), t.rhs_stats()[1]
        x = np.zeros(n)
        for j, v in zip(basis, values):
            if j < n:
                x[j] = v
        fractional = [j for j in np.flatnonzero(np.isfinite(ub)) if abs(x[j] - round(x[j])) > 1e-6]
        assert fractional[0] == column and math.floor(x[column]) == bound
        ub[column] = bound
        ref = dr.dual_simplex(explicit_bounds_md(lp, ub), basis)
        assert ref.outcome == "optimal" and ref.max_band == 1 and len(ref.trace) == pivots
        optimum = bounded_optimum(lp, ub)
        assert abs(optimum - objective) <= 1e-8
        t.set_upper_bound(column, bound)
        assert t.rhs_stats()[1] == read_before + 1
        assert t.right_hand_side()[m:].tolist() == ub[np.isfinite(ub)].tolist()
        assert t.run_dual(1 << 20) == (pivots, engine.OPTIMAL)
        assert dual_trace(t, skip=done_before) == ref.trace
        assert close_to(t.objective_function_value(), optimum)
    assert t.reinversions() == 0
    t.close()


def infeasible_after_the_change():
    """x1 + x2 <= 2, x1 + x2 >= 1, c = (1, 1): optimum 1 on the basis [2, 0]."""
    return MatrixData(nr_normal=2, nr_eq=0, nr_range=0, nr_le=1, nr_ge=1, b=np.array([2.0, 1.0]), cost=np.array([1.0, 1.0]),
                      upper_bound=np.full(2, np.inf), dense=np.asfortranarray(np.ones((2, 2))))


def test_a_change_that_makes_the_lp_infeasible():
    t = engine.Tableau(infeasible_after_the_change(), engine=engine.ENGINE_TABLEAU, trace_capacity=64)
    assert t.solve_relaxation() == engine.OPTIMAL
    assert t.objective_function_value() == 1.0 and t.basis_indices().tolist() == [2, 0]
    t.change_right_hand_side([1], [4.0])
    assert t.run_dual(1 << 20) == (0, engine.INFEASIBLE)
    t.change_right_hand_side([1], [1.0])
    assert t.run_dual(1 << 20) == (0, engine.OPTIMAL)
    assert t.objective_function_value() == 1.0
    assert t.right_hand_side().tolist() == [2.0, 1.0]
    t.close()


def test_a_later_warm_start_sees_the_new_rhs():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed)
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    t.change_right_hand_side(np.arange(0, m, 3), b2[::3])
    assert t.run_dual(1 << 20) == (16, engine.OPTIMAL)
    basis, b_before, objective = t.basis_indices(), t.b(), t.objective_function_value()
    t.from_basis(basis)
    assert t.reinversions() == 1 and np.array_equal(t.right_hand_side(), b2)
    assert np.abs(t.b() - b_before).max() <= b_bound(b_before)
    assert np.abs(t.b() - dense_b(lp, b2, basis)).max() <= b_bound(b_before)
    assert close_to(t.objective_function_value(), objective)
    assert t.run(1 << 20) == (0, engine.OPTIMAL)
    t.close()


def test_the_reinversion_interval_rebuilds_on_the_new_rhs():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed)
    t.set_reinversion_interval(4)
    walk_the_chain(m, n, seed, t, lp)
    assert t.reinversions() >= 4                               # 16, 5, 8, 5 dual pivots, a rebuild every fourth
    t.close()


def test_refused_in_phase_one():
    md, _ = dr.covering_lp(24, 32, 1)
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (lambda: t.change_right_hand_side([0], [1.0]), lambda: t.set_upper_bound(0, 1.0), t.right_hand_side, t.rhs_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    assert t.solve_relaxation() == engine.OPTIMAL
    assert t.rhs_stats() == (0, 0, 0, 0)
    t.close()


@pytest.mark.parametrize("kind", [engine.ENGINE_REVISED, engine.ENGINE_LU])
def test_refused_on_the_other_engines(kind):
    lp = dense_lp(24, 32, 1)
    t = engine.Tableau(le_lp(lp, lp["b"]), engine=kind)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    objective = t.objective_function_value()
    for call in (lambda: t.change_right_hand_side([0], [1.0]), lambda: t.set_upper_bound(0, 1.0), t.right_hand_side, t.rhs_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_UNSUPPORTED
    assert t.run(1 << 20) == (0, engine.OPTIMAL) and t.objective_function_value() == objective
    t.close()


def test_argument_errors_change_nothing():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed)
    before = (t.b(), t.right_hand_side(), t.rhs_stats(), t.objective_function_value())

    def unchanged():
        return (np.array_equal(t.b(), before[0]) and np.array_equal(t.right_hand_side(), before[1]) and t.rhs_stats() == before[2]
                and t.objective_function_value() == before[3])

    for rows, values in (([0, m], [1.0, 1.0]), ([-1], [1.0]), ([3, 5, 3], [1.0, 2.0, 3.0]), ([0, 1], [1.0, float("nan")]),
                         ([2], [float("inf")])):
        with pytest.raises(engine.RelpError) as err:
            t.change_right_hand_side(rows, values)
        assert status_of(err) == E_ARG and unchanged()
    assert engine.load_library().relp_change_right_hand_side(t.handle, None, None, -1) == E_ARG and unchanged()
    t.change_right_hand_side([], [])                          # count == 0: a no-op
    t.change_right_hand_side([4, 7], lp["b"][[4, 7]])         # no entry moves: nothing is read, nothing is launched
    assert np.array_equal(t.b(), before[0]) and t.rhs_stats() == (1, 0, pending_rows(t), 0)
    # the handle solves on
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    t.change_right_hand_side(np.arange(0, m, 3), b2[::3])
    assert t.run_dual(1 << 20) == (16, engine.OPTIMAL)
    assert close_to(t.objective_function_value(), oracle_optimum(m, n, seed, b2.tobytes()))
    t.close()


def test_upper_bound_argument_errors():
    lp, ub0 = bounded_case()
    n = lp["A"].shape[1]
    t = engine.Tableau(bounded_md(lp, ub0), engine=engine.ENGINE_TABLEAU, trace_capacity=4096)
    assert t.solve_relaxation() == engine.OPTIMAL
    before = (t.b(), t.right_hand_side(), t.rhs_stats())
    for column, value in ((1, 1.0), (n, 1.0), (-1, 1.0), (0, float("inf")), (0, float("nan"))):
        with pytest.raises(engine.RelpError) as err:
            t.set_upper_bound(column, value)
        assert status_of(err) == E_ARG
        assert np.array_equal(t.b(), before[0]) and np.array_equal(t.right_hand_side(), before[1]) and t.rhs_stats() == before[2]
    ub = np.array(ub0)
    ub[20] = 1.0
    t.set_upper_bound(20, 1.0)
    assert t.run_dual(1 << 20) == (1, engine.OPTIMAL)
    assert close_to(t.objective_function_value(), bounded_optimum(lp, ub))
    t.set_upper_bound(20, -1.0)                                # below 0 is accepted: x_20 >= 0 makes the LP infeasible
    assert t.run_dual(1 << 20)[1] == engine.INFEASIBLE
    t.close()
