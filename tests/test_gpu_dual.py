"""The dual simplex loop of the tableau engine (relp_run_dual), its two step-wise selectors and relp_set_right_hand_side, through
the ctypes binding, against the test reference tests/dual_reference.py (same rules, numpy f64) and the committed f64 oracle.

Covering LPs `min c'x, A x >= b, c > 0` (dual_reference.covering_lp) start from the all-surplus basis, which is dual feasible at
once.  No tie band of these inputs ever holds two entries (tests/test_dual_reference.py asserts it), so the device must walk the
reference's pivots one for one; one case is built to tie exactly -- two rows of different 256-row blocks share the minimum b_i, the
smaller leaving column in the later row -- and the infeasible LP ties two ratios.  Shapes: one block of rows and columns; more than 256 stored columns (40 x 300: 340 of them, two
workgroups of partials, the second one partial); more than 256 rows (257 x 8: the second block of minima holds one row; 300 x
40); update_block 3 on 32 x 48 (21 pivots on 13 distinct rows: rows return to occupied slots of W and the block flushes seven
times).  Two more cases tie on purpose, to overflow the lists the pickers keep of the blocks / slots inside a tie band: 16,385 rows
that all share b_i = -1 (65 blocks against a list of 64) and 8,400 columns at ratio 1 (33 slots against a list of 32).  Tolerances: the project's own 1e-9 relative on objectives (OBJ_RTOL) and tol_feas = 1e-7 on b.
"""
import functools
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
TOL = dr.TOLERANCES
E_STATE, E_UNSUPPORTED = -5, -6


@functools.lru_cache(maxsize=None)
def covering(m, n, seed):
    """The LP, the reference's dual solve from the surplus basis and the oracle's two-phase optimum (computed once, read only)."""
    md, _ = dr.covering_lp(m, n, seed)
    ref = dr.dual_simplex(md, dr.surplus_basis(m, n))
    assert ref.outcome == "optimal"
    oracle = relp_f64.OracleF64(md.ensure_csc())
    assert oracle.run() == "optimal"
    return {"md": md, "trace": ref.trace, "objective": oracle.objective}


def status_of(err):
    return int(re.search(r"\((-?\d+)\)", str(err.value)).group(1))


def dual_trace(t, skip=0):
    rows = t.trace()[skip:]
    assert all(phase == 2 for phase, _, _, _ in rows)
    return [(q, r, leaving) for _, q, r, leaving in rows]


def close_to(value, expected):
    return abs(value - expected) <= OBJ_RTOL * max(1.0, abs(expected))


def warm_started(m, n, seed, **config):
    case = covering(m, n, seed)
    t = engine.Tableau(case["md"], engine=engine.ENGINE_TABLEAU, trace_capacity=4096, **config)
    t.from_basis(dr.surplus_basis(m, n))
    assert t.phase == 2 and t.b().max() < 0
    return case, t


def assert_dual_solve(case, t):
    done, outcome = t.run_dual(1 << 20)
    assert outcome == engine.OPTIMAL and done == len(case["trace"])
    assert dual_trace(t) == case["trace"]
    assert close_to(t.objective_function_value(), case["objective"])


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", [(8, 8, 1), (24, 32, 1), (32, 48, 3)])
def test_loop_walks_the_reference_pivots(m, n, seed, update_block):
    case, t = warm_started(m, n, seed, update_block=update_block)
    assert t.update_block() == (3 if update_block == 3 else 64)
    assert_dual_solve(case, t)
    assert t.check_basis()[2] >= -TOL_FEAS
    assert t.run(1 << 20) == (0, engine.OPTIMAL)           # the primal loop agrees: nothing left to price
    t.close()


def test_more_than_one_block_of_columns():
    case, t = warm_started(40, 300, 4)
    assert t.nr_columns() == 340
    assert_dual_solve(case, t)
    t.close()


@pytest.mark.parametrize("m,n,seed", [(257, 8, 2), (300, 40, 5)])
def test_more_than_one_block_of_rows(m, n, seed):
    case, t = warm_started(m, n, seed)
    assert_dual_solve(case, t)
    t.close()


def test_two_rows_in_the_tie_band_of_different_blocks():
    """Rows 3 and 260 (two blocks of 256 rows) share the most negative b_i exactly; the surplus columns of the two rows are
    exchanged in the basis, so the smaller leaving column sits in row 260: Bland on the leaving column, not the first row."""
    m, n = 300, 40
    md, _ = dr.covering_lp(m, n, 5)
    md.b = md.b.copy()
    md.b[3] = md.b[260] = md.b.max() + 1.0
    basis = dr.surplus_basis(m, n)
    basis[3], basis[260] = basis[260], basis[3]
    ref = dr.dual_simplex(md, basis)
    assert ref.outcome == "optimal" and ref.max_band == 2 and ref.trace[0][1:] == (260, n + 3)
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096)
    t.from_basis(basis)
    assert t.b()[3] == t.b()[260] == t.b().min()
    assert t.select_dual_pivot_row() == 260
    assert t.run_dual(1 << 20) == (len(ref.trace), engine.OPTIMAL)
    assert dual_trace(t) == ref.trace
    assert close_to(t.objective_function_value(), ref.objective)
    t.close()


def test_step_calls_follow_the_rules_on_the_device_state():
    m, n, seed = 24, 32, 1
    case, t = warm_started(m, n, seed)
    full, _, _ = dr.standard_form(case["md"])
    steps = []
    for _ in range(len(case["trace"]) + 1):
        b, basis = t.b(), t.basis_indices()
        row = t.select_dual_pivot_row()
        assert row == dr.select_dual_pivot_row(b, basis, TOL["tol_feas"], TOL["tol_tie"])
        if row is None:
            break
        d = t.relative_costs()
        in_basis = np.zeros(n + m, dtype=bool)
        in_basis[basis] = True
        column = t.select_dual_pivot_column(row)
        assert column is not None
        assert column == dr.select_dual_pivot_column(d, t.basis_inverse_row(row) @ full, in_basis, TOL["tol_pivot"], TOL["tol_zero"],
                                                     TOL["tol_tie"])
        alpha = t.generate_column(column)
        assert alpha[row] < -TOL["tol_pivot"]
        leaving = t.bring_into_basis(column, row, d[column])
        assert leaving == basis[row]
        steps.append((column, row, leaving))
    assert steps == case["trace"]
    assert dual_trace(t) == case["trace"]
    assert close_to(t.objective_function_value(), case["objective"])
    t.close()


def test_infeasible_lp_and_the_ratio_tie():
    """x1 + x2 <= 2, x1 + x2 >= 4 from the slack basis [2, 3]: row 1 leaves, columns 0 and 1 tie at ratio 1 and the lower one
    enters; then row 0 (b = -2) has no negative entry."""
    t = engine.Tableau(dr.infeasible_pair(), engine=engine.ENGINE_TABLEAU, trace_capacity=16)
    t.from_basis(np.array([2, 3], dtype=np.int32))
    assert t.run_dual(1 << 20) == (1, engine.INFEASIBLE)
    assert dual_trace(t) == [(0, 1, 3)]
    t.close()


@pytest.mark.parametrize("m,n,seed,negative_rows,pivots,objective", [(24, 32, 1, 10, 16, -24.71127268), (40, 300, 4, 17, 32, -258.8750536)])
def test_resolve_after_a_change_of_the_right_hand_side(m, n, seed, negative_rows, pivots, objective):
    lp = synthetic.dense_lp(m, n, seed)
    t = engine.Tableau(MatrixData.from_dense_le(lp["A"], lp["b"], lp["c"]), engine=engine.ENGINE_TABLEAU, trace_capacity=4096)
    assert t.solve_relaxation() == engine.OPTIMAL
    primal_pivots, basis = t.iterations(), t.basis_indices()
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    changed = MatrixData.from_dense_le(lp["A"], b2, lp["c"])
    ref = dr.dual_simplex(changed, basis)
    assert ref.outcome == "optimal" and len(ref.trace) == pivots
    oracle = relp_f64.OracleF64(changed.ensure_csc())
    assert oracle.run() == "optimal" and abs(oracle.objective - objective) <= 1e-7
    t.set_right_hand_side(b2)
    assert t.basis_indices().tolist() == basis.tolist()
    assert t.b().min() < 0 and int((t.b() < -TOL_FEAS).sum()) == negative_rows
    assert t.run_dual(1 << 20) == (pivots, engine.OPTIMAL)
    assert dual_trace(t, skip=primal_pivots) == ref.trace
    assert close_to(t.objective_function_value(), oracle.objective)
    assert t.check_basis()[2] >= -TOL_FEAS
    t.close()


def test_refused_in_phase_one():
    case = covering(24, 32, 1)
    t = engine.Tableau(case["md"], engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    with pytest.raises(engine.RelpError) as err:
        t.run_dual(10)
    assert status_of(err) == E_STATE
    assert t.solve_relaxation() == engine.OPTIMAL and close_to(t.objective_function_value(), case["objective"])
    t.close()


@pytest.mark.parametrize("kind", [engine.ENGINE_REVISED, engine.ENGINE_LU])
def test_refused_on_the_other_engines(kind):
    case = covering(24, 32, 1)
    t = engine.Tableau(case["md"], engine=kind)
    t.from_basis(dr.surplus_basis(24, 32))
    for call in (lambda: t.run_dual(10), t.select_dual_pivot_row, lambda: t.select_dual_pivot_column(0),
                 lambda: t.set_right_hand_side(np.ones(24))):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_UNSUPPORTED
    t.close()
    t = engine.Tableau(case["md"], engine=kind)
    with pytest.raises(engine.RelpError) as err:
        t.run_dual(10)
    assert status_of(err) == E_UNSUPPORTED
    assert t.solve_relaxation() == engine.OPTIMAL and close_to(t.objective_function_value(), case["objective"])
    t.close()


def test_refused_from_a_basis_that_is_not_dual_feasible():
    """The slack basis of a <= LP with negative costs: d = c < 0."""
    lp = synthetic.dense_lp(24, 32, 1)
    md = MatrixData.from_dense_le(lp["A"], lp["b"], lp["c"])
    oracle = relp_f64.OracleF64(md.ensure_csc())
    assert oracle.run() == "optimal"
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    t.from_basis(np.arange(32, 32 + 24, dtype=np.int32))
    with pytest.raises(engine.RelpError) as err:
        t.run_dual(10)
    assert status_of(err) == E_STATE and "dual feasible" in str(err.value)
    assert t.iterations() == 0
    assert t.run(1 << 20)[1] == engine.OPTIMAL and close_to(t.objective_function_value(), oracle.objective)
    t.close()


def test_reinversion_inside_the_dual_loop():
    case, t = warm_started(32, 48, 3)
    t.set_reinversion_interval(4)
    before = t.reinversions()                              # (the warm start itself re-tabulated once)
    assert_dual_solve(case, t)
    assert t.reinversions() - before >= 1
    assert t.check_basis()[2] >= -TOL_FEAS
    t.close()


def covering_from(A, b):
    m, n = A.shape
    return MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=0, nr_ge=m, b=np.asarray(b, dtype=np.float64), cost=np.ones(n),
                      upper_bound=np.full(n, np.inf), dense=np.asfortranarray(A, dtype=np.float64))


def test_row_pick_with_more_blocks_in_the_tie_band_than_the_list_holds():
    """16,385 rows = 65 blocks of 256, the last one of a single row, every b_i = -1.0 exactly: all 65 block minima are inside the
    tie band, one more than the 64 the block list holds, so the pick walks every block.  The surplus columns of rows 0 and 16,384
    are exchanged in the basis: the smallest leaving column sits in the last block's only row.  The step call picks with 1,024
    threads, the loop's two kernels with 256 in every workgroup.  The tableau of 16,385 x 16,387 doubles (2.1 GB) is what 65
    blocks cost; the reference solve at this size is not computed, only its row pick."""
    m, n = 16385, 2
    md = covering_from(np.ones((m, n)), np.ones(m))
    basis = dr.surplus_basis(m, n)
    basis[0], basis[m - 1] = basis[m - 1], basis[0]
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=16)
    t.from_basis(basis)
    assert t.b().min() == t.b().max() == -1.0
    row = t.select_dual_pivot_row()
    assert row == dr.select_dual_pivot_row(t.b(), t.basis_indices(), TOL["tol_feas"], TOL["tol_tie"]) == m - 1
    assert t.run_dual(1)[0] == 1
    (_, r, leaving), = dual_trace(t)
    assert (r, leaving) == (m - 1, n)
    t.close()


def test_entering_column_with_more_slots_in_the_tie_band_than_the_list_holds():
    """8,702 stored columns = 34 slots of 256.  Row 0 (b = -2) leaves; its entries are 0 in the columns below 300 and -1 from
    there on, and every cost is 1: 8,400 columns tie at ratio exactly 1, the minima of slots 1 to 33 are inside the band (slot 0
    holds no candidate), one more than the 32 the slot list holds, so the pick walks every slot.  Column 300 enters."""
    m, n = 2, 8700
    A = np.ones((m, n))
    A[0, :300] = 0.0
    md = covering_from(A, [2.0, 1.0])
    basis = dr.surplus_basis(m, n)
    ref = dr.dual_simplex(md, basis)
    assert ref.outcome == "optimal" and ref.max_band >= 8400 and ref.trace[0] == (300, 0, n)
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=16)
    t.from_basis(basis)
    assert t.nr_columns() == 8702
    assert t.run_dual(1 << 20) == (len(ref.trace), engine.OPTIMAL)
    assert dual_trace(t) == ref.trace
    assert close_to(t.objective_function_value(), ref.objective)
    t.close()
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    t.from_basis(basis)
    assert t.select_dual_pivot_column(0) == 300
    t.close()
