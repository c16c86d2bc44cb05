"""Host-driver paths of the three engines that no other GPU test pins: what `from_basis` refuses and the state it leaves
behind, its two paths (signed-permutation shortcut and the general factorisation), the two row selectors of the step-wise
API, `basis_inverse()` with updates pending, a trace shorter than the solve, the ranging lists growing on one handle and an
rhs change summed in shares.

The LP is `synthetic.dense_lp(24, 32, SEED)` with SEED = 1: through the CPU oracle it is feasible and optimal after 18
pivots, all of them in phase 2 (b > 0: the all-slack basis is feasible, phase 1 is empty and no row is removed).
"""
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic
from oracle import relp_f64

pytestmark = pytest.mark.gpu

M, N, SEED = 24, 32, 1
KINDS = [engine.ENGINE_REVISED, engine.ENGINE_TABLEAU, engine.ENGINE_LU]
E_ARG, E_SINGULAR = -1, -4
TOL = 1e-9


@pytest.fixture(scope="module")
def problem():
    """The LP, the oracle's state at the start and at the optimum (computed once, read only)."""
    lp = synthetic.dense_lp(M, N, SEED)
    md = MatrixData.from_dense_le(lp["A"], lp["b"], lp["c"])
    start = relp_f64.OracleF64(md.ensure_csc())
    b_start = start.b().copy()
    ref = relp_f64.OracleF64(md.ensure_csc())
    assert ref.run() == "optimal" and len(ref.trace) >= 10 and ref.m == M
    return {"md": md, "A": np.asarray(lp["A"]), "b_start": b_start, "objective": ref.objective, "b_opt": ref.b().copy(),
            "basis_opt": ref.basis().astype(np.int32)}


def slack_basis():
    return np.arange(N, N + M, dtype=np.int32)


def basis_matrix(A, basis):
    """Columns of [A | I] (every constraint is <=: slack column N + i is e_i)."""
    B = np.zeros((M, M))
    for k, j in enumerate(basis):
        if j < N:
            B[:, k] = A[:, j]
        else:
            B[j - N, k] = 1.0
    return B


def status_of(err):
    return int(re.search(r"\((-?\d+)\)", str(err.value)).group(1))


def assert_reaches_the_optimum(t, problem):
    assert t.solve_relaxation() == engine.OPTIMAL
    assert abs(t.objective_function_value() - problem["objective"]) <= TOL * max(1.0, abs(problem["objective"]))


@pytest.mark.parametrize("kind", KINDS)
def test_from_basis_refuses_a_column_out_of_range(problem, kind):
    t = engine.Tableau(problem["md"], engine=kind)
    n_provider = t.nr_columns() - t.nr_artificial_variables()
    assert n_provider == N + M
    basis = slack_basis()
    basis[5] = n_provider
    with pytest.raises(engine.RelpError) as err:
        t.from_basis(basis)
    assert status_of(err) == E_ARG
    assert_reaches_the_optimum(t, problem)
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_from_basis_refuses_a_column_twice(problem, kind):
    t = engine.Tableau(problem["md"], engine=kind)
    basis = problem["basis_opt"].copy()
    basis[7] = basis[3]
    with pytest.raises(engine.RelpError) as err:
        t.from_basis(basis)
    assert status_of(err) == E_SINGULAR
    if kind != engine.ENGINE_LU:                           # (the LU engine does not promise its state after this refusal)
        assert_reaches_the_optimum(t, problem)
    t.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["slack", "optimal"])
def test_from_basis_on_both_paths(problem, kind, which):
    """The all-slack basis is a signed permutation (the revised engine's shortcut), the optimal basis is general."""
    basis = slack_basis() if which == "slack" else problem["basis_opt"]
    t = engine.Tableau(problem["md"], engine=kind)
    t.from_basis(basis)
    assert t.phase == 2 and t.basis_indices().tolist() == basis.tolist()
    identity = t.basis_inverse() @ basis_matrix(problem["A"], basis)
    assert np.max(np.abs(identity - np.eye(M))) <= TOL
    np.testing.assert_allclose(t.b(), problem["b_start"] if which == "slack" else problem["b_opt"], rtol=TOL, atol=TOL)
    if which == "optimal":
        assert t.run(1 << 20) == (0, engine.OPTIMAL)
        assert abs(t.objective_function_value() - problem["objective"]) <= TOL * max(1.0, abs(problem["objective"]))
    else:
        assert_reaches_the_optimum(t, problem)
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_row_selectors_agree(problem, kind):
    """select_primal_pivot_row() on the column the device holds and select_primal_pivot_row(column=...) on its copy."""
    t = engine.Tableau(problem["md"], engine=kind)
    assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE     # (empty)
    for _ in range(10):
        q, dq = t.select_primal_pivot_column(engine.STEEPEST_DESCENT)
        col = t.generate_column(q)
        on_device = t.select_primal_pivot_row()
        of_copy = t.select_primal_pivot_row(column=col)
        assert on_device is not None and on_device == of_copy
        t.bring_into_basis(q, on_device, dq)
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_trace_with_a_capacity_below_the_pivot_count(problem, kind):
    """The trace keeps the first `trace_capacity` pivots; the four arrays sit `trace_capacity` apart in one buffer."""
    ref = relp_f64.OracleF64(problem["md"].ensure_csc())
    assert ref.run() == "optimal"
    t = engine.Tableau(problem["md"], engine=kind, trace_capacity=5)
    assert_reaches_the_optimum(t, problem)
    assert t.iterations() == len(ref.trace) > 5
    assert t.trace() == ref.trace[:5]
    t.close()


def optimal_tableau(problem, **kwargs):
    t = engine.Tableau(problem["md"], engine=engine.ENGINE_TABLEAU, **kwargs)
    assert_reaches_the_optimum(t, problem)
    return t


def test_ranging_lists_grow_and_are_reused(problem):
    """A 1-row query, 17 rows, 1 row on one handle (its device lists are allocated, grown, reused) against three fresh handles."""
    lists = [np.array([3], dtype=np.int32), np.arange(17, dtype=np.int32), np.array([M - 1], dtype=np.int32)]
    one = optimal_tableau(problem)
    for rows in lists:
        fresh = optimal_tableau(problem)
        for query in ("row_ratios", "rhs_ranging"):
            got, want = getattr(one, query)(rows), getattr(fresh, query)(rows)
            for g, w in zip(got, want):
                assert g.shape == (len(rows),) and np.array_equal(g, w)
        fresh.close()
    one.close()


@pytest.mark.parametrize("splits", [4, 2])
def test_rhs_change_in_shares(problem, splits, monkeypatch):
    """RELP_TAB_RHS_SPLITS (read at create) 4 and 2: the per-share partial sums of a full-list change against B b = rhs solved
    on the CPU from the problem's own columns, and (a consistency check) against the engine's own B^-1 times the new rhs."""
    monkeypatch.setenv("RELP_TAB_RHS_SPLITS", str(splits))
    t = optimal_tableau(problem)
    rhs = t.right_hand_side()
    new_rhs = rhs * (1.0 + 0.01 * (1 + np.arange(M) % 3))
    Binv = t.basis_inverse()
    t.change_right_hand_side(np.arange(M), new_rhs)
    assert t.rhs_stats()[3] == splits
    np.testing.assert_allclose(t.b(), np.linalg.solve(basis_matrix(problem["A"], t.basis_indices()), new_rhs), rtol=TOL, atol=TOL)
    np.testing.assert_allclose(t.b(), Binv @ new_rhs, rtol=TOL, atol=TOL)
    np.testing.assert_array_equal(t.right_hand_side(), new_rhs)
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_basis_inverse_with_updates_pending(problem, kind):
    t = engine.Tableau(problem["md"], engine=kind, update_block=4)
    assert t.update_block() == 4
    assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE
    assert t.run(7)[0] == 7                                # 7 = 4 + 3: three updates are pending
    identity = t.basis_inverse() @ basis_matrix(problem["A"], t.basis_indices())
    assert np.max(np.abs(identity - np.eye(M))) <= TOL
    t.close()
