"""Warm start (`from_basis`) and re-inversion / re-tabulation of the two dense engines at any number of rows.

A rebuild solves with the factors of the basis for many right-hand sides in one launch: the m rows of B^-1 (revised engine)
or every stored column of the tableau.  Up to m = 9,984 each workgroup keeps its work vector x in LDS; beyond that the
workgroups keep x in slabs of global memory and walk the right-hand sides in a grid-stride loop (relp_kernels_lu.hip:
k_lu_ftran_cols_slab, k_lu_btran_rows_slab).  RELP_RETAB_GLOBAL=1 takes the second path at any m and RELP_RETAB_GROUPS=n
caps its workgroups, so the small cases here run it with several trips per slab and a partial last trip; the arithmetic is
the same in the same order, so its results are asked to equal the LDS path's bit for bit.  The last two tests run at
m = 10,000, where no switch is needed.
"""
import contextlib
import os
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic
from oracle import relp_f64
import edge_lps

pytestmark = pytest.mark.gpu

DENSE_KINDS = [engine.ENGINE_REVISED, engine.ENGINE_TABLEAU]
TOL = 1e-9
OBJ_RTOL = 1e-9


@contextlib.contextmanager
def environment(**values):
    """Environment variables as the engine reads them at create; None = unset."""
    old = {k: os.environ.get(k) for k in values}
    for k, v in values.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def create(md, groups=None, **kwargs):
    """An engine on the forced slab path with at most `groups` workgroups, or (groups None) with neither switch set."""
    with environment(RELP_RETAB_GLOBAL=None if groups is None else 1, RELP_RETAB_GROUPS=groups):
        return engine.Tableau(md, **kwargs)


def rebuilt_state(t):
    return {"Binv": t.basis_inverse(), "b": t.b(), "d": t.relative_costs(), "minus_pi": t.minus_pi()}


def assert_same_state(plain, forced, what):
    for key in plain:
        assert np.array_equal(plain[key], forced[key]), (what, key)


def dense_le(m, n, seed):
    lp = synthetic.dense_lp(m, n, seed)
    return lp, MatrixData.from_dense_le(lp["A"], lp["b"], lp["c"])


def basis_matrix(A, basis):
    """Columns of [A | I] (every constraint is <=: slack column n + i is e_i)."""
    m, n = A.shape
    B = np.zeros((m, m))
    for k, j in enumerate(basis):
        if j < n:
            B[:, k] = A[:, j]
        else:
            B[j - n, k] = 1.0
    return B


# ------------------------------------------------------------------------------------------------
# 1. forced slab path == LDS path, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """synthetic.dense_lp(24, 32, 1), the LP of tests/test_gpu_host_driver.py, and the oracle's optimal basis."""
    lp, md = dense_le(24, 32, 1)
    ref = relp_f64.OracleF64(md.ensure_csc())
    assert ref.run() == "optimal" and len(ref.trace) == 18
    basis = ref.basis().astype(np.int32)
    assert int((basis < 32).sum()) == 8
    return {"md": md, "basis": basis}


@pytest.mark.parametrize("kind", DENSE_KINDS)
def test_forced_slab_path_equals_the_lds_path_bit_for_bit(small, kind):
    """56 stored columns (tableau) or 24 rows (revised) over 3 workgroups: several trips per slab, the last one partial."""
    plain = create(small["md"], engine=kind)
    forced = create(small["md"], groups=3, engine=kind)
    plain.from_basis(small["basis"])
    forced.from_basis(small["basis"])
    assert_same_state(rebuilt_state(plain), rebuilt_state(forced), kind)
    lds, slab, groups, nbytes = forced.retab_stats()
    assert (lds, slab, groups) == (0, 1, 3) and nbytes >= 3 * 24 * 8
    assert plain.retab_stats() == (1, 0, 0, 0)
    assert forced.run(1 << 20) == (0, engine.OPTIMAL)
    plain.close()
    forced.close()


# ------------------------------------------------------------------------------------------------
# 2. more workgroups asked for than right-hand sides, and m = 1
# ------------------------------------------------------------------------------------------------
def warm_start(t, basis):
    """from_basis and what it leaves: ("ok", state, run's answer) or ("refused", status)."""
    try:
        t.from_basis(basis)
    except engine.RelpError as e:
        return ("refused", int(re.search(r"\((-?\d+)\)", str(e)).group(1)))
    return ("ok", rebuilt_state(t), t.run(1 << 20))


@pytest.mark.parametrize("kind", DENSE_KINDS)
@pytest.mark.parametrize("name", ["1x1 le", "range row"])
def test_more_workgroups_asked_for_than_right_hand_sides(name, kind):
    md = edge_lps.CASES[name]
    ref = relp_f64.OracleF64(md.ensure_csc())
    ref.run()
    basis = ref.basis().astype(np.int32)
    plain = create(md, engine=kind)
    forced = create(md, groups=64, engine=kind)
    # (at create every column is stored, the artificial block included)
    right_hand_sides = forced.nr_rows() if kind == engine.ENGINE_REVISED else forced.nr_columns()
    want, got = warm_start(plain, basis), warm_start(forced, basis)
    assert got[0] == want[0], (name, want, got)
    if want[0] == "ok":
        assert_same_state(want[1], got[1], name)
        assert got[2] == want[2], name
    else:
        assert got[1] == want[1], name
    lds, slab, groups, _ = forced.retab_stats()
    assert lds == 0 and groups <= right_hand_sides
    assert groups >= 1 if slab else groups == 0
    assert plain.retab_stats()[1:] == (0, 0, 0)
    plain.close()
    forced.close()


# ------------------------------------------------------------------------------------------------
# 3. m one past the thread count
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DENSE_KINDS)
def test_one_row_more_than_threads(kind):
    """m = 257 = kLuThreads + 1: the loops over the slab take a second pass for one entry."""
    lp, md = dense_le(257, 8, 2)
    ref = relp_f64.OracleF64(md.ensure_csc())
    assert ref.run() == "optimal" and len(ref.trace) == 8
    basis = ref.basis().astype(np.int32)
    assert int((basis < 8).sum()) == 6
    t = create(md, groups=5, engine=kind)
    t.from_basis(basis)
    assert t.retab_stats()[:3] == (0, 1, 5)
    identity = t.basis_inverse() @ basis_matrix(np.asarray(lp["A"]), basis)
    assert np.max(np.abs(identity - np.eye(257))) <= TOL
    np.testing.assert_allclose(t.b(), ref.b(), rtol=0, atol=TOL)
    assert t.run(1 << 20) == (0, engine.OPTIMAL)
    t.close()


# ------------------------------------------------------------------------------------------------
# 4. re-inversion every 4 pivots on the forced path keeps the oracle's pivots
# ------------------------------------------------------------------------------------------------
def test_reinversion_every_few_pivots_on_the_slab_path_keeps_the_oracle_path():
    """The loop of tests/test_gpu_parity.py::test_reinversion_every_few_pivots_keeps_the_oracle_path with every rebuild on
    the slab path, 3 workgroups (on the CPU oracle 39 of the 40 cases have 8 pivots or more and 9 are quirk cases, which
    the tableau engine skips: 40 + 40 + 31 = 111 runs)."""
    rng = np.random.default_rng(99)
    checked = 0
    for case in range(40):
        m, n = int(rng.integers(5, 70)), int(rng.integers(5, 100))
        d = synthetic.mixed_lp(m, n, 9300 + case, nnz_per_col=int(rng.integers(2, 6)), frac_negative_cost=0.1,
                               infeasible=(case % 9 == 8))
        md = MatrixData.from_sparse_dict(d)
        ref = relp_f64.OracleF64(md)
        status = ref.run(200000)
        quirk = any(r >= md.nr_eq + md.nr_range for r in ref.filtered_rows())
        for kind, block in ((engine.ENGINE_REVISED, 0), (engine.ENGINE_REVISED, 3), (engine.ENGINE_TABLEAU, 3)):
            if quirk and kind == engine.ENGINE_TABLEAU:
                continue                                   # defined by the explicit inverse only
            t = create(md, groups=3, engine=kind, update_block=block, trace_capacity=1 << 15)
            t.set_reinversion_interval(4)
            assert engine.OUTCOME_NAMES[t.solve_relaxation()] == status, case
            assert t.trace() == ref.trace, case
            if len(ref.trace) >= 8:
                assert t.reinversions() >= 1, case
                assert t.retab_stats()[1] >= 1, case
            assert t.retab_stats()[:2] == (0, t.reinversions()), case      # every rebuild is one batch solve, on the slabs
            if status == "optimal":
                assert abs(t.objective_function_value() - ref.objective) <= OBJ_RTOL * max(1.0, abs(ref.objective)), case
            t.close()
            checked += 1
    assert checked >= 100


# ------------------------------------------------------------------------------------------------
# 5, 6. the real size, no switch set
# ------------------------------------------------------------------------------------------------
BIG_M, BIG_N, BIG_SEED, BIG_HEAD = 10000, 16, 1, 14


@pytest.fixture(scope="module")
def big():
    """synthetic.dense_lp(10000, 16, 1) through the CPU oracle (computed once, read only): optimal after 28 pivots, all in
    phase 2, 11 structural columns in the optimal basis."""
    lp, md = dense_le(BIG_M, BIG_N, BIG_SEED)
    ref = relp_f64.OracleF64(md.ensure_csc())
    assert ref.run() == "optimal" and len(ref.trace) == 28 and {ph for ph, _, _, _ in ref.trace} == {2}
    assert int((ref.basis() < BIG_N).sum()) == 11
    return {"md": md, "trace": list(ref.trace), "objective": ref.objective}


@pytest.mark.parametrize("kind", [engine.ENGINE_TABLEAU, engine.ENGINE_REVISED])
def test_warm_start_at_ten_thousand_rows(big, kind):
    """Engine A pivots 14 times from the slack basis; a fresh engine B is warm-started on A's basis.  (B^-1 is not
    downloaded at this size.)  Before the slab path the tableau engine refused this with RELP_E_SINGULAR (-4)."""
    with environment(RELP_RETAB_GLOBAL=None, RELP_RETAB_GROUPS=None):
        a = engine.Tableau(big["md"], engine=kind, trace_capacity=4096)
        b = engine.Tableau(big["md"], engine=kind, trace_capacity=4096)
    assert a.run(1 << 20)[1] == engine.PHASE_ONE_DONE      # (empty)
    assert a.run(BIG_HEAD) == (BIG_HEAD, engine.RUNNING)
    b.from_basis(a.basis_indices())
    b_a, b_b = a.b(), b.b()
    scale = max(1.0, float(np.max(np.abs(b_a))))
    assert np.max(np.abs(b_b - b_a)) <= TOL * scale
    assert abs(b.objective_function_value() - a.objective_function_value()) <= TOL * scale
    lds, slab, groups, nbytes = b.retab_stats()
    assert lds == 0 and slab == 1 and groups >= 1 and nbytes >= groups * BIG_M * 8
    assert a.run(1 << 20)[1] == engine.OPTIMAL
    assert b.run(1 << 20)[1] == engine.OPTIMAL
    assert a.trace() == big["trace"]
    assert b.trace() == big["trace"][BIG_HEAD:]
    for t in (a, b):
        assert abs(t.objective_function_value() - big["objective"]) <= OBJ_RTOL * max(1.0, abs(big["objective"]))
        t.close()


def test_retabulation_at_ten_thousand_rows(big):
    """A hand-set interval of 10 pivots on the tableau engine: 28 pivots, two re-tabulations.  Before the slab path the
    interval was ignored at this size and relp_reinversions stayed 0."""
    with environment(RELP_RETAB_GLOBAL=None, RELP_RETAB_GROUPS=None):
        t = engine.Tableau(big["md"], engine=engine.ENGINE_TABLEAU, trace_capacity=4096)
    t.set_reinversion_interval(10)
    assert t.solve_relaxation() == engine.OPTIMAL
    assert t.trace() == big["trace"]
    assert t.reinversions() >= 2
    assert t.retab_stats()[:2] == (0, t.reinversions())
    assert abs(t.objective_function_value() - big["objective"]) <= OBJ_RTOL * max(1.0, abs(big["objective"]))
    t.close()
