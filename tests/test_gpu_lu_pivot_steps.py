"""Every step of the LU engine's persistent pivot kernel (relp_kernels_ft.hip: k_ft_run) in every kernel layout, under every
pivot rule and both ratio rules, against the f64 CPU oracle pivot by pivot.

The other LU tests run layout 0 at sizes where most branches of PRICE and of the ratio test are never taken.  The LPs here are
the smallest that take them:

* `sparse_lp(40, 150, 3, nnz_per_col=30)`: 70 rows, fewer columns than one chunk of 512 threads; 147 columns of 9..24 entries
  (second tier of the PRICE copy) and 3 of more than 24 (priced from the CSC arrays).
* `sparse_lp(40, 1300, 5, nnz_per_col=10)`: 326 rows, more than two chunks of columns and not a multiple of 512; 367 columns
  within the first tier, 933 in the second.
* `sparse_lp(850, 1100, 9)`: 1,072 rows, more than the two rows per thread layout 0 keeps in registers; the first 400 pivots
  only (a full solve takes the oracle far longer).

Layouts 1 and 2 are forced through RELP_FT_BIG (read at create); the layout-2 case with RELP_FT_GRID_PRICE enters the kernel
with the column a grid-wide PRICE chose.
"""
import functools

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from oracle import relp_f64
from rust_lp_amd import MatrixData, engine, synthetic
from test_gpu_parity import OBJ_RTOL, VEC_TOL

pytestmark = pytest.mark.gpu

# name -> (arguments of synthetic.sparse_lp, pivots compared (None = the whole solve), the oracle's outcome)
LPS = {
    "70x150-long-columns": ((40, 150, 3), {"nnz_per_col": 30}, None, "optimal"),
    "326x1300": ((40, 1300, 5), {"nnz_per_col": 10}, None, "optimal"),
    "1072x1100-prefix": ((850, 1100, 9), {}, 400, "iteration_limit"),
}
RULES = [(engine.FIRST_PROFITABLE_WITH_MEMORY, engine.STEEPEST_DESCENT), (engine.FIRST_PROFITABLE, engine.FIRST_PROFITABLE),
         (engine.STEEPEST_DESCENT, engine.STEEPEST_DESCENT)]


@functools.lru_cache(maxsize=None)
def _problem(name):
    args, kw, _, _ = LPS[name]
    return MatrixData.from_sparse_dict(synthetic.sparse_lp(*args, **kw))


@functools.lru_cache(maxsize=None)
def _reference(name, rules, ratio_rule):
    """The oracle's run, computed once per (LP, rules, ratio rule) and shared by the layouts; nobody changes it."""
    _, _, pivots, outcome = LPS[name]
    ref = relp_f64.OracleF64(_problem(name), phase_one_rule=rules[0], phase_two_rule=rules[1], ratio_rule=ratio_rule)
    status = ref.run() if pivots is None else ref.run(max_iters=pivots)
    assert status == outcome, (name, rules, ratio_rule, status)
    return ref


def _check(name, layout, rules, ratio_rule, grid_price=False):
    _, _, pivots, outcome = LPS[name]
    ref = _reference(name, rules, ratio_rule)
    t = engine.Tableau(_problem(name), engine=engine.ENGINE_LU, phase_one_rule=rules[0], phase_two_rule=rules[1],
                       ratio_rule=ratio_rule, trace_capacity=1 << 13)
    lay = t.lu_kernel_layout()
    assert lay["persistent_kernel"] and lay["layout"] == layout and bool(lay["grid_price"]) == grid_price, lay
    if name == "1072x1100-prefix":
        assert t.nr_rows() > 1024
    total, oc = 0, engine.RUNNING
    limit = pivots if pivots is not None else 1 << 20
    while total < limit:
        done, oc = t.run(limit - total)
        total += done
        if oc not in (engine.RUNNING, engine.PHASE_ONE_DONE):
            break
    if outcome == "optimal":
        assert oc == engine.OPTIMAL
    else:
        assert total == pivots
    assert t.trace() == ref.trace
    # as assert_state_close of test_gpu_parity.py: objective, b, basis
    assert abs(t.objective_function_value() - ref.objective) <= OBJ_RTOL * max(1.0, abs(ref.objective))
    bref = ref.b()
    assert np.max(np.abs(t.b() - bref)) <= VEC_TOL * max(1.0, np.max(np.abs(bref)))
    assert t.basis_indices().tolist() == ref.basis().tolist()
    t.close()


@pytest.mark.parametrize("ratio_rule", [engine.RATIO_REFERENCE, engine.RATIO_LARGEST_PIVOT])
@pytest.mark.parametrize("rules", RULES, ids=["memory-dantzig", "first-first", "dantzig-dantzig"])
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("name", list(LPS))
def test_pivot_steps_match_the_oracle(name, layout, rules, ratio_rule, monkeypatch):
    monkeypatch.setenv("RELP_FT_BIG", str(layout))
    _check(name, layout, rules, ratio_rule)


def test_external_price_entry_in_layout_2(monkeypatch):
    """Dantzig's rule with PRICE as a grid launch per pivot: the kernel makes one pivot per launch with the column in the
    record."""
    monkeypatch.setenv("RELP_FT_BIG", "2")
    monkeypatch.setenv("RELP_FT_GRID_PRICE", "1")
    _check("326x1300", 2, RULES[2], engine.RATIO_REFERENCE, grid_price=True)
