"""The test reference of the dual simplex (tests/dual_reference.py) against itself and against the committed f64 oracle, on the
covering LPs `min c'x, A x >= b, c > 0` of `dual_reference.covering_lp`, from the all-surplus basis (dual feasible at once).

The f64 reference must walk the pivots of the exact (Fraction) one -- no tie band of these inputs ever holds two entries, so
the sequence does not hang on rounding -- and end on the optimum of the oracle's two-phase primal solve of the same
`MatrixData`.  The pivot counts are the ones the GPU tests (tests/test_gpu_dual.py) rely on."""
import pytest

import rust_lp_amd  # noqa: F401
from oracle import relp_f64

import dual_reference as dr

OBJ_RTOL = 1e-9
CASES = [(8, 8, 1, 5), (8, 8, 2, 3), (24, 32, 1, 13), (32, 48, 3, 21), (40, 300, 4, 39)]


@pytest.mark.parametrize("m,n,seed,pivots", CASES)
def test_f64_trace_equals_the_exact_one_and_ends_on_the_oracle_optimum(m, n, seed, pivots):
    md, exact = dr.covering_lp(m, n, seed)
    f64 = dr.dual_simplex(md, dr.surplus_basis(m, n))
    frac = dr.dual_simplex(md, dr.surplus_basis(m, n), exact=exact)
    assert f64.outcome == "optimal" and frac.outcome == "optimal"
    assert len(f64.trace) == pivots and len(frac.trace) == pivots
    assert f64.trace == frac.trace
    assert f64.max_band == 1 and frac.max_band == 1
    oracle = relp_f64.OracleF64(md.ensure_csc())
    assert oracle.run() == "optimal"
    assert len(oracle.trace) > 3 * pivots                  # the two-phase primal needs several times the pivots
    for objective in (f64.objective, float(frac.objective)):
        assert abs(objective - oracle.objective) <= OBJ_RTOL * max(1.0, abs(oracle.objective))
    assert min(f64.b) >= -1e-7 and min(frac.b) >= 0


@pytest.mark.parametrize("m,n,seed,pivots", [(300, 40, 5, 102), (257, 8, 2, 16)])
def test_f64_pivot_counts_of_the_tall_cases(m, n, seed, pivots):
    md, _ = dr.covering_lp(m, n, seed)
    f64 = dr.dual_simplex(md, dr.surplus_basis(m, n))
    assert f64.outcome == "optimal" and len(f64.trace) == pivots and f64.max_band == 1


def test_infeasible_lp_and_the_ratio_tie():
    """x1 + x2 <= 2, x1 + x2 >= 4: one pivot (the tie between columns 0 and 1 goes to the lower index), then no candidate."""
    md = dr.infeasible_pair()
    for exact in (None, dr.exact_of(md)):
        res = dr.dual_simplex(md, [2, 3], exact=exact)
        assert res.outcome == "infeasible" and res.trace == [(0, 1, 3)] and res.max_band == 2
