"""The PRICE copy of the structural columns (relp_kernels.h: PriceEll) at the sizes where its tables part: a column of up to
kPriceSlots = 8 entries lives in the k-major table alone, a longer one is flagged there and kept once more, complete, among the
long columns (up to kPriceLongSlots = 24 entries), a longer one still is priced from the CSC arrays.  Layout 2 of the persistent
kernel reads the same tables with 32-bit row indices.  The LP has a column of 9 entries, one of 25 and a full one among short
ones, with costs that bring each of the three into the basis and out again; every pivot prices all of them, so a wrong
slot, flag or list shows in the trace.
"""
import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from oracle import relp_f64
from rust_lp_amd import MatrixData, engine, synthetic

pytestmark = pytest.mark.gpu

M, N, SEED = 40, 72, 20251019


def _lp():
    """min c'x, A x <= b, x >= 0 with A > 0, b > 0, c < 0 (feasible at the origin, bounded); small integers throughout."""
    def draw(stream, count, mod):
        return (synthetic.splitmix64(SEED, stream, np.arange(count, dtype=np.uint64)) % np.uint64(mod)).astype(np.int64)
    lengths = [9, 25, M] + [1 + int(v) for v in draw(11, N - 3, 8)]              # the three long columns, then 1 .. 8 entries
    order = np.argsort(draw(12, N, 1 << 30), kind="stable")                      # ... shuffled among each other
    cost = -(1 + draw(14, N, 30))
    cost[:3] = [-30, -60, -100]                            # (attractive: each of the three enters the basis and leaves it again)
    col_ptr, row_idx, values = [0], [], []
    for j in order:
        rows = np.argsort(draw(100 + int(j), M, 1 << 30), kind="stable")[:lengths[j]]
        vals = 1 + draw(300 + int(j), lengths[j], 9)
        for k in np.argsort(rows, kind="stable"):
            row_idx.append(int(rows[k])); values.append(float(vals[k]))
        col_ptr.append(len(row_idx))
    return {"m": M, "n": N, "nr_eq": 0, "nr_range": 0, "nr_le": M, "nr_ge": 0,
            "col_ptr": np.array(col_ptr, dtype=np.int64), "row_idx": np.array(row_idx, dtype=np.int32),
            "values": np.array(values, dtype=np.float64), "b": (20 + draw(13, M, 60)).astype(np.float64),
            "c": cost[order].astype(np.float64), "ub": np.full(N, np.inf)}


@pytest.fixture(scope="module")
def case():
    md = MatrixData.from_sparse_dict(_lp())
    counts = np.diff(md.col_ptr)
    assert sorted(counts)[-3:] == [9, 25, M] and (counts <= 8).sum() == N - 3
    ref = relp_f64.OracleF64(md)
    assert ref.run() == "optimal"
    entered = {p[1] for p in ref.trace}
    assert all(j in entered for j in np.flatnonzero(counts > 8)), "a long column never enters: the LP does not exercise its prices"
    return md, ref


@pytest.mark.parametrize("layout", [0, 2])
def test_long_and_very_long_columns_are_priced_like_the_oracle_prices_them(case, layout, monkeypatch):
    md, ref = case
    if layout == 2:
        monkeypatch.setenv("RELP_FT_BIG", "2")             # (read when the engine is made)
    t = engine.Tableau(md, engine=engine.ENGINE_LU, trace_capacity=4096)
    lay = t.lu_kernel_layout()
    assert lay["persistent_kernel"] and lay["layout"] == layout, lay
    assert t.solve_relaxation() == engine.OPTIMAL
    assert t.trace() == ref.trace, "pivot sequence differs from the CPU oracle"
    assert abs(t.objective_function_value() - ref.objective) <= 1e-9 * max(1.0, abs(ref.objective))
