"""The tableau flush rewrites only the columns with a nonzero entry among the pending rows R0 (the others have
T0 + W R0 = T0).  Every case runs the same LP twice in one process, with RELP_TAB_FLUSH_ALL=1 (every owned column,
the control) and without it, and asks for equal float64 results: the pivot trace, b, the basis, the objective and
every column of the tableau.  `==`, not a tolerance: a skipped column keeps its bits exactly (a -0.0 the full flush
would have turned into +0.0 compares equal)."""
import contextlib
import os

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def flush_all(on):
    """RELP_TAB_FLUSH_ALL as the engine reads it at create."""
    old = os.environ.get("RELP_TAB_FLUSH_ALL")
    os.environ["RELP_TAB_FLUSH_ALL"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["RELP_TAB_FLUSH_ALL"]
        else:
            os.environ["RELP_TAB_FLUSH_ALL"] = old


def dense_md(lp):
    return MatrixData.from_dense_le(lp["A"], lp["b"], lp["c"])


def state(t):
    return {"trace": t.trace(), "b": t.b(), "basis": t.basis_indices(), "objective": t.objective_function_value(),
            "T": np.stack([t.generate_column(j) for j in range(t.nr_columns())])}


def assert_same(full, listed):
    assert listed["trace"] == full["trace"]
    assert np.array_equal(listed["b"], full["b"])
    assert np.array_equal(listed["basis"], full["basis"])
    assert listed["objective"] == full["objective"]
    assert listed["T"].shape == full["T"].shape
    bad = np.argwhere(~(listed["T"] == full["T"]))
    assert bad.size == 0, f"{len(bad)} tableau entries differ, first (column, row) {tuple(bad[0])}"


def run_both(make, drive):
    """make() -> Tableau, drive(t) -> None; returns {flush_all: (state, (flushes, columns flushed))}."""
    out = {}
    for on in (True, False):
        with flush_all(on):
            t = make()
        drive(t)
        stats = t.flush_stats()
        out[on] = (state(t), stats)
        t.close()
    assert_same(out[True][0], out[False][0])
    return out


def owned_columns(stats_full):
    flushes, cols = stats_full
    assert flushes > 0 and cols % flushes == 0
    return cols // flushes


def test_dense_c2_size_skips_about_half_the_columns():
    """2,000 x 2,000 (bench.py's c2), K = 64, the first 640 pivots from the slack basis: the basic slacks' columns are
    unit vectors whose R0 entries are zero unless their row was pivoted in the block, so close to half of the 4,000
    stored columns are skipped at every flush."""
    lp = synthetic.dense_lp(2000, 2000, 20250001)
    md = dense_md(lp)

    def drive(t):
        assert t.update_block() == 64
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        done, oc = t.run(640)
        assert done == 640 and oc == engine.RUNNING

    out = run_both(lambda: engine.Tableau(md, trace_capacity=1 << 12, engine=engine.ENGINE_TABLEAU), drive)
    n_owned = owned_columns(out[True][1])
    flushes, cols = out[False][1]
    assert n_owned == 4000 and flushes == out[True][1][0] == 10
    skipped = 1.0 - cols / (flushes * n_owned)
    assert 0.25 < skipped < 0.55, skipped


def test_dense_solve_to_optimum():
    lp = synthetic.dense_lp(300, 420, 7)
    md = dense_md(lp)

    def drive(t):
        assert t.solve_relaxation() == engine.OPTIMAL

    out = run_both(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=16, engine=engine.ENGINE_TABLEAU), drive)
    n_owned = owned_columns(out[True][1])
    flushes, cols = out[False][1]
    assert flushes == out[True][1][0] and cols < flushes * n_owned


@pytest.mark.parametrize("path,block", [("netlib/SC205.SIF", 4), ("netlib/25FV47.SIF", 16)])
def test_lp_with_artificials(path, block):
    """Phase 1 over the artificial block, the flush at the phase boundary, the removal of artificials left basic."""
    from lp_files import load
    gf, ex, md, emd = load(path, fixed=True)

    def drive(t):
        assert t.nr_artificial_variables() > 0
        assert t.solve_relaxation() == engine.OPTIMAL

    out = run_both(lambda: engine.Tableau(md, trace_capacity=1 << 15, update_block=block, engine=engine.ENGINE_TABLEAU), drive)
    n_owned = owned_columns(out[True][1])
    flushes, cols = out[False][1]
    assert flushes == out[True][1][0] and cols < flushes * n_owned


def test_retabulation():
    """The tableau rebuilt from the basis columns every 100 pivots (reinversion interval): flushes before and after."""
    lp = synthetic.dense_lp(320, 480, 11)
    md = dense_md(lp)

    def drive(t):
        t.set_reinversion_interval(100)
        assert t.solve_relaxation() == engine.OPTIMAL
        assert t.reinversions() > 0

    out = run_both(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=32, engine=engine.ENGINE_TABLEAU), drive)
    flushes, cols = out[False][1]
    assert cols < flushes * owned_columns(out[True][1])


def test_native_sharded_loop_thread_ranks():
    """Two engines on one GPU, each on its own column range, driven by relp_shard_run with the in-process collectives of
    tests/shard_threads.py: every rank lists and flushes its own columns."""
    import ctypes as C
    import torch
    from shard_threads import ThreadRank, ThreadWorld, run_ranks
    world, m, n, block = 2, 256, 512, 16
    lp = synthetic.dense_lp(m, n, 5)
    lib = engine.load_library()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()

    def solve(on):
        shared = ThreadWorld(world)
        tabs, ranks = [], []
        for r in range(world):
            cfg = engine.default_config(shard_rank=r, shard_count=world, engine=engine.ENGINE_TABLEAU, update_block=block,
                                        trace_capacity=1 << 14)
            md = MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=lp["b"], cost=lp["c"],
                            upper_bound=np.full(n, np.inf))
            lo, hi = engine.shard_plan(md, cfg)
            md.dense = np.asfortranarray(lp["A"][:, lo:hi])
            with flush_all(on):
                t = engine.Tableau(md, config=cfg)
            tabs.append(t)
            ranks.append(ThreadRank(shared, r, lib, t.handle, torch, dev))

        def body(r):
            t = tabs[r]
            done, oc = C.c_int64(), C.c_int32()
            assert lib.relp_shard_run(t.handle, 1 << 20, C.byref(done), C.byref(oc)) == 0, (lib.relp_last_error(t.handle).decode(), shared.errors)
            assert oc.value == engine.PHASE_ONE_DONE                  # (empty)
            assert lib.relp_shard_run(t.handle, 1 << 20, C.byref(done), C.byref(oc)) == 0, (lib.relp_last_error(t.handle).decode(), shared.errors)
            assert oc.value == engine.OPTIMAL
            return t.trace(), t.b(), t.basis_indices(), t.objective_function_value(), t.flush_stats()
        res = run_ranks(world, body)
        assert not shared.errors, shared.errors
        for t in tabs:
            t.close()
        return res

    full, listed = solve(True), solve(False)
    for (tr_f, b_f, bas_f, obj_f, st_f), (tr_l, b_l, bas_l, obj_l, st_l) in zip(full, listed):
        assert tr_l == tr_f and tr_l == full[0][0]
        assert np.array_equal(b_l, b_f) and np.array_equal(bas_l, bas_f) and obj_l == obj_f
        assert st_l[0] == st_f[0] and st_l[1] <= st_f[1]
    # rank 0 owns structural columns only (dense: nothing to skip), rank 1 the slacks
    assert listed[1][4][1] < full[1][4][1]
