"""The tableau engine's per-pivot kernels walk the p pending rows of an update block (W <- E W, the tableau row over R0,
the tableau column over W) with their loads issued in batches: RELP_TAB_LOAD_BATCH, read at create, is the batch size, and
1 is the serial loop (the control).  Only the loads move: every entry of W gets the same single fma and every fma chain
keeps its order, so each case runs the same LP once per batch size the kernels are instantiated for, in one process, and
asks for equal float64 results -- the pivot trace, b, the basis, the objective and every column of the tableau -- with
`==`, no tolerance.  RELP_TAB_W_SPLIT (how many workgroups share the columns of W for 256 rows in the fused update) is
varied the same way."""
import contextlib
import os

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic

pytestmark = pytest.mark.gpu

BATCHES = (1, 8, 16, 32)           # tab_load_batch (relp_kernels_tableau.hip); 1 first: the control
# (batch, split): every batch size with the default split, then other numbers of workgroups per 256 rows of W
VARIANTS = tuple((b, None) for b in BATCHES) + ((8, 1), (8, 3), (8, 4), (32, 4))


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


def dense_md(lp):
    return MatrixData.from_dense_le(lp["A"], lp["b"], lp["c"])


def state(t):
    return {"trace": t.trace(), "b": t.b(), "basis": t.basis_indices(), "objective": t.objective_function_value(),
            "T": np.stack([t.generate_column(j) for j in range(t.nr_columns())])}


def assert_same(control, got, what):
    assert got["trace"] == control["trace"], what
    assert np.array_equal(got["b"], control["b"]), what
    assert np.array_equal(got["basis"], control["basis"]), what
    assert got["objective"] == control["objective"], what
    assert got["T"].shape == control["T"].shape, what
    bad = np.argwhere(~(got["T"] == control["T"]))
    assert bad.size == 0, f"{what}: {len(bad)} tableau entries differ, first (column, row) {tuple(bad[0])}"


def run_variants(make, drive, variants=VARIANTS, **env):
    """make() -> Tableau, drive(t) -> list of states; every variant against the first one (batch 1)."""
    assert variants[0][0] == 1
    control = None
    for batch, split in variants:
        with environment(RELP_TAB_LOAD_BATCH=batch, RELP_TAB_W_SPLIT=split, **env):
            t = make()
        assert t.load_batch() == batch
        states = drive(t)
        t.close()
        if control is None:
            control = states
            continue
        assert len(states) == len(control)
        for k, (c, g) in enumerate(zip(control, states)):
            assert_same(c, g, f"batch {batch}, split {split}, state {k}")
    return control


def test_unknown_batch_sizes_fall_back_to_the_default():
    lp = synthetic.dense_lp(24, 36, 3)
    md = dense_md(lp)
    with environment(RELP_TAB_LOAD_BATCH=None):
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    default = t.load_batch()
    t.close()
    assert default in BATCHES and default != 1
    for value in ("0", "-4", "7", "64", "1000", "x"):
        with environment(RELP_TAB_LOAD_BATCH=value):
            t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
        assert t.load_batch() == default, value
        t.close()
    with environment(RELP_TAB_LOAD_BATCH=8):
        t = engine.Tableau(md, engine=engine.ENGINE_REVISED)
    assert t.load_batch() == 0                      # not a tableau engine
    t.close()


def test_dense_c2_size_through_flushes_and_to_the_optimum():
    """2,000 x 2,000 (bench.py's c2), K = 64: the state after 700 pivots from the slack basis (ten flushes and 60 pending
    rows, which the column kernel walks for every column of the tableau), and the state at the optimum."""
    lp = synthetic.dense_lp(2000, 2000, 20250001)
    md = dense_md(lp)

    def drive(t):
        assert t.update_block() == 64
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        done, oc = t.run(700)
        assert done == 700 and oc == engine.RUNNING
        mid = state(t)
        assert t.flush_stats()[0] == 10
        assert t.solve_relaxation() == engine.OPTIMAL
        return [mid, state(t)]

    out = run_variants(lambda: engine.Tableau(md, trace_capacity=1 << 17, engine=engine.ENGINE_TABLEAU), drive)
    assert len(out[1]["trace"]) > 700


@pytest.mark.parametrize("block", [3, 13, 64, 100])
def test_update_blocks_that_leave_a_tail_in_the_batch(block):
    """p runs over 0 .. K-1 in every update block: with K = 3, 13, 64 and 100 it passes every remainder of every batch
    size.  The state is also taken in the middle of a block (p = K - 1 pending rows, or 37)."""
    lp = synthetic.dense_lp(300, 420, 7)
    md = dense_md(lp)

    def drive(t):
        assert t.update_block() == block
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        pending = min(block - 1, 37)
        done, oc = t.run(2 * block + pending)
        assert done == 2 * block + pending and oc == engine.RUNNING
        mid = state(t)
        assert t.solve_relaxation() == engine.OPTIMAL
        return [mid, state(t)]

    out = run_variants(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=block, engine=engine.ENGINE_TABLEAU),
                       drive)
    assert len(out[1]["trace"]) > 3 * block


@pytest.mark.parametrize("path,block", [("netlib/SC205.SIF", 4), ("netlib/25FV47.SIF", 16)])
def test_lp_with_artificials_through_the_phase_switch(path, block):
    from lp_files import load
    gf, ex, md, emd = load(path, fixed=True)

    def drive(t):
        assert t.nr_artificial_variables() > 0
        assert t.solve_relaxation() == engine.OPTIMAL
        return [state(t)]

    out = run_variants(lambda: engine.Tableau(md, trace_capacity=1 << 15, update_block=block, engine=engine.ENGINE_TABLEAU),
                       drive)
    assert {ph for ph, _, _, _ in out[0]["trace"]} == {1, 2}


@pytest.mark.parametrize("block", [13, 64])
def test_unfused_update(block):
    """RELP_FUSED_UPDATE=0: k_ratio_blocks + k_tab_update_all, which walk the pending rows through the same helper."""
    lp = synthetic.dense_lp(300, 500, 4242)
    md = dense_md(lp)

    def drive(t):
        assert t.solve_relaxation() == engine.OPTIMAL
        return [state(t)]

    unfused = run_variants(lambda: engine.Tableau(md, trace_capacity=1 << 15, update_block=block, engine=engine.ENGINE_TABLEAU),
                           drive, variants=tuple((b, None) for b in BATCHES), RELP_FUSED_UPDATE="0")
    with environment(RELP_TAB_LOAD_BATCH=1, RELP_FUSED_UPDATE="1"):
        t = engine.Tableau(md, trace_capacity=1 << 15, update_block=block, engine=engine.ENGINE_TABLEAU)
    fused = drive(t)
    t.close()
    assert_same(unfused[0], fused[0], "fused against unfused")


def test_stepwise_api():
    """select column / generate column / select row / bring into basis: k_tab_column, k_tab_row_update and
    k_tab_update_w_vectors on their own, 45 pivots with K = 20."""
    lp = synthetic.dense_lp(280, 300, 19)
    md = dense_md(lp)

    def drive(t):
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        for _ in range(45):
            q, dq = t.select_primal_pivot_column(engine.STEEPEST_DESCENT)
            col = t.generate_column(q)
            r = t.select_primal_pivot_row()
            assert r is not None and col[r] > 0
            t.bring_into_basis(q, r, dq)
        return [state(t)]

    run_variants(lambda: engine.Tableau(md, trace_capacity=1 << 12, update_block=20, engine=engine.ENGINE_TABLEAU), drive,
                 variants=tuple((b, None) for b in BATCHES))


def test_retabulation():
    """The tableau rebuilt from the basis columns every 100 pivots (reinversion interval), K = 32."""
    lp = synthetic.dense_lp(320, 480, 11)
    md = dense_md(lp)

    def drive(t):
        t.set_reinversion_interval(100)
        assert t.solve_relaxation() == engine.OPTIMAL
        assert t.reinversions() > 0
        return [state(t)]

    run_variants(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=32, engine=engine.ENGINE_TABLEAU), drive)


def test_native_sharded_loop_thread_ranks():
    """Two engines on one GPU, each on its own column range, driven by relp_shard_run with the in-process collectives of
    tests/shard_threads.py: the fused update takes the entering column from the gathered messages."""
    import ctypes as C
    import torch
    from shard_threads import ThreadRank, ThreadWorld, run_ranks
    world, m, n, block = 2, 256, 512, 13
    lp = synthetic.dense_lp(m, n, 5)
    lib = engine.load_library()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()

    def solve(batch, split):
        shared = ThreadWorld(world)
        tabs, ranks = [], []
        for r in range(world):
            cfg = engine.default_config(shard_rank=r, shard_count=world, engine=engine.ENGINE_TABLEAU, update_block=block,
                                        trace_capacity=1 << 14)
            md = MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=lp["b"], cost=lp["c"],
                            upper_bound=np.full(n, np.inf))
            lo, hi = engine.shard_plan(md, cfg)
            md.dense = np.asfortranarray(lp["A"][:, lo:hi])
            with environment(RELP_TAB_LOAD_BATCH=batch, RELP_TAB_W_SPLIT=split):
                t = engine.Tableau(md, config=cfg)
            assert t.load_batch() == batch
            tabs.append(t)
            ranks.append(ThreadRank(shared, r, lib, t.handle, torch, dev))

        def body(r):
            t = tabs[r]
            done, oc = C.c_int64(), C.c_int32()
            assert lib.relp_shard_run(t.handle, 1 << 20, C.byref(done), C.byref(oc)) == 0, (lib.relp_last_error(t.handle).decode(), shared.errors)
            assert oc.value == engine.PHASE_ONE_DONE                  # (empty)
            assert lib.relp_shard_run(t.handle, 1 << 20, C.byref(done), C.byref(oc)) == 0, (lib.relp_last_error(t.handle).decode(), shared.errors)
            assert oc.value == engine.OPTIMAL
            return t.trace(), t.b(), t.basis_indices(), t.objective_function_value()
        res = run_ranks(world, body)
        assert not shared.errors, shared.errors
        for t in tabs:
            t.close()
        return res

    control = solve(1, None)
    assert len(control[0][0]) > 3 * block
    for batch, split in VARIANTS[1:]:
        got = solve(batch, split)
        for (tr_c, b_c, bas_c, obj_c), (tr_g, b_g, bas_g, obj_g) in zip(control, got):
            assert tr_g == tr_c and tr_g == control[0][0], (batch, split)
            assert np.array_equal(b_g, b_c) and np.array_equal(bas_g, bas_c) and obj_g == obj_c, (batch, split)
