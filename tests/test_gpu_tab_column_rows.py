"""The fused single-GPU loop of the tableau engine forms the tableau column with 256, 128 or 64 rows per workgroup
(RELP_TAB_COLUMN_ROWS, read at create; 256 is the control).  Below 256 the 256 threads of a workgroup stand on the same rows
in 2 or 4 slices, each slice loads its own share of the p pending rows of W at once, and the fma chain of a row is handed from
slice to slice: the chain of every row keeps its operations and their order, and a minimum over other blocks of rows is still
the minimum.  So each case solves the same LP once per value in one process and asks for equal float64 results -- the pivot
trace, b, the basis, the objective and every column of the tableau -- with `==`, no tolerance.  The unfused launches, the
step-wise calls and the sharded loop keep 256 rows whatever the switch says."""
import contextlib
import os

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic

pytestmark = pytest.mark.gpu

ROWS = (256, 128, 64)              # tab_column_rows (relp_kernels_tableau.hip); 256 first: the control


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


def run_rows(make, drive, rows=ROWS, **env):
    """make() -> Tableau, drive(t) -> list of states; every value of RELP_TAB_COLUMN_ROWS against the first one (256)."""
    assert rows[0] == 256
    control = None
    for r in rows:
        with environment(RELP_TAB_COLUMN_ROWS=r, RELP_TAB_LOAD_BATCH=None, **env):
            t = make()
        assert t.column_rows() == r
        states = drive(t)
        t.close()
        if control is None:
            control = states
            continue
        assert len(states) == len(control)
        for k, (c, g) in enumerate(zip(control, states)):
            assert_same(c, g, f"{r} rows per workgroup, state {k}")
    return control


def test_the_switch_and_the_default():
    lp = synthetic.dense_lp(24, 36, 3)
    md = dense_md(lp)
    lib = engine.load_library()
    for value in (None, "0", "-64", "32", "100", "512", "x"):
        with environment(RELP_TAB_COLUMN_ROWS=value, RELP_TAB_LOAD_BATCH=None):
            t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
        assert t.column_rows() == lib.relp_tab_column_rows_for(0, 24), value
        t.close()
    for value in ROWS:
        with environment(RELP_TAB_COLUMN_ROWS=value, RELP_TAB_LOAD_BATCH=None):
            t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
        assert t.column_rows() == value
        t.close()
    with environment(RELP_TAB_COLUMN_ROWS=64, RELP_TAB_LOAD_BATCH=1):
        t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    assert t.column_rows() == 64 and t.load_batch() == 1        # the two switches do not touch each other
    t.close()
    for block, value, rows in ((64, None, lib.relp_tab_column_rows_for(0, 24)), (65, None, 256), (100, None, 256), (100, 64, 64),
                               (100, 128, 128)):
        with environment(RELP_TAB_COLUMN_ROWS=value, RELP_TAB_LOAD_BATCH=None):
            t = engine.Tableau(md, update_block=block, engine=engine.ENGINE_TABLEAU)
        assert t.column_rows() == rows, (block, value)          # above 64 pivots per block only a value asked for leaves 256
        t.close()
    with environment(RELP_TAB_COLUMN_ROWS=64):
        t = engine.Tableau(md, engine=engine.ENGINE_REVISED)
    assert t.column_rows() == 0                     # not a tableau engine
    t.close()


@pytest.mark.parametrize("m", [5, 63, 64, 65, 130, 257, 300])
def test_row_counts_at_the_block_edges(m):
    """A last block of 1 row (65, 257), of 63 rows, exactly one and two blocks, fewer rows than one slice: the state after 20
    pivots with K = 13 (7 pending rows: two slices of 2, one of 2 and one of 1) and at the optimum."""
    lp = synthetic.dense_lp(m, m + m // 2 + 3, 100 + m)
    md = dense_md(lp)

    def drive(t):
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        done, oc = t.run(20)
        mid = state(t)
        mid["trace"] = (done, oc, mid["trace"])
        assert t.solve_relaxation() == engine.OPTIMAL
        return [mid, state(t)]

    out = run_rows(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=13, engine=engine.ENGINE_TABLEAU), drive)
    assert len(out[1]["trace"]) >= 1


@pytest.mark.parametrize("block", [1, 3, 13, 64, 100])
def test_update_blocks_and_shares(block):
    """p runs over 0 .. K-1 in every update block: empty slices (p < 4), shares of equal and of unequal length, a last slice
    that starts at p, and with K = 100 shares above 16 (the 32- and 64-entry register arrays).  States: right after a flush
    (p = 0), in the middle of a block (p = K - 1 pending rows, or 37), and at the optimum."""
    lp = synthetic.dense_lp(300, 420, 7)
    md = dense_md(lp)

    def drive(t):
        assert t.update_block() == block
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        done, oc = t.run(2 * block)
        assert done == 2 * block and oc == engine.RUNNING
        flushed = state(t)
        pending = min(block - 1, 37)
        done, oc = t.run(pending)
        assert done == pending and oc == engine.RUNNING
        mid = state(t)
        assert t.solve_relaxation() == engine.OPTIMAL
        return [flushed, mid, state(t)]

    out = run_rows(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=block, engine=engine.ENGINE_TABLEAU), drive)
    assert len(out[2]["trace"]) > 3 * block


def tie_lp():
    """200 x 260 with rows 63 = 64 and 127 = 128 (coefficients and right-hand side, the smallest of the LP).  Column 0 has a
    single 1 in row 64 and column 1 a single 1 in row 128, with the two lowest costs: they enter first, each in the only row
    it has, and change nothing else.  From then on rows 63 | 64 (and 127 | 128) tie in every ratio test they win, and the
    leaving-column order picks the higher row, whose basic column is 0 (1)."""
    lp = synthetic.dense_lp(200, 260, 31)
    A, b, c = lp["A"].copy(order="F"), lp["b"].copy(), lp["c"].copy()
    A[:, 0] = 0.0
    A[:, 1] = 0.0
    A[64, :] = A[63, :]
    A[128, :] = A[127, :]
    A[64, 0] = 1.0
    A[128, 1] = 1.0
    b[63] = b[64] = 1.0
    b[127] = b[128] = 1.25
    c[0], c[1] = -2.5, -2.375
    return {"A": A, "b": b, "c": c}


def test_ratio_ties_across_the_block_edges():
    """The tie band lists two blocks of minima under 64 rows per workgroup (63 | 64 and 127 | 128; the latter also under 128)
    that are one block under 256, and the winner is the row in the later block."""
    md = dense_md(tie_lp())

    def drive(t):
        assert t.solve_relaxation() == engine.OPTIMAL
        return [state(t)]

    out = run_rows(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=13, engine=engine.ENGINE_TABLEAU), drive)
    trace = out[0]["trace"]
    assert [(q, r) for _, q, r, _ in trace[:2]] == [(0, 64), (1, 128)]
    later = [(r, leaving) for _, _, r, leaving in trace[2:]]
    assert (64, 0) in later and (128, 1) in later       # the tied pair's higher row left, not row 63 / 127


def shadow_lp():
    """300 x 420 whose rows 63, 64 and 255 have the smallest right-hand sides (0.7 of the smallest other one): they are pivot
    rows early and more than once (a pivot row that repeats inside a block reuses its slot of W), so the shadow row of the
    previous pivot falls on the last row of a block of 64, on the first row of the next one and on the last row of a block
    of 256."""
    lp = synthetic.dense_lp(300, 420, 57)
    b = lp["b"].copy()
    b[[63, 64, 255]] = 0.7 * b.min()
    return {"A": lp["A"], "b": b, "c": lp["c"]}


def test_shadow_row_at_the_block_edges_and_slot_reuse():
    md = dense_md(shadow_lp())

    def drive(t):
        assert t.update_block() == 64
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        done, oc = t.run(40)
        assert done == 40 and oc == engine.RUNNING
        mid = state(t)
        assert t.solve_relaxation() == engine.OPTIMAL
        return [mid, state(t)]

    out = run_rows(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=64, engine=engine.ENGINE_TABLEAU), drive)
    rows = [r for _, _, r, _ in out[0]["trace"]]
    assert len(rows) == 40 and {63, 64, 255} <= set(rows)
    assert len(set(rows)) < len(rows)                   # a pivot row repeats inside the block


@pytest.mark.parametrize("path,block", [("netlib/SC205.SIF", 4), ("netlib/SC105.SIF", 13)])
def test_lp_with_artificials_through_the_phase_switch(path, block):
    from lp_files import load
    gf, ex, md, emd = load(path, fixed=True)

    def drive(t):
        assert t.nr_artificial_variables() > 0
        assert t.solve_relaxation() == engine.OPTIMAL
        return [state(t)]

    out = run_rows(lambda: engine.Tableau(md, trace_capacity=1 << 15, update_block=block, engine=engine.ENGINE_TABLEAU), drive)
    assert {ph for ph, _, _, _ in out[0]["trace"]} == {1, 2}


def test_retabulation():
    """The tableau rebuilt from the basis columns every 100 pivots (reinversion interval), K = 32."""
    lp = synthetic.dense_lp(320, 480, 11)
    md = dense_md(lp)

    def drive(t):
        t.set_reinversion_interval(100)
        assert t.solve_relaxation() == engine.OPTIMAL
        assert t.reinversions() > 0
        return [state(t)]

    run_rows(lambda: engine.Tableau(md, trace_capacity=1 << 14, update_block=32, engine=engine.ENGINE_TABLEAU), drive)


def test_unfused_update_keeps_256_rows():
    """RELP_FUSED_UPDATE=0 (k_ratio_blocks + k_tab_update_all behind the column kernel): the same results with and without
    RELP_TAB_COLUMN_ROWS=64 as with 256, and the same as the fused loop."""
    lp = synthetic.dense_lp(300, 500, 4242)
    md = dense_md(lp)

    def solve(**env):
        with environment(RELP_TAB_LOAD_BATCH=None, **env):
            t = engine.Tableau(md, trace_capacity=1 << 15, update_block=13, engine=engine.ENGINE_TABLEAU)
        assert t.solve_relaxation() == engine.OPTIMAL
        out = state(t)
        t.close()
        return out

    plain = solve(RELP_FUSED_UPDATE="0", RELP_TAB_COLUMN_ROWS=256)
    assert_same(plain, solve(RELP_FUSED_UPDATE="0", RELP_TAB_COLUMN_ROWS=64), "unfused, 64 rows asked for")
    assert_same(plain, solve(RELP_FUSED_UPDATE="1", RELP_TAB_COLUMN_ROWS=64), "fused with 64 rows against unfused")


def test_stepwise_calls_keep_256_rows():
    """select column / generate column / select row / bring into basis between two stretches of the loop: the step-wise calls
    read nothing the loop left in the block minima, whatever their geometry was."""
    lp = synthetic.dense_lp(280, 300, 19)
    md = dense_md(lp)

    def drive(t):
        assert t.run(1 << 20)[1] == engine.PHASE_ONE_DONE       # (empty)
        assert t.run(30)[0] == 30
        for _ in range(15):
            q, dq = t.select_primal_pivot_column(engine.STEEPEST_DESCENT)
            col = t.generate_column(q)
            r = t.select_primal_pivot_row()
            assert r is not None and col[r] > 0
            t.bring_into_basis(q, r, dq)
        assert t.run(30)[0] == 30
        return [state(t)]

    run_rows(lambda: engine.Tableau(md, trace_capacity=1 << 12, update_block=20, engine=engine.ENGINE_TABLEAU), drive)


def test_native_sharded_loop_keeps_256_rows():
    """Two engines on one GPU, each on its own column range, driven by relp_shard_run with the in-process collectives of
    tests/shard_threads.py: a message carries one minimum per 256 rows, with RELP_TAB_COLUMN_ROWS=256 and with 64."""
    import ctypes as C
    import torch
    from shard_threads import ThreadRank, ThreadWorld, run_ranks
    world, m, n, block = 2, 300, 512, 13
    lp = synthetic.dense_lp(m, n, 5)
    lib = engine.load_library()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()

    def solve(rows):
        shared = ThreadWorld(world)
        tabs, ranks = [], []
        for r in range(world):
            cfg = engine.default_config(shard_rank=r, shard_count=world, engine=engine.ENGINE_TABLEAU, update_block=block,
                                        trace_capacity=1 << 14)
            md = MatrixData(nr_normal=n, nr_eq=0, nr_range=0, nr_le=m, nr_ge=0, b=lp["b"], cost=lp["c"],
                            upper_bound=np.full(n, np.inf))
            lo, hi = engine.shard_plan(md, cfg)
            md.dense = np.asfortranarray(lp["A"][:, lo:hi])
            with environment(RELP_TAB_COLUMN_ROWS=rows, RELP_TAB_LOAD_BATCH=None):
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
            return t.trace(), t.b(), t.basis_indices(), t.objective_function_value()
        res = run_ranks(world, body)
        assert not shared.errors, shared.errors
        for t in tabs:
            t.close()
        return res

    control = solve(256)
    assert len(control[0][0]) > 3 * block
    got = solve(64)
    for (tr_c, b_c, bas_c, obj_c), (tr_g, b_g, bas_g, obj_g) in zip(control, got):
        assert tr_g == tr_c and tr_g == control[0][0]
        assert np.array_equal(b_g, b_c) and np.array_equal(bas_g, bas_c) and obj_g == obj_c
