"""relp_pool_create .. relp_pool_stats of the tableau engine through the C ABI: the bit contracts of the price and of the add against a
twin handle that calls relp_add_columns with the host data of the same columns, the read-only contract (also inside a trial), the
stale rule, the refusals, and engine.column_generation on the cutting-stock instance of tests/pool_reference.py.

LPs: lp = synthetic.dense_lp(m, n + k, seed) as in tests/test_gpu_columns_in_place.py; the engine gets the first n columns and is
solved to the optimum, the pool holds the k columns held back: (24, 32, 1) with 17 pool columns and (40, 300, 4) with 70 (a second
slice of the pool).  update_block 3 (a flush every third iteration) and 64 (the block stays open: the calls run with rows pending).
Two handles made by the same calls hold the same bits (tests/test_gpu_columns_in_place.py relies on it too); `a` uses the pool,
`c` is the twin."""
import ctypes as C
import functools

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic

import column_reference as colref
import pool_reference as ref

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5
LPS = [(24, 32, 1, 17), (40, 300, 4, 70)]
BLOCKS = [3, 64]
OBJ_TOL = 1e-9                # tests/test_gpu_trial.py's margin against the committed oracle


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    lp = synthetic.dense_lp(m, n, seed)
    for v in lp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lp


def solved(m, n, seed, k, update_block):
    """(the new columns, their costs, a handle on the first n columns at the optimum)."""
    lp = dense_lp(m, n + k, seed)
    t = engine.Tableau(colref.narrow(lp, n), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, update_block=update_block)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    return (*pool_columns(m, n, seed, k), t)


def pool_columns(m, n, seed, k):
    """The columns held back: the even ones dense, the odd ones sparse (column j keeps its rows i % 4 == j % 4), column 2 empty.  By
    the f64 oracle's duals at the optimum of the narrow LP both LPS have columns with d < -0.04 and columns with d > 0.01."""
    lp = dense_lp(m, n + k, seed)
    A_new, cost = colref.new_columns(lp, n)
    i, j = np.indices(A_new.shape)
    A_new[(j % 2 == 1) & (i % 4 != j % 4)] = 0.0
    A_new[:, 2] = 0.0
    cost[2] = 1.5                                          # (an empty column with a negative cost would make the LP unbounded)
    return A_new, cost


def getters(t):
    """Everything a caller can read but relp_pool_stats, as bytes."""
    return dict(d=t.relative_costs().tobytes(), b=t.b().tobytes(), pi=t.minus_pi().tobytes(), basis=t.basis_indices().tobytes(),
                objective=t.objective_function_value(), trace=t.trace(), reinversions=t.reinversions(), flushes=t.flush_stats(),
                rhs=t.right_hand_side().tobytes(), rows=t.nr_rows(), columns=t.nr_columns(), iterations=t.iterations(),
                stats=(t.cut_stats(), t.column_stats(), t.rhs_stats(), t.cost_stats(), t.removal_stats(), t.ranging_stats(), t.gomory_stats(),
                       t.trial_stats(), t.retab_stats()))


def status_of(call):
    with pytest.raises(engine.RelpError) as err:
        call()
    return int(str(err.value).split("(")[1].split(")")[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


# ---- the price ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_block", BLOCKS)
@pytest.mark.parametrize("m,n,seed,k", LPS)
def test_price_and_twin(m, n, seed, k, update_block):
    A_new, cost, a = solved(m, n, seed, k, update_block)
    _, _, c = solved(m, n, seed, k, update_block)
    pool = a.pool(A_new, cost)
    nnz = int(np.count_nonzero(A_new))
    assert pool.stats()[:2] == (k, nnz) and pool.stats()[2] % 64 == 0 and pool.stats()[2] >= nnz and pool.stats()[3] == 0
    d = pool.reduced_costs()
    assert bits(d) == bits(ref.reduced_costs(A_new, cost, a.minus_pi()))          # the model: fma chains over -pi as the getter gives it
    assert bits(d[2:3]) == bits(cost[2:3])                                        # the column without entries: d = cost to the bit
    c.add_columns(A_new, cost)
    assert bits(d) == bits(c.relative_costs()[n + m:])                            # the twin: what relp_add_columns would have made
    assert (d < -1e-7).any() and (d > 0).any()
    active = np.ones(k, dtype=np.uint8)
    for segments, tol in ((1, 1e-7), (3, 0.0), (k, 1e-7), (5, 0.05)):
        ids, dw = pool.price(segments, tol)
        want_ids, want_d = ref.winners(d, active, segments, tol)
        assert ids.tolist() == want_ids.tolist() and bits(dw) == bits(want_d)
    best = int(pool.price()[0][0])
    pool.set_active([best], False)                         # the column that would have won is switched off: the next one wins
    active[best] = 0
    assert pool.price()[0].tolist() == ref.winners(d, active, 1, 1e-7)[0].tolist() != [best]
    assert bits(pool.reduced_costs()) == bits(d)           # reduced costs cover inactive columns too
    pool.set_active([best], True)
    assert pool.price()[0].tolist() == [best] and pool.stats()[3] == 7
    pool.close()
    a.close()
    c.close()


# ---- the add -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_add", [False, True])
@pytest.mark.parametrize("update_block", BLOCKS)
@pytest.mark.parametrize("m,n,seed,k", LPS)
def test_add_and_twin(m, n, seed, k, update_block, host_add, monkeypatch):
    if host_add:
        monkeypatch.setenv("RELP_POOL_HOST_ADD", "1")
    else:
        monkeypatch.delenv("RELP_POOL_HOST_ADD", raising=False)
    A_new, cost, a = solved(m, n, seed, k, update_block)
    monkeypatch.delenv("RELP_POOL_HOST_ADD", raising=False)
    _, _, c = solved(m, n, seed, k, update_block)
    pool = a.pool(A_new, cost)
    first = [k - 1, 2, 9, 0] + ([64, 65] if k > 65 else [])      # descending, the empty column, both slices
    second = [5, 1, 12]
    for round_, ids in enumerate((first, second)):
        # the second add runs after pivots on the widened tableau: added columns before it, rows pending with block 64
        before = a.nr_columns()
        pool.add(ids)
        c.add_columns(A_new[:, ids], cost[ids])
        assert getters(a) == getters(c)
        for j in range(before, before + len(ids)):
            assert a.generate_column(j).tobytes() == c.generate_column(j).tobytes()
        assert a.generate_column(0).tobytes() == c.generate_column(0).tobytes()
        flags = np.ones(k, dtype=np.uint8)
        flags[first if round_ == 0 else first + second] = 0
        d = pool.reduced_costs()
        assert pool.price(k, 0.0)[0].tolist() == ref.winners(d, flags, k, 0.0)[0].tolist()      # the added columns' flags are cleared
        ra, rc = a.run(1 << 20), c.run(1 << 20)
        assert ra == rc and ra[1] == engine.OPTIMAL
        assert getters(a) == getters(c)                     # trace against trace, and every other getter
    assert a.column_stats()[0] == len(first) + len(second)
    # a column taken out again is re-activated by the caller
    out = [j for j in range(n + m, a.nr_columns()) if j not in set(a.basis_indices().tolist())][:1]
    if out:
        a.remove_columns(out)
        pool.set_active([(first + second)[out[0] - n - m]], True)
    pool.close()
    a.close()
    c.close()


# ---- read-only ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_block", BLOCKS)
def test_price_and_reduced_costs_are_read_only(update_block):
    m, n, seed, k = LPS[0]
    A_new, cost, a = solved(m, n, seed, k, update_block)
    pool = a.pool(A_new, cost)
    before = getters(a)
    column = a.generate_column(3).tobytes()
    d = pool.reduced_costs()
    pool.price(4, 1e-7)
    assert getters(a) == before and a.generate_column(3).tobytes() == column
    a.trial_begin()
    inside = getters(a)
    assert bits(pool.reduced_costs()) == bits(d)
    assert pool.price(4, 1e-7)[0].tolist() == ref.winners(d, np.ones(k), 4, 1e-7)[0].tolist()
    assert getters(a) == inside
    assert status_of(lambda: pool.add([0])) == E_STATE      # inside a trial
    assert getters(a) == inside
    a.trial_end(keep=False)
    assert dict(getters(a), stats=None) == dict(before, stats=None)     # (relp_trial_stats moved)
    pool.add([0])                                           # and outside it the add goes through
    assert a.column_stats()[0] == 1
    pool.close()
    a.close()


# ---- the stale rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_block", BLOCKS)
def test_cut_rows_and_the_stale_rule(update_block):
    m, n, seed, k = LPS[0]
    A_new, cost, a = solved(m, n, seed, k, update_block)
    _, _, c = solved(m, n, seed, k, update_block)
    pool = a.pool(A_new, cost)
    # a loose cut x_0 + x_1 <= 1e6: its slack is basic, so it can be taken out again
    G, rhs = np.zeros((1, n)), np.array([1e6])
    G[0, :2] = 1.0
    a.add_cuts(G, rhs)
    c.add_cuts(G, rhs)
    assert a.nr_rows() == m + 1
    # the twin's pool is created after the cut, with explicit zeros in the cut row
    cols, rows = np.nonzero(A_new.T)
    ptr, idx, val = [0], [], []
    for j in range(k):
        r = rows[cols == j]
        idx += r.tolist() + [m]
        val += A_new[r, j].tolist() + [0.0]
        ptr.append(len(idx))
    twin_pool = c.pool((ptr, idx, val), cost)
    assert twin_pool.stats()[:2] == pool.stats()[:2]        # the explicit zeros are dropped
    d = pool.reduced_costs()
    assert bits(d) == bits(twin_pool.reduced_costs())
    assert bits(d) == bits(ref.reduced_costs(A_new, cost, a.minus_pi()[:m]))
    late = a.pool(np.vstack([A_new, np.ones((1, k))]), cost)   # a pool of `a` over the cut row as well
    assert late.reduced_costs().shape == (k,)
    a.remove_cuts([m])                                      # removes a row at rows_at_create of `pool`, below that of `late`
    assert a.nr_rows() == m
    assert bits(pool.reduced_costs()) == bits(ref.reduced_costs(A_new, cost, a.minus_pi()))
    assert pool.price(3, 1e-7)[0].shape[0] >= 1
    before = getters(a)
    for call in (late.reduced_costs, late.price, lambda: late.add([0])):
        assert status_of(call) == E_STATE
    assert "stale" in a._lib.relp_last_error(a._h).decode()
    assert getters(a) == before and late.stats()[3] == 0
    late.set_active([0], False)                             # the flags of a stale pool can still be set
    pool.add([0, 1])                                        # the valid pool still adds
    assert a.column_stats()[0] == 2
    for p in (late, pool, twin_pool):
        p.close()
    a.close()
    c.close()


@pytest.mark.parametrize("update_block", BLOCKS)
def test_a_pool_created_inside_a_trial_over_a_cut_row_is_stale_after_the_rollback(update_block):
    m, n, seed, k = LPS[0]
    A_new, cost, a = solved(m, n, seed, k, update_block)
    a.reserve_cuts(4)                                       # (a cut inside a trial needs its room beforehand)
    old = a.pool(A_new, cost)
    d_old = old.reduced_costs()
    outside = getters(a)
    a.trial_begin()
    early = a.pool(A_new, cost)                             # created inside the trial, before its cut: over the old rows
    G, rhs = np.zeros((1, n)), np.array([1e6])
    G[0, :2] = 1.0
    a.add_cuts(G, rhs)
    assert a.nr_rows() == m + 1
    inside = a.pool(np.vstack([A_new, np.ones((1, k))]), cost)      # every column has an entry in the cut row
    assert inside.reduced_costs().shape == (k,) and inside.price(3, 1e-7)[0].shape[0] >= 1
    inside.set_active([1], False)
    a.trial_end(keep=False)
    assert a.nr_rows() == m and bits(old.reduced_costs()) == bits(d_old)
    before = getters(a)
    assert dict(before, stats=None) == dict(outside, stats=None)
    for call in (inside.reduced_costs, inside.price, lambda: inside.add([0])):
        assert status_of(call) == E_STATE
    assert "stale" in a._lib.relp_last_error(a._h).decode() and "trial" in a._lib.relp_last_error(a._h).decode()
    assert getters(a) == before and inside.stats() == (k, int(np.count_nonzero(A_new)) + k, inside.stats()[2], 1)
    a.add_cuts(G, rhs)                                      # another cut in the place of the one that went: the pool stays stale
    assert a.nr_rows() == m + 1 and status_of(inside.reduced_costs) == E_STATE
    a.remove_cuts([m])
    for pool in (old, early):                               # pools over the old rows are as valid as ever
        assert bits(pool.reduced_costs()) == bits(ref.reduced_costs(A_new, cost, a.minus_pi()))
    early.add([0, 1])
    assert a.column_stats()[0] == 2
    # a trial that is kept takes no row back: a pool created inside it stays valid
    a.trial_begin()
    a.add_cuts(G, rhs)
    kept = a.pool(np.vstack([A_new, np.ones((1, k))]), cost)
    a.trial_end(keep=True)
    assert a.nr_rows() == m + 1 and kept.reduced_costs().shape == (k,)
    a.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_written():
    m, n, seed, k = LPS[0]
    A_new, cost, a = solved(m, n, seed, k, 64)
    pool = a.pool(A_new, cost)
    lib, h, p = a._lib, a._h, pool._p
    before, d, stats = getters(a), pool.reduced_costs(), pool.stats()
    ids, dw, found = np.full(k + 2, -77, dtype=np.int32), np.full(k + 2, -77.0), C.c_int32(-77)

    def price(segments, tol, ids_ptr=ids.ctypes.data, d_ptr=dw.ctypes.data, found_ref=C.byref(found)):
        return lib.relp_pool_price(h, p, segments, tol, ids_ptr, d_ptr, found_ref)

    for segments, tol in ((0, 0.0), (-1, 0.0), (k + 1, 0.0), (1, -1e-9), (1, float("nan")), (1, float("inf"))):
        assert price(segments, tol) == E_ARG
    assert price(1, 0.0, ids_ptr=None) == E_ARG and price(1, 0.0, d_ptr=None) == E_ARG and price(1, 0.0, found_ref=None) == E_ARG
    assert (ids == -77).all() and (dw == -77.0).all() and found.value == -77
    assert lib.relp_pool_reduced_costs(h, p, None) == E_ARG

    def call(fn, listed, *more):
        arr = np.asarray(listed, dtype=np.int32)
        return fn(h, p, arr.ctypes.data, arr.shape[0], *more)

    for listed in ([3, 3], [k], [-1], [0, k + 5]):
        assert call(lib.relp_pool_add, listed) == E_ARG
        assert call(lib.relp_pool_set_active, listed, 0) == E_ARG
    assert call(lib.relp_pool_set_active, [1], 2) == E_ARG and call(lib.relp_pool_set_active, [1], -1) == E_ARG
    assert lib.relp_pool_add(h, p, None, 2) == E_ARG and lib.relp_pool_add(h, p, None, -1) == E_ARG
    assert lib.relp_pool_add(h, p, None, 0) == 0            # count == 0: a no-op
    assert lib.relp_pool_add(h, C.c_void_p(12345), None, 0) == E_ARG and lib.relp_pool_destroy(h, None) == E_ARG      # not a pool of this handle
    bad = np.array([0.0, float("nan")])
    for ptr, idx, val, cst in (([0, 2], [0, 0], [1.0, 2.0], [1.0]), ([0, 1], [m], [1.0], [1.0]), ([1, 1], [0], [1.0], [1.0]),
                               ([0, 2], [0, 1], bad, [1.0]), ([0, 1], [0], [1.0], [float("inf")])):
        assert status_of(lambda: a.pool((ptr, idx, val), cst)) == E_ARG
        assert "relp_pool_create" in a._lib.relp_last_error(a._h).decode()
    out = C.c_void_p(99)
    assert lib.relp_pool_create(h, -1, None, None, None, None, C.byref(out)) == E_ARG and not out.value
    assert getters(a) == before and pool.stats() == stats and bits(pool.reduced_costs()) == bits(d)
    assert pool.price(k, 0.0)[0].tolist() == ref.winners(d, np.ones(k), k, 0.0)[0].tolist()      # every flag is still 1
    empty = a.pool(np.zeros((m, 0)), np.zeros(0))           # a pool without columns finds nothing
    assert empty.price(3, 0.0)[0].shape == (0,) and empty.stats() == (0, 0, 0, 1) and empty.reduced_costs().shape == (0,)
    a.close()                                               # the handle frees the pools that are still alive


def test_other_engines_and_phase_one_refuse():
    lp = dense_lp(24, 49, 1)
    md = colref.narrow(lp, 32)
    t = engine.Tableau(md, engine=engine.ENGINE_REVISED)
    assert status_of(lambda: t.pool(np.ones((24, 1)), [1.0])) == -6
    t.close()
    ge = MatrixData(nr_normal=2, nr_eq=0, nr_range=0, nr_le=0, nr_ge=2, b=np.array([1.0, 1.0]), cost=np.ones(2), upper_bound=np.full(2, np.inf),
                    dense=np.asfortranarray(np.eye(2)))
    t = engine.Tableau(ge, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    assert status_of(lambda: t.pool(np.ones((2, 1)), [1.0])) == E_STATE
    t.close()


# ---- column generation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_block", BLOCKS)
@pytest.mark.parametrize("segments", [1, 4])
def test_column_generation_on_the_cutting_stock_instance(segments, update_block):
    first, patterns = ref.initial_patterns(), ref.maximal_patterns()
    md = MatrixData(nr_normal=len(first), nr_eq=0, nr_range=0, nr_le=0, nr_ge=len(ref.WIDTHS), b=np.array(ref.DEMAND, dtype=np.float64),
                    cost=np.ones(len(first)), upper_bound=np.full(len(first), np.inf), dense=np.asfortranarray(ref.block(first)))
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, update_block=update_block)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2 and t.nr_rows() == len(ref.WIDTHS)
    pool = t.pool(ref.block(patterns), np.ones(len(patterns)))
    rounds, added, outcome = engine.column_generation(t, pool, segments=segments, tol=1e-7, max_rounds=ref.round_cap(segments))
    objective, optimum = t.objective_function_value(), float(ref.FULL_OPTIMUM)
    print(f"segments {segments}, block {update_block}: {rounds} rounds, {added} of {len(patterns)} columns, objective {objective!r}, "
          f"optimum {optimum!r}, difference {abs(objective - optimum):.3e}")
    assert outcome == engine.OPTIMAL and 1 <= rounds <= ref.round_cap(segments)
    assert abs(objective - optimum) <= OBJ_TOL
    assert added < len(patterns) and t.column_stats()[0] == added
    assert pool.price(len(patterns), 1e-7)[0].shape == (0,)
    pool.close()
    t.close()
