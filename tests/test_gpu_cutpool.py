"""relp_cutpool_create .. relp_cutpool_stats of the tableau engine through the C ABI: the slacks against the model and against the b
that relp_add_cuts then produces, the read-only contract (also inside a trial), the bit contract of the add against a twin handle
that calls relp_add_cuts with the host data of the same cuts (on both add paths), the room rule inside a trial, the refusals, and
engine.row_generation on the instance of tests/cutpool_reference.py.

LPs: MatrixData.from_dense_le(**synthetic.dense_lp(m, n, seed)) as in tests/test_gpu_cuts_in_place.py at (24, 32, 1) and (40, 300, 4),
solved to the optimum x*.  The pool: 70 cuts (a second slice) with G = default_rng(seed).integers(0, 8, (70, n)); the even cuts dense,
the odd ones sparse (cut k keeps its columns j % 4 == k % 4), cut 2 without entries; beta = 0.9 G x* for k % 3 != 0 (violated at x*)
and 1.1 G x* + 1 else (satisfied).  update_block 3 (a flush every third iteration) and 64 (the block stays open: the calls run with
rows pending).  Two handles made by the same calls hold the same bits (tests/test_gpu_pool.py relies on it too); `a` uses the pool,
`c` is the twin."""
import ctypes as C
import functools

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic

import cutpool_reference as ref

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
LPS = [(24, 32, 1), (40, 300, 4)]
BLOCKS = [3, 64]
K = 70
OBJ_TOL = 1e-9                # the margin tests/test_gpu_pool.py and tests/test_gpu_trial.py use against the exact optimum
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    lp = synthetic.dense_lp(m, n, seed)
    for v in lp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lp


def solved(m, n, seed, update_block):
    lp = dense_lp(m, n, seed)
    md = MatrixData.from_dense_le(lp["A"], np.array(lp["b"]), np.array(lp["c"]))
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, update_block=update_block)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    return t


def vertex_of(t, n):
    return ref.vertex(t.b(), t.basis_indices(), n)


def pool_cuts(n, seed, x):
    """(G, beta) of the docstring at the vertex x."""
    G = np.random.default_rng(seed).integers(0, 8, (K, n)).astype(np.float64)
    k, j = np.indices(G.shape)
    G[(k % 2 == 1) & (j % 4 != k % 4)] = 0.0
    G[2] = 0.0
    gx = G @ x
    beta = np.where(np.arange(K) % 3 != 0, 0.9 * gx, 1.1 * gx + 1.0)
    beta[2] = 1.5
    return G, beta


def getters(t):
    """Everything a caller can read but relp_cutpool_stats, as bytes."""
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


# ---- the slacks and the separation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_block", BLOCKS)
@pytest.mark.parametrize("m,n,seed", LPS)
def test_slacks_separation_and_twin(m, n, seed, update_block):
    a, c = solved(m, n, seed, update_block), solved(m, n, seed, update_block)
    x = vertex_of(a, n)
    G, beta = pool_cuts(n, seed, x)
    pool = a.cut_pool(G, beta)
    nnz = int(np.count_nonzero(G))
    assert pool.stats()[:2] == (K, nnz) and pool.stats()[2] % 64 == 0 and pool.stats()[2] >= nnz and pool.stats()[3] == 0
    s = pool.slacks()
    assert bits(s) == bits(ref.slacks(G, beta, x))                                # the model: fma chains over x as the getters give it
    assert bits(s[2:3]) == bits(beta[2:3])                                        # the cut without entries: s = rhs to the bit
    assert (s < -1e-7).any() and (s > 0).any()
    # against the b of the new rows that relp_add_cuts produces: the same sum in another order (rows ascending, not columns)
    ids = [K - 1, 2, 9, 0, 64, 65, 5, 1, 12]
    c.add_cuts(G[ids], beta[ids])
    b_new = c.b()[m:m + len(ids)]
    for i, k in enumerate(ids):
        L = int(np.count_nonzero(G[k]))
        bound = 2 * L * U * float(np.abs(G[k] * x).sum())
        print(f"cut {k}: slack {s[k]!r}, b_new {b_new[i]!r}, difference {abs(s[k] - b_new[i]):.3e}, bound {bound:.3e}")
        assert abs(s[k] - b_new[i]) <= bound
    # the winners: the model over the device's slacks
    norm, active = ref.norms(G), np.ones(K, dtype=np.uint8)
    for segments, tol, eff in ((1, 1e-7, False), (3, 0.0, True), (K, 1e-7, False), (5, 0.05, True), (K, 0.0, True)):
        got_ids, got_s = pool.separate(segments, tol, eff)
        want_ids, want_s = ref.winners(s, norm, active, segments, tol, eff)
        assert got_ids.tolist() == want_ids.tolist() and bits(got_s) == bits(want_s)
    best = int(pool.separate()[0][0])
    pool.set_active([best], False)                         # the cut that would have won is switched off: the next one wins
    active[best] = 0
    assert pool.separate()[0].tolist() == ref.winners(s, norm, active, 1, 1e-7)[0].tolist() != [best]
    assert bits(pool.slacks()) == bits(s)                  # the slacks cover inactive cuts too
    pool.set_active([best], True)
    assert pool.separate()[0].tolist() == [best] and pool.stats()[3] == 8
    pool.close()
    a.close()
    c.close()


@pytest.mark.parametrize("update_block", BLOCKS)
@pytest.mark.parametrize("m,n,seed", LPS)
def test_slack_equals_b_new_to_the_bit_where_both_orders_coincide(m, n, seed, update_block):
    """A cut over basic structural columns whose rows ascend with the columns, and over non-basic ones (x = +0.0: they leave the
    chain as it is, and relp_add_cuts does not list them): ascending columns and ascending rows are then one order."""
    a, c = solved(m, n, seed, update_block), solved(m, n, seed, update_block)
    basis = a.basis_indices()
    row_of = {int(j): r for r, j in enumerate(basis) if j < n}
    best = {}                                               # the longest run of basic columns, ascending, whose rows ascend too
    for j in sorted(row_of):
        best[j] = max([best[i] for i in best if row_of[i] < row_of[j]], key=len, default=[]) + [j]
    chosen = max(best.values(), key=len)
    nonbasic = [j for j in range(n) if j not in row_of][:3]
    assert len(chosen) >= 2
    rng = np.random.default_rng(seed + 7)
    G = np.zeros((2, n))
    G[0, chosen + nonbasic] = rng.uniform(0.5, 2.0, len(chosen) + len(nonbasic))
    G[1, chosen[:1]] = 3.0                                  # a single entry: trivially one order
    beta = np.array([0.5, -1.0])
    pool = a.cut_pool(G, beta)
    s = pool.slacks()
    c.add_cuts(G, beta)
    assert bits(s) == bits(c.b()[m:m + 2])
    pool.add([0, 1])
    assert bits(a.b()) == bits(c.b())
    a.close()
    c.close()


# ---- read-only ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_block", BLOCKS)
def test_slacks_and_separate_are_read_only(update_block):
    m, n, seed = LPS[0]
    a = solved(m, n, seed, update_block)
    G, beta = pool_cuts(n, seed, vertex_of(a, n))
    pool = a.cut_pool(G, beta)
    before = getters(a)
    column = a.generate_column(3).tobytes()
    s = pool.slacks()
    pool.separate(4, 1e-7, True)
    assert getters(a) == before and a.generate_column(3).tobytes() == column
    a.reserve_cuts(4)
    before = getters(a)
    a.trial_begin()
    inside = getters(a)
    assert bits(pool.slacks()) == bits(s)
    assert pool.separate(4, 1e-7)[0].tolist() == ref.winners(s, ref.norms(G), np.ones(K), 4, 1e-7)[0].tolist()
    assert getters(a) == inside
    a.trial_end(keep=False)
    assert dict(getters(a), stats=None) == dict(before, stats=None)     # (relp_trial_stats moved)
    pool.close()
    a.close()


# ---- the add -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_add", [False, True])
@pytest.mark.parametrize("update_block", BLOCKS)
@pytest.mark.parametrize("m,n,seed", LPS)
def test_add_and_twin(m, n, seed, update_block, host_add, monkeypatch):
    if host_add:
        monkeypatch.setenv("RELP_CUTPOOL_HOST_ADD", "1")
    else:
        monkeypatch.delenv("RELP_CUTPOOL_HOST_ADD", raising=False)
    a = solved(m, n, seed, update_block)
    monkeypatch.delenv("RELP_CUTPOOL_HOST_ADD", raising=False)
    c = solved(m, n, seed, update_block)
    G, beta = pool_cuts(n, seed, vertex_of(a, n))
    pool = a.cut_pool(G, beta)
    first = [K - 1, 2, 9, 0, 64, 65, 7, 1, 13]              # nine cuts (a second tile of k_tab_cut_rows): descending, the cut without entries, both slices
    second = [5, 4, 12, 8, 10, 11, 14, 16, 17, 19, 20, 22]  # 9 + 12 > 16: the tableau grows a second time
    for round_, ids in enumerate((first, second)):
        # the second add runs after dual pivots on the taller tableau: cut rows before it, rows pending with block 64
        rows_before, columns_before = a.nr_rows(), a.nr_columns()
        pool.add(ids)
        c.add_cuts(G[ids], beta[ids])
        assert a.nr_rows() == rows_before + len(ids) and a.nr_columns() == columns_before + len(ids)
        assert getters(a) == getters(c)
        for j in (0, 3, columns_before, columns_before + len(ids) - 1):
            assert a.generate_column(j).tobytes() == c.generate_column(j).tobytes()
        flags = np.ones(K, dtype=np.uint8)
        flags[first if round_ == 0 else first + second] = 0
        s = pool.slacks()
        assert pool.separate(K, 0.0)[0].tolist() == ref.winners(s, ref.norms(G), flags, K, 0.0)[0].tolist()      # the added cuts' flags are cleared
        ra, rc = a.run_dual(1 << 20), c.run_dual(1 << 20)
        assert ra == rc and ra[1] == engine.OPTIMAL and (round_ or ra[0] >= 1)
        assert getters(a) == getters(c)                     # trace against trace, the objective, the basis and every other getter
    assert a.cut_stats()[0] == len(first) + len(second) and a.cut_stats()[1] == c.cut_stats()[1] >= 21
    # a later rebuild includes the cuts on both handles alike
    a.flush()
    c.flush()
    assert getters(a) == getters(c)
    pool.close()
    a.close()
    c.close()


@pytest.mark.parametrize("host_add", [False, True])
@pytest.mark.parametrize("update_block", BLOCKS)
def test_add_inside_a_trial_and_the_rollback(update_block, host_add, monkeypatch):
    m, n, seed = LPS[0]
    if host_add:
        monkeypatch.setenv("RELP_CUTPOOL_HOST_ADD", "1")
    else:
        monkeypatch.delenv("RELP_CUTPOOL_HOST_ADD", raising=False)
    a = solved(m, n, seed, update_block)
    monkeypatch.delenv("RELP_CUTPOOL_HOST_ADD", raising=False)
    c = solved(m, n, seed, update_block)
    G, beta = pool_cuts(n, seed, vertex_of(a, n))
    pool = a.cut_pool(G, beta)
    a.reserve_cuts(4)
    c.reserve_cuts(4)
    parent = getters(a)
    s = pool.slacks()
    ids = [7, 1, 64]
    a.trial_begin()
    c.trial_begin()
    pool.add(ids)                                           # within the reserved room
    c.add_cuts(G[ids], beta[ids])
    assert getters(a) == getters(c) and a.nr_rows() == m + 3
    ra, rc = a.run_dual(1 << 20), c.run_dual(1 << 20)
    assert ra == rc and getters(a) == getters(c)
    inside = getters(a)
    assert status_of(lambda: pool.add([4, 5])) == E_STATE   # 3 + 2 > 4: it would have to grow
    assert "room" in a._lib.relp_last_error(a._h).decode() and "relp_cutpool_add" in a._lib.relp_last_error(a._h).decode()
    assert getters(a) == inside
    a.trial_end(keep=False)
    c.trial_end(keep=False)
    assert dict(getters(a), stats=None) == dict(parent, stats=None) and getters(a) == getters(c)      # the parent to the bit
    assert bits(pool.slacks()) == bits(s)
    flags = np.ones(K, dtype=np.uint8)
    flags[ids] = 0                                          # pools are no part of the snapshot: the flags stay cleared
    assert (s[ids] < 0).all()
    assert pool.separate(K, 0.0)[0].tolist() == ref.winners(s, ref.norms(G), flags, K, 0.0)[0].tolist()
    pool.set_active(ids, True)                              # the caller re-activates them
    assert pool.separate(K, 0.0)[0].tolist() == ref.winners(s, ref.norms(G), np.ones(K), K, 0.0)[0].tolist()
    pool.add(ids)                                           # and outside the trial the add goes through again
    c.add_cuts(G[ids], beta[ids])
    assert getters(a) == getters(c)
    pool.close()
    a.close()
    c.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_written():
    m, n, seed = LPS[0]
    a = solved(m, n, seed, 64)
    G, beta = pool_cuts(n, seed, vertex_of(a, n))
    pool = a.cut_pool(G, beta)
    other = a.cut_pool(G[:3], beta[:3])                     # a handle may hold several
    lib, h, p = a._lib, a._h, pool._p
    before, s, stats = getters(a), pool.slacks(), pool.stats()
    ids, sw, found = np.full(K + 2, -77, dtype=np.int32), np.full(K + 2, -77.0), C.c_int32(-77)

    def separate(segments, tol, eff=0, ids_ptr=ids.ctypes.data, s_ptr=sw.ctypes.data, found_ref=C.byref(found)):
        return lib.relp_cutpool_separate(h, p, segments, tol, eff, ids_ptr, s_ptr, found_ref)

    for segments, tol, eff in ((0, 0.0, 0), (-1, 0.0, 0), (K + 1, 0.0, 0), (1, -1e-9, 0), (1, float("nan"), 0), (1, float("inf"), 0), (1, 0.0, 2),
                               (1, 0.0, -1)):
        assert separate(segments, tol, eff) == E_ARG
    assert separate(1, 0.0, ids_ptr=None) == E_ARG and separate(1, 0.0, s_ptr=None) == E_ARG and separate(1, 0.0, found_ref=None) == E_ARG
    assert (ids == -77).all() and (sw == -77.0).all() and found.value == -77
    assert lib.relp_cutpool_slacks(h, p, None) == E_ARG

    def call(fn, listed, *more):
        arr = np.asarray(listed, dtype=np.int32)
        return fn(h, p, arr.ctypes.data, arr.shape[0], *more)

    for listed in ([3, 3], [K], [-1], [0, K + 5]):
        assert call(lib.relp_cutpool_add, listed) == E_ARG
        assert call(lib.relp_cutpool_set_active, listed, 0) == E_ARG
    assert call(lib.relp_cutpool_set_active, [1], 2) == E_ARG and call(lib.relp_cutpool_set_active, [1], -1) == E_ARG
    assert lib.relp_cutpool_add(h, p, None, 2) == E_ARG and lib.relp_cutpool_add(h, p, None, -1) == E_ARG
    assert lib.relp_cutpool_add(h, p, None, 0) == 0         # count == 0: a no-op
    assert lib.relp_cutpool_add(h, C.c_void_p(12345), None, 0) == E_ARG and lib.relp_cutpool_destroy(h, None) == E_ARG      # not a pool of this handle
    column_pool = a.pool(np.ones((m, 1)), [1.0])            # a column pool is no cut pool
    assert lib.relp_cutpool_slacks(h, column_pool._p, s.ctypes.data) == E_ARG
    bad = np.array([0.0, float("nan")])
    for ptr, idx, val, rhs in (([0, 2], [0, 0], [1.0, 2.0], [1.0]), ([0, 1], [n], [1.0], [1.0]), ([1, 1], [0], [1.0], [1.0]),
                               ([0, 2], [0, 1], bad, [1.0]), ([0, 1], [0], [1.0], [float("inf")])):
        assert status_of(lambda: a.cut_pool((ptr, idx, val), rhs)) == E_ARG
        assert "relp_cutpool_create" in a._lib.relp_last_error(a._h).decode()
    out = C.c_void_p(99)
    assert lib.relp_cutpool_create(h, -1, None, None, None, None, C.byref(out)) == E_ARG and not out.value
    assert getters(a) == before and pool.stats() == stats and bits(pool.slacks()) == bits(s)
    assert pool.separate(K, 0.0)[0].tolist() == ref.winners(s, ref.norms(G), np.ones(K), K, 0.0)[0].tolist()      # every flag is still 1
    assert bits(other.slacks()) == bits(s[:3])
    empty = a.cut_pool(np.zeros((0, n)), np.zeros(0))       # a pool without cuts finds nothing
    assert empty.separate(3, 0.0)[0].shape == (0,) and empty.stats() == (0, 0, 0, 1) and empty.slacks().shape == (0,)
    zeros = a.cut_pool(([0, 2], [0, 1], [0.0, 2.0]), [1.0])  # explicit zeros are dropped
    assert zeros.stats()[:2] == (1, 1)
    a.close()                                               # the handle frees the pools that are still alive


def test_other_engines_and_phase_one_refuse():
    lp = dense_lp(24, 32, 1)
    md = MatrixData.from_dense_le(lp["A"], np.array(lp["b"]), np.array(lp["c"]))
    t = engine.Tableau(md, engine=engine.ENGINE_REVISED)
    assert status_of(lambda: t.cut_pool(np.ones((1, 32)), [1.0])) == E_UNSUPPORTED
    t.close()
    ge = MatrixData(nr_normal=2, nr_eq=0, nr_range=0, nr_le=0, nr_ge=2, b=np.array([1.0, 1.0]), cost=np.ones(2), upper_bound=np.full(2, np.inf),
                    dense=np.asfortranarray(np.eye(2)))
    t = engine.Tableau(ge, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    assert status_of(lambda: t.cut_pool(np.ones((1, 2)), [1.0])) == E_STATE
    t.close()


# ---- row generation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_block", BLOCKS)
@pytest.mark.parametrize("per_round,by_efficacy", sorted(ref.EXACT_ROUNDS))
def test_row_generation_on_the_tangent_planes_of_a_ball(per_round, by_efficacy, update_block):
    G, rhs = ref.instance()
    md = MatrixData.from_dense_le(np.eye(ref.DIM), np.full(ref.DIM, ref.SIDE), np.array(ref.COST))
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, update_block=update_block)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2 and t.nr_rows() == ref.DIM
    assert abs(t.objective_function_value() - sum(ref.COST) * ref.SIDE) <= OBJ_TOL  # the corner of the box
    pool = t.cut_pool(G, rhs)
    cap = ref.round_cap(per_round, by_efficacy)
    rounds, added, objective = engine.row_generation(t, pool, tol=1e-7, per_round=per_round, max_rounds=cap, by_efficacy=by_efficacy)
    optimum = float(ref.FULL_OPTIMUM)
    print(f"per_round {per_round}, by_efficacy {by_efficacy}, block {update_block}: {rounds} rounds (exact: "
          f"{ref.EXACT_ROUNDS[(per_round, by_efficacy)]}, cap {cap}), {added} of {ref.CUTS} cuts, objective {objective!r}, optimum {optimum!r}, "
          f"difference {abs((objective if objective is not None else np.inf) - optimum):.3e}")
    assert objective is not None and 1 <= rounds <= cap
    assert abs(objective - optimum) <= OBJ_TOL
    assert added < ref.CUTS and t.cut_stats()[0] == added
    assert pool.separate(ref.CUTS, 1e-7)[0].shape == (0,)
    pool.close()
    t.close()
