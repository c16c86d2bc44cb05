"""relp_change_cost / relp_set_cost / relp_get_cost / relp_cost_stats of the tableau engine: cost coefficients moved on the current
basis without a flush or a re-tabulation, through the ctypes binding, against relp_set_cost (flush + reprice of the same handle
state), a twin handle created with the new costs and warm-started by relp_from_basis on the same basis (only code that existed
before these calls), the numpy solve of tests/cost_reference.py and the committed f64 oracle's fresh two-phase optimum.

LPs: `MatrixData.from_dense_le(**synthetic.dense_lp(m, n, seed))` at (24, 32, 1), (40, 300, 4: more than 256 stored columns), (300, 40,
5: more than 256 rows) and (257, 8, 2), with poll_interval = 1 and update_block 3 (a flush every third enqueued iteration) and -1 (64:
the block stays open, the change reads T0 + W R0).  Tolerances: the project's 1e-9 relative on objectives (OBJ_RTOL) and
1e-9 * max(1, max|d|) between the d (and the -pi) of the in-place change, of relp_set_cost, of the twin and of numpy.

The bases are known on the CPU: the engine walks the committed oracle's pivots one for one on these inputs (asserted), so the lists
are checked there to hold both basic and non-basic columns.  The pending rows p that relp_cost_stats reports are the DISTINCT pivot
rows since the last flush, computed here from the trace: the host counts the iterations it ENQUEUES towards the next flush, and a
loop that polls after every iteration enqueues exactly one no-op iteration after the last pivot (tests/test_gpu_rhs_in_place.py)."""
import functools
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic
from oracle import relp_f64

import cost_reference as cr
import ranging_reference as rr

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-9
TOL_COST = 1e-7
E_ARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
SHAPES = [(24, 32, 1), (40, 300, 4), (300, 40, 5), (257, 8, 2)]
PRIMAL_PIVOTS = {(24, 32, 1): 18, (40, 300, 4): 49, (300, 40, 5): 43, (257, 8, 2): 8}
# basic columns among every third structural column at the optimum (the oracle's basis, counted on the CPU)
BASIC_OF_EVERY_THIRD = {(24, 32, 1): 1, (40, 300, 4): 9, (300, 40, 5): 6, (257, 8, 2): 2}
# primal pivots of the re-solve after every third cost moved, and of the four chained changes on (40, 300, 4) at update_block 3, as
# seen on the MI355X (the textbook simplex on the CPU, cost_reference.primal_pivots, by which the costs were chosen, needs the same
# numbers: every re-solve of the chain passes the reprice that follows the eighth flush, 24 pivots)
RESOLVE_PIVOTS = {(24, 32, 1): 9, (40, 300, 4): 28, (300, 40, 5): 39, (257, 8, 2): 5}
CHAIN_PIVOTS = [28, 48, 71, 70]


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    """A, b, c of the dense <= LP (computed once, read only: every test copies what it changes)."""
    lp = synthetic.dense_lp(m, n, seed)
    for v in lp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lp


def le_md(lp, cost, b=None):
    return MatrixData.from_dense_le(lp["A"], np.array(lp["b"] if b is None else b, dtype=np.float64), np.array(cost, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def oracle_solution(m, n, seed, cost_bytes=None, b_bytes=None):
    """(objective, basis) of the f64 oracle's fresh two-phase solve."""
    lp = dense_lp(m, n, seed)
    cost = lp["c"] if cost_bytes is None else np.frombuffer(cost_bytes)
    oracle = relp_f64.OracleF64(le_md(lp, cost, None if b_bytes is None else np.frombuffer(b_bytes)).ensure_csc())
    assert oracle.run() == "optimal"
    return oracle.objective, tuple(int(j) for j in oracle.basis())


def status_of(err):
    return int(re.search(r"\((-?\d+)\)", str(err.value)).group(1))


def close_to(value, expected):
    return abs(value - expected) <= OBJ_RTOL * max(1.0, abs(expected))


def d_bound(d):
    return 1e-9 * max(1.0, float(np.abs(d).max()))


def solved(m, n, seed, **config):
    lp = dense_lp(m, n, seed)
    t = engine.Tableau(le_md(lp, lp["c"]), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    assert t.iterations() == PRIMAL_PIVOTS[(m, n, seed)]
    assert tuple(t.basis_indices().tolist()) == oracle_solution(m, n, seed)[1]
    return lp, t


def twin_of(lp, cost, basis, b=None, **config):
    """A handle created with `cost` and warm-started on `basis`: a re-tabulation, no code of the in-place change."""
    t = engine.Tableau(le_md(lp, cost, b), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    t.from_basis(basis)
    return t


def pending_rows(t):
    """The distinct pivot rows since the last flush, from the trace of a handle of `solved()` that has only run its primal solve:
    N pivots and one no-op iteration were enqueued, and a flush follows every update_block-th of them."""
    rows = [r for _, _, r, _ in t.trace()]
    flushed = t.update_block() * ((len(rows) + 1) // t.update_block())
    return len(set(rows[flushed:]))


def every_third(lp, key):
    n = lp["A"].shape[1]
    cols = np.arange(0, n, 3)
    c2 = lp["c"].copy()
    c2[cols] = 0.5 * c2[cols] - 0.125
    assert (c2[cols] != lp["c"][cols]).all()
    basis = oracle_solution(*key)[1]
    basic = [j for j in cols if j in basis]
    assert len(basic) == BASIC_OF_EVERY_THIRD[key] and 0 < len(basic) < len(cols)      # both kinds, known on the CPU
    return cols, c2


def check_equal_to_the_rebuilds(m, n, seed, update_block, flush):
    key = (m, n, seed)
    lp, a = solved(m, n, seed, update_block=update_block)
    _, s = solved(m, n, seed, update_block=update_block)
    cols, c2 = every_third(lp, key)
    p = pending_rows(a)
    if update_block == 3:
        assert p == {(24, 32, 1): 0, (40, 300, 4): 1, (300, 40, 5): 1, (257, 8, 2): 0}[key]
    else:
        assert 1 <= p <= PRIMAL_PIVOTS[key]                    # no flush has happened: every pivot row is pending
    if flush:
        a.flush()
        p = 0
    basis = a.basis_indices()
    before = dict(d=a.relative_costs(), b=a.b(), trace=len(a.trace()), reinversions=a.reinversions(), flushes=a.flush_stats())
    assert a.cost_stats() == (0, 0, 0, 0) and np.array_equal(a.cost(), lp["c"])
    a.change_cost(cols, c2[cols])
    s.set_cost(c2)
    twin = twin_of(lp, c2, basis, update_block=update_block)
    d_ref, minus_pi_ref, objective_ref = cr.reduced_costs(le_md(lp, lp["c"]), basis, c2)
    assert a.cost_stats() == (1, BASIC_OF_EVERY_THIRD[key], p, 1)
    assert np.array_equal(a.cost(), c2) and np.array_equal(s.cost(), c2)
    d_a = a.relative_costs()
    bound = d_bound(d_ref)
    for name, other in (("set_cost", s), ("twin", twin)):
        print(f"{key} block {update_block} p {p}: max|d - d_{name}| = {np.abs(d_a - other.relative_costs()).max():.3e}, "
              f"max|pi - pi_{name}| = {np.abs(a.minus_pi() - other.minus_pi()).max():.3e}, bound {bound:.3e}")
        assert np.abs(d_a - other.relative_costs()).max() <= bound
        assert np.abs(a.minus_pi() - other.minus_pi()).max() <= bound
        assert close_to(a.objective_function_value(), other.objective_function_value())
    print(f"   against numpy: d {np.abs(d_a - d_ref).max():.3e}, pi {np.abs(a.minus_pi() - minus_pi_ref).max():.3e}")
    assert np.abs(d_a - d_ref).max() <= bound
    assert np.abs(a.minus_pi() - minus_pi_ref).max() <= bound
    assert close_to(a.objective_function_value(), objective_ref)
    assert d_a[basis].tobytes() == before["d"][basis].tobytes()                # the columns flagged basic keep their d
    assert a.b().tobytes() == before["b"].tobytes() and a.basis_indices().tolist() == basis.tolist()
    assert len(a.trace()) == before["trace"] and a.reinversions() == before["reinversions"] and a.flush_stats() == before["flushes"]
    assert s.reinversions() == before["reinversions"]                          # set_cost: a reprice, no re-tabulation
    for t in (a, s, twin):
        t.close()


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_equal_to_the_rebuilds(m, n, seed, update_block):
    check_equal_to_the_rebuilds(m, n, seed, update_block, flush=False)


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_equal_to_the_rebuilds_after_a_flush(m, n, seed):
    check_equal_to_the_rebuilds(m, n, seed, -1, flush=True)


def test_an_open_block_over_the_split_path(monkeypatch):
    """(300, 40, 5) with the block open: six basic entries in two shares, the pending rows' term in share 0 only."""
    monkeypatch.setenv("RELP_TAB_COST_SPLITS", "2")
    key = (300, 40, 5)
    lp, a = solved(*key)
    cols, c2 = every_third(lp, key)
    basis, p = a.basis_indices(), pending_rows(a)
    assert p >= 1
    a.change_cost(cols, c2[cols])
    assert a.cost_stats() == (1, 6, p, 2)
    d_ref, minus_pi_ref, _ = cr.reduced_costs(le_md(lp, lp["c"]), basis, c2)
    print(f"max|d - d_numpy| = {np.abs(a.relative_costs() - d_ref).max():.3e}, bound {d_bound(d_ref):.3e}")
    assert np.abs(a.relative_costs() - d_ref).max() <= d_bound(d_ref)
    assert np.abs(a.minus_pi() - minus_pi_ref).max() <= d_bound(d_ref)
    a.close()


def resolve_and_compare(lp, key, t, cost, pins, step, **config):
    """`cost` is in effect on `t`: run() to the optimum, against the oracle's fresh solve and the twin's run from the same basis."""
    basis, done_before = t.basis_indices(), t.iterations()
    twin = twin_of(lp, cost, basis, **config)
    pivots, outcome = t.run(1 << 20)
    assert outcome == engine.OPTIMAL
    optimum = oracle_solution(*key, cost_bytes=np.asarray(cost).tobytes())[0]
    print(f"step {step}: {pivots} pivots, objective {t.objective_function_value():.12f}, oracle {optimum:.12f}")
    assert close_to(t.objective_function_value(), optimum)
    assert twin.run(1 << 20) == (pivots, engine.OPTIMAL)
    assert t.trace()[done_before:] == twin.trace()
    assert pivots == pins[step]
    twin.close()
    return pivots


@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_resolve_after_a_change(m, n, seed):
    key = (m, n, seed)
    lp, t = solved(m, n, seed)
    cols, c2 = every_third(lp, key)
    t.change_cost(cols, c2[cols])
    resolve_and_compare(lp, key, t, c2, RESOLVE_PIVOTS, key)
    assert t.reinversions() == 0
    t.close()


def chain_costs(c):
    """The four cost vectors of the chain, each built on the one before."""
    c1 = c.copy()
    c1[::3] = 0.5 * c1[::3] - 0.125
    c2 = c1.copy()
    c2[7] *= 4.0
    c3 = np.array(c[::-1])
    c4 = c3.copy()
    c4[1::2] *= 0.25
    return [c1, c2, c3, c4]


def test_chained_resolves_pass_a_reprice():
    key = (40, 300, 4)
    lp, t = solved(*key, update_block=3)
    current = lp["c"].copy()
    pivots = []
    for step, cost in enumerate(chain_costs(lp["c"])):
        cols = np.flatnonzero(cost != current)
        assert len(cols) == [100, 1, 300, 150][step]
        t.change_cost(cols, cost[cols])
        assert np.array_equal(t.cost(), cost)
        pivots.append(resolve_and_compare(lp, key, t, cost, CHAIN_PIVOTS, step, update_block=3))
        current = cost
    assert max(pivots) >= 3 * 8 + 3                            # a reprice (every 8 flushes of 3 pivots) fell inside a re-solve
    assert t.cost_stats()[0] == 4 and t.reinversions() == 0
    t.close()


@functools.lru_cache(maxsize=None)
def ranging_case(direction):
    """On (24, 32, 1): (column j, row r, Pick, delta) for the first basic structural column whose `direction` ratio is finite with a
    tie band of one and a clear gap; delta = the move halfway from the ratio to its runner-up (at most ratio + 0.5), after which
    exactly one non-basic column is negative beyond tol_cost -- asserted here, in numpy."""
    key = (24, 32, 1)
    lp, basis = dense_lp(*key), oracle_solution(*key)[1]
    n = lp["A"].shape[1]
    T, _, d, in_basis = rr.tableau(le_md(lp, lp["c"]), basis)
    side = 0 if direction == "down" else 1
    for r, j in enumerate(basis):
        if j >= n:
            continue
        pick = rr.row_ratios(T, d, in_basis, [r])[0][side]
        if not np.isfinite(pick.ratio) or pick.band != 1 or pick.gap < 1e-3:
            continue
        delta = pick.ratio + min(0.5 * (pick.runner_up - pick.ratio), 0.5)
        d_new = d + (delta if direction == "down" else -delta) * T[r]
        negative = np.flatnonzero(~in_basis & (d_new < -TOL_COST))
        if negative.tolist() == [pick.index]:
            return j, r, pick, delta
    raise AssertionError("no basic column with a clear range end")


@pytest.mark.parametrize("direction", ["up", "down"])
def test_ranging_meets_change(direction):
    key = (24, 32, 1)
    j, r, pick, delta = ranging_case(direction)
    sign = 1.0 if direction == "up" else -1.0
    lp, t = solved(*key)
    assert t.basis_indices()[r] == j
    dec, inc = t.cost_ranging([j])
    reach = float(inc[0] if direction == "up" else dec[0])
    assert abs(reach - pick.ratio) <= 1e-9 * max(1.0, pick.ratio)
    down_ratio, down_column, up_ratio, up_column = t.row_ratios([r])
    assert int((up_column if direction == "up" else down_column)[0]) == pick.index
    c_j = float(lp["c"][j])
    t.change_cost([j], [c_j + sign * reach / 2])
    assert t.run(1 << 20) == (0, engine.OPTIMAL)               # inside the range: the basis stays optimal
    t.change_cost([j], [c_j + sign * delta])
    d = t.relative_costs()
    nonbasic = np.ones(len(d), dtype=bool)
    nonbasic[t.basis_indices()] = False
    assert np.flatnonzero(nonbasic & (d < -TOL_COST)).tolist() == [pick.index]
    done_before = t.iterations()
    assert t.run(1)[0] == 1
    assert t.trace()[done_before][1] == pick.index             # the first pivot enters the column ranging named
    assert t.run(1 << 20)[1] == engine.OPTIMAL
    c2 = lp["c"].copy()
    c2[j] = c_j + sign * delta
    assert close_to(t.objective_function_value(), oracle_solution(*key, cost_bytes=c2.tobytes())[0])
    t.close()


def test_a_nonbasic_cost_lowered_past_its_reduced_cost():
    key = (24, 32, 1)
    lp, basis = dense_lp(*key), oracle_solution(*key)[1]
    n = lp["A"].shape[1]
    d_ref, _, _ = cr.reduced_costs(le_md(lp, lp["c"]), basis, lp["c"])
    j = next(k for k in range(n) if k not in basis and d_ref[k] > 1e-3)
    lp, t = solved(*key)
    dec, inc = t.cost_ranging([j])
    assert abs(dec[0] - d_ref[j]) <= d_bound(d_ref) and np.isinf(inc[0])
    t.change_cost([j], [lp["c"][j] - dec[0] / 2])
    assert t.run(1 << 20) == (0, engine.OPTIMAL)
    t.change_cost([j], [lp["c"][j] - dec[0] - 1e-3])
    d = t.relative_costs()
    assert abs(d[j] + 1e-3) <= d_bound(d_ref)
    nonbasic = np.ones(len(d), dtype=bool)
    nonbasic[t.basis_indices()] = False
    assert np.flatnonzero(nonbasic & (d < -TOL_COST)).tolist() == [j]
    assert t.cost_stats()[:2] == (2, 0)                        # no tableau row was read
    done_before = t.iterations()
    assert t.run(1)[0] == 1 and t.trace()[done_before][1] == j
    assert t.run(1 << 20)[1] == engine.OPTIMAL
    c2 = lp["c"].copy()
    c2[j] -= dec[0] + 1e-3
    assert close_to(t.objective_function_value(), oracle_solution(*key, cost_bytes=c2.tobytes())[0])
    t.close()


LONG = (300, 300, 8)


@functools.lru_cache(maxsize=None)
def long_case():
    """300 x 300, seed 8: the 300 structural columns as the basis (cond 6.6e3, the best of seeds 1..8: numpy's solve is good to about
    cond * 2^-53 = 1e-12 relative, far inside the bound), every cost changed: 300 basic entries, two LDS chunks of 256."""
    lp = dense_lp(*LONG)
    cond = np.linalg.cond(lp["A"])
    assert cond < 1e4
    n = lp["A"].shape[1]
    c2 = lp["c"] * (0.5 + (np.arange(n) % 7) / 7)
    assert (c2 != lp["c"]).all()
    c2.setflags(write=False)
    basis = np.arange(n, dtype=np.int32)
    return lp, c2, basis, cr.reduced_costs(le_md(lp, lp["c"]), basis, c2)


@pytest.mark.parametrize("forced", [None, 1, 3])
def test_a_long_list_in_shares(forced, monkeypatch):
    if forced:
        monkeypatch.setenv("RELP_TAB_COST_SPLITS", str(forced))
    else:
        monkeypatch.delenv("RELP_TAB_COST_SPLITS", raising=False)
    lp, c2, basis, (d_ref, minus_pi_ref, _) = long_case()
    n = len(c2)
    order = np.random.default_rng(7).permutation(n)
    assert (order != np.arange(n)).any()
    bits = []
    for cols in (np.arange(n), order):
        t = twin_of(lp, lp["c"], basis)
        d_before = t.relative_costs()
        t.change_cost(cols, c2[cols])
        stats = t.cost_stats()
        assert stats[:3] == (1, n, 0)
        assert stats[3] == (forced if forced else 300 // 24)   # the rule: at least 24 entries per share while the grid is small
        d = t.relative_costs()
        print(f"shares {stats[3]}: max|d - d_numpy| = {np.abs(d - d_ref).max():.3e}, bound {d_bound(d_ref):.3e}")
        assert np.abs(d - d_ref).max() <= d_bound(d_ref)
        assert np.abs(t.minus_pi() - minus_pi_ref).max() <= d_bound(d_ref)
        assert d[basis].tobytes() == d_before[basis].tobytes()
        bits.append(d.tobytes())
        t.close()
    assert bits[0] == bits[1]                                  # the caller's order cannot change a bit


def test_later_rebuilds_build_on_the_new_costs():
    key = (24, 32, 1)
    lp, t = solved(*key)
    cols, c2 = every_third(lp, key)
    basis = t.basis_indices()
    t.change_cost(cols, c2[cols])
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    twin = twin_of(lp, c2, basis, b=b2)
    bound = d_bound(twin.relative_costs())
    t.set_right_hand_side(b2)                                  # a re-tabulation
    assert t.reinversions() == 1
    assert np.abs(t.relative_costs() - twin.relative_costs()).max() <= bound
    assert np.abs(t.minus_pi() - twin.minus_pi()).max() <= bound
    assert close_to(t.objective_function_value(), twin.objective_function_value())
    t.from_basis(basis)
    assert t.reinversions() == 2 and np.array_equal(t.cost(), c2)
    assert np.abs(t.relative_costs() - twin.relative_costs()).max() <= bound
    assert close_to(t.objective_function_value(), twin.objective_function_value())
    for h in (t, twin):
        h.close()


def test_the_dual_loop_reads_the_new_reduced_costs():
    """A non-basic cost raised keeps the basis dual feasible; the rhs change and relp_run_dual that follow reach the optimum of the
    LP with the new cost and the new rhs."""
    key = (24, 32, 1)
    lp, t = solved(*key)
    n = lp["A"].shape[1]
    basis = oracle_solution(*key)[1]
    j = next(k for k in range(n) if k not in basis)
    c2 = lp["c"].copy()
    c2[j] += 0.75
    t.change_cost([j], [c2[j]])
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    t.change_right_hand_side(np.arange(0, len(b2), 3), b2[::3])
    pivots, outcome = t.run_dual(1 << 20)
    assert outcome == engine.OPTIMAL and pivots > 0
    assert close_to(t.objective_function_value(), oracle_solution(*key, cost_bytes=c2.tobytes(), b_bytes=b2.tobytes())[0])
    assert t.run(1 << 20) == (0, engine.OPTIMAL)
    t.close()


def test_refused_in_phase_one():
    import dual_reference as dr
    md, _ = dr.covering_lp(24, 32, 1)
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (lambda: t.change_cost([0], [1.0]), lambda: t.set_cost(np.ones(32)), t.cost, t.cost_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    assert t.solve_relaxation() == engine.OPTIMAL
    assert t.cost_stats() == (0, 0, 0, 0)
    t.close()


@pytest.mark.parametrize("kind", [engine.ENGINE_REVISED, engine.ENGINE_LU])
def test_refused_on_the_other_engines(kind):
    lp = dense_lp(24, 32, 1)
    t = engine.Tableau(le_md(lp, lp["c"]), engine=kind)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    objective = t.objective_function_value()
    for call in (lambda: t.change_cost([0], [1.0]), lambda: t.set_cost(np.ones(32)), t.cost, t.cost_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_UNSUPPORTED
    assert t.run(1 << 20) == (0, engine.OPTIMAL) and t.objective_function_value() == objective
    t.close()


def test_argument_errors_change_nothing():
    key = (24, 32, 1)
    m, n, seed = key
    lp, t = solved(*key)
    before = (t.relative_costs(), t.cost(), t.cost_stats(), t.objective_function_value())

    def unchanged():
        return (t.relative_costs().tobytes() == before[0].tobytes() and np.array_equal(t.cost(), before[1])
                and t.cost_stats() == before[2] and t.objective_function_value() == before[3])

    for cols, values in (([0, n], [1.0, 1.0]), ([-1], [1.0]), ([3, 5, 3], [1.0, 2.0, 3.0]), ([0, 1], [1.0, float("nan")]),
                         ([2], [float("inf")])):
        with pytest.raises(engine.RelpError) as err:
            t.change_cost(cols, values)
        assert status_of(err) == E_ARG and unchanged()
    lib = engine.load_library()
    assert lib.relp_change_cost(t.handle, None, None, -1) == E_ARG and unchanged()
    assert lib.relp_change_cost(t.handle, None, None, 2) == E_ARG and unchanged()
    bad = lp["c"].copy()
    bad[5] = float("nan")
    with pytest.raises(engine.RelpError) as err:
        t.set_cost(bad)
    assert status_of(err) == E_ARG and unchanged()
    t.change_cost([], [])                                     # count == 0: a no-op, not counted
    assert unchanged()
    t.change_cost([4, 7], lp["c"][[4, 7]])                    # no entry moves: d keeps its bits, a change that read 0 rows
    assert t.relative_costs().tobytes() == before[0].tobytes() and t.cost_stats() == (1, 0, pending_rows(t), 0)
    # the handle solves on
    cols, c2 = every_third(lp, key)
    t.change_cost(cols, c2[cols])
    assert t.run(1 << 20)[1] == engine.OPTIMAL
    assert close_to(t.objective_function_value(), oracle_solution(*key, cost_bytes=c2.tobytes())[0])
    t.close()
