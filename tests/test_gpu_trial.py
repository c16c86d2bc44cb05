"""relp_trial_begin / relp_trial_end / relp_trial_stats / relp_strong_branch of the tableau engine through the C ABI: the bit contract
of the rollback (kernel path and RELP_TRIAL_MEMCPY=1), cuts inside a trial, the room rule of relp_run_dual, the refusals, and
relp_strong_branch against the same steps made by hand on a fresh handle and against the committed f64 oracle on the child LPs.

LPs, helpers and shapes are those of tests/test_gpu_rhs_in_place.py ((24, 32, 1), (40, 300, 4: more than 256 stored columns), (300, 40,
5: more than 256 rows)); the integer programs are INSTANCES of tests/test_gomory_reference.py.  OBJ_RTOL (1e-9 relative) is the
project's bound between two objectives that reach an optimum by different flush schedules; everything else is compared to the bit.

`state(t)` is every getter and every *_stats call of the contract as bytes.  relp_get_basis_inverse flushes the open block (and every
eighth flush reprices d), so it is taken first in the state before a trial and last in the state after it, and a twin that is to
stay bit-equal makes the same calls in the same order; it is refused inside a trial.  The host counts the iterations it ENQUEUES
towards the next flush: a handle of `solved()` (poll_interval = 1) has enqueued its pivots and one no-op iteration, so its
since_flush is (pivots + 1) % update_block while no other flush has happened (`since_flush_of`)."""
import math
import struct

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine
from oracle import relp_f64

import dual_reference as dr
from test_gomory_reference import INSTANCES
from test_gpu_rhs_in_place import E_ARG, E_STATE, E_UNSUPPORTED, OBJ_RTOL, PRIMAL_PIVOTS, close_to, dense_lp, le_lp, pending_rows, solved, status_of

pytestmark = pytest.mark.gpu

SHAPES = [(24, 32, 1), (40, 300, 4), (300, 40, 5)]


def state(t, inverse=None):
    """Every getter of the rollback contract.  inverse: "first" / "last" / None (see the module docstring)."""
    out = {}
    if inverse == "first":
        out["inverse"] = t.basis_inverse().tobytes()
    n = t.nr_columns()
    out.update(b=t.b().tobytes(), d=t.relative_costs().tobytes(), objective=struct.pack("d", t.objective_function_value()),
               minus_pi=t.minus_pi().tobytes(), basis=t.basis_indices().tobytes(), bfs=tuple(t.current_bfs()),
               rhs=t.right_hand_side().tobytes(), cost=t.cost().tobytes(), rows=t.nr_rows(), columns=n, trace=tuple(t.trace()),
               iterations=t.iterations(), degenerate=t.degenerate_pivots(), cut_stats=t.cut_stats(), rhs_stats=t.rhs_stats(),
               cost_stats=t.cost_stats(), ranging_stats=t.ranging_stats(), gomory_stats=t.gomory_stats(), column_stats=t.column_stats(),
               removal_stats=t.removal_stats(), flush_stats=t.flush_stats(), reinversions=t.reinversions(),
               generated=b"".join(t.generate_column(j).tobytes() for j in (0, n // 2, n - 1)))
    if inverse == "last":
        out["inverse"] = t.basis_inverse().tobytes()
    return out


def differing(a, b):
    return sorted(k for k in a if a[k] != b[k])


def since_flush_of(t):
    """since_flush of a handle of `solved()` that has only run its primal solve."""
    pending_rows(t)                                    # (asserts that the no-op iteration completed no block)
    return (t.iterations() + 1) % t.update_block()


def negative_row_change(lp, m):
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    return np.arange(0, m, 3), b2[::3]


# ---- 1. the bit contract of the rollback ------------------------------------------------------------------------------------
@pytest.mark.parametrize("memcpy", [False, True])
@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_rollback_restores_every_getter_to_the_bit(m, n, seed, update_block, memcpy, monkeypatch):
    if memcpy:
        monkeypatch.setenv("RELP_TRIAL_MEMCPY", "1")
    else:
        monkeypatch.delenv("RELP_TRIAL_MEMCPY", raising=False)
    lp, t = solved(m, n, seed, update_block=update_block)
    _, twin = solved(m, n, seed, update_block=update_block)
    before, twin_before = state(t, "first"), state(twin, "first")
    assert not differing(before, twin_before)
    rows, values = negative_row_change(lp, m)
    assert t.trial_stats() == (0, 0, 0, 0)
    t.trial_begin()
    t.change_right_hand_side(rows, values)
    done, outcome = t.run_dual(1 << 20)
    room = t.update_block() - 1                        # (the inverse of the state before flushed: since_flush = 0)
    assert outcome == engine.OPTIMAL or (outcome == engine.RUNNING and done == room)
    assert done >= 1
    t.change_cost([0, n - 1], [lp["c"][0] + 0.25, lp["c"][n - 1] - 0.125])
    inside = state(t)
    assert {"b", "d", "objective", "basis", "rhs", "cost", "trace", "iterations", "rhs_stats", "cost_stats"} <= set(differing(inside, state(twin)))
    t.trial_end(False)
    after, twin_after = state(t, "last"), state(twin, "last")
    print(f"{(m, n, seed)} block {t.update_block()} memcpy {memcpy}: {done} pivots inside, snapshot {t.trial_stats()[2]} bytes")
    assert not differing(after, before), differing(after, before)
    assert not differing(after, twin_after)
    begun, rolled_back, held, left = t.trial_stats()
    assert (begun, rolled_back) == (1, 1) and held > 8 * (m + n) and left == room - done
    # the same change for real, here and on the twin that never opened a trial: the same pivots, the same bits
    for h in (t, twin):
        h.change_right_hand_side(rows, values)
        assert h.run_dual(1 << 20)[1] == engine.OPTIMAL
    end, twin_end = state(t), state(twin)
    assert end["trace"] == twin_end["trace"] and len(end["trace"]) > len(before["trace"])
    assert not differing(end, twin_end), differing(end, twin_end)
    t.close()
    twin.close()


# ---- 2. cuts inside a trial -------------------------------------------------------------------------------------------------
def gomory_cuts_of(t, count):
    G, rhs, _, status = t.gomory_cuts(np.arange(t.nr_rows()))
    made = np.flatnonzero(status == engine.GOMORY_CUT)[:count]
    assert made.size == count
    return G[made], rhs[made]


@pytest.mark.parametrize("count", [1, 9])
def test_cuts_added_inside_a_trial_leave_with_it(count):
    m, n, seed = 24, 32, 1
    _, t = solved(m, n, seed, update_block=-1)
    _, twin = solved(m, n, seed, update_block=-1)
    assert pending_rows(t) >= 1                         # a block is open
    for h in (t, twin):
        h.reserve_cuts(16)
    G, rhs = gomory_cuts_of(t, count)
    G2, rhs2 = gomory_cuts_of(twin, count)
    assert G.tobytes() == G2.tobytes() and rhs.tobytes() == rhs2.tobytes()
    before = state(t)
    assert before["cut_stats"][:2] == (0, 16)
    t.trial_begin()
    t.add_cuts(G, rhs)
    assert (t.nr_rows(), t.nr_columns(), t.cut_stats()[0]) == (before["rows"] + count, before["columns"] + count, count)
    done, outcome = t.run_dual(1 << 20)                 # (to the end, or to the room: either way the same on the twin below)
    assert done >= 1
    if outcome == engine.OPTIMAL:
        assert t.objective_function_value() > struct.unpack("d", before["objective"])[0]
    t.trial_end(False)
    after = state(t)
    assert not differing(after, before), differing(after, before)
    assert not differing(after, state(twin))
    outcomes = []
    for h in (t, twin):
        h.add_cuts(G, rhs)
        outcomes.append(h.run_dual(1 << 20))
    assert outcomes[0] == outcomes[1] and outcomes[0][0] >= done
    end, twin_end = state(t), state(twin)
    assert end["rows"] == before["rows"] + count and not differing(end, twin_end), differing(end, twin_end)
    t.close()
    twin.close()


def test_a_cut_that_would_have_to_grow_is_refused_inside_a_trial():
    _, t = solved(24, 32, 1, update_block=-1)
    G, rhs = gomory_cuts_of(t, 1)
    before = state(t)
    assert before["cut_stats"][1] == 0                  # no room reserved
    t.trial_begin()
    with pytest.raises(engine.RelpError) as err:
        t.add_cuts(G, rhs)
    assert status_of(err) == E_STATE
    assert not differing(state(t), before)
    t.trial_end(False)
    assert not differing(state(t), before)
    t.add_cuts(G, rhs)                                  # outside a trial the add grows as ever
    assert t.cut_stats()[:2] == (1, 16)
    t.close()


# ---- 3. the room rule -------------------------------------------------------------------------------------------------------
def test_run_dual_inside_a_trial_stops_when_the_block_would_fill():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed, update_block=3)
    _, twin = solved(m, n, seed, update_block=3)
    since_flush = since_flush_of(t)
    assert since_flush == (PRIMAL_PIVOTS[(m, n, seed)] + 1) % 3 == 1
    rows, values = negative_row_change(lp, m)
    flushes, reinversions = t.flush_stats(), t.reinversions()
    t.trial_begin()
    t.change_right_hand_side(rows, values)
    done, outcome = t.run_dual(100)
    assert outcome == engine.RUNNING and done == t.update_block() - 1 - since_flush == 1
    assert t.run_dual(100) == (0, engine.RUNNING)       # the room is used up: nothing more happens
    assert t.flush_stats() == flushes and t.reinversions() == reinversions
    t.trial_end(True)
    assert t.trial_stats()[:2] == (1, 0) and t.trial_stats()[3] == 0
    assert t.iterations() == PRIMAL_PIVOTS[(m, n, seed)] + 1             # kept
    assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    assert t.flush_stats()[0] > flushes[0]              # the due flush happened in the loop, as usual
    twin.change_right_hand_side(rows, values)
    assert twin.run_dual(1 << 20)[1] == engine.OPTIMAL
    print(f"objective {t.objective_function_value()!r} after a kept trial, {twin.objective_function_value()!r} on the twin")
    assert close_to(t.objective_function_value(), twin.objective_function_value())
    with pytest.raises(engine.RelpError) as err:
        t.trial_end(True)                               # no trial is open any more
    assert status_of(err) == E_STATE
    t.close()
    twin.close()


def test_no_reinversion_inside_a_trial():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed, update_block=-1)
    rows, values = negative_row_change(lp, m)
    t.set_reinversion_interval(1)
    reinversions = t.reinversions()
    t.trial_begin()
    t.change_right_hand_side(rows, values)
    done, outcome = t.run_dual(1 << 20)
    assert outcome == engine.OPTIMAL and done > 1
    assert t.reinversions() == reinversions
    t.trial_end(True)
    t.change_right_hand_side(rows[:1], values[:1] * 0.5)
    done, _ = t.run_dual(1 << 20)
    assert done == 0 or t.reinversions() > reinversions                   # outside the trial the interval holds again
    t.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_what_flushes_rebuilds_or_reallocates_is_refused_inside_a_trial():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed, update_block=-1)
    t.reserve_cuts(16)
    t.add_cuts(*gomory_cuts_of(t, 1))
    basis = t.basis_indices()
    cut_row = t.nr_rows() - 1
    t.trial_begin()
    before = state(t)
    refused = {
        "flush": t.flush, "set_cost": lambda: t.set_cost(lp["c"]), "set_right_hand_side": lambda: t.set_right_hand_side(t.right_hand_side()),
        "from_basis": lambda: t.from_basis(basis), "remove_cuts": lambda: t.remove_cuts([cut_row]), "remove_columns": lambda: t.remove_columns([0]),
        "reserve_cuts": lambda: t.reserve_cuts(64), "reserve_columns": lambda: t.reserve_columns(4),
        "add_cuts that grows": lambda: t.add_cuts(np.ones((16, n)), np.full(16, 1e6)),
        "add_columns": lambda: t.add_columns(np.ones((t.nr_rows(), 1)), [1.0]), "set_reinversion_interval": lambda: t.set_reinversion_interval(5),
        "run": lambda: t.run(10), "solve_relaxation": t.solve_relaxation, "bring_into_basis": lambda: t.bring_into_basis(0, 0, 0.0),
        "basis_inverse": t.basis_inverse, "trial_begin": t.trial_begin, "strong_branch": lambda: t.strong_branch([0], 1),
    }
    for name, call in refused.items():
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE, name
        assert not differing(state(t), before), name
    assert t.trial_stats()[0] == 1
    t.trial_end(False)
    with pytest.raises(engine.RelpError) as err:
        t.trial_end(False)
    assert status_of(err) == E_STATE
    with pytest.raises(engine.RelpError) as err:
        t._ck(t._lib.relp_trial_end(t._h, 2))
    assert status_of(err) == E_STATE                    # (no trial is open: the state comes before the argument)
    t.flush()                                           # outside a trial everything works again
    t.close()


@pytest.mark.parametrize("kind", [engine.ENGINE_REVISED, engine.ENGINE_LU])
def test_refused_on_the_other_engines(kind):
    lp = dense_lp(24, 32, 1)
    t = engine.Tableau(le_lp(lp, lp["b"]), engine=kind)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    objective = t.objective_function_value()
    for call in (t.trial_begin, t.trial_end, t.trial_stats, lambda: t.strong_branch([0], 1)):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_UNSUPPORTED
    assert t.run(1 << 20) == (0, engine.OPTIMAL) and t.objective_function_value() == objective
    t.close()


def test_refused_in_phase_one():
    md, _ = dr.covering_lp(24, 32, 1)
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (t.trial_begin, t.trial_end, t.trial_stats, lambda: t.strong_branch([0], 1)):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    assert t.solve_relaxation() == engine.OPTIMAL
    assert t.trial_stats() == (0, 0, 0, 0)
    t.close()


# ---- 5. strong_branch against the by-hand path ------------------------------------------------------------------------------
def md_of(inst, extra_row=None, kind=None, rhs=None):
    """The integer program as the engine takes it; with one more <= row (kind "le") or >= row ("ge") for a child LP."""
    A, b = [list(r) for r in inst["A"]], list(inst["b"])
    nr_le, nr_ge = inst["nr_le"], inst["nr_ge"]
    if kind == "le":
        at = inst["nr_eq"] + nr_le
        A.insert(at, list(extra_row)); b.insert(at, rhs); nr_le += 1
    elif kind == "ge":
        A.append(list(extra_row)); b.append(rhs); nr_ge += 1
    upper = np.full(4, np.inf) if inst["upper"] is None else np.array(inst["upper"], dtype=np.float64)
    return MatrixData(nr_normal=4, nr_eq=inst["nr_eq"], nr_range=0, nr_le=nr_le, nr_ge=nr_ge, b=np.array(b, dtype=np.float64),
                      cost=-np.array(inst["c"], dtype=np.float64), upper_bound=upper, dense=np.asfortranarray(np.array(A, dtype=np.float64)))


def open_tableau(md, **config):
    t = engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1, **config)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    return t


def prepare_by_hand(t, max_pivots, since_flush):
    """What relp_strong_branch does before its first trial: the room for one cut as relp_add_cuts would grow it, the one flush."""
    cuts, room = t.cut_stats()[:2]
    if cuts + 1 > room:
        t.reserve_cuts(max(cuts + 1, 2 * room, 16))
    if since_flush + max_pivots + 1 > t.update_block():
        t.flush()


def child_by_hand(t, column, side, b_r, max_pivots, nn):
    """One child on a prepared handle, for real: the cut, the pivots, the objective."""
    g = np.zeros((1, nn))
    g[0, column] = 1.0 if side == 0 else -1.0
    t.add_cuts(g, [math.floor(b_r) if side == 0 else -math.ceil(b_r)])
    done, outcome = t.run_dual(max_pivots)
    return (math.inf if outcome == engine.INFEASIBLE else t.objective_function_value()), outcome, done


def fractional_structural_rows(t, nn, away=1e-6):
    b, basis = t.b(), t.basis_indices()
    f = b - np.floor(b)
    return [i for i in range(b.shape[0]) if 0 <= basis[i] < nn and away <= f[i] <= 1 - away]


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_strong_branch_equals_the_steps_by_hand_and_the_oracle(name):
    inst = INSTANCES[name]
    t = open_tableau(md_of(inst))
    t.flush()                                           # since_flush = 0 from here on, here and on every fresh handle below
    block = t.update_block()
    rows = fractional_structural_rows(t, 4)
    assert rows, "the LP optimum is fractional on every instance"
    b, basis = t.b(), t.basis_indices()
    evaluated = 0
    for max_pivots in (1, 2, block - 1):
        objective, outcome, pivots, status = t.strong_branch(rows, max_pivots)
        assert (status == engine.BRANCH_EVALUATED).all()
        evaluated += len(rows)
        for k, r in enumerate(rows):
            for side in (0, 1):
                fresh = open_tableau(md_of(inst))
                fresh.flush()
                assert fresh.b().tobytes() == b.tobytes() and fresh.basis_indices().tobytes() == basis.tobytes()
                prepare_by_hand(fresh, max_pivots, 0)
                want = child_by_hand(fresh, int(basis[r]), side, b[r], max_pivots, 4)
                fresh.close()
                got = (objective[k, side], outcome[k, side], pivots[k, side])
                assert struct.pack("d", got[0]) == struct.pack("d", want[0]) and got[1:] == want[1:], (name, max_pivots, r, side, got, want)
                if max_pivots == block - 1:
                    bound = math.floor(b[r]) if side == 0 else math.ceil(b[r])
                    unit = [1.0 if c == basis[r] else 0.0 for c in range(4)]
                    oracle = relp_f64.OracleF64(md_of(inst, unit, "le" if side == 0 else "ge", float(bound)).ensure_csc())
                    verdict = oracle.run()
                    print(f"{name} row {r} side {side}: {got}, oracle {verdict} {oracle.objective if verdict == 'optimal' else ''}")
                    assert got[1] in (engine.OPTIMAL, engine.INFEASIBLE)
                    if got[1] == engine.OPTIMAL:
                        assert verdict == "optimal" and close_to(got[0], oracle.objective)
                    else:
                        assert verdict == "infeasible" and got[0] == math.inf
    assert t.trial_stats()[:2] == (2 * evaluated, 2 * evaluated)
    t.close()


@pytest.mark.parametrize("m,n,seed,max_pivots,flushes", [(24, 32, 1, 1, False), (24, 32, 1, 2, True), (40, 300, 4, 1, True)])
def test_strong_branch_with_the_conditional_flush(m, n, seed, max_pivots, flushes):
    lp, t = solved(m, n, seed, update_block=3)
    since_flush = since_flush_of(t)
    assert (since_flush + max_pivots + 1 > 3) == flushes
    rows = fractional_structural_rows(t, n)[:3]
    assert len(rows) == 3
    b, basis = t.b(), t.basis_indices()
    objective, outcome, pivots, _ = t.strong_branch(rows, max_pivots)
    for k, r in enumerate(rows):
        for side in (0, 1):
            _, fresh = solved(m, n, seed, update_block=3)
            prepare_by_hand(fresh, max_pivots, since_flush)
            want = child_by_hand(fresh, int(basis[r]), side, b[r], max_pivots, n)
            fresh.close()
            got = (objective[k, side], outcome[k, side], pivots[k, side])
            assert struct.pack("d", got[0]) == struct.pack("d", want[0]) and got[1:] == want[1:], (r, side, got, want)
    t.close()


def test_the_infeasible_child():
    """max x1 with 2 x1 + 2 x2 <= 3: the optimum is x1 = 1.5 in row 0.  Down (x1 <= 1) is optimal with x1 = 1, up (x1 >= 2) is
    infeasible."""
    t = open_tableau(MatrixData.from_dense_le(np.array([[2.0, 2.0]]), np.array([3.0]), np.array([-1.0, 0.0])))
    assert t.basis_indices().tolist() == [0] and t.b().tolist() == [1.5]
    objective, outcome, pivots, status = t.strong_branch([0], 5)
    assert status.tolist() == [engine.BRANCH_EVALUATED]
    assert outcome.tolist() == [[engine.OPTIMAL, engine.INFEASIBLE]]
    assert objective[0, 0] == -1.0 and objective[0, 1] == math.inf
    assert pivots[0, 0] == 1
    assert t.b().tolist() == [1.5] and t.nr_rows() == 1 and t.objective_function_value() == -1.5
    t.close()


def test_the_running_child():
    m, n, seed = 40, 300, 4
    _, t = solved(m, n, seed, update_block=3)
    since_flush = since_flush_of(t)
    rows = fractional_structural_rows(t, n)
    b, basis = t.b(), t.basis_indices()
    objective, outcome, pivots, _ = t.strong_branch(rows, 1)
    # (RELP_RUNNING says the limit was reached, not that a pivot is left: the children that do need a second pivot are those
    # that make two when allowed two)
    _, _, pivots_of_two, _ = t.strong_branch(rows, 2)
    longer = [(k, side) for k in range(len(rows)) for side in (0, 1) if pivots_of_two[k, side] == 2]
    assert longer, "some child of the (40, 300, 4) optimum needs more than one pivot"
    assert all(outcome[k, side] == engine.RUNNING and pivots[k, side] == 1 for k, side in longer)
    k, side = longer[0]
    assert pivots[k, side] == 1 and math.isfinite(objective[k, side]) and objective[k, side] >= t.objective_function_value()
    _, fresh = solved(m, n, seed, update_block=3)
    prepare_by_hand(fresh, 1, since_flush)
    want = child_by_hand(fresh, int(basis[rows[k]]), side, b[rows[k]], 1, n)
    assert want == (objective[k, side], engine.RUNNING, 1)
    more, end = fresh.run_dual(1 << 20)
    assert more >= 1 and end in (engine.OPTIMAL, engine.INFEASIBLE)       # the twin does need more than one pivot
    if end == engine.OPTIMAL:
        assert fresh.objective_function_value() >= objective[k, side]     # the value after one pivot was a valid bound
    fresh.close()
    t.close()


# ---- 6. strong_branch is read-only ------------------------------------------------------------------------------------------
def test_strong_branch_is_read_only_and_its_arguments_are_checked():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed, update_block=3)
    _, twin = solved(m, n, seed, update_block=3)
    since_flush = since_flush_of(t)
    b, basis = t.b(), t.basis_indices()
    f = b - np.floor(b)
    slack_rows = [i for i in range(m) if basis[i] >= n]
    structural = [i for i in range(m) if basis[i] < n]
    assert slack_rows and len(structural) >= 2
    away = float(np.sort(np.minimum(f, 1 - f)[structural])[len(structural) // 2])       # about half the structural rows are inside
    assert 0 < away < 0.5
    rows = structural + slack_rows[:2] + structural[:1]                                  # any order, a row twice
    want_status = [engine.BRANCH_EVALUATED if away <= f[i] <= 1 - away else engine.BRANCH_FRACTION for i in structural]
    want_status += [engine.BRANCH_NOT_STRUCTURAL] * 2 + want_status[:1]
    assert {0, 1, 2} <= set(want_status)
    before = state(t)
    # refusals first: nothing written, nothing changed
    lib, h = t._lib, t._h
    r32 = np.array(rows, dtype=np.int32)
    k = len(rows)
    obj, oc, piv, st = np.full(2 * k, 7.0), np.full(2 * k, 7, dtype=np.int32), np.full(2 * k, 7, dtype=np.int32), np.full(k, 7, dtype=np.int32)
    raw = lambda rows_p, count, mp, aw, o=obj, c=oc, p=piv, s=st: lib.relp_strong_branch(   # noqa: E731
        h, rows_p, count, mp, aw, None if o is None else o.ctypes.data, None if c is None else c.ctypes.data,
        None if p is None else p.ctypes.data, None if s is None else s.ctypes.data)
    bad_row = np.array([0, m], dtype=np.int32)
    assert raw(bad_row.ctypes.data, 2, 1, away) == E_ARG and raw(np.array([-1], dtype=np.int32).ctypes.data, 1, 1, away) == E_ARG
    assert raw(r32.ctypes.data, -1, 1, away) == E_ARG and raw(None, k, 1, away) == E_ARG
    for missing in range(4):
        args = [obj, oc, piv, st]
        args[missing] = None
        assert raw(r32.ctypes.data, k, 1, away, *args) == E_ARG
    assert raw(r32.ctypes.data, k, 0, away) == E_ARG and raw(r32.ctypes.data, k, t.update_block(), away) == E_ARG
    for bad_away in (-0.1, 0.5, math.nan, math.inf):
        assert raw(r32.ctypes.data, k, 1, bad_away) == E_ARG
    assert (obj == 7.0).all() and (oc == 7).all() and (piv == 7).all() and (st == 7).all()
    assert raw(r32.ctypes.data, 0, 1, away) == 0 and raw(None, 0, 1, away, None, None, None, None) == 0      # count == 0: a no-op
    assert (obj == 7.0).all() and (st == 7).all()
    assert not differing(state(t), before) and t.trial_stats() == (0, 0, 0, 0)
    # the call itself
    objective, outcome, pivots, status = t.strong_branch(rows, 2, away=away)
    assert status.tolist() == want_status
    for x, s in enumerate(want_status):
        if s == engine.BRANCH_EVALUATED:
            assert np.isfinite(objective[x]).any() or (objective[x] == math.inf).all()
            assert set(outcome[x].tolist()) <= {engine.OPTIMAL, engine.INFEASIBLE, engine.RUNNING}
        else:
            assert np.isnan(objective[x]).all() and outcome[x].tolist() == [-1, -1] and pivots[x].tolist() == [0, 0]
    assert objective[0].tobytes() == objective[-1].tobytes()                              # the row named twice: the same bits
    evaluated = want_status.count(engine.BRANCH_EVALUATED)
    assert t.trial_stats()[:2] == (2 * evaluated, 2 * evaluated)
    prepare_by_hand(twin, 2, since_flush)
    after, twin_after = state(t), state(twin)
    assert not differing(after, twin_after), differing(after, twin_after)
    assert after["cut_stats"][:2] == (0, 16) and after["rows"] == m
    # skipped entries alone: neither the room nor the flush
    _, lone = solved(m, n, seed, update_block=3)
    lone_before = state(lone)
    _, _, _, status = lone.strong_branch(slack_rows, 2)
    assert (status == engine.BRANCH_NOT_STRUCTURAL).all() and not differing(state(lone), lone_before)
    # a basis that is not dual feasible is refused like relp_run_dual refuses it
    nonbasic = next(j for j in range(n) if j not in set(basis.tolist()))
    lone.change_cost([nonbasic], [-1e6])
    with pytest.raises(engine.RelpError) as err:
        lone.strong_branch(structural[:1], 1)
    assert status_of(err) == E_STATE and "not dual feasible" in str(err.value)
    for h2 in (t, twin, lone):
        h2.close()
