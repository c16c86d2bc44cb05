"""relp_remove_cuts / relp_remove_columns / relp_removal_stats of the tableau engine through the ctypes binding: cut rows whose slack
is basic and non-basic added columns leave the tableau in place.

The history of a cuts case: `synthetic.dense_lp` at the shapes of tests/test_gpu_cuts_in_place.py solved to the optimum x*; nine cuts
G = default_rng(7000 * seed + cut_seed).integers(0, 8, (9, n)), five of them tight (beta = 0.9 G x*, violated at x*) and four loose
(beta = 1.5 G x* + 1) in a shuffled order; relp_run_dual; relp_change_cost on every other basic structural column (to 0.05 of its
cost: x shrinks and tight cuts come loose) and relp_run, so that slacks re-enter the basis in rows that are not their own.  The cut
seeds (CUT_SEED) were chosen with the committed f64 oracle, which gives the slacks that are basic at the optimum of each stage: a
tight cut whose slack is basic at the end left its own row and came back in the row of a ratio test (per shape the seed among
0 .. 5 with the most such cuts and at least one loose cut whose slack stays basic throughout).  Every test asserts from
basis_indices() that it removes at least one cut whose slack is basic outside its own row and one inside it.

The twin: a second handle goes through the same calls (the same bits: the engine is deterministic) and calls flush() where the first
removes.  Every surviving entry -- generate_column of every surviving column over the surviving rows, d, b, -pi, the objective, the
right-hand side, the costs -- is byte-equal to the twin's under the index maps, and basis_indices equals the twin's with its columns
mapped.  The flags are not readable through the binding: they show in what follows, the pivots of relp_run / relp_run_dual on both.

After a removal: check_basis within the bounds of the cut and column tests, the handle rebuilt by from_basis on its own basis and a
fresh engine on the LP without the removed cuts or columns with from_basis agree to 1e-9 (the project's bound), and relp_run /
relp_run_dual end at the f64 oracle's optimum of the smaller LP (OBJ_RTOL)."""
import functools
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine, synthetic
from oracle import relp_f64

import cut_reference as cutref
import remove_reference as rr

pytestmark = pytest.mark.gpu

OBJ_RTOL = 1e-9
TOL_FEAS = 1e-7
IDENT_TOL = 1e-6              # check_basis: |B^-1 B - I| and |d_B|, the bound of tests/test_gpu_columns_in_place.py
E_ARG, E_STATE, E_UNSUPPORTED = -1, -5, -6
SHAPES = [(24, 32, 1), (40, 300, 4), (300, 40, 5), (257, 8, 2), (255, 8, 3), (250, 12, 6)]
KT, KL = 5, 4
# per shape the seed of the cuts (see the module docstring)
CUT_SEED = {(24, 32, 1): 0, (40, 300, 4): 3, (300, 40, 5): 2, (257, 8, 2): 5, (255, 8, 3): 2, (250, 12, 6): 1}


@functools.lru_cache(maxsize=None)
def dense_lp(m, n, seed):
    lp = synthetic.dense_lp(m, n, seed)
    for v in lp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lp


def le_md(A, b, c):
    return MatrixData.from_dense_le(np.asfortranarray(A), np.array(b, dtype=np.float64), np.array(c, dtype=np.float64))


def status_of(err):
    return int(re.search(r"\((-?\d+)\)", str(err.value)).group(1))


def close_to(value, expected):
    return abs(value - expected) <= OBJ_RTOL * max(1.0, abs(expected))


def near(value, expected, what=""):
    bound = 1e-9 * max(1.0, float(np.abs(expected).max()))
    err = float(np.abs(np.asarray(value) - np.asarray(expected)).max())
    print(f"   {what}: max error {err:.3e}, bound {bound:.3e}")
    return err <= bound


def new_handle(md, **config):
    return engine.Tableau(md, engine=engine.ENGINE_TABLEAU, trace_capacity=8192, poll_interval=1, **config)


def oracle_objective(md):
    oracle = relp_f64.OracleF64(md.ensure_csc())
    assert oracle.run() == "optimal"
    return oracle.objective


# ---- the history of a cuts case, the same calls on every handle ---------------------------------------------------------------
def cut_mix(lp, basis, seed, cut_seed, kt=KT, kl=KL):
    """(G, beta, tight): kt cuts violated at the optimum of `basis` and kl loose ones, shuffled."""
    n = lp["A"].shape[1]
    rng = np.random.default_rng(7000 * seed + cut_seed)
    G = rng.integers(0, 8, (kt + kl, n)).astype(float)
    tight = np.zeros(kt + kl, dtype=bool)
    tight[:kt] = True
    rng.shuffle(tight)
    at_x = G @ cutref.optimum_x(lp, basis)
    return G, np.where(tight, 0.9 * at_x, 1.5 * at_x + 1.0), tight


def cost_move(lp, basis, n):
    """(columns, values): every other basic structural column, ascending, to 0.05 of its cost."""
    cols = np.array(sorted(int(j) for j in basis if j < n)[::2], dtype=np.int32)
    return cols, 0.05 * np.asarray(lp["c"])[cols]


def cuts_history(t, lp, seed, cut_seed):
    """solve, add the cuts, run_dual, move the costs, run.  Returns (G, beta, the costs in effect)."""
    n = lp["A"].shape[1]
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    G, beta, _ = cut_mix(lp, t.basis_indices(), seed, cut_seed)
    t.add_cuts(G, beta)
    assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    cols, values = cost_move(lp, t.basis_indices(), n)
    t.change_cost(cols, values)
    assert t.run(1 << 20)[1] == engine.OPTIMAL
    c2 = np.array(lp["c"])
    c2[cols] = values
    return G, beta, c2


def cut_pair(m, n, seed, **config):
    lp = dense_lp(m, n, seed)
    a, twin = (new_handle(le_md(lp["A"], lp["b"], lp["c"]), **config) for _ in range(2))
    G, beta, c2 = cuts_history(a, lp, seed, CUT_SEED[(m, n, seed)])
    cuts_history(twin, lp, seed, CUT_SEED[(m, n, seed)])
    return lp, a, twin, G, beta, c2


def removable_cuts(t, first_row, first_slack, k):
    """(inside, outside): the cuts c < k whose slack first_slack + c is basic in its own row first_row + c / in another row"""
    where = {int(j): r for r, j in enumerate(t.basis_indices())}
    inside = [c for c in range(k) if where.get(first_slack + c) == first_row + c]
    outside = [c for c in range(k) if first_slack + c in where and where[first_slack + c] != first_row + c]
    return inside, outside


def surviving(a, twin, rows_c, cols):
    """The index sets of a removal on `a` read off the twin, which still has everything: (tableau rows kept, constraints kept,
    columns kept, column map old -> new)."""
    basis = twin.basis_indices()
    where = {int(j): r for r, j in enumerate(basis)}
    rows_t = [where[j] for j in cols if j in where]
    keep_t = np.setdiff1d(np.arange(twin.nr_rows()), rows_t)
    keep_c = np.setdiff1d(np.arange(twin.nr_rows()), rows_c)
    keep_j = np.setdiff1d(np.arange(twin.nr_columns()), cols)
    return keep_t, keep_c, keep_j, rr.index_map(twin.nr_columns(), cols)


def assert_same_bits(a, twin, keep_t, keep_c, keep_j, col_map):
    assert a.nr_rows() == keep_t.size == keep_c.size and a.nr_columns() == keep_j.size
    assert a.relative_costs().tobytes() == twin.relative_costs()[keep_j].tobytes()
    assert a.b().tobytes() == twin.b()[keep_t].tobytes()
    assert a.minus_pi().tobytes() == twin.minus_pi()[keep_c].tobytes()
    assert a.right_hand_side().tobytes() == twin.right_hand_side()[keep_c].tobytes()
    assert a.objective_function_value() == twin.objective_function_value()
    assert a.cost().tobytes() == twin.cost().tobytes()
    assert a.basis_indices().tolist() == col_map[twin.basis_indices()[keep_t]].tolist()
    for new, old in enumerate(keep_j):
        assert a.generate_column(new).tobytes() == twin.generate_column(int(old))[keep_t].tobytes(), f"column {old} -> {new}"
    assert a.trace() == twin.trace() and a.reinversions() == twin.reinversions() and a.retab_stats() == twin.retab_stats()
    assert a.flush_stats() == twin.flush_stats()


def assert_sound(t, md_small, to_fresh=None):
    """check_basis, the rebuild of the handle on its own basis, a fresh engine on the smaller LP (md_small, whose column j of the
    handle is to_fresh[j]; None: no fresh engine), then both loops against the oracle."""
    ident, basic, min_b = t.check_basis()
    print(f"   check_basis: identity {ident:.3e}, basic costs {basic:.3e}, min b {min_b:.3e}")
    assert ident <= IDENT_TOL and basic <= IDENT_TOL and min_b >= -TOL_FEAS
    basis = t.basis_indices()
    state = dict(b=t.b(), d=t.relative_costs(), pi=t.minus_pi(), objective=t.objective_function_value())
    if to_fresh is not None:
        fresh = new_handle(md_small)
        fresh.from_basis(np.asarray(to_fresh)[basis].astype(np.int32))
        assert near(fresh.b(), state["b"], "b against a fresh engine") and near(fresh.relative_costs()[to_fresh], state["d"], "d against a fresh engine")
        assert near(fresh.minus_pi(), state["pi"], "-pi against a fresh engine") and close_to(fresh.objective_function_value(), state["objective"])
        fresh.close()
    t.from_basis(basis)
    assert near(t.b(), state["b"], "b after from_basis") and near(t.relative_costs(), state["d"], "d after from_basis")
    assert near(t.minus_pi(), state["pi"], "-pi after from_basis") and close_to(t.objective_function_value(), state["objective"])
    optimum = oracle_objective(md_small)
    assert t.run(1 << 20)[1] == engine.OPTIMAL and close_to(t.objective_function_value(), optimum)
    assert t.run_dual(1 << 20)[1] == engine.OPTIMAL and close_to(t.objective_function_value(), optimum)
    assert t.check_basis()[2] >= -TOL_FEAS


def le_order(n, m_le, k_struct):
    """to_fresh for a <= LP: handle columns [n | m_le slacks | tail] onto the fresh LP's [n + k_struct structural | slacks]; the caller fills the tail."""
    return np.concatenate([np.arange(n), n + k_struct + np.arange(m_le)])


# ---- cuts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flush_first", [False, True])
@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", SHAPES)
def test_remove_cuts_against_the_twin(m, n, seed, update_block, flush_first):
    k = KT + KL
    lp, a, twin, G, beta, c2 = cut_pair(m, n, seed, update_block=update_block)
    if flush_first:
        a.flush()
        twin.flush()
    inside, outside = removable_cuts(a, m, n + m, k)
    print(f"({m}, {n}, {seed}) block {update_block}: slacks basic in their own row {inside}, in another row {outside}")
    assert inside and outside                                 # both kinds are removed: the test cannot pass vacuously
    gone = sorted(inside + outside, key=lambda c: (c * 7) % k)         # (not ascending)
    rows = [m + c for c in gone]
    flushes, reinversions = a.flush_stats()[0], a.reinversions()
    assert a.removal_stats() == (0, 0, 0, 0)
    a.remove_cuts(rows)
    twin.flush()
    stats = a.removal_stats()
    print(f"   removal_stats {stats}")
    keep_t, keep_c, keep_j, col_map = surviving(a, twin, rows, [n + m + c for c in gone])
    first_t = min(set(range(m + k)) - set(keep_t.tolist()))
    assert stats[:2] == (len(gone), 0) and stats[2] == (m + k - first_t) * (n + m + k) + keep_t.size * (k - min(gone))
    assert a.flush_stats()[0] == flushes + (1 if stats[3] else 0) and (stats[3] == 0 or not flush_first)
    assert stats[3] >= 1 or flush_first or update_block != -1       # (block 64, never flushed: the removal flushes an open block)
    assert a.reinversions() == reinversions and a.cut_stats()[:2] == (k - len(gone), 16)
    assert_same_bits(a, twin, keep_t, keep_c, keep_j, col_map)
    kept = np.setdiff1d(np.arange(k), gone)
    md_small = cutref.stacked(lp, G[kept], beta[kept], cost=c2)
    assert_sound(a, md_small, np.arange(n + m + kept.size))
    a.close()
    twin.close()


@pytest.mark.parametrize("update_block", [3, -1])
def test_remove_all_cuts_and_add_again_in_the_same_room(update_block):
    """Every cut goes once its slack is basic.  The removable ones go first, on two handles (the same calls: the same bits); the
    tight ones that are left are relaxed to a right-hand side they cannot bind at (relp_change_right_hand_side, relp_run_dual,
    relp_run): at an optimum such a cut has a positive slack, which is therefore basic -- asserted from basis_indices.  Then the LP
    is the one before the cuts, and 16 cuts are added into the room of the first 9 without growth."""
    m, n, seed = 24, 32, 1
    k = KT + KL
    lp, a, twin, G, beta, c2 = cut_pair(m, n, seed, update_block=update_block)
    for t in (a, twin):
        inside, outside = removable_cuts(t, m, n + m, k)
        t.remove_cuts([m + c for c in inside + outside])
    assert a.relative_costs().tobytes() == twin.relative_costs().tobytes() and a.b().tobytes() == twin.b().tobytes()
    kept = np.setdiff1d(np.arange(k), inside + outside)
    left = kept.size
    assert a.cut_stats()[:2] == (left, 16) and a.nr_rows() == m + left
    # relax what is left until its slack is basic, then remove it: the tableau of the LP without cuts
    big = 10.0 * float(np.abs(beta).max()) + 100.0
    a.change_right_hand_side(np.arange(m, m + left, dtype=np.int32), np.full(left, big))
    assert a.run_dual(1 << 20)[1] == engine.OPTIMAL and a.run(1 << 20)[1] == engine.OPTIMAL
    inside, outside = removable_cuts(a, m, n + m, left)
    print(f"   after relaxing: {left} cuts left, slacks basic in their own row {inside}, in another row {outside}")
    assert sorted(inside + outside) == list(range(left))      # a cut that cannot bind has its slack basic at an optimum
    a.remove_cuts(np.arange(m, m + left, dtype=np.int32)[::-1])
    assert a.cut_stats()[:2] == (0, 16) and a.nr_rows() == m and a.nr_columns() == n + m and a.removal_stats()[0] == k
    md0 = le_md(lp["A"], lp["b"], c2)
    assert_sound(a, md0, np.arange(n + m))
    # add after remove: the same room, no growth, the indices of a first add
    G2, beta2, _ = cut_mix(lp, a.basis_indices(), seed, 77, kt=3, kl=13)
    a.add_cuts(G2, beta2)
    assert a.cut_stats()[:2] == (16, 16) and a.nr_rows() == m + 16 and a.basis_indices()[m:].tolist() == list(range(n + m, n + m + 16))
    assert a.run_dual(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), oracle_objective(cutref.stacked(lp, G2, beta2, cost=c2)))
    ident, basic, min_b = a.check_basis()
    assert ident <= IDENT_TOL and basic <= IDENT_TOL and min_b >= -TOL_FEAS
    a.close()
    twin.close()


def test_the_neighbouring_calls_on_shifted_indices():
    """rhs change, ranging, row ratios and a cost change after a removal, against the twin that never had the removed cuts: a fresh
    engine on the smaller LP warm-started on the same basis."""
    m, n, seed, k = 40, 300, 4, KT + KL
    lp, a, twin, G, beta, c2 = cut_pair(m, n, seed)
    twin.close()
    inside, outside = removable_cuts(a, m, n + m, k)
    assert inside and outside
    gone = inside[:1] + outside[:1]
    a.remove_cuts([m + c for c in gone])
    kept = np.setdiff1d(np.arange(k), gone)
    other = new_handle(cutref.stacked(lp, G[kept], beta[kept], cost=c2))
    other.from_basis(a.basis_indices())
    rows = np.array([m, m + kept.size - 1, 0], dtype=np.int32)            # cut rows by their new indices
    for name in ("rhs_ranging", "row_ratios"):
        for g, w in zip(getattr(a, name)(rows), getattr(other, name)(rows)):
            if g.dtype == np.int32:
                assert g.tolist() == w.tolist(), name
            else:
                assert np.array_equal(np.isinf(g), np.isinf(w)), name
                finite = ~np.isinf(w)
                assert near(g[finite], w[finite], name) if finite.any() else True
    values = a.right_hand_side()[rows[:2]] * np.array([0.97, 1.05])
    cols = np.arange(1, n, 5)
    for t in (a, other):
        t.change_right_hand_side(rows[:2], values)
    assert near(a.b(), other.b(), "b after the rhs change") and np.array_equal(a.right_hand_side(), other.right_hand_side())
    for t in (a, other):
        assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), other.objective_function_value())
    for t in (a, other):
        t.change_cost(cols, 0.5 * c2[cols])
        assert t.run(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), other.objective_function_value())
    c3 = c2.copy()
    c3[cols] = 0.5 * c2[cols]
    rhs = beta[kept].copy()
    rhs[[0, kept.size - 1]] = values
    assert close_to(a.objective_function_value(), oracle_objective(cutref.stacked(lp, G[kept], rhs, cost=c3)))
    a.close()
    other.close()


# ---- columns ------------------------------------------------------------------------------------------------------------------
def columns_history(t, lp, n, k):
    """solve the LP of the first n columns, add the k columns held back -- the odd ones at cost +1, which never price out (A > 0,
    -pi >= 0) --, run."""
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    A_new = np.array(lp["A"][:, n:])
    cost = np.array(lp["c"][n:])
    cost[1::2] = 1.0
    t.add_columns(A_new, cost)
    assert t.run(1 << 20)[1] == engine.OPTIMAL
    return A_new, cost


@pytest.mark.parametrize("flush_first", [False, True])
@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("m,n,seed", [(24, 32, 1), (40, 300, 4), (300, 40, 5), (255, 8, 3)])
def test_remove_columns_against_the_twin(m, n, seed, update_block, flush_first):
    k = 9
    lp = dense_lp(m, n + k, seed)
    a, twin = (new_handle(le_md(lp["A"][:, :n], lp["b"], lp["c"][:n]), update_block=update_block) for _ in range(2))
    A_new, cost = columns_history(a, lp, n, k)
    columns_history(twin, lp, n, k)
    if flush_first:
        a.flush()
        twin.flush()
    basic = set(int(j) for j in a.basis_indices())
    gone = [c for c in range(k) if n + m + c not in basic]
    print(f"({m}, {n}, {seed}) block {update_block}: added columns basic {sorted(set(range(k)) - set(gone))}, removed {gone}")
    assert set(gone) >= {1, 3, 5, 7}                            # (at an optimum a column at cost +1 has d >= 1: it is not basic)
    cols = [n + m + c for c in gone][::-1]
    flushes = a.flush_stats()[0]
    a.remove_columns(cols)
    twin.flush()
    stats = a.removal_stats()
    keep_t, keep_c, keep_j, col_map = surviving(a, twin, [], cols)
    assert stats[:3] == (0, len(gone), m * (k - min(gone))) and a.flush_stats()[0] == flushes + (1 if stats[3] else 0)
    assert stats[3] == 0 or not flush_first
    assert stats[3] >= 1 or flush_first or update_block != -1       # (block 64, never flushed: the removal flushes an open block)
    print(f"   removal_stats {stats}")
    assert a.column_stats()[:2] == (k - len(gone), 16) and a.cut_stats()[:2] == (0, 0)
    assert_same_bits(a, twin, keep_t, keep_c, keep_j, col_map)
    kept = np.setdiff1d(np.arange(k), gone)
    md_small = le_md(np.hstack([lp["A"][:, :n], A_new[:, kept]]), lp["b"], np.concatenate([lp["c"][:n], cost[kept]]))
    assert_sound(a, md_small, np.concatenate([le_order(n, m, kept.size), n + np.arange(kept.size)]))
    a.close()
    twin.close()


def test_remove_every_added_column_and_add_again_in_the_same_room():
    m, n, seed, k = 24, 32, 1, 9
    lp = dense_lp(m, n + k, seed)
    a = new_handle(le_md(lp["A"][:, :n], lp["b"], lp["c"][:n]))
    plain = new_handle(le_md(lp["A"][:, :n], lp["b"], lp["c"][:n]))
    assert a.solve_relaxation() == engine.OPTIMAL and plain.solve_relaxation() == engine.OPTIMAL
    plain.flush()
    A_new = np.array(lp["A"][:, n:])
    a.add_columns(A_new, np.ones(k))                            # at cost +1 none prices out: all stay non-basic
    assert a.run(1 << 20) == (0, engine.OPTIMAL)
    a.remove_columns(np.arange(n + m, n + m + k))
    assert a.column_stats()[:2] == (0, 16) and a.nr_columns() == n + m and a.removal_stats()[:2] == (0, k)
    # the tableau of the handle that never had them, flushed
    assert a.relative_costs().tobytes() == plain.relative_costs().tobytes() and a.b().tobytes() == plain.b().tobytes()
    assert a.basis_indices().tolist() == plain.basis_indices().tolist() and a.minus_pi().tobytes() == plain.minus_pi().tobytes()
    for j in range(n + m):
        assert a.generate_column(j).tobytes() == plain.generate_column(j).tobytes()
    a.add_columns(A_new, np.array(lp["c"][n:]))                 # the room is there: no growth, the indices of a first add
    assert a.column_stats()[:2] == (k, 16) and a.nr_columns() == n + m + k
    assert a.run(1 << 20)[1] == engine.OPTIMAL
    assert close_to(a.objective_function_value(), oracle_objective(le_md(lp["A"], lp["b"], lp["c"])))
    ident, basic, min_b = a.check_basis()
    assert ident <= IDENT_TOL and basic <= IDENT_TOL and min_b >= -TOL_FEAS
    a.close()
    plain.close()


# ---- cuts and columns interleaved, also with == rows ----------------------------------------------------------------------------
def equality_rows(lp, dup):
    """4 independent == rows and `dup` integer combinations of them (redundant: the phase switch removes `dup` rows) that hold at
    x_f = x* / 2 rounded down to 64ths; the construction of tests/test_gpu_cuts_in_place.py."""
    n = lp["A"].shape[1]
    rng = np.random.default_rng(424242)
    oracle = relp_f64.OracleF64(le_md(lp["A"], lp["b"], lp["c"]).ensure_csc())
    assert oracle.run() == "optimal"
    x_f = np.floor(32.0 * cutref.optimum_x(lp, oracle.basis())) / 64.0
    R = rng.integers(0, 4, (4, n)).astype(float)
    C = rng.integers(0, 3, (dup, 4)).astype(float)
    C[C.sum(axis=1) == 0, 0] = 1.0
    E = np.vstack([R, C @ R])
    return E, E @ x_f


def mixed_md(E, e_rhs, A_le, b_le, cost):
    """== rows E over the first columns (zero on the others), then <= rows."""
    n_all = A_le.shape[1]
    Ew = np.zeros((E.shape[0], n_all))
    Ew[:, :E.shape[1]] = E
    return MatrixData(nr_normal=n_all, nr_eq=E.shape[0], nr_range=0, nr_le=A_le.shape[0], nr_ge=0, b=np.concatenate([e_rhs, b_le]),
                      cost=np.array(cost, dtype=np.float64), upper_bound=np.full(n_all, np.inf), dense=np.asfortranarray(np.vstack([Ew, A_le])))


def interleaved_history(t, lp, n, eq, seed):
    """solve; add 4 columns; run; add 3 tight and 3 loose cuts; run_dual; add 3 columns with entries in the cut rows (two at cost
    +1); run.  The added columns have no entry in the == rows.  Returns the dense <= part of the final LP over [n | 7 added]
    columns, its rhs and the costs: rows [m | 6 cuts]."""
    m = lp["A"].shape[0]
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    assert t.nr_rows() == eq + m
    pad = np.zeros((eq, 7))
    A1, c1 = np.array(lp["A"][:, n:n + 4]), np.array(lp["c"][n:n + 4])
    c1[1] = 1.0
    t.add_columns(np.vstack([pad[:, :4], A1]), c1)
    assert t.run(1 << 20)[1] == engine.OPTIMAL
    x = np.zeros(n)
    for j, v in t.current_bfs():
        if j < n:
            x[j] = v
    rng = np.random.default_rng(31 * seed + eq)
    G = rng.integers(0, 8, (6, n)).astype(float)
    tight = np.array([True, False, True, False, True, False])
    beta = np.where(tight, 0.9 * (G @ x), 1.5 * (G @ x) + 1.0)
    t.add_cuts(G, beta)
    assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    A2 = np.vstack([np.array(lp["A"][:, n + 4:n + 7]), rng.integers(0, 4, (6, 3)).astype(float)])
    c2 = np.array(lp["c"][n + 4:n + 7])
    c2[[0, 2]] = 1.0
    t.add_columns(np.vstack([pad[:, :3], A2]), c2)
    assert t.run(1 << 20)[1] == engine.OPTIMAL
    A_le = np.zeros((m + 6, n + 7))
    A_le[:m, :n], A_le[m:, :n] = lp["A"][:, :n], G
    A_le[:m, n:n + 4] = A1
    A_le[:, n + 4:] = A2
    return A_le, np.concatenate([lp["b"], beta]), np.concatenate([lp["c"][:n], c1, c2])


@pytest.mark.parametrize("update_block", [3, -1])
@pytest.mark.parametrize("dup", [None, 3])
def test_cuts_and_columns_interleaved(dup, update_block):
    """Provider columns of the handle: [n | slacks of the <= rows | 4 added | 6 cut slacks | 3 added]; rows [== kept | m | 6 cuts].
    Removed: the non-basic added columns, then -- by their indices as they are then -- the cuts whose slack is basic; each step
    against a twin that flushes instead."""
    m, n, seed = 24, 32, 1
    lp = dense_lp(m, n + 7, seed)
    narrow = dict(A=np.array(lp["A"][:, :n]), b=lp["b"], c=np.array(lp["c"][:n]))
    if dup is None:
        E, e_rhs, eq = np.zeros((0, n)), np.zeros(0), 0
    else:
        E, e_rhs = equality_rows(narrow, dup)
        eq = 4
    md = mixed_md(E, e_rhs, narrow["A"], narrow["b"], narrow["c"])
    a, twin, second = (new_handle(md, update_block=update_block) for _ in range(3))      # second: the twin of the second removal
    A_le, b_le, cost = interleaved_history(a, lp, n, eq, seed)
    interleaved_history(twin, lp, n, eq, seed)
    interleaved_history(second, lp, n, eq, seed)
    rows0, first_tail = eq + m, n + m
    tail = [("col", 0), ("col", 1), ("col", 2), ("col", 3)] + [("cut", c) for c in range(6)] + [("col", 4), ("col", 5), ("col", 6)]
    basic = set(int(j) for j in a.basis_indices())
    gone_cols = [first_tail + x for x, (kind, _) in enumerate(tail) if kind == "col" and first_tail + x not in basic]
    assert len(gone_cols) >= 2                                   # (the three columns at cost +1 never price out)
    a.remove_columns(gone_cols)
    twin.flush()
    keep_t, keep_c, keep_j, col_map = surviving(a, twin, [], gone_cols)
    assert_same_bits(a, twin, keep_t, keep_c, keep_j, col_map)
    twin.close()
    twin = second
    twin.remove_columns(gone_cols)                               # the same calls as `a` so far: the same bits
    assert a.relative_costs().tobytes() == twin.relative_costs().tobytes() and a.b().tobytes() == twin.b().tobytes()
    tail = [e for x, e in enumerate(tail) if first_tail + x not in gone_cols]
    # the cuts whose slack is basic, by their indices now
    where = {int(j): r for r, j in enumerate(a.basis_indices())}
    slack_of = {c: first_tail + x for x, (kind, c) in enumerate(tail) if kind == "cut"}
    gone_cuts = [c for c in range(6) if slack_of[c] in where]
    outside = [c for c in gone_cuts if where[slack_of[c]] != rows0 + c]
    print(f"   dup {dup} block {update_block}: removed columns {gone_cols}, cuts {gone_cuts}, of them basic outside their row {outside}")
    assert gone_cuts
    rows = [rows0 + c for c in gone_cuts]
    a.remove_cuts(rows)
    twin.flush()
    keep_t, keep_c, keep_j, col_map = surviving(a, twin, rows, [slack_of[c] for c in gone_cuts])
    assert_same_bits(a, twin, keep_t, keep_c, keep_j, col_map)
    assert a.removal_stats()[:2] == (len(gone_cuts), len(gone_cols))
    assert a.cut_stats()[:2] == (6 - len(gone_cuts), 16) and a.column_stats()[:2] == (7 - len(gone_cols), 16)
    # the smaller LP: the surviving added columns as structural columns, the surviving cuts as <= rows
    tail = [e for e in tail if not (e[0] == "cut" and e[1] in gone_cuts)]
    kept_cols = [i for kind, i in tail if kind == "col"]
    kept_cuts = [c for kind, c in tail if kind == "cut"]
    rows_le = list(range(m)) + [m + c for c in kept_cuts]
    cols_s = list(range(n)) + [n + i for i in kept_cols]
    md_small = mixed_md(E, e_rhs, A_le[np.ix_(rows_le, cols_s)], b_le[rows_le], cost[cols_s])
    to_fresh = None
    if dup is None:                                             # (with == rows a fresh engine has the redundant rows again: no common basis)
        k_s = len(kept_cols)
        order = [n + kept_cols.index(i) if kind == "col" else n + k_s + m + kept_cuts.index(i) for kind, i in tail]
        to_fresh = np.concatenate([le_order(n, m, k_s), np.array(order, dtype=np.int64)])
    assert_sound(a, md_small, to_fresh)
    a.close()
    twin.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def everything(t):
    return dict(d=t.relative_costs().tobytes(), b=t.b().tobytes(), pi=t.minus_pi().tobytes(), basis=t.basis_indices().tobytes(),
                objective=t.objective_function_value(), trace=t.trace(), reinversions=t.reinversions(), flushes=t.flush_stats(),
                rhs=t.right_hand_side().tobytes(), rows=t.nr_rows(), columns=t.nr_columns(), cost=t.cost().tobytes(), cuts=t.cut_stats(),
                added=t.column_stats(), removed=t.removal_stats(), retab=t.retab_stats())


def test_refusals_leave_everything_as_it_was():
    m, n, seed, k = 24, 32, 1, KT + KL
    lp, wide = dense_lp(m, n, seed), dense_lp(m, n + 3, seed)
    a = new_handle(le_md(lp["A"], lp["b"], lp["c"]))           # (update_block -1: the block stays open, a refusal must not flush it)
    cuts_history(a, lp, seed, CUT_SEED[(m, n, seed)])
    a.add_columns(np.vstack([np.array(wide["A"][:, n:]), np.zeros((k, 3))]), np.array([1.0, wide["c"][n + 1], 1.0]))
    assert a.run(1 << 20)[1] == engine.OPTIMAL
    where = {int(j): r for r, j in enumerate(a.basis_indices())}
    first_slack, first_added = n + m, n + m + k
    basic_cuts = [c for c in range(k) if first_slack + c in where]
    tight_cuts = [c for c in range(k) if first_slack + c not in where]
    basic_added = [c for c in range(3) if first_added + c in where]
    loose_added = [c for c in range(3) if first_added + c not in where]
    assert basic_cuts and tight_cuts and loose_added
    before = everything(a)
    columns_before = [a.generate_column(j).tobytes() for j in (0, n, first_slack, first_added)]
    lib, h = a._lib, a._h

    def raw(call, values, count=None):
        arr = None if values is None else np.ascontiguousarray(values, dtype=np.int32)
        return getattr(lib, call)(h, None if arr is None else arr.ctypes.data, len(values) if count is None else count)

    good_row, good_col = m + basic_cuts[0], first_added + loose_added[0]
    cases = {
        "cuts: count < 0": ("relp_remove_cuts", [good_row], -1, E_ARG),
        "cuts: rows missing": ("relp_remove_cuts", None, 1, E_ARG),
        "cuts: a constraint row": ("relp_remove_cuts", [m - 1], None, E_ARG),
        "cuts: behind the last row": ("relp_remove_cuts", [m + k], None, E_ARG),
        "cuts: negative": ("relp_remove_cuts", [-1], None, E_ARG),
        "cuts: named twice": ("relp_remove_cuts", [good_row, good_row], None, E_ARG),
        "cuts: a good one and a bad one": ("relp_remove_cuts", [good_row, 0], None, E_ARG),
        "cuts: slack not basic": ("relp_remove_cuts", [m + tight_cuts[0]], None, E_STATE),
        "cuts: a good one and a tight one": ("relp_remove_cuts", [good_row, m + tight_cuts[0]], None, E_STATE),
        "columns: count < 0": ("relp_remove_columns", [good_col], -1, E_ARG),
        "columns: columns missing": ("relp_remove_columns", None, 1, E_ARG),
        "columns: a structural column": ("relp_remove_columns", [0], None, E_ARG),
        "columns: a cut slack": ("relp_remove_columns", [first_slack + basic_cuts[0]], None, E_ARG),
        "columns: behind the last column": ("relp_remove_columns", [first_added + 3], None, E_ARG),
        "columns: named twice": ("relp_remove_columns", [good_col, good_col], None, E_ARG),
    }
    if basic_added:
        cases["columns: basic"] = ("relp_remove_columns", [first_added + basic_added[0]], None, E_STATE)
        cases["columns: a good one and a basic one"] = ("relp_remove_columns", [good_col, first_added + basic_added[0]], None, E_STATE)
    for name, (call, values, count, want) in cases.items():
        assert raw(call, values, count) == want, name
        assert everything(a) == before, name
    assert [a.generate_column(j).tobytes() for j in (0, n, first_slack, first_added)] == columns_before
    assert raw("relp_remove_cuts", [], 0) == 0 and raw("relp_remove_columns", None, 0) == 0      # count == 0: a no-op, no flush
    a.remove_cuts([])
    assert everything(a) == before
    assert lib.relp_removal_stats(h, None) == E_ARG
    assert raw("relp_remove_cuts", [good_row]) == 0 and raw("relp_remove_columns", [good_col - 1]) == 0      # the good calls are taken
    assert a.removal_stats()[:2] == (1, 1) and a.nr_rows() == m + k - 1 and a.nr_columns() == n + m + k + 3 - 2
    a.close()


def test_refused_in_phase_one_and_on_the_other_engines():
    lp = dense_lp(24, 32, 1)
    cover, _ = __import__("dual_reference").covering_lp(6, 5, 3)          # >= rows: the engine starts in phase 1
    t = engine.Tableau(cover, engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (lambda: t.remove_cuts([6]), lambda: t.remove_columns([5]), t.removal_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    t.close()
    for kind in (engine.ENGINE_REVISED, engine.ENGINE_LU):
        t = engine.Tableau(le_md(lp["A"], lp["b"], lp["c"]), engine=kind)
        assert t.solve_relaxation() == engine.OPTIMAL
        objective = t.objective_function_value()
        for call in (lambda: t.remove_cuts([24]), lambda: t.remove_columns([56]), t.removal_stats):
            with pytest.raises(engine.RelpError) as err:
                call()
            assert status_of(err) == E_UNSUPPORTED
        assert t.nr_rows() == 24 and t.objective_function_value() == objective
        t.close()
