"""relp_gomory_cuts / relp_gomory_stats of the tableau engine through the C ABI, against tests/gomory_reference.py (numpy f64 and
brute force): the rounds gomory_cuts -> add_cuts -> run_dual on the integer programs of tests/test_gomory_reference.py, the violation
of an added cut, the call at p = 0 and with an open update block, the read-only contract, the refusals and the counters.

Rounding bounds.  gamma(N) = N u / (1 - N u) (kernel_harness.gamma) times the sum S of the absolute values of the terms involved:
  * b of an added cut row is  beta - sum_r g_B(r) b_r  with  g_c = -pi_c + sum_i y_i A[i,c] + y_bound(c)  and  beta = -f0 + sum_i
    y_i rhs_i:  N = (rows of A + 8 tree levels + 2) + (m + 1) + (basic structural columns + 1);  S = sum_c |x_c| (sum_i |y_i A[i,c]|
    + |pi_c| + |y_bound(c)|) + sum_i |y_i rhs_i| + f0.  (The identity b_new = -f0 is exact for an exact tableau; the tableau's own
    pivoting error is not part of the bound.)
  * a cut at p pending rows against the same cut after the flush: every entry of the row moves by the p fmas of the open block
    against the flush's own order, 2 (p + 1) roundings on terms no larger in sum than assumed below, so  N' = N_g + 2 (p + 1)  on
    S_c = sum_i |A[i,c]| (|y_i| + |a_{s_i}|) + |pi_c| + |a_c| + the bound-row terms  (a = the row's entries; assumes no cancellation
    inside T0 + W R0 beyond the entry's own size)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine

import gomory_reference as gr
import kernel_harness as kh
from test_gomory_reference import CAP, INSTANCES, PER_ROUND, make, points_of
from test_gpu_rhs_in_place import E_ARG, E_STATE, E_UNSUPPORTED, dense_lp, le_lp, pending_rows, solved, status_of

pytestmark = pytest.mark.gpu


def md_of(inst):
    A = np.asfortranarray(np.array(inst["A"], dtype=np.float64))
    upper = np.full(4, np.inf) if inst["upper"] is None else np.array(inst["upper"], dtype=np.float64)
    return MatrixData(nr_normal=4, nr_eq=inst["nr_eq"], nr_range=0, nr_le=inst["nr_le"], nr_ge=inst["nr_ge"],
                      b=np.array(inst["b"], dtype=np.float64), cost=-np.array(inst["c"], dtype=np.float64), upper_bound=upper, dense=A)


def open_integer_program(name):
    t = engine.Tableau(md_of(INSTANCES[name]), engine=engine.ENGINE_TABLEAU, trace_capacity=4096, poll_interval=1)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    return t


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_rounds_walk_the_reference_to_the_integer_optimum(name):
    inst = INSTANCES[name]
    best = max(int(np.dot(p, inst["c"])) for p in points_of(inst))
    t = open_integer_program(name)
    start = [int(j) for j in t.basis_indices()]
    ref = gr.rounds(make(inst, False), start, max_rounds=CAP, cuts_per_round=PER_ROUND)
    assert ref and ref[-1].objective is not None
    done = 0
    for rnd in ref:                                    # the driver's loop, one round at a time
        b, basis = t.b(), t.basis_indices()
        rows = gr.pick_rows(b, basis, [True] * t.nr_columns(), 1e-6, PER_ROUND)
        assert rows == rnd.rows
        G, rhs, fraction, status = t.gomory_cuts(rows)
        assert (status == engine.GOMORY_CUT).all()
        for k, (g, beta, f0) in enumerate(rnd.cuts):
            assert np.allclose(G[k], g, rtol=0, atol=1e-9) and abs(rhs[k] - beta) <= 1e-9 and abs(fraction[k] - f0) <= 1e-9
        t.add_cuts(G, rhs)
        assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
        done += 1
        print(f"{name} round {done}: objective {t.objective_function_value()!r}, reference {rnd.objective!r}")
        assert abs(t.objective_function_value() - rnd.objective) <= 1e-9 * max(1.0, abs(rnd.objective))
        assert sorted(int(j) for j in t.basis_indices()) == sorted(rnd.basis)
    assert abs(t.objective_function_value() + best) <= 1e-9 * max(1, abs(best))
    t.close()
    # the driver on a second handle: the same rounds, cuts and objectives
    twin = open_integer_program(name)
    rounds, added, objectives, outcome = engine.gomory_rounds(twin, None, CAP, PER_ROUND)
    assert outcome == engine.OPTIMAL and rounds == len(ref) and added == sum(len(r.cuts) for r in ref)
    assert all(abs(o - r.objective) <= 1e-9 * max(1.0, abs(r.objective)) for o, r in zip(objectives, ref))
    assert abs(objectives[-1] + best) <= 1e-9 * max(1, abs(best))
    twin.close()


def reference_lp(lp):
    m = lp["A"].shape[0]
    return gr.LP(lp["A"].tolist(), lp["b"].tolist(), lp["c"].tolist(), 0, m, 0)


def violation_bound(ref_lp, row, b_r, basis, r, x):
    """(gamma(N) * S, detail) of the first bound of the module docstring for the cut of row r."""
    in_basis = [False] * ref_lp.ncol
    for j in basis:
        in_basis[int(j)] = True
    detail = {}
    g, beta, f0, status = gr.cut(ref_lp, row, b_r, int(basis[r]), in_basis, detail=detail)
    assert status == gr.CUT
    pi, y = detail["pi"], detail["y"]
    S = Fraction(f0)
    for c in range(ref_lp.n):
        terms = sum(abs(Fraction(y[i]) * Fraction(ref_lp.full[i][c])) for i in range(ref_lp.m)) + abs(Fraction(pi[c]))
        S += abs(Fraction(x[c])) * terms
    S += sum(abs(Fraction(y[i]) * Fraction(ref_lp.rhs[i])) for i in range(ref_lp.m))
    basic_structural = sum(1 for j in basis if int(j) < ref_lp.n)
    N = (ref_lp.mc + ref_lp.nr_cuts + 8 + 2) + (ref_lp.m + 1) + (basic_structural + 1)
    return float(kh.gamma(N) * S), detail


@pytest.mark.parametrize("update_block", [3, -1])
def test_b_of_an_added_cut_is_minus_the_fraction(update_block):
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed, update_block=update_block)
    basis, b = t.basis_indices(), t.b()
    ref_lp = reference_lp(lp)
    T, _, _ = ref_lp.tableau(basis)
    x = np.zeros(n)
    for i, j in enumerate(basis):
        if j < n:
            x[j] = b[i]
    rows = [i for i in range(m) if 1e-3 <= b[i] - math.floor(b[i]) <= 1 - 1e-3][:9]
    assert len(rows) == 9
    G, rhs, fraction, status = t.gomory_cuts(rows)
    assert (status == engine.GOMORY_CUT).all()
    assert np.array_equal(fraction, b[rows] - np.floor(b[rows]))
    t.add_cuts(G, rhs)
    b_new = t.b()[m:]
    for k, r in enumerate(rows):
        bound, _ = violation_bound(ref_lp, T[r], b[r], basis, r, x)
        print(f"row {r}: b_new + f0 = {b_new[k] + fraction[k]:.3e}, bound {bound:.3e}")
        assert abs(b_new[k] + fraction[k]) <= bound
    assert t.run_dual(1 << 20)[1] == engine.OPTIMAL
    t.close()


def test_open_block_and_flushed_agree():
    m, n, seed = 40, 300, 4
    lp, t = solved(m, n, seed, update_block=-1)
    p = pending_rows(t)
    assert p >= 1
    basis, b = t.basis_indices(), t.b()
    rows = np.array([i for i in range(m) if 1e-3 <= b[i] - math.floor(b[i]) <= 1 - 1e-3][:9], dtype=np.int32)
    open_block = t.gomory_cuts(rows)
    assert t.gomory_stats() == (1, len(rows), len(rows), p)
    t.flush()
    flushed = t.gomory_cuts(rows)
    assert t.gomory_stats() == (2, 2 * len(rows), 2 * len(rows), 0)
    assert np.array_equal(open_block[3], flushed[3]) and np.array_equal(open_block[2], flushed[2])
    ref_lp = reference_lp(lp)
    T, _, _ = ref_lp.tableau(basis)
    A = np.abs(lp["A"])
    N = m + 8 + 2 + 2 * (p + 1)
    worst = 0.0
    for k, r in enumerate(rows):
        _, detail = violation_bound(ref_lp, T[r], b[r], basis, r, np.zeros(n))
        y, pi = np.abs(np.array(detail["y"], dtype=np.float64)), np.abs(np.array(detail["pi"], dtype=np.float64))
        a_slack = np.abs(T[r][n:n + m])
        S = A.T @ (y + a_slack) + pi[:n] + np.abs(T[r][:n])
        bound = float(kh.gamma(N)) * S
        diff = np.abs(open_block[0][k] - flushed[0][k])
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all()
        S_beta = float(np.abs(lp["b"]) @ (y + a_slack)) + 1.0
        assert abs(open_block[1][k] - flushed[1][k]) <= float(kh.gamma(m + 1 + 2 * (p + 1))) * S_beta
    print(f"p = {p}: largest |g_open - g_flushed| / bound = {worst:.3f}")
    t.close()


def snapshot(t):
    return (t.b().tobytes(), t.relative_costs().tobytes(), t.basis_indices().tobytes(), t.minus_pi().tobytes(), t.objective_function_value(),
            len(t.trace()), t.reinversions(), t.flush_stats(), t.right_hand_side().tobytes(), t.ranging_stats(), t.cut_stats())


@pytest.mark.parametrize("update_block", [3, -1])
def test_the_call_changes_nothing_and_repeats_its_bits(update_block):
    m, n, seed = 40, 300, 4
    lp, t = solved(m, n, seed, update_block=update_block)
    _, twin = solved(m, n, seed, update_block=update_block)
    before = snapshot(t)
    assert before == snapshot(twin)
    rows = np.concatenate([np.arange(m - 1, -1, -1), [3, 3]]).astype(np.int32)      # descending, one row three times
    flags = np.ones(t.nr_columns(), dtype=np.uint8)
    flags[1::3] = 0
    first = t.gomory_cuts(rows) + t.gomory_cuts(rows, flags, engine.GOMORY_MIXED, 0.01)
    assert snapshot(t) == before
    again = t.gomory_cuts(rows) + t.gomory_cuts(rows, flags, engine.GOMORY_MIXED, 0.01)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    assert snapshot(t) == before
    assert np.array_equal(first[0][-1], first[0][-2]) and np.array_equal(first[0][-1], first[0][m - 1 - 3])   # the repeated row
    assert set(first[3].tolist()) <= {0, 2} and (first[3] == 0).sum() >= m // 2
    assert set(first[7].tolist()) <= {0, 1, 2} and (first[7] == 1).any() and (first[7] == 0).any()
    skipped = first[7] != 0
    assert (first[4][skipped] == 0).all() and (first[5][skipped] == 0).all()
    assert t.gomory_stats()[0] == 4 and t.gomory_stats()[1] == 4 * len(rows) and t.gomory_stats()[3] == pending_rows(t)
    # a fractional cut with a continuous non-basic column in the row: status 4, all zero
    nonbasic = np.flatnonzero(t.relative_costs() > 1e-6)
    only = np.ones(t.nr_columns(), dtype=np.uint8)
    only[nonbasic[0]] = 0
    G4, rhs4, f4, st4 = t.gomory_cuts(rows[:8], only)
    assert (st4[first[3][:8] == 0] == engine.GOMORY_CONTINUOUS).all() and (G4 == 0).all() and (rhs4 == 0).all()
    assert np.array_equal(f4, first[2][:8])
    # the handle that was queried and the one that was not walk the same dual pivots to the same b
    b2 = lp["b"].copy()
    b2[::3] *= 0.5
    for handle in (t, twin):
        handle.change_right_hand_side(np.arange(0, m, 3), b2[::3])
    result = t.run_dual(1 << 20)
    assert result[1] == engine.OPTIMAL and result == twin.run_dual(1 << 20)
    assert t.trace() == twin.trace() and t.b().tobytes() == twin.b().tobytes()
    t.close()
    twin.close()


def raw_call(lib, t, rows, count, kind=0, away=1e-6, drop=None, nn=32):
    out = dict(coefficients=np.full((4, nn), -7.0), rhs=np.full(4, -7.0), fraction=np.full(4, -7.0), status=np.full(4, -7, dtype=np.int32))
    r = np.array(rows, dtype=np.int32)
    ptr = {k: (None if k == drop else v.ctypes.data) for k, v in out.items()}
    st = lib.relp_gomory_cuts(t.handle, None if drop == "rows" else r.ctypes.data, count, None, kind, away, ptr["coefficients"], ptr["rhs"],
                              ptr["fraction"], ptr["status"])
    untouched = all((v == -7).all() for v in out.values())
    return st, untouched


def test_argument_errors_write_nothing():
    m, n, seed = 24, 32, 1
    lp, t = solved(m, n, seed)
    lib = engine.load_library()
    before = snapshot(t)
    for rows, count in (([0, m], 2), ([-1], 1), ([0, 1, 2, m + 5], 4), ([0], -1)):
        assert raw_call(lib, t, rows, count) == (E_ARG, True)
    for kind in (-1, 2):
        assert raw_call(lib, t, [0], 1, kind=kind) == (E_ARG, True)
    for away in (-1e-9, 0.5, 0.75, math.inf, math.nan):
        assert raw_call(lib, t, [0], 1, away=away) == (E_ARG, True)
    for drop in ("rows", "coefficients", "rhs", "status"):
        assert raw_call(lib, t, [0], 1, drop=drop) == (E_ARG, True)
    assert raw_call(lib, t, [0], 0) == (0, True)                                   # count == 0: a no-op
    assert lib.relp_gomory_cuts(t.handle, None, 0, None, 0, 0.0, None, None, None, None) == 0
    assert t.gomory_stats() == (0, 0, 0, 0) and snapshot(t) == before
    st, untouched = raw_call(lib, t, [5, 0, 5], 3, drop="fraction")                # fraction may be NULL
    assert st == 0 and not untouched
    assert t.gomory_stats()[:2] == (1, 3)
    assert raw_call(lib, t, [0], 1, away=0.0)[0] == 0
    t.close()


def test_refused_in_phase_one_on_other_engines_with_range_rows_and_with_added_columns():
    lp = dense_lp(24, 32, 1)
    inst = INSTANCES["bounded"]
    t = engine.Tableau(md_of(inst), engine=engine.ENGINE_TABLEAU)
    assert t.phase == 1
    for call in (lambda: t.gomory_cuts([0]), t.gomory_stats):
        with pytest.raises(engine.RelpError) as err:
            call()
        assert status_of(err) == E_STATE
    t.close()
    for kind in (engine.ENGINE_REVISED, engine.ENGINE_LU):
        t = engine.Tableau(le_lp(lp, lp["b"]), engine=kind)
        assert t.solve_relaxation() == engine.OPTIMAL
        for call in (lambda: t.gomory_cuts([0]), t.gomory_stats):
            with pytest.raises(engine.RelpError) as err:
                call()
            assert status_of(err) == E_UNSUPPORTED
        t.close()
    ranged = MatrixData(nr_normal=4, nr_eq=0, nr_range=1, nr_le=2, nr_ge=0, b=np.array([20.0, 31.0, 37.0]), cost=-np.array([5.0, 4.0, 6.0, 3.0]),
                        upper_bound=np.full(4, np.inf), ranges=np.array([8.0]),
                        dense=np.asfortranarray(np.array([[1.0, 2, 1, 3], [3, 5, 2, 7], [6, 2, 8, 3]])))
    t = engine.Tableau(ranged, engine=engine.ENGINE_TABLEAU)
    assert t.solve_relaxation() == engine.OPTIMAL and t.phase == 2
    with pytest.raises(engine.RelpError) as err:
        t.gomory_cuts([0])
    assert status_of(err) == E_UNSUPPORTED
    t.close()
    _, t = solved(24, 32, 1)
    t.add_columns(np.ones((t.nr_rows(), 1)), [1.0])
    with pytest.raises(engine.RelpError) as err:
        t.gomory_cuts([0])
    assert status_of(err) == E_STATE
    assert t.gomory_stats() == (0, 0, 0, 0)
    t.close()
