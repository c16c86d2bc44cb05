"""tests/pool_reference.py proves its own inputs (CPU tier): the model of the price on a hand-checked pool, and the cutting-stock
instance of tests/test_gpu_pool.py -- the exact column-generation loop over Fractions ends inside the round cap the GPU test uses, at
the exact optimum of the LP over all patterns, which oracle/relp_exact.py solves here and the GPU test carries as a number."""
from fractions import Fraction

import numpy as np
import pytest

import pool_reference as ref
from oracle import relp_exact as rx


def test_the_price_model_on_a_hand_checked_pool():
    minus_pi = np.array([0.5, -2.0, 0.25, 0.0])
    A = np.array([[2.0, 0.0, 0.0, 4.0],
                  [1.0, 0.0, 1.0, 0.0],
                  [0.0, 0.0, 4.0, 0.0],
                  [0.0, 0.0, 9.0, 1.0]])
    cost = np.array([0.5, 3.0, 1.0, -2.0])
    d = ref.reduced_costs(A, cost, minus_pi)
    assert d.tolist() == [0.5 + 1.0 - 2.0, 3.0, 1.0 - 2.0 + 1.0, -2.0 + 2.0]         # [-0.5, 3, 0, 0]: exact in binary
    all_on = np.ones(4, dtype=np.uint8)
    assert ref.winners(d, all_on, 1, 0.0)[0].tolist() == [0]
    assert ref.winners(d, all_on, 1, 0.5)[0].tolist() == []                              # d == -tol is no candidate
    assert ref.winners(d, np.array([0, 1, 1, 1]), 1, 0.0)[0].tolist() == []              # the only candidate is inactive
    ids, dw = ref.winners(np.array([-1.0, -3.0, -3.0, 2.0, -0.5]), np.ones(5), 2, 0.0)   # shares of 3: [0, 3) and [3, 5)
    assert ids.tolist() == [1, 4] and dw.tolist() == [-3.0, -0.5]                        # the lower index of the equal minima
    assert ref.winners(np.array([-1.0, -3.0, 2.0]), np.ones(3), 3, 0.0)[0].tolist() == [0, 1]
    # the chain is one fma per entry by ascending row, whatever the caller's order
    assert ref.reduced_cost(1.0, [2, 0], [3.0, 0.1], [0.1, 0.0, 1e16]) == ref.reduced_cost(1.0, [0, 2], [0.1, 3.0], [0.1, 0.0, 1e16])


def test_the_instance():
    pool = ref.maximal_patterns()
    assert len(pool) == 35 == len(set(pool))
    for p in pool:
        used = sum(a * w for a, w in zip(p, ref.WIDTHS))
        assert used <= ref.ROLL and ref.ROLL - used < min(ref.WIDTHS)
    assert ref.initial_patterns() == [(2, 0, 0, 0, 0), (0, 2, 0, 0, 0), (0, 0, 3, 0, 0), (0, 0, 0, 5, 0), (0, 0, 0, 0, 8)]
    assert ref.block(pool).shape == (5, 35) and ref.block(pool)[:, 0].tolist() == list(pool[0])


def test_the_full_lp_has_the_carried_optimum():
    objective, _ = ref.exact_master(ref.maximal_patterns())
    assert objective == ref.FULL_OPTIMUM == Fraction(985, 17)
    # the initial patterns alone are feasible and dearer
    first, _ = ref.exact_master(ref.initial_patterns())
    assert first == sum(Fraction(d, ref.ROLL // w) for d, w in zip(ref.DEMAND, ref.WIDTHS)) > ref.FULL_OPTIMUM


@pytest.mark.parametrize("segments", [1, 4])
def test_the_exact_loop_ends_inside_the_cap_at_the_optimum(segments):
    pool = ref.maximal_patterns()
    rounds, added, objective, ended = ref.exact_column_generation(segments, ref.round_cap(segments))
    print(f"segments {segments}: {rounds} rounds, {len(added)} of {len(pool)} columns added: {added}")
    assert ended and rounds == ref.EXACT_ROUNDS[segments] and ref.round_cap(segments) == 2 * rounds < len(pool)
    assert objective == ref.FULL_OPTIMUM
    assert len(added) == len(set(added)) < len(pool)       # fewer columns than the pool holds
