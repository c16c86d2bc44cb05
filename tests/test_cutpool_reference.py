"""tests/cutpool_reference.py, the reference of the cut-pool tests, checked on the CPU: the model of relp_cutpool_slacks and
relp_cutpool_separate on hand-made data, the agreement of the two models (this one over dense blocks, tests/kernel_harness_cutpool.py
over sliced ELL), and the exact row-generation loop on the committed instance: it ends inside the round cap at a vertex that no pool
cut violates, which is the optimum of the LP over all cuts, and the constants the GPU tests rely on are its results."""
from fractions import Fraction

import numpy as np
import pytest

import cutpool_reference as ref
import kernel_harness as kh
import kernel_harness_cutpool as khc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def test_the_vertex_and_the_slacks():
    # rows 0 .. 3 basic in columns 2, 7 (a slack), 0, 9 (a slack) of 3 structural columns
    x = ref.vertex([1.5, 4.0, -2.0, 8.0], [2, 7, 0, 9], 3)
    assert x.tolist() == [-2.0, 0.0, 1.5] and not np.signbit(x[1])
    G = np.array([[1.0, 5.0, 2.0], [0.0, 0.0, 0.0], [0.0, 3.0, 0.0], [-0.5, 0.0, 0.0]])
    rhs = np.array([2.0, -1.0, 4.0, 0.0])
    s = ref.slacks(G, rhs, x)
    assert s.tolist() == [2.0 - (1.0 * -2.0 + 2.0 * 1.5), -1.0, 4.0, -1.0]      # a cut without entries has its rhs; x_1 = 0 adds nothing
    assert ref.norms(G).tolist() == [np.sqrt(30.0), 0.0, 3.0, 0.5]


def test_the_chain_is_an_fma_chain_in_ascending_column_order():
    # (1 + 2^-30)^2 needs the fma: the product rounded first would lose the 2^-60
    a = 1.0 + 2.0 ** -30
    x = np.array([1.0, a])
    s = ref.slack(0.0, np.array([1, 0]), np.array([a, -(1.0 + 2.0 ** -29)]), x)      # given descending, summed ascending
    want = 0.0 - kh.fma_exact(a, a, kh.fma_exact(-(1.0 + 2.0 ** -29), 1.0, 0.0))     # (descending, a * a would be rounded first: 0.0)
    assert bits([s]) == bits([want]) and s == -(2.0 ** -60)


def test_the_winners():
    s = np.array([-1.0, -4.0, 0.5, -4.0, -3.0, -0.25, -8.0])
    norm = np.array([1.0, 4.0, 1.0, 2.0, 0.0, 1.0, 16.0])
    on = np.ones(7)
    assert ref.winners(s, norm, on, 1, 0.0)[0].tolist() == [6]
    assert ref.winners(s, norm, on, 1, 0.0, True)[0].tolist() == [4]                 # keys -1, -1, ., -2, -3 (norm 0 as 1), -.25, -.5
    ids, sl = ref.winners(s, norm, on, 3, 0.0)                                        # shares [0, 3), [3, 6), [6, 7)
    assert ids.tolist() == [1, 3, 6] and sl.tolist() == [-4.0, -4.0, -8.0]
    assert ref.winners(s, norm, on, 3, 0.0, True)[0].tolist() == [0, 4, 6]            # the tie of the keys of 0 and 1: the lower index
    assert ref.winners(s, norm, on, 7, 0.25)[0].tolist() == [0, 1, 3, 4, 6]           # s == -tol is no candidate
    off = on.copy()
    off[[6, 1]] = 0
    assert ref.winners(s, norm, off, 1, 0.0)[0].tolist() == [3]
    assert ref.winners(s, norm, on, 2, 8.0)[0].shape == (0,)


def test_both_models_agree():
    rng = np.random.default_rng(11)
    m, n, count = 9, 12, 70
    cuts = khc.random_cuts(rng, n, count, 5, empty=(3, 64))
    case = khc.Case(m, n, cuts, seed=12)
    G = np.zeros((count, n))
    for k, cut in enumerate(cuts):
        for c, v in cut:
            G[k, c] = v
    x = ref.vertex(case.b, case.basis, n)
    assert bits(x) == bits(case.x())
    s = ref.slacks(G, case.rhs, x)
    assert bits(s) == bits(case.slacks())
    assert bits(ref.norms(G)) == bits(case.norm)
    for segments, by_efficacy in ((1, 0), (4, 1), (70, 0)):
        want = case.separate_expected(segments, 1e-7, by_efficacy, s=case.slacks())
        ids, sl = ref.winners(case.slacks(), case.norm, case.active, segments, 1e-7, bool(by_efficacy))
        found = int(want["found"][0])
        assert want["out_k"][:found].tolist() == ids.tolist() and bits(want["out_s"][:found]) == bits(sl)


def test_the_instance():
    G, rhs = ref.instance()
    assert G.shape == (ref.CUTS, ref.DIM) and rhs.shape == (ref.CUTS,) and (np.abs(G) <= 9).all() and (G == np.round(G)).all()
    assert (np.abs(G).sum(axis=1) > 0).all() and np.isfinite(rhs).all()
    G2, rhs2 = ref.instance()
    assert bits(G) == bits(G2) and bits(rhs) == bits(rhs2)                            # generated, not drawn
    centre = np.full(ref.DIM, ref.SIDE / 2)
    assert ((rhs - G @ centre) > 0).all()                                             # the centre of the ball satisfies every cut
    objective, x = ref.exact_lp(G, rhs, [])
    assert objective == Fraction(sum(ref.COST)) * Fraction(ref.SIDE) and x == [Fraction(ref.SIDE)] * ref.DIM      # the box alone: its corner
    assert sum(1 for k in range(ref.CUTS) if Fraction(float(rhs[k])) < sum(Fraction(G[k, j]) * x[j] for j in range(ref.DIM))) > 20


@pytest.mark.parametrize("per_round,by_efficacy", sorted(ref.EXACT_ROUNDS))
def test_exact_row_generation_ends_at_the_optimum_inside_the_cap(per_round, by_efficacy):
    G, rhs = ref.instance()
    cap = ref.round_cap(per_round, by_efficacy)
    rounds, added, objective, x, done = ref.exact_row_generation(per_round, cap, by_efficacy)
    assert done and rounds == ref.EXACT_ROUNDS[(per_round, by_efficacy)] <= cap < ref.CUTS
    assert len(set(added)) == len(added) <= rounds * per_round
    # feasible for the LP over all cuts and optimal for a relaxation of it: optimal for it
    assert all(0 <= v <= Fraction(ref.SIDE) for v in x)
    assert all(sum(Fraction(G[k, j]) * x[j] for j in range(ref.DIM)) <= Fraction(float(rhs[k])) for k in range(ref.CUTS))
    assert objective == ref.FULL_OPTIMUM == sum(Fraction(c) * v for c, v in zip(ref.COST, x))
    assert float(ref.FULL_OPTIMUM) > sum(ref.COST) * ref.SIDE + 50                    # far from the box's corner
