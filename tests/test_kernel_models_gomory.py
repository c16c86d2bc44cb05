"""The f64 model of launch_tab_gomory (tests/kernel_harness_gomory.py, tests/gomory_reference.py) against the rule and the sums over
Fractions on the case table of tests/kernel_gomory_cases.py -- CPU tier; tests/test_gpu_kernels_gomory.py holds the device to the
f64 model bit for bit."""
import numpy as np
import pytest

import gomory_reference as gr
from kernel_gomory_cases import BATCH_CASES, CASES


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_f64_model_is_within_the_rounding_bound_of_the_fraction_model(name):
    case = CASES[name]()
    pi, y, bad, g = case.expected()
    assert pi.shape == (case.count, case.n_owned) and y.shape == (case.count, case.m) and g.shape == (case.count, case.nn)
    assert np.isfinite(pi).all() and np.isfinite(g).all() and (pi >= 0).all()
    assert not case.exact_violations(pi, y, g)
    skipped = case.f0 < 0
    assert (pi[skipped] == 0).all() and (bad[skipped] == 0).all()
    assert (pi[:, :case.art] == 0).all() and (pi[:, ~case.cand()] == 0).all()


def test_the_table_covers_what_it_names():
    built = {name: make() for name, make in CASES.items()}
    assert sorted({c.n_owned for c in built.values()} & {1, 255, 256, 257}) == [1, 255, 256, 257]
    assert {c.count for c in built.values()} >= {1, 7, 8, 9} and {c.p for c in built.values()} >= {0, 1, 8, 9, 16}
    assert {c.nn for c in built.values()} >= {1, 257}
    for k in (0, 1, 255, 256, 257, 513):
        case = built[f"{k} row{'' if k == 1 else 's'} of A with y" if k else "no row of A with y"]
        free = sum(1 for v, r in enumerate(case.vrow0) if case.flags[case.nn + v] != 1)
        assert free == k
        assert (np.count_nonzero(case.expected()[1], axis=1) <= k).all()
    assert built["fractional, a continuous column"].expected()[2].any()            # status 4 is reached
    assert not built["mixed, continuous columns"].expected()[2].any()
    mixed = built["mixed, continuous columns"]
    E, cont = mixed.entries(), ~mixed.integer() & mixed.cand()
    assert (E[:, cont] > 0).any() and (E[:, cont] < 0).any()                        # a continuous column of either sign
    special = built["list of 7, descending"]
    pi = special.expected()[0]
    assert pi[0, 0] == 0 and pi[0, 1] == 0 and pi[0, 2] == 0 and pi[0, 3] == 0      # 0.0, -0.0 and the integers
    assert pi[0, 4] == special.f0[0] and pi[0, 5] == special.f0[0]                  # f == f0
    assert (pi[0, 6:10] == 0).all()                                                 # f within tol_zero of 0 and of 1, |a| <= tol_zero
    assert 3e-11 < pi[0, 10] < 5e-11 and 3e-11 < 1 - pi[0, 11] < 5e-11              # just outside the two bands
    assert pi[0, 12] == 0.75 and pi[0, 13] == 0.25
    assert len(BATCH_CASES) == 2


def test_the_reference_and_the_kernel_model_agree_on_an_lp():
    """gomory_reference.cut (plain sums) and structural_f64 (the device's order) on the same row of a small LP."""
    lp = gr.LP([[3, 5, 2, 7], [6, 2, 8, 3], [1, 2, 1, 3]], [31, 37, 6], [-5, 2, -6, 3], 0, 2, 1, [3, np.inf, 2, np.inf])
    basis = gr.optimal_basis(gr.LP([[3, 5, 2, 7], [6, 2, 8, 3], [1, 2, 1, 3]], [31, 37, 6], [-5, 2, -6, 3], 0, 2, 1, [3, np.inf, 2, np.inf], exact=True))
    T, b, _ = lp.tableau(basis)
    in_basis = [j in basis for j in range(lp.ncol)]
    for r in range(lp.m):
        detail = {}
        g, beta, f0, status = gr.cut(lp, T[r], b[r], basis[r], in_basis, detail=detail)
        if status != gr.CUT:
            continue
        pi, y = np.array(detail["pi"]), np.array(detail["y"])
        A = np.array([row[:lp.n] for row in lp.full[:lp.mc]])
        g2 = gr.structural_f64(pi[None, :lp.n], y[None, :], A, np.arange(lp.mc), lp.bound_row)[0]
        assert np.allclose(g2, g, rtol=0, atol=1e-12)
        assert abs(gr.beta_f64(f0, y, lp.rhs) - beta) <= 1e-12
