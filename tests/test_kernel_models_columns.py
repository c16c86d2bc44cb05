"""CPU tier of the kernel tests of the columns added in place: the reference model of launch_tab_add_columns
(tests/kernel_harness_columns.py) against data on which every summation order gives the same exact result (small integers), against
`fractions.Fraction` arithmetic on a small case, and the image construction against itself (what a case may and may not change).
No GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_columns as khc


@pytest.mark.parametrize("m,n_store,count,entries,p", [(7, 5, 1, 1, 0), (30, 41, 9, 20, 3), (40, 33, 17, 0, 5), (300, 12, 3, 290, 2)])
def test_model_on_integers_where_every_order_is_exact(m, n_store, count, entries, p):
    case = khc.Case(m, n_store, count, entries, p, integers=True, seed=11, c_lo=2 if n_store > 5 else 0, col_off=2 if n_store > 5 else 0)
    new = khc.model_new_columns(case.T0, case.cols, case.coef, case.c_lo)
    T0, coef = np.rint(case.T0).astype(np.int64), np.rint(case.coef).astype(np.int64)
    ref = coef.T @ T0[case.cols - case.c_lo] if entries else np.zeros((count, m), dtype=np.int64)
    assert np.array_equal(new, ref.astype(np.float64))
    img, _ = case.expected()
    R0 = img["R0"].reshape(case.kmax + 1, case.ld_r)
    assert np.array_equal(R0[:p, case.n_owned:case.n_owned + count], ref[:, case.S].T.astype(np.float64))


def test_model_against_fractions_on_a_small_case():
    case = khc.Case(9, 6, 3, 5, 2, seed=5)
    new = khc.model_new_columns(case.T0, case.cols, case.coef)
    for k in range(3):
        for i in range(9):
            assert new[k][i] == khc.entry_exact(case.T0, case.cols, case.coef, k, i)
            exact = sum(Fraction(case.coef[e][k]) * Fraction(case.T0[case.cols[e]][i]) for e in range(5))
            # data below 2 in magnitude: every partial sum below 32, so each of the 5 roundings of the chain is at most 32 * 2^-53
            assert abs(Fraction(new[k][i]) - exact) <= 5 * 32 * kh.EPS53


def test_the_order_of_the_list_is_the_order_of_the_sum():
    """The model sums in ascending list order: reversing the list changes bits on real data (so a kernel that walked it otherwise
    would be caught), while a permutation of the new columns only permutes the result."""
    case = khc.Case(64, 40, 4, 30, 0, seed=3)
    new = khc.model_new_columns(case.T0, case.cols, case.coef)
    rev = khc.model_new_columns(case.T0, case.cols[::-1], case.coef[::-1])
    assert (new != rev).any() and np.abs(new - rev).max() < 1e-12
    perm = [2, 0, 3, 1]
    assert np.array_equal(khc.model_new_columns(case.T0, case.cols, case.coef[:, perm]), new[perm])


def test_model_of_d_is_the_chain_from_the_cost_over_ascending_rows():
    minus_pi = np.array([0.5, -1.25, 3.0, 0.1])
    want = kh.fma_exact(3.0, 0.3, kh.fma_exact(-1.25, 2.0, kh.fma_exact(0.5, -1.0, 7.0)))
    assert khc.model_d(7.0, minus_pi, [2, 0, 1], [0.3, -1.0, 2.0]) == want
    assert khc.model_d(7.0, minus_pi, [3, 2, 0, 1], [0.0, 0.3, -1.0, 2.0]) == want        # an explicit zero is no entry
    assert khc.model_d(7.0, minus_pi, [], []) == 7.0
    # small integers: exact in any order
    assert khc.model_d(2.0, np.array([1.0, 2.0, 3.0]), [2, 1, 0], [1.0, -1.0, 4.0]) == 2.0 + 4.0 - 2.0 + 3.0


def test_images_state_what_may_change():
    case = khc.Case(30, 257, 9, 20, 3, kmax=5, c_lo=2, col_off=4, seed=1)
    before = case.images()
    after, new = case.expected()
    assert not khc.diff_images(before, before) and khc.diff_images(before, after)
    m, n, cnt = case.m, case.n_owned, case.count
    T0b, T0a = before["T0"].reshape(n + cnt, case.ld_t), after["T0"].reshape(n + cnt, case.ld_t)
    changed = khc.image_bits(T0b) != khc.image_bits(T0a)
    assert not changed[:n].any() and not changed[:, m:].any()                  # the old columns; behind the rows up to the pitch
    assert changed[n:, :m].all() and T0a[n:, :m].tobytes() == new.tobytes()
    for name in ("cols", "coef", "S", "d_new", "cost_new"):
        assert not khc.diff_images({name: before[name]}, {name: after[name]})
    R0b, R0a = before["R0"].reshape(case.kmax + 1, case.ld_r), after["R0"].reshape(case.kmax + 1, case.ld_r)
    assert (khc.image_bits(R0b[:, :n]) == khc.image_bits(R0a[:, :n])).all() and (R0a[3:, n:n + cnt] == 0.0).all()
    assert (khc.image_bits(R0a[:, n + cnt:]) == kh.SENTINEL_BITS).all()
    assert R0a[:3, n:n + cnt].tobytes() == np.ascontiguousarray(new[:, case.S].T).tobytes()
    assert (after["in_basis"][case.flags.size:] == 0).all() and np.array_equal(after["in_basis"][:case.flags.size], case.flags)
    assert (after["vrow0"][case.first_virtual:] == -1).all() and (after["vrow1"][case.first_virtual:] == -1).all()
    assert (after["vsign"][case.first_virtual:] == 1).all() and (after["vrow0"][:case.first_virtual] == kh.SENTINEL_INT).all()
    assert after["d"][case.n_store:].tobytes() == case.d_new.tobytes() and after["cost_store"][case.n_store:].tobytes() == case.cost_new.tobytes()
    assert (khc.image_bits(after["d"][:case.c_lo]) == kh.SENTINEL_BITS).all()
