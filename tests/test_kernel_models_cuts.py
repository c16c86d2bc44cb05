"""CPU tier of the kernel tests of the in-place cut rows: the reference model of launch_tab_add_cuts
(tests/kernel_harness_cuts.py) against data on which every summation order gives the same exact result (small integers), against
`fractions.Fraction` arithmetic on a small case, and the image construction against itself (what a case may and may not change).
No GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_cuts as khc


def integer_reference(case):
    """T[new] = g - coef' T[rows] with T = T0 + W' R0 in plain int64 arithmetic (exact, order-free)."""
    T0, W, R0 = (np.rint(x).astype(np.int64) for x in (case.T0, case.W, case.R0))
    coef, g = np.rint(case.coef).astype(np.int64), np.rint(case.g_of_column()).astype(np.int64)
    p = case.p if case.entries else 0
    T = T0 + (R0[:p].T @ W[:p] if p else 0)                    # n_owned x m
    new = g - T[:, case.rows] @ coef
    new[case.basic()] = 0
    return new


@pytest.mark.parametrize("m,n_store,count,entries,p", [(7, 5, 1, 1, 0), (30, 41, 9, 20, 3), (40, 33, 17, 0, 5), (300, 12, 3, 290, 2)])
def test_model_on_integers_where_every_order_is_exact(m, n_store, count, entries, p):
    case = khc.Case(m, n_store, count, entries, p, integers=True, seed=11, col_off=2 if n_store > 5 else 0, basic=(0, 2), barred=(1,))
    new, u = khc.model_cut_rows(case.T0, case.W, case.R0, case.rows, case.coef, case.g_of_column(), case.basic())
    assert np.array_equal(new, integer_reference(case).astype(np.float64))
    if p and entries:
        assert np.array_equal(u, (np.rint(case.coef).T @ np.rint(case.W)[:, case.rows].T))
    else:
        assert u.shape == (count, 0)
    assert (new[case.basic()] == 0.0).all() and case.basic().sum() == 2


def test_model_against_fractions_on_a_small_case():
    case = khc.Case(9, 6, 3, 5, 2, seed=5, basic=(1,))
    new, u = khc.model_cut_rows(case.T0, case.W, case.R0, case.rows, case.coef, case.g_of_column(), case.basic())
    g = case.g_of_column()
    exact_T = lambda c, r: Fraction(case.T0[c][r]) + sum(Fraction(case.W[j][r]) * Fraction(case.R0[j][c]) for j in range(2))   # noqa: E731
    for k in range(3):
        for j in range(2):                                                     # fewer than 256 entries: one chain in thread order + zeros
            chain = [kh.chain_exact(0.0, [case.coef[e][k]], [case.W[j][case.rows[e]]]) for e in range(5)]
            assert u[k][j] == sum_tree(chain)
        for c in range(6):
            if case.basic()[c]:
                assert new[c][k] == 0.0 and not np.signbit(new[c][k])
                continue
            assert new[c][k] == khc.entry_exact(case.T0, case.W, case.R0, case.rows, case.coef, g[c][k], k, c, u[k])
            exact = Fraction(g[c][k]) - sum(Fraction(case.coef[e][k]) * exact_T(c, case.rows[e]) for e in range(5))
            # data below 2 in magnitude: |u| <= 20, every partial sum below 128, so each of the 8 roundings of the chain is at most
            # 128 * 2^-53, and the 5 roundings inside each of the two u (below 32 * 2^-53 each) are scaled by |R0| < 2
            assert abs(Fraction(new[c][k]) - exact) <= (8 * 128 + 2 * 2 * 5 * 32) * kh.EPS53


def sum_tree(values):
    """The fixed tree over 256 thread sums: thread t holds values[t] (0.0 beyond), s[t] += s[t + half] for half = 128 .. 1."""
    s = np.zeros(256)
    s[:len(values)] = values
    half = 128
    while half:
        s[:half] = s[:half] + s[half:2 * half]
        half //= 2
    return s[0]


def test_the_order_of_the_list_is_the_order_of_the_sum():
    """The model sums in ascending list order: reversing the list changes bits on real data (so a kernel that walked it otherwise
    would be caught), while a permutation of the cuts only permutes the result."""
    case = khc.Case(64, 40, 4, 30, 0, seed=3)
    new, _ = khc.model_cut_rows(case.T0, case.W, case.R0, case.rows, case.coef, case.g_of_column(), case.basic())
    rev, _ = khc.model_cut_rows(case.T0, case.W, case.R0, case.rows[::-1], case.coef[::-1], case.g_of_column(), case.basic())
    assert (new != rev).any() and np.abs(new - rev).max() < 1e-12
    perm = [2, 0, 3, 1]
    swapped, _ = khc.model_cut_rows(case.T0, case.W, case.R0, case.rows, case.coef[:, perm], case.g_of_column()[:, perm], case.basic())
    assert np.array_equal(swapped, new[:, perm])


def test_images_state_what_may_change():
    case = khc.Case(30, 257, 9, 20, 3, kmax=5, c_lo=2, col_off=4, seed=1, basic=(0, 7), barred=(3,))
    before = case.images()
    after, new, u = case.expected()
    assert not khc.diff_images(before, before) and khc.diff_images(before, after)
    m, n, cnt = case.m, case.n_owned, case.count
    T0b, T0a = before["T0"].reshape(n + cnt, case.ld_t), after["T0"].reshape(n + cnt, case.ld_t)
    changed = khc.image_bits(T0b) != khc.image_bits(T0a)
    assert not changed[:n, :m].any() and not changed[:, m + cnt:].any()        # the old rows; behind the new rows up to the pitch
    assert changed[:n, m:m + cnt].all() and changed[n:, :m + cnt].all()
    assert np.array_equal(T0a[n:, :m + cnt], np.eye(cnt, m + cnt, k=m))
    for name in ("A", "rows", "coef"):
        assert not khc.diff_images({name: before[name]}, {name: after[name]})
    assert (after["W"].reshape(case.kmax, case.ld_b)[:, m:m + cnt] == 0.0).all()
    assert (after["R0"].reshape(case.kmax + 1, case.ld_r)[:, n:n + cnt] == 0.0).all()
    assert after["basis"][m:].tolist() == list(range(case.flags.size, case.flags.size + cnt))
    assert after["idcol"][m:].tolist() == list(range(case.n_store, case.n_store + cnt))
    assert (after["pos_of_row"][m:] == -1).all() and (after["pos_of_row"][:m] == kh.SENTINEL_INT).all()
    assert (after["in_basis"][case.flags.size:] == 1).all() and np.array_equal(after["in_basis"][:case.flags.size], case.flags)
    assert after["u"].reshape(cnt, case.kmax)[:, :3].tobytes() == u.tobytes()
    assert (khc.image_bits(after["u"].reshape(cnt, case.kmax)[:, 3:]) == kh.SENTINEL_BITS).all()
    assert case.basic().sum() == 2 and (new[case.basic()] == 0.0).all()
