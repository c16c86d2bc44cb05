"""launch_tab_add_columns alone, through tests/kernels/harness_columns.cpp: single launches on constructed operands
with sentinel-filled images, every returned image compared bit for bit with the model of tests/kernel_harness_columns.py -- the
written columns, and everything outside them, behind m, n and the pitches, unchanged.

Shapes (m, n_store, count, list length, p): (7, 5, 1, 1, 0), (30, 257, 9, 20, 3) with a second tile, (255, 300, 3, 255, 0),
(320, 40, 10, 300, 9) with a second LDS chunk of the list and more than 256 rows, (64, 513, 17, 64, 33) with three tiles and p
past one load batch of 32; an empty list while rows are pending, a full update block of 128 rows, c_lo / col_off > 0, and each
load batch of kernel_harness.BATCHES.  A list of 300 entries over 40 columns repeats columns, which the engine's lists never do
and the kernel does not mind.  The list is not cut into shares, so there is no case with more than one."""
import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_columns as khc

pytestmark = pytest.mark.gpu

CASES = {
    "smallest": dict(m=7, n_store=5, count=1, entries=1, p=0, kmax=1),
    "two tiles": dict(m=30, n_store=257, count=9, entries=20, p=3, kmax=5),
    "list of 255": dict(m=255, n_store=300, count=3, entries=255, p=0, kmax=4),
    "second chunk of the list, two row blocks": dict(m=320, n_store=40, count=10, entries=300, p=9, kmax=9),
    "three tiles, p 33": dict(m=64, n_store=513, count=17, entries=64, p=33, kmax=40),
    "owned columns from 3, tableau from 6": dict(m=30, n_store=270, count=9, entries=20, p=3, kmax=5, c_lo=3, col_off=6),
    "empty list with rows pending": dict(m=12, n_store=9, count=2, entries=0, p=2, kmax=3),
    "a full update block": dict(m=140, n_store=20, count=8, entries=100, p=128, kmax=128),
}


def run(case):
    want, new = case.expected()
    got = case.launch()
    problems = khc.diff_images(got, want)
    assert not problems, "\n".join(problems)
    return got, new


@pytest.mark.parametrize("batch", kh.BATCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_image_bit_for_bit(name, batch):
    case = khc.Case(**CASES[name], batch=batch, seed=len(name))
    got, new = run(case)
    # a fixed sample of the written entries against the Fraction chain itself
    rng = np.random.default_rng(7)
    T0 = got["T0"].reshape(case.n_owned + case.count, case.ld_t)
    for _ in range(12):
        k, i = int(rng.integers(case.count)), int(rng.integers(case.m))
        want = khc.entry_exact(case.T0, case.cols, case.coef, k, i, case.c_lo)
        assert kh.bits(np.array([T0[case.n_owned + k][i]]))[0] == kh.bits(np.array([want]))[0]


def test_integer_data_is_exact():
    case = khc.Case(**CASES["three tiles, p 33"], integers=True, seed=2)
    got, _ = run(case)
    T0, coef = np.rint(case.T0).astype(np.int64), np.rint(case.coef).astype(np.int64)
    ref = coef.T @ T0[case.cols - case.c_lo]
    assert np.array_equal(got["T0"].reshape(case.n_owned + case.count, case.ld_t)[case.n_owned:, :case.m], ref.astype(np.float64))
    R0 = got["R0"].reshape(case.kmax + 1, case.ld_r)
    assert np.array_equal(R0[:case.p, case.n_owned:case.n_owned + case.count], ref[:, case.S].T.astype(np.float64))


def test_the_same_launch_gives_the_same_bits():
    case = khc.Case(**CASES["two tiles"], seed=9)
    first, second = case.launch(), case.launch()
    assert not khc.diff_images(first, second)


def test_an_image_that_does_not_hold_the_launch_is_refused():
    case = khc.Case(**CASES["smallest"])
    case.ld_r = case.n_owned                                   # no room for the new column in R0
    with pytest.raises(kh.HarnessRefused):
        case.launch()
