"""launch_tab_add_cuts alone, through tests/kernels/harness_cuts.cpp: single launches on constructed operands with
sentinel-filled images, every returned image compared bit for bit with the model of tests/kernel_harness_cuts.py -- the written rows
and columns, and everything outside them, behind m, n and the pitches, unchanged.

Shapes (m_old, n_store, count, list length, p): (7, 5, 1, 1, 0), (30, 257, 9, 20, 3), (255, 300, 3, 255, 0), (64, 513, 17, 300, 33).
They cover a second and a third cut tile (9, 17 cuts), a partial last tile, a second LDS chunk of the list, more than 256 and
more than 512 columns, p past one load batch of 32, c_lo / col_off > 0, a basic-flagged and a barred column, and each load batch
of kernel_harness.BATCHES.  A list of 300 entries over 64 rows repeats rows, which the engine's lists never do and the kernel does
not mind; "second chunk of the list" is the same path with 300 distinct rows of 320.  Further cases: an empty list while rows are
pending (nothing pending is read), and a full update block of 128 rows."""
import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_cuts as khc

pytestmark = pytest.mark.gpu

CASES = {
    "smallest": dict(m=7, n_store=5, count=1, entries=1, p=0, kmax=1),
    "two tiles, two column blocks": dict(m=30, n_store=257, count=9, entries=20, p=3, kmax=5, basic=(0, 200), barred=(3,)),
    "list of 255": dict(m=255, n_store=300, count=3, entries=255, p=0, kmax=4, basic=(17,), barred=(18,)),
    "three tiles, three column blocks, p 33": dict(m=64, n_store=513, count=17, entries=300, p=33, kmax=40, basic=(5, 300, 512 - 6), barred=(6,)),
    "second chunk of the list": dict(m=320, n_store=40, count=10, entries=300, p=9, kmax=9, basic=(1,), barred=(2,)),
    "owned columns from 3, tableau from 6": dict(m=30, n_store=270, count=9, entries=20, p=3, kmax=5, c_lo=3, col_off=6, basic=(0, 200), barred=(3,)),
    "empty list with rows pending": dict(m=12, n_store=9, count=2, entries=0, p=2, kmax=3),
    "a full update block": dict(m=140, n_store=20, count=8, entries=100, p=128, kmax=128),
}


def run(case):
    want, new, u = case.expected()
    got = case.launch()
    problems = khc.diff_images(got, want)
    assert not problems, "\n".join(problems)
    return got, new, u


@pytest.mark.parametrize("batch", kh.BATCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_image_bit_for_bit(name, batch):
    case = khc.Case(**CASES[name], batch=batch, seed=len(name))
    got, new, u = run(case)
    # a fixed sample of the written entries against the Fraction chain itself
    rng = np.random.default_rng(7)
    T0 = got["T0"].reshape(case.n_owned + case.count, case.ld_t)
    g, basic = case.g_of_column(), case.basic()
    for _ in range(12):
        c, k = int(rng.integers(case.n_owned)), int(rng.integers(case.count))
        want = 0.0 if basic[c] else khc.entry_exact(case.T0, case.W, case.R0, case.rows, case.coef, g[c][k], k, c, u[k])
        assert kh.bits(np.array([T0[c][case.m + k]]))[0] == kh.bits(np.array([want]))[0]


def test_integer_data_is_exact():
    case = khc.Case(**CASES["three tiles, three column blocks, p 33"], integers=True, seed=2)
    got, new, _ = run(case)
    T0, W, R0 = (np.rint(x).astype(np.int64) for x in (case.T0, case.W, case.R0))
    T = T0 + R0.T @ W
    ref = np.rint(case.g_of_column()).astype(np.int64) - T[:, case.rows] @ np.rint(case.coef).astype(np.int64)
    ref[case.basic()] = 0
    assert np.array_equal(got["T0"].reshape(case.n_owned + case.count, case.ld_t)[:case.n_owned, case.m:case.m + case.count], ref.astype(np.float64))


def test_the_same_launch_gives_the_same_bits():
    case = khc.Case(**CASES["two tiles, two column blocks"], seed=9)
    first, second = case.launch(), case.launch()
    assert not khc.diff_images(first, second)


def test_an_image_that_does_not_hold_the_launch_is_refused():
    case = khc.Case(**CASES["smallest"])
    case.ld_t = case.m                                         # no room for the new row
    with pytest.raises(kh.HarnessRefused):
        case.launch()
