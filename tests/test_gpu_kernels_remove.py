"""launch_tab_compact alone, through tests/kernels/harness_remove.cpp: single launches on sentinel-filled images, the
returned image compared bit for bit with np.delete on its live part (tests/remove_reference.py: expected) -- the survivors in order
with their bits, 0.0 in the vacated rows and columns, and the pitch padding, the room rows and the room columns untouched.

Cases (tests/kernel_harness_remove.py: CASES), each for the shipped B = 4 and for B = 1: one removed row with 1, 255, 256, 257, 515,
1023, 1025 and 2051 rows to move under it (one chunk is 256 B rows: 256 B - 1, 256 B + 1 and 2 * 256 B + 3 for both B); the first
row, the last row, two adjacent rows, every other row of the last 9, 70 scattered rows, every row; 2,100 columns (more than the
2,048 workgroups of a launch); the first column of a tail, the last column, adjacent columns, 1, 8 and 9 columns at once, every
column, with 63, 64, 65 and 257 rows (workgroups of 64 rows); rows and columns together; empty lists."""
import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_remove as khr
import remove_reference as rr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", khr.BATCHES)
@pytest.mark.parametrize("name", list(khr.CASES))
def test_the_image_bit_for_bit(name, B):
    case = khr.CASES[name]
    img = khr.image_of(case, seed=len(name))
    want = rr.expected(img, case["m"], case["n"], case["rows"], case["cols"])
    got = khr.launch(img, case["m"], case["n"], case["rows"], case["cols"], batch=B)
    problem = khr.diff_bits(got, want)
    assert not problem, problem


def test_empty_lists_leave_every_word():
    case = khr.CASES["nothing"]
    img = khr.image_of(case)
    got = khr.launch(img, case["m"], case["n"], [], [])
    assert np.array_equal(kh.bits(got), kh.bits(img))


def test_the_same_launch_gives_the_same_bits():
    case = khr.CASES["rows and columns together"]
    img = khr.image_of(case, seed=3)
    first, second = (khr.launch(img, case["m"], case["n"], case["rows"], case["cols"]) for _ in range(2))
    assert np.array_equal(kh.bits(first), kh.bits(second))


def test_a_list_outside_the_image_is_refused():
    case = khr.CASES["nothing"]
    img = khr.image_of(case)
    for rows, cols in (([20], []), ([], [6]), ([3, 3], []), ([], [4, 2])):
        with pytest.raises(kh.HarnessRefused):
            khr.launch(img, case["m"], case["n"], rows, cols)
