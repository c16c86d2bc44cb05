"""launch_tab_trial_copy on the GPU through tests/kernels/harness_trial.cpp: tables of 1, 2 and 32 segments with the lengths 0, 1, 7,
8, 15, 16, 17 and 4,099 bytes, total 16-byte units below the grid and far above it (beyond one stride iteration of the capped
grid).  Every run goes forward (sources -> destinations), then the sources are scrambled and the same table runs backwards; after
each launch the WHOLE image is compared with the expected one, which covers the copied bytes, the 8-byte canaries before and
right behind every destination, the sources and the gaps."""
import numpy as np
import pytest

import kernel_harness_trial as kt

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 7, 8, 15, 16, 17, 4099]


def there_and_back(case):
    got, want = case.launch(case.image, case.src, case.dst)
    assert kt.first_difference(got, want) is None, "forward: " + kt.first_difference(got, want)
    for d, s, n in zip(case.dst, case.src, case.lengths):
        assert np.array_equal(got[d:d + n], case.image[s:s + n])
        assert np.array_equal(got[d - kt.CANARY:d], case.image[d - kt.CANARY:d])
        assert np.array_equal(got[d + n:d + n + kt.CANARY], case.image[d + n:d + n + kt.CANARY])
    scrambled = got.copy()
    for s, n in zip(case.src, case.lengths):
        scrambled[s:s + n] ^= 0xFF
    back, want_back = case.launch(scrambled, case.dst, case.src)
    assert kt.first_difference(back, want_back) is None, "back: " + kt.first_difference(back, want_back)
    assert kt.first_difference(back, got) is None          # the scrambled sources hold their old bytes again, nothing else moved


@pytest.mark.parametrize("length", LENGTHS)
def test_one_segment(length):
    there_and_back(kt.Case([length], seed=length))


@pytest.mark.parametrize("lengths", [(17, 0), (4099, 15), (0, 0), (7, 16), (1, 4099)])
def test_two_segments(lengths):
    there_and_back(kt.Case(lengths, seed=sum(lengths)))


@pytest.mark.parametrize("shift", [0, 3])
def test_thirty_two_segments(shift):
    case = kt.Case([LENGTHS[(s + shift) % len(LENGTHS)] for s in range(32)], seed=shift)
    assert case.units() < kt.grid_units()
    there_and_back(case)


def test_thirty_two_segments_of_tails_alone():
    case = kt.Case([15, 1, 7, 8] * 8, seed=5)
    assert case.units() == 0
    there_and_back(case)


def test_far_above_the_grid():
    # more units than one stride iteration of the capped grid covers (grid x 256 threads x 4 units): the second iteration runs, and
    # the boundary between the segments falls inside a stride
    case = kt.Case([4 * kt.grid_units() * kt.UNIT + 4099, 17, 5 * kt.UNIT * 1000 + 7], seed=9)
    assert case.units() > 4 * kt.grid_units()
    there_and_back(case)
