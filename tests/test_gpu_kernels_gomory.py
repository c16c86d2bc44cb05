"""launch_tab_gomory on the GPU through tests/kernels/harness_gomory.cpp, on the case table of tests/kernel_gomory_cases.py: pi, y, the
status-4 flags and g are bit-equal to the f64 model (tests/kernel_harness_gomory.py), within the gamma(N) bound of the Fraction
value, every input image is unchanged and the sentinels behind every output are intact."""
import pytest

import kernel_harness as kh
from kernel_gomory_cases import BATCH_CASES, CASES

pytestmark = pytest.mark.gpu


def check(case):
    img = case.launch()
    problems = case.compare(img)
    assert not problems, "\n".join(problems)
    n, m = case.n_owned, case.m
    pi = img["pi"][:case.count * n].reshape(case.count, n)
    y = img["y"][:case.count * m].reshape(case.count, m)
    g = img["g"][:case.count * case.nn].reshape(case.count, case.nn)
    assert not case.exact_violations(pi, y, g)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case(name):
    check(CASES[name]())


@pytest.mark.parametrize("batch", kh.BATCHES)
@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_every_load_batch(name, batch):
    check(BATCH_CASES[name](batch))


def test_a_second_launch_gives_the_same_bits():
    case = CASES["mixed, pending rows, bound and cut rows"]()
    first, again = case.launch(), case.launch()
    for name in ("pi", "y", "bad", "g"):
        assert not kh.diff_unchanged(again[name], first[name], name)
