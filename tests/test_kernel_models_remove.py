"""CPU tier of the kernel tests of the rows and columns removed in place: the numpy model of launch_tab_compact that walks an image
IN PLACE in the chunked order of k_tab_drop_rows / k_tab_drop_columns (tests/remove_reference.py) against plain np.delete, bit for
bit over the whole image -- live part, vacated rows and columns, pitch padding and room -- on every case the GPU test runs, for the
shipped B and for B = 1.  It is the hazard argument of relp_kernels.h checked on the host: a walk that read an element after
overwriting it would differ from np.delete.  A deliberately wrong walk (stores before loads) is shown to differ, so the comparison
can fail.  No GPU, no library."""
import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_remove as khr
import remove_reference as rr


@pytest.mark.parametrize("B", khr.BATCHES)
@pytest.mark.parametrize("name", list(khr.CASES))
def test_in_place_model_equals_np_delete(name, B):
    case = khr.CASES[name]
    img = khr.image_of(case, seed=len(name))
    want = rr.expected(img, case["m"], case["n"], case["rows"], case["cols"])
    got = rr.model_compact(img, case["m"], case["n"], case["rows"], case["cols"], B)
    assert not khr.diff_bits(got, want)


def test_expected_keeps_everything_outside_the_live_part():
    case = khr.CASES["rows and columns together"]
    img = khr.image_of(case)
    m, n = case["m"], case["n"]
    want = rr.expected(img, m, n, case["rows"], case["cols"])
    assert np.all(kh.bits(want[n:]) == kh.SENTINEL_BITS) and np.all(kh.bits(want[:, m:]) == kh.SENTINEL_BITS)
    nr, nc = len(case["rows"]), len(case["cols"])
    assert np.all(kh.bits(want[:n, m - nr:m]) == 0) and np.all(kh.bits(want[n - nc:n, :m]) == 0)
    # the survivors keep their order and their bits: row 4 is the old row 4 - 2, column 6 the old column 5
    assert np.array_equal(kh.bits(want[5, 2:698]), kh.bits(img[6, 4:700])) and np.array_equal(kh.bits(want[0, :2]), kh.bits(img[0, :2]))
    assert np.array_equal(kh.bits(rr.expected(img, m, n, [], [])), kh.bits(img))


def test_the_sources_lie_at_or_below_their_destination_and_skip_the_removed_rows():
    rows = [3, 4, 9, 20]
    dst = np.arange(0, 26)
    src = rr.row_sources(30, rows, dst)
    assert src.tolist() == [i for i in range(30) if i not in rows]
    assert np.all(src >= dst)
    assert rr.index_map(6, [1, 4]).tolist() == [0, -1, 1, 2, -1, 3]


def test_a_walk_that_stores_before_it_loads_is_caught():
    """The control: chunks walked from the bottom up overwrite sources of the chunks above them."""
    case = khr.CASES["515 moved rows"]
    m, n, rows = case["m"], case["n"], np.asarray(case["rows"])
    img = khr.image_of(case)
    want = rr.expected(img, m, n, rows, [])
    wrong = img.copy()
    bases = list(range(int(rows[0]), m, rr.THREADS))
    for base in reversed(bases):
        dst = np.arange(base, min(base + rr.THREADS, m))
        moved = dst[dst < m - 1]
        for c in range(n):
            wrong[c, moved] = wrong[c, rr.row_sources(m, rows, moved)]
    assert khr.diff_bits(wrong, want)
