"""launch_pool_price, launch_pool_add_operands and launch_pool_set_active alone, through tests/kernels/harness_pool.cpp:
single launches on constructed sliced-ELL pools with sentinel-filled images, every returned image compared bit for bit with the
model of tests/kernel_harness_pool.py (Fraction fma chains, winners in the total order (d, index)) -- what is written, and everything
outside it, unchanged.

Shapes (m, pool columns, longest column, segments): (7, 1, 1, 1); (30, 64, 5, 1) one full slice; (30, 65, 5, 3) a second slice and a
ragged last share; (40, 257, 40, 257) every column its own share, and a second round of 256 shares in k_pool_winners; (320, 130,
300, 2) one long column among short ones; (12, 5000, 3, 2) and (12, 257, 3, 1): shares cut into ten and into two chunks of 256
columns, folded by k_pool_fold, the only other path of the launch.  The add side: ids descending and from different slices, a
chosen column of 300 entries (a second round of 256 in k_pool_chosen), union lists of 1, 256 and 257 entries (the scan's second round
of 256 rows), an empty column alone."""
import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_pool as khp

pytestmark = pytest.mark.gpu

SHAPES = {
    "one column": (7, 1, 1, 1),
    "one slice": (30, 64, 5, 1),
    "second slice, ragged last share": (30, 65, 5, 3),
    "every column its own share": (40, 257, 40, 257),
    "one long column among short ones": (320, 130, 300, 2),
    "ten chunks per share": (12, 5000, 3, 2),
    "one column into the second chunk": (12, 257, 3, 1),
}
TOL = 1e-7


def make(name, seed=None):
    m, count, longest, segments = SHAPES[name]
    rng = np.random.default_rng(len(name) if seed is None else seed)
    long_column = 17 if count > 17 else 0
    return khp.Case(m, khp.random_columns(rng, m, count, longest, long_column=long_column), seed=len(name) + 1), segments


def check(got, want):
    problems = khp.diff_images(got, want)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("name", list(SHAPES))
def test_price_every_image_bit_for_bit(name):
    case, segments = make(name)
    check(case.price(segments, TOL), case.price_expected(segments, TOL))
    d = case.reduced_costs()
    assert case.count == 1 or ((d < -TOL).any() and (d > 0).any())      # the data has candidates and non-candidates


@pytest.mark.parametrize("name", ["one column", "second slice, ragged last share", "one long column among short ones"])
def test_reduced_costs_alone_and_price_without_the_vector(name):
    case, segments = make(name)
    check(case.price(0, 0.0), case.price_expected(0, 0.0))                          # relp_pool_reduced_costs: d_all only
    check(case.price(segments, TOL, write_d=False), case.price_expected(segments, TOL, write_d=False))     # relp_pool_price: no d_all


@pytest.mark.parametrize("longest", [15, 16, 17, 32])
def test_a_chain_of_one_load_batch_one_short_one_over_and_two(longest):
    """65 columns over 40 rows in three shares: column 17 has `longest` entries -- one short of a batch of sixteen loads, one batch,
    one over, two batches -- and its last entry stands in the highest row with a non-zero multiplier there; the others have 1 to 5."""
    m = 40
    rng = np.random.default_rng(longest)
    columns = khp.random_columns(rng, m, 65, longest, long_column=17)
    columns[17][-1] = (m - 1, columns[17][-1][1])
    case = khp.Case(m, columns, seed=longest + 1)
    assert len(columns[17]) == longest and max(len(c) for k, c in enumerate(columns) if k != 17) <= 5
    assert case.mpi[m - 1] != 0.0 and columns[17][-1][1] != 0.0
    check(case.price(3, TOL), case.price_expected(3, TOL))


def test_an_empty_column_prices_at_its_cost_and_padding_adds_nothing():
    rng = np.random.default_rng(3)
    columns = khp.random_columns(rng, 30, 70, 5, empty=(0, 7, 64, 69))
    columns[9] = [(2, -0.0), (-1, 123.0), (11, 1.5)]       # a -0.0 coefficient, then a hole in the middle of a column
    case = khp.Case(30, columns, seed=4, pad_value=np.nan)  # every padded value is NaN: one touched entry would poison the chain
    got = case.price(0, 0.0)
    check(got, case.price_expected(0, 0.0))
    for k in (0, 7, 64, 69):
        assert kh.bits(got["d_all"][k:k + 1])[0] == kh.bits(case.cost[k:k + 1])[0]
    assert np.isfinite(got["d_all"]).all()
    check(case.price(4, TOL), case.price_expected(4, TOL))


def test_the_selection_rule():
    """Integer data, so the reduced costs are known exactly: d = cost + (-pi)_row * 1."""
    m, count = 8, 200
    columns = [[(k % m, 1.0)] for k in range(count)]
    case = khp.Case(m, columns, n_store=m, seed=5, cost=np.zeros(count))
    case.idcol = np.arange(m, dtype=np.int32)
    case.cost_store = np.zeros(m)
    case.d = np.array([3.0, -2.0, 1.0, -5.0, 0.0, -5.0, -0.25, 7.0])
    case.mpi = khp.minus_pi(case.d, case.cost_store, case.idcol)
    d = case.reduced_costs()
    assert d[3] == -5.0 and d[5] == -5.0 and d[6] == -0.25
    # shares of 50: [0, 50) holds the minimum -5 at 3, 5, 11, 13, ..: the lowest index wins
    got = case.price(4, 0.0)
    check(got, case.price_expected(4, 0.0))
    assert got["found"][0] == 4 and got["out_k"][:4].tolist() == [3, 51, 101, 155] and (got["out_d"][:4] == -5.0).all()
    # inactive columns that would have won: every column with d == -5 off; -2 wins, lowest index again
    case.active[[k for k in range(count) if d[k] == -5.0]] = 0
    got = case.price(4, 0.0)
    check(got, case.price_expected(4, 0.0))
    assert got["out_k"][:4].tolist() == [1, 57, 105, 153] and (got["out_d"][:4] == -2.0).all()
    # d == -tol exactly is no candidate: with tol = 2 only the (inactive) -5 are below, so no share has a winner
    got = case.price(4, 2.0)
    check(got, case.price_expected(4, 2.0))
    assert got["found"][0] == 0
    # a share without a candidate in front of shares with one: the columns of the first share are inactive
    case.active[:] = 1
    case.active[0:50] = 0
    got = case.price(4, 0.25)                             # (-0.25 == -tol: no candidate either)
    check(got, case.price_expected(4, 0.25))
    assert got["found"][0] == 3 and got["out_k"][:3].tolist() == [51, 101, 155]
    case.cost[:] = 10.0                                    # nothing prices out at all
    got = case.price(200, 0.0)
    check(got, case.price_expected(200, 0.0))
    assert got["found"][0] == 0


def test_an_empty_pool_finds_nothing():
    case = khp.Case(5, [], seed=1)
    got = case.price(3, 0.0, write_d=False)
    check(got, case.price_expected(3, 0.0, write_d=False))
    assert got["found"][0] == 0


ADDS = {
    "one column": ("one column", [0]),
    "descending ids": ("one slice", [60, 31, 30, 2]),
    "different slices": ("second slice, ragged last share", [64, 3, 40]),
    "nine columns over four slices": ("every column its own share", [256, 0, 64, 65, 17, 128, 200, 255, 1]),
    "the long column and short ones": ("one long column among short ones", [129, 17, 64, 5]),
}


@pytest.mark.parametrize("name", list(ADDS))
def test_add_operands_every_image_bit_for_bit(name):
    shape, ids = ADDS[name]
    case, _ = make(shape)
    check(case.add(ids), case.add_expected(ids))


@pytest.mark.parametrize("entries", [1, 256, 257])
def test_union_lists_at_the_scan_edges(entries):
    rng = np.random.default_rng(entries)
    m = 300
    wide = [(r, float(v)) for r, v in zip(range(256), kh.real_data(rng, 256))]
    columns = khp.random_columns(rng, m, 66, 4)
    columns[1], columns[65], columns[40] = wide, [(299, 2.0)], [(256, -3.0), (3, 0.5)][::-1]
    case = khp.Case(m, columns, seed=8)
    ids = {1: [65], 256: [1], 257: [40, 1]}[entries]
    assert len(case.add_shape(ids)[0]) == entries
    check(case.add(ids), case.add_expected(ids))


def test_an_empty_column_alone_is_added():
    rng = np.random.default_rng(2)
    case = khp.Case(9, khp.random_columns(rng, 9, 3, 2, empty=(1,)), seed=2)
    got = case.add([1])
    check(got, case.add_expected([1]))
    assert got["entries_out"][0] == 0 and kh.bits(got["d_new"])[0] == kh.bits(case.cost[1:2])[0]


def test_set_active():
    active = np.array([1, 0, 1, 1, 0, 2, 1], dtype=np.uint8)
    got = khp.set_active(active, [4, 0, 5], 1)
    assert got["active"].tolist() == [1, 0, 1, 1, 1, 1, 1] and got["ids"].tolist() == [4, 0, 5]
    assert khp.set_active(active, [2], 0)["active"].tolist() == [1, 0, 0, 1, 0, 2, 1]


def test_the_same_launch_gives_the_same_bits():
    case, segments = make("second slice, ragged last share")
    check(case.price(segments, TOL), case.price(segments, TOL))
    check(case.add([64, 3, 40]), case.add([64, 3, 40]))


def test_an_image_that_does_not_hold_the_launch_is_refused():
    case, segments = make("second slice, ragged last share")
    for short in ("row", "val", "cost", "active", "d", "idcol", "d_all", "part_d", "out_k", "out_d", "found"):
        with pytest.raises(kh.HarnessRefused):
            case.price(segments, TOL, lengths={short: case.price_images(segments)[short].size - 1})
    with pytest.raises(kh.HarnessRefused):
        case.price(66, TOL)                               # more shares than columns
    ids = [64, 3, 40]
    for short in ("rank", "coef", "col_a", "d_new", "cost_new", "entries_out"):
        with pytest.raises(kh.HarnessRefused):
            case.add(ids, lengths={short: case.add_images(ids)[short].size - 1})
    with pytest.raises(kh.HarnessRefused):
        case.add(ids, entries=len(case.add_shape(ids)[0]) - 1)      # a union list longer than the caller said: coef would not hold it
    with pytest.raises(kh.HarnessRefused):
        case.add(ids, longest=case.add_shape(ids)[1] - 1)
    with pytest.raises(kh.HarnessRefused):
        case.add([3, 3])
    with pytest.raises(kh.HarnessRefused):
        case.add([65])
    bad = khp.Case(30, [[(30, 1.0)]], seed=1)              # a row behind the engine's rows
    with pytest.raises(kh.HarnessRefused):
        bad.price(1, 0.0)
