"""launch_cutpool_separate and launch_cutpool_add_operands alone, through tests/kernels/harness_cutpool.cpp: single
launches on constructed sliced-ELL pools with sentinel-filled images, every returned image compared bit for bit with the model of
tests/kernel_harness_cutpool.py (Fraction fma chains, winners in the total order (key, index)) -- what is written, and everything
outside it, unchanged.

Shapes (rows m, structural columns, pool cuts, longest cut, segments): pools of 1, 63, 64, 65, 257 and 5,000 cuts -- one lane, a
slice short of one lane, one full slice, a second slice, a second chunk of 256 (two chunks per share, folded by k_pool_fold) and
twenty chunks in two shares; (40, 50, 257, 40, 257) every cut its own share and a second round of 256 shares in k_cutpool_winners;
(30, 320, 130, 300, 2) one long cut among short ones (the padding, and eighteen full batches of sixteen loads with a tail);
nr_normal = 1.  The add side: 1, 8 and 9 chosen cuts (the tile of 8 of k_tab_cut_rows), union lists of 0, 1, 256 and 257 rows (the
scan's second round of 256 rows, the second round of 256 staged operands in k_cutpool_chosen), ids descending and from different
slices, a cut without entries alone."""
import numpy as np
import pytest

import kernel_harness as kh
import kernel_harness_cutpool as khc

pytestmark = pytest.mark.gpu

SHAPES = {
    "one cut": (7, 9, 1, 1, 1),
    "a slice short of one lane": (20, 30, 63, 5, 2),
    "one slice": (20, 30, 64, 5, 1),
    "second slice, ragged last share": (20, 30, 65, 5, 3),
    "every cut its own share": (40, 50, 257, 40, 257),
    "two chunks per share": (12, 16, 257, 3, 1),
    "one long cut among short ones": (30, 320, 130, 300, 2),
    "ten chunks per share": (12, 16, 5000, 3, 2),
    "one structural column": (5, 1, 70, 1, 4),
}
TOL = 1e-7


def make(name, seed=None):
    m, nr_normal, count, longest, segments = SHAPES[name]
    rng = np.random.default_rng(len(name) if seed is None else seed)
    long_cut = 17 if count > 17 else 0
    return khc.Case(m, nr_normal, khc.random_cuts(rng, nr_normal, count, longest, long_cut=long_cut), seed=len(name) + 1), segments


def check(got, want):
    problems = khc.diff_images(got, want)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("by_efficacy", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_separate_every_image_bit_for_bit(name, by_efficacy):
    case, segments = make(name)
    s = case.slacks()
    check(case.separate(segments, TOL, by_efficacy), case.separate_expected(segments, TOL, by_efficacy, s=s))
    assert case.count == 1 or ((s < -TOL).any() and (s > 0).any())      # the data has violated cuts and satisfied ones


@pytest.mark.parametrize("name", ["one cut", "second slice, ragged last share", "one long cut among short ones"])
def test_slacks_alone(name):
    case, _ = make(name)
    check(case.separate(0, 0.0), case.separate_expected(0, 0.0))                    # relp_cutpool_slacks: x and s_all only


@pytest.mark.parametrize("by_efficacy", [0, 1])
@pytest.mark.parametrize("longest", [15, 16, 17, 32])
def test_a_chain_of_one_load_batch_one_short_one_over_and_two(longest, by_efficacy):
    """65 cuts over 40 structural columns in three shares: cut 17 has `longest` entries -- one short of a batch of sixteen loads, one
    batch, one over, two batches -- and its last entry stands on the highest structural column, basic with a non-zero value; the
    others have 1 to 5."""
    m, n = 20, 40
    rng = np.random.default_rng(longest)
    cuts = khc.random_cuts(rng, n, 65, longest, long_cut=17)
    cuts[17][-1] = (n - 1, cuts[17][-1][1])
    basis = khc.random_basis(rng, m, n, 10)
    if n - 1 not in basis:
        basis[np.flatnonzero(basis >= n)[0]] = n - 1
    case = khc.Case(m, n, cuts, seed=longest + 1, basis=basis)
    assert len(cuts[17]) == longest and max(len(c) for k, c in enumerate(cuts) if k != 17) <= 5
    assert case.x()[n - 1] != 0.0 and cuts[17][-1][1] != 0.0
    check(case.separate(3, TOL, by_efficacy), case.separate_expected(3, TOL, by_efficacy))


def test_a_cut_without_entries_has_its_rhs_and_padding_adds_nothing():
    rng = np.random.default_rng(3)
    cuts = khc.random_cuts(rng, 30, 70, 5, empty=(0, 7, 64, 69))
    cuts[9] = [(2, -0.0), (-1, 123.0), (11, 1.5)]          # a -0.0 coefficient, then a hole in the middle of a cut
    cuts[10] = [(4, -0.0)]                                  # a -0.0 coefficient next to padding alone
    case = khc.Case(20, 30, cuts, seed=4, pad_value=np.nan)  # every padded value is NaN: one touched entry would poison the chain
    got = case.separate(0, 0.0)
    check(got, case.separate_expected(0, 0.0))
    for k in (0, 7, 64, 69):
        assert kh.bits(got["s_all"][k:k + 1])[0] == kh.bits(case.rhs[k:k + 1])[0]
    assert np.isfinite(got["s_all"]).all()
    for by_efficacy in (0, 1):                              # norms of 0 among the cuts without entries
        check(case.separate(4, TOL, by_efficacy), case.separate_expected(4, TOL, by_efficacy))


def test_every_structural_column_non_basic():
    rng = np.random.default_rng(6)
    m, n = 12, 20
    case = khc.Case(m, n, khc.random_cuts(rng, n, 66, 4), seed=6, basis=np.arange(n, n + m))
    got = case.separate(3, 0.0)
    check(got, case.separate_expected(3, 0.0))
    assert (kh.bits(got["x"]) == kh.bits(np.zeros(n))).all() and (kh.bits(got["s_all"]) == kh.bits(case.rhs)).all()      # x = +0.0: s = rhs - 0.0
    ids = [65, 2, 40]
    got = case.add(ids)                                     # and the union list of an add is empty
    check(got, case.add_expected(ids))
    assert got["entries_out"][0] == 0 and (kh.bits(got["b"][m:]) == kh.bits(case.rhs[ids])).all()


def selection_case(**kw):
    """Integer data, so the slacks are known exactly: cut k is x_{k % 8} <= rhs with x = b = (3, -2, 1, -5, 0, -5, -0.25, 7) negated
    into the slack: s_k = 0 - 1 * x_j."""
    m, count = 8, 200
    cuts = [[(k % m, 1.0)] for k in range(count)]
    b = -np.array([3.0, -2.0, 1.0, -5.0, 0.0, -5.0, -0.25, 7.0])
    return khc.Case(m, m, cuts, seed=5, rhs=np.zeros(count), basis=np.arange(m), b=b, **kw)


def test_the_selection_rule():
    case = selection_case()
    s = case.slacks()
    assert s[3] == -5.0 and s[5] == -5.0 and s[6] == -0.25
    # shares of 50: [0, 50) holds the minimum -5 at 3, 5, 11, 13, ..: the lowest index wins among equal keys
    got = case.separate(4, 0.0)
    check(got, case.separate_expected(4, 0.0))
    assert got["found"][0] == 4 and got["out_k"][:4].tolist() == [3, 51, 101, 155] and (got["out_s"][:4] == -5.0).all()
    # inactive cuts that would have won: every cut with s == -5 off; -2 wins, lowest index again
    case.active[[k for k in range(200) if s[k] == -5.0]] = 0
    got = case.separate(4, 0.0)
    check(got, case.separate_expected(4, 0.0))
    assert got["out_k"][:4].tolist() == [1, 57, 105, 153] and (got["out_s"][:4] == -2.0).all()
    # s == -tol exactly is no candidate: with tol = 2 only the (inactive) -5 are below, so no share has a winner
    got = case.separate(4, 2.0)
    check(got, case.separate_expected(4, 2.0))
    assert got["found"][0] == 0
    # a share without a candidate in front of shares with one: the cuts of the first share are inactive
    case.active[:] = 1
    case.active[0:50] = 0
    got = case.separate(4, 0.25)                           # (-0.25 == -tol: no candidate either)
    check(got, case.separate_expected(4, 0.25))
    assert got["found"][0] == 3 and got["out_k"][:3].tolist() == [51, 101, 155]
    case.rhs[:] = 10.0                                      # nothing is violated at all
    got = case.separate(200, 0.0)
    check(got, case.separate_expected(200, 0.0))
    assert got["found"][0] == 0


def test_efficacy_ranks_by_the_norm_and_a_zero_norm_counts_as_one():
    """Cuts 4 x_1 <= 0 (s = -8, norm 4, key -2), x_1 <= 0 twice (s = -2, key -2), 0 <= -3 (no entries: norm 0, key -3) and
    8 x_3 <= 0 (s = -40, key -5) at x = (.., 2, .., 5, ..)."""
    m = 8
    cuts = [[(1, 4.0)], [(1, 1.0)], [(1, 1.0)], [], [(3, 8.0)]]
    b = np.array([3.0, 2.0, 1.0, 5.0, 0.0, 5.0, 0.25, 7.0])
    case = khc.Case(m, m, cuts, seed=5, rhs=[0.0, 0.0, 0.0, -3.0, 0.0], basis=np.arange(m), b=b)
    assert case.slacks().tolist() == [-8.0, -2.0, -2.0, -3.0, -40.0] and case.norm.tolist() == [4.0, 1.0, 1.0, 0.0, 8.0]
    got = case.separate(1, 0.0, 0)
    check(got, case.separate_expected(1, 0.0, 0))
    assert got["out_k"][0] == 4 and got["out_s"][0] == -40.0
    got = case.separate(1, 0.0, 1)                         # by efficacy: -40 / 8 = -5 still wins, and comes back as the slack
    check(got, case.separate_expected(1, 0.0, 1))
    assert got["out_k"][0] == 4 and got["out_s"][0] == -40.0 and got["part_d"][0] == -5.0
    case.active[4] = 0                                      # then the cut without entries: key -3 / 1
    got = case.separate(1, 0.0, 1)
    check(got, case.separate_expected(1, 0.0, 1))
    assert got["out_k"][0] == 3 and got["out_s"][0] == -3.0
    case.active[3] = 0                                      # then a tie in the key (-8 / 4 == -2 / 1): the lowest index, with its own slack
    got = case.separate(1, 0.0, 1)
    check(got, case.separate_expected(1, 0.0, 1))
    assert got["out_k"][0] == 0 and got["out_s"][0] == -8.0
    case.active[0] = 0
    got = case.separate(1, 0.0, 1)
    check(got, case.separate_expected(1, 0.0, 1))
    assert got["out_k"][0] == 1 and got["out_s"][0] == -2.0
    got = case.separate(1, 2.0, 1)                         # the test is on the slack, not on the key: s == -tol is out
    check(got, case.separate_expected(1, 2.0, 1))
    assert got["found"][0] == 0


def test_an_empty_pool_finds_nothing():
    case = khc.Case(5, 4, [], seed=1)
    got = case.separate(3, 0.0)
    check(got, case.separate_expected(3, 0.0))
    assert got["found"][0] == 0


ADDS = {
    "one cut": ("one cut", [0]),
    "descending ids": ("one slice", [60, 31, 30, 2]),
    "different slices": ("second slice, ragged last share", [64, 3, 40]),
    "eight cuts": ("every cut its own share", [256, 0, 64, 65, 17, 128, 200, 255]),
    "nine cuts over five slices": ("every cut its own share", [256, 0, 64, 65, 17, 128, 200, 255, 1]),
    "the long cut and short ones": ("one long cut among short ones", [129, 17, 64, 5]),
    "one structural column": ("one structural column", [69, 0]),
}


@pytest.mark.parametrize("name", list(ADDS))
def test_add_operands_every_image_bit_for_bit(name):
    shape, ids = ADDS[name]
    case, _ = make(shape)
    check(case.add(ids), case.add_expected(ids))


@pytest.mark.parametrize("entries", [0, 1, 256, 257])
def test_union_lists_at_the_scan_edges(entries):
    """300 rows over 300 structural columns, column j basic in row 299 - j (so ascending columns are descending rows) but for the
    columns 257 .. 299, which are not basic."""
    rng = np.random.default_rng(entries + 1)
    m = n = 300
    basis = np.array([299 - r if 299 - r < 257 else n + r for r in range(m)], dtype=np.int32)
    wide = [(j, float(v)) for j, v in zip(range(256), kh.real_data(rng, 256))]
    cuts = khc.random_cuts(rng, 257, 66, 4)
    cuts[1], cuts[65], cuts[40], cuts[7] = wide, [(3, 2.0)], [(3, 0.5), (256, -3.0), (280, 1.25)], [(270, 1.0), (299, -1.0)]
    case = khc.Case(m, n, cuts, seed=8, basis=basis)
    ids = {0: [7], 1: [65], 256: [1], 257: [40, 1]}[entries]
    assert len(case.add_shape(ids)[0]) == entries
    got = case.add(ids)
    check(got, case.add_expected(ids))
    assert got["entries_out"][0] == entries
    check(case.add(ids, room=min(entries + 5, m)), case.add_expected(ids, room=min(entries + 5, m)))      # a bound that is not tight


def test_a_cut_without_entries_alone_is_added():
    rng = np.random.default_rng(2)
    case = khc.Case(9, 6, khc.random_cuts(rng, 6, 3, 2, empty=(1,)), seed=2)
    got = case.add([1])
    check(got, case.add_expected([1]))
    assert got["entries_out"][0] == 0 and kh.bits(got["b"][9:])[0] == kh.bits(case.rhs[1:2])[0]


def test_the_same_launch_gives_the_same_bits():
    case, segments = make("second slice, ragged last share")
    check(case.separate(segments, TOL, 1), case.separate(segments, TOL, 1))
    check(case.add([64, 3, 40]), case.add([64, 3, 40]))


def test_an_image_that_does_not_hold_the_launch_is_refused():
    case, segments = make("second slice, ragged last share")
    for short in ("col", "val", "rhs", "norm", "active", "basis", "x", "s_all", "part_d", "out_k", "out_s", "found"):
        with pytest.raises(kh.HarnessRefused):
            case.separate(segments, TOL, lengths={short: case.separate_images(segments)[short].size - 1})
    with pytest.raises(kh.HarnessRefused):
        case.separate(66, TOL)                            # more shares than cuts
    with pytest.raises(kh.HarnessRefused):
        case.separate(segments, TOL, 2)
    ids = [64, 3, 40]
    for short in ("mark", "coef", "A", "b", "entries_out"):
        with pytest.raises(kh.HarnessRefused):
            case.add(ids, lengths={short: case.add_images(ids)[short].size - 1})
    with pytest.raises(kh.HarnessRefused):
        case.add(ids, room=len(case.add_shape(ids)[0]) - 1)      # a union list longer than the caller's bound: coef would not hold it
    with pytest.raises(kh.HarnessRefused):
        case.add(ids, longest=case.add_shape(ids)[2] - 1)
    with pytest.raises(kh.HarnessRefused):
        case.add([3, 3])
    with pytest.raises(kh.HarnessRefused):
        case.add([65])
    bad = khc.Case(5, 30, [[(30, 1.0)]], seed=1)           # a column behind the structural ones
    with pytest.raises(kh.HarnessRefused):
        bad.separate(1, 0.0)
    twice = khc.Case(5, 30, [[(3, 1.0)]], seed=1, basis=[3, 40, 3, 41, 42])      # a column basic in two rows
    with pytest.raises(kh.HarnessRefused):
        twice.separate(1, 0.0)
