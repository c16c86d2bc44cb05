"""CPU tier of the kernel tests: the harness refuses bad calls before any HIP call, the reference fma is right, the models of
tests/kernel_harness.py agree with each other, and every comparison function reports a result that is wrong by one term, one
word, one swapped pair of columns or one sign of zero.  For T5 - T8 (the in-place changes and the batched ratio queries) also: the
host functions that choose the number of splits, the tree order of the pending sums, and that no case of the shared tables
(tests/kernel_query_cases.py) depends on how the compiler rounds a tie band's bound.  No kernel runs here and no product code is
altered."""
from fractions import Fraction

import numpy as np
import pytest

import kernel_harness as kh
import kernel_query_cases as kq


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _tab(m=5, n=7, p=2, seed=0):
    rng = np.random.default_rng(seed)
    return kh.real_data(rng, (n, m)), kh.real_data(rng, (p, m)), kh.real_data(rng, (p, n))


def _refused(code, fn, *a, **k):
    with pytest.raises(kh.HarnessRefused) as e:
        fn(*a, **k)
    assert e.value.code == code
    assert kh.load().rkh_sticky_error() == 0, "a refusal must come before any HIP call"


def test_refusals_tab_flush():
    T0, W, R0 = _tab()
    _refused(kh.REFUSED_SHAPE, kh.tab_flush, T0, W, R0, kmax=1)                       # p > kmax
    _refused(kh.REFUSED_SHAPE, kh.tab_flush, T0, W, R0, kmax=129)                     # kmax > 128
    _refused(kh.REFUSED_SHAPE, kh.tab_flush, np.zeros((0, 5)), np.zeros((0, 5)), np.zeros((0, 0)), kmax=4)   # n_owned < 1
    _refused(kh.REFUSED_SHAPE, kh.tab_flush, np.zeros((3, 0)), np.zeros((0, 0)), np.zeros((0, 3)), kmax=4)   # m < 1
    _refused(kh.REFUSED_INDEX, kh.tab_flush, T0, W, R0, kmax=4, c_lo=-1)
    _refused(kh.REFUSED_LENGTH, kh.tab_flush, T0, W, R0[:, :-1], kmax=4)
    _refused(kh.REFUSED_LENGTH, kh.tab_flush, T0, W, R0, kmax=4, lengths=dict(T0=7 * 5))     # the image has pitch 6
    _refused(kh.REFUSED_LENGTH, kh.tab_flush, T0, W, R0, kmax=4, lengths=dict(R0=4 * 8))     # R0 has kmax + 1 rows
    _refused(kh.REFUSED_LENGTH, kh.tab_flush, T0, W, R0, kmax=4, lengths=dict(cols=6))


def test_refusals_tab_vector():
    T0, W, R0 = _tab()
    _refused(kh.REFUSED_SHAPE, kh.tab_vector, T0, W, R0, kmax=1)
    _refused(kh.REFUSED_INDEX, kh.tab_vector, T0, W, R0, kmax=4, q=7)
    _refused(kh.REFUSED_INDEX, kh.tab_vector, T0, W, R0, kmax=4, q=-1)
    _refused(kh.REFUSED_INDEX, kh.tab_vector, T0, W, R0, kmax=4, row=5)
    for batch in (0, 2, 4, 7, 9, 64):
        _refused(kh.REFUSED_BATCH, kh.tab_vector, T0, W, R0, kmax=4, batch=batch)
    _refused(kh.REFUSED_LENGTH, kh.tab_vector, T0, W, R0, kmax=4, lengths=dict(vec=5))       # alpha has ld_b entries
    _refused(kh.REFUSED_LENGTH, kh.tab_vector, T0, W, R0, kmax=4, row=1, lengths=dict(vec=7))
    _refused(kh.REFUSED_LENGTH, kh.tab_vector, T0, W[:, :-1], R0, kmax=4)


def test_refusals_tab_update_all():
    T0, W, R0 = _tab()
    rng = np.random.default_rng(1)
    kw = dict(S=[0, 3], d=kh.real_data(rng, 7), in_basis=np.zeros(7, np.uint8), alpha=kh.real_data(rng, 5), b=kh.real_data(rng, 5),
              basis=np.arange(5), kmax=4, r=1, q=2)
    args = (T0, W, R0)
    _refused(kh.REFUSED_SHAPE, kh.tab_update_all, *args, **{**kw, "kmax": 1})
    _refused(kh.REFUSED_SHAPE, kh.tab_update_all, *args, **{**kw, "kmax": 2})         # r is new and W has no free column
    _refused(kh.REFUSED_INDEX, kh.tab_update_all, *args, **{**kw, "r": 5})
    _refused(kh.REFUSED_INDEX, kh.tab_update_all, *args, **{**kw, "q": 7})
    _refused(kh.REFUSED_INDEX, kh.tab_update_all, *args, **{**kw, "S": [0, 0]})       # not distinct
    _refused(kh.REFUSED_INDEX, kh.tab_update_all, *args, **{**kw, "S": [0, 5]})
    _refused(kh.REFUSED_INDEX, kh.tab_update_all, *args, **kw, leaving=7)             # neither a column nor a wrapped artificial
    _refused(kh.REFUSED_INDEX, kh.tab_update_all, *args, **kw, last_selected=7)
    _refused(kh.REFUSED_BATCH, kh.tab_update_all, *args, **kw, batch=4)
    _refused(kh.REFUSED_LENGTH, kh.tab_update_all, *args, **{**kw, "alpha": np.ones(4)})
    _refused(kh.REFUSED_LENGTH, kh.tab_update_all, *args, **kw, lengths=dict(trace=8))
    _refused(kh.REFUSED_LENGTH, kh.tab_update_all, *args, **kw, lengths=dict(k1=2))


def test_refusals_revised():
    rng = np.random.default_rng(2)
    m, p = 6, 3
    W, Binv, v = kh.real_data(rng, (p, m)), kh.real_data(rng, (m, m)), kh.real_data(rng, m)
    S = [4, 0, 2]
    _refused(kh.REFUSED_SHAPE, kh.apply_w, W, S, v, kmax=2)
    _refused(kh.REFUSED_SHAPE, kh.apply_w, W, S, v, kmax=200)
    _refused(kh.REFUSED_INDEX, kh.apply_w, W, [4, 0, 6], v, kmax=4)
    _refused(kh.REFUSED_INDEX, kh.apply_w, W, [4, 4, 2], v, kmax=4)
    _refused(kh.REFUSED_LENGTH, kh.apply_w, W, S, v[:-1], kmax=4)
    _refused(kh.REFUSED_LENGTH, kh.apply_w, W, S, v, kmax=4, lengths=dict(alpha=6))
    _refused(kh.REFUSED_SHAPE, kh.eta_update_w, W, S, v, kmax=3, r=1)                 # r is new and W is full
    _refused(kh.REFUSED_INDEX, kh.eta_update_w, W, S, v, kmax=4, r=6)
    _refused(kh.REFUSED_LENGTH, kh.eta_update_w, W, S, v, kmax=4, r=1, lengths=dict(wr=3))
    _refused(kh.REFUSED_SHAPE, kh.rho_deferred, W, S, Binv, kmax=2, r=0)
    _refused(kh.REFUSED_INDEX, kh.rho_deferred, W, S, Binv, kmax=4, r=-1)
    _refused(kh.REFUSED_LENGTH, kh.rho_deferred, W, S, Binv[:, :-1], kmax=4, r=0)
    _refused(kh.REFUSED_SHAPE, kh.flush_revised, W, S, Binv, kmax=2)
    _refused(kh.REFUSED_INDEX, kh.flush_revised, W, [0, 1, -1], Binv, kmax=4)
    _refused(kh.REFUSED_LENGTH, kh.flush_revised, W, S, Binv, kmax=4, lengths=dict(R=4 * 6))
    _refused(kh.REFUSED_SHAPE, kh.explicit_update, np.zeros((0, 0)), np.zeros(0), r=0)
    _refused(kh.REFUSED_INDEX, kh.explicit_update, Binv, v, r=6)
    _refused(kh.REFUSED_LENGTH, kh.explicit_update, Binv, v[:-1], r=0)
    _refused(kh.REFUSED_LENGTH, kh.explicit_update, Binv, v, r=0, lengths=dict(Binv=36))


# ---- the fma -------------------------------------------------------------------------------------------------------------
def test_fma_exact_hand_computed_cases():
    e = 2.0 ** -52
    # (1 + e)(1 - e) = 1 - e^2 exactly; plain multiplication rounds it to 1, so a * b - 1 gives 0 and the fma gives -e^2
    assert kh.fma_exact(1 + e, 1 - e, -1.0) == -(2.0 ** -104)
    assert (1 + e) * (1 - e) - 1.0 == 0.0
    # a halfway case: 1 + 2^-53 rounds to even (1), 1 + 2^-53 + 2^-105 rounds up
    assert kh.fma_exact(2.0 ** -53, 1.0, 1.0) == 1.0
    assert kh.fma_exact(2.0 ** -53, 1 + e, 1.0) == 1 + e
    assert kh.fma_exact(3.0, 5.0, 7.0) == 22.0
    assert kh.fma_exact(0.1, 10.0, -1.0) == float(Fraction(0.1) * 10 - 1) == 2.0 ** -54
    # signed zeros
    z = lambda x: (x, bool(np.signbit(x)))
    assert z(kh.fma_exact(0.0, 5.0, -0.0)) == (0.0, False)          # (+0) + (-0) = +0
    assert z(kh.fma_exact(-0.0, 5.0, -0.0)) == (0.0, True)          # (-0) + (-0) = -0
    assert z(kh.fma_exact(2.0, 0.0, -0.0)) == (0.0, False)          # the documented fma(u, 0.0, -0.0) = +0.0
    assert z(kh.fma_exact(2.0, 3.0, -6.0)) == (0.0, False)          # exact cancellation = +0
    assert kh.fma_exact(0.0, 5.0, 3.5) == 3.5


def test_fma_vec_equals_fma_exact_bit_for_bit():
    rng = np.random.default_rng(20260001)
    n = 30000
    a, b, c = (kh.real_data(rng, n, 0.05, 0.05) for _ in range(3))
    k = n // 3
    c[:k] = -(a[:k] * b[:k]) * (1 + rng.integers(-2, 3, k) * 2.0 ** -52)          # near and exact cancellation
    a[k:2 * k] = np.round(a[k:2 * k] * 2 ** 26) / 2 ** 26                          # short factors: exact products, halfway sums
    b[k:2 * k] = np.round(b[k:2 * k] * 2 ** 26) / 2 ** 26 + 2.0 ** -27
    c[k:2 * k] *= 2.0 ** rng.integers(-60, 60, k)
    got = kh.fma_vec(a, b, c)
    want = np.array([kh.fma_exact(x, y, w) for x, y, w in zip(a, b, c)])
    assert not kh.diff_bits(got, want)


# ---- the models agree with each other ---------------------------------------------------------------------------------------
def test_flush_models_agree():
    rng = np.random.default_rng(3)
    m, n, p = 37, 21, 9
    T0, W, R0 = kh.int_data(rng, (n, m)), kh.int_data(rng, (p, m)), kh.int_data(rng, (p, n))
    want = kh.model_flush_int(T0, W, R0)
    # the chain model of a column (T2) and of a row (T3) is exact on integers too
    for q in (0, n - 1):
        assert not kh.diff_values(kh.model_tab_column(T0, W, R0, q), want[q])
    for i in (0, m - 1):
        assert not kh.diff_values(kh.model_tab_row(T0, W, R0, i), want[:, i])
    # the rational model, entry by entry
    for c, i in kh.flush_sample(m, n, 5, count=50):
        t, s = kh.flush_exact_entry(T0, W, R0, c, i)
        assert t == Fraction(float(want[c, i])) and s >= abs(t)
    bad, worst = kh.flush_real_check(want, T0, W, R0, kh.flush_sample(m, n, 5, count=50))
    assert not bad and worst == 0.0
    # the selector: written down directly against the integer product
    for pp in (0, 1, 5, 9):
        Ws, Rs = kh.selector_operands(m, n, pp)
        assert not kh.diff_values(kh.model_flush_int(T0, Ws, Rs) - T0, kh.model_flush_selector(m, n, pp))
    # real data: the fma chain stays within the flush's a-priori bound of the exact value
    T0, W, R0 = kh.real_data(rng, (n, m)), kh.real_data(rng, (p, m)), kh.real_data(rng, (p, n))
    chain = np.stack([kh.model_tab_column(T0, W, R0, q) for q in range(n)])
    bad, worst = kh.flush_real_check(chain, T0, W, R0, kh.flush_sample(m, n, 6, count=50))
    assert not bad and 0.0 < worst < 2 * p + 1
    assert chain[3, 4] == kh.chain_exact(T0[3, 4], W[:, 4], R0[:, 3])


def test_revised_models_agree():
    rng = np.random.default_rng(4)
    m, p = 19, 6
    W, Binv = kh.int_data(rng, (p, m)), kh.int_data(rng, (m, m))
    S = kh.distinct_rows(rng, m, p)
    v = kh.int_data(rng, m)
    Wi, Bi = W.astype(np.int64), Binv.astype(np.int64)
    assert not kh.diff_values(kh.model_apply_w(W, S, v), (v.astype(np.int64) + Wi.T @ v.astype(np.int64)[S]).astype(float))
    new, R = kh.model_flush_revised(W, S, Binv)
    assert not kh.diff_values(new, (Bi + Wi.T @ Bi[S]).astype(float))
    r = int(S[2])
    assert not kh.diff_values(kh.model_rho_deferred(W, S, Binv, r), (Bi[r] + Wi[:, r] @ Bi[S]).astype(float))
    # (I + W S') after one more pivot = E (I + W S'): the model of the W update against the definition
    alpha = kh.int_data(rng, m, zeros=0.3)
    for r in (int(S[1]), int(np.setdiff1d(np.arange(m), S)[0])):
        alpha[r] = 4.0                                                               # 1 / 4 and a / 4 are exact
        mod = kh.model_eta_update_w(W, S, alpha, r)
        M = np.eye(m)
        M[:, S] += W.T
        u = -alpha / alpha[r]
        u[r] = 1.0 / alpha[r] - 1.0
        E = np.eye(m)
        E[:, r] += u
        Mn = np.eye(m)
        Mn[:, mod["S"]] += mod["W"].T
        assert not kh.diff_values(Mn, E @ M)
    out, rho = kh.model_explicit_update(Binv, alpha, r)
    E = np.eye(m)
    E[:, r] += u
    assert not kh.diff_values(out, E @ Binv)


def test_update_all_model_against_definitions():
    rng = np.random.default_rng(5)
    m, n, p = 9, 300, 3
    T0, W, R0 = kh.int_data(rng, (n, m)), kh.int_data(rng, (p, m)), kh.int_data(rng, (p, n))
    S = [2, 7, 4]
    R0[:] = (T0[:, S]).T                                                                # R0 = S' T0
    alpha, b, d = kh.int_data(rng, m), kh.int_data(rng, m), kh.int_data(rng, n, zeros=0.0) - 20.0
    r, q = 5, 17
    alpha[r], d[q] = 4.0, -8.0
    T = kh.model_flush_int(T0, W, R0)
    mod = kh.model_tab_update_all(T0, W, R0, S, d, np.zeros(n, np.uint8), alpha, b, np.arange(m), r, q, rule=2, leaving=3)
    assert mod["jt"] == 3 and mod["n_eta"] == 4 and list(mod["S"]) == S + [r]
    assert not kh.diff_values(mod["R0"][3], T0[:, r])
    assert not kh.diff_values(mod["d"], np.where(np.arange(n) == q, 0.0, d - (d[q] / alpha[r]) * T[:, r]))
    for blk in range(2):
        cand = [(mod["d"][c], c) for c in range(blk * 256, min(n, blk * 256 + 256)) if c != q and mod["d"][c] < -1e-9]
        assert (mod["k1"][blk], mod["j"][blk]) == min(cand)
    assert mod["b"][r] == b[r] / 4.0 and mod["basis"][r] == q and mod["in_basis"][q] == 1
    # rule 1 with memory: keys are distances from last_selected in the search order
    mod = kh.model_tab_update_all(T0, W, R0, S, d, np.zeros(n, np.uint8), alpha, b, np.arange(m), r, q, rule=1, last_selected=100)
    for blk in range(2):
        cand = [(float((c - 100) % n), c) for c in range(blk * 256, min(n, blk * 256 + 256)) if c != q and mod["d"][c] < -1e-9]
        assert (mod["k1"][blk], mod["j"][blk]) == min(cand)
    assert mod["j"][0] >= 100 and mod["k1"][1] >= 156.0                                # block 0 wraps behind column 100


# ---- every comparison function reports one wrong term, word, pair or sign ----------------------------------------------------
def _flush_case(seed, integer):
    rng = np.random.default_rng(seed)
    m, n, p = 33, 18, 7
    gen = kh.int_data if integer else kh.real_data
    return gen(rng, (n, m)), gen(rng, (p, m)), gen(rng, (p, n))


def test_comparators_report_one_dropped_term():
    # integer flush: the last pending row dropped at one entry
    T0, W, R0 = _flush_case(7, True)
    W[-1, 5], R0[-1, 4] = 3.0, -2.0
    want = kh.model_flush_int(T0, W, R0)
    got = want.copy()
    assert not kh.diff_values(got, want)
    got[4, 5] -= W[-1, 5] * R0[-1, 4]
    assert kh.diff_values(got, want)
    # real flush: the same against the a-priori bound, at a sampled entry
    T0, W, R0 = _flush_case(8, False)
    sample = kh.flush_sample(33, 18, 9)
    exact = np.stack([kh.model_tab_column(T0, W, R0, q) for q in range(18)])
    bad, worst = kh.flush_real_check(exact, T0, W, R0, sample)
    assert not bad
    c, i = sample[len(sample) // 2]
    for j in (0, 6):                                                                  # the first and the last pending row
        got = exact.copy()
        got[c, i] -= W[j, i] * R0[j, c]
        bad, _ = kh.flush_real_check(got, T0, W, R0, sample)
        assert [(x[0], x[1]) for x in bad] == [(c, i)]
    got = exact.copy()
    got[c, i] += W[2, i] * R0[2, c]                                                   # a term applied twice
    assert kh.flush_real_check(got, T0, W, R0, sample)[0]
    # chains: one fma step left out of one entry changes the float64 value
    want = kh.model_tab_column(T0, W, R0, 3)
    got = want.copy()
    got[11] = kh.chain_exact(T0[3, 11], W[:-1, 11], R0[:-1, 3])
    assert kh.diff_values(got, want) and kh.diff_bits(got, want)
    # ... and so does a single rounding more (product and sum rounded separately)
    got = want.copy()
    alt = T0[3]
    for j in range(7):
        alt = alt + W[j] * R0[j, 3]
    assert (alt != want).any()
    got[:] = alt
    assert kh.diff_values(got, want)


def test_comparators_report_swapped_columns_and_misplaced_tiles():
    T0, W, R0 = _flush_case(10, True)
    want = kh.model_flush_int(T0, W, R0)
    got = want.copy()
    got[[2, 3]] = got[[3, 2]]
    assert kh.diff_values(got, want)
    # the selector names the source: a swapped pair of columns and a row taken from the wrong pending row both show
    Ws, Rs = kh.selector_operands(33, 18, 7)
    delta = kh.model_flush_int(T0, Ws, Rs) - T0
    want = kh.model_flush_selector(33, 18, 7)
    assert not kh.diff_values(delta, want)
    sw = delta.copy()
    sw[[0, 17]] = sw[[17, 0]]
    assert kh.diff_values(sw, want)
    sw = delta.copy()
    sw[:, [1, 8]] = sw[:, [8, 1]]                                                     # rows 1 and 8 both read pending row 1: equal
    assert not kh.diff_values(sw, want)
    sw[:, [1, 2]] = sw[:, [2, 1]]
    assert kh.diff_values(sw, want)
    # real sample check: two columns swapped
    T0, W, R0 = _flush_case(11, False)
    exact = np.stack([kh.model_tab_column(T0, W, R0, q) for q in range(18)])
    got = exact.copy()
    got[[15, 16]] = got[[16, 15]]
    assert kh.flush_real_check(got, T0, W, R0, kh.flush_sample(33, 18, 9))[0]


def test_comparators_report_one_sentinel_word_and_one_rewritten_const_word():
    region = np.full((4, 6), kh.SENTINEL)
    assert not kh.sentinel_violations(region)
    region[2, 5] = 0.0
    assert len(kh.sentinel_violations(region)) == 1
    region[2, 5] = np.nan                                                             # another NaN is not the sentinel
    assert len(kh.sentinel_violations(region)) == 1
    region[2, 5] = np.array([kh.SENTINEL_BITS ^ np.uint64(1)], dtype=np.uint64).view(np.float64)[0]
    assert len(kh.sentinel_violations(region)) == 1
    ints = np.full(5, kh.SENTINEL_INT, dtype=np.int32)
    assert not kh.sentinel_violations(ints)
    ints[4] = 0
    assert len(kh.sentinel_violations(ints)) == 1
    before = kh.w_image(np.ones((2, 5)), 5, 2, 4)
    after = before.copy()
    assert not kh.diff_unchanged(after, before)
    after[3, 15] = 0.0                                                                # a stale column's padding
    assert len(kh.diff_unchanged(after, before)) == 1
    after = before.copy()
    after[1, 2] = np.nextafter(1.0, 2.0)
    assert len(kh.diff_unchanged(after, before)) == 1


def test_comparators_report_a_lost_sign_of_zero_and_a_nan():
    want = np.array([1.0, -0.0, 0.0, 2.0])
    got = want.copy()
    assert not kh.diff_bits(got, want) and not kh.diff_values(got, want)
    got[1] = 0.0
    assert len(kh.diff_bits(got, want)) == 1
    assert not kh.diff_values(got, want)                                              # values only: the sign of a zero is open
    assert len(kh.diff_unchanged(got, want)) == 1
    got = want.copy()
    got[3] = np.nan
    assert kh.diff_values(got, want) and kh.diff_bits(got, want)
    both = want.copy()
    both[3] = np.nan
    assert kh.diff_values(got, both) and kh.diff_bits(got, both)                      # NaN must not appear in an output at all
    # pivot_b / update_w / update_inverse: the models keep the bits of an entry a zero factor leaves alone
    alpha = np.array([0.0, 2.0, -0.0, 4.0])
    b = np.array([-0.0, 1.0, -0.0, 3.0])
    bn, _ = kh.model_pivot_b(alpha, b, 3)
    assert not kh.diff_bits(bn[[0, 2]], np.array([-0.0, -0.0]))
    Wn, _ = kh.model_update_w(np.array([[-0.0, 1.0, -0.0, 1.0]]), np.array([0.0]), alpha, 3, 1)
    assert not kh.diff_bits(Wn[0], np.array([-0.0, 1.0, -0.0, 1.0]))
    Wn, _ = kh.model_update_w(np.array([[-0.0, 1.0, -0.0, 1.0]]), np.array([2.0]), alpha, 3, 1)
    assert not kh.diff_bits(Wn[0, [0, 2]], np.array([-0.0, -0.0]))                  # u = -0 / 4 is a zero factor
    out, _ = kh.model_explicit_update(np.full((4, 4), -0.0), alpha, 3)
    assert not kh.diff_bits(out[[0, 2]], np.full((2, 4), -0.0))
    assert kh.diff_bits(out[1], np.full(4, -0.0))                                     # fma(-2, -0/4, -0) = +0


# ========================================================================================================================
# T5 - T8: the in-place changes and the batched ratio queries
# ========================================================================================================================
def _rhs_args(m=6, n=5, p=2, count=7, splits=2, seed=3, c_lo=0, integer=False):
    rng = np.random.default_rng(seed)
    data = kh.int_data if integer else kh.real_data
    return dict(T0=data(rng, (n, m)), W=data(rng, (p, m)), R0=data(rng, (p, n)), b=data(rng, m),
                cols=(c_lo + rng.integers(0, n, count)).astype(np.int32), delta=data(rng, count), kmax=4, splits=splits, c_lo=c_lo)


def _cost_args(m=9, n=8, p=2, count=5, ncount=2, splits=2, seed=4, c_lo=0, col_off=0):
    rng = np.random.default_rng(seed)
    flags = np.zeros(c_lo + n - col_off, dtype=np.uint8)
    flags[c_lo + 1 - col_off] = 1
    flags[c_lo + 3 - col_off] = 2
    d = kh.real_data(rng, n)
    d[1] = -0.0
    return dict(T0=kh.real_data(rng, (n, m)), W=kh.real_data(rng, (p, m)), R0=kh.real_data(rng, (p, n)), d=d, in_basis=flags,
                rows=np.sort(rng.permutation(m)[:count]).astype(np.int32), delta=kh.real_data(rng, count),
                ncols=np.array([c_lo + 3, c_lo + 6][:ncount], dtype=np.int32), ndelta=kh.real_data(rng, ncount), kmax=4, splits=splits,
                c_lo=c_lo, col_off=col_off)


def _ratio_args(m=6, n=7, p=2, seed=5):
    rng = np.random.default_rng(seed)
    return dict(T0=kh.real_data(rng, (n, m)), W=kh.real_data(rng, (p, m)), R0=kh.real_data(rng, (p, n)), d=np.abs(kh.real_data(rng, n)),
                in_basis=np.zeros(n, np.uint8), rows=np.array([4, 0, 4], np.int32), tol=kq.TOL_REAL, kmax=4)


def _ranging_args(m=6, n=7, p=2, seed=6):
    rng = np.random.default_rng(seed)
    return dict(T0=kh.real_data(rng, (n, m)), W=kh.real_data(rng, (p, m)), R0=kh.real_data(rng, (p, n)), b=np.abs(kh.real_data(rng, m)),
                basis=np.array([9, 3, kh.WRAPPED_ARTIFICIAL_BASE, 1, 0, 5], np.int32), cols=np.array([6, 0, 6], np.int32), tol=kq.TOL_REAL, kmax=4)


def test_refusals_tab_rhs_change():
    a = _rhs_args()
    _refused(kh.REFUSED_SHAPE, kh.tab_rhs_change, **{**a, "cols": a["cols"][:0], "delta": a["delta"][:0], "splits": 1})   # count < 1
    _refused(kh.REFUSED_SHAPE, kh.tab_rhs_change, **{**a, "kmax": 1})
    _refused(kh.REFUSED_SPLITS, kh.tab_rhs_change, **{**a, "splits": 0})
    _refused(kh.REFUSED_SPLITS, kh.tab_rhs_change, **{**a, "splits": 8})                  # > count
    big = _rhs_args(count=300)
    _refused(kh.REFUSED_SPLITS, kh.tab_rhs_change, **{**big, "splits": 257})              # > kTabRhsMaxSplits
    for bad in (-1, 5):
        cols = a["cols"].copy()
        cols[3] = bad
        _refused(kh.REFUSED_INDEX, kh.tab_rhs_change, **{**a, "cols": cols})
    _refused(kh.REFUSED_INDEX, kh.tab_rhs_change, **{**a, "c_lo": 2})                     # the same list is below the owned range now
    for batch in (0, 2, 7, 64):
        _refused(kh.REFUSED_BATCH, kh.tab_rhs_change, **a, batch=batch)
    _refused(kh.REFUSED_LENGTH, kh.tab_rhs_change, **{**a, "delta": a["delta"][:-1]})
    _refused(kh.REFUSED_LENGTH, kh.tab_rhs_change, **{**a, "b": a["b"][:-1]})
    _refused(kh.REFUSED_LENGTH, kh.tab_rhs_change, **a, lengths=dict(partial=2 * 6))      # ld_partial = ld_b = 16
    _refused(kh.REFUSED_LENGTH, kh.tab_rhs_change, **a, lengths=dict(v=2))


def test_refusals_tab_cost_change():
    a = _cost_args()
    empty = dict(rows=a["rows"][:0], delta=a["delta"][:0])
    _refused(kh.REFUSED_SHAPE, kh.tab_cost_change, **{**a, **empty, "ncols": a["ncols"][:0], "ndelta": a["ndelta"][:0], "splits": 1})
    _refused(kh.REFUSED_SPLITS, kh.tab_cost_change, **{**a, **empty})                     # count = 0 runs as one split
    _refused(kh.REFUSED_SPLITS, kh.tab_cost_change, **{**a, "splits": 0})
    _refused(kh.REFUSED_SPLITS, kh.tab_cost_change, **{**a, "splits": 6})
    _refused(kh.REFUSED_ORDER, kh.tab_cost_change, **{**a, "rows": a["rows"][::-1].copy()})
    rows = a["rows"].copy()
    rows[1] = rows[0]
    _refused(kh.REFUSED_ORDER, kh.tab_cost_change, **{**a, "rows": rows})                 # strictly ascending
    rows = a["rows"].copy()
    rows[-1] = 9
    _refused(kh.REFUSED_INDEX, kh.tab_cost_change, **{**a, "rows": rows})                 # out of range
    _refused(kh.REFUSED_ORDER, kh.tab_cost_change, **{**a, "ncols": np.array([6, 3], np.int32)})
    _refused(kh.REFUSED_INDEX, kh.tab_cost_change, **{**a, "ncols": np.array([3, 8], np.int32)})
    _refused(kh.REFUSED_ORDER, kh.tab_cost_change, **{**a, "ncols": np.array([1, 6], np.int32)})   # a direct term on a column flagged 1
    _refused(kh.REFUSED_INDEX, kh.tab_cost_change, **{**a, "in_basis": np.full(8, 3, np.uint8)})
    _refused(kh.REFUSED_INDEX, kh.tab_cost_change, **{**a, "col_off": 8})
    _refused(kh.REFUSED_BATCH, kh.tab_cost_change, **a, batch=4)
    _refused(kh.REFUSED_LENGTH, kh.tab_cost_change, **{**a, "in_basis": a["in_basis"][:-1]})     # n_store - col_off flags
    _refused(kh.REFUSED_LENGTH, kh.tab_cost_change, **{**a, "col_off": 2})                       # the flags are too many now
    _refused(kh.REFUSED_LENGTH, kh.tab_cost_change, **{**a, "d": a["d"][:-1]})
    _refused(kh.REFUSED_LENGTH, kh.tab_cost_change, **a, lengths=dict(partial=8))


def test_refusals_tab_row_ratios_and_rhs_ranging():
    a = _ratio_args()
    _refused(kh.REFUSED_SHAPE, kh.tab_row_ratios, **{**a, "rows": a["rows"][:0]})
    _refused(kh.REFUSED_SHAPE, kh.tab_row_ratios, **{**a, "tol": (-1e-9, 0.0, 0.0)})
    _refused(kh.REFUSED_SHAPE, kh.tab_row_ratios, **{**a, "tol": (1e-9, np.nan, 0.0)})
    _refused(kh.REFUSED_INDEX, kh.tab_row_ratios, **{**a, "rows": np.array([4, 6], np.int32)})
    _refused(kh.REFUSED_INDEX, kh.tab_row_ratios, **{**a, "rows": np.array([-1], np.int32)})
    _refused(kh.REFUSED_INDEX, kh.tab_row_ratios, **a, col_off=7)
    _refused(kh.REFUSED_BATCH, kh.tab_row_ratios, **a, batch=9)
    _refused(kh.REFUSED_LENGTH, kh.tab_row_ratios, **a, col_off=1)                        # n_store - col_off flags
    _refused(kh.REFUSED_LENGTH, kh.tab_row_ratios, **{**a, "tol": (1e-9, 1e-9)})
    _refused(kh.REFUSED_LENGTH, kh.tab_row_ratios, **a, lengths=dict(part_k=2 * 3))       # the 64-word tail belongs to it
    _refused(kh.REFUSED_LENGTH, kh.tab_row_ratios, **a, lengths=dict(ratio=3))
    b = _ranging_args()
    _refused(kh.REFUSED_SHAPE, kh.tab_rhs_ranging, **{**b, "cols": b["cols"][:0]})
    _refused(kh.REFUSED_SHAPE, kh.tab_rhs_ranging, **{**b, "tol": (1e-9, 0.0, -1.0)})
    _refused(kh.REFUSED_INDEX, kh.tab_rhs_ranging, **{**b, "cols": np.array([7], np.int32)})
    _refused(kh.REFUSED_INDEX, kh.tab_rhs_ranging, **b, c_lo=1)
    _refused(kh.REFUSED_INDEX, kh.tab_rhs_ranging, **{**b, "basis": np.array([9, 3, -2, 1, 0, 5], np.int32)})
    _refused(kh.REFUSED_ORDER, kh.tab_rhs_ranging, **{**b, "basis": np.array([9, 3, 9, 1, 0, 5], np.int32)})   # duplicates
    _refused(kh.REFUSED_BATCH, kh.tab_rhs_ranging, **b, batch=0)
    _refused(kh.REFUSED_LENGTH, kh.tab_rhs_ranging, **{**b, "basis": b["basis"][:-1]})
    _refused(kh.REFUSED_LENGTH, kh.tab_rhs_ranging, **b, lengths=dict(part=2 * 3))
    _refused(kh.REFUSED_LENGTH, kh.tab_rhs_ranging, **b, lengths=dict(row=3))


# ---- tab_rhs_splits / tab_cost_splits ------------------------------------------------------------------------------------------
def test_splits_entry_refusals_and_rule():
    _refused(kh.REFUSED_SHAPE, kh.tab_splits, 2, 10, 10)
    _refused(kh.REFUSED_SHAPE, kh.tab_splits, 0, 0, 10)
    _refused(kh.REFUSED_LENGTH, kh.tab_splits, 0, 10, 10, lengths=dict(out=2))
    for which, unit in ((0, 256), (1, kh.COST_SHARE_MIN)):
        for count in (-5, 0):
            for forced in (0, 1, 7):
                assert kh.tab_splits(which, 1000, count, forced) == 1                      # count < 1 -> 1
        for count in (1, 2, 255, 256, 257, 1000):
            for forced in (1, 2, 255, 256, 257, 100000):
                assert kh.tab_splits(which, 1000, count, forced) == min(forced, count, 256)
        sizes = sorted({256 * k + e for k in (1, 2, 3, 8, 64, 512, 600, 1300) for e in (-1, 0, 1)})
        counts = sorted({u * k + e for u in (24, 256) for k in (1, 2, 3, 5, 40, 256, 257, 300) for e in (-1, 0, 1)} | {1, 2})
        for size in sizes:
            for count in counts:
                got = kh.tab_splits(which, size, count)
                assert got == kh.model_splits(which, size, count), (which, size, count, got)
                assert 1 <= got <= max(1, count)
                grid = (kh.COST_GRID if which else kh.RHS_GRID) // kh.scan_blocks(size)
                assert got == max(1, min(grid, count // unit, 256))
    assert kh.tab_splits(0, 255, 256 * 7 + 255) == 7 and kh.tab_splits(0, 257, 256 * 7) == 7 and kh.tab_splits(0, 257, 100000) == 256
    assert kh.tab_splits(0, 256 * 3 + 1, 100000) == 128 and kh.tab_splits(1, 256 * 3 + 1, 100000) == 256
    assert kh.tab_splits(1, 10000, 408) == 17 and kh.tab_splits(1, 10000, 47) == 1 and kh.tab_splits(1, 10000, 48) == 2


# ---- the models against the definition, scalar by scalar -----------------------------------------------------------------------
def _pending_scalar(delta, x):
    """One pending row by k_tab_*_pending's comment: 256 thread chains with the Fraction fma, then the tree."""
    s = [kh.chain_exact(0.0, delta[t::256], x[t::256]) for t in range(256)]
    half = 128
    while half:
        for t in range(half):
            s[t] = s[t] + s[t + half]
        half //= 2
    return s[0]


def test_pending_sum_is_the_tree_not_the_plain_sum():
    rng = np.random.default_rng(11)
    delta, X = kh.real_data(rng, 300), kh.real_data(rng, (3, 300))
    tree = kh.model_pending(delta, X)
    for j in range(3):
        assert tree[j] == _pending_scalar(delta, X[j])
    plain = kh.model_pending(delta, X, order="plain")
    assert (tree != plain).any(), "the data must tell the two orders apart"
    exact = [sum(Fraction(a) * Fraction(b) for a, b in zip(delta, X[j])) for j in range(3)]
    for j in range(3):
        assert abs(Fraction(tree[j]) - exact[j]) <= kh.gamma(2 + 8) * sum(abs(Fraction(a) * Fraction(b)) for a, b in zip(delta, X[j]))
    assert kh.model_pending(delta[:1], X[:, :1])[0] == delta[0] * X[0, 0]                 # 255 threads add +0.0


def test_rhs_change_model_against_the_definition():
    for splits, count in ((1, 7), (2, 7), (4, 5), (3, 300)):
        a = _rhs_args(count=count, splits=splits)
        exp = kh.rhs_change_expected(**a)
        T0, W, R0, b, cols, delta = (a[k] for k in ("T0", "W", "R0", "b", "cols", "delta"))
        v = [_pending_scalar(delta, R0[j, cols]) for j in range(2)]
        assert not kh.diff_bits(exp["v"][:2], np.array(v)) and not kh.sentinel_violations(exp["v"][2:])
        share = -(-count // splits)
        for i in range(6):
            parts = []
            for s in range(splits):
                lo, hi = min(s * share, count), min(s * share + share, count)
                acc = kh.chain_exact(0.0, delta[lo:hi], [T0[cols[k], i] for k in range(lo, hi)])
                if s == 0:
                    acc = kh.chain_exact(acc, W[:, i], v)
                parts.append(acc)
            total = parts[0]
            for s in range(1, splits):
                total = total + parts[s]
            assert exp["b"][i] == b[i] + total
            if splits > 1:
                assert [exp["partial"][s * 16 + i] for s in range(splits)] == parts
        if (splits, count) == (4, 5):                                                      # shares 2, 2, 1, 0: the empty one is +0.0
            assert not kh.diff_bits(exp["partial"][3 * 16:3 * 16 + 6], np.zeros(6))
        assert not kh.sentinel_violations(exp["b"][6:]) and not kh.sentinel_violations(exp["partial"].reshape(splits, 16)[:, 6:])
        if splits == 1:
            assert not kh.sentinel_violations(exp["partial"])


def test_cost_change_model_against_the_definition():
    for splits, count, c_lo, col_off in ((1, 5, 0, 0), (2, 5, 0, 0), (4, 5, 3, 2), (1, 0, 0, 0)):
        a = _cost_args(count=count, splits=splits, c_lo=c_lo, col_off=col_off)
        exp = kh.cost_change_expected(**a)
        T0, W, R0, d, rows, delta = (a[k] for k in ("T0", "W", "R0", "d", "rows", "delta"))
        p = 2 if count else 0
        u = [_pending_scalar(delta, W[j, rows]) for j in range(p)]
        assert not kh.diff_bits(exp["u"][:p], np.array(u)) and not kh.sentinel_violations(exp["u"][p:])
        share = -(-count // splits)
        for c in range(8):
            got = exp["d"][c_lo + c]
            if c == 1:                                                                     # flagged 1: -0.0 stays -0.0
                assert not kh.diff_bits([got], [-0.0])
                assert not kh.sentinel_violations(exp["partial"].reshape(splits, 8)[:, c])
                continue
            parts = []
            for s in range(splits):
                lo, hi = min(s * share, count), min(s * share + share, count)
                acc = kh.chain_exact(0.0, delta[lo:hi], [T0[c, rows[k]] for k in range(lo, hi)])
                if s == 0:
                    acc = kh.chain_exact(acc, u, R0[:p, c])
                    for k, nc in enumerate(a["ncols"]):
                        if nc == c_lo + c:
                            acc = acc - a["ndelta"][k]
                parts.append(acc)
            total = parts[0]
            for s in range(1, splits):
                total = total + parts[s]
            assert got == d[c] - total
            if splits > 1:
                assert [exp["partial"][s * 8 + c] for s in range(splits)] == parts
        assert not kh.sentinel_violations(exp["d"][:c_lo])
    # columns below col_off move whatever the flags would say without the offset
    a = _cost_args(c_lo=0, col_off=2)
    a["in_basis"][:] = 1
    exp = kh.cost_change_expected(**{**a, "ncols": a["ncols"][:0], "ndelta": a["ndelta"][:0]})
    assert exp["moves"].tolist() == [True, True] + [False] * 6


def _ratio_scalar(entries, weights, ok_index, keys, tol, by_key):
    """One direction of one list entry from the definition: (minimum, pick).  entries: the candidate test values v (already turned so
    that v > tol.pivot qualifies), weights: d or b, keys: what the pick minimises inside the band."""
    pivot, zero, tie = tol
    best, cand = np.inf, []
    for i, (v, w) in enumerate(zip(entries, weights)):
        if ok_index[i] and v > pivot:
            r = (0.0 if w <= zero else w) / v
            cand.append((r, i))
            best = min(best, r)
    if not cand:
        return np.inf, -1
    bound = best + tie * max(1.0, abs(best))
    inside = [i for r, i in cand if r <= bound]
    return best, min(inside, key=(lambda i: keys[i]) if by_key else None)


def test_ratio_models_against_the_definition():
    a = _ratio_args()
    a["in_basis"][2] = 1
    a["in_basis"][5] = 2
    a["d"][3] = 0.0
    for col_off, c_lo in ((0, 0), (2, 0), (1, 3)):
        flags = np.zeros(c_lo + 7 - col_off, np.uint8)
        flags[c_lo + 2 - col_off], flags[c_lo + 5 - col_off] = 1, 2
        exp = kh.model_row_ratios(a["T0"], a["W"], a["R0"], a["d"], flags, a["rows"], a["tol"], c_lo, col_off)
        for k, r in enumerate(a["rows"]):
            e = [kh.chain_exact(a["T0"][c, r], a["W"][:, r], a["R0"][:, c]) for c in range(7)]
            okc = [c_lo + c - col_off >= 0 and flags[c_lo + c - col_off] == 0 for c in range(7)]
            for direction in range(2):
                v = [x if direction else -x for x in e]
                best, pick = _ratio_scalar(v, a["d"], okc, None, a["tol"], False)
                assert exp["ratio"][direction * 3 + k] == best
                assert exp["column"][direction * 3 + k] == (pick + c_lo - col_off if pick >= 0 else -1)
    b = _ranging_args()
    b["b"][1] = -0.5
    exp = kh.model_rhs_ranging(b["T0"], b["W"], b["R0"], b["b"], b["basis"], b["cols"], b["tol"])
    for k, c in enumerate(b["cols"]):
        al = [kh.chain_exact(b["T0"][c, i], b["W"][:, i], b["R0"][:, c]) for i in range(6)]
        for direction in range(2):
            v = [-x if direction else x for x in al]
            best, pick = _ratio_scalar(v, b["b"], [True] * 6, b["basis"], b["tol"], True)
            assert exp["ratio"][direction * 3 + k] == best and exp["row"][direction * 3 + k] == pick


# ---- the case tables are clean -------------------------------------------------------------------------------------------------
def test_no_case_of_the_ratio_tables_depends_on_the_rounding_of_the_bound():
    seen = {"overflow": 0, "none": 0, "band": 0}
    for name, builder in kq.ROW_RATIO_CASES:
        kw = kq.finish_minus_zero(builder(), True)
        exp = kh.model_row_ratios(kw["T0"], kw["W"], kw["R0"], kw["d"], kw["in_basis"], kw["rows"], kw["tol"], kw["c_lo"], kw["col_off"])
        assert (exp["column"] == exp["column_fma"]).all(), name
        assert not exp["between"].any(), name
        seen["none"] += int((exp["column"] == -1).any())
    for name, builder in kq.RHS_RANGING_CASES:
        kw = kq.finish_minus_zero(builder(), False)
        exp = kh.model_rhs_ranging(kw["T0"], kw["W"], kw["R0"], kw["b"], kw["basis"], kw["cols"], kw["tol"], kw["c_lo"])
        assert (exp["row"] == exp["row_fma"]).all(), name
        assert not exp["between"].any(), name
        seen["none"] += int((exp["row"] == -1).any())
    assert seen["none"] >= 4
    # the designed cases are what their names say
    by_name = dict(kq.ROW_RATIO_CASES)
    for blocks in (32, 33):
        kw = by_name[f"list overflow: {blocks} / {65 - blocks} of 34 blocks inside the band, p=9"]()
        E = kh.model_rows_of_T(kw["T0"], kw["W"], kw["R0"], kw["rows"][:1])[0]
        for direction, want in ((0, blocks), (1, 65 - blocks)):
            v = E if direction else -E
            with np.errstate(all="ignore"):
                r = np.where(v > kw["tol"][0], kw["d"] / v, np.inf)
            in_band = (r.reshape(34, 256) <= 1.0 + kq.TIE).any(axis=1)
            assert in_band.sum() == want and in_band[0] and r.argmin() // 256 == 33
        exp = kh.model_row_ratios(kw["T0"], kw["W"], kw["R0"], kw["d"], kw["in_basis"], kw["rows"], kw["tol"])
        assert exp["column"][0] == 7 and exp["column"][2] == 8 and exp["ratio"][0] == 1.0
    by_name = dict(kq.RHS_RANGING_CASES)
    for blocks in (64, 65):
        kw = by_name[f"list overflow: {blocks} / {129 - blocks} of 66 blocks inside the band"]()
        A = kw["T0"][kw["cols"][0]]
        for direction, want in ((0, blocks), (1, 129 - blocks)):
            v = -A if direction else A
            with np.errstate(all="ignore"):
                r = np.where(v > kw["tol"][0], kw["b"] / v, np.inf)
            in_band = (r.reshape(66, 256) <= 1.0 + kq.TIE).any(axis=1)
            assert in_band.sum() == want and in_band[0] and r.argmin() // 256 == 65
        exp = kh.model_rhs_ranging(kw["T0"], kw["W"], kw["R0"], kw["b"], kw["basis"], kw["cols"], kw["tol"])
        assert exp["row"][0] == 7 and exp["row"][2] == 8
        assert kw["T0"].nbytes + kw["b"].nbytes + kw["basis"].nbytes < 1 << 20


def test_sum_case_tables_cover_the_paths():
    for cost in (False, True):
        table = [kw for _, kw in kq.SUM_CASES[cost]]
        assert {(kw["count"], kw["splits"]) for kw in table} >= set(kq.COUNT_SPLITS)
        assert {kw["p"] for kw in table} >= set(kq.P_SWEEP) and {kw["m"] for kw in table} >= set(kq.SIZES)
        assert {kw["c_lo"] for kw in table} == {0, 300}
        assert any(hi == lo for kw in table for lo, hi in kh.share_bounds(kw["count"], kw["splits"]) if kw["count"])       # an empty share
        assert any(hi - lo > 256 for kw in table for lo, hi in kh.share_bounds(kw["count"], kw["splits"]))                 # a second LDS chunk
    cost = [kw for _, kw in kq.SUM_CASES[True]]
    assert {kw["col_off"] for kw in cost} == {0, 5} and {kw["ncount"] for kw in cost if kw["count"] == 0} == {1, 300}
    assert any(kw["ncount"] and kw["count"] for kw in cost)
    a = kq.sum_operands(dict(kq.SUM_CASES[True])[next(n for n, kw in kq.SUM_CASES[True] if kw["col_off"] and kw["c_lo"] == 0)], True, False)
    assert (a["in_basis"][:5] == 1).all() and kh.cost_moves(len(a["d"]), 0, 5, a["in_basis"])[:5].all()
    assert 2 in a["in_basis"]


# ---- every comparison reports what it is there for -----------------------------------------------------------------------------
def test_sum_comparisons_report_order_and_list_errors():
    a = _rhs_args(m=40, count=9, splits=3)
    exp = kh.rhs_change_expected(**a)
    assert not kh.compare_images(exp, exp, kh.RHS_IMAGES)
    short = kh.rhs_change_expected(**{**a, "cols": a["cols"][:-1], "delta": a["delta"][:-1]})        # one dropped list entry
    assert any(f.startswith("b") for f in kh.compare_images({**exp, "b": short["b"]}, exp, kh.RHS_IMAGES))
    swapped = kh.rhs_change_expected(**a, swap_shares=(1, 2))                                          # (p0 + p2) + p1
    assert any(f.startswith("b") for f in kh.compare_images({**exp, "b": swapped["b"]}, exp, kh.RHS_IMAGES))
    five = _rhs_args(count=5, splits=4)
    exp5 = kh.rhs_change_expected(**five)
    left = exp5["partial"].copy()
    left[3 * 16:3 * 16 + 6] = kh.SENTINEL                                                               # the empty share never written
    assert len(kh.compare_images({**exp5, "partial": left}, exp5, kh.RHS_IMAGES)) >= 5
    past = exp["v"].copy()
    past[2] = 0.0                                                                                       # v at p written
    assert len(kh.compare_images({**exp, "v": past}, exp, kh.RHS_IMAGES)) == 1
    c = _cost_args()
    expc = kh.cost_change_expected(**c)
    assert not kh.compare_images(expc, expc, kh.COST_IMAGES)
    d = expc["d"].copy()
    d[1] = 0.0                                                                                          # -0.0 - 0.0: equal value, other bits
    assert len(kh.compare_images({**expc, "d": d}, expc, kh.COST_IMAGES)) == 1
    c2 = dict(c, d=c["d"].copy())
    c2["d"][1] = kh.SENTINEL
    expn = kh.cost_change_expected(**c2)
    assert not kh.compare_images(expn, expn, kh.COST_IMAGES)                                            # the sentinel in d is no finding ...
    d = expn["d"].copy()
    d[1] = np.nan
    assert len(kh.compare_images({**expn, "d": d}, expn, kh.COST_IMAGES)) == 1                          # ... another NaN is
    part = expc["partial"].copy()
    part[8 + 1] = 0.0                                                                                   # a basic column's partial slot
    assert len(kh.compare_images({**expc, "partial": part}, expc, kh.COST_IMAGES)) == 1
    unshifted = kh.cost_change_expected(**{**_cost_args(col_off=2), "col_off": 0, "in_basis": np.concatenate([_cost_args(col_off=2)["in_basis"], [0, 0]])})
    shifted = kh.cost_change_expected(**_cost_args(col_off=2))
    assert kh.diff_image(unshifted["d"], shifted["d"], "d")                                             # flags read without - col_off


def test_ratio_comparisons_report_wrong_picks():
    name = "the minimum in the last block, the lowest in-band column in block 0"
    kw = dict(kq.ROW_RATIO_CASES)[name]()
    m_args = (kw["T0"], kw["W"], kw["R0"], kw["d"], kw["in_basis"], kw["rows"])
    exp = kh.model_row_ratios(*m_args, kw["tol"])
    before = kh.query_images(kw["T0"], kw["W"], kw["R0"], kw["kmax"], d=kw["d"])
    before.update(in_basis=kw["in_basis"], rows=kw["rows"])
    count = len(kw["rows"])
    scratch = 2 * count * 4 + kh.SCRATCH_TAIL
    good = dict(before, ratio=exp["ratio"], column=exp["column"], part_k=np.full(scratch, kh.SENTINEL), part_j=np.full(scratch, kh.SENTINEL_INT, np.int32))
    assert not kh.compare_row_ratios(good, exp, before)
    assert exp["column"][0] == 7 and exp["column"][count] == 8
    higher = exp["column"].copy()
    higher[0] = 3 * 256 + 200                                                                           # the tie went to a higher column
    assert len(kh.compare_row_ratios({**good, "column": higher}, exp, before)) == 1
    k1_only = kh.model_row_ratios(*m_args, (kw["tol"][0], kw["tol"][1], 0.0))                           # a band bound of k1 alone
    assert k1_only["column"][0] == 3 * 256 + 200 and kh.compare_row_ratios({**good, "column": k1_only["column"]}, exp, before)
    tail = good["part_j"].copy()
    tail[-1] = 0
    assert len(kh.compare_row_ratios({**good, "part_j": tail}, exp, before)) == 1
    tail = good["part_k"].copy()
    tail[-kh.SCRATCH_TAIL] = np.inf
    assert len(kh.compare_row_ratios({**good, "part_k": tail}, exp, before)) == 1
    dd = before["d"].copy()
    dd[5] = np.nextafter(dd[5], 9.0)
    assert len(kh.compare_row_ratios({**good, "d": dd}, exp, before)) == 1

    name = "the minimum in the last block, the smallest leaving column in block 0"
    kw = dict(kq.RHS_RANGING_CASES)[name]()
    m_args = (kw["T0"], kw["W"], kw["R0"], kw["b"], kw["basis"], kw["cols"])
    exp = kh.model_rhs_ranging(*m_args, kw["tol"])
    before = kh.query_images(kw["T0"], kw["W"], kw["R0"], kw["kmax"], b=kw["b"])
    before.update(basis=kw["basis"], cols=kw["cols"])
    count = len(kw["cols"])
    good = dict(before, ratio=exp["ratio"], row=exp["row"], part=np.full(2 * count * 4 + kh.SCRATCH_TAIL, kh.SENTINEL))
    assert not kh.compare_rhs_ranging(good, exp, before)
    assert exp["row"][0] == 7
    larger = exp["row"].copy()
    larger[0] = 256 + 37                                                                                # inside the band, a larger leaving column
    assert len(kh.compare_rhs_ranging({**good, "row": larger}, exp, before)) == 1
    k1_only = kh.model_rhs_ranging(*m_args, (kw["tol"][0], kw["tol"][1], 0.0))
    assert k1_only["row"][0] != 7 and kh.compare_rhs_ranging({**good, "row": k1_only["row"]}, exp, before)
    tail = good["part"].copy()
    tail[-1] = 1.0
    assert len(kh.compare_rhs_ranging({**good, "part": tail}, exp, before)) == 1
    # unsigned keys: a leaving column with the top bit set loses to every other one.  (The harness refuses such a basis -- the
    # engine's leaving columns are below 2^31, where both readings agree -- so this is the model's reading only.)
    basis = kw["basis"].astype(np.int64)
    basis[7] = 3_000_000_000
    wrapped = basis.astype(np.uint32).view(np.int32)
    unsigned = kh.model_rhs_ranging(kw["T0"], kw["W"], kw["R0"], kw["b"], wrapped, kw["cols"], kw["tol"])
    signed = kh.model_rhs_ranging(kw["T0"], kw["W"], kw["R0"], kw["b"], wrapped, kw["cols"], kw["tol"], signed_keys=True)
    assert signed["row"][0] == 7 and unsigned["row"][0] != 7
    assert kh.compare_rhs_ranging({**good, "row": signed["row"]}, unsigned, before)
