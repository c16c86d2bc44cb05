"""CPU tier of the kernel tests: the harness refuses bad calls before any HIP call, the reference fma is right, the models of
tests/kernel_harness.py agree with each other, and every comparison function reports a result that is wrong by one term, one
word, one swapped pair of columns or one sign of zero.  No kernel runs here and no product code is altered."""
from fractions import Fraction

import numpy as np
import pytest

import kernel_harness as kh


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
