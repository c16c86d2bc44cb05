"""Kernel-level tests of the tableau engine's blocked update, one launcher at a time, on operands the test constructs
(tests/kernel_harness.py, tests/kernels/harness.cpp):

  T1  launch_tab_flush       T0 += W R0 on all three paths, exactly: integer data against the int64 product, real data against
                             the exact rational value with the a-priori bound (2p + 1) 2^-53 (|T0| + sum |W||R0|) -- no summation
                             order is asserted for the MFMA; FlushList::count, cols, R0c and the statistics
  T2  launch_tab_column      alpha = T0[:,q] + W R0[:,q], bit for bit against the ascending fma chain, batches 1, 8, 16, 32
  T3  launch_tab_row         row r of T over the owned columns, likewise
  T4  launch_tab_update_all  the unfused per-pivot update, every output against the documented arithmetic

After every call the regions a kernel must not write still hold the sentinel NaN (pitch padding, stale rows of R0 and columns of
W, skipped columns, const buffers); a NaN in an output would show a read past row p or row m.
"""
import numpy as np
import pytest

import kernel_harness as kh

pytestmark = pytest.mark.gpu

OBSERVED = {}          # path -> [largest error / (2^-53 S), MFMA result == ascending fma chain on every sampled entry]


def ok(*findings):
    flat = [f for group in findings for f in group]
    assert not flat, "\n".join(flat)


def flush_path(m, n, listed):
    if n * m < kh.FLUSH_LDS_THRESHOLD:
        return "small"
    return "lds_listed" if listed else "lds_all"


def expected_list(R0, c_lo):
    """Owned columns with a nonzero (or NaN) R0 entry in a pending row, as storage columns, ascending."""
    if R0.shape[0] == 0:
        return np.zeros(0, dtype=np.int32)
    return (c_lo + np.nonzero(~(R0 == 0.0).all(axis=0))[0]).astype(np.int32)


def run_flush(T0, W, R0, kmax, c_lo, listed, want, stats=(3, 1000), real_sample=None):
    """One flush; checks the result (`want`: the exact integer result, or None with `real_sample` for real data), the list,
    the statistics and every region that must keep its bits.  Returns the logical result."""
    n, m = T0.shape
    p = W.shape[0]
    path = flush_path(m, n, listed)
    out = kh.tab_flush(T0, W, R0, kmax, c_lo=c_lo, listed=listed, stats=stats)
    t_up, w_up, r_up = kh.tab_images(out, m, n, p, kmax, T0, W, R0)
    t = kh.image(out["T0"], n, kh.ld_t(m))
    got = t[:, :m]
    ok(kh.diff_unchanged(kh.image(out["W"], kmax, kh.ld_b(m)), w_up, "W"),
       kh.diff_unchanged(kh.image(out["R0"], kmax + 1, kh.ld_r(n)), r_up, "R0"),
       kh.sentinel_violations(t[:, m:], "T0 padding"))
    cols = expected_list(R0, c_lo) if path == "lds_listed" else c_lo + np.arange(n, dtype=np.int32)
    if p == 0:
        ok(kh.diff_unchanged(t, t_up, "T0 (p = 0)"))
        assert tuple(out["stats"]) == stats, "p = 0 leaves the statistics alone"
        ok(kh.sentinel_violations(out["cols"], "cols"), kh.sentinel_violations(out["count"], "count"),
           kh.sentinel_violations(out["R0c"], "R0c"))
        return got
    assert tuple(out["stats"]) == (stats[0] + 1, stats[1] + len(cols)), (out["stats"], len(cols))
    if path == "lds_listed":
        assert out["count"][0] == len(cols)
        ok(kh.diff_values(out["cols"][:len(cols)], cols, "cols"), kh.sentinel_violations(out["cols"][len(cols):], "cols past count"))
        r0c = kh.image(out["R0c"], kmax, kh.ld_r(n))
        ok(kh.diff_unchanged(r0c[:p, :len(cols)], R0[:, cols - c_lo], "R0c"),
           kh.sentinel_violations(r0c[:p, len(cols):], "R0c past count"), kh.sentinel_violations(r0c[p:], "R0c past p"))
        skipped = np.setdiff1d(np.arange(n), cols - c_lo)
        ok(kh.diff_unchanged(got[skipped], T0[skipped], "skipped T0 column"))       # bits: a skipped -0.0 stays -0.0
    else:
        ok(kh.sentinel_violations(out["cols"], "cols"), kh.sentinel_violations(out["count"], "count"),
           kh.sentinel_violations(out["R0c"], "R0c"))
    if want is not None:
        ok(kh.diff_values(got, want, "T"))
    if real_sample is not None:
        bad, worst = kh.flush_real_check(got, T0, W, R0, real_sample)
        assert not bad, f"beyond (2p + 1) 2^-53 S: {bad[:5]}"
        assert not np.isnan(got).any()
        chain_equal = all(got[c, i] == kh.chain_exact(T0[c, i], W[:, i], R0[:, c]) for c, i in real_sample[:60])
        obs = OBSERVED.setdefault(path, [0.0, True])
        obs[0] = max(obs[0], worst)
        obs[1] = obs[1] and chain_equal
        print(f"flush {path} m={m} n={n} p={p}: largest error {worst:.3f} x 2^-53 S, equals the fma chain: {chain_equal}")
    return got


def flush_case(m, n, p, kmax, c_lo, listed, seed, selector=False):
    rng = np.random.default_rng(seed)
    # integer data: == the int64 product
    T0, W, R0 = kh.int_data(rng, (n, m)), kh.int_data(rng, (p, m)), kh.int_data(rng, (p, n))
    run_flush(T0, W, R0, kmax, c_lo, listed, kh.model_flush_int(T0, W, R0))
    # real data: within the a-priori bound of the exact value at every tile corner and 200 seeded entries
    T0, W, R0 = kh.real_data(rng, (n, m)), kh.real_data(rng, (p, m)), kh.real_data(rng, (p, n))
    run_flush(T0, W, R0, kmax, c_lo, listed, None, real_sample=kh.flush_sample(m, n, seed))
    if selector and p > 0:
        T0 = kh.int_data(rng, (n, m))
        Ws, Rs = kh.selector_operands(m, n, p)
        got = run_flush(T0, Ws, Rs, kmax, c_lo, listed, None)
        ok(kh.diff_values(got - T0, kh.model_flush_selector(m, n, p), "selector (1 + column + 1000 pending row)"))


# ---- T1: shapes ------------------------------------------------------------------------------------------------------------
SMALL_M = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129]
SMALL_N = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257]
SMALL_BASES = [(65, 129), (33, 17)]                    # (m, n_owned)
LDS_SHAPES = [(256, 256), (255, 258), (257, 256), (129, 513), (127, 517), (33, 2049), (513, 129), (2049, 33)]
LDS_BASES = [(256, 256), (129, 513)]
P_ALL = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 127, 128]


def _ids(cases, fmt):
    return [fmt.format(*c) for c in cases]


SMALL_SHAPE_CASES = ([(m, 129) for m in SMALL_M] + [(65, n) for n in SMALL_N] + [(m, 17) for m in (1, 16, 17, 129)] +
                     [(33, n) for n in (1, 128, 129, 257)] + [(257, 255)])


@pytest.mark.parametrize("m,n", SMALL_SHAPE_CASES, ids=_ids(SMALL_SHAPE_CASES, "(m, n_owned) = ({}, {})"))
def test_flush_small_path_shapes(m, n):
    assert m * n < kh.FLUSH_LDS_THRESHOLD
    # (the engine hands this path a FlushList with `cols` set as well; k_tab_flush rewrites every owned column and leaves it alone)
    flush_case(m, n, 17, 128, 0, bool((m + n) % 2), 1000 + 7 * m + n, selector=(m, n) in SMALL_BASES or (m, n) == (257, 255))


LDS_SHAPE_CASES = [(m, n, listed) for (m, n) in LDS_SHAPES for listed in (False, True)]


@pytest.mark.parametrize("m,n,listed", LDS_SHAPE_CASES, ids=_ids(LDS_SHAPE_CASES, "(m, n_owned) = ({}, {}) listed={}"))
def test_flush_lds_paths_shapes(m, n, listed):
    assert m * n >= kh.FLUSH_LDS_THRESHOLD
    flush_case(m, n, 17, 128, 0, listed, 2000 + 3 * m + n, selector=True)


# p, kmax in {p, 128}, c_lo in {0, 70}, one factor at a time around each path's base shapes
P_CASES = ([(p, 128, 0) for p in P_ALL] + [(p, p, 0) for p in P_ALL if p != 128] + [(p, 128, 70) for p in (0, 5, 16, 33, 128)] +
           [(p, p, 70) for p in (5, 33)])
PATHS = [("small", SMALL_BASES, False), ("lds_all", LDS_BASES, False), ("lds_listed", LDS_BASES, True)]
P_PATH_CASES = [(path, base, p, kmax, c_lo) for path, bases, _ in PATHS for k, base in enumerate(bases)
                for (p, kmax, c_lo) in (P_CASES if k == 0 else [(0, 128, 0), (4, 4, 70), (17, 128, 70), (127, 128, 0), (128, 128, 70)])]


@pytest.mark.parametrize("path,base,p,kmax,c_lo", P_PATH_CASES,
                         ids=[f"{path} (m, n_owned) = {base} p = {p} kmax = {kmax} c_lo = {c_lo}" for path, base, p, kmax, c_lo in P_PATH_CASES])
def test_flush_pending_rows(path, base, p, kmax, c_lo):
    m, n = base
    listed = path == "lds_listed"
    assert flush_path(m, n, listed) == path
    flush_case(m, n, p, kmax, c_lo, listed, 3000 + 11 * p + kmax + c_lo + m, selector=p in (5, 16, 33, 128) and kmax == 128)


def _random_triples(path):
    rng = np.random.default_rng({"small": 41, "lds_all": 42, "lds_listed": 43}[path])
    out = []
    while len(out) < 20:
        if path == "small":
            m, n = int(rng.integers(1, 300)), int(rng.integers(1, 300))
            if m * n >= kh.FLUSH_LDS_THRESHOLD:
                continue
        else:
            m = int(rng.integers(32, 700))
            n = int(rng.integers(-(-kh.FLUSH_LDS_THRESHOLD // m), -(-kh.FLUSH_LDS_THRESHOLD // m) + 300))
        out.append((path, m, n, int(rng.integers(1, 41))))
    return out


RANDOM_CASES = [c for path in ("small", "lds_all", "lds_listed") for c in _random_triples(path)]


@pytest.mark.parametrize("path,m,n,p", RANDOM_CASES, ids=[f"{path} random (m, n_owned, p) = ({m}, {n}, {p})" for path, m, n, p in RANDOM_CASES])
def test_flush_random_triples(path, m, n, p):
    listed = path == "lds_listed"
    assert flush_path(m, n, listed) == path
    flush_case(m, n, p, int(p if (m + n) % 2 else 128), 70 * (n % 2), listed, 4000 + m * 1000 + n + p)


# ---- T1: the listed path's columns -------------------------------------------------------------------------------------------
def _listed_patterns(n):
    pats = [("none: count = 0", []), ("every other one", list(range(0, n, 2))), ("exactly 128", list(range(3, 3 + 128))),
            ("all", list(range(n)))]
    pats += [(f"exactly one, at owned position {x}", [x]) for x in (0, 63, 64, 127, 128, n - 1)]
    return pats


LISTED_CASES = [(base, name, cols, c_lo) for base in LDS_BASES for (name, cols) in _listed_patterns(base[1]) for c_lo in (0, 70)
                if c_lo == 0 or name.startswith(("none", "every", "exactly one, at owned position 64"))]


@pytest.mark.parametrize("base,name,cols,c_lo", LISTED_CASES,
                         ids=[f"(m, n_owned) = {base} c_lo = {c_lo} {name}" for base, name, cols, c_lo in LISTED_CASES])
def test_flush_listed_columns(base, name, cols, c_lo):
    m, n = base
    p, kmax = 9, 128
    rng = np.random.default_rng(5000 + len(cols) + c_lo + m)
    T0, W = kh.int_data(rng, (n, m)), kh.int_data(rng, (p, m), zeros=0.1)
    T0[rng.random((n, m)) < 0.1] = -0.0                            # skipped columns that hold -0.0 keep it
    R0 = np.zeros((p, n))
    for c in cols:
        R0[rng.integers(0, p), c] = float(rng.integers(1, 9))      # one nonzero is enough to list a column
    for c in cols[::3]:                                            # every third listed column is dense
        R0[:, c] = rng.integers(1, 9, p).astype(float) * rng.choice([-1.0, 1.0], p)
    assert list(expected_list(R0, c_lo)) == [c_lo + c for c in cols]
    want = kh.model_flush_int(T0, W, R0)
    got = run_flush(T0, W, R0, kmax, c_lo, True, want)
    if not cols:
        ok(kh.diff_unchanged(got, T0, "T0 with an empty list"))
    # flush-all on the same operands: the same values (the sign of a zero in a column the list skips is open there)
    run_flush(T0, W, R0, kmax, c_lo, False, want)


@pytest.mark.parametrize("base", LDS_BASES, ids=[f"(m, n_owned) = {b}" for b in LDS_BASES])
def test_flush_listed_nan_counts_as_nonzero(base):
    """One column whose only nonzero R0 entry is a NaN: it is listed and becomes NaN; every other column keeps its bits."""
    m, n = base
    p, kmax, c = 9, 128, 77
    rng = np.random.default_rng(6000 + m)
    T0, W = kh.int_data(rng, (n, m)), kh.int_data(rng, (p, m), zeros=0.1)
    T0[rng.random((n, m)) < 0.1] = -0.0
    R0 = np.zeros((p, n))
    R0[4, c] = np.nan
    out = kh.tab_flush(T0, W, R0, kmax, c_lo=70, listed=True, stats=(0, 0))
    got = kh.image(out["T0"], n, kh.ld_t(m))
    assert out["count"][0] == 1 and out["cols"][0] == 70 + c and tuple(out["stats"]) == (1, 1)
    assert np.isnan(got[c, :m]).all()
    others = np.arange(n) != c
    ok(kh.diff_unchanged(got[others, :m], T0[others], "unlisted column"), kh.sentinel_violations(got[:, m:], "T0 padding"),
       kh.sentinel_violations(out["cols"][1:], "cols past count"))


def test_flush_observations():
    """Not an assertion: what the MFMA flush was seen to do on the real data of this run (profiles/r16_kernel_harness.md)."""
    for path, (worst, chain_equal) in sorted(OBSERVED.items()):
        print(f"OBSERVED flush path {path}: largest error {worst:.3f} x 2^-53 S; equals the ascending fma chain bit for bit: {chain_equal}")


# ---- T2, T3 ------------------------------------------------------------------------------------------------------------------
SIZES = [1, 255, 256, 257, 513]
P_VEC = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128]
VEC_BASES = [(257, 256), (255, 513)]


def _vec_cases(index_of):
    """(m, n, p, index, c_lo): one factor at a time around the two base shapes; index_of(m, n) = the size the index runs over."""
    cases = []
    for (bm, bn) in VEC_BASES:
        shapes = [(m, bn) for m in SIZES] + [(bm, n) for n in SIZES]
        for (m, n) in shapes:
            cases.append((m, n, 17, index_of(m, n) - 1, 0))
        for p in P_VEC:
            cases.append((bm, bn, p, index_of(bm, bn) // 2, 0 if (bm, bn) == VEC_BASES[0] else 70))
        for idx in (0, index_of(bm, bn) - 1, 255, 256):
            if idx < index_of(bm, bn):
                cases.append((bm, bn, 33, idx, 70 if idx in (0, 255) else 0))
    cases.append((1, 1, 1, 0, 70))
    return sorted(set(cases))


def _vec_operands(m, n, p, seed):
    rng = np.random.default_rng(seed)
    return kh.real_data(rng, (n, m), 0.05, 0.05), kh.real_data(rng, (p, m), 0.1, 0.05), kh.real_data(rng, (p, n), 0.1, 0.05)


def _vec_check(m, n, p, c_lo, want, sample_chain, **which):
    kmax = 128 if (m + n + p) % 2 else max(p, 1)
    results = []
    T0, W, R0 = which.pop("ops")
    for batch in kh.BATCHES:
        out = kh.tab_vector(T0, W, R0, kmax, c_lo=c_lo, batch=batch, **which)
        t_up, w_up, r_up = kh.tab_images(out, m, n, p, kmax, T0, W, R0)
        size = len(want)
        ok(kh.diff_values(out["vec"][:size], want, f"batch {batch}"), kh.sentinel_violations(out["vec"][size:], "past the end"),
           kh.diff_unchanged(kh.image(out["T0"], n, kh.ld_t(m)), t_up, "T0"),
           kh.diff_unchanged(kh.image(out["W"], kmax, kh.ld_b(m)), w_up, "W"),
           kh.diff_unchanged(kh.image(out["R0"], kmax + 1, kh.ld_r(n)), r_up, "R0"))
        results.append(out["vec"][:size].copy())
    for batch, res in zip(kh.BATCHES[1:], results[1:]):
        ok(kh.diff_bits(res, results[0], f"batch {batch} against batch 1"))
    for k in sorted({0, len(want) - 1, len(want) // 2, min(255, len(want) - 1), min(256, len(want) - 1)}):
        assert want[k] == sample_chain(k), "the vectorised model against the Fraction chain"


COLUMN_CASES = _vec_cases(lambda m, n: n)


@pytest.mark.parametrize("m,n,p,q,c_lo", COLUMN_CASES, ids=_ids(COLUMN_CASES, "m = {} n_owned = {} p = {} q = {} c_lo = {}"))
def test_tab_column(m, n, p, q, c_lo):
    T0, W, R0 = _vec_operands(m, n, p, 7000 + m + 3 * n + 5 * p + q)
    want = kh.model_tab_column(T0, W, R0, q)
    _vec_check(m, n, p, c_lo, want, lambda i: kh.chain_exact(T0[q, i], W[:, i], R0[:, q]), ops=(T0, W, R0), q=q)


ROW_CASES = _vec_cases(lambda m, n: m)


@pytest.mark.parametrize("m,n,p,r,c_lo", ROW_CASES, ids=_ids(ROW_CASES, "m = {} n_owned = {} p = {} r = {} c_lo = {}"))
def test_tab_row(m, n, p, r, c_lo):
    T0, W, R0 = _vec_operands(m, n, p, 8000 + m + 3 * n + 5 * p + r)
    want = kh.model_tab_row(T0, W, R0, r)
    _vec_check(m, n, p, c_lo, want, lambda c: kh.chain_exact(T0[c, r], W[:, r], R0[:, c]), ops=(T0, W, R0), row=r)


# ---- T4 ------------------------------------------------------------------------------------------------------------------------
def update_all_case(m, n, p_old, new, jt=None, c_lo=0, rule=0, last_selected=-1, alpha_r_negative=False, b_r_zero=False,
                    wrapped_leaving=False, trace_full=False, seed=0):
    rng = np.random.default_rng(9000 + seed + m * 7 + n * 3 + p_old)
    kmax = 128
    T0 = kh.real_data(rng, (n, m), 0.05, 0.05)
    W = kh.real_data(rng, (p_old, m), 0.15, 0.1)                 # -0.0 where a zero factor must leave it
    R0 = kh.real_data(rng, (p_old, n), 0.1, 0.05)
    S = kh.distinct_rows(rng, m, p_old)
    if new:
        free = np.setdiff1d(np.arange(m), S)
        r = int(free[len(free) // 2])
    else:
        r = int(S[jt])
    if p_old:
        W[rng.random(p_old) < 0.25, r] = 0.0                      # wr with exact zeros
    q = n - 1 if n < 3 else int(rng.integers(0, n))
    alpha = kh.real_data(rng, m, 0.2, 0.1)                        # exact zeros of both signs
    alpha[r] = -1.75 if alpha_r_negative else 1.375
    b = kh.real_data(rng, m, 0.1, 0.1)
    b[r] = 0.0 if b_r_zero else (-0.625 if alpha_r_negative else 0.625)
    d = kh.real_data(rng, n, 0.05)
    d[q] = -1.25
    in_basis = (rng.random(n) < 0.3).astype(np.uint8)
    in_basis[q] = 0
    leaving = kh.WRAPPED_ARTIFICIAL_BASE + 5 if wrapped_leaving else c_lo + int(np.nonzero(np.arange(n) != q)[0][0] if n > 1 else 0)
    if not wrapped_leaving and n > 1:
        in_basis[leaving - c_lo] = 1
    basis = rng.integers(0, c_lo + n, m).astype(np.int32)
    basis[r] = leaving
    trace_cap = 6
    kw = dict(c_lo=c_lo, rule=rule, last_selected=last_selected, leaving=leaving, phase=1 + seed % 2, degenerate=4,
              iterations=6 if trace_full else 2, trace_cap=trace_cap, tol_cost=1e-9, minus_objective=3.25)
    mod = kh.model_tab_update_all(T0, W, R0, S, d, in_basis, alpha, b, basis, r, q, **kw)
    assert (mod["jt"] == p_old) == new
    p_new = mod["n_eta"]
    results = []
    for batch in kh.BATCHES:
        out = kh.tab_update_all(T0, W, R0, S, d, in_basis, alpha, b, basis, kmax, r, q, batch=batch, **kw)
        t_up, w_up, r_up = kh.tab_images(out, m, n, p_old, kmax, T0, W, R0)
        r0 = kh.image(out["R0"], kmax + 1, kh.ld_r(n))
        w = kh.image(out["W"], kmax, kh.ld_b(m))
        tag = f"batch {batch} "
        ok(kh.diff_unchanged(kh.image(out["T0"], n, kh.ld_t(m)), t_up, tag + "T0"),
           # R0: the pending rows keep their bits, the appended row is T0's row r (a copy: bits), the rest is untouched
           kh.diff_unchanged(r0[:p_old], r_up[:p_old], tag + "R0 pending rows"),
           kh.diff_bits(r0[p_old:p_new, :n], mod["R0"][p_old:p_new], tag + "appended R0 row"),
           kh.sentinel_violations(r0[p_old:p_new, n:], tag + "R0 padding of the appended row"),
           kh.sentinel_violations(r0[p_new:], tag + "R0 past p"),
           # W <- E W: bits (an entry a zero factor leaves alone keeps them), columns past the new p and the padding untouched
           kh.diff_bits(w[:p_new, :m], mod["W"], tag + "W"),
           kh.sentinel_violations(w[:p_new, m:], tag + "W padding"), kh.sentinel_violations(w[p_new:], tag + "W past p"),
           kh.diff_unchanged(out["wr"], kh.vec_image(mod["wr"], p_old, kmax), tag + "wr"),
           kh.diff_values(out["S"][:p_new], mod["S"], tag + "S"), kh.sentinel_violations(out["S"][p_new:], tag + "S past p"),
           kh.diff_values(out["pos"], mod["pos"], tag + "pos_of_row"),
           kh.diff_values(out["d"][c_lo:], mod["d"], tag + "d"), kh.sentinel_violations(out["d"][:c_lo], tag + "d below c_lo"),
           kh.diff_values(out["k1"], mod["k1"], tag + "PRICE partial keys"), kh.diff_values(out["j"], mod["j"], tag + "PRICE partial columns"),
           kh.diff_unchanged(out["alpha"], kh.vec_image(alpha, m, kh.ld_b(m)), tag + "alpha"),
           kh.diff_bits(out["b"][:m], mod["b"], tag + "b"), kh.sentinel_violations(out["b"][m:], tag + "b padding"),
           kh.diff_values(out["basis"], mod["basis"], tag + "basis"), kh.diff_values(out["in_basis"], mod["in_basis"], tag + "in_basis"),
           kh.diff_values(out["trace"], mod["trace"], tag + "trace"))
        assert out["d"][c_lo + q] == 0.0, "the column q itself gets d = 0"
        assert list(out["irec"]) == [p_new, mod["jt"], p_old, mod["degenerate"], 0, c_lo + q, r, leaving]
        assert out["lrec"][0] == mod["iterations"] and out["drec"][0] == mod["minus_objective"]
        results.append(out)
    for batch, out in zip(kh.BATCHES[1:], results[1:]):
        for key in ("W", "R0", "d", "b", "k1"):
            ok(kh.diff_unchanged(out[key], results[0][key], f"{key}: batch {batch} against batch 1"))
    # the vectorised model against the Fraction chain at a few entries
    wr = mod["wr"]
    for c in sorted({0, n - 1, n // 2, q}):
        base = R0[mod["jt"], c] if not new else T0[c, r]
        row = kh.chain_exact(base, wr, R0[:, c])
        want = 0.0 if c == q else kh.fma_exact(-(d[q] / alpha[r]), row, d[c])
        assert mod["d"][c] == want
    return mod


T4_CASES = {}
for _m in (1, 255, 256, 257):
    _p = 8 if _m > 8 else 0                              # (m = 1 has one row: the block is empty before its only pivot)
    T4_CASES[f"m = {_m} n_owned = 257 r new p = {_p} → {_p + 1}"] = dict(m=_m, n=257, p_old=_p, new=True)
for _n in (1, 256, 257):
    T4_CASES[f"m = 257 n_owned = {_n} r new p = 9 → 10"] = dict(m=257, n=_n, p_old=9, new=True)
for _p in (0, 1, 7, 8, 9, 127):
    T4_CASES[f"r new in the block p = {_p} → {_p + 1}"] = dict(m=256, n=257, p_old=_p, new=True, seed=_p)
for _p in (1, 9, 127):
    T4_CASES[f"r already in the block p = {_p} jt = 0"] = dict(m=257, n=256, p_old=_p, new=False, jt=0)
    T4_CASES[f"r already in the block p = {_p} jt = p_old - 1"] = dict(m=257, n=256, p_old=_p, new=False, jt=_p - 1, c_lo=70)
T4_CASES["alpha_r negative (the dual loop's case)"] = dict(m=255, n=256, p_old=9, new=True, alpha_r_negative=True, c_lo=70)
T4_CASES["b_r = 0: degenerate counts"] = dict(m=255, n=256, p_old=7, new=False, jt=3, b_r_zero=True)
T4_CASES["leaving column at kWrappedArtificialBase + 5: no flag cleared"] = dict(m=256, n=256, p_old=8, new=True, wrapped_leaving=True)
T4_CASES["trace full (iterations >= trace_cap)"] = dict(m=256, n=257, p_old=8, new=True, trace_full=True, c_lo=70)
for _rule in (0, 1, 2):
    T4_CASES[f"rule {_rule} with last_selected set"] = dict(m=257, n=257, p_old=9, new=True, rule=_rule, last_selected=150, c_lo=70 * (_rule % 2))
T4_CASES["rule 1 without memory (last_selected = -1)"] = dict(m=64, n=300, p_old=3, new=False, jt=1, rule=1)


@pytest.mark.parametrize("name", list(T4_CASES))
def test_tab_update_all(name):
    update_all_case(**T4_CASES[name])
