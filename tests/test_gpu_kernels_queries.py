"""Kernel-level tests of the tableau engine's in-place changes and batched ratio queries, one launcher at a time, on operands the
test constructs (tests/kernel_harness.py, tests/kernels/harness.cpp; the case tables: tests/kernel_query_cases.py):

  T5  launch_tab_rhs_change    b += T0' delta + W' (R0 delta): b, v and every split's partial bit for bit against the documented
                               order (thread chains, the 256-thread tree, shares, split 0 continuing over the pending rows, the
                               partials added in split order), for the batches 1, 8, 16, 32; integer data against the int64 result;
                               real data against the exact rational value within gamma_N S
  T6  launch_tab_cost_change   d -= T0 delta + R0' (W delta) - direct terms, likewise; a column flagged 1 keeps its d to the bit
                               (sentinel NaN, -0.0, 1e300), columns below col_off and barred columns move
  T7  launch_tab_row_ratios    per list entry and direction the minimum ratio and the lowest column inside its tie band, exactly
  T8  launch_tab_rhs_ranging   per list entry and direction the minimum ratio and the row inside its tie band with the smallest
                               leaving column (unsigned), exactly

Every operand a launcher takes as const comes back bit for bit, the sentinel NaN still fills pitch padding, v / u at and beyond p,
the partials' padding, the partials of a single split and the tails behind the scratch of T7 / T8.
"""
import numpy as np
import pytest

import kernel_harness as kh
import kernel_query_cases as kq

pytestmark = pytest.mark.gpu


def ok(*findings):
    flat = [f for group in findings for f in group]
    assert not flat, "\n".join(flat)


def _sample(width, seed, keep=None):
    pts = np.unique(np.random.default_rng(seed).integers(0, width, 200))
    return [int(e) for e in pts if keep is None or keep[e]]


def _ids(cases):
    return [c[0] for c in cases]


# ---- T5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", kq.SUM_CASES[False], ids=_ids(kq.SUM_CASES[False]))
def test_rhs_change(name, kw):
    m, p, count = kw["m"], kw["p"], kw["count"]
    for integer in (True, False):
        args = kq.sum_operands(kw, False, integer)
        for splits in (sorted({1, kw["splits"]}) if integer else [kw["splits"]]):
            a = dict(args, splits=splits)
            exp = kh.rhs_change_expected(**a)
            first = None
            for batch in kh.BATCHES:
                out = kh.tab_rhs_change(**a, batch=batch)
                ok(kh.compare_images(out, exp, kh.RHS_IMAGES))
                assert not np.isnan(out["b"][:m]).any(), "a NaN in b: a read at or past row p or past the list"
                if integer:
                    ok(kh.diff_values(out["b"][:m], kh.rhs_change_int(a["T0"], a["W"], a["R0"], a["b"], a["cols"], a["delta"], a["c_lo"]),
                                      "b (int64)"))
                first = out if first is None else first
                ok(kh.diff_unchanged(out["b"], first["b"], f"b of batch {batch} against batch {kh.BATCHES[0]}"))
        if not integer:
            cl = a["cols"].astype(np.int64) - a["c_lo"]
            bad, worst = kh.exact_check(first["b"], a["b"], a["T0"][cl], a["delta"], a["W"], a["R0"][:, cl],
                                        kh.sum_roundings(count, splits, p), _sample(m, kw["seed"]))
            print(f"rhs_change {name}: largest error {worst:.3f} x 2^-53 S")
            assert not bad, f"beyond gamma_N S: {bad[:5]}"
            # the vectorised model against the Fraction fma itself on one row
            i = m // 2
            lo, hi = kh.share_bounds(count, splits)[0]
            acc = kh.chain_exact(0.0, a["delta"][lo:hi], a["T0"][cl[lo:hi], i])
            acc = kh.chain_exact(acc, a["W"][:, i], exp["v"][:p])
            assert acc == exp["parts"][0][i]


# ---- T6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", kq.SUM_CASES[True], ids=_ids(kq.SUM_CASES[True]))
def test_cost_change(name, kw):
    n, count = kw["n"], kw["count"]
    for integer in (True, False):
        args = kq.sum_operands(kw, True, integer)
        for splits in (sorted({1, kw["splits"]}) if integer else [kw["splits"]]):
            a = dict(args, splits=splits)
            exp = kh.cost_change_expected(**a)
            moves, c_lo = exp["moves"], a["c_lo"]
            first = None
            for batch in kh.BATCHES:
                out = kh.tab_cost_change(**a, batch=batch)
                ok(kh.compare_images(out, exp, kh.COST_IMAGES))
                got = out["d"][c_lo:]
                assert not np.isnan(got[moves]).any(), "a NaN in d: a read at or past row p or past the list"
                ok(kh.diff_unchanged(got[~moves], a["d"][~moves], "d of a column flagged 1"))
                if integer:
                    want = kh.cost_change_int(a["T0"], a["W"], a["R0"], a["d"], a["rows"], a["delta"], a["ncols"], a["ndelta"], moves, c_lo)
                    ok(kh.diff_values(got[moves], want[moves], "d (int64)"))
                first = out if first is None else first
                ok(kh.diff_unchanged(out["d"], first["d"], f"d of batch {batch} against batch {kh.BATCHES[0]}"))
        if not integer:
            rows = a["rows"].astype(np.int64)
            p = a["W"].shape[0] if count else 0
            direct = np.zeros(n)
            direct[a["ncols"].astype(np.int64) - c_lo] = a["ndelta"]
            bad, worst = kh.exact_check(first["d"][c_lo:], a["d"], a["T0"][:, rows].T, a["delta"], a["R0"][:p], a["W"][:p][:, rows],
                                        kh.sum_roundings(count, splits, p) + 1, _sample(n, kw["seed"], moves), sign=-1, extra=direct)
            print(f"cost_change {name}: largest error {worst:.3f} x 2^-53 S")
            assert not bad, f"beyond gamma_N S: {bad[:5]}"


# ---- T7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", kq.ROW_RATIO_CASES, ids=_ids(kq.ROW_RATIO_CASES))
def test_row_ratios(name, builder):
    kw = kq.finish_minus_zero(builder(), True)
    exp = kh.model_row_ratios(kw["T0"], kw["W"], kw["R0"], kw["d"], kw["in_basis"], kw["rows"], kw["tol"], kw["c_lo"], kw["col_off"])
    assert (exp["column"] == exp["column_fma"]).all() and not exp["between"].any(), "the case depends on the rounding of the bound"
    before = kh.query_images(kw["T0"], kw["W"], kw["R0"], kw["kmax"], kw["c_lo"], d=kw["d"])
    before.update(in_basis=kw["in_basis"], rows=kw["rows"])
    for batch in kh.BATCHES:
        ok(kh.compare_row_ratios(kh.tab_row_ratios(**kw, batch=batch), exp, before))
    k, c = len(kw["rows"]) - 1, kw["T0"].shape[0] // 2                    # the vectorised model against the Fraction fma itself
    assert exp["E"][k, c] == kh.chain_exact(kw["T0"][c, kw["rows"][k]], kw["W"][:, kw["rows"][k]], kw["R0"][:, c])


# ---- T8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,builder", kq.RHS_RANGING_CASES, ids=_ids(kq.RHS_RANGING_CASES))
def test_rhs_ranging(name, builder):
    kw = kq.finish_minus_zero(builder(), False)
    exp = kh.model_rhs_ranging(kw["T0"], kw["W"], kw["R0"], kw["b"], kw["basis"], kw["cols"], kw["tol"], kw["c_lo"])
    assert (exp["row"] == exp["row_fma"]).all() and not exp["between"].any(), "the case depends on the rounding of the bound"
    before = kh.query_images(kw["T0"], kw["W"], kw["R0"], kw["kmax"], kw["c_lo"], b=kw["b"])
    before.update(basis=kw["basis"], cols=kw["cols"])
    for batch in kh.BATCHES:
        ok(kh.compare_rhs_ranging(kh.tab_rhs_ranging(**kw, batch=batch), exp, before))
    k, i = len(kw["cols"]) - 1, kw["T0"].shape[1] // 2
    cl = int(kw["cols"][k]) - kw["c_lo"]
    assert exp["A"][k, i] == kh.chain_exact(kw["T0"][cl, i], kw["W"][:, i], kw["R0"][:, cl])
