"""Kernel-level tests of the revised engine's deferred and explicit update, unsharded (row_lo = 0, row_hi = m), one launcher
family at a time on operands the test constructs (tests/kernel_harness.py, tests/kernels/harness.cpp):

  R1  launch_apply_w                                  alpha = v + W (S'v)
  R2  launch_eta_prepare + launch_update_w            wr, the slot choice, W <- W + u W[r,:] and the target column
  R3  launch_rho_deferred                             rho over {r} U S: the 8-unrolled part, the tail, zero coefficients
  R4  launch_flush_snapshot / _apply / _reset         B0inv += W (S' B0inv), pos_of_row back to -1, n_eta = 0
  R5  launch_compute_rho + launch_update_inverse      the explicit rank-1 update

Every result is compared with the documented chain of fmas (ascending j, one IEEE division) as float64 values, bit patterns where
the kernels promise bits, and every region a kernel must not write still holds what was uploaded (the NaN sentinel in pitch
padding and stale columns).  The padding COLUMNS of B^-1 are different: the kernels of this engine rewrite them (rho is written
"ld_b entries, padding zero", the rank-1 update and the flush walk whole rows), so they are uploaded as zeros, as
launch_set_identity leaves them, and must come back as zeros.
"""
import numpy as np
import pytest

import kernel_harness as kh

pytestmark = pytest.mark.gpu

M_ALL = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513]
P_ALL = [1, 7, 8, 9, 15, 16, 17, 127, 128]


def ok(*findings):
    flat = [f for group in findings for f in group]
    assert not flat, "\n".join(flat)


def cases(p_base_m=257):
    """(m, p, r in S): one factor at a time around the base shapes (65, 9) and (p_base_m, 17)."""
    out = []
    for m in M_ALL:
        out += [(m, min(9, m), True), (m, min(9, max(m - 1, 0)), False)]
    for p in P_ALL:
        out += [(p_base_m, p, True), (p_base_m, p, False)]
    out += [(65, 17, True), (65, 17, False)]
    return sorted({c for c in out if c[1] >= 1 or not c[2]})


def _ids(cs):
    return [f"m = {m} p = {p} r {'in' if ins else 'not in'} S" for m, p, ins in cs]


def operands(m, p, r_in_s, seed, kmax_full=None):
    rng = np.random.default_rng(seed + 13 * m + 101 * p + r_in_s)
    W = kh.real_data(rng, (p, m), 0.1, 0.05)
    S = kh.distinct_rows(rng, m, p)
    if r_in_s and p > 0:
        r = int(S[p // 2])
    else:
        free = np.setdiff1d(np.arange(m), S)
        r = int(free[len(free) // 2])
    kmax = 128 if (kmax_full if kmax_full is not None else (m + p) % 2) else p + (0 if r_in_s else 1)
    return rng, W, S, r, min(kmax, 128)


R1_CASES = sorted({(m, p, True) for m, p, _ in cases()})          # (r plays no part in alpha = v + W (S'v))


@pytest.mark.parametrize("m,p,r_in_s", R1_CASES, ids=[f"m = {m} p = {p}" for m, p, _ in R1_CASES])
def test_apply_w(m, p, r_in_s):
    rng, W, S, _, kmax = operands(m, p, True, 100)
    v = kh.real_data(rng, m, 0.1, 0.05)
    want = kh.model_apply_w(W, S, v)
    out = kh.apply_w(W, S, v, kmax)
    ok(kh.diff_values(out["alpha"][:m], want, "alpha"), kh.sentinel_violations(out["alpha"][m:], "alpha padding"),
       kh.diff_unchanged(kh.image(out["W"], kmax, kh.ld_b(m)), kh.w_image(W, m, p, kmax), "W"),
       kh.diff_unchanged(out["v"], kh.vec_image(v, m, kh.ld_b(m)), "v"))
    for i in {0, m - 1, m // 2}:
        assert want[i] == kh.chain_exact(v[i], W[:, i], v[S])


R2_CASES = [c for c in cases() if c[2] or c[1] < 128]          # a new row needs a free column of W


@pytest.mark.parametrize("m,p,r_in_s", R2_CASES, ids=_ids(R2_CASES))
def test_eta_prepare_update_w(m, p, r_in_s):
    rng, W, S, r, kmax = operands(m, p, r_in_s, 200)
    if p:
        W[rng.random(p) < 0.25, r] = 0.0                          # zero factors in row r of W
    alpha = kh.real_data(rng, m, 0.2, 0.1)                        # alpha with exact zeros of both signs
    alpha[r] = -1.375 if m % 2 else 1.75
    mod = kh.model_eta_update_w(W, S, alpha, r)
    p_new = mod["n_eta"]
    assert p_new == p + (0 if r_in_s else 1)
    out = kh.eta_update_w(W, S, alpha, kmax, r)
    w = kh.image(out["W"], kmax, kh.ld_b(m))
    pos = np.full(m, -1, dtype=np.int32)
    pos[mod["S"]] = np.arange(p_new)
    ok(kh.diff_bits(out["wr"][:p], mod["wr"], "wr"), kh.sentinel_violations(out["wr"][p:], "wr past p"),
       kh.diff_values(out["S"][:p_new], mod["S"], "S"), kh.sentinel_violations(out["S"][p_new:], "S past p"),
       kh.diff_values(out["pos"], pos, "pos_of_row"),
       kh.diff_bits(w[:p_new, :m], mod["W"], "W"),
       kh.sentinel_violations(w[:p_new, m:], "W padding"), kh.sentinel_violations(w[p_new:], "W past p"),
       kh.diff_unchanged(out["alpha"], kh.vec_image(alpha, m, kh.ld_b(m)), "alpha"))
    assert list(out["irec"]) == [p_new, mod["jt"], p]
    # the Fraction chain at a few entries: u by one IEEE division, one fma where neither factor is zero, the target column
    ar = alpha[r]
    for i in {0, m - 1, m // 2, r}:
        u = 1.0 / ar - 1.0 if i == r else -alpha[i] / ar
        for j in {j for j in (0, p - 1, mod["jt"]) if 0 <= j < p}:
            e = kh.fma_exact(u, W[j, r], W[j, i]) if (u != 0.0 and W[j, r] != 0.0) else W[j, i]
            if j == mod["jt"]:
                e = e + u
            assert kh.bits(np.array([e]))[0] == kh.bits(mod["W"][j, i:i + 1])[0]
        if not r_in_s:
            assert mod["W"][p, i] == u


R3_CASES = cases()


@pytest.mark.parametrize("m,p,r_in_s", R3_CASES, ids=_ids(R3_CASES))
def test_rho_deferred(m, p, r_in_s):
    """Values only: the 8-unrolled part of k_rho_deferred adds 0 * x for a zero coefficient, its tail skips it, and the
    documentation leaves the sign of a zero open."""
    rng, W, S, r, kmax = operands(m, p, r_in_s, 300)
    if p:
        W[rng.random(p) < 0.3, r] = 0.0                           # zero coefficients in the unrolled part and in the tail
        if p >= 9:
            W[[0, 7, p - 1], r] = 0.0
    Binv = kh.real_data(rng, (m, m), 0.1, 0.05)
    want = kh.model_rho_deferred(W, S, Binv, r)
    out = kh.rho_deferred(W, S, Binv, kmax, r)
    ok(kh.diff_values(out["rho"][:m], want, "rho"), kh.diff_values(out["rho"][m:], np.zeros(kh.ld_b(m) - m), "rho padding"),
       kh.diff_unchanged(kh.image(out["W"], kmax, kh.ld_b(m)), kh.w_image(W, m, p, kmax), "W"),
       kh.diff_unchanged(kh.image(out["Binv"], m, kh.ld_b(m)), kh.binv_image(Binv, m), "Binv"))
    for c in {0, m - 1, m // 2}:
        nz = [j for j in range(p) if W[j, r] != 0.0]
        assert want[c] == kh.chain_exact(Binv[r, c], W[nz, r], Binv[S[nz], c])


R4_CASES = cases(p_base_m=129)


@pytest.mark.parametrize("m,p,r_in_s", [c for c in R4_CASES if c[2]], ids=_ids([c for c in R4_CASES if c[2]]))
def test_flush_snapshot_apply_reset(m, p, r_in_s):
    rng, W, S, _, kmax = operands(m, p, True, 400)
    Binv = kh.real_data(rng, (m, m), 0.1, 0.05)
    want, R = kh.model_flush_revised(W, S, Binv)
    out = kh.flush_revised(W, S, Binv, kmax)
    b = kh.image(out["Binv"], m, kh.ld_b(m))
    snap = kh.image(out["R"], kmax, kh.ld_b(m))
    ok(kh.diff_values(b[:, :m], want, "B0inv"), kh.diff_values(b[:, m:], np.zeros((m, kh.ld_b(m) - m)), "B0inv padding"),
       kh.diff_unchanged(snap[:p], kh.binv_image(Binv, m)[S], "snapshot"), kh.sentinel_violations(snap[p:], "snapshot past p"),
       kh.diff_unchanged(kh.image(out["W"], kmax, kh.ld_b(m)), kh.w_image(W, m, p, kmax), "W"),
       kh.diff_values(out["pos"], np.full(m, -1, dtype=np.int32), "pos_of_row"),
       kh.diff_values(out["S"][:p], S, "S"), kh.sentinel_violations(out["S"][p:], "S past p"))
    assert list(out["irec"]) == [0, 0, 0]
    # the accumulator starts at 0 and is added to the stored entry once at the end
    for i, c in {(0, 0), (m - 1, m - 1), (m // 2, m - 1), (m - 1, m // 3), (min(63, m - 1), min(64, m - 1))}:
        assert want[i, c] == Binv[i, c] + kh.chain_exact(0.0, W[:, i], Binv[S, c])


R5_M = sorted(set(M_ALL))


@pytest.mark.parametrize("m", R5_M, ids=[f"m = {m}" for m in R5_M])
@pytest.mark.parametrize("r_at", ["first", "middle", "last"])
def test_compute_rho_update_inverse(m, r_at):
    rng = np.random.default_rng(500 + m + len(r_at))
    r = {"first": 0, "middle": m // 2, "last": m - 1}[r_at]
    Binv = kh.real_data(rng, (m, m), 0.1, 0.1)                    # exact zeros and -0.0 in the rows that must keep their bits
    alpha = kh.real_data(rng, m, 0.25, 0.1)                       # alpha with exact zeros of both signs
    alpha[r] = -1.375 if m % 2 else 1.75
    want, rho = kh.model_explicit_update(Binv, alpha, r)
    out = kh.explicit_update(Binv, alpha, r)
    b = kh.image(out["Binv"], m, kh.ld_b(m))
    untouched = np.nonzero((alpha == 0.0) & (np.arange(m) != r))[0]
    ok(kh.diff_values(out["rho"][:m], rho, "rho"), kh.diff_bits(out["rho"][m:], np.zeros(kh.ld_b(m) - m), "rho padding"),
       kh.diff_values(b[:, :m], want, "B^-1"), kh.diff_bits(b[r], out["rho"], "row r := rho"),
       kh.diff_unchanged(b[untouched, :m], Binv[untouched], "rows with alpha_i == 0"),
       kh.diff_values(b[:, m:], np.zeros((m, kh.ld_b(m) - m)), "B^-1 padding"),
       kh.diff_unchanged(out["alpha"], kh.vec_image(alpha, m, kh.ld_b(m)), "alpha"))
    for i, c in {(0, 0), (m - 1, m - 1), (m // 2, 0), (r, m // 2)}:
        rc = Binv[r, c] / alpha[r]
        e = rc if i == r else (kh.fma_exact(-alpha[i], rc, Binv[i, c]) if alpha[i] != 0.0 else Binv[i, c])
        assert want[i, c] == e
