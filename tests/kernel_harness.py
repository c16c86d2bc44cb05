"""Helper module of the kernel tests (not collected by pytest): the ctypes binding of tests/kernels/librelp_kernel_harness.so,
the reference models of the blocked-update launchers in numpy + fractions.Fraction, and the comparison functions.

Reference arithmetic.  The kernels document one fma per pending row in ascending j and one IEEE division for u, theta and
b_r / alpha_r.  ``fma_exact`` is the correctly rounded fma, float(Fraction(a) * Fraction(b) + Fraction(c)), with IEEE signed
zeros.  ``fma_vec`` is the same function over numpy arrays (error-free product and sum, then one rounding to odd and one to
nearest: Boldo & Melquiond, "Emulation of a FMA and correctly rounded sums", IEEE TC 2008); tests/test_kernel_models.py holds it
to ``fma_exact`` bit for bit, and every GPU case re-checks a fixed sample of its entries with the Fraction chain itself.

Layouts.  Logical arrays are C-ordered: T0[c][i] (n_owned x m), W[j][i] (p x m), R0[j][c] (p x n_owned), Binv[i][j] (m x m).
The harness returns whole device images: T0 n_owned x ld_t, W kmax x ld_b, R0 (kmax + 1) x ld_r, Binv m x ld_b; the functions
below cut them into the logical part and the rest.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "kernels", "librelp_kernel_harness.so")

REFUSED_SHAPE, REFUSED_INDEX, REFUSED_BATCH, REFUSED_LENGTH = -1, -2, -3, -4
HIP_ERROR_BASE = 1000
SENTINEL_BITS = np.uint64(0x7FF80000C0FFEE01)
SENTINEL = np.array([SENTINEL_BITS], dtype=np.uint64).view(np.float64)[0]
SENTINEL_INT = -0x5A5A5A5B
WRAPPED_ARTIFICIAL_BASE = 1 << 30         # relp_layout.hpp: kWrappedArtificialBase (checked against the library on load)
EPS53 = 2.0 ** -53
FLUSH_LDS_THRESHOLD = 1 << 16            # launch_tab_flush: n_owned * m >= this -> the LDS-staged kernels
BATCHES = (1, 8, 16, 32)


def round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def ld_b(m): return round_up(m, 16)
def ld_t(m): return round_up(m, 2)
def ld_r(n): return round_up(n, 2)
def scan_blocks(n): return (n + 255) // 256


# ------------------------------------------------------------------------------------------------------------------------
# binding
# ------------------------------------------------------------------------------------------------------------------------
class HarnessRefused(Exception):
    def __init__(self, code):
        super().__init__(f"the harness refused the call (code {code})")
        self.code = code


class HarnessFault(Exception):
    """A HIP call of the harness failed (now or earlier in this process: the error is sticky)."""


_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run build() (make -C tests/kernels)")
        _lib = C.CDLL(LIB_PATH)
        _lib.rkh_sentinel_bits.restype = C.c_uint64
        assert np.uint64(_lib.rkh_sentinel_bits()) == SENTINEL_BITS
        assert _lib.rkh_sentinel_int() == SENTINEL_INT
        assert _lib.rkh_wrapped_artificial_base() == WRAPPED_ARTIFICIAL_BASE
    return _lib


def _call(name, scalars, arrays):
    """lib.name(*scalars, *(pointer, length of every array)).  Input arrays must already have their dtype."""
    lib = load()
    sticky = lib.rkh_sticky_error()
    if sticky:
        raise HarnessFault(f"an earlier harness call failed with HIP error {sticky - HIP_ERROR_BASE}; nothing is launched any more")
    args = [C.c_int64(int(s)) if wide else C.c_int(int(s)) for s, wide in scalars]
    for a in arrays:
        assert a.flags["C_CONTIGUOUS"]
        args += [C.c_void_p(a.ctypes.data), C.c_int64(a.size)]
    fn = getattr(lib, name)
    fn.restype = C.c_int
    rc = fn(*args)
    if rc < 0:
        raise HarnessRefused(rc)
    if rc:
        raise HarnessFault(f"{name}: HIP error {rc - HIP_ERROR_BASE}")


def _f64(a): return np.ascontiguousarray(a, dtype=np.float64)
def _i32(a): return np.ascontiguousarray(a, dtype=np.int32)
def _w(x): return (x, True)
def _n(x): return (x, False)


def tab_flush(T0, W, R0, kmax, c_lo=0, listed=False, fill=True, stats=(0, 0), lengths=None):
    """launch_tab_flush.  Returns a dict of whole device images."""
    T0, W, R0 = _f64(T0), _f64(W), _f64(R0)
    n, m = T0.shape
    p = W.shape[0]
    L = dict(T0=n * ld_t(m), W=kmax * ld_b(m), R0=(kmax + 1) * ld_r(n), cols=n, count=1, R0c=kmax * ld_r(n), stats=2)
    L.update(lengths or {})
    out = dict(T0=np.zeros(L["T0"]), W=np.zeros(L["W"]), R0=np.zeros(L["R0"]), cols=np.zeros(L["cols"], np.int32),
               count=np.zeros(L["count"], np.int32), R0c=np.zeros(L["R0c"]), stats=np.zeros(L["stats"], np.uint64))
    _call("rkh_tab_flush", [_w(m), _w(n), _w(p), _w(kmax), _w(c_lo), _n(listed), _n(fill)],
          [T0, W, R0, np.array(stats, dtype=np.uint64), out["T0"], out["W"], out["R0"], out["cols"], out["count"], out["R0c"],
           out["stats"]])
    return out


def tab_vector(T0, W, R0, kmax, c_lo=0, batch=8, q=0, row=-1, fill=True, lengths=None):
    """launch_tab_column (row < 0: column q, counted from c_lo) or launch_tab_row (row >= 0)."""
    T0, W, R0 = _f64(T0), _f64(W), _f64(R0)
    n, m = T0.shape
    p = W.shape[0]
    L = dict(vec=ld_r(n) if row >= 0 else ld_b(m), T0=n * ld_t(m), W=kmax * ld_b(m), R0=(kmax + 1) * ld_r(n))
    L.update(lengths or {})
    out = {k: np.zeros(v) for k, v in L.items()}
    _call("rkh_tab_vector", [_w(m), _w(n), _w(p), _w(kmax), _w(c_lo), _n(batch), _w(q), _w(row), _n(fill)],
          [T0, W, R0, out["vec"], out["T0"], out["W"], out["R0"]])
    return out


def tab_update_all(T0, W, R0, S, d, in_basis, alpha, b, basis, kmax, r, q, c_lo=0, batch=8, fill=True, rule=0, last_selected=-1,
                   leaving=0, phase=2, degenerate=0, iterations=0, trace_cap=8, tol_cost=1e-9, minus_objective=0.0, lengths=None):
    T0, W, R0 = _f64(T0), _f64(W), _f64(R0)
    n, m = T0.shape
    p = W.shape[0]
    na = c_lo + n
    L = dict(T0=n * ld_t(m), W=kmax * ld_b(m), R0=(kmax + 1) * ld_r(n), wr=kmax, S=kmax, pos=m, d=na, k1=scan_blocks(n),
             j=scan_blocks(n), alpha=ld_b(m), b=ld_b(m), basis=m, in_basis=na, trace=4 * trace_cap, irec=8, lrec=1, drec=1)
    L.update(lengths or {})
    dt = dict(S=np.int32, pos=np.int32, j=np.int32, basis=np.int32, in_basis=np.uint8, trace=np.int32, irec=np.int32, lrec=np.int64)
    out = {k: np.zeros(v, dtype=dt.get(k, np.float64)) for k, v in L.items()}
    _call("rkh_tab_update_all", [_w(m), _w(n), _w(p), _w(kmax), _w(c_lo), _n(batch), _w(r), _w(q), _n(fill)],
          [_i32([rule, last_selected, leaving, phase, degenerate]), np.array([iterations, trace_cap], dtype=np.int64),
           _f64([tol_cost, minus_objective]), T0, W, R0, _i32(S), _f64(d), np.ascontiguousarray(in_basis, dtype=np.uint8),
           _f64(alpha), _f64(b), _i32(basis)] +
          [out[k] for k in ("T0", "W", "R0", "wr", "S", "pos", "d", "k1", "j", "alpha", "b", "basis", "in_basis", "trace", "irec",
                            "lrec", "drec")])
    return out


def apply_w(W, S, v, kmax, fill=True, lengths=None):
    W = _f64(W)
    p, m = W.shape
    L = dict(alpha=ld_b(m), W=kmax * ld_b(m), v=ld_b(m))
    L.update(lengths or {})
    out = {k: np.zeros(x) for k, x in L.items()}
    _call("rkh_apply_w", [_w(m), _w(p), _w(kmax), _n(fill)], [W, _i32(S), _f64(v), out["alpha"], out["W"], out["v"]])
    return out


def eta_update_w(W, S, alpha, kmax, r, fill=True, lengths=None):
    W = _f64(W)
    p, m = W.shape
    L = dict(W=kmax * ld_b(m), wr=kmax, S=kmax, pos=m, irec=3, alpha=ld_b(m))
    L.update(lengths or {})
    dt = dict(S=np.int32, pos=np.int32, irec=np.int32)
    out = {k: np.zeros(x, dtype=dt.get(k, np.float64)) for k, x in L.items()}
    _call("rkh_eta_update_w", [_w(m), _w(p), _w(kmax), _w(r), _n(fill)],
          [W, _i32(S), _f64(alpha), out["W"], out["wr"], out["S"], out["pos"], out["irec"], out["alpha"]])
    return out


def rho_deferred(W, S, Binv, kmax, r, fill=True, lengths=None):
    W, Binv = _f64(W), _f64(Binv)
    p, m = W.shape
    L = dict(rho=ld_b(m), W=kmax * ld_b(m), Binv=m * ld_b(m))
    L.update(lengths or {})
    out = {k: np.zeros(x) for k, x in L.items()}
    _call("rkh_rho_deferred", [_w(m), _w(p), _w(kmax), _w(r), _n(fill)], [W, _i32(S), Binv, out["rho"], out["W"], out["Binv"]])
    return out


def flush_revised(W, S, Binv, kmax, fill=True, lengths=None):
    W, Binv = _f64(W), _f64(Binv)
    p, m = W.shape
    L = dict(Binv=m * ld_b(m), W=kmax * ld_b(m), R=kmax * ld_b(m), pos=m, S=kmax, irec=3)
    L.update(lengths or {})
    dt = dict(S=np.int32, pos=np.int32, irec=np.int32)
    out = {k: np.zeros(x, dtype=dt.get(k, np.float64)) for k, x in L.items()}
    _call("rkh_flush_revised", [_w(m), _w(p), _w(kmax), _n(fill)],
          [W, _i32(S), Binv, out["Binv"], out["W"], out["R"], out["pos"], out["S"], out["irec"]])
    return out


def explicit_update(Binv, alpha, r, fill=True, lengths=None):
    Binv = _f64(Binv)
    m = Binv.shape[0]
    L = dict(rho=ld_b(m), Binv=m * ld_b(m), alpha=ld_b(m))
    L.update(lengths or {})
    out = {k: np.zeros(x) for k, x in L.items()}
    _call("rkh_explicit_update", [_w(m), _w(r), _n(fill)], [_f64(alpha), Binv, out["rho"], out["Binv"], out["alpha"]])
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the fma
# ------------------------------------------------------------------------------------------------------------------------
def _neg(x) -> bool:
    return bool(np.signbit(x))


def fma_exact(a: float, b: float, c: float) -> float:
    """Correctly rounded a * b + c (finite arguments), with the signed zeros of IEEE 754 round-to-nearest."""
    a, b, c = float(a), float(b), float(c)
    if a == 0.0 or b == 0.0:
        if c != 0.0:
            return c
        return -0.0 if (_neg(a) != _neg(b)) and _neg(c) else 0.0
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        return 0.0                              # exact cancellation of nonzero terms: +0
    return float(exact)


def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_vec(a, b, c):
    """fma_exact over arrays (broadcast).  Magnitudes must stay clear of overflow and of the subnormal range."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        s, e = _two_sum(tl, ul)                 # v = round-to-odd(tl + ul)
        bits = s.copy().view(np.int64)
        fix = (e != 0.0) & ((bits & 1) == 0)
        step = np.where((e > 0.0) == (s > 0.0), 1, -1)
        v = np.where(fix, bits + step, bits).astype(np.int64).view(np.float64)
        z = th + v
        plain = (a == 0.0) | (b == 0.0) | ~np.isfinite(a) | ~np.isfinite(b) | ~np.isfinite(c)
        return np.where(plain, a * b + c, z)


def chain_exact(base: float, xs, ys) -> float:
    """base = fma(xs[j], ys[j], base) for ascending j, with the Fraction fma."""
    for x, y in zip(xs, ys):
        base = fma_exact(x, y, base)
    return base


# ------------------------------------------------------------------------------------------------------------------------
# models (logical arrays in, logical arrays out)
# ------------------------------------------------------------------------------------------------------------------------
def model_tab_column(T0, W, R0, q):
    a = np.array(T0[q], dtype=np.float64)
    for j in range(W.shape[0]):
        a = fma_vec(W[j], R0[j, q], a)
    return a


def model_tab_row(T0, W, R0, row):
    t = np.array(T0[:, row], dtype=np.float64)
    for j in range(W.shape[0]):
        t = fma_vec(W[j, row], R0[j], t)
    return t


def select_key(rule, n, last_selected, j, d_j):
    if rule == 2:
        return d_j
    last = last_selected if rule == 1 else -1
    if last >= 0:
        return float(j - last if j >= last else j - last + n)
    return float(j)


def model_update_w(W, wr, alpha, r, jt):
    """W <- E W and the target column; returns (new W with p or p + 1 rows, u)."""
    p, m = W.shape
    ar = alpha[r]
    with np.errstate(all="ignore"):
        u = -alpha / ar
        u[r] = 1.0 / ar - 1.0
    Wn = np.array(W, dtype=np.float64)
    for j in range(p):
        if wr[j] != 0.0:
            upd = fma_vec(u, wr[j], W[j])
            Wn[j] = np.where(u != 0.0, upd, W[j])
    if jt < p:
        Wn[jt] = Wn[jt] + u
    else:
        Wn = np.vstack([Wn, u[None, :]])
    return Wn, u


def model_pivot_b(alpha, b, r):
    br = b[r] / alpha[r]
    out = np.where(alpha != 0.0, fma_vec(-alpha, br, b), b)
    out[r] = br
    return out, br


def model_tab_update_all(T0, W, R0, S, d, in_basis, alpha, b, basis, r, q, c_lo=0, rule=0, last_selected=-1, leaving=0, phase=2,
                         degenerate=0, iterations=0, trace_cap=8, tol_cost=1e-9, minus_objective=0.0):
    """The unfused per-pivot update as k_tab_update_all documents it.  q counts from c_lo; keys use storage columns."""
    n, m = T0.shape
    p = W.shape[0]
    S = list(S)
    jt = S.index(r) if r in S else p
    wr = np.array(W[:, r], dtype=np.float64)
    alpha_r, b_r, d_q = alpha[r], b[r], d[q]
    base = R0[jt] if jt < p else T0[:, r]
    row = np.array(base, dtype=np.float64)
    for j in range(p):
        row = fma_vec(wr[j], R0[j], row)
    theta = d_q / alpha_r
    dn = fma_vec(-theta, row, d)
    dn[q] = 0.0
    R0n = np.array(R0, dtype=np.float64) if jt < p else np.vstack([R0, np.array(base)[None, :]])
    n_all = c_lo + n
    k1 = np.full(scan_blocks(n), np.inf)
    kj = np.full(scan_blocks(n), 0x7FFFFFFF, dtype=np.int64)
    for c in range(n):
        j = c_lo + c
        basic = (c == q) or (in_basis[c] and j != leaving)
        if not basic and dn[c] < -tol_cost:
            key = select_key(rule, n_all, last_selected, j, dn[c])
            blk = c // 256
            if key < k1[blk] or (key == k1[blk] and j < kj[blk]):
                k1[blk], kj[blk] = key, j
    Wn, _ = model_update_w(W, wr, alpha, r, jt)
    bn, br = model_pivot_b(alpha, b, r)
    basis_n = np.array(basis, dtype=np.int32)
    basis_n[r] = c_lo + q
    inb = np.zeros(n_all, dtype=np.uint8)
    inb[c_lo:] = in_basis
    if leaving < WRAPPED_ARTIFICIAL_BASE:
        inb[leaving] = 0
    inb[c_lo + q] = 1
    trace = np.full((4, trace_cap), SENTINEL_INT, dtype=np.int32)
    if iterations < trace_cap:
        trace[:, iterations] = (phase, c_lo + q, r, leaving)
    Sn = S + [r] if jt == p else S
    pos = np.full(m, -1, dtype=np.int32)
    for j, s in enumerate(Sn):
        pos[s] = j
    return dict(R0=R0n, d=dn, k1=k1, j=kj.astype(np.int32), W=Wn, b=bn, basis=basis_n, in_basis=inb, trace=trace.reshape(-1),
                wr=wr, S=np.array(Sn, dtype=np.int32), pos=pos, jt=jt, n_eta=len(Sn),
                minus_objective=fma_exact(-d_q, br, minus_objective), iterations=iterations + 1,
                degenerate=degenerate + (1 if br == 0.0 else 0))


def model_apply_w(W, S, v):
    a = np.array(v, dtype=np.float64)
    for j in range(W.shape[0]):
        a = fma_vec(W[j], v[S[j]], a)
    return a


def model_eta_update_w(W, S, alpha, r):
    p = W.shape[0]
    S = list(S)
    jt = S.index(r) if r in S else p
    wr = np.array(W[:, r], dtype=np.float64)
    Wn, _ = model_update_w(W, wr, np.array(alpha, dtype=np.float64), r, jt)
    Sn = S + [r] if jt == p else S
    return dict(W=Wn, wr=wr, S=np.array(Sn, dtype=np.int32), jt=jt, n_eta=len(Sn), n_eta_old=p)


def model_rho_deferred(W, S, Binv, r):
    """rho = Binv[r] + sum_j W[j][r] Binv[S[j]], ascending j.  A zero coefficient contributes 0 * x in the 8-unrolled part of the
    kernel and nothing in its tail: the VALUE is the same, the sign of a zero is not documented."""
    acc = np.array(Binv[r], dtype=np.float64)
    for j in range(W.shape[0]):
        if W[j, r] != 0.0:
            acc = fma_vec(W[j, r], Binv[S[j]], acc)
    return acc


def model_flush_revised(W, S, Binv):
    """Binv + (sum_k W[k][i] R[k][c] accumulated from 0 in ascending k), the sum added to the stored entry once."""
    p, m = W.shape
    R = np.array(Binv[np.asarray(S, dtype=np.int64)], dtype=np.float64).reshape(p, m)
    acc = np.zeros((m, m))
    for k in range(p):
        acc = fma_vec(W[k][:, None], R[k][None, :], acc)
    return Binv + acc, R


def model_explicit_update(Binv, alpha, r):
    rho = Binv[r] / alpha[r]
    out = np.array(Binv, dtype=np.float64)
    for i in range(Binv.shape[0]):
        if i == r:
            out[i] = rho
        elif alpha[i] != 0.0:
            out[i] = fma_vec(-alpha[i], rho, Binv[i])
    return out, rho


# the flush of the tableau engine ------------------------------------------------------------------------------------------
def model_flush_int(T0, W, R0):
    """T0 + W' R0 for integer-valued operands, in int64 (exact; every order of summation gives this float64)."""
    Ti, Wi, Ri = (np.asarray(x).astype(np.int64) for x in (T0, W, R0))
    assert (Ti == T0).all() and (Wi == W).all() and (Ri == R0).all(), "integer data expected"
    return (Ti + Ri.T @ Wi).astype(np.float64)


def selector_operands(m, n, p):
    """W[j][i] = 1 where j == i mod p, R0[j][c] = 1 + c + 1000 j: (T - T0)[c][i] names the R0 row and column that reached it."""
    W = np.zeros((p, m))
    if p:
        W[np.arange(m) % p, np.arange(m)] = 1.0
    R0 = 1.0 + np.arange(n)[None, :] + 1000.0 * np.arange(p)[:, None]
    return W, R0


def model_flush_selector(m, n, p):
    """The expected T - T0 of selector_operands, written down directly (not through a product)."""
    if p == 0:
        return np.zeros((n, m))
    return 1.0 + np.arange(n)[:, None] + 1000.0 * (np.arange(m)[None, :] % p)


def flush_exact_entry(T0, W, R0, c, i):
    """(exact rational T[c][i], S = |T0| + sum |W||R0|)"""
    t = Fraction(float(T0[c, i]))
    s = abs(t)
    for j in range(W.shape[0]):
        term = Fraction(float(W[j, i])) * Fraction(float(R0[j, c]))
        t += term
        s += abs(term)
    return t, s


def flush_sample(m, n, seed, count=200, tile_rows=(16, 32, 64, 128), tile_cols=(16, 64, 128)):
    """Every tile corner (rows / columns next to a multiple of a tile edge, first and last) plus `count` seeded entries."""
    def edges(size, tiles):
        e = {0, size - 1}
        for t in tiles:
            for k in range(t, size + 1, t):
                e.update(x for x in (k - 1, k) if 0 <= x < size)
        return sorted(e)
    rows, cols = edges(m, tile_rows), edges(n, tile_cols)
    if len(rows) * len(cols) > 400:           # keep the corners of the largest tiles and the ends
        rows, cols = edges(m, (128,)), edges(n, (128,))
    pts = {(c, i) for c in cols for i in rows}
    rng = np.random.default_rng(seed)
    pts.update(zip(rng.integers(0, n, count).tolist(), rng.integers(0, m, count).tolist()))
    return sorted(pts)


def flush_real_check(got, T0, W, R0, sample):
    """Entries of `sample` against the exact value with the a-priori bound (2p + 1) 2^-53 (|T0| + sum |W||R0|).
    Returns (violations, largest error / (2^-53 S))."""
    p = W.shape[0]
    bad, worst = [], 0.0
    for c, i in sample:
        g = float(got[c, i])
        if not np.isfinite(g):
            bad.append((c, i, g, "not finite"))
            continue
        t, s = flush_exact_entry(T0, W, R0, c, i)
        err = abs(Fraction(g) - t)
        if s > 0:
            worst = max(worst, float(err / (Fraction(EPS53) * s)))
        if err > (2 * p + 1) * Fraction(EPS53) * s:
            bad.append((c, i, g, float(t)))
    return bad, worst


# ------------------------------------------------------------------------------------------------------------------------
# images and comparison functions (each returns a list of findings; empty = nothing to report)
# ------------------------------------------------------------------------------------------------------------------------
def image(flat, rows, ld):
    return np.asarray(flat).reshape(rows, ld)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def diff_values(got, want, what="values", limit=5):
    """Entries that differ as float64 VALUES (+0 == -0); a NaN on either side is always a finding."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return [f"{what}: shape {got.shape} != {want.shape}"]
    if got.dtype.kind == "f":
        bad = ~(got == want)                    # NaN compares unequal to everything
    else:
        bad = got != want
    idx = np.argwhere(bad)
    return [f"{what}{tuple(i)}: got {got[tuple(i)]!r}, want {want[tuple(i)]!r}" for i in idx[:limit]] + \
           ([f"{what}: {len(idx)} entries differ"] if len(idx) > limit else [])


def diff_bits(got, want, what="bits", limit=5):
    """Entries whose bit patterns differ (-0.0 != +0.0); a NaN in `got` is a finding even when `want` holds the same one."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return [f"{what}: shape {got.shape} != {want.shape}"]
    bad = (bits(got) != bits(want)).reshape(got.shape) | np.isnan(got)
    idx = np.argwhere(bad)
    return [f"{what}{tuple(i)}: got {got[tuple(i)]!r} ({bits(got).reshape(got.shape)[tuple(i)]:#x}), want {want[tuple(i)]!r}"
            for i in idx[:limit]] + ([f"{what}: {len(idx)} entries differ"] if len(idx) > limit else [])


def diff_unchanged(got, before, what="const", limit=5):
    """A buffer the launcher takes as const (or must leave alone): bit for bit what was uploaded, NaN sentinels included."""
    got, before = np.asarray(got), np.asarray(before)
    if got.shape != before.shape:
        return [f"{what}: shape {got.shape} != {before.shape}"]
    if got.dtype.kind == "f":
        bad = (bits(got) != bits(before)).reshape(got.shape)
    else:
        bad = got != before
    idx = np.argwhere(bad)
    return [f"{what}{tuple(i)} was rewritten: {got[tuple(i)]!r}" for i in idx[:limit]] + \
           ([f"{what}: {len(idx)} entries rewritten"] if len(idx) > limit else [])


def sentinel_violations(region, what="sentinel", limit=5):
    """Words of a region that must still hold the sentinel's bit pattern (float64 regions) or SENTINEL_INT (int32 regions)."""
    region = np.asarray(region)
    if region.dtype.kind == "f":
        bad = bits(region).reshape(region.shape) != SENTINEL_BITS
    else:
        bad = region != SENTINEL_INT
    idx = np.argwhere(bad)
    return [f"{what}{tuple(i)} was written: {region[tuple(i)]!r}" for i in idx[:limit]] + \
           ([f"{what}: {len(idx)} words written"] if len(idx) > limit else [])


def tab_images(out, m, n, p, kmax, T0, W, R0, fill=True):
    """What was uploaded for T0, W, R0 by the harness's rules (whole images), to compare returned images with."""
    f = SENTINEL if fill else 0.0
    t = np.full((n, ld_t(m)), f); t[:, :m] = T0
    w = np.full((kmax, ld_b(m)), f); w[:p, :m] = W
    r = np.full((kmax + 1, ld_r(n)), f); r[:p, :n] = R0
    return t, w, r


def w_image(W, m, p, kmax, fill=True):
    w = np.full((kmax, ld_b(m)), SENTINEL if fill else 0.0)
    w[:p, :m] = W
    return w


def binv_image(Binv, m):
    b = np.zeros((m, ld_b(m)))
    b[:, :m] = Binv
    return b


def vec_image(v, m, length, fill=True):
    a = np.full(length, SENTINEL if fill else 0.0)
    a[:m] = v
    return a


# ------------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------------
def real_data(rng, shape, zeros=0.0, neg_zeros=0.0):
    """Magnitudes uniform in [0.5, 2) with random signs; a share of exact +0.0 and of -0.0 mixed in."""
    a = rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    if zeros:
        a[rng.random(shape) < zeros] = 0.0
    if neg_zeros:
        a[rng.random(shape) < neg_zeros] = -0.0
    return a


def int_data(rng, shape, zeros=0.3):
    a = rng.integers(-8, 9, shape).astype(np.float64)
    a[rng.random(shape) < zeros] = 0.0
    return a


def distinct_rows(rng, m, p):
    return rng.permutation(m)[:p].astype(np.int32)
