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

T5 - T8 (the in-place changes and the batched ratio queries, at the end of the file): the models return the whole EXPECTED image
of every buffer, the sentinel where the launcher must not write, and ``diff_image`` compares image with image.  Their case tables
are in tests/kernel_query_cases.py.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
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
            # build() makes it; a tests/ directory put in place after the build has lost it, so make it here as the tests of
            # tests/cpp make their programs (the Makefile needs the engine library build() made: without it make fails)
            made = subprocess.run(["make", "-C", os.path.dirname(LIB_PATH), "ARCH=gfx950"], capture_output=True, text=True)
            if made.returncode:
                raise FileNotFoundError(f"{LIB_PATH} is missing and make -C tests/kernels failed: run build()\n{made.stderr[-2000:]}")
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run build() (make -C tests/kernels)")
        _lib = C.CDLL(LIB_PATH)
        _lib.rkh_sentinel_bits.restype = C.c_uint64
        assert np.uint64(_lib.rkh_sentinel_bits()) == SENTINEL_BITS
        assert _lib.rkh_sentinel_int() == SENTINEL_INT
        assert _lib.rkh_wrapped_artificial_base() == WRAPPED_ARTIFICIAL_BASE
    return _lib


def invoke(name, *args):
    """Every call of the library that may launch goes through here: nothing is called once the library's sticky HIP error is set
    (one for all families), a negative return code is a refusal, any other a HIP error.  `args` are ctypes values."""
    lib = load()
    sticky = lib.rkh_sticky_error()
    if sticky:
        raise HarnessFault(f"an earlier harness call failed with HIP error {sticky - HIP_ERROR_BASE}; nothing is launched any more")
    fn = getattr(lib, name)
    fn.restype = C.c_int
    rc = fn(*args)
    if rc < 0:
        raise HarnessRefused(rc)
    if rc:
        raise HarnessFault(f"{name}: HIP error {rc - HIP_ERROR_BASE}")


def _call(name, scalars, arrays, reals=(), lengths=None):
    """lib.name(*scalars, *reals, *(pointer, length of every array)); the family modules tests/kernel_harness_*.py call through
    here too.  A scalar is an int (passed as int64) or (value, wide); the reals are passed as doubles.  `arrays` is a list of arrays
    or a dict of named images; `lengths` overrides the length passed for a named image (the refusal tests).  Input arrays must
    already have their dtype."""
    args = []
    for s in scalars:
        value, wide = s if isinstance(s, tuple) else (s, True)
        args.append(C.c_int64(int(value)) if wide else C.c_int(int(value)))
    args += [C.c_double(r) for r in reals]
    for key, a in (arrays.items() if isinstance(arrays, dict) else enumerate(arrays)):
        assert a.flags["C_CONTIGUOUS"]
        args += [C.c_void_p(a.ctypes.data), C.c_int64((lengths or {}).get(key, a.size))]
    invoke(name, *args)


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


# ========================================================================================================================
# T5 - T8: the in-place changes (launch_tab_rhs_change, launch_tab_cost_change) and the batched ratio queries
# (launch_tab_row_ratios, launch_tab_rhs_ranging)
# ========================================================================================================================
REFUSED_SPLITS, REFUSED_ORDER = -5, -6
MAX_SPLITS = 256                         # kTabRhsMaxSplits = kTabCostMaxSplits
RHS_GRID, COST_GRID, COST_SHARE_MIN = 512, 1280, 24
RATIO_CHUNK = 8                          # kTabRatioChunk
SCRATCH_TAIL = 64                        # sentinel words behind the partial minima of T7 / T8
ENTERING_LIST_MAX, LEAVING_LIST_MAX = 32, 64     # select_entering / block_minima_pick: listed slots before every slot is walked


def _u8(a): return np.ascontiguousarray(a, dtype=np.uint8)


def _outs(L, lengths, dt):
    L = dict(L)
    L.update(lengths or {})
    return {k: np.zeros(v, dtype=dt.get(k, np.float64)) for k, v in L.items()}


def tab_splits(which, size, count, forced=0, lengths=None):
    """tab_rhs_splits (which = 0, size = m) / tab_cost_splits (which = 1, size = stored columns); no HIP call."""
    out = np.zeros((lengths or {}).get("out", 1), dtype=np.int32)
    _call("rkh_tab_splits", [_n(which), _w(size), _w(count), _w(forced)], [out])
    return int(out[0])


def tab_rhs_change(T0, W, R0, b, cols, delta, kmax, splits=1, c_lo=0, batch=8, fill=True, lengths=None):
    """launch_tab_rhs_change.  cols: storage columns.  Whole images back."""
    T0, W, R0 = _f64(T0), _f64(W), _f64(R0)
    n, m = T0.shape
    p = W.shape[0]
    cols, delta = _i32(cols), _f64(delta)
    count = cols.size
    out = _outs(dict(b=ld_b(m), v=kmax, partial=max(splits, 0) * ld_b(m), T0=n * ld_t(m), W=kmax * ld_b(m), R0=(kmax + 1) * ld_r(n),
                     cols=count, delta=count), lengths, dict(cols=np.int32))
    _call("rkh_tab_rhs_change", [_w(m), _w(n), _w(p), _w(kmax), _w(c_lo), _n(batch), _w(count), _w(splits), _n(fill)],
          [T0, W, R0, _f64(b), cols, delta] + [out[k] for k in ("b", "v", "partial", "T0", "W", "R0", "cols", "delta")])
    return out


def tab_cost_change(T0, W, R0, d, in_basis, rows, delta, ncols, ndelta, kmax, splits=1, c_lo=0, col_off=0, batch=8, fill=True,
                    lengths=None):
    """launch_tab_cost_change.  d: the owned columns; in_basis: c_lo + n_owned - col_off flags by tableau column; ncols: storage
    columns."""
    T0, W, R0 = _f64(T0), _f64(W), _f64(R0)
    n, m = T0.shape
    p = W.shape[0]
    rows, delta, ncols, ndelta, in_basis = _i32(rows), _f64(delta), _i32(ncols), _f64(ndelta), _u8(in_basis)
    out = _outs(dict(d=c_lo + n, u=kmax, partial=max(splits, 0) * ld_r(n), in_basis=max(c_lo + n - col_off, 0), T0=n * ld_t(m),
                     W=kmax * ld_b(m), R0=(kmax + 1) * ld_r(n), rows=rows.size, delta=rows.size, ncols=ncols.size, ndelta=ncols.size),
                lengths, dict(in_basis=np.uint8, rows=np.int32, ncols=np.int32))
    _call("rkh_tab_cost_change",
          [_w(m), _w(n), _w(p), _w(kmax), _w(c_lo), _w(col_off), _n(batch), _w(rows.size), _w(ncols.size), _w(splits), _n(fill)],
          [T0, W, R0, _f64(d), in_basis, rows, delta, ncols, ndelta] +
          [out[k] for k in ("d", "u", "partial", "in_basis", "T0", "W", "R0", "rows", "delta", "ncols", "ndelta")])
    return out


def tab_row_ratios(T0, W, R0, d, in_basis, rows, tol, kmax, c_lo=0, col_off=0, batch=8, fill=True, lengths=None):
    """launch_tab_row_ratios.  tol = (pivot, zero, tie).  ratio / column: [direction][list entry]."""
    T0, W, R0 = _f64(T0), _f64(W), _f64(R0)
    n, m = T0.shape
    p = W.shape[0]
    rows, in_basis = _i32(rows), _u8(in_basis)
    count = rows.size
    scratch = 2 * count * scan_blocks(n) + SCRATCH_TAIL
    out = _outs(dict(ratio=2 * count, column=2 * count, part_k=scratch, part_j=scratch, d=c_lo + n, in_basis=max(c_lo + n - col_off, 0),
                     T0=n * ld_t(m), W=kmax * ld_b(m), R0=(kmax + 1) * ld_r(n), rows=count), lengths,
                dict(column=np.int32, part_j=np.int32, in_basis=np.uint8, rows=np.int32))
    _call("rkh_tab_row_ratios", [_w(m), _w(n), _w(p), _w(kmax), _w(c_lo), _w(col_off), _n(batch), _w(count), _n(fill)],
          [_f64(tol), T0, W, R0, _f64(d), in_basis, rows] +
          [out[k] for k in ("ratio", "column", "part_k", "part_j", "d", "in_basis", "T0", "W", "R0", "rows")])
    return out


def tab_rhs_ranging(T0, W, R0, b, basis, cols, tol, kmax, c_lo=0, batch=8, fill=True, lengths=None):
    """launch_tab_rhs_ranging.  cols: storage columns.  ratio / row: [direction][list entry]."""
    T0, W, R0 = _f64(T0), _f64(W), _f64(R0)
    n, m = T0.shape
    p = W.shape[0]
    cols, basis = _i32(cols), _i32(basis)
    count = cols.size
    scratch = 2 * count * scan_blocks(m) + SCRATCH_TAIL
    out = _outs(dict(ratio=2 * count, row=2 * count, part=scratch, b=ld_b(m), basis=m, T0=n * ld_t(m), W=kmax * ld_b(m),
                     R0=(kmax + 1) * ld_r(n), cols=count), lengths, dict(row=np.int32, basis=np.int32, cols=np.int32))
    _call("rkh_tab_rhs_ranging", [_w(m), _w(n), _w(p), _w(kmax), _w(c_lo), _n(batch), _w(count), _n(fill)],
          [_f64(tol), T0, W, R0, _f64(b), basis, cols] +
          [out[k] for k in ("ratio", "row", "part", "b", "basis", "T0", "W", "R0", "cols")])
    return out


# ---- models of the sums --------------------------------------------------------------------------------------------------
def model_splits(which, size, count, forced=0):
    """tab_rhs_splits / tab_cost_splits as relp_kernels.h states the rule."""
    if count < 1:
        return 1
    if forced >= 1:
        return min(forced, count, MAX_SPLITS)
    blocks = scan_blocks(size)
    if which == 0:
        return max(1, min(RHS_GRID // blocks, count // 256, MAX_SPLITS))
    return max(1, min(COST_GRID // blocks, count // COST_SHARE_MIN, MAX_SPLITS))


def share_bounds(count, splits):
    """[lo, hi) of every split: equal shares of ceil(count / splits) entries, the last ones short or empty."""
    share = (count + splits - 1) // splits
    return [(min(s * share, count), min(min(s * share, count) + share, count)) for s in range(splits)]


def model_pending(delta, X, order="tree"):
    """sum_k delta[k] X[j][k] for every row j of X (p x count) as k_tab_rhs_pending / k_tab_cost_pending form it: thread t's fma
    chain over k = t, t + 256, ... from 0.0, then the tree s[t] += s[t + half], half = 128 .. 1.  order = "plain": the 256 thread
    sums added left to right instead (what the tree is NOT; the CPU tier uses it)."""
    X = np.asarray(X, dtype=np.float64)
    p, count = X.shape
    trips = (count + 255) // 256
    s = np.zeros((p, 256))
    for trip in range(trips):
        k = np.arange(trip * 256, min((trip + 1) * 256, count))
        s[:, :k.size] = fma_vec(delta[k][None, :], X[:, k], s[:, :k.size])
    if order == "plain":
        acc = s[:, 0].copy()
        for t in range(1, 256):
            acc = acc + s[:, t]
        return acc
    half = 128
    while half:
        s[:, :half] = s[:, :half] + s[:, half:2 * half]
        half //= 2
    return s[:, 0].copy()


def model_shares(term, delta, count, splits, width):
    """parts[s] = the fma chain from 0.0 over the share of split s, term(k) = the vector entry k multiplies."""
    parts = np.zeros((splits, width))
    for s, (lo, hi) in enumerate(share_bounds(count, splits)):
        acc = np.zeros(width)
        for k in range(lo, hi):
            acc = fma_vec(delta[k], term(k), acc)
        parts[s] = acc
    return parts


def sum_in_split_order(parts):
    total = parts[0].copy()
    for s in range(1, parts.shape[0]):
        total = total + parts[s]
    return total


def rhs_change_expected(T0, W, R0, b, cols, delta, kmax, splits=1, c_lo=0, swap_shares=None):
    """Every image launch_tab_rhs_change must leave, by the comments of k_tab_rhs_pending / _apply / _reduce.
    swap_shares = (s, t): the partials of splits s and t added in swapped places (a wrong order, for the CPU tier)."""
    T0, W, R0, b, delta = (np.asarray(x, dtype=np.float64) for x in (T0, W, R0, b, delta))
    n, m = T0.shape
    p = W.shape[0]
    cl = np.asarray(cols, dtype=np.int64) - c_lo
    count = cl.size
    v = model_pending(delta, R0[:, cl]) if p else np.zeros(0)
    parts = model_shares(lambda k: T0[cl[k]], delta, count, splits, m)
    for j in range(p):
        parts[0] = fma_vec(W[j], v[j], parts[0])
    order = list(range(splits))
    if swap_shares:
        s, t = swap_shares
        order[s], order[t] = order[t], order[s]
    bn = b + (parts[0] if splits == 1 else sum_in_split_order(parts[order]))
    partial = np.full((max(splits, 1), ld_b(m)), SENTINEL)
    if splits > 1:
        partial[:, :m] = parts
    t_up, w_up, r_up = tab_images(None, m, n, p, kmax, T0, W, R0)
    return dict(b=vec_image(bn, m, ld_b(m)), v=vec_image(v, p, kmax), partial=partial.reshape(-1)[:splits * ld_b(m)], T0=t_up.reshape(-1),
                W=w_up.reshape(-1), R0=r_up.reshape(-1), cols=np.asarray(cols, dtype=np.int32), delta=delta.copy(), parts=parts)


def cost_moves(n, c_lo, col_off, in_basis):
    """The owned columns launch_tab_cost_change moves (cost_moves_column): all but those flagged 1 by TABLEAU column c - col_off."""
    c = c_lo + np.arange(n)
    j = c - col_off
    flags = np.asarray(in_basis)
    inside = (j >= 0) & (j < flags.size)
    basic = np.zeros(n, dtype=bool)
    basic[inside] = flags[j[inside]] == 1
    return ~basic


def cost_change_expected(T0, W, R0, d, in_basis, rows, delta, ncols, ndelta, kmax, splits=1, c_lo=0, col_off=0, swap_shares=None):
    """Every image launch_tab_cost_change must leave, by the comments of k_tab_cost_pending / _apply / _reduce."""
    T0, W, R0, d, delta, ndelta = (np.asarray(x, dtype=np.float64) for x in (T0, W, R0, d, delta, ndelta))
    n, m = T0.shape
    p_img = W.shape[0]
    rows = np.asarray(rows, dtype=np.int64)
    ncl = np.asarray(ncols, dtype=np.int64) - c_lo
    count = rows.size
    p = p_img if count else 0                              # only direct terms: the launcher forces p = 0 and splits = 1
    assert count or splits == 1
    u = model_pending(delta, W[:, rows]) if p else np.zeros(0)
    parts = model_shares(lambda k: T0[:, rows[k]], delta, count, splits, n)
    for j in range(p):
        parts[0] = fma_vec(u[j], R0[j], parts[0])
    parts[0][ncl] = parts[0][ncl] - ndelta
    order = list(range(splits))
    if swap_shares:
        s, t = swap_shares
        order[s], order[t] = order[t], order[s]
    moves = cost_moves(n, c_lo, col_off, in_basis)
    total = parts[0] if splits == 1 else sum_in_split_order(parts[order])
    dn = np.full(c_lo + n, SENTINEL)
    dn[c_lo:] = np.where(moves, d - total, d)
    keep = bits(d)[~moves]
    dn_bits = bits(dn).copy()
    dn_bits[c_lo:][~moves] = keep                          # a column flagged 1 keeps its d to the bit (np.where keeps NaN payloads, this is explicit)
    partial = np.full((max(splits, 1), ld_r(n)), SENTINEL)
    if splits > 1:
        partial[:, :n][:, moves] = parts[:, moves]
    t_up, w_up, r_up = tab_images(None, m, n, p_img, kmax, T0, W, R0)
    return dict(d=dn_bits.view(np.float64), u=vec_image(u, p, kmax), partial=partial.reshape(-1)[:splits * ld_r(n)],
                in_basis=np.asarray(in_basis, dtype=np.uint8).copy(), T0=t_up.reshape(-1), W=w_up.reshape(-1), R0=r_up.reshape(-1),
                rows=rows.astype(np.int32), delta=delta.copy(), ncols=np.asarray(ncols, dtype=np.int32), ndelta=ndelta.copy(),
                parts=parts, moves=moves)


def diff_image(got, want, what, limit=5):
    """A whole returned image against the expected one, bit for bit: where `want` holds the sentinel the word must still hold it,
    elsewhere the bits are equal and no NaN has appeared."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return [f"{what}: shape {got.shape} != {want.shape}"]
    if got.dtype.kind != "f":
        return diff_unchanged(got, want, what, limit)
    bg, bw = bits(got).reshape(got.shape), bits(want).reshape(want.shape)
    bad = (bg != bw) | (np.isnan(got) & (bw != SENTINEL_BITS))
    idx = np.argwhere(bad)
    return [f"{what}{tuple(i)}: got {got[tuple(i)]!r} ({bg[tuple(i)]:#x}), want {want[tuple(i)]!r} ({bw[tuple(i)]:#x})"
            for i in idx[:limit]] + ([f"{what}: {len(idx)} words differ"] if len(idx) > limit else [])


def image_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def diff_images(got, want, limit=5):
    """Every returned image (a dict) against the expected one, bit for bit (the sentinels included: what the launch must not
    write)."""
    problems = []
    for name in want:
        g, w = image_bits(got[name]), image_bits(want[name])
        if g.shape != w.shape:
            problems.append(f"{name}: {g.shape} words returned, {w.shape} expected")
            continue
        bad = np.flatnonzero(g != w)
        if bad.size:
            shown = ", ".join(f"[{int(x)}] {got[name].reshape(-1)[x]!r} != {want[name].reshape(-1)[x]!r}" for x in bad[:limit])
            problems.append(f"{name}: {bad.size} words differ: {shown}")
    return problems


RHS_IMAGES = ("b", "v", "partial", "T0", "W", "R0", "cols", "delta")
COST_IMAGES = ("d", "u", "partial", "in_basis", "T0", "W", "R0", "rows", "delta", "ncols", "ndelta")


def compare_images(out, exp, names):
    return [f for k in names for f in diff_image(out[k], exp[k], k)]


# ---- exact values (integers and rationals) -----------------------------------------------------------------------------------
def rhs_change_int(T0, W, R0, b, cols, delta, c_lo=0):
    """b + T0' delta + W' (R0 delta) in int64 for integer-valued operands: every order of summation gives this float64."""
    Ti, Wi, Ri, bi, di = (np.asarray(x).astype(np.int64) for x in (T0, W, R0, b, delta))
    assert all((a == x).all() for a, x in ((Ti, T0), (Wi, W), (Ri, R0), (bi, b), (di, delta))), "integer data expected"
    cl = np.asarray(cols, dtype=np.int64) - c_lo
    out = bi + di @ Ti[cl] + (Ri[:, cl] @ di) @ Wi
    assert np.abs(out).max() < 2 ** 52
    return out.astype(np.float64)


def cost_change_int(T0, W, R0, d, rows, delta, ncols, ndelta, moves, c_lo=0):
    Ti, Wi, Ri, di, ni = (np.asarray(x).astype(np.int64) for x in (T0, W, R0, delta, ndelta))
    dd = np.asarray(d, dtype=np.float64)                   # (integer-valued where a column moves; anything where it is pinned)
    rows = np.asarray(rows, dtype=np.int64)
    acc = Ti[:, rows] @ di + ((Wi[:, rows] @ di) @ Ri if rows.size else 0)
    acc[np.asarray(ncols, dtype=np.int64) - c_lo] -= ni
    assert np.abs(acc).max() < 2 ** 52
    with np.errstate(all="ignore"):
        return np.where(moves, dd - acc, dd)


_SCALE = 60


def _ints(a):
    """float64 array -> Python ints of a * 2^60 (exact: asserted)."""
    y = np.asarray(a, dtype=np.float64) * 2.0 ** _SCALE
    assert np.all(np.floor(y) == y) and np.all(np.abs(y) < 2.0 ** 1000), "data finer than 2^-60"
    return [int(v) for v in y.reshape(-1).tolist()]


def gamma(N):
    """gamma_N = N u / (1 - N u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1)."""
    return Fraction(N) * Fraction(EPS53) / (1 - Fraction(N) * Fraction(EPS53))


def sum_roundings(count, splits, p):
    """Roundings on the longest path from an input to the output: share length + ceil(count / 256) + 8 tree levels + p + splits + 1."""
    return (count + splits - 1) // max(splits, 1) + (count + 255) // 256 + 8 + p + splits + 1


def exact_check(got, base, A, delta, U, X, N, sample, sign=1, extra=None):
    """got[e] against base[e] + sign * (sum_k delta[k] A[k][e] + sum_j U[j][e] sum_k delta[k] X[j][k]) as exact rationals
    (fractions.Fraction over integers scaled by powers of two), bound gamma_N * S, S = the sum of the absolute values of all terms,
    |base[e]| included; extra[e] (a direct term) is added as it stands.  A: count x width, U: p x width, X: p x count.  Returns (violations, largest error / (2^-53 S))."""
    count, p = len(delta), U.shape[0]
    di = _ints(delta)
    xi = [_ints(X[j]) for j in range(p)]
    vj = [sum(a * b for a, b in zip(di, xi[j])) for j in range(p)]                     # scale 2^120
    vabs = [sum(abs(a * b) for a, b in zip(di, xi[j])) for j in range(p)]
    bad, worst = [], 0.0
    one = 1 << _SCALE
    for e in sample:
        ai = _ints(A[:, e]) if count else []
        ui = _ints(U[:, e]) if p else []
        bi = _ints(base[e:e + 1])[0]
        xe = _ints(extra[e:e + 1])[0] if extra is not None else 0
        t1 = sum(a * b for a, b in zip(di, ai))                                          # scale 2^120
        s1 = sum(abs(a * b) for a, b in zip(di, ai))
        t2 = sum(a * b for a, b in zip(ui, vj))                                          # scale 2^180
        s2 = sum(abs(a) * b for a, b in zip(ui, vabs))
        exact = Fraction(bi + xe, one) + sign * (Fraction(t1, one ** 2) + Fraction(t2, one ** 3))
        S = Fraction(abs(bi) + abs(xe), one) + Fraction(s1, one ** 2) + Fraction(s2, one ** 3)
        g = float(got[e])
        if not np.isfinite(g):
            bad.append((e, g, "not finite"))
            continue
        err = abs(Fraction(g) - exact)
        if S > 0:
            worst = max(worst, float(err / (Fraction(EPS53) * S)))
        if err > gamma(N) * S:
            bad.append((e, g, float(exact)))
    return bad, worst


# ---- models of the ratio queries ---------------------------------------------------------------------------------------------
def band_bounds(k1, tie):
    """k1 + tie * max(1, |k1|) with two roundings and as one fma: the compiler may contract the expression."""
    s = max(1.0, abs(float(k1)))
    return float(k1) + float(tie) * s, fma_exact(tie, s, k1)


def model_rows_of_T(T0, W, R0, rows):
    """E[k][c] = T[rows[k], c]: T0, then one fma per pending row in ascending j (tab_row_entry)."""
    rows = np.asarray(rows, dtype=np.int64)
    E = np.array(T0[:, rows].T, dtype=np.float64)
    for j in range(W.shape[0]):
        E = fma_vec(W[j, rows][:, None], R0[j][None, :], E)
    return E


def model_columns_of_T(T0, W, R0, cl):
    """A[k][i] = T[i, cl[k]]: T0, then one fma per pending row in ascending j (tab_column_entry)."""
    cl = np.asarray(cl, dtype=np.int64)
    A = np.array(T0[cl], dtype=np.float64)
    for j in range(W.shape[0]):
        A = fma_vec(W[j][None, :], R0[j, cl][:, None], A)
    return A


def _pick_lowest(ratio, key, bound):
    inside = ratio <= bound
    return int(key[inside].min())


def model_row_ratios(T0, W, R0, d, in_basis, rows, tol, c_lo=0, col_off=0):
    """launch_tab_row_ratios.  Returns ratio, column (2 x count, [direction][entry], the pick with the two-rounding bound),
    column_fma (the pick with the contracted bound) and between (candidates whose ratio lies between the two bounds)."""
    T0, W, R0, d = (np.asarray(x, dtype=np.float64) for x in (T0, W, R0, d))
    n = T0.shape[0]
    flags = np.asarray(in_basis)
    tol_pivot, tol_zero, tol_tie = (float(t) for t in tol)
    j = c_lo + np.arange(n) - col_off
    inside = (j >= 0) & (j < flags.size)
    nonbasic = np.zeros(n, dtype=bool)
    nonbasic[inside] = flags[j[inside]] == 0
    E = model_rows_of_T(T0, W, R0, rows)
    count = E.shape[0]
    dz = np.where(d <= tol_zero, 0.0, d)
    ratio = np.full((2, count), np.inf)
    column = np.full((2, count), -1, dtype=np.int32)
    column_fma = column.copy()
    between = np.zeros((2, count), dtype=np.int64)
    for direction in range(2):
        V = -E if direction else E
        for k in range(count):
            cand = nonbasic & (V[k] < -tol_pivot)
            if not cand.any():
                continue
            with np.errstate(all="ignore"):
                r = dz[cand] / (-V[k][cand])
            k1 = r.min()
            b2, b1 = band_bounds(k1, tol_tie)
            ratio[direction, k] = k1
            column[direction, k] = _pick_lowest(r, j[cand], b2)
            column_fma[direction, k] = _pick_lowest(r, j[cand], b1)
            between[direction, k] = int(((r > min(b1, b2)) & (r <= max(b1, b2))).sum())
    return dict(ratio=ratio.reshape(-1), column=column.reshape(-1), column_fma=column_fma.reshape(-1), between=between.reshape(-1), E=E)


def model_rhs_ranging(T0, W, R0, b, basis, cols, tol, c_lo=0, signed_keys=False):
    """launch_tab_rhs_ranging.  As model_row_ratios; the pick is the row inside the band with the smallest basis entry as an
    UNSIGNED 32-bit value (signed_keys: the wrong comparison, for the CPU tier)."""
    T0, W, R0, b = (np.asarray(x, dtype=np.float64) for x in (T0, W, R0, b))
    m = T0.shape[1]
    tol_pivot, tol_zero, tol_tie = (float(t) for t in tol)
    key = np.asarray(basis, dtype=np.int32).astype(np.int64)
    if not signed_keys:
        key = key & 0xFFFFFFFF
    A = model_columns_of_T(T0, W, R0, np.asarray(cols, dtype=np.int64) - c_lo)
    count = A.shape[0]
    bz = np.where(b <= tol_zero, 0.0, b)
    ratio = np.full((2, count), np.inf)
    row = np.full((2, count), -1, dtype=np.int32)
    row_fma = row.copy()
    between = np.zeros((2, count), dtype=np.int64)
    idx = np.arange(m)
    for direction in range(2):
        V = -A if direction else A
        for k in range(count):
            q = V[k] > tol_pivot
            if not q.any():
                continue
            with np.errstate(all="ignore"):
                r = bz[q] / V[k][q]
            gmin = r.min()
            b2, b1 = band_bounds(gmin, tol_tie)
            ratio[direction, k] = gmin
            for bound, dst in ((b2, row), (b1, row_fma)):
                ins = r <= bound
                dst[direction, k] = int(idx[q][ins][np.argmin(key[q][ins])])
            between[direction, k] = int(((r > min(b1, b2)) & (r <= max(b1, b2))).sum())
    return dict(ratio=ratio.reshape(-1), row=row.reshape(-1), row_fma=row_fma.reshape(-1), between=between.reshape(-1), A=A)


def compare_row_ratios(out, exp, before):
    """`before`: dict of the uploaded images (d, in_basis, T0, W, R0, rows) the launcher must leave alone."""
    nscr = out["part_k"].size - SCRATCH_TAIL
    return (diff_bits(out["ratio"], exp["ratio"], "ratio") + diff_values(out["column"], exp["column"], "column") +
            sentinel_violations(out["part_k"][nscr:], "part_k tail") + sentinel_violations(out["part_j"][nscr:], "part_j tail") +
            [f for k in ("d", "in_basis", "T0", "W", "R0", "rows") for f in diff_unchanged(out[k], before[k], k)])


def compare_rhs_ranging(out, exp, before):
    nscr = out["part"].size - SCRATCH_TAIL
    return (diff_bits(out["ratio"], exp["ratio"], "ratio") + diff_values(out["row"], exp["row"], "row") +
            sentinel_violations(out["part"][nscr:], "part tail") +
            [f for k in ("b", "basis", "T0", "W", "R0", "cols") for f in diff_unchanged(out[k], before[k], k)])


def query_images(T0, W, R0, kmax, c_lo=0, d=None, b=None):
    """What the harness uploads for a read-only query (flat images)."""
    n, m = T0.shape
    t, w, r = tab_images(None, m, n, W.shape[0], kmax, T0, W, R0)
    img = dict(T0=t.reshape(-1), W=w.reshape(-1), R0=r.reshape(-1))
    if d is not None:
        img["d"] = np.full(c_lo + n, SENTINEL)
        img["d"][c_lo:] = d
    if b is not None:
        img["b"] = vec_image(b, m, ld_b(m))
    return img
