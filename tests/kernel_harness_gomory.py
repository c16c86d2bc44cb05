"""Helper module of the kernel tests of the Gomory cuts (not collected by pytest): the calls of
tests/kernels/harness_gomory.cpp (through tests/kernel_harness.py), the cases of launch_tab_gomory, the f64 model in the order relp_kernels.h states
(tests/gomory_reference.py: pi_f64, structural_f64 over kernel_harness.model_rows_of_T / model_pending(order="tree")) and the same
over Fractions.

Layouts.  Logical arrays are C-ordered as in kernel_harness: T0[c][i] (n_owned x m), W[j][i] (p x m), R0[j][c] (p x n_owned),
A[sp][i] (structural column sp, rows of A: the constraints, then the cut rows).  Stored column c = c_lo + index; tableau column
j = c - col_off; structural sp = j < nr_normal; virtual v = j - nr_normal.  `Case.images()` lays them into whole device images with the
case's pitches and the sentinels of kernel_harness everywhere else and behind every output."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import gomory_reference as gr
import kernel_harness as kh

TAIL = 64                                # sentinel words behind every output
TOL_ZERO = 1e-11


class Case:
    """m rows; `art` kept artificial columns in front (owned: c_lo <= col_off = c_lo + art), nn structural columns, nv virtual
    columns (the slack of the rows `slack_rows`, signs alternating from `first_sign`), so n_owned = art + nn + nv.  A has mc
    constraint rows and `cuts` cut rows, the tableau rows m - cuts ..; `y_rows` of the rows of A get a non-basic slack with a
    fractional entry, every other slack of a row of A is basic (pi exactly 0.0).  rows / f0: the list (f0 < 0: skipped)."""

    def __init__(self, m, nn, rows, p, *, kmax=None, art=0, c_lo=0, mc=None, cuts=0, y_rows=None, kind=0, batch=8, flags=None, seed=0,
                 bound_rows=(), basic=(), barred=(), special=True, f0=None, tol_zero=TOL_ZERO):
        rng = np.random.default_rng(seed)
        self.m, self.nn, self.p, self.kind, self.batch, self.tol_zero = m, nn, p, kind, batch, tol_zero
        self.kmax = kmax if kmax is not None else max(p, 1)
        self.c_lo, self.art, self.col_off = c_lo, art, c_lo + art
        self.cuts = cuts
        self.mc = m - cuts - len(bound_rows) if mc is None else mc
        self.cut_row0 = m - cuts
        self.n_a = self.mc + cuts
        a_rows = np.concatenate([np.arange(self.mc), self.cut_row0 + np.arange(cuts)]).astype(np.int64)
        self.a_rows = a_rows
        # the virtual columns: one per row of A and per bound row (an equality row would have none: the first row of A when mc > 2)
        slack_rows = [int(r) for r in a_rows if not (self.mc > 2 and r == 0)]
        self.bound_row = np.full(nn, -1, dtype=np.int32)
        for k, (c, r) in enumerate(bound_rows):
            self.bound_row[c] = r
            slack_rows.append(r)
        self.vrow0 = np.array(slack_rows, dtype=np.int32)
        self.nv = len(slack_rows)
        self.vsign = np.where(np.arange(self.nv) % 2 == 0, 1, -1).astype(np.int32)
        self.n_owned = art + nn + self.nv
        self.n_tab = nn + self.nv
        self.rows = np.asarray(rows, dtype=np.int32)
        self.count = self.rows.size
        T0 = kh.real_data(rng, (self.n_owned, m), zeros=0.1, neg_zeros=0.05)
        self.W = kh.real_data(rng, (p, m), zeros=0.1, neg_zeros=0.05)
        self.R0 = kh.real_data(rng, (p, self.n_owned), zeros=0.1, neg_zeros=0.05)
        self.f0 = np.asarray(f0, dtype=np.float64) if f0 is not None else np.where(np.arange(self.count) % 5 == 4, -1.0, 0.25 + 0.0625 * (np.arange(self.count) % 7))
        self.flags = np.zeros(self.n_tab, dtype=np.uint8)
        for j in basic:
            self.flags[j] = 1
        for j in barred:
            self.flags[j] = 2
        # the slacks of the rows of A outside y_rows are basic: y is exactly 0.0 there
        if y_rows is not None:
            keep = set(int(a_rows[i]) for i in y_rows)
            for v, r in enumerate(slack_rows):
                if r in set(a_rows.tolist()) and r not in keep:
                    self.flags[nn + v] = 1
        self.is_integer = None if flags is None else np.asarray(flags(self.n_tab), dtype=np.uint8)
        if special and p == 0 and self.count:
            # entries the rule treats specially, in the first list entry's row (p = 0: the entry is T0 itself)
            r, f = int(self.rows[0]), float(self.f0[0]) if self.f0[0] >= 0 else 0.25
            values = [0.0, -0.0, 3.0, -2.0, 5.0 + f, -4.0 + f, 2.0 + 0.5 * tol_zero, 2.0 - 0.5 * tol_zero, 0.5 * tol_zero, -0.5 * tol_zero,
                      1.0 + 4 * tol_zero, 1.0 - 4 * tol_zero, 0.75, -0.75]
            for k, v in enumerate(values):
                if art + k < self.n_owned:
                    T0[art + k, r] = v
        self.T0 = T0
        self.A = kh.real_data(rng, (nn, self.n_a), zeros=0.1, neg_zeros=0.05)
        self.ld_t, self.ld_b, self.ld_r = kh.ld_t(m) + 2, kh.ld_b(m), kh.ld_r(self.n_owned) + 2
        self.ld_a = kh.round_up(self.n_a + 3, 2)
        self.nbc = kh.scan_blocks(self.n_owned)

    # -- the model --
    def cand(self):
        j = np.arange(self.n_owned) - self.art
        out = np.zeros(self.n_owned, dtype=bool)
        inside = j >= 0
        out[inside] = self.flags[j[inside]] != 1
        return out

    def integer(self):
        out = np.ones(self.n_owned, dtype=bool)
        if self.is_integer is not None:
            out[self.art:] = self.is_integer != 0
        return out

    def entries(self):
        return kh.model_rows_of_T(self.T0, self.W, self.R0, self.rows)

    def y_of(self, pi):
        y = np.zeros((self.count, self.m))
        for v in range(self.nv):
            if self.vrow0[v] >= 0:
                y[:, self.vrow0[v]] = self.vsign[v] * pi[:, self.art + self.nn + v]
        return y

    def expected(self):
        """(pi, y, bad, g) of the f64 model."""
        E = self.entries()
        pi, badc = gr.pi_f64(E, self.f0, self.cand(), self.integer(), self.kind, self.tol_zero)
        y = self.y_of(pi)
        bad = np.zeros((self.count, self.nbc))
        for blk in range(self.nbc):
            bad[:, blk] = badc[:, blk * 256:(blk + 1) * 256].any(axis=1)
        g = gr.structural_f64(pi[:, self.art:self.art + self.nn], y, self.A.T, self.a_rows, self.bound_row)
        return pi, y, bad, g

    def exact_violations(self, pi, y, g):
        """pi against the rule over Fractions on the f64 entry (gamma(4): the rule rounds at most four times) and g against the
        Fraction sum of the f64 pi and y (gamma(N) S, N = ceil(rows of A / 256) + 8 tree levels + 2).  Returns the problems."""
        E = self.entries()
        cand, integer = self.cand(), self.integer()
        problems = []
        tol = Fraction(self.tol_zero)
        for k in range(self.count):
            if self.f0[k] < 0:
                continue
            for c in range(self.n_owned):
                if not cand[c] or not math.isfinite(E[k, c]):
                    continue
                a, f0 = Fraction(float(E[k, c])), Fraction(float(self.f0[k]))
                exact, _ = gr.pi_of(a, f0, bool(integer[c]), self.kind, tol)
                S = abs(exact)
                if integer[c] and abs(a) > tol:                  # one rounding of 1 - tol_zero decides the upper band in f64
                    f = a - math.floor(a)
                    if abs(f - (1 - tol)) <= Fraction(2.0 ** -52):
                        continue
                    if self.kind == gr.MIXED and f > f0:         # 1 - f cancels: the rounding of f (at most u, f < 1) is carried
                        S += f0 / (1 - f0)                       # into pi by the slope f0 / (1 - f0)
                if abs(Fraction(float(pi[k, c])) - exact) > kh.gamma(4) * S:
                    problems.append(f"pi[{k}][{c}] = {pi[k, c]!r}, exact {float(exact)!r}")
        N = (self.n_a + 255) // 256 + 8 + 2
        for k in range(self.count):
            for sp in range(self.nn):
                terms = [Fraction(float(y[k, self.a_rows[i]])) * Fraction(float(self.A[sp, i])) for i in range(self.n_a)]
                terms.append(-Fraction(float(pi[k, self.art + sp])))
                if self.bound_row[sp] >= 0:
                    terms.append(Fraction(float(y[k, self.bound_row[sp]])))
                exact, S = sum(terms), sum(abs(t) for t in terms)
                if abs(Fraction(float(g[k, sp])) - exact) > kh.gamma(N) * S:
                    problems.append(f"g[{k}][{sp}] = {g[k, sp]!r}, exact {float(exact)!r}")
        return problems

    # -- images --
    def images(self):
        m, n, kmax, p = self.m, self.n_owned, self.kmax, self.p
        f = lambda size: np.full(size, kh.SENTINEL)   # noqa: E731
        T0 = f((n, self.ld_t)); T0[:, :m] = self.T0
        W = f((kmax, self.ld_b)); W[:p, :m] = self.W
        R0 = f((kmax + 1, self.ld_r)); R0[:p, :n] = self.R0
        A = f((max(self.nn, 1), self.ld_a)); A[:self.nn, :self.n_a] = self.A
        return dict(T0=T0.reshape(-1), W=W.reshape(-1), R0=R0.reshape(-1), in_basis=self.flags.copy(),
                    is_integer=(self.is_integer.copy() if self.is_integer is not None else np.zeros(1, dtype=np.uint8)),
                    vrow0=self.vrow0.copy(), vsign=self.vsign.copy(), bound_row=self.bound_row.copy(), A=A.reshape(-1), rows=self.rows.copy(),
                    f0=self.f0.copy(), pi=f(self.count * n + TAIL), y=f(self.count * m + TAIL), bad=f(self.count * self.nbc + TAIL),
                    g=f(self.count * self.nn + TAIL))

    def launch(self):
        """The images after rkg_tab_gomory."""
        assert kh.load().rkg_chunk() == kh.RATIO_CHUNK
        img = self.images()
        scalars = [self.m, self.n_owned, self.c_lo, self.col_off, self.p, self.kmax, self.batch, self.count, self.kind, self.ld_t, self.ld_b,
                   self.ld_r, self.ld_a, self.mc, self.cuts, self.cut_row0, self.nn, self.nv, 0 if self.is_integer is None else 1]
        names = ("T0", "W", "R0", "in_basis", "is_integer", "vrow0", "vsign", "bound_row", "A", "rows", "f0", "pi", "y", "bad",
                 "g")
        kh._call("rkg_tab_gomory", scalars, {name: img[name] for name in names}, reals=[self.tol_zero])
        return img

    def compare(self, img):
        """Every output against the f64 model bit for bit, the sentinels behind it, and every input image unchanged."""
        pi, y, bad, g = self.expected()
        before = self.images()
        problems = []
        for name, want in (("pi", pi), ("y", y), ("bad", bad), ("g", g)):
            got = img[name]
            problems += kh.diff_bits(got[:want.size], want.reshape(-1), name)
            problems += kh.sentinel_violations(got[want.size:], name + " tail")
        for name in ("T0", "W", "R0", "in_basis", "is_integer", "vrow0", "vsign", "bound_row", "A", "rows", "f0"):
            problems += kh.diff_unchanged(img[name], before[name], name)
        return problems
