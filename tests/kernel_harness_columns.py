"""Helper module of the kernel tests of the columns added in place (not collected by pytest): the calls of
tests/kernels/harness_columns.cpp (through tests/kernel_harness.py), the reference model of launch_tab_add_columns in the summation order relp_kernels.h
states, and the construction of the device images a case starts from and must end with.

Reference arithmetic: `kernel_harness.fma_vec` (held to `fma_exact`, the Fraction fma, by tests/test_kernel_models.py) over vectors,
`chain_exact` for single entries.  The order of launch_tab_add_columns:
  T0[new k][i]  from 0.0: fma(coef[e][k], T0[cols[e]][i], acc) over e ascending (the list is not cut into shares)
  R0[j][new k]  the entry T0[new k][S[j]] just written for j < p, 0.0 for the other rows of R0 (the scratch row included)
  d, cost, flag the caller's d_new and cost_new, flag 0; descriptors vrow0 = vrow1 = -1, vsign = 1
W is not read: T = (I + W S') T0 is linear in T0.

Layouts.  Logical arrays are C-ordered as in kernel_harness: T0[c][i] (n_owned x m), R0[j][c] (p x n_owned), coef[e][k].
`Case.images()` lays them into whole device images with the case's pitches and the sentinels of kernel_harness everywhere else;
`Case.expected()` is every image after the launch."""
from __future__ import annotations

import numpy as np

import kernel_harness as kh

COL_TILE = 8
image_bits, diff_images = kh.image_bits, kh.diff_images


# ------------------------------------------------------------------------------------------------------------------------
# the model (logical arrays in, logical arrays out)
# ------------------------------------------------------------------------------------------------------------------------
def model_new_columns(T0, cols, coef, c_lo=0):
    """new[k][i]: the stored columns launch_tab_add_columns writes into T0 (count x m).  cols: storage columns."""
    T0, coef = np.asarray(T0, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    count = coef.shape[1]
    new = np.zeros((count, T0.shape[1]))
    for k in range(count):
        acc = np.zeros(T0.shape[1])
        for e in range(len(cols)):
            acc = kh.fma_vec(coef[e, k], T0[int(cols[e]) - c_lo], acc)
        new[k] = acc
    return new


def entry_exact(T0, cols, coef, k, i, c_lo=0):
    """One written entry by the Fraction chain."""
    return kh.chain_exact(0.0, [coef[e][k] for e in range(len(cols))], [T0[int(c) - c_lo][i] for c in cols])


def model_d(cost, minus_pi, rows, values):
    """d of one new column as Engine::add_columns forms it: an fma chain from the cost over its nonzero entries, rows ascending."""
    order = np.argsort(np.asarray(rows))
    acc = float(cost)
    for e in order:
        if values[e] != 0.0:
            acc = kh.fma_exact(float(minus_pi[rows[e]]), float(values[e]), acc)
    return acc


# ------------------------------------------------------------------------------------------------------------------------
# a case: logical operands, pitches, images
# ------------------------------------------------------------------------------------------------------------------------
class Case:
    """m rows, n_store stored columns of which the last n_owned = n_store - c_lo are owned, `count` new columns over a list of
    `entries` identity columns, p pending rows of kmax.  Tableau column = storage column - col_off.  `extra`: columns of room beyond
    the new ones in every pitch and image."""

    def __init__(self, m, n_store, count, entries, p, *, kmax=None, c_lo=0, col_off=0, batch=8, extra=3, seed=0, integers=False):
        rng = np.random.default_rng(seed)
        self.m, self.n_store, self.count, self.entries, self.p = m, n_store, count, entries, p
        self.kmax = kmax if kmax is not None else max(p, 1)
        self.c_lo, self.col_off, self.batch, self.extra = c_lo, col_off, batch, extra
        self.n_owned = n_store - c_lo
        data = (lambda shape: kh.int_data(rng, shape)) if integers else (lambda shape: kh.real_data(rng, shape, zeros=0.1, neg_zeros=0.05))
        self.T0, self.R0 = data((self.n_owned, m)), data((p, self.n_owned))
        # the identity columns of the list: distinct owned columns as the engine's lists have them; a list longer than the owned
        # columns (the kernel does not care) repeats columns
        self.cols = (c_lo + rng.choice(self.n_owned, size=entries, replace=entries > self.n_owned)).astype(np.int32)
        self.coef = data((entries, count))
        self.S = kh.distinct_rows(rng, m, p).astype(np.int32) if p else np.zeros(0, dtype=np.int32)
        self.d_new, self.cost_new = data(count), data(count)
        self.flags = rng.integers(0, 3, n_store - col_off).astype(np.uint8)
        self.ld_t = kh.round_up(m + extra, 2)
        self.ld_r = kh.round_up(self.n_owned + count + extra, 2)
        self.first_virtual = 4

    def images(self):
        """Every device image before the launch: the logical data where the engine keeps it, sentinels elsewhere."""
        m, n, cnt, kmax, p = self.m, self.n_owned, self.count, self.kmax, self.p
        f, i = (lambda size: np.full(size, kh.SENTINEL)), (lambda size: np.full(size, kh.SENTINEL_INT, dtype=np.int32))
        T0 = f((n + cnt, self.ld_t)); T0[:n, :m] = self.T0
        R0 = f((kmax + 1, self.ld_r)); R0[:p, :n] = self.R0
        d = f(self.n_store + cnt); d[self.c_lo:self.n_store] = np.arange(n) * 0.5 - 3.0
        cost = f(self.n_store + cnt); cost[:self.n_store] = 1.25
        flags = np.full(self.flags.size + cnt, 2, dtype=np.uint8); flags[:self.flags.size] = self.flags
        S = i(kmax); S[:p] = self.S
        return dict(T0=T0.reshape(-1), R0=R0.reshape(-1), d=d, cost_store=cost, in_basis=flags, S=S, vrow0=i(self.first_virtual + cnt),
                    vrow1=i(self.first_virtual + cnt), vsign=i(self.first_virtual + cnt), cols=self.cols.copy(),
                    coef=np.ascontiguousarray(self.coef).reshape(-1), d_new=self.d_new.copy(), cost_new=self.cost_new.copy())

    def expected(self):
        """Every image after the launch, by the comments of k_tab_col_apply / k_tab_col_tail."""
        m, n, cnt, kmax, p = self.m, self.n_owned, self.count, self.kmax, self.p
        img = {k: v.copy() for k, v in self.images().items()}
        new = model_new_columns(self.T0, self.cols, self.coef, self.c_lo)
        T0 = img["T0"].reshape(n + cnt, self.ld_t)
        T0[n:, :m] = new
        R0 = img["R0"].reshape(kmax + 1, self.ld_r)
        R0[:, n:n + cnt] = 0.0
        if p:
            R0[:p, n:n + cnt] = new[:, self.S].T
        k = np.arange(cnt)
        img["d"][self.n_store + k] = self.d_new
        img["cost_store"][self.n_store + k] = self.cost_new
        img["in_basis"][self.flags.size + k] = 0
        img["vrow0"][self.first_virtual + k] = -1
        img["vrow1"][self.first_virtual + k] = -1
        img["vsign"][self.first_virtual + k] = 1
        return img, new

    def launch(self):
        """The images after rkcol_tab_add_columns."""
        assert kh.load().rkcol_col_tile() == COL_TILE
        img = self.images()
        scalars = [self.m, self.n_owned, self.c_lo, self.col_off, self.p, self.kmax, self.batch, self.count, self.entries, self.ld_t, self.ld_r,
                   self.first_virtual]
        names = ("T0", "R0", "d", "cost_store", "in_basis", "S", "vrow0", "vrow1", "vsign", "cols", "coef", "d_new", "cost_new")
        kh._call("rkcol_tab_add_columns", scalars, {name: img[name] for name in names})
        return img
