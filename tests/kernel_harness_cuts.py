"""Helper module of the kernel tests of the in-place cut rows (not collected by pytest): the calls of
tests/kernels/harness_cuts.cpp (through tests/kernel_harness.py), the reference model of launch_tab_add_cuts in the summation order relp_kernels.h
states, and the construction of the device images a case starts from and must end with.

Reference arithmetic: `kernel_harness.fma_vec` (held to `fma_exact`, the Fraction fma, by tests/test_kernel_models.py) over vectors,
`chain_exact` for single entries.  The order of launch_tab_add_cuts:
  u[k][j]      thread t of 256 sums coef[e][k] * W[j][rows[e]] over e = t, t + 256, ... ascending from 0.0, then the tree
               s[t] += s[t + half], half = 128 .. 1 (`kernel_harness.model_pending`); only when p > 0 and the list is not empty
  acc[k][c]    from 0.0: fma(coef[e][k], T0[c][rows[e]], acc) over e ascending, then fma(u[k][j], R0[j][c], acc) over j ascending
  T0[c][m + k] g[c][k] - acc for a structural column, 0.0 - acc for any other, exactly 0.0 for a column flagged basic (1)

Layouts.  Logical arrays are C-ordered as in kernel_harness: T0[c][i] (n_owned x m), W[j][i] (p x m), R0[j][c] (p x n_owned),
coef[e][k], g[sp][k] (structural column sp, cut k).  `Case.images()` lays them into whole device images with the case's pitches and
the sentinels of kernel_harness everywhere else; `Case.expected()` is every image after the launch."""
from __future__ import annotations

import numpy as np

import kernel_harness as kh

CUT_TILE = 8
image_bits, diff_images = kh.image_bits, kh.diff_images


# ------------------------------------------------------------------------------------------------------------------------
# the model (logical arrays in, logical arrays out)
# ------------------------------------------------------------------------------------------------------------------------
def model_u(coef, W, rows):
    """u[k][j], count x p."""
    coef, W = np.asarray(coef, dtype=np.float64), np.asarray(W, dtype=np.float64)
    count = coef.shape[1]
    rows = np.asarray(rows, dtype=np.int64)
    return np.stack([kh.model_pending(coef[:, k], W[:, rows]) for k in range(count)]) if W.shape[0] else np.zeros((count, 0))


def model_cut_rows(T0, W, R0, rows, coef, g_of_column, basic):
    """(new[c][k], u): the entries T0[c][m + k] launch_tab_add_cuts writes for the old columns, and u (count x p, or count x 0 when
    nothing pending is read).  g_of_column[c][k]: the cut coefficients of column c (zeros for a column that is not structural);
    basic[c]: the column is flagged basic."""
    T0, W, R0, coef, g = (np.asarray(x, dtype=np.float64) for x in (T0, W, R0, coef, g_of_column))
    rows = np.asarray(rows, dtype=np.int64)
    n = T0.shape[0]
    count = g.shape[1]
    p = W.shape[0] if rows.size else 0                         # an empty list: the launcher reads no pending row
    u = model_u(coef, W[:p], rows)
    new = np.zeros((n, count))
    for k in range(count):
        acc = np.zeros(n)
        for e in range(rows.size):
            acc = kh.fma_vec(coef[e, k], T0[:, rows[e]], acc)
        for j in range(p):
            acc = kh.fma_vec(u[k, j], R0[j], acc)
        new[:, k] = np.where(np.asarray(basic, dtype=bool), 0.0, g[:, k] - acc)
    return new, u


def entry_exact(T0, W, R0, rows, coef, g, k, c, u_kj):
    """One written entry by the Fraction chain: g - chain(chain(0, coef[:, k], T0[c, rows]), u[k], R0[:, c])."""
    acc = kh.chain_exact(0.0, [coef[e][k] for e in range(len(rows))], [T0[c][r] for r in rows])
    acc = kh.chain_exact(acc, list(u_kj), [R0[j][c] for j in range(len(u_kj))])
    return float(g) - acc


# ------------------------------------------------------------------------------------------------------------------------
# a case: logical operands, pitches, images
# ------------------------------------------------------------------------------------------------------------------------
class Case:
    """m_old rows, n_store stored columns of which the last n_owned = n_store - c_lo are owned, `count` cuts over a list of
    `entries` rows, p pending rows of kmax.  Structural columns: the storage columns [struct_c0, struct_c0 + nr_normal);
    tableau column = storage column - col_off.  `extra`: rows and columns of room beyond the cuts in every pitch and image."""

    def __init__(self, m, n_store, count, entries, p, *, kmax=None, c_lo=0, col_off=0, struct_c0=None, nr_normal=None, batch=8, extra=3,
                 seed=0, integers=False, basic=(), barred=(), cuts_before=2):
        rng = np.random.default_rng(seed)
        self.m, self.n_store, self.count, self.entries, self.p = m, n_store, count, entries, p
        self.kmax = kmax if kmax is not None else max(p, 1)
        self.c_lo, self.col_off, self.batch = c_lo, col_off, batch
        self.n_owned = n_store - c_lo
        self.struct_c0 = col_off if struct_c0 is None else struct_c0
        self.nr_normal = max(1, (n_store - self.struct_c0) // 2) if nr_normal is None else nr_normal
        data = (lambda shape: kh.int_data(rng, shape)) if integers else (lambda shape: kh.real_data(rng, shape, zeros=0.1, neg_zeros=0.05))
        self.T0, self.W, self.R0 = data((self.n_owned, m)), data((p, m)), data((p, self.n_owned))
        # distinct rows as the engine's lists have them; a list longer than m (the kernel does not care) repeats rows
        self.rows = np.sort(rng.choice(m, size=entries, replace=entries > m)).astype(np.int32)
        self.coef = data((entries, count))
        self.g = data((self.nr_normal, count))
        n_tab = n_store - col_off
        self.flags = np.zeros(n_tab, dtype=np.uint8)
        for j in basic:
            self.flags[j] = 1
        for j in barred:
            self.flags[j] = 2
        # pitches: the roundings of create() applied to a room of count + extra
        self.ld_t, self.ld_b = kh.round_up(m + count + extra, 2), kh.round_up(m + count + extra, 16)
        self.ld_r = kh.round_up(self.n_owned + count + extra, 2)
        self.a_row0 = 5 + cuts_before                                        # constraint rows and earlier cuts in front
        self.ld_a = kh.round_up(self.a_row0 + count + extra, 2)
        self.first_virtual = 4

    # -- logical helpers --
    def g_of_column(self):
        out = np.zeros((self.n_owned, self.count))
        c = self.c_lo + np.arange(self.n_owned)
        sp = c - self.struct_c0
        inside = (sp >= 0) & (sp < self.nr_normal)
        out[inside] = self.g[sp[inside]]
        return out

    def basic(self):
        j = self.c_lo + np.arange(self.n_owned) - self.col_off
        inside = (j >= 0) & (j < self.flags.size)
        out = np.zeros(self.n_owned, dtype=bool)
        out[inside] = self.flags[j[inside]] == 1
        return out

    # -- images --
    def images(self):
        """Every device image before the launch: the logical data where the engine keeps it, sentinels elsewhere."""
        m, n, cnt, kmax, p = self.m, self.n_owned, self.count, self.kmax, self.p
        f, i = (lambda size: np.full(size, kh.SENTINEL)), (lambda size: np.full(size, kh.SENTINEL_INT, dtype=np.int32))
        T0 = f((n + cnt, self.ld_t)); T0[:n, :m] = self.T0
        W = f((kmax, self.ld_b)); W[:p, :m] = self.W
        R0 = f((kmax + 1, self.ld_r)); R0[:p, :n] = self.R0
        d = f(self.n_store + cnt); d[self.c_lo:self.n_store] = np.arange(n) * 0.5 - 3.0
        cost = f(self.n_store + cnt); cost[:self.n_store] = 1.25
        flags = np.full(self.flags.size + cnt, 2, dtype=np.uint8); flags[:self.flags.size] = self.flags
        A = f((self.nr_normal, self.ld_a)); A[:, self.a_row0:self.a_row0 + cnt] = self.g
        return dict(T0=T0.reshape(-1), W=W.reshape(-1), R0=R0.reshape(-1), d=d, cost_store=cost, in_basis=flags, idcol=i(m + cnt), basis=i(m + cnt),
                    pos_of_row=i(m + cnt), vrow0=i(self.first_virtual + cnt), vrow1=i(self.first_virtual + cnt), vsign=i(self.first_virtual + cnt),
                    A=A.reshape(-1), rows=self.rows.copy(), coef=np.ascontiguousarray(self.coef).reshape(-1), u=f(cnt * kmax))

    def expected(self):
        """Every image after the launch, by the comments of k_tab_cut_pending / k_tab_cut_rows / k_tab_cut_tail."""
        m, n, cnt, kmax = self.m, self.n_owned, self.count, self.kmax
        img = {k: v.copy() for k, v in self.images().items()}
        new, u = model_cut_rows(self.T0, self.W, self.R0, self.rows, self.coef, self.g_of_column(), self.basic())
        T0 = img["T0"].reshape(n + cnt, self.ld_t)
        T0[:n, m:m + cnt] = new
        T0[n:, :m + cnt] = 0.0
        T0[n + np.arange(cnt), m + np.arange(cnt)] = 1.0
        img["W"].reshape(kmax, self.ld_b)[:, m:m + cnt] = 0.0
        img["R0"].reshape(kmax + 1, self.ld_r)[:, n:n + cnt] = 0.0
        ui = img["u"].reshape(cnt, kmax)
        ui[:, :u.shape[1]] = u
        k = np.arange(cnt)
        img["d"][self.n_store + k] = 0.0
        img["cost_store"][self.n_store + k] = 0.0
        img["in_basis"][self.flags.size + k] = 1
        img["idcol"][m + k] = self.n_store + k
        img["basis"][m + k] = self.flags.size + k
        img["pos_of_row"][m + k] = -1
        img["vrow0"][self.first_virtual + k] = m + k
        img["vrow1"][self.first_virtual + k] = -1
        img["vsign"][self.first_virtual + k] = 1
        return img, new, u

    def launch(self):
        """The images after rkc_tab_add_cuts."""
        assert kh.load().rkc_cut_tile() == CUT_TILE
        img = self.images()
        scalars = [self.m, self.n_owned, self.c_lo, self.col_off, self.p, self.kmax, self.batch, self.count, self.entries, self.ld_t, self.ld_b,
                   self.ld_r, self.ld_a, self.a_row0, self.struct_c0, self.nr_normal, self.first_virtual]
        names = ("T0", "W", "R0", "d", "cost_store", "in_basis", "idcol", "basis", "pos_of_row", "vrow0", "vrow1", "vsign", "A",
                 "rows", "coef", "u")
        kh._call("rkc_tab_add_cuts", scalars, {name: img[name] for name in names})
        return img
