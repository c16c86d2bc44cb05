"""Helper module of the kernel tests of the column pool (not collected by pytest): the calls of
tests/kernels/harness_pool.cpp (through tests/kernel_harness.py), the reference model of launch_pool_price and launch_pool_add_operands in the orders
relp_kernels.h states, and the construction of the device images a case starts from and must end with.

Reference arithmetic: `kernel_harness.fma_exact` (the Fraction fma) chains.
  (-pi)_i  = d[idcol[i]] - cost_store[idcol[i]]                     one f64 subtraction
  d_k      = cost[k], then fma((-pi)_row, value, d_k) over the stored entries of column k in stored order; padding (row -1) skipped
  winner   of a share: the active column with the smallest d_k < -tol, the lowest index among equal d_k; shares of
           ceil(count / segments) columns, priced in chunks of CHUNK columns (one partial per chunk)
  the add  rank[i] = place of row i among the rows the chosen columns touch (ascending) or -1, cols = idcol of those rows,
           coef[e][x] / col_a[a0 + x][row] = the value of column ids[x] in that row, 0.0 elsewhere; d_new, cost_new; active = 0

The sliced-ELL image is packed here independently of relp_pool.hpp: column k is lane k % 64 of slice k // 64, entry e at
slice_ptr[k // 64] + e * 64 + k % 64.  A column is a list of (row, value); a test may store a hole (row -1, any value) anywhere."""
from __future__ import annotations

import numpy as np

import kernel_harness as kh

SLICE, CHUNK = 64, 256
diff_images = kh.diff_images


def _check_constants():
    lib = kh.load()
    assert (lib.rkpool_slice(), lib.rkpool_chunk()) == (SLICE, CHUNK)


# ------------------------------------------------------------------------------------------------------------------------
# the image and the model
# ------------------------------------------------------------------------------------------------------------------------
def pack_ell(columns, pad_value=0.0):
    """(slice_ptr, row, val) of the columns, each a list of (row, value) in the order they are to be stored."""
    count = len(columns)
    slices = (count + SLICE - 1) // SLICE
    slice_ptr = np.zeros(slices + 1, dtype=np.int64)
    for s in range(slices):
        width = max(len(c) for c in columns[s * SLICE:(s + 1) * SLICE])
        slice_ptr[s + 1] = slice_ptr[s] + width * SLICE
    row = np.full(int(slice_ptr[-1]), -1, dtype=np.int32)
    val = np.full(int(slice_ptr[-1]), pad_value, dtype=np.float64)
    for k, col in enumerate(columns):
        for e, (r, v) in enumerate(col):
            at = int(slice_ptr[k // SLICE]) + e * SLICE + k % SLICE
            row[at], val[at] = r, v
    return slice_ptr, row, val


def minus_pi(d, cost_store, idcol):
    return np.asarray(d)[idcol] - np.asarray(cost_store)[idcol]


def chain(cost, column, mpi):
    acc = float(cost)
    for r, v in column:
        if r >= 0:
            acc = kh.fma_exact(float(mpi[r]), float(v), acc)
    return acc


def segment_size(count, segments):
    return (count + segments - 1) // segments


def segment_chunks(count, segments):
    return max(1, (segment_size(count, segments) + CHUNK - 1) // CHUNK)


def model_winners(d, active, lo, hi, tol):
    """(d, index) of the winner among the columns [lo, hi), or (inf, -1)."""
    best, best_k = np.inf, -1
    for k in range(lo, hi):
        if active[k] and d[k] < -tol and (best_k < 0 or d[k] < best):
            best, best_k = d[k], k
    return best, best_k


def random_columns(rng, m, count, longest, long_column=None, empty=()):
    """`count` columns over m rows, rows ascending, lengths in [1, min(longest, 5)] but for `long_column` (exactly `longest`
    entries) and the `empty` ones."""
    columns = []
    for k in range(count):
        n = 0 if k in empty else longest if k == long_column or long_column is None and k == 0 else int(rng.integers(1, min(longest, 5) + 1))
        rows = np.sort(rng.permutation(m)[:n])
        columns.append([(int(r), float(v)) for r, v in zip(rows, kh.real_data(rng, n))])
    return columns


class Case:
    """A pool of `columns` over m rows beside a tableau of n_store stored columns: d and cost_store random, idcol a random injection
    of the rows into the stored columns."""

    def __init__(self, m, columns, *, n_store=None, seed=0, cost=None, active=None, pad_value=0.0):
        rng = np.random.default_rng(seed)
        self.m, self.columns, self.count = m, columns, len(columns)
        self.n_store = n_store if n_store is not None else m + 5
        self.slice_ptr, self.row, self.val = pack_ell(columns, pad_value)
        self.cost = kh.real_data(rng, self.count) if cost is None else np.asarray(cost, dtype=np.float64)
        self.active = np.ones(self.count, dtype=np.uint8) if active is None else np.asarray(active, dtype=np.uint8)
        self.d = kh.real_data(rng, self.n_store)
        self.cost_store = kh.real_data(rng, self.n_store, zeros=0.3)
        self.idcol = rng.permutation(self.n_store)[:m].astype(np.int32)
        self.mpi = minus_pi(self.d, self.cost_store, self.idcol)

    def reduced_costs(self):
        return np.array([chain(self.cost[k], self.columns[k], self.mpi) for k in range(self.count)])

    def pool_images(self):
        return dict(slice_ptr=self.slice_ptr.copy(), row=self.row.copy(), val=self.val.copy(), cost=self.cost.copy(), active=self.active.copy(),
                    d=self.d.copy(), cost_store=self.cost_store.copy(), idcol=self.idcol.copy(), minus_pi=np.full(self.m, kh.SENTINEL))

    # -- launch_pool_price ------------------------------------------------------------------------------------------------
    def price_images(self, segments, write_d=True):
        f, i = (lambda n: np.full(n, kh.SENTINEL)), (lambda n: np.full(n, kh.SENTINEL_INT, dtype=np.int32))
        parts = segments * segment_chunks(self.count, segments) if segments else 0
        img = self.pool_images()
        img.update(d_all=f(self.count if write_d else 0), part_d=f(parts), part_k=i(parts), out_k=i(segments), out_d=f(segments),
                   found=i(1 if segments else 0))
        return img

    def price_expected(self, segments, tol, write_d=True, d=None):
        img = self.price_images(segments, write_d)
        d = self.reduced_costs() if d is None else d
        if self.count:
            img["minus_pi"][:] = self.mpi                  # (a pool without columns launches nothing)
        if write_d:
            img["d_all"][:] = d
        if segments and self.count:
            size, chunks = segment_size(self.count, segments), segment_chunks(self.count, segments)
            found = 0
            for s in range(segments):
                best, best_k = np.inf, -1
                for c in range(chunks):
                    lo = s * size + c * CHUNK
                    hi = max(lo, min(lo + CHUNK, (s + 1) * size, self.count))
                    pd, pk = model_winners(d, self.active, lo, hi, tol)
                    img["part_d"][s * chunks + c], img["part_k"][s * chunks + c] = pd, pk
                    if pk >= 0 and (best_k < 0 or pd < best):
                        best, best_k = pd, pk
                if chunks > 1:                              # k_pool_fold: the share's winner into its first slot
                    img["part_d"][s * chunks], img["part_k"][s * chunks] = best, best_k
                if best_k >= 0:
                    img["out_k"][found], img["out_d"][found] = best_k, best
                    found += 1
            img["found"][0] = found
        elif segments:
            img["found"][0] = 0
        return img

    def price(self, segments, tol, write_d=True, lengths=None):
        img = self.price_images(segments, write_d)
        _launch("rkpool_price", [self.count, self.m, self.n_store, segments], [tol], img,
                ("slice_ptr", "row", "val", "cost", "active", "d", "cost_store", "idcol", "minus_pi", "d_all", "part_d", "part_k", "out_k", "out_d", "found"),
                lengths)
        return img

    # -- launch_pool_add_operands -----------------------------------------------------------------------------------------
    def add_shape(self, ids):
        ids = [k for k in ids if 0 <= k < self.count]         # (an id outside the pool is the harness's to refuse)
        touched = sorted({r for k in ids for r, _ in self.columns[k] if r >= 0})
        longest = max([max([e + 1 for e, (r, _) in enumerate(self.columns[k]) if r >= 0], default=0) for k in ids], default=0)
        return touched, longest

    def add_images(self, ids, a0=2, extra=3):
        f, i = (lambda n: np.full(n, kh.SENTINEL)), (lambda n: np.full(n, kh.SENTINEL_INT, dtype=np.int32))
        touched, _ = self.add_shape(ids)
        self.ld_c, self.a0 = kh.round_up(self.m + extra, 2), a0
        img = self.pool_images()
        img.update(ids=np.asarray(ids, dtype=np.int32), rank=i(self.m), cols=i(len(touched) + 2), entries_out=i(1),
                   coef=f(len(touched) * len(ids)), col_a=f((a0 + len(ids)) * self.ld_c), d_new=f(len(ids)), cost_new=f(len(ids)))
        return img

    def add_expected(self, ids, a0=2, extra=3):
        img = self.add_images(ids, a0, extra)
        touched, _ = self.add_shape(ids)
        place = {r: e for e, r in enumerate(touched)}
        img["rank"][:] = [place.get(i, -1) for i in range(self.m)]
        img["minus_pi"][:] = self.mpi
        img["cols"][:len(touched)] = self.idcol[touched]
        img["entries_out"][0] = len(touched)
        coef = img["coef"].reshape(len(touched), len(ids)) if touched else img["coef"]
        coef[...] = 0.0
        col_a = img["col_a"].reshape(a0 + len(ids), self.ld_c)
        col_a[a0:, :self.m] = 0.0
        for x, k in enumerate(ids):
            for r, v in self.columns[k]:
                if r >= 0:
                    coef[place[r], x] = v
                    col_a[a0 + x, r] = v
            img["d_new"][x] = chain(self.cost[k], self.columns[k], self.mpi)
            img["cost_new"][x] = self.cost[k]
            img["active"][k] = 0
        return img

    def add(self, ids, a0=2, extra=3, lengths=None, longest=None, entries=None):
        img = self.add_images(ids, a0, extra)
        touched, lg = self.add_shape(ids)
        scalars = [self.count, self.m, self.n_store, len(ids), lg if longest is None else longest, len(touched) if entries is None else entries,
                   self.ld_c, a0]
        _launch("rkpool_add_operands", scalars, [], img,
                ("slice_ptr", "row", "val", "cost", "active", "d", "cost_store", "idcol", "minus_pi", "ids", "rank", "cols", "entries_out", "coef", "col_a",
                 "d_new", "cost_new"), lengths)
        return img


def set_active(active, ids, flag):
    img = dict(active=np.asarray(active, dtype=np.uint8).copy(), ids=np.asarray(ids, dtype=np.int32))
    _launch("rkpool_set_active", [img["active"].size, img["ids"].size, flag], [], img, ("active", "ids"), None)
    return img


def _launch(name, scalars, reals, img, names, lengths):
    """One harness call on the images; `lengths` overrides the length passed for an image (the refusal tests)."""
    _check_constants()
    kh._call(name, scalars, {n: img[n] for n in names}, reals, lengths)
