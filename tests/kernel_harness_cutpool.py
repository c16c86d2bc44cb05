"""Helper module of the kernel tests of the cut pool (not collected by pytest): the calls of
tests/kernels/harness_cutpool.cpp (through tests/kernel_harness.py), the reference model of launch_cutpool_separate and launch_cutpool_add_operands in
the orders relp_kernels.h states, and the construction of the device images a case starts from and must end with.

Reference arithmetic: `kernel_harness.fma_exact` (the Fraction fma) chains.
  x_j      = b[r] where basis[r] == j for a structural j, +0.0 elsewhere
  s_k      = rhs[k] - acc, acc = 0.0 then fma(value, x[column], acc) over the stored entries of cut k in stored order; padding
             (column -1) skipped
  key      = s_k, or s_k / norm_k by efficacy (norm 0 counts as 1): one f64 division
  winner   of a share: the active cut with the smallest key among those with s_k < -tol, the lowest index among equal keys; shares
           of ceil(count / segments) cuts, separated in chunks of CHUNK cuts (one partial per chunk)
  the add  mark[j] = 0 (no chosen cut touches column j), 1 (touched, not basic) or 2 + place (touched and basic: its row's place
           in the union list); rows = those rows ascending; coef[e][x] / A[j][a_row0 + x] = the value of cut ids[x] on column j,
           0.0 elsewhere; b[m + x] = rhs - (fma chain of coef[e][x] * b[rows[e]] over the WHOLE list, zeros included); active = 0

The sliced-ELL image is packed by kernel_harness_pool.pack_ell, independently of relp_pool.hpp.  A cut is a list of (column, value);
a test may store a hole (column -1, any value) anywhere."""
from __future__ import annotations

import numpy as np

import kernel_harness as kh
import kernel_harness_pool as khp

SLICE, CHUNK = khp.SLICE, khp.CHUNK
diff_images = kh.diff_images
segment_size, segment_chunks = khp.segment_size, khp.segment_chunks


def _check_constants():
    lib = kh.load()
    assert (lib.rkcutpool_slice(), lib.rkcutpool_chunk()) == (SLICE, CHUNK)


def norm_of(cut):
    acc = 0.0
    for c, v in cut:
        if c >= 0:
            acc = kh.fma_exact(float(v), float(v), acc)
    return float(np.sqrt(acc))


def key_of(s, norm, by_efficacy):
    return float(s) / (1.0 if norm == 0.0 else float(norm)) if by_efficacy else float(s)


def model_winner(s, key, active, lo, hi, tol):
    """(key, index) of the winner among the cuts [lo, hi), or (inf, -1)."""
    best, best_k = np.inf, -1
    for k in range(lo, hi):
        if active[k] and s[k] < -tol and (best_k < 0 or key[k] < best):
            best, best_k = key[k], k
    return best, best_k


def random_cuts(rng, nr_normal, count, longest, long_cut=None, empty=()):
    """`count` cuts over nr_normal columns, columns ascending, lengths in [1, min(longest, 5)] but for `long_cut` (exactly `longest`
    entries) and the `empty` ones."""
    return khp.random_columns(rng, nr_normal, count, longest, long_column=long_cut, empty=empty)


def random_basis(rng, m, nr_normal, structural):
    """m basis entries: `structural` distinct structural columns in random rows, the other rows basic in columns behind them."""
    basis = (nr_normal + rng.permutation(4 * m)[:m]).astype(np.int32)
    rows = rng.permutation(m)[:structural]
    basis[rows] = rng.permutation(nr_normal)[:structural]
    return basis


class Case:
    """A pool of `cuts` over nr_normal structural columns beside a tableau of m rows: b random, the basis as given or random with
    about half of min(m, nr_normal) structural columns basic."""

    def __init__(self, m, nr_normal, cuts, *, seed=0, rhs=None, active=None, basis=None, b=None, pad_value=0.0):
        rng = np.random.default_rng(seed)
        self.m, self.nr_normal, self.cuts, self.count = m, nr_normal, cuts, len(cuts)
        self.slice_ptr, self.col, self.val = khp.pack_ell(cuts, pad_value) if cuts else (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32),
                                                                                         np.zeros(0))
        self.rhs = kh.real_data(rng, self.count) if rhs is None else np.asarray(rhs, dtype=np.float64)
        self.norm = np.array([norm_of(c) for c in cuts], dtype=np.float64)
        self.active = np.ones(self.count, dtype=np.uint8) if active is None else np.asarray(active, dtype=np.uint8)
        self.b = kh.real_data(rng, m) if b is None else np.asarray(b, dtype=np.float64)
        self.basis = random_basis(rng, m, nr_normal, (min(m, nr_normal) + 1) // 2) if basis is None else np.asarray(basis, dtype=np.int32)

    def x(self):
        x = np.zeros(self.nr_normal)
        for r, j in enumerate(self.basis):
            if 0 <= j < self.nr_normal:
                x[j] = self.b[r]
        return x

    def slacks(self):
        x = self.x()
        out = np.zeros(self.count)
        for k, cut in enumerate(self.cuts):
            acc = 0.0
            for c, v in cut:
                if c >= 0:
                    acc = kh.fma_exact(float(v), float(x[c]), acc)
            out[k] = self.rhs[k] - acc
        return out

    def pool_images(self):
        return dict(slice_ptr=self.slice_ptr.copy(), col=self.col.copy(), val=self.val.copy(), rhs=self.rhs.copy(), norm=self.norm.copy(),
                    active=self.active.copy(), basis=self.basis.copy())

    # -- launch_cutpool_separate ------------------------------------------------------------------------------------------
    def separate_images(self, segments):
        f, i = (lambda n: np.full(n, kh.SENTINEL)), (lambda n: np.full(n, kh.SENTINEL_INT, dtype=np.int32))
        parts = segments * segment_chunks(self.count, segments) if segments else 0
        img = self.pool_images()
        img.update(b=self.b.copy(), x=f(self.nr_normal), s_all=f(self.count), part_d=f(parts), part_k=i(parts), out_k=i(segments),
                   out_s=f(segments), found=i(1 if segments else 0))
        return img

    def separate_expected(self, segments, tol, by_efficacy=0, s=None):
        img = self.separate_images(segments)
        if self.count:
            img["x"][:] = self.x()                         # (a pool without cuts launches nothing but the winners)
            s = self.slacks() if s is None else s
            img["s_all"][:] = s
        if segments and self.count:
            key = np.array([key_of(s[k], self.norm[k], by_efficacy) for k in range(self.count)])
            size, chunks = segment_size(self.count, segments), segment_chunks(self.count, segments)
            found = 0
            for sg in range(segments):
                best, best_k = np.inf, -1
                for c in range(chunks):
                    lo = sg * size + c * CHUNK
                    hi = max(lo, min(lo + CHUNK, (sg + 1) * size, self.count))
                    pd, pk = model_winner(s, key, self.active, lo, hi, tol)
                    img["part_d"][sg * chunks + c], img["part_k"][sg * chunks + c] = pd, pk
                    if pk >= 0 and (best_k < 0 or pd < best):
                        best, best_k = pd, pk
                if chunks > 1:                              # k_pool_fold: the share's winner into its first slot
                    img["part_d"][sg * chunks], img["part_k"][sg * chunks] = best, best_k
                if best_k >= 0:
                    img["out_k"][found], img["out_s"][found] = best_k, s[best_k]
                    found += 1
            img["found"][0] = found
        elif segments:
            img["found"][0] = 0
        return img

    def separate(self, segments, tol, by_efficacy=0, lengths=None):
        img = self.separate_images(segments)
        _launch("rkcutpool_separate", [self.count, self.m, self.nr_normal, segments, by_efficacy], [tol], img,
                ("slice_ptr", "col", "val", "rhs", "norm", "active", "basis", "b", "x", "s_all", "part_d", "part_k", "out_k", "out_s", "found"),
                lengths)
        return img

    # -- launch_cutpool_add_operands --------------------------------------------------------------------------------------
    def add_shape(self, ids):
        """(the union list: rows ascending whose basic column is structural and touched, the touched columns, the longest cut)."""
        ids = [k for k in ids if 0 <= k < self.count]         # (an id outside the pool is the harness's to refuse)
        touched = {c for k in ids for c, _ in self.cuts[k] if c >= 0}
        rows = [r for r in range(self.m) if int(self.basis[r]) in touched]
        longest = max([max([e + 1 for e, (c, _) in enumerate(self.cuts[k]) if c >= 0], default=0) for k in ids], default=0)
        return rows, touched, longest

    def add_images(self, ids, a_row0=3, extra=2, room=None):
        f, i = (lambda n: np.full(n, kh.SENTINEL)), (lambda n: np.full(n, kh.SENTINEL_INT, dtype=np.int32))
        rows, touched, _ = self.add_shape(ids)
        self.room = min(len(touched), self.m) if room is None else room
        self.ld_a, self.a_row0 = a_row0 + len(ids) + extra, a_row0
        img = self.pool_images()
        img.update(b=np.concatenate([self.b, f(len(ids))]), ids=np.asarray(ids, dtype=np.int32), mark=i(self.nr_normal), rows=i(self.room + 2),
                   entries_out=i(1), coef=f(self.room * len(ids)), A=f(self.nr_normal * self.ld_a))
        return img

    def add_expected(self, ids, a_row0=3, extra=2, room=None):
        img = self.add_images(ids, a_row0, extra, room)
        rows, touched, _ = self.add_shape(ids)
        place = {int(self.basis[r]): e for e, r in enumerate(rows)}
        img["mark"][:] = [2 + place[j] if j in place else 1 if j in touched else 0 for j in range(self.nr_normal)]
        img["rows"][:len(rows)] = rows
        img["entries_out"][0] = len(rows)
        coef = img["coef"].reshape(self.room, len(ids)) if self.room else img["coef"]
        coef[...] = 0.0
        A = img["A"].reshape(self.nr_normal, self.ld_a)
        A[:, a_row0:a_row0 + len(ids)] = 0.0
        for x, k in enumerate(ids):
            for c, v in self.cuts[k]:
                if c >= 0:
                    A[c, a_row0 + x] = v
                    if c in place:
                        coef[place[c], x] = v
            acc = 0.0
            for e, r in enumerate(rows):
                acc = kh.fma_exact(float(coef[e, x]), float(self.b[r]), acc)
            img["b"][self.m + x] = self.rhs[k] - acc
            img["active"][k] = 0
        return img

    def add(self, ids, a_row0=3, extra=2, room=None, lengths=None, longest=None):
        img = self.add_images(ids, a_row0, extra, room)
        _, _, lg = self.add_shape(ids)
        scalars = [self.count, self.m, self.nr_normal, len(ids), lg if longest is None else longest, self.room, self.ld_a, a_row0]
        _launch("rkcutpool_add_operands", scalars, [], img,
                ("slice_ptr", "col", "val", "rhs", "norm", "active", "basis", "b", "ids", "mark", "rows", "entries_out", "coef", "A"), lengths)
        return img


def _launch(name, scalars, reals, img, names, lengths):
    """One harness call on the images; `lengths` overrides the length passed for an image (the refusal tests)."""
    _check_constants()
    kh._call(name, scalars, {n: img[n] for n in names}, reals, lengths)
