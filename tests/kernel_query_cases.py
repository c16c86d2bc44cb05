"""Helper module of the kernel tests (not collected by pytest): the case tables of T5 - T8 (launch_tab_rhs_change,
launch_tab_cost_change, launch_tab_row_ratios, launch_tab_rhs_ranging).  tests/test_gpu_kernels_queries.py runs them on the GPU;
tests/test_kernel_models.py walks the same tables on the CPU (every case must be clean: the pick of a ratio query may not depend
on how the compiler rounds the band's bound).  A case is (id, builder); the builder returns the keyword arguments of the binding.

Constructed ties use dyadic tolerances (pivot 2^-10, zero 2^-30, tie 2^-20) and integer-valued W, R0, so that every entry of T, every
ratio and the bound are exact: "equal bits" is k1 itself, "inside" is k1 + tie / 4, "outside" is k1 + 4 tie.
"""
import numpy as np

import kernel_harness as kh

TOL_REAL = (1e-7, 1e-9, 1e-9)                          # (pivot, zero, tie)
TOL_DYADIC = (2.0 ** -10, 2.0 ** -30, 2.0 ** -20)
TIE = TOL_DYADIC[2]
INSIDE, OUTSIDE, FAR = 1.0 + TIE / 4, 1.0 + 4 * TIE, 2.0
SIZES = (1, 2, 255, 256, 257, 513)
P_SWEEP = (0, 1, 7, 8, 9, 15, 17, 31, 33, 127, 128)
COUNT_SPLITS = ((1, 1), (5, 4), (24, 1), (25, 2), (255, 1), (256, 1), (257, 1), (257, 2), (257, 256), (513, 2), (600, 3), (700, 7))
LIST_LENGTHS = (1, 7, 8, 9, 17, 64)


# ---- T5 / T6 -----------------------------------------------------------------------------------------------------------------
def sum_cases(cost):
    """(id, dict(m, n, p, kmax, c_lo, col_off, count, ncount, splits, seed)).  T6 needs count <= m (its rows ascend strictly), so
    its (count, splits) table runs at m = 700, n_owned = 300 and its count = 0 cases at m = 64, n_owned = 700."""
    cases = []

    def add(tag, **kw):
        kw.setdefault("col_off", 0)
        kw.setdefault("ncount", 0)
        kw.setdefault("kmax", 128)
        kw["seed"] = 7000 + 31 * len(cases) + (500 if cost else 0)
        cases.append((f"{tag} m={kw['m']} n_owned={kw['n']} p={kw['p']} c_lo={kw['c_lo']} col_off={kw['col_off']} "
                      f"count={kw['count']} ncount={kw['ncount']} splits={kw['splits']}", kw))

    for x in SIZES:
        for c_lo in (0, 300):
            count = min(9, x) if cost else 9
            off = 5 if cost and c_lo + x > 5 and (x + c_lo // 300) % 2 else 0
            add("shape", m=x, n=x, p=9, c_lo=c_lo, col_off=off, count=count, ncount=min(3, x) if cost else 0, splits=min(2, count))
    for p in P_SWEEP:
        add("pending", m=257, n=257, p=p, kmax=128 if p % 2 else max(p, 1), c_lo=0, col_off=5 if cost and p % 3 == 0 else 0, count=17,
            ncount=5 if cost and p % 2 else 0, splits=3 if p in (9, 128) else 1)
    for count, splits in COUNT_SPLITS:
        add("list", m=700, n=300 if cost else 64, p=9, c_lo=300 if count == 257 else 0, col_off=5 if cost and count % 2 == 0 else 0,
            count=count, ncount=7 if cost and count in (5, 257, 700) else 0, splits=splits)
    if cost:
        for ncount in (1, 300):
            add("direct only", m=64, n=700, p=9, c_lo=0, col_off=5, count=0, ncount=ncount, splits=1)
    return cases


def sum_operands(kw, cost, integer):
    """The arguments of kh.tab_rhs_change / kh.tab_cost_change for one case (dict), seeded."""
    rng = np.random.default_rng(kw["seed"] + (1 if integer else 0))
    data = kh.int_data if integer else kh.real_data
    m, n, p, c_lo, count = kw["m"], kw["n"], kw["p"], kw["c_lo"], kw["count"]
    T0, W, R0 = data(rng, (n, m)), data(rng, (p, m)), data(rng, (p, n))
    delta = data(rng, count)
    if not cost:
        cols = (c_lo + rng.integers(0, n, count)).astype(np.int32)          # any order, repeats
        return dict(T0=T0, W=W, R0=R0, b=data(rng, m), cols=cols, delta=delta, kmax=kw["kmax"], splits=kw["splits"], c_lo=c_lo)
    off = kw["col_off"]
    n_tab = c_lo + n - off
    flags = rng.choice(np.array([0, 0, 0, 1, 1, 2], dtype=np.uint8), n_tab)
    if c_lo == 0 and off:
        flags[:off] = 1              # in_basis[c] for the kept artificial block c < col_off, were it indexed without - col_off
        flags[off:2 * off] = 0
    moves = kh.cost_moves(n, c_lo, off, flags)
    d = data(rng, n)
    pinned = np.nonzero(~moves)[0]
    d[pinned] = np.array([kh.SENTINEL, -0.0, 1e300])[pinned % 3]          # a basic column keeps its d to the bit, whatever it holds
    rows = np.sort(rng.permutation(m)[:count]).astype(np.int32)
    free = np.nonzero(moves)[0]
    ncount = min(kw["ncount"], free.size)
    ncols = (c_lo + np.sort(rng.permutation(free)[:ncount])).astype(np.int32)
    return dict(T0=T0, W=W, R0=R0, d=d, in_basis=flags, rows=rows, delta=delta, ncols=ncols, ndelta=data(rng, ncount), kmax=kw["kmax"],
                splits=kw["splits"], c_lo=c_lo, col_off=off)


# ---- T7 / T8: operands with designed entries ----------------------------------------------------------------------------------
def _int_tableau(rng, m, n, p):
    return kh.int_data(rng, (n, m)), kh.int_data(rng, (p, m)), kh.int_data(rng, (p, n))


def _set_row(T0, W, R0, r, entries):
    """T0[:, r] such that row r of T = T0 + W' R0 is `entries` exactly (integer W, R0 and dyadic entries: every partial sum of the
    fma chain is exact)."""
    T0[:, r] = entries - W[:, r] @ R0
    assert (kh.model_rows_of_T(T0, W, R0, [r])[0] == entries).all()


def _set_column(T0, W, R0, c, entries):
    T0[c] = entries - R0[:, c] @ W
    assert (kh.model_columns_of_T(T0, W, R0, [c])[0] == entries).all()


def _place(entries, weights, spec):
    """spec: (index, entry, ratio): entries[index] = entry and weights[index] (d or b) = ratio * |entry|, exactly."""
    for idx, entry, ratio in spec:
        entries[idx] = entry
        weights[idx] = ratio * abs(entry)
        assert weights[idx] / abs(entry) == ratio


def _row_case(m, n, p, spec, seed, c_lo=0, col_off=0, tol=TOL_DYADIC, kmax=None, rows=None, basic=(), d_fix=()):
    """A T7 case whose list entry 0 (row rows[0]) has the entries of `spec` (local column, entry, ratio) and zeros elsewhere."""
    rng = np.random.default_rng(seed)
    T0, W, R0 = _int_tableau(rng, m, n, p)
    rows = np.asarray(rows if rows is not None else [m // 2, 0, m - 1], dtype=np.int32)
    entries, d = np.zeros(n), kh.int_data(rng, n, zeros=0.0) + 0.5
    _place(entries, d, spec)
    for c, value in d_fix:
        d[c] = value
    _set_row(T0, W, R0, rows[0], entries)
    flags = np.zeros(c_lo + n - col_off, dtype=np.uint8)
    for c, flag in basic:
        flags[c_lo + c - col_off] = flag
    return dict(T0=T0, W=W, R0=R0, d=d, in_basis=flags, rows=rows, tol=tol, kmax=p if kmax is None else kmax, c_lo=c_lo, col_off=col_off)


def _column_case(m, n, p, spec, seed, c_lo=0, tol=TOL_DYADIC, kmax=None, cols=None, basis=None, b_fix=()):
    """A T8 case whose list entry 0 (column cols[0], local) has the entries of `spec` (row, entry, ratio) and zeros elsewhere."""
    rng = np.random.default_rng(seed)
    T0, W, R0 = _int_tableau(rng, m, n, p)
    cols = np.asarray(cols if cols is not None else [n // 2, 0, n - 1], dtype=np.int32)
    entries, b = np.zeros(m), np.abs(kh.int_data(rng, m, zeros=0.0)) + 0.5
    _place(entries, b, spec)
    for i, value in b_fix:
        b[i] = value
    _set_column(T0, W, R0, cols[0], entries)
    if basis is None:
        basis = rng.permutation(m + 50)[:m]
    return dict(T0=T0, W=W, R0=R0, b=b, basis=np.asarray(basis, dtype=np.int32), cols=(c_lo + cols).astype(np.int32), tol=tol,
                kmax=p if kmax is None else kmax, c_lo=c_lo)


def _random_row_case(m, n, p, count, seed, c_lo=0, col_off=0, kmax=128):
    rng = np.random.default_rng(seed)
    T0, W, R0 = kh.real_data(rng, (n, m), 0.05, 0.02), kh.real_data(rng, (p, m), 0.05), kh.real_data(rng, (p, n), 0.05)
    d = np.abs(kh.real_data(rng, n))
    pick = rng.random(n)
    share = 0.004 * (seed % 3)                             # (a third of the cases without a ratio of 0)
    d[pick < share] = 0.0
    d[(pick >= share) & (pick < 2 * share)] = TOL_REAL[1]
    d[(pick >= 2 * share) & (pick < 3 * share)] *= -1.0
    flags = rng.choice(np.array([0, 0, 0, 1, 2], dtype=np.uint8), c_lo + n - col_off)
    if n <= 2:
        flags[:] = 0
    rows = rng.integers(0, m, count).astype(np.int32)                        # unsorted, with repeats
    if count >= 9:
        rows[5] = rows[2]
    return dict(T0=T0, W=W, R0=R0, d=d, in_basis=flags, rows=rows, tol=TOL_REAL, kmax=kmax, c_lo=c_lo, col_off=col_off)


def _random_column_case(m, n, p, count, seed, c_lo=0, kmax=128):
    rng = np.random.default_rng(seed)
    T0, W, R0 = kh.real_data(rng, (n, m), 0.05, 0.02), kh.real_data(rng, (p, m), 0.05), kh.real_data(rng, (p, n), 0.05)
    b = np.abs(kh.real_data(rng, m))
    pick = rng.random(m)
    share = 0.004 * (seed % 3)                             # (a third of the cases without a ratio of 0)
    b[pick < share] = 0.0
    b[(pick >= share) & (pick < 2 * share)] = TOL_REAL[1]
    b[(pick >= 2 * share) & (pick < 3 * share)] *= -1.0
    basis = rng.permutation(m + 40)[:m].astype(np.int64)
    art = rng.random(m) < 0.2
    basis[art] += kh.WRAPPED_ARTIFICIAL_BASE
    cols = (c_lo + rng.integers(0, n, count)).astype(np.int32)
    if count >= 9:
        cols[5] = cols[2]
    return dict(T0=T0, W=W, R0=R0, b=b, basis=basis.astype(np.int32), cols=cols, tol=TOL_REAL, kmax=kmax, c_lo=c_lo)


def _band_spec(n_blocks, in_band_blocks, sign, shift):
    """One candidate per 256-block: the minimum 1.0 twice in the last block (equal bits), ratio INSIDE in `in_band_blocks` - 1 other
    blocks with block 0 among them (its lowest index the pick), OUTSIDE at a still lower index of block 0, FAR everywhere else."""
    last = n_blocks - 1
    spec = [(last * 256 + 255 - shift, sign * 3.0, 1.0), (last * 256 + 200 - shift, sign * 5.0, 1.0),
            (7 + shift, sign * 2.0, INSIDE), (3 + shift, sign * 4.0, OUTSIDE)]
    for blk in range(1, last):
        spec.append((blk * 256 + (37 * blk + shift) % 256, sign * (1.0 + blk % 3), INSIDE if blk < in_band_blocks - 1 else FAR))
    return spec


def row_ratio_cases():
    cases = []

    def add(name, builder):
        cases.append((name, builder))

    for k, x in enumerate(SIZES):
        for c_lo in (0, 300):
            off = 5 if c_lo + x > 5 and (k + c_lo // 300) % 2 else 0
            add(f"shape m=n_owned={x} c_lo={c_lo} col_off={off}",
                lambda x=x, c_lo=c_lo, off=off: _random_row_case(x, x, 9, 9, 8100 + x + c_lo, c_lo, off))
    for p in P_SWEEP:
        add(f"pending p={p}", lambda p=p: _random_row_case(257, 257, p, 9, 8200 + p, 0, 5 if p % 2 else 0, kmax=128 if p % 2 else max(p, 1)))
    for count in LIST_LENGTHS:
        add(f"list length {count}", lambda count=count: _random_row_case(257, 257, 3, count, 8300 + count))
    neg, pos = -1.0, 1.0
    pv = TOL_DYADIC[0]
    add("one row, one column: a candidate downwards", lambda: _row_case(1, 1, 3, [(0, -2.0, 1.5)], 8398, rows=[0, 0]))
    add("two rows, two columns: one candidate each way", lambda: _row_case(2, 2, 3, [(0, 2.0, 1.5), (1, -4.0, 0.75)], 8399, c_lo=300, col_off=5, rows=[1, 0, 1]))
    add("no candidate in either direction", lambda: _row_case(33, 300, 5, [], 8401, d_fix=[(4, -3.0)]))
    add("no candidate upwards", lambda: _row_case(33, 300, 5, [(10, -2.0, 1.5), (290, -1.0, 1.0), (40, -3.0, INSIDE)], 8402))
    add("a whole block without a candidate",
        lambda: _row_case(9, 769, 3, [(5, -2.0, FAR), (6, 2.0, FAR), (700, -1.0, 1.0), (701, 4.0, 1.0), (600, -1.0, INSIDE), (601, 1.0, OUTSIDE)], 8403))
    add("entries of exactly +-tol.pivot",
        lambda: _row_case(9, 300, 3, [(2, -pv, 0.25), (3, pv, 0.25), (280, -2 * pv, 1.0), (281, 2 * pv, 1.0), (100, -pv * (1 + 2.0 ** -30), FAR),
                                      (101, pv * (1 + 2.0 ** -30), FAR)], 8404))
    add("an entry of -0.0 with tol.pivot = 0",
        lambda: _row_case(9, 300, 0, [(2, neg, 1.0), (3, pos, 1.0)], 8405, tol=(0.0, TOL_DYADIC[1], TIE), d_fix=[(1, -5.0)]) | dict(minus_zero=1))
    z = TOL_DYADIC[1]
    add("d of exactly tol.zero, below it and 0: a tie at ratio 0 across blocks",
        lambda: _row_case(9, 600, 3, [(300, neg, 1.0), (10, -2.0, 1.0), (550, -3.0, 1.0), (5, neg, 1.0), (301, pos, 1.0), (20, 2.0, 1.0), (580, 1.0, 1.0)],
                          8406, tol=(pv, z, 0.0), d_fix=[(300, z), (10, -1.0), (550, 0.0), (5, z * (1 + 2.0 ** -52)), (301, 0.0), (20, z), (580, -0.0)]))
    add("the minimum in the last block, the lowest in-band column in block 0",
        lambda: _row_case(9, 1024, 3, _band_spec(4, 3, neg, 0) + _band_spec(4, 4, pos, 1), 8407))
    add("the same behind col_off = 5: columns below it are no candidates",
        lambda: _row_case(9, 1024, 3, _band_spec(4, 3, neg, 0) + _band_spec(4, 4, pos, 1) + [(2, neg, 0.5), (1, pos, 0.5)], 8408, col_off=5))
    add("a basic and a barred column inside the band",
        lambda: _row_case(9, 1024, 3, _band_spec(4, 3, neg, 0) + _band_spec(4, 4, pos, 1) + [(5, neg, INSIDE), (6, pos, 1.0)], 8409,
                          basic=[(5, 1), (6, 2)]))
    add("every candidate in lane 63 of its wavefront",
        lambda: _row_case(9, 513, 3, [(63, -2.0, FAR), (127, -1.0, INSIDE), (191, -4.0, 1.0), (255, -1.0, OUTSIDE), (319, -2.0, 1.0), (447, 3.0, 1.0),
                                      (511, 1.0, INSIDE), (383, 2.0, FAR)], 8410))
    for p in (0, 9):
        for blocks in (kh.ENTERING_LIST_MAX, kh.ENTERING_LIST_MAX + 1):
            add(f"list overflow: {blocks} / {65 - blocks} of 34 blocks inside the band, p={p}",
                lambda p=p, blocks=blocks: _row_case(4, 34 * 256, p, _band_spec(34, blocks, neg, 0) + _band_spec(34, 65 - blocks, pos, 1), 8420 + p + blocks,
                                                     rows=[2, 0]))
    return cases


def rhs_ranging_cases():
    cases = []

    def add(name, builder):
        cases.append((name, builder))

    for x in SIZES:
        for c_lo in (0, 300):
            add(f"shape m=n_owned={x} c_lo={c_lo}", lambda x=x, c_lo=c_lo: _random_column_case(x, x, 9, 9, 9100 + x + c_lo, c_lo))
    for p in P_SWEEP:
        add(f"pending p={p}", lambda p=p: _random_column_case(257, 257, p, 9, 9200 + p, kmax=128 if p % 2 else max(p, 1)))
    for count in LIST_LENGTHS:
        add(f"list length {count}", lambda count=count: _random_column_case(257, 257, 3, count, 9300 + count))
    pv, z = TOL_DYADIC[0], TOL_DYADIC[1]
    art = kh.WRAPPED_ARTIFICIAL_BASE

    def basis_with(m, fixed, seed):
        """Distinct leaving columns >= 100, with the rows of `fixed` set to the given ones."""
        basis = 100 + np.random.default_rng(seed).permutation(m)
        for i, value in fixed:
            basis[i] = value
        return basis

    add("one row, one column: a row for a decrease", lambda: _column_case(1, 1, 3, [(0, 2.0, 1.5)], 9398, cols=[0, 0], basis=[art + 2]))
    add("two rows, two columns: one row each way", lambda: _column_case(2, 2, 3, [(0, -2.0, 1.5), (1, 4.0, 0.75)], 9399, c_lo=300, cols=[1, 0, 1]))
    add("no row in either direction", lambda: _column_case(300, 33, 5, [], 9401, b_fix=[(4, -3.0)]))
    add("no row for an increase", lambda: _column_case(300, 33, 5, [(10, 2.0, 1.5), (290, 1.0, 1.0), (40, 3.0, INSIDE)], 9402))
    add("a whole block without a row",
        lambda: _column_case(769, 9, 3, [(5, 2.0, FAR), (6, -2.0, FAR), (700, 1.0, 1.0), (701, -4.0, 1.0), (600, 1.0, INSIDE), (601, -1.0, OUTSIDE)], 9403,
                             basis=basis_with(769, [(600, 3), (601, 2)], 1)))
    add("entries of exactly +-tol.pivot",
        lambda: _column_case(300, 9, 3, [(2, pv, 0.25), (3, -pv, 0.25), (280, 2 * pv, 1.0), (281, -2 * pv, 1.0), (100, pv * (1 + 2.0 ** -30), FAR),
                                         (101, -pv * (1 + 2.0 ** -30), FAR)], 9404))
    add("an entry of -0.0 with tol.pivot = 0",
        lambda: _column_case(300, 9, 0, [(2, 1.0, 1.0), (3, -1.0, 1.0)], 9405, tol=(0.0, z, TIE), b_fix=[(1, -5.0)]) | dict(minus_zero=1))
    add("b of exactly tol.zero, below it and 0: a tie at ratio 0 across blocks, a wrapped artificial in the lowest row",
        lambda: _column_case(600, 9, 3, [(2, 1.0, 1.0), (300, 1.0, 1.0), (10, 2.0, 1.0), (550, 3.0, 1.0), (5, 1.0, 1.0), (301, -1.0, 1.0), (20, -2.0, 1.0),
                                         (580, -1.0, 1.0), (1, -1.0, 1.0)],
                             9406, tol=(pv, z, 0.0),
                             b_fix=[(2, 0.0), (300, z), (10, -1.0), (550, 0.0), (5, z * (1 + 2.0 ** -52)), (301, 0.0), (20, z), (580, -0.0), (1, 0.0)],
                             basis=basis_with(600, [(2, art + 1), (300, 40), (10, 41), (550, 7), (5, 1), (1, art), (301, 60), (20, 50), (580, art + 5)], 2)))
    add("the minimum in the last block, the smallest leaving column in block 0",
        lambda: _column_case(1024, 9, 3, _band_spec(4, 3, 1.0, 0) + _band_spec(4, 4, -1.0, 1), 9407,
                             basis=basis_with(1024, [(7, 5), (3, 1), (8, 6), (4, 2), (1023, art + 3), (1022, art + 4)], 3)))
    add("every row of the band a wrapped artificial but one",
        lambda: _column_case(1024, 9, 3, _band_spec(4, 4, 1.0, 0) + _band_spec(4, 4, -1.0, 1), 9408,
                             basis=art + np.arange(1024) - np.where(np.arange(1024) == 586, art - 99, 0)))
    add("every row in lane 63 of its wavefront",
        lambda: _column_case(513, 9, 3, [(63, 2.0, FAR), (127, 1.0, INSIDE), (191, 4.0, 1.0), (255, 1.0, OUTSIDE), (319, 2.0, 1.0), (447, -3.0, 1.0),
                                         (511, -1.0, INSIDE), (383, -2.0, FAR)], 9410,
                             basis=basis_with(513, [(127, 9), (191, 30), (319, 20), (255, 1), (447, 8), (511, 3)], 4)))
    L = kh.LEAVING_LIST_MAX
    for blocks in (L, L + 1):
        add(f"list overflow: {blocks} / {2 * L + 1 - blocks} of 66 blocks inside the band",
            lambda blocks=blocks: _column_case(66 * 256, 2, 0, _band_spec(66, blocks, 1.0, 0) + _band_spec(66, 2 * L + 1 - blocks, -1.0, 1), 9420 + blocks,
                                               cols=[1, 0], basis=basis_with(66 * 256, [(7, 5), (8, 6), (3, 1), (4, 2)], 5)))
    return cases


def finish_minus_zero(kw, rows_not_columns):
    """Cases flagged minus_zero: entry 0 of the listed row / column is -0.0 in T0 (p = 0, so the entry of T is T0's)."""
    kw = dict(kw)
    if kw.pop("minus_zero", 0):
        if rows_not_columns:
            kw["T0"][0, kw["rows"][0]] = -0.0
            kw["T0"][1, kw["rows"][0]] = -0.0
        else:
            kw["T0"][kw["cols"][0] - kw["c_lo"], 0] = -0.0
            kw["T0"][kw["cols"][0] - kw["c_lo"], 1] = -0.0
    return kw


SUM_CASES = {False: sum_cases(False), True: sum_cases(True)}
ROW_RATIO_CASES = row_ratio_cases()
RHS_RANGING_CASES = rhs_ranging_cases()
