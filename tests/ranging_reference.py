"""The two batched ratio queries of the tableau engine -- relp_row_ratios and relp_rhs_ranging (include/relp_engine.h)
-- as a test reference over numpy f64: the tableau T = B^-1 [A | slacks], b = B^-1 rhs and d = c - c_B' T of a given basis from
`dual_reference.standard_form` and `np.linalg.solve`, the rules with the tolerances of `dual_reference.TOLERANCES`.

TEST INFRASTRUCTURE ONLY; the row kinds of dual_reference (no variable bounds, no range rows), where engine row k has the identity
column n + k when every row is a <= row.

Rules:
  row ratios, row r   candidates are the non-basic columns j; down: T[r, j] < -tol_pivot with ratio dz_j / -T[r, j], up: T[r, j] >
                      tol_pivot with ratio dz_j / T[r, j]; dz_j = 0 when d_j <= tol_zero, else d_j; the minimum ratio, and among the
                      ratios <= min + tol_tie * max(1, |min|) the lowest j
  rhs ranging, row k  a = T[:, idcol[k]]; decrease: a_i > tol_pivot with ratio bz_i / a_i, increase: a_i < -tol_pivot with ratio
                      bz_i / -a_i; bz_i = 0 when b_i <= tol_zero, else b_i; the minimum ratio, and among the ratios inside the same
                      band the row with the smallest leaving column basis[i]
Every result carries the size of its tie band and the relative gap to the runner-up, so that a test can tell the entries a device
may legitimately decide differently (band > 1, or a gap at rounding level) from the ones it must reproduce."""
from __future__ import annotations

from typing import NamedTuple, Sequence

import numpy as np

import dual_reference as dr


class Pick(NamedTuple):
    ratio: float        # the minimum, inf without a candidate
    index: int          # the column (row ratios) or the row (ranging) that wins the tie rule, -1 without a candidate
    band: int           # candidates inside the tie band of the minimum (0 without a candidate)
    gap: float          # (runner_up - ratio) / max(1, |ratio|), inf without a runner-up
    runner_up: float    # the smallest ratio outside the band, inf without one


NONE = Pick(np.inf, -1, 0, np.inf, np.inf)


def tableau(md, basis: Sequence[int]):
    """(T, b, d, in_basis) of `basis` over the columns of dual_reference.standard_form."""
    full, rhs, cost = dr.standard_form(md)
    basis = [int(j) for j in basis]
    B = full[:, basis]
    T = np.linalg.solve(B, full)
    b = np.linalg.solve(B, rhs)
    d = cost - cost[basis] @ T
    in_basis = np.zeros(full.shape[1], dtype=bool)
    in_basis[basis] = True
    return T, b, d, in_basis


def _pick(ratios: np.ndarray, keys: np.ndarray, indices: np.ndarray, tol_tie: float) -> Pick:
    """The minimum of `ratios`; inside its band the entry with the smallest key; indices = what is reported."""
    if ratios.size == 0:
        return NONE
    mn = float(ratios.min())
    inside = ratios <= mn + tol_tie * max(1.0, abs(mn))
    winner = int(indices[inside][np.argmin(keys[inside])])
    runner_up = float(ratios[~inside].min()) if (~inside).any() else np.inf
    return Pick(mn, winner, int(inside.sum()), (runner_up - mn) / max(1.0, abs(mn)), runner_up)


def row_ratios(T, d, in_basis, rows: Sequence[int], **tolerances):
    """[(down, up)] of Picks, one pair per entry of `rows`."""
    tol = dict(dr.TOLERANCES)
    tol.update(tolerances)
    dz = np.where(d <= tol["tol_zero"], 0.0, d)
    free = ~np.asarray(in_basis)
    out = []
    for r in rows:
        row = T[int(r)]
        pair = []
        for sign in (-1.0, 1.0):
            v = sign * row                              # down: the candidates are the negative entries
            cand = np.flatnonzero(free & (v > tol["tol_pivot"]))
            pair.append(_pick(dz[cand] / v[cand], cand, cand, tol["tol_tie"]))
        out.append(tuple(pair))
    return out


def rhs_ranging(T, b, basis: Sequence[int], idcol: Sequence[int], rows: Sequence[int], **tolerances):
    """[(decrease, increase)] of Picks, one pair per entry of `rows`; idcol[k] = the identity column of row k."""
    tol = dict(dr.TOLERANCES)
    tol.update(tolerances)
    bz = np.where(b <= tol["tol_zero"], 0.0, b)
    leaving = np.asarray([int(j) for j in basis])
    out = []
    for k in rows:
        a = T[:, int(idcol[int(k)])]
        pair = []
        for sign in (1.0, -1.0):
            v = sign * a
            cand = np.flatnonzero(v > tol["tol_pivot"])
            pair.append(_pick(bz[cand] / v[cand], leaving[cand], cand, tol["tol_tie"]))
        out.append(tuple(pair))
    return out
