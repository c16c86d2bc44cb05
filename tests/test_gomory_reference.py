"""tests/gomory_reference.py against brute force (CPU tier): on small integer programs every Gomory cut of every round keeps every
integer feasible point and cuts the vertex it was made at off by exactly f0 (over Fractions), the objective never improves from
round to round, and the rounds end at the enumerated integer optimum -- over Fractions inside the cap of 20 rounds at 3 cuts per
round, and over f64 at the same optimum.

Instances: 4 columns x 3 rows, max c'x, A x <= b, x >= 0 integer, coefficients in 1..9, rhs in 15..40, drawn with random.seed(7) (A
row by row, then b, then c, twelve in a row); six of them are used.  BOUNDED adds a >= row (sigma = -1) and two upper bounds (the
bound-row term).  The mixed cuts are checked for validity on sampled mixed points and for the violation f0; no convergence claim."""
from __future__ import annotations

import math
import random
from fractions import Fraction

import numpy as np
import pytest

import gomory_reference as gr

CAP, PER_ROUND = 20, 3
USED = (1, 2, 4, 5, 10, 11)


def drawn():
    random.seed(7)
    out = []
    for _ in range(12):
        A = [[random.randint(1, 9) for _ in range(4)] for _ in range(3)]
        b = [random.randint(15, 40) for _ in range(3)]
        c = [random.randint(1, 9) for _ in range(4)]
        out.append(dict(A=A, b=b, c=c, nr_eq=0, nr_le=3, nr_ge=0, upper=None, box=40))
    return out


BOUNDED = dict(A=[[3, 5, 2, 7], [6, 2, 8, 3], [1, 2, 1, 3]], b=[31, 37, 6], c=[5, -2, 6, -3], nr_eq=0, nr_le=2, nr_ge=1,
               upper=[3, math.inf, 2, math.inf], box=19)
INSTANCES = {f"seed7_{k}": inst for k, inst in enumerate(drawn()) if k in USED}
INSTANCES["bounded"] = BOUNDED


def make(inst, exact):
    return gr.LP(inst["A"], inst["b"], [-v for v in inst["c"]], inst["nr_eq"], inst["nr_le"], inst["nr_ge"], inst["upper"], exact=exact)


def points_of(inst):
    return gr.integer_points(inst["A"], inst["b"], inst["nr_eq"], inst["nr_le"], inst["nr_ge"], inst["upper"], inst["box"])


_cache = {}


def solved(name):
    """(integer feasible points, integer optimum of max c'x, optimal basis, exact rounds, f64 rounds), computed once."""
    if name not in _cache:
        inst = INSTANCES[name]
        pts = points_of(inst)
        best = max(int(np.dot(p, inst["c"])) for p in pts)
        lp = make(inst, True)
        basis = gr.optimal_basis(lp)
        assert basis is not None
        exact = gr.rounds(lp, basis, max_rounds=CAP + 1, cuts_per_round=PER_ROUND)
        f64 = gr.rounds(make(inst, False), basis, max_rounds=CAP + 1, cuts_per_round=PER_ROUND)
        _cache[name] = (pts, best, basis, exact, f64, lp)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_cuts_keep_every_integer_point_and_cut_off_the_vertex(name):
    pts, _, _, exact, _, _ = solved(name)
    assert exact, "the LP optimum is fractional on every instance"
    for rnd in exact:
        for g, beta, f0 in rnd.cuts:
            assert 0 < f0 < 1
            assert sum(gc * xc for gc, xc in zip(g, rnd.vertex)) - beta == f0          # violated by exactly f0
            for p in pts:
                assert sum(gc * int(xc) for gc, xc in zip(g, p)) <= beta, (name, p.tolist())


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_rounds_end_at_the_integer_optimum(name):
    _, best, basis, exact, f64, lp = solved(name)
    assert len(exact) <= CAP, "the Fraction reference must stay inside the cap"
    objectives = [r.objective for r in exact]
    assert all(o is not None for o in objectives)
    fresh = make(INSTANCES[name], True)                # (lp has grown by the cuts)
    start = fresh.objective(basis, fresh.tableau(basis)[1])
    for before, after in zip([start] + objectives, objectives):
        assert after >= before                         # the engine minimises -c'x: the objective never improves
    assert objectives[-1] == -best
    assert len(f64) <= CAP and f64[-1].objective is not None
    assert abs(f64[-1].objective + best) <= 1e-9 * max(1, abs(best))
    fo = [r.objective for r in f64]
    assert all(b >= a - 1e-9 for a, b in zip(fo, fo[1:]))


def test_statuses_and_skips():
    lp = make(INSTANCES["seed7_1"], True)
    basis = gr.optimal_basis(lp)
    T, b, _ = lp.tableau(basis)
    in_basis = [j in basis for j in range(lp.ncol)]
    r = next(i for i in range(lp.m) if b[i] != math.floor(b[i]))
    flags = [True] * lp.ncol
    flags[basis[r]] = False
    assert gr.cut(lp, T[r], b[r], basis[r], in_basis, flags)[3] == gr.NOT_INTEGER
    assert gr.cut(lp, T[r], Fraction(3), basis[r], in_basis)[3] == gr.FRACTION
    assert gr.cut(lp, T[r], b[r], basis[r], in_basis, away=0.4999999)[3] in (gr.FRACTION, gr.CUT)
    cont = [True] * lp.ncol
    j = next(j for j in range(lp.ncol) if not in_basis[j] and T[r][j] != 0)
    cont[j] = False
    g, beta, f0, status = gr.cut(lp, T[r], b[r], basis[r], in_basis, cont)
    assert status == gr.CONTINUOUS and all(v == 0 for v in g) and beta == 0 and f0 == b[r] - math.floor(b[r])
    assert gr.cut(lp, T[r], b[r], basis[r], in_basis, cont, kind=gr.MIXED)[3] == gr.CUT


@pytest.mark.parametrize("name", ["seed7_2", "seed7_4", "bounded"])
def test_mixed_cuts_hold_on_sampled_mixed_points(name):
    """Columns 0 and 1 integer, everything else (the slacks too) continuous: every mixed cut of the fractional rows of the optimum
    holds at every sampled mixed feasible point and is violated at the vertex by f0."""
    inst = INSTANCES[name]
    lp = make(inst, True)
    basis = gr.optimal_basis(lp)
    T, b, _ = lp.tableau(basis)
    in_basis = [j in basis for j in range(lp.ncol)]
    flags = [j < 2 for j in range(lp.ncol)]
    vertex = gr.vertex_of(lp, basis, b)
    cuts = []
    for r in range(lp.m):
        g, beta, f0, status = gr.cut(lp, T[r], b[r], basis[r], in_basis, flags, kind=gr.MIXED)
        if status == gr.CUT:
            assert sum(gc * xc for gc, xc in zip(g, vertex)) - beta == f0
            cuts.append((g, beta))
    rng = random.Random(11)
    A, rhs = inst["A"], inst["b"]
    upper = inst["upper"] or [math.inf] * 4
    kept = 0
    for x0 in range(0, 13):
        for x1 in range(0, 13):
            for _ in range(12):
                x = [Fraction(x0), Fraction(x1), Fraction(0), Fraction(0)]
                if x0 > upper[0] or x1 > upper[1]:
                    continue
                le = range(inst["nr_eq"], inst["nr_eq"] + inst["nr_le"])
                for c in (2, 3):                       # the continuous part: a 16th of what the <= rows and the bound leave
                    room = [(rhs[i] - sum(Fraction(a) * xc for a, xc in zip(A[i], x))) / A[i][c] for i in le]
                    if math.isfinite(upper[c]):
                        room.append(Fraction(upper[c]))
                    x[c] = max(Fraction(0), min(room)) * Fraction(rng.randint(0, 16), 16)
                v = [sum(Fraction(a) * xc for a, xc in zip(row, x)) for row in A]
                ok = all((v[i] == rhs[i]) if i < inst["nr_eq"] else (v[i] <= rhs[i]) if i < inst["nr_eq"] + inst["nr_le"] else (v[i] >= rhs[i])
                         for i in range(len(A)))
                if not ok:
                    continue
                kept += 1
                for g, beta in cuts:
                    assert sum(gc * xc for gc, xc in zip(g, x)) <= beta, (name, x)
    assert kept >= 50
