"""The two entry points of the Gomory cuts -- relp_gomory_cuts, relp_gomory_stats -- are declared in include/relp_engine.h, exported
by the library, bound in rust_lp_amd.engine and wrapped in include/relp.hpp (no compute calls: there is no GPU in the CPU tier);
what Tableau.gomory_cuts hands to the C call; and the reference of the GPU tests on a cut known by hand."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_gomory_cuts", "relp_gomory_stats")
METHODS = ("gomory_cuts", "gomory_stats")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    args = engine._SIGNATURES["relp_gomory_cuts"][1]
    assert len(args) == 10 and args[2] is ctypes.c_int32 and args[4] is ctypes.c_int32 and args[5] is ctypes.c_double
    assert re.search(r"RELP_GOMORY_FRACTIONAL\s*=\s*0", header) and re.search(r"RELP_GOMORY_MIXED\s*=\s*1", header)
    assert (engine.GOMORY_FRACTIONAL, engine.GOMORY_MIXED) == (0, 1)


def test_python_and_cpp_wrappers_exist():
    for name in METHODS:
        assert callable(getattr(engine.Tableau, name, None)), f"engine.Tableau.{name} is missing"
    assert callable(engine.gomory_rounds)
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    for name, symbol in zip(METHODS, SYMBOLS):
        assert re.search(r"\b%s\s*\(" % name, hpp) and symbol in hpp, f"relp_host::Tableau::{name} is missing"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    assert lib.relp_gomory_cuts(None, None, 0, None, 0, 0.0, None, None, None, None) == -1
    assert lib.relp_gomory_stats(None, None) == -1


def test_the_calls_are_documented():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Gomory cuts from tableau rows" in design and "k_tab_gomory_rows" in design and "k_tab_gomory_structural" in design
    for text in (design, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "relp_gomory_cuts" in text


class _Recorder:
    """Stands in for the library: records what Tableau.gomory_cuts hands to relp_gomory_cuts."""

    def __init__(self):
        self.calls = []

    def relp_gomory_cuts(self, h, rows, count, flags, kind, away, coef, rhs, fraction, status):
        take = lambda p, t, n: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(t)), (n,)).copy()   # noqa: E731
        self.calls.append((take(rows, ctypes.c_int32, count) if count else np.zeros(0), None if flags is None else take(flags, ctypes.c_uint8, 6),
                           kind, away))
        np.ctypeslib.as_array(ctypes.cast(status, ctypes.POINTER(ctypes.c_int32)), (max(count, 1),))[:count] = 0
        return 0


def test_arguments_reach_the_c_call():
    t = engine.Tableau.__new__(engine.Tableau)
    t._lib, t._h = _Recorder(), None
    t.provider = type("P", (), {"nr_normal": 4})()
    t.nr_columns = lambda: 6
    G, rhs, fraction, status = t.gomory_cuts([2, 0, 2])
    assert G.shape == (3, 4) and rhs.shape == fraction.shape == status.shape == (3,) and status.tolist() == [0, 0, 0]
    rows, flags, kind, away = t._lib.calls[-1]
    assert rows.tolist() == [2, 0, 2] and flags is None and kind == 0 and away == 1e-6
    t.gomory_cuts([1], is_integer=[1, 1, 0, 0, 5, 0], kind=engine.GOMORY_MIXED, away=0.01)
    rows, flags, kind, away = t._lib.calls[-1]
    assert flags.tolist() == [1, 1, 0, 0, 1, 0] and kind == 1 and away == 0.01
    with pytest.raises(ValueError):
        t.gomory_cuts([[0, 1]])
    with pytest.raises(ValueError):
        t.gomory_cuts([0], is_integer=[1, 1])


def test_the_reference_on_a_cut_known_by_hand():
    """max x2, 3 x1 + 2 x2 <= 6, -3 x1 + 2 x2 <= 0 (the textbook example): the optimum is (1, 3/2); the row of x2 reads
    x2 + s1/4 + s2/4 = 3/2, so the cut is s1/4 + s2/4 >= 1/2, in structural space x2 <= 1."""
    import gomory_reference as gr
    lp = gr.LP([[3, 2], [-3, 2]], [6, 0], [0, -1], 0, 2, 0, exact=True)
    basis = gr.optimal_basis(lp)
    assert sorted(basis) == [0, 1]
    T, b, _ = lp.tableau(basis)
    r = basis.index(1)
    assert b[r] == Fraction(3, 2)
    g, beta, f0, status = gr.cut(lp, T[r], b[r], 1, [True, True, False, False])
    assert status == gr.CUT and f0 == Fraction(1, 2)
    assert g == [0, Fraction(1)] and beta == 1
    lpf = gr.LP([[3, 2], [-3, 2]], [6, 0], [0, -1], 0, 2, 0)
    Tf, bf, _ = lpf.tableau(basis)
    gf, betaf, f0f, _ = gr.cut(lpf, Tf[r], bf[r], 1, [True, True, False, False])
    assert np.allclose(gf, [0, 1]) and abs(betaf - 1) < 1e-12 and abs(f0f - 0.5) < 1e-12
