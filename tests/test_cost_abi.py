"""The four entry points of the in-place cost change -- relp_change_cost, relp_set_cost, relp_get_cost, relp_cost_stats -- are
declared in include/relp_engine.h, exported by the library, bound in rust_lp_amd.engine and wrapped in include/relp.hpp (no compute
calls: there is no GPU in the CPU tier)."""
import ctypes
import os
import re

import rust_lp_amd  # noqa: F401
from rust_lp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_change_cost", "relp_set_cost", "relp_get_cost", "relp_cost_stats")
METHODS = ("change_cost", "set_cost", "cost", "cost_stats")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    assert engine._SIGNATURES["relp_change_cost"][1][-1] is ctypes.c_int32
    assert len(engine._SIGNATURES["relp_set_cost"][1]) == 2 and len(engine._SIGNATURES["relp_get_cost"][1]) == 2


def test_python_and_cpp_wrappers_exist():
    for name in METHODS:
        assert callable(getattr(engine.Tableau, name, None)), f"engine.Tableau.{name} is missing"
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    for name, symbol in zip(METHODS, SYMBOLS):
        assert re.search(r"\b%s\s*\(" % name, hpp) and symbol in hpp, f"relp_host::Tableau::{name} is missing"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    assert lib.relp_change_cost(None, None, None, 0) == -1
    assert lib.relp_set_cost(None, None) == -1
    assert lib.relp_get_cost(None, None) == -1
    assert lib.relp_cost_stats(None, None) == -1


def test_the_switch_and_the_calls_are_documented():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "RELP_TAB_COST_SPLITS" in design
    for text in (design, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "relp_change_cost" in text


def test_the_numpy_reference_on_a_basis_known_by_hand():
    """cost_reference on min -x1 - 2 x2, x1 + x2 <= 3, x2 <= 2 at the basis (x1, x2): pi = (-1, -1), d = (0, 0, 1, 1), objective -5."""
    import numpy as np
    import cost_reference as cr
    from rust_lp_amd import MatrixData
    md = MatrixData.from_dense_le(np.asfortranarray([[1.0, 1.0], [0.0, 1.0]]), np.array([3.0, 2.0]), np.array([-1.0, -1.0]))
    d, minus_pi, objective = cr.reduced_costs(md, [0, 1], [-1.0, -2.0])
    assert np.allclose(d, [0, 0, 1, 1]) and np.allclose(minus_pi, [1, 1]) and abs(objective + 5) < 1e-12
    assert np.allclose(cr.tableau_row(md, [0, 1], 0), [1, 0, 1, -1])
    assert cr.primal_pivots(md, [2, 3], [-1.0, -2.0]) == 2
