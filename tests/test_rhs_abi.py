"""The four entry points of the in-place right-hand-side change -- relp_change_right_hand_side, relp_set_upper_bound,
relp_get_right_hand_side, relp_rhs_stats -- are declared in include/relp_engine.h, exported by the library, bound in
rust_lp_amd.engine and wrapped in include/relp.hpp (no compute calls: there is no GPU in the CPU tier)."""
import ctypes
import os
import re

import rust_lp_amd  # noqa: F401
from rust_lp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_change_right_hand_side", "relp_set_upper_bound", "relp_get_right_hand_side", "relp_rhs_stats")
METHODS = ("change_right_hand_side", "set_upper_bound", "right_hand_side", "rhs_stats")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    assert engine._SIGNATURES["relp_change_right_hand_side"][1][-1] is ctypes.c_int32
    assert engine._SIGNATURES["relp_set_upper_bound"][1][1:] == [ctypes.c_int32, ctypes.c_double]


def test_python_and_cpp_wrappers_exist():
    for name in METHODS:
        assert callable(getattr(engine.Tableau, name, None)), f"engine.Tableau.{name} is missing"
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    for name, symbol in zip(METHODS, SYMBOLS):
        assert re.search(r"\b%s\s*\(" % name, hpp) and symbol in hpp, f"relp_host::Tableau::{name} is missing"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    assert lib.relp_change_right_hand_side(None, None, None, 0) == -1
    assert lib.relp_set_upper_bound(None, 0, 1.0) == -1
    assert lib.relp_get_right_hand_side(None, None) == -1
    assert lib.relp_rhs_stats(None, None) == -1


def test_the_switch_and_the_calls_are_documented():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "RELP_TAB_RHS_SPLITS" in design
    for text in (design, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "relp_change_right_hand_side" in text
