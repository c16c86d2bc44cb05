"""The three entry points of the batched ratio queries -- relp_row_ratios, relp_rhs_ranging, relp_ranging_stats -- are declared in
include/relp_engine.h, exported by the library, bound in rust_lp_amd.engine and wrapped in include/relp.hpp (no compute calls: there
is no GPU in the CPU tier)."""
import ctypes
import os
import re

import rust_lp_amd  # noqa: F401
from rust_lp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_row_ratios", "relp_rhs_ranging", "relp_ranging_stats")
METHODS = ("row_ratios", "rhs_ranging", "ranging_stats")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    for name in SYMBOLS[:2]:                                   # (handle, rows, count, ratio, index, ratio, index)
        assert len(engine._SIGNATURES[name][1]) == 7 and engine._SIGNATURES[name][1][2] is ctypes.c_int32


def test_python_and_cpp_wrappers_exist():
    for name in METHODS + ("cost_ranging",):
        assert callable(getattr(engine.Tableau, name, None)), f"engine.Tableau.{name} is missing"
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    for name, symbol in zip(METHODS, SYMBOLS):
        assert re.search(r"\b%s\s*\(" % name, hpp) and symbol in hpp, f"relp_host::Tableau::{name} is missing"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    assert lib.relp_row_ratios(None, None, 0, None, None, None, None) == -1
    assert lib.relp_rhs_ranging(None, None, 0, None, None, None, None) == -1
    assert lib.relp_ranging_stats(None, None) == -1


def test_the_calls_are_documented():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in SYMBOLS:
            assert name in text, f"{name} is not named in {doc}"
