"""The three entry points of the cut rows and added columns removed in place -- relp_remove_cuts, relp_remove_columns,
relp_removal_stats -- are declared in include/relp_engine.h, exported by the library with the argument types of the header, bound in
rust_lp_amd.engine and wrapped in include/relp.hpp (no compute calls: there is no GPU in the CPU tier); the lists a caller passes
reach the C call as int32 arrays with their count."""
import ctypes
import os
import re

import numpy as np

import rust_lp_amd  # noqa: F401
from rust_lp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_remove_cuts", "relp_remove_columns", "relp_removal_stats")
METHODS = ("remove_cuts", "remove_columns", "removal_stats")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    # the argument types of the header: (handle, const int32_t *, int32_t) twice, (const handle, int64_t *)
    assert re.search(r"relp_remove_cuts\(relp_engine_t \*h, const int32_t \*rows, int32_t count\)", header)
    assert re.search(r"relp_remove_columns\(relp_engine_t \*h, const int32_t \*columns, int32_t count\)", header)
    assert re.search(r"relp_removal_stats\(const relp_engine_t \*h, int64_t \*out4\)", header)
    for name in SYMBOLS[:2]:
        assert engine._SIGNATURES[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32])
    assert engine._SIGNATURES["relp_removal_stats"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)])


def test_python_and_cpp_wrappers_exist():
    for name in METHODS:
        assert callable(getattr(engine.Tableau, name, None)), f"engine.Tableau.{name} is missing"
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    for name, symbol in zip(METHODS, SYMBOLS):
        assert re.search(r"\b%s\s*\(" % name, hpp) and symbol in hpp, f"relp_host::Tableau::{name} is missing"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    rows = np.array([3], dtype=np.int32)
    assert lib.relp_remove_cuts(None, rows.ctypes.data, 1) == -1
    assert lib.relp_remove_columns(None, None, 0) == -1
    assert lib.relp_removal_stats(None, None) == -1


def test_the_calls_are_documented():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "removed in place" in design and "k_tab_drop_rows" in design and "k_tab_drop_columns" in design
    for text in (design, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "relp_remove_cuts" in text and "relp_remove_columns" in text
    header = open(os.path.join(ROOT, "include", "relp_engine.h")).read()
    assert "Dropping a cut is not built" not in header and "Dropping a column is not built" not in header


class _Recorder:
    """Stands in for the library: records what Tableau.remove_cuts / remove_columns hand to the C calls."""

    def __init__(self):
        self.calls = []

    def _take(self, name, p, count):
        self.calls.append((name, np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)), (count,)).copy().tolist() if count else []))
        return 0

    def relp_remove_cuts(self, h, rows, count):
        return self._take("cuts", rows, count)

    def relp_remove_columns(self, h, columns, count):
        return self._take("columns", columns, count)


def test_lists_reach_the_c_calls_as_int32_with_their_count():
    t = engine.Tableau.__new__(engine.Tableau)
    t._lib, t._h = _Recorder(), None
    t.remove_cuts([30, 28])
    t.remove_cuts(np.array([5], dtype=np.int64))
    t.remove_cuts(7)                                           # one row as a scalar
    t.remove_cuts([])
    t.remove_columns(np.arange(60, 63))
    assert t._lib.calls == [("cuts", [30, 28]), ("cuts", [5]), ("cuts", [7]), ("cuts", []), ("columns", [60, 61, 62])]
