"""The seven entry points of the cut pool -- relp_cutpool_create, relp_cutpool_destroy, relp_cutpool_set_active, relp_cutpool_slacks,
relp_cutpool_separate, relp_cutpool_add, relp_cutpool_stats -- are declared in include/relp_engine.h, exported by the library, bound
in rust_lp_amd.engine and wrapped in include/relp.hpp (no compute calls: there is no GPU in the CPU tier; the refusals on another
engine need a handle and stand in tests/test_gpu_cutpool.py); what Tableau.cut_pool, CutPool and engine.row_generation hand to the C
calls."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_cutpool_create", "relp_cutpool_destroy", "relp_cutpool_set_active", "relp_cutpool_slacks", "relp_cutpool_separate",
           "relp_cutpool_add", "relp_cutpool_stats")
METHODS = ("slacks", "separate", "add", "set_active", "stats", "close")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    assert re.search(r"typedef\s+struct\s+relp_cutpool\s+relp_cutpool_t\s*;", header)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    separate = engine._SIGNATURES["relp_cutpool_separate"][1]
    assert len(separate) == 8 and separate[2] is ctypes.c_int32 and separate[3] is ctypes.c_double and separate[4] is ctypes.c_int32
    assert re.search(r"relp_cutpool_separate\s*\(\s*relp_engine_t\s*\*h,\s*relp_cutpool_t\s*\*pool,\s*int32_t\s+segments,\s*double\s+tol,\s*"
                     r"int32_t\s+by_efficacy,\s*int32_t\s*\*ids_out\s*,\s*double\s*\*slack_out\s*,\s*int32_t\s*\*found\s*\)", header)
    create = engine._SIGNATURES["relp_cutpool_create"][1]
    assert len(create) == 7 and create[1] is ctypes.c_int32
    assert re.search(r"relp_cutpool_create\s*\(\s*relp_engine_t\s*\*h,\s*int32_t\s+count,\s*const\s+int64_t\s*\*row_ptr,\s*const\s+int32_t\s*"
                     r"\*col_idx,\s*const\s+double\s*\*values,\s*const\s+double\s*\*rhs,\s*relp_cutpool_t\s*\*\*pool\s*\)", header)
    assert engine._SIGNATURES["relp_cutpool_set_active"][1][3:] == [ctypes.c_int32, ctypes.c_int32]
    assert engine._SIGNATURES["relp_cutpool_add"][1][3] is ctypes.c_int32 and len(engine._SIGNATURES["relp_cutpool_slacks"][1]) == 3
    assert len(engine._SIGNATURES["relp_cutpool_stats"][1]) == 3 and len(engine._SIGNATURES["relp_cutpool_destroy"][1]) == 2


def test_python_and_cpp_wrappers_exist():
    assert callable(getattr(engine.Tableau, "cut_pool", None)) and callable(engine.row_generation)
    for name in METHODS:
        assert callable(getattr(engine.CutPool, name, None)), f"engine.CutPool.{name} is missing"
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    assert re.search(r"\bclass\s+CutPool\b", hpp) and re.search(r"\bCutPool\s+cut_pool\s*\(", hpp)
    for symbol in SYMBOLS:
        assert symbol in hpp, f"include/relp.hpp does not call {symbol}"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    assert lib.relp_cutpool_create(None, 0, None, None, None, None, None) == -1
    assert lib.relp_cutpool_destroy(None, None) == -1
    assert lib.relp_cutpool_set_active(None, None, None, 0, 1) == -1
    assert lib.relp_cutpool_slacks(None, None, None) == -1
    assert lib.relp_cutpool_separate(None, None, 1, 0.0, 0, None, None, None) == -1
    assert lib.relp_cutpool_add(None, None, None, 0) == -1
    assert lib.relp_cutpool_stats(None, None, None) == -1


def test_the_calls_are_documented():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Cut pool separated and added in place" in design and "RELP_CUTPOOL_HOST_ADD" in design
    for kernel in ("k_cutpool_x", "k_cutpool_separate", "k_cutpool_winners", "k_cutpool_entries", "k_cutpool_union", "k_cutpool_chosen"):
        assert kernel in design, f"DESIGN.md does not report {kernel}"
    for doc in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in SYMBOLS:
            assert name in text, f"{doc} does not name {name}"


class _Recorder:
    """Stands in for the library: records what the pool methods hand to the C calls."""

    def __init__(self, winners=()):
        self.calls, self.winners, self.runs = [], list(winners), 0

    @staticmethod
    def _take(p, t, n):
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(t)), (n,)).copy() if n else np.zeros(0)

    def relp_cutpool_create(self, h, count, ptr, idx, val, rhs, out):
        ptr_a = self._take(ptr, ctypes.c_int64, count + 1)
        nnz = int(ptr_a[-1])
        self.calls.append(("create", count, ptr_a, self._take(idx, ctypes.c_int32, nnz), self._take(val, ctypes.c_double, nnz),
                           self._take(rhs, ctypes.c_double, count)))
        out._obj.value = 0xC0DE
        return 0

    def relp_cutpool_destroy(self, h, p):
        self.calls.append(("destroy", p.value))
        return 0

    def relp_cutpool_set_active(self, h, p, ids, count, flag):
        self.calls.append(("set_active", self._take(ids, ctypes.c_int32, count).tolist(), flag))
        return 0

    def relp_cutpool_slacks(self, h, p, out):
        self.calls.append(("slacks",))
        return 0

    def relp_cutpool_separate(self, h, p, segments, tol, by_efficacy, ids, s, found):
        self.calls.append(("separate", segments, tol, by_efficacy))
        won = self.winners.pop(0) if self.winners else []
        np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_int32)), (max(segments, 1),))[:len(won)] = won
        np.ctypeslib.as_array(ctypes.cast(s, ctypes.POINTER(ctypes.c_double)), (max(segments, 1),))[:len(won)] = [-1.0 - k for k in won]
        found._obj.value = len(won)
        return 0

    def relp_cutpool_add(self, h, p, ids, count):
        self.calls.append(("add", self._take(ids, ctypes.c_int32, count).tolist()))
        return 0

    def relp_cutpool_stats(self, h, p, out):
        out[0], out[1], out[2], out[3] = 3, 5, 192, 2
        return 0

    def relp_run_dual(self, h, max_iters, done, outcome):
        self.runs += 1
        outcome._obj.value = engine.OPTIMAL
        return 0

    def relp_objective_function_value(self, h, out):
        out._obj.value = -42.5
        return 0

    def relp_last_error(self, h):
        return b"refused"


class _Provider:
    nr_normal = 3


def _tableau(winners=()):
    t = engine.Tableau.__new__(engine.Tableau)
    t._lib, t._h, t.provider = _Recorder(winners), 1, _Provider()
    t.objective_function_value = lambda: -42.5
    return t


def test_arguments_reach_the_c_calls():
    t = _tableau([[2, 0]])
    G = np.array([[1.0, 0.0, 3.0], [0.0, 0.0, 0.0], [0.0, -2.0, 4.0]])
    pool = t.cut_pool(G, [1.0, 2.0, 3.0])
    _, count, ptr, idx, val, rhs = t._lib.calls[-1]                     # the conversion of Tableau.add_cuts: CSR by row
    assert count == 3 == pool.count and ptr.tolist() == [0, 2, 2, 4] and idx.tolist() == [0, 2, 1, 2] and val.tolist() == [1.0, 3.0, -2.0, 4.0]
    assert rhs.tolist() == [1.0, 2.0, 3.0]
    sparse = t.cut_pool(([0, 1], [2], [5.0]), [7.0])
    assert t._lib.calls[-1][1] == 1 and t._lib.calls[-1][3].tolist() == [2] and sparse.count == 1
    with pytest.raises(ValueError):
        t.cut_pool(np.zeros((2, 2)), [1.0, 1.0])                         # not one column per structural column
    ids, s = pool.separate(segments=2, tol=0.5, by_efficacy=True)
    assert t._lib.calls[-1] == ("separate", 2, 0.5, 1) and ids.tolist() == [2, 0] and s.tolist() == [-3.0, -1.0]
    assert pool.separate()[0].shape == (0,) and t._lib.calls[-1] == ("separate", 1, 1e-7, 0)
    pool.add([2, 0])
    pool.set_active(1, False)
    pool.set_active([0, 2], True)
    assert t._lib.calls[-3:] == [("add", [2, 0]), ("set_active", [1], 0), ("set_active", [0, 2], 1)]
    assert pool.slacks().shape == (3,) and pool.stats() == (3, 5, 192, 2)
    with pytest.raises(ValueError):
        pool.add([[0, 1]])
    pool.close()
    assert t._lib.calls[-1] == ("destroy", 0xC0DE)
    pool.close()                                                         # closing twice is fine, and destroys once
    assert [c[0] for c in t._lib.calls].count("destroy") == 1
    with pytest.raises(engine.RelpError):
        pool.separate()


def test_row_generation_loops_until_nothing_is_violated():
    t = _tableau([[4, 9], [1], []])
    pool = t.cut_pool(np.zeros((12, 3)), np.ones(12))
    assert engine.row_generation(t, pool, tol=1e-9, per_round=2, max_rounds=10, by_efficacy=True) == (2, 3, -42.5)
    assert t._lib.runs == 3                                              # run_dual, separate, add; twice; run_dual, separate: nothing
    assert [c for c in t._lib.calls if c[0] in ("separate", "add")] == [("separate", 2, 1e-9, 1), ("add", [4, 9]), ("separate", 2, 1e-9, 1),
                                                                       ("add", [1]), ("separate", 2, 1e-9, 1)]
    t = _tableau([[4], [5], [6]])
    pool = t.cut_pool(np.zeros((12, 3)), np.ones(12))
    assert engine.row_generation(t, pool, max_rounds=2) == (2, 2, None)  # the cap: violated cuts are left
    t = _tableau([[0]])
    small = t.cut_pool(np.zeros((3, 3)), np.ones(3))
    engine.row_generation(t, small, per_round=50, max_rounds=1)
    assert [c for c in t._lib.calls if c[0] == "separate"][0] == ("separate", 3, 1e-7, 0)      # never more shares than cuts
