"""The seven entry points of the column pool -- relp_pool_create, relp_pool_destroy, relp_pool_set_active, relp_pool_reduced_costs,
relp_pool_price, relp_pool_add, relp_pool_stats -- are declared in include/relp_engine.h, exported by the library, bound in
rust_lp_amd.engine and wrapped in include/relp.hpp (no compute calls: there is no GPU in the CPU tier); what Tableau.pool, ColumnPool
and engine.column_generation hand to the C calls."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_pool_create", "relp_pool_destroy", "relp_pool_set_active", "relp_pool_reduced_costs", "relp_pool_price", "relp_pool_add",
           "relp_pool_stats")
METHODS = ("reduced_costs", "price", "add", "set_active", "stats", "close")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    assert re.search(r"typedef\s+struct\s+relp_pool\s+relp_pool_t\s*;", header)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    price = engine._SIGNATURES["relp_pool_price"][1]
    assert len(price) == 7 and price[2] is ctypes.c_int32 and price[3] is ctypes.c_double
    assert len(engine._SIGNATURES["relp_pool_create"][1]) == 7 and engine._SIGNATURES["relp_pool_create"][1][1] is ctypes.c_int32
    assert engine._SIGNATURES["relp_pool_set_active"][1][3:] == [ctypes.c_int32, ctypes.c_int32]
    assert engine._SIGNATURES["relp_pool_add"][1][3] is ctypes.c_int32


def test_python_and_cpp_wrappers_exist():
    assert callable(getattr(engine.Tableau, "pool", None)) and callable(engine.column_generation)
    for name in METHODS:
        assert callable(getattr(engine.ColumnPool, name, None)), f"engine.ColumnPool.{name} is missing"
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    assert re.search(r"\bclass\s+Pool\b", hpp) and re.search(r"\bPool\s+pool\s*\(", hpp)
    for symbol in SYMBOLS:
        assert symbol in hpp, f"include/relp.hpp does not call {symbol}"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    assert lib.relp_pool_create(None, 0, None, None, None, None, None) == -1
    assert lib.relp_pool_destroy(None, None) == -1
    assert lib.relp_pool_set_active(None, None, None, 0, 1) == -1
    assert lib.relp_pool_reduced_costs(None, None, None) == -1
    assert lib.relp_pool_price(None, None, 1, 0.0, None, None, None) == -1
    assert lib.relp_pool_add(None, None, None, 0) == -1
    assert lib.relp_pool_stats(None, None, None) == -1


def test_the_calls_are_documented():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Column pool priced and added in place" in design and "RELP_POOL_HOST_ADD" in design
    for kernel in ("k_pool_price", "k_pool_winners", "k_pool_entries", "k_pool_union", "k_pool_chosen"):
        assert kernel in design, f"DESIGN.md does not report {kernel}"
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
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

    def relp_pool_create(self, h, count, ptr, idx, val, cost, out):
        ptr_a = self._take(ptr, ctypes.c_int64, count + 1)
        nnz = int(ptr_a[-1])
        self.calls.append(("create", count, ptr_a, self._take(idx, ctypes.c_int32, nnz), self._take(val, ctypes.c_double, nnz),
                           self._take(cost, ctypes.c_double, count)))
        out._obj.value = 0xBEEF
        return 0

    def relp_pool_destroy(self, h, p):
        self.calls.append(("destroy", p.value))
        return 0

    def relp_pool_set_active(self, h, p, ids, count, flag):
        self.calls.append(("set_active", self._take(ids, ctypes.c_int32, count).tolist(), flag))
        return 0

    def relp_pool_reduced_costs(self, h, p, out):
        self.calls.append(("reduced_costs",))
        return 0

    def relp_pool_price(self, h, p, segments, tol, ids, d, found):
        self.calls.append(("price", segments, tol))
        won = self.winners.pop(0) if self.winners else []
        np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_int32)), (max(segments, 1),))[:len(won)] = won
        np.ctypeslib.as_array(ctypes.cast(d, ctypes.POINTER(ctypes.c_double)), (max(segments, 1),))[:len(won)] = [-1.0 - k for k in won]
        found._obj.value = len(won)
        return 0

    def relp_pool_add(self, h, p, ids, count):
        self.calls.append(("add", self._take(ids, ctypes.c_int32, count).tolist()))
        return 0

    def relp_pool_stats(self, h, p, out):
        out[0], out[1], out[2], out[3] = 3, 5, 192, 2
        return 0

    def relp_run(self, h, max_iters, done, outcome):
        self.runs += 1
        outcome._obj.value = engine.OPTIMAL
        return 0

    def relp_nr_rows(self, h):
        return 3

    def relp_last_error(self, h):
        return b"refused"


def _tableau(winners=()):
    t = engine.Tableau.__new__(engine.Tableau)
    t._lib, t._h = _Recorder(winners), 1
    return t


def test_arguments_reach_the_c_calls():
    t = _tableau([[2, 0]])
    A = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -2.0], [3.0, 0.0, 4.0]])
    pool = t.pool(A, [1.0, 2.0, 3.0])
    _, count, ptr, idx, val, cost = t._lib.calls[-1]                    # the conversion of Tableau.add_columns: CSC by column
    assert count == 3 == pool.count and ptr.tolist() == [0, 2, 2, 4] and idx.tolist() == [0, 2, 1, 2] and val.tolist() == [1.0, 3.0, -2.0, 4.0]
    assert cost.tolist() == [1.0, 2.0, 3.0]
    sparse = t.pool(([0, 1], [2], [5.0]), [7.0])
    assert t._lib.calls[-1][1] == 1 and t._lib.calls[-1][3].tolist() == [2] and sparse.count == 1
    with pytest.raises(ValueError):
        t.pool(np.zeros((2, 2)), [1.0, 1.0])                             # not one row per engine row
    ids, d = pool.price(segments=2, tol=0.5)
    assert t._lib.calls[-1] == ("price", 2, 0.5) and ids.tolist() == [2, 0] and d.tolist() == [-3.0, -1.0]
    assert pool.price()[0].shape == (0,) and t._lib.calls[-1] == ("price", 1, 1e-7)
    pool.add([2, 0])
    pool.set_active(1, False)
    pool.set_active([0, 2], True)
    assert t._lib.calls[-3:] == [("add", [2, 0]), ("set_active", [1], 0), ("set_active", [0, 2], 1)]
    assert pool.reduced_costs().shape == (3,) and pool.stats() == (3, 5, 192, 2)
    with pytest.raises(ValueError):
        pool.add([[0, 1]])
    pool.close()
    assert t._lib.calls[-1] == ("destroy", 0xBEEF)
    pool.close()                                                         # closing twice is fine, and destroys once
    assert [c[0] for c in t._lib.calls].count("destroy") == 1
    with pytest.raises(engine.RelpError):
        pool.price()


def test_column_generation_loops_until_nothing_prices_out():
    t = _tableau([[4, 9], [1], []])
    pool = t.pool(np.zeros((3, 12)), np.ones(12))
    assert engine.column_generation(t, pool, segments=2, tol=1e-9, max_rounds=10) == (2, 3, engine.OPTIMAL)
    assert t._lib.runs == 3                                              # run, price, add; run, price, add; run, price: nothing
    assert [c for c in t._lib.calls if c[0] in ("price", "add")] == [("price", 2, 1e-9), ("add", [4, 9]), ("price", 2, 1e-9), ("add", [1]),
                                                                    ("price", 2, 1e-9)]
    t = _tableau([[4], [5], [6]])
    pool = t.pool(np.zeros((3, 12)), np.ones(12))
    assert engine.column_generation(t, pool, max_rounds=2) == (2, 2, engine.RUNNING)     # the cap: candidates are left
