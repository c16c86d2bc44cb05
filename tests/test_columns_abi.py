"""The three entry points of the columns added in place -- relp_add_columns, relp_reserve_columns, relp_column_stats -- are declared
in include/relp_engine.h, exported by the library, bound in rust_lp_amd.engine and wrapped in include/relp.hpp (no compute calls:
there is no GPU in the CPU tier); the conversion of a dense block, a vector or a CSC triple into the CSC the C call takes, and the
numpy reference of the GPU tests on a basis known by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import rust_lp_amd  # noqa: F401
from rust_lp_amd import MatrixData, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("relp_add_columns", "relp_reserve_columns", "relp_column_stats")
METHODS = ("add_columns", "reserve_columns", "column_stats")


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "relp_engine.h")).read(), flags=re.S)
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in relp_engine.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine._SIGNATURES, f"{name} has no ctypes signature"
    assert engine._SIGNATURES["relp_add_columns"][1][1] is ctypes.c_int32 and len(engine._SIGNATURES["relp_add_columns"][1]) == 6
    assert engine._SIGNATURES["relp_reserve_columns"][1] == [ctypes.c_void_p, ctypes.c_int32]


def test_python_and_cpp_wrappers_exist():
    for name in METHODS:
        assert callable(getattr(engine.Tableau, name, None)), f"engine.Tableau.{name} is missing"
    hpp = open(os.path.join(ROOT, "include", "relp.hpp")).read()
    for name, symbol in zip(METHODS, SYMBOLS):
        assert re.search(r"\b%s\s*\(" % name, hpp) and symbol in hpp, f"relp_host::Tableau::{name} is missing"


def test_null_handles_are_rejected_not_crashing():
    lib = engine.load_library()
    assert lib.relp_add_columns(None, 0, None, None, None, None) == -1
    assert lib.relp_reserve_columns(None, 4) == -1
    assert lib.relp_column_stats(None, None) == -1


def test_the_calls_are_documented():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Columns added in place" in design and "k_tab_col_apply" in design and "k_tab_col_tail" in design
    for text in (design, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "relp_add_columns" in text
    header = open(os.path.join(ROOT, "include", "relp_engine.h")).read()
    for name in SYMBOLS:
        assert name in header
    assert "coefficient 0 on every added column" in header


class _Recorder:
    """Stands in for the library: records what Tableau.add_columns hands to relp_add_columns."""

    def __init__(self, rows):
        self.calls, self.rows = [], rows

    def relp_nr_rows(self, h):
        return self.rows

    def relp_add_columns(self, h, count, ptr, idx, val, cost):
        nnz = int(np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int64)), (count + 1,))[-1]) if count else 0
        take = lambda p, t, n: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(t)), (n,)).copy() if n else np.zeros(0)   # noqa: E731
        self.calls.append((count, take(ptr, ctypes.c_int64, count + 1), take(idx, ctypes.c_int32, nnz), take(val, ctypes.c_double, nnz),
                           take(cost, ctypes.c_double, count)))
        return 0


def _tableau_without_a_handle(rows):
    t = engine.Tableau.__new__(engine.Tableau)
    t._lib, t._h = _Recorder(rows), None
    return t


def test_dense_vector_and_csc_arguments_reach_the_c_call_as_csc():
    t = _tableau_without_a_handle(4)
    A = np.array([[0.0, 1.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    t.add_columns(A, [5.0, 6.0, 7.0])
    count, ptr, idx, val, cost = t._lib.calls[-1]
    assert count == 3 and ptr.tolist() == [0, 2, 3, 3] and idx.tolist() == [1, 3, 0] and val.tolist() == [2.0, 3.0, 1.0]
    assert cost.tolist() == [5.0, 6.0, 7.0]
    t.add_columns(([0, 2], [3, 1], [3.0, 2.0]), [5.0])         # a CSC triple goes through as it is
    count, ptr, idx, val, cost = t._lib.calls[-1]
    assert count == 1 and ptr.tolist() == [0, 2] and idx.tolist() == [3, 1] and val.tolist() == [3.0, 2.0]
    t.add_columns(np.array([1.0, 0.0, 0.0, 2.0]), 4.0)         # one column as a vector and a scalar
    assert t._lib.calls[-1][0] == 1 and t._lib.calls[-1][2].tolist() == [0, 3] and t._lib.calls[-1][4].tolist() == [4.0]
    t.add_columns(np.zeros((4, 0)), np.zeros(0))               # no column
    assert t._lib.calls[-1][0] == 0
    for bad in (lambda: t.add_columns(np.ones((3, 2)), [1.0, 2.0]), lambda: t.add_columns(A, [1.0]), lambda: t.add_columns(([0, 1], [0]), [1.0]),
                lambda: t.add_columns(([0, 5], [0], [1.0]), [1.0]), lambda: t.add_columns(np.ones(3), 1.0)):
        with pytest.raises(ValueError):
            bad()


def test_the_numpy_reference_on_a_basis_known_by_hand():
    """column_reference on min -x1 - 2 x2, x1 + x2 <= 3, x2 <= 2 at the optimum basis (x1, x2) = (1, 2), -pi = (1, 1), with the new
    column (1, 2)' of cost -4: B^-1 a = (-1, 2)', d = -4 + 1 + 2 = -1, everything over the old columns as it was.  Engine order
    [x1, x2 | s1, s2 | x3], wide order [x1, x2, x3 | s1, s2]."""
    import column_reference as colref
    lp = dict(A=np.asfortranarray([[1.0, 1.0, 1.0], [0.0, 1.0, 2.0]]), b=np.array([3.0, 2.0]), c=np.array([-1.0, -2.0, -4.0]))
    md0 = colref.narrow(lp, 2)
    assert md0.nr_normal == 2 and md0.nr_le == 2
    A_new, cost = colref.new_columns(lp, 2)
    assert A_new.tolist() == [[1.0], [2.0]] and cost.tolist() == [-4.0]
    md2 = colref.wide(lp, 2, A_new, None)
    assert md2.nr_normal == 3 and isinstance(md2, MatrixData)
    assert colref.to_wide([0, 1, 2, 3, 4], 2, 2, 1).tolist() == [0, 1, 3, 4, 2]
    assert colref.to_engine([0, 1, 2, 3, 4], 2, 2, 1).tolist() == [0, 1, 4, 2, 3]
    ref = colref.Tableau(md2, [0, 1], 2, 2, 1)
    assert np.allclose(ref.T[:, 4], [-1, 2]) and np.allclose(ref.b, [1, 2]) and np.allclose(ref.d, [0, 0, 1, 1, -1])
    assert np.allclose(ref.minus_pi, [1, 1]) and abs(ref.objective + 5) < 1e-12
    sparse, _ = colref.new_columns(dict(A=np.ones((8, 6)), c=np.zeros(6)), 3, sparse=True)
    assert sparse.shape == (8, 3) and sparse[:, 1].tolist() == [0, 1, 0, 0, 0, 1, 0, 0]
