"""tests/cpp/test_cost_in_place.cpp: the in-place cost change through include/relp.hpp (change_cost, set_cost, run, objective; the
refusals).  Built by tests/cpp/cost_in_place.mk (`__graft_entry__.build()`).  CPU tier: the program compiles and links against the
library.  GPU tier: it runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BINARY = os.path.join(CPP, "test_cost_in_place")
MAKE = ["make", "-C", CPP, "-f", "cost_in_place.mk"]         # a makefile of its own beside tests/cpp/Makefile


def test_cpp_cost_test_compiles_and_links():
    import rust_lp_amd  # noqa: F401  (builds the library when it is missing)
    from rust_lp_amd import engine
    engine.load_library()
    subprocess.check_call(MAKE, stdout=subprocess.DEVNULL)
    assert os.access(BINARY, os.X_OK)


@pytest.mark.gpu
def test_cpp_cost_test_passes_on_the_gpu():
    if not os.access(BINARY, os.X_OK):
        subprocess.check_call(MAKE, stdout=subprocess.DEVNULL)
    res = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
