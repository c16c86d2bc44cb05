"""tests/cpp/test_rhs_in_place.cpp: the in-place right-hand-side change through include/relp.hpp (change, run_dual, objective; an
upper bound tightened; the refusals).  Built by tests/cpp/Makefile (`__graft_entry__.build()`).  CPU tier: the program compiles and
links against the library.  GPU tier: it runs."""
import pytest

import cpp_programs


def test_cpp_rhs_test_compiles_and_links():
    cpp_programs.links_against_the_library("test_rhs_in_place")


@pytest.mark.gpu
def test_cpp_rhs_test_passes_on_the_gpu():
    cpp_programs.make_target("test_rhs_in_place", only_if_missing=True)
    cpp_programs.run("test_rhs_in_place", timeout=300)
