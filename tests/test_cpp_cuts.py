"""tests/cpp/test_layout_cuts.cpp: Layout::add_cuts on the host (plain g++, no library) -- CPU tier, it runs here.
tests/cpp/test_cuts.cpp: cut rows added in place through include/relp.hpp (add_cuts, reserve_cuts, run_dual, objective; the
refusals) -- CPU tier: the program compiles and links against the library; GPU tier: it runs.
Both are built by tests/cpp/Makefile (`__graft_entry__.build()`)."""
import pytest

import cpp_programs


def test_layout_add_cuts_on_the_host():
    cpp_programs.make_target("test_layout_cuts")
    cpp_programs.run("test_layout_cuts", timeout=60)


def test_cpp_cuts_test_compiles_and_links():
    cpp_programs.links_against_the_library("test_cuts")


@pytest.mark.gpu
def test_cpp_cuts_test_passes_on_the_gpu():
    cpp_programs.make_target("test_cuts", only_if_missing=True)
    cpp_programs.run("test_cuts", timeout=300)
