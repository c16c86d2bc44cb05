"""tests/cpp/test_layout_remove.cpp: Layout::remove_cuts / remove_columns on the host (plain g++, no library) -- CPU tier, it runs
here.  tests/cpp/test_remove.cpp: cut rows and added columns removed in place through include/relp.hpp (remove_cuts, remove_columns,
removal_stats; the refusals) -- CPU tier: the program compiles and links against the library; GPU tier: it runs.
Both are built by tests/cpp/Makefile (`__graft_entry__.build()`)."""
import pytest

import cpp_programs


def test_layout_remove_on_the_host():
    cpp_programs.make_target("test_layout_remove")
    cpp_programs.run("test_layout_remove", timeout=60)


def test_cpp_remove_test_compiles_and_links():
    cpp_programs.links_against_the_library("test_remove")


@pytest.mark.gpu
def test_cpp_remove_test_passes_on_the_gpu():
    cpp_programs.make_target("test_remove", only_if_missing=True)
    cpp_programs.run("test_remove", timeout=300)
