"""tests/cpp/test_layout_columns.cpp: Layout::add_columns on the host (plain g++, no library) -- CPU tier, it runs here.
tests/cpp/test_columns.cpp: columns added in place through include/relp.hpp (add_columns, reserve_columns, run, objective; the
refusals) -- CPU tier: the program compiles and links against the library; GPU tier: it runs.
Both are built by tests/cpp/Makefile (`__graft_entry__.build()`)."""
import pytest

import cpp_programs


def test_layout_add_columns_on_the_host():
    cpp_programs.make_target("test_layout_columns")
    cpp_programs.run("test_layout_columns", timeout=60)


def test_cpp_columns_test_compiles_and_links():
    cpp_programs.links_against_the_library("test_columns")


@pytest.mark.gpu
def test_cpp_columns_test_passes_on_the_gpu():
    cpp_programs.make_target("test_columns", only_if_missing=True)
    cpp_programs.run("test_columns", timeout=300)
