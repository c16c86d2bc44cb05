"""tests/cpp/test_ranging.cpp: the batched ratio queries through include/relp.hpp (row_ratios, rhs_ranging, ranging_stats on one small
LP; the refusals).  Built by tests/cpp/Makefile (`__graft_entry__.build()`).  CPU tier: the program compiles and links against the
library.  GPU tier: it runs."""
import pytest

import cpp_programs


def test_cpp_ranging_test_compiles_and_links():
    cpp_programs.links_against_the_library("test_ranging")


@pytest.mark.gpu
def test_cpp_ranging_test_passes_on_the_gpu():
    cpp_programs.make_target("test_ranging", only_if_missing=True)
    cpp_programs.run("test_ranging", timeout=300)
