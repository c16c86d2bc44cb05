"""tests/cpp/test_gomory.cpp: the host side of relp_gomory_cuts that needs no device (rust-lp_amd/csrc/relp_gomory.hpp: the argument
checks, the statuses decided per entry, the slack rows of a Layout, the beta chain) -- plain g++, no library, CPU tier: it runs here,
once as it is and once built with -fsanitize=address,undefined (a stand-alone program with its own main).
Built by tests/cpp/Makefile (`__graft_entry__.build()`)."""
import pytest

import cpp_programs


@pytest.mark.parametrize("binary", ["test_gomory", "test_gomory_asan"])
def test_the_host_side_of_gomory_cuts(binary):
    cpp_programs.make_target(binary)
    cpp_programs.run(binary, timeout=60)
