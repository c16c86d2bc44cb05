"""tests/cpp/test_pool.cpp: the host side of the column pool (rust-lp_amd/csrc/relp_pool.hpp: the sliced-ELL packer, the segment
arithmetic of relp_pool_price, the stale rule, the argument checks) -- plain g++, no library, CPU tier: it runs here, once as it is
and once built with -fsanitize=address,undefined (a stand-alone program with its own main).  Built by tests/cpp/Makefile
(`__graft_entry__.build()`)."""
import pytest

import cpp_programs


@pytest.mark.parametrize("binary", ["test_pool", "test_pool_asan"])
def test_the_host_side_of_the_column_pool(binary):
    cpp_programs.make_target(binary)
    cpp_programs.run(binary, timeout=60)
