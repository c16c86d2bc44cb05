"""tests/cpp/test_cutpool.cpp: the host side of the cut pool (rust-lp_amd/csrc/relp_cutpool.hpp: the adapter onto the sliced-ELL
packer, the norms, the segment arithmetic of relp_cutpool_separate, the key, the argument checks) -- plain g++, no library, CPU
tier: it runs here, once as it is and once built with -fsanitize=address,undefined (a stand-alone program with its own main).
Built by tests/cpp/Makefile (`__graft_entry__.build()`)."""
import pytest

import cpp_programs


@pytest.mark.parametrize("binary", ["test_cutpool", "test_cutpool_asan"])
def test_the_host_side_of_the_cut_pool(binary):
    cpp_programs.make_target(binary)
    cpp_programs.run(binary, timeout=60)
