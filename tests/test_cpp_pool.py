"""tests/cpp/test_pool.cpp: the host side of the column pool (rust-lp_amd/csrc/relp_pool.hpp: the sliced-ELL packer, the segment
arithmetic of relp_pool_price, the stale rule, the argument checks) -- plain g++, no library, CPU tier: it runs here, once as it is
and once built with -fsanitize=address,undefined (a stand-alone program with its own main).  Built by tests/cpp/pool.mk, a line of
`__graft_entry__.build()`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("binary", ["test_pool", "test_pool_asan"])
def test_the_host_side_of_the_column_pool(binary):
    subprocess.check_call(["make", "-C", CPP, "-f", "pool.mk", binary], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CPP, binary)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
