"""tests/cpp/test_cutpool.cpp: the host side of the cut pool (rust-lp_amd/csrc/relp_cutpool.hpp: the adapter onto the sliced-ELL
packer, the norms, the segment arithmetic of relp_cutpool_separate, the key, the argument checks) -- plain g++, no library, CPU
tier: it runs here, once as it is and once built with -fsanitize=address,undefined (a stand-alone program with its own main).
Built by tests/cpp/cutpool.mk, a line of `__graft_entry__.build()`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("binary", ["test_cutpool", "test_cutpool_asan"])
def test_the_host_side_of_the_cut_pool(binary):
    subprocess.check_call(["make", "-C", CPP, "-f", "cutpool.mk", binary], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CPP, binary)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
