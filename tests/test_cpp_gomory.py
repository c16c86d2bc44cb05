"""tests/cpp/test_gomory.cpp: the host side of relp_gomory_cuts that needs no device (rust-lp_amd/csrc/relp_gomory.hpp: the argument
checks, the statuses decided per entry, the slack rows of a Layout, the beta chain) -- plain g++, no library, CPU tier: it runs here,
once as it is and once built with -fsanitize=address,undefined (a stand-alone program with its own main).  Built by
tests/cpp/gomory.mk, a line of `__graft_entry__.build()`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("binary", ["test_gomory", "test_gomory_asan"])
def test_the_host_side_of_gomory_cuts(binary):
    subprocess.check_call(["make", "-C", CPP, "-f", "gomory.mk", binary], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CPP, binary)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
