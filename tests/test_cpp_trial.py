"""tests/cpp/test_trial.cpp: the planner of the trial snapshot (rust-lp_amd/csrc/relp_trial.hpp: 16-byte-aligned offsets, no overlap,
the unit prefix sums of the segment table, both directions, the refusals) -- plain g++, no library, CPU tier: it runs here, once as
it is and once built with -fsanitize=address,undefined (a stand-alone program with its own main).  Built by tests/cpp/trial.mk, a
line of `__graft_entry__.build()`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("binary", ["test_trial", "test_trial_asan"])
def test_the_planner_of_the_trial_snapshot(binary):
    subprocess.check_call(["make", "-C", CPP, "-f", "trial.mk", binary], stdout=subprocess.DEVNULL)
    res = subprocess.run([os.path.join(CPP, binary)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
