"""tests/cpp/test_trial.cpp: the planner of the trial snapshot (rust-lp_amd/csrc/relp_trial.hpp: 16-byte-aligned offsets, no overlap,
the unit prefix sums of the segment table, both directions, the refusals) -- plain g++, no library, CPU tier: it runs here, once as
it is and once built with -fsanitize=address,undefined (a stand-alone program with its own main).
Built by tests/cpp/Makefile (`__graft_entry__.build()`)."""
import pytest

import cpp_programs


@pytest.mark.parametrize("binary", ["test_trial", "test_trial_asan"])
def test_the_planner_of_the_trial_snapshot(binary):
    cpp_programs.make_target(binary)
    cpp_programs.run(binary, timeout=60)
