"""tests/cpp/test_layout_remove.cpp: Layout::remove_cuts / remove_columns on the host (plain g++, no library) -- CPU tier, it runs
here.  tests/cpp/test_remove.cpp: cut rows and added columns removed in place through include/relp.hpp (remove_cuts, remove_columns,
removal_stats; the refusals) -- CPU tier: the program compiles and links against the library; GPU tier: it runs.  Both are built by
tests/cpp/remove.mk, a line of `__graft_entry__.build()`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LAYOUT_BINARY = os.path.join(CPP, "test_layout_remove")
LAYOUT_MAKE = ["make", "-C", CPP, "-f", "remove.mk", "test_layout_remove"]
BINARY = os.path.join(CPP, "test_remove")
MAKE = ["make", "-C", CPP, "-f", "remove.mk"]


def test_layout_remove_on_the_host():
    subprocess.check_call(LAYOUT_MAKE, stdout=subprocess.DEVNULL)
    res = subprocess.run([LAYOUT_BINARY], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout


def test_cpp_remove_test_compiles_and_links():
    import rust_lp_amd  # noqa: F401  (builds the library when it is missing)
    from rust_lp_amd import engine
    engine.load_library()
    subprocess.check_call(MAKE, stdout=subprocess.DEVNULL)
    assert os.access(BINARY, os.X_OK)


@pytest.mark.gpu
def test_cpp_remove_test_passes_on_the_gpu():
    if not os.access(BINARY, os.X_OK):
        subprocess.check_call(MAKE, stdout=subprocess.DEVNULL)
    res = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
