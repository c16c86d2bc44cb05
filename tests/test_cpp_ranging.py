"""tests/cpp/test_ranging.cpp: the batched ratio queries through include/relp.hpp (row_ratios, rhs_ranging, ranging_stats on one small
LP; the refusals).  Built by tests/cpp/ranging.mk (`__graft_entry__.build()`).  CPU tier: the program compiles and links against the
library.  GPU tier: it runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
BINARY = os.path.join(CPP, "test_ranging")
MAKE = ["make", "-C", CPP, "-f", "ranging.mk"]               # a makefile of its own beside tests/cpp/Makefile


def test_cpp_ranging_test_compiles_and_links():
    import rust_lp_amd  # noqa: F401  (builds the library when it is missing)
    from rust_lp_amd import engine
    engine.load_library()
    subprocess.check_call(MAKE, stdout=subprocess.DEVNULL)
    assert os.access(BINARY, os.X_OK)


@pytest.mark.gpu
def test_cpp_ranging_test_passes_on_the_gpu():
    if not os.access(BINARY, os.X_OK):
        subprocess.check_call(MAKE, stdout=subprocess.DEVNULL)
    res = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
