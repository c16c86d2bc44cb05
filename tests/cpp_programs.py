"""Helper module of tests/test_cpp_*.py (not collected by pytest): the programs of tests/cpp, each a target of tests/cpp/Makefile under
its own name (`__graft_entry__.build()` makes them all).  A test makes its target, runs it and holds it to the one contract every
program keeps through tests/cpp/check.hpp: exit code 0 and a summary line with " 0 failed"."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def binary(name):
    return os.path.join(CPP, name)


def make_target(name, only_if_missing=False):
    """`make -C tests/cpp name`; only_if_missing: a program that is there is taken as it is (the GPU tier runs what was built)."""
    if not (only_if_missing and os.access(binary(name), os.X_OK)):
        subprocess.check_call(["make", "-C", CPP, name], stdout=subprocess.DEVNULL)


def links_against_the_library(name):
    """The CPU tier of a program over include/relp.hpp: it compiles and links against the engine library."""
    import rust_lp_amd  # noqa: F401  (builds the library when it is missing)
    from rust_lp_amd import engine
    engine.load_library()
    make_target(name)
    assert os.access(binary(name), os.X_OK)


def run(name, timeout):
    """Runs the program: exit code 0 and " 0 failed" in its output.  Returns the finished process."""
    res = subprocess.run([binary(name)], capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-1000:]
    assert " 0 failed" in res.stdout
    return res
