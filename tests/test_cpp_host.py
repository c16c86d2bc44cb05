"""The C++ host side above the C ABI (include/relp.hpp, the mirror of the reference's `MatrixData` / `Tableau` /
`PivotRule` / `OptimizationResult`): tests/cpp/test_tableau.cpp restates the reference's own unit tests of the
pivot path in C++ (tableau/mod.rs, strategy/pivot_rule.rs, two_phase/mod.rs, src/tests/problem_{1,2}.rs).
CPU tier: the header and the test program compile and link against the library.  GPU tier: the program runs."""
import os

import pytest

import cpp_programs


def test_cpp_host_header_compiles_and_links():
    cpp_programs.links_against_the_library("test_tableau")
    # C++17 only on the host side: no HIP header is pulled in through relp.hpp
    src = open(os.path.join(cpp_programs.ROOT, "include", "relp.hpp")).read()
    assert "hip/" not in src


def test_host_lu_factorisation_fusion_and_packing():
    """tests/cpp/test_lu_host.cpp (no GPU): P B Q = L U on the reference's factorisation cases (decomposition/mod.rs:301-491)
    and seeded LP-like bases, FTRAN / BTRAN against dense elimination, and the fused, ELL-packed schedules executed pass by pass
    like the device does, with pivots masked the way a Forrest-Tomlin update masks them."""
    cpp_programs.make_target("test_lu_host")
    cpp_programs.run("test_lu_host", timeout=600)


def test_device_lu_factorisation_as_a_host_model():
    """tests/cpp/test_lu_device_model.cpp (no GPU): the device-side LU factorisation (relp_lu_factor_core.h)
    compiled for the host -- the code the kernel k_lu_factor runs, its parallel loops serial -- on the reference's
    factorisation cases (decomposition/mod.rs:301-491), LP-like random bases and providers with slack, bound and artificial
    columns: P B Q = L U, row and column views, FTRAN / BTRAN against dense solves and against lu_factor."""
    cpp_programs.make_target("test_lu_device_model")
    cpp_programs.run("test_lu_device_model", timeout=600)


def test_standard_form_layout():
    """tests/cpp/test_layout.cpp (no GPU): the standard form the engine builds (rust-lp_amd/csrc/relp_layout.cpp) -- the
    reference's known answer for problem_1 (matrix_data.rs:680-755), the initial basis, rhs, -pi and phase-1 objective
    against the C oracle, row removal against a fresh layout, and the shard plans of every engine kind."""
    cpp_programs.make_target("test_layout")
    cpp_programs.run("test_layout", timeout=600)


def test_device_and_pinned_buffers_against_recording_stubs():
    """tests/cpp/test_buffers.cpp (no GPU): DeviceBuf / PinnedBuf (rust-lp_amd/csrc/relp_buffers.hpp) against stubs of the HIP
    calls they make -- lengths through alloc, ensure, adopt, swap and move, an empty buffer after a refused allocation, every copy
    and fill as one call on the caller's stream followed by one wait (none for the enqueue-only download), ranges that do not
    fit refused without a call, every allocation freed once."""
    cpp_programs.make_target("test_buffers")
    cpp_programs.run("test_buffers", timeout=600)


@pytest.mark.gpu
def test_cpp_host_tests_pass_on_the_gpu():
    cpp_programs.make_target("test_tableau", only_if_missing=True)
    res = cpp_programs.run("test_tableau", timeout=300)
    for kind in ("BasisInverseRows", "LUDecomposition", "DenseTableau"):
        assert any(line.startswith(kind) and line.rstrip().endswith("ok") for line in res.stdout.splitlines()), res.stdout
