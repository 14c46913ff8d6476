"""Successive-right-hand-side projection (fddh_problem_solve_projected) on the CPU build of the host layer
(tests/cpu_shim).  The C-ABI stand-in there has no fdd_projection_* entries, the host layer references them weakly, so
every pass runs as its composition from the multi-vector entries (host/projection.hpp): this file is that
implementation's test, and tests/test_gpu_projection.py holds the kernels to it.

The checks themselves are tests/projection_checks.py, one child process each (the stand-in library must not stay loaded
in the test process).  Observed on this build, 4x4x4 elements at N = 3: the stored images differ from A X_k by 3.5e-16
relative, X^T A X from the identity by 4.4e-16; an exact float64 projection of 0.7 f_0 - 1.3 f_1 + 0.4 f_2 onto the basis
of three solves at 1e-10 leaves 9.1e-11 |f|, 1.1e5 times below the 1e-5 the in-span solve is held to (100 times is
required)."""
import os
import subprocess
import sys

import pytest

import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


@pytest.fixture(scope="module")
def cpu_host_lib():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    assert os.path.exists(HOST_CPU_SO)
    return HOST_CPU_SO


def run_check(lib_path, name):
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "projection_checks.py"), lib_path, name], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-6000:] + out.stderr[-4000:]
    return out.stdout


def test_basis_is_a_orthonormal_and_a_rhs_in_its_span_costs_nothing(cpu_host_lib):
    """A X_k within 1e-12 of the operator's, X^T A X = I within 1e-10; f in the span: 0 iterations at 1e-5 where the plain
    solve iterates, and the exact projection stays 100 times below that bar (the figures are in the module docstring)"""
    out = run_check(cpu_host_lib, "basis_and_span")
    assert "exact projection leaves" in out


@pytest.mark.parametrize("method", ["fcg", "gmres"])
def test_sequence_needs_fewer_iterations_and_meets_the_tolerance(cpu_host_lib, method):
    """eight slowly varying right-hand sides at capacity 4, without and with the V-cycle: every solve meets the
    tolerance and agrees with the plain solve, a restart happens, and the iterations add up to fewer"""
    out = run_check(cpu_host_lib, "sequence_" + method)
    assert "vcycle 0:" in out and "vcycle 1:" in out


def test_lifecycle(cpu_host_lib):
    run_check(cpu_host_lib, "lifecycle")


def test_two_ranks_agree_with_one(cpu_host_lib):
    """two ranks of one process on 8x4x4 elements: the same figures on both ranks, no iteration in the span, and each
    solution within 10 x the span test's tolerance x |u|_inf of the one-rank run's (the solves themselves run tighter:
    projection_checks.check_two_ranks says why)"""
    run_check(cpu_host_lib, "two_ranks")


def test_fused_flag_names_the_missing_entry_and_the_default_falls_back(cpu_host_lib):
    """"fused_projection" 1 is refused here, naming the entry the library lacks; every other test of this file ran on the
    default, which quietly composed the passes"""
    out = run_check(cpu_host_lib, "fused_flag")
    assert "refused:" in out and "fdd_projection_dots" in out and "fused_projection" in out
