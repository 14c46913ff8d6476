"""Chebyshev-Jacobi inner solve (flag "inner_solver" = 1) on the CPU build of the host layer (tests/cpu_shim).  The C-ABI
stand-in there has neither fdd_cheby_step nor the fused gather epilogue, the host layer references them weakly, so every
step runs as its composition from vector_vector_addition and vector_diagonal_scaling_dev (Subdomain::chebyshev_dofs):
this file is that form's test, and tests/test_gpu_chebyshev.py holds the kernels to its bits.

The checks themselves are tests/chebyshev_checks.py, one child process each (the stand-in library must not stay loaded in
the test process)."""
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
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "chebyshev_checks.py"), lib_path, name], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-6000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("shape", ["E2N3", "E3N3", "E3N7"])
def test_recurrence_bound_map_and_outer_solves(cpu_host_lib, shape):
    """orders 1, 2, 4, 7 against the numpy recurrence (1e-12; order 1 to 1 ulp); M is linear, symmetric, positive and
    repeatable; at N = 3 also: lambda <= lambda_true <= upper * lambda on the dense operator, the preconditioner application
    bit for bit through the dof-space hook, both outer solvers against the oracle's with the numpy recurrence plugged in,
    pcg_steps(5) against five single steps, and inner_solver 0 giving its earlier bits again; on the smallest shape the
    invalidation of the cached diagonal and bound by set_D_hat"""
    out = run_check(cpu_host_lib, shape)
    assert "recurrence %s:" % shape in out and "map %s:" % shape in out


def test_two_rank_composite(cpu_host_lib):
    out = run_check(cpu_host_lib, "composite")
    assert "composite: iterations" in out


def test_refusals_leave_the_problem_usable(cpu_host_lib):
    out = run_check(cpu_host_lib, "refusals")
    assert out.count("refused:") >= 10


def test_kernel_flags_name_the_missing_entry(cpu_host_lib):
    """ "chebyshev_kernels" / "fused_chebyshev" 1 are refused here, naming the entry the library lacks; every other test of
    this file ran on the default, which composed the steps"""
    out = run_check(cpu_host_lib, "kernel_flags")
    assert out.count("refused:") == 2 and "fdd_cheby_step" in out
