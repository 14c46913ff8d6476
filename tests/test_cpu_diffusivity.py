"""Variable diffusivity on the CPU build of the host layer (tests/cpu_shim): the scaled factor arrays G' = kappa G run through
the stand-in's kernels, which were there before -- the coefficient line instance is the GPU's (tests/test_gpu_stiffness_coef.py,
tests/test_gpu_diffusivity.py).  The checks themselves are tests/diffusivity_checks.py and tests/diffusivity_refusals.py, one
child process each (the stand-in library must not stay loaded in the test process).

Figures on the stand-in (each check prints its own): operator against numpy at most 2.7e-16 of max|Au| (bound 1e-12), the inner
operator 1.2e-15, its diagonal 8.6e-16; largest true residual 0.996 tau |f^| (bound 10); the error against the exact solution
for the smooth kappa at most 1.003 x the dense solve's own (bound 1.05), which is 9.97e-4, 7.03e-6, 2.58e-8 at N = 3, 5, 7;
the jump 1 : 1000 on box (4,2,2), N = 5: 5 outer iterations with the kappa-aware hierarchy, 61 with the kappa-free one."""
import os
import subprocess
import sys

import pytest

import diffusivity_checks as C
import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")
SHIM_SO = os.path.join(SHIM_DIR, "_build", "libfdd_cpu_shim.so")


@pytest.fixture(scope="module")
def cpu_host_lib():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    assert os.path.exists(HOST_CPU_SO)
    return HOST_CPU_SO


def run_check(lib_path, name):
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "diffusivity_checks.py"), lib_path, name], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-6000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.parametrize("case", list(C.OPERATOR_CASES))
def test_operator_against_numpy(cpu_host_lib, case):
    """stiffness against D^T [kappa G] D u to 1e-12 max|Au|; kappa = 2 twice the unscaled result bit for bit; symmetry; the
    inner operator and its exact diagonal against the assembled K_kappa; the mesh's arrays stay; clearing restores the bits"""
    out = run_check(cpu_host_lib, "operator_" + case)
    assert out.count("operator %s:" % case) == 2


@pytest.mark.parametrize("N", (3, 5, 7))
def test_solves_meet_the_dense_matrix(cpu_host_lib, N):
    """smooth kappa and the jump 1 : 100 through the five inner configurations and both outer methods (the stand-in
    refuses a Helmholtz shift, so the third coefficient is the GPU's)"""
    out = run_check(cpu_host_lib, "solves_N%d" % N)
    assert out.count("true residual") == 2 * 5 * 2 + 1


@pytest.mark.parametrize("case", list(C.HIERARCHY_CASES))
def test_level_zero_matrix_is_the_restatement(cpu_host_lib, case):
    assert "as bits" in run_check(cpu_host_lib, "hierarchy_" + case)


def test_kappa_aware_hierarchy_is_no_worse_across_a_jump(cpu_host_lib):
    assert "kappa-aware" in run_check(cpu_host_lib, "hierarchy_jump")


def test_clearing_and_setting_twice(cpu_host_lib):
    assert "clearing:" in run_check(cpu_host_lib, "clearing")


def test_refusals_leave_the_problem_as_it_was(cpu_host_lib):
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "diffusivity_refusals.py"), cpu_host_lib, SHIM_SO], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-6000:] + out.stderr[-4000:]
    for name in ("fdd_stiffness_matrix_lines_coef", "fdd_stiffness_matrix_lines_coef_f32", "fdd_stiffness_matrix_lines_coef_direct"):
        assert "missing: %s\n" % name in out.stdout  # the stand-in has none of the three entries
    assert out.stdout.count("refused:") == 15
