"""The yardstick of the Helmholtz solves (tests/test_gpu_helmholtz.py), without a GPU: what the dense reference of
tests/helmholtz_checks.py gives on the 2^3-element unit box -- the error of (-laplace + lam) u = (3 pi^2 + lam) sin sin sin
against the exact solution as a share of the Poisson error of field_checks.source_solve_error, and the condition number
of the Jacobi-scaled matrix, which is what a shift on the exact diagonal buys -- and what the host entries answer on a
kernel library without the kernels.

The figures this reference gives (each test prints its own):
  error / Poisson error   lam = 0     1       1e2     1e4     1e6
                  N = 3   1.000   0.991   0.590   0.0374  0.00039
                  N = 5   1.000   0.997   0.773   0.106   0.00127
                  N = 7   1.000   0.998   0.867   0.186   0.00321
  cond(D^-1/2 A D^-1/2), N = 7:  175.1   169.7   45.22   2.048   1.012
"""
import json
import os
import subprocess
import sys

import pytest

import field_checks as F
import helmholtz_checks as C
import support as S

LAMBDAS = (0.0, 1.0, 1e2, 1e4, 1e6)
RATIOS = {3: (1.000, 0.991, 0.590, 0.0374, 0.00039), 5: (1.000, 0.997, 0.773, 0.106, 0.00127), 7: (1.000, 0.998, 0.867, 0.186, 0.00321)}
CONDITION_N7 = (175.1, 169.7, 45.22, 2.048, 1.012)


@pytest.mark.parametrize("N", (3, 5, 7))
def test_error_against_the_exact_solution_never_exceeds_the_poisson_error(N):
    poisson = F.source_solve_error(N)
    ratios = [C.box(N).solve_error(lam) / poisson for lam in LAMBDAS]
    print("N = %d: error / Poisson error" % N, ["%.4g" % r for r in ratios])
    for lam, r, want in zip(LAMBDAS, ratios, RATIOS[N]):
        assert r <= 1.0 + 1e-8, (N, lam, r)  # lam = 0 is the Poisson solve itself, to the rounding of the dense solve
        assert abs(r / want - 1.0) <= 0.02, (N, lam, r, want)


def test_condition_number_of_the_jacobi_scaled_matrix():
    kappa = [C.box(7).jacobi_condition(lam) for lam in LAMBDAS]
    print("N = 7: cond(D^-1/2 A D^-1/2)", ["%.4g" % k for k in kappa])
    for lam, k, want in zip(LAMBDAS, kappa, CONDITION_N7):
        assert abs(k / want - 1.0) <= 0.005, (lam, k, want)
    assert all(a >= b for a, b in zip(kappa, kappa[1:]))


def test_cg_bound_of_the_shifted_problem():
    """the bound the GPU test holds the diagonally scaled solve to: kappa = 2.05 and tau = 1e-10 give 14 (+ 2 there)"""
    assert C.cg_bound(C.box(7).jacobi_condition(1e4), 1e-10) == 14
    assert C.cg_bound(4.0, 0.5) == 2  # 2 (1/3)^k <= 1/2 from k = 2 on


# ---- the host entries on the CPU build of the host layer, whose kernel library has no fdd_shift_add* entries ----
SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


@pytest.fixture(scope="module")
def refusals():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "helmholtz_refusals.py"), HOST_CPU_SO], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]  # the library loads against the header: every declared entry is bound
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_host_library_without_the_kernels_has_the_four_entries(refusals):
    assert refusals["entries"] == ["fddh_helmholtz_info", "fddh_helmholtz_node_operator", "fddh_helmholtz_set", "fddh_helmholtz_shift"]


def test_set_names_the_first_missing_kernel_entry(refusals):
    rc, text = refusals["set"]
    assert rc != 0 and "fdd_shift_add," in text and "does not export" in text, (rc, text)


def test_the_problem_stays_usable_and_unshifted(refusals):
    assert refusals["info"] == {"active": False, "min": 0.0, "max": 0.0} and refusals["shift_max"] == 0.0
    its, rel = refusals["solve"]
    assert its > 0 and rel < 1e-6, refusals["solve"]
