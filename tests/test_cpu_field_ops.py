"""The yardstick of the field operators (mass, gradient, weak divergence; include/fdd_hip.h: fdd_field_*), without a GPU:
what their numpy restatement (tests/field_checks.py) gives in float64 against np.longdouble and against the oracle's
stiffness operator -- the figures the bounds of tests/test_gpu_field_ops.py are set from --, what the host entries answer
on a kernel library without the kernels, and the discretisation error of -laplace(u) = s from f = B s.

Worst float64-against-longdouble figures this restatement gives on the shapes below (each test prints its own; the bounds
leave 10x to 100x and more over them):
  gradient 8.6e-14 T and mass 2.6e-13 pointwise (Kershaw (6,2,2) N=11), weak divergence 1.7e-15 T_w, wdiv(grad u) against
  the oracle's stiffness 2.6e-14 max|Au| (box (2,3,2) N=7; Kershaw at most 6.8e-16), |grad(a.X + c) - a| 2.6e-12 (Kershaw
  N=11; 3.2e-13 at N=7), adjoint 1.5e-17 of the sum of the absolute terms."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import field_checks as F
import support as S

SHAPES = [("box", (2, 3, 2), 7), ("kershaw", (6, 2, 2), 7), ("kershaw", (6, 2, 2), 11), ("kershaw", (3, 2, 2), 3), ("kershaw", (2, 2, 2), 2), ("kershaw", (2, 1, 1), 15), ("deformed", (2, 2, 2), 7)]
IDS = ["%s-%dx%dx%d-N%d" % ((k,) + E + (N,)) for k, E, N in SHAPES]


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request):
    kind, E, N = request.param
    mesh = F.mesh_of(kind, E, N)
    return mesh, F.geometry(mesh, np.longdouble), F.geometry(mesh, np.float64), F.fields(mesh, 100 + N)


def test_gradient_in_double_against_long_double(case):
    mesh, ref, dbl, (u, v, phi) = case
    T = F.gradient_scale(ref, u)
    err = max(float(np.abs(a - b).max()) for a, b in zip(F.gradient(dbl, u), F.gradient(ref, u)))
    print("gradient: %.2e T" % (err / T))
    assert err <= 1e-12 * T


def test_mass_in_double_against_long_double(case):
    mesh, ref, dbl, _ = case
    rel = float(np.abs(F.mass(dbl) / F.mass(ref) - 1).max())
    print("mass: %.2e" % rel)
    assert (F.mass(ref) > 0).all() and rel <= 1e-11


def test_mass_sums_to_the_volume_of_the_unit_cube(case):
    mesh, ref, dbl, _ = case
    assert abs(float(F.mass(dbl).sum()) - 1.0) <= 1e-12


def test_weak_divergence_in_double_against_long_double(case):
    mesh, ref, dbl, (u, v, phi) = case
    Tw = F.weak_divergence_scale(ref, v)
    err = float(np.abs(F.weak_divergence(dbl, v) - F.weak_divergence(ref, v)).max())
    print("weak divergence: %.2e T_w" % (err / Tw))
    assert err <= 1e-11 * Tw


def test_weak_divergence_of_the_gradient_is_the_oracles_stiffness(case):
    mesh, ref, dbl, (u, v, phi) = case
    Au, _ = S.oracle_stiffness(u, mesh.g, np.ascontiguousarray(S.gll(mesh.N)[2]), mesh.N)
    err = float(np.abs(F.weak_divergence(dbl, F.gradient(dbl, u)) - Au).max())
    print("wdiv(grad u) - Au: %.2e max|Au|" % (err / np.abs(Au).max()))
    assert err <= 1e-12 * np.abs(Au).max()


def test_gradient_of_a_linear_field_is_its_slope(case):
    mesh, ref, dbl, _ = case
    g = F.gradient(dbl, F.linear_field(mesh))
    err = max(float(np.abs(g[a] - F.LINEAR[a]).max()) for a in range(3))
    print("linear: %.2e" % err)
    assert err <= 1e-10


def test_weak_divergence_is_the_adjoint_of_the_gradient(case):
    mesh, ref, dbl, (u, v, phi) = case
    lhs, rhs, scale = F.adjoint_sides(dbl, F.weak_divergence(dbl, v), v, phi, F.gradient(dbl, phi))
    print("adjoint: %.2e of the absolute terms" % (abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-13 * scale


def test_a_transposed_metric_is_an_error_of_order_T():
    """what the bounds are there to catch: J^-T in the place of J^-1 misses the gradient by a share of T no bound above allows"""
    mesh = F.mesh_of("kershaw", (6, 2, 2), 7)
    g = F.geometry(mesh, np.float64)
    u = F.fields(mesh, 107)[0]
    good = F.gradient(g, u)
    g.I = [[g.I[a][b] for a in range(3)] for b in range(3)]
    err = max(float(np.abs(a - b).max()) for a, b in zip(F.gradient(g, u), good))
    assert err >= 1e-2 * F.gradient_scale(g, u)


# ---- the host entries on the CPU build of the host layer, whose kernel library has no fdd_field_* entries ----
SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


@pytest.fixture(scope="module")
def refusals():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "field_refusals.py"), HOST_CPU_SO], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]  # the library loads against the header: every declared entry is bound
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_host_library_without_the_kernels_has_the_three_entries(refusals):
    assert refusals["entries"] == ["fddh_field_gradient", "fddh_field_mass", "fddh_field_weak_divergence"]


def test_entries_name_the_missing_kernel_entry(refusals):
    for name, (rc, text) in refusals["box"].items():
        assert rc != 0 and "fdd_field_mass" in text and "does not export" in text, (name, rc, text)


def test_entries_keep_the_rank_check_and_the_null_text(refusals):
    for name, (rc, text) in refusals["uninit"].items():
        assert rc != 0 and text.startswith("fddh_init has not been called on this thread"), (name, rc, text)
    for name, (rc, text) in refusals["null"].items():
        assert rc != 0 and text == "null argument", (name, rc, text)


# ---- the source-term problem, as the yardstick of the solve test on the GPU ----
def test_source_term_solve_converges_at_the_computed_rate():
    """-laplace(u) = 3 pi^2 sin(pi x) sin(pi y) sin(pi z) on 2x2x2 elements, f = B s, dense solve: max error against the exact
    solution 4.8e-4 (N=3), 1.14e-6 (N=5), 1.6e-9 (N=7)"""
    err = {N: F.source_solve_error(N) for N in (3, 5, 7)}
    print("source-term solve:", err)
    for N, want in ((3, 4.8e-4), (5, 1.14e-6), (7, 1.6e-9)):
        assert abs(err[N] / want - 1.0) <= 0.05, (N, err[N])
    assert err[3] / err[5] >= 50 and err[5] / err[7] >= 50
