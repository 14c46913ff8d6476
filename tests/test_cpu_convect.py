"""The yardstick of the convection term (include/fdd_hip.h: fdd_field_convect, fdd_field_weak_convect), without a GPU: what
the numpy restatement (tests/convect_checks.py) gives in float64 against np.longdouble -- the figures the bounds of
tests/test_gpu_convect.py stand on --, that the (3n+1)/2-point rule integrates the term exactly on affine elements while
the collocated form does not, and what the host entries answer on a kernel library without the kernels.

Worst float64-against-longdouble figures on the shapes below (each test prints its own): convect 2.9e-14 T_c (Kershaw
N = 15), weak_convect 3.3e-16 T_wc.  Exactness in long double: 1.9e-19 T_wc at worst.  Separation: the collocated weak form
misses the exact one by 4.2e-3 T_wc (N = 15) to 8.7e-1 T_wc (N = 1).  Host tables against the long double ones: nodes
1.1e-16, weights 3.0e-16, P 3.0e-15 max|P|, Pd 2.7e-15 max|Pd| (N = 15)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import convect_checks as C
import field_checks as F
import support as S

SHAPES = [("box", (2, 3, 2), 7), ("kershaw", (2, 1, 1), 7), ("deformed", (2, 2, 2), 7), ("kershaw", (2, 2, 2), 2), ("deformed", (2, 1, 1), 1), ("kershaw", (2, 1, 1), 15), ("deformed", (1, 1, 2), 8)]
IDS = ["%s-%dx%dx%d-N%d" % ((k,) + E + (N,)) for k, E, N in SHAPES]


@pytest.mark.parametrize("kind,E,N", SHAPES, ids=IDS)
def test_restatement_in_double_against_long_double(kind, E, N):
    mesh = F.mesh_of(kind, E, N)
    ref, dbl = F.geometry(mesh, np.longdouble), F.geometry(mesh, np.float64)
    c, u = C.fields(mesh, 500 + N)
    Tc, Twc = C.convect_scale(ref, c, u), C.weak_convect_scale(ref, c, u)
    err = float(np.abs(C.convect(dbl, c, u) - C.convect(ref, c, u)).max())
    werr = float(np.abs(C.weak_convect(dbl, c, u) - C.weak_convect(ref, c, u)).max())
    print("convect: %.2e T_c, weak_convect: %.2e T_wc" % (err / Tc, werr / Twc))
    assert err <= 1e-11 * Tc and werr <= 1e-11 * Twc


# ---- the rule is exact on affine elements, the collocated form is not ----
BOX_DEGREES = (1, 2, 3, 7, 8, 15)


@pytest.fixture(scope="module", params=BOX_DEGREES)
def box(request):
    N = request.param
    mesh = F.mesh_of("box", (2, 1, 2), N)
    g = F.geometry(mesh, np.longdouble)
    c, u = C.fields(mesh, 600 + N)
    return N, g, c, u, C.weak_convect(g, c, u, M=2 * (N + 1) + 2), C.weak_convect_scale(g, c, u)


def test_the_three_halves_rule_is_exact_on_the_box(box):
    N, g, c, u, exact, Twc = box
    err = float(np.abs(C.weak_convect(g, c, u) - exact).max())
    print("N = %d: (3n+1)/2 points against 2n+2: %.2e T_wc" % (N, err / Twc))
    assert err <= 1e-15 * Twc


def test_the_collocated_weak_form_is_told_apart(box):
    N, g, c, u, exact, Twc = box
    gap = float(np.abs(C.collocated_weak(g, c, u) - exact).max())
    print("N = %d: mass . convect against the exact integral: %.2e T_wc" % (N, gap / Twc))
    assert gap > 1e-8 * Twc


# ---- the host entries on the CPU build of the host layer, whose kernel library has no fdd_field_* entries ----
SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


@pytest.fixture(scope="module")
def report():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "convect_refusals.py"), HOST_CPU_SO], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("N", (1, 2, 7, 8, 15))
def test_quadrature_tables_of_the_host_library(report, N):
    t = {k: np.array(v) for k, v in report["tables"][str(N)].items()}
    n, M = N + 1, (3 * (N + 1) + 1) // 2
    z, w, P, Pd = C.tables(N, np.longdouble, t["D"])
    assert len(t["z"]) == M and len(t["P"]) == M * n
    got_P, got_Pd = t["P"].reshape(M, n), t["Pd"].reshape(M, n)
    figures = (float(np.abs(t["z"] - z).max()), float(np.abs(t["w"] - w).max()), float(np.abs(got_P - P).max() / np.abs(P).max()), float(np.abs(got_Pd - Pd).max() / np.abs(Pd).max()))
    print("N = %d: z %.1e, w %.1e, P %.1e max|P|, Pd %.1e max|Pd|" % ((N,) + figures))
    assert figures[0] <= 1e-14 and figures[1] <= 1e-14 and figures[2] <= 1e-13 and figures[3] <= 1e-12
    assert np.abs(got_P.sum(axis=1) - 1).max() <= 1e-14 and abs(t["w"].sum() - 2) <= 1e-14
    assert (np.diff(t["z"]) > 0).all() and (t["w"] > 0).all()


def test_quadrature_follows_a_changed_table(report):
    before = np.array(report["tables"]["7"]["Pd"])
    assert np.array_equal(np.array(report["moved"]), 2.0 * before) and np.abs(before).max() > 0


def test_operator_entries_name_the_missing_kernel_entry(report):
    for name, (rc, text) in report["box"].items():
        assert rc != 0 and "fdd_field_convect" in text and "does not export" in text, (name, rc, text)


def test_operator_entries_keep_the_rank_check_and_the_null_text(report):
    for name, (rc, text) in report["uninit"].items():
        assert rc != 0 and text.startswith("fddh_init has not been called on this thread"), (name, rc, text)
    for name, (rc, text) in report["null"].items():
        assert rc != 0 and text == "null argument", (name, rc, text)
