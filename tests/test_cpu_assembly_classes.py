"""The classes of the rows of the subdomain's gather Qt (host/assembly_classes.hpp, flag "assemble_in_stiffness"), on the CPU
build of the host layer (tests/cpu_shim): no GPU.

The classifier reads Qt's own arrays.  Here Qt is rebuilt in numpy from fddh_problem_sub_point_dofs (Qt = Q^T, one unit entry
per point with a dof, columns ascending) and every statement of the header is checked against it on boxes of 4x1x1, 5x2x2,
8x3x2 and 1x1x1 elements at N = 7:
  - single, pair and general partition the rows, every point carries the class of its dof's row, and a row is never split;
  - a pair row is, in column order, the point (7, j, k) of list element e and the point (0, j, k) of element e + 1 with
    e // 4 == (e + 1) // 4 -- so no pair crosses a workgroup of four elements or the end of an x-row (5x2x2: x-rows of five);
  - the general rows' own CSR holds exactly the other rows, in order, with their dofs;
  - the counts are those of the lattice: the box is Dirichlet on all six faces, so its dofs are the (7 Ex - 1)(7 Ey - 1)
    (7 Ez - 1) interior nodes; a node off every element face is a single row (6 Ex * 6 Ey * 6 Ez), a node on one x-face and
    off the y- and z-faces lies between elements e and e + 1 of an x-row (e = ex + Ex (ey + Ey ez)) and is a pair row where
    e % 4 != 3 (36 per such face), and all other rows are general.
A Kershaw list classifies too (the classes do not look at the factors); the flag has no effect there, the line form does not
run.  The stand-in has neither fdd_stiffness_matrix_lines_direct nor fdd_csr_plan_gather_mapped: the flag is off and refuses
to be set, naming the entry."""
import os
import subprocess
import sys

import pytest

import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")

PRELUDE = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H, lib
lib._host = lib._Lib(%r, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
H.init(0, use_torch_stream=False); H.comm_single(); H.set_print(False)

BITS = 29
GENERAL, SINGLE, PAIR_LOW, PAIR_HIGH = 0, 1, 2, 3

def qt_of(pd, nrows):
    '''Q^T of the boolean scatter: per dof its points, ascending'''
    pts = np.flatnonzero(pd >= 0)
    order = np.argsort(pd[pts], kind="stable")
    col = pts[order].astype(np.int64)
    ptr = np.zeros(nrows + 1, np.int64)
    np.add.at(ptr, pd[pts] + 1, 1)
    return np.cumsum(ptr), col

def check(p, E):
    pd = p.sub_point_dofs()
    nrows = int(pd.max()) + 1
    ptr, col = qt_of(pd, nrows)
    info = p.assembly_info()
    pcd, rptr, rcol, rmap = p.assembly_arrays()
    assert len(pcd) == len(pd) and np.array_equal(pcd < 0, pd < 0) and np.array_equal(pcd[pd < 0], pd[pd < 0])
    has = pd >= 0
    assert np.array_equal(pcd[has] & ((1 << BITS) - 1), pd[has])
    cls = np.where(has, pcd >> BITS, -1)
    assert set(np.unique(cls[has])) <= {GENERAL, SINGLE, PAIR_LOW, PAIR_HIGH}
    row_class = np.full(nrows, -1)
    counts = {"general": 0, "single": 0, "pair": 0}
    for r in range(nrows):
        c = col[ptr[r]:ptr[r + 1]]
        k = cls[c]
        if len(c) == 1 and k[0] == SINGLE:
            row_class[r] = SINGLE
        elif len(c) == 2 and k[0] == PAIR_LOW and k[1] == PAIR_HIGH:
            e0, at0, e1, at1 = c[0] // 512, c[0] %% 512, c[1] // 512, c[1] %% 512
            assert at0 & 7 == 7 and at1 & 7 == 0 and at0 >> 3 == at1 >> 3 and e1 == e0 + 1 and e0 // 4 == e1 // 4, (r, c)
            assert e0 %% E[0] != E[0] - 1, (r, c)  # not across the end of an x-row
            row_class[r] = PAIR_LOW
        else:
            assert (k == GENERAL).all() and len(c) != 1, (r, c, k)  # never split, and no single row left to the gather
            row_class[r] = GENERAL
    general_rows = np.flatnonzero(row_class == GENERAL)
    assert np.array_equal(rmap, general_rows)
    assert np.array_equal(np.diff(rptr), (ptr[1:] - ptr[:-1])[general_rows]) and rptr[0] == 0
    assert np.array_equal(rcol, np.concatenate([col[ptr[r]:ptr[r + 1]] for r in general_rows]) if len(general_rows) else np.zeros(0))
    # the lattice
    Ex, Ey, Ez = E
    assert nrows == (7 * Ex - 1) * (7 * Ey - 1) * (7 * Ez - 1)
    single = 216 * Ex * Ey * Ez
    pair = 36 * sum(1 for ez in range(Ez) for ey in range(Ey) for ex in range(Ex - 1) if (ex + Ex * (ey + Ey * ez)) %% 4 != 3)
    want = {"general": nrows - single - pair, "single": single, "pair": pair}
    assert info["rows"] == want, (info, want)
    assert {k: int((row_class == v).sum()) for k, v in (("general", GENERAL), ("single", SINGLE), ("pair", PAIR_LOW))} == want
    pts = info["points"]
    assert pts["single"] == single and pts["pair_low"] == pair and pts["pair_high"] == pair and pts["none"] == int((pd < 0).sum())
    assert pts["general"] == len(rcol) == int(has.sum()) - single - 2 * pair
    assert info["enabled"] is False and info["in_effect"] is False and info["why_not"] == "the flag is off", info
    return want
""" % (S.ROOT, S.HERE, HOST_CPU_SO)


def run(code):
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    out = subprocess.run([sys.executable, "-c", PRELUDE + code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.parametrize("E", [(4, 1, 1), (5, 2, 2), (8, 3, 2), (1, 1, 1)])
def test_box_classes_partition_the_rows_and_count_as_the_lattice_says(E):
    out = run(r"""
E = %r
p = H.Problem.box(E, (1, 1, 1), 7, 6, True)
want = check(p, E)
if E == (5, 2, 2):
    assert want["pair"] == 36 * 12  # three of the four faces of every x-row of five: one always lies across a workgroup
if E == (1, 1, 1) or E == (4, 1, 1):
    assert want["general"] == 0
print("classes ok", want)
""" % (E,))
    assert "classes ok" in out, out


def test_kershaw_list_classifies_and_the_flag_is_refused_without_the_entries():
    out = run(r"""
p = H.Problem.kershaw((3, 2, 2), (1, 1, 1), 7, 6, 0.3, True)
info = p.assembly_info()
assert not info["in_effect"] and sum(info["rows"].values()) == int(p.sub_point_dofs().max()) + 1 and info["rows"]["pair"] > 0, info
pcd, rptr, rcol, rmap = p.assembly_arrays()
assert len(rmap) == info["rows"]["general"] and len(rcol) == info["points"]["general"]
try:
    p.set_flag("assemble_in_stiffness", 1)
except lib.FddError as e:
    print("refused:", e)
else:
    raise SystemExit("the flag was accepted without the kernel entries")
p.set_flag("assemble_in_stiffness", 0)
assert p.assembly_info() == info
print("kershaw ok")
""")
    assert "refused:" in out and "fdd_stiffness_matrix_lines_direct" in out and "kershaw ok" in out, out
