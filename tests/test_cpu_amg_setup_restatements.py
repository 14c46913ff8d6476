"""The Python restatements of host/low_order.hpp (tests/amg_setup_restatements.py) against the host build itself, without
a GPU: libfdd_host on the CPU stand-in of the kernel library (tests/cpu_shim), in a child process as test_cpu_amg.py does.
The restatements are the reference of the device setup kernels (test_gpu_amg_setup_kernels.py), so they are held here to
what the host computes -- bit for bit -- and never to the kernels under test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import amg_setup_restatements as R
import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")

CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import support as S, amg_setup_restatements as R
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H, lib
lib._host = lib._Lib(%r, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
H.init(0, use_torch_stream=False); H.comm_single(); H.set_print(False)
kind, N, expect_geometric = %r, %d, %r
p = H.Problem.box((2, 2, 2), (1, 1, 1), N, 2, True) if kind == "box" else H.Problem.kershaw((2, 2, 2), (1, 1, 1), N, 2, 0.3)
for lvl in range(p.info["num_levels"]):
    p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
p.amg_build(device=False)
assert p.amg_setup_info()["levels_built_on_device"] == 0
lv = p.amg_levels()[0]
dof, nd, n = p.sub_point_dofs(), p.info["sub_num_dofs"], N + 1
x, y, z = (p.mesh_array(c) for c in "xyz")
assert len(dof) == len(x) == 8 * n**3 and lv["A"].shape == (nd, nd)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

# the level-0 matrix: low_order::assemble_fem
K, mask, (ptr, col, val), dets = R.assemble_fem_ref(x, y, z, dof, nd, N)
assert dets.min() > 0.0
A = lv["A"]
assert np.array_equal(ptr, A.indptr) and np.array_equal(col, A.indices), "pattern of A"
assert np.array_equal(bits(val), bits(A.data)), "values of A: %%d of %%d differ" %% ((bits(val) != bits(A.data)).sum(), len(val))
if kind == "kershaw":
    assert np.diff(ptr).max() > 7

# the level-0 interpolator: low_order::geometric_level, where the host coarsened level 0 on the lattice
geometric = p.amg_level_transfer(0)
assert geometric == expect_geometric, geometric
if geometric:
    ref = S.gll(N)[0]
    keep = R.coarse_nodes_ref(n, ref)
    lo, hi, wl = R.interp_tables_ref(ref, keep)
    g = R.geometric_level_ref(dof, nd, n, keep, lo, hi, wl)
    assert not g["refused"] and g["unplaced"] == 0
    P = lv["P"]
    assert P.shape == (nd, g["num_coarse"])
    assert np.array_equal(g["P"][0], P.indptr) and np.array_equal(g["P"][1], P.indices), "pattern of P"
    assert np.array_equal(bits(g["P"][2]), bits(P.data)), "values of P"
print("ok", kind, N, nd, len(val), geometric)
"""


@pytest.mark.parametrize("kind,N,geometric", [("box", 3, False), ("box", 4, False), ("box", 7, True), ("kershaw", 7, True)], ids=["box_N3", "box_N4", "box_N7", "kershaw_N7"])
def test_restatements_are_the_host_build(kind, N, geometric):
    """assemble_fem_ref gives amg_levels()[0]["A"] and, where level 0 is coarsened on the lattice (degree 7: 8 -> 4 nodes;
    degrees 3 and 4 start with an aggregation level, which the test asserts rather than assumes), geometric_level_ref on
    sub_point_dofs() gives amg_levels()[0]["P"]: pointers and columns equal, values as uint64 bits."""
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    code = CHILD % (S.ROOT, S.HERE, HOST_CPU_SO, kind, N, geometric)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_restatement_details_on_built_inputs():
    """What the host builds never show: a refused row, the merge of equal columns, a dof without a point, values outside
    [0, num_dofs) -- on a tiny lattice whose answer is worked out by hand."""
    n, keep = 3, [0, 2]
    ref = np.array([-1.0, 0.25, 1.0])
    lo, hi, wl = R.interp_tables_ref(ref, keep)
    assert list(lo) == [0, 0, 1] and list(hi) == [0, 1, 1] and list(wl) == [1.0, 0.375, 1.0]
    # one element; dof 0 on every corner, dof 1 at the centre, dof 2 nowhere, the value 7 (>= num_dofs) on one mid-edge
    pd = np.full(27, -1)
    for c in (0, 2, 6, 8, 18, 20, 24, 26):
        pd[c] = 0
    pd[13] = 1
    pd[1] = 7
    g = R.geometric_level_ref(pd, 3, n, keep, lo, hi, wl)
    assert list(g["first"]) == [0, 13, R.INT_MAX] and list(g["kept"]) == [1, 0, 0] and list(g["flag"]) == [1, 0, 1]
    assert list(g["cmap"]) == [0, -1, 1] and g["unplaced"] == 1 and g["merged"] == 7 and not g["refused"]
    ptr, col, val = g["P"]
    assert list(ptr) == [0, 1, 2, 3] and list(col) == [0, 0, 1]
    w = np.float64(0.375)
    terms = [a * b * c for c in (w, 1 - w) for b in (w, 1 - w) for a in (w, 1 - w)]  # corner bit a = direction a, x fastest
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    assert list(val) == [1.0, s, 1.0]
    assert list(g["coarse_point_dof"]) == [0] * 8 and g["owner_dof"][0] == 0 and g["owner_dof"][13] == 1 and (g["owner_dof"] >= 0).sum() == 2
    # a kept node whose dof is not kept: only rows handed a cmap that is not their own chain's can see it
    rows, _ = R.interp_rows_ref(np.array([-1, -1, 1]), g["first"], pd, n, keep, lo, hi, wl)
    assert rows[0] is None and rows[1] is None and rows[2] == [(1, 1.0)]
    # from_triplets: stable by column, equal columns summed from the first one on
    ptr, col, val = R.from_triplets_ref(2, [1, 0, 1, 1, 1], [3, 2, 1, 3, 3], [1e16, 5.0, 2.0, 1.0, -1e16])
    assert list(ptr) == [0, 1, 3] and list(col) == [2, 1, 3] and list(val) == [5.0, 2.0, (np.float64(1e16) + 1.0) - 1e16]
    dp, dq = R.dof_points_ref(pd, 3)
    assert list(dp) == [0, 8, 9, 9] and list(dq) == [0, 2, 6, 8, 18, 20, 24, 26, 13]
