"""Surface weights and outward normals of element faces: the kernel entry fdd_field_surface (include/fdd_hip.h) against the
np.longdouble restatement of tests/boundary_checks.py (surface, on field_checks.geometry), and its refusals.

Bounds: area 1e-11 relative and normal 1e-11 absolute, the bound of tests/test_gpu_field_ops.py for the same contractions
(float64 against long double delivers 1e-13: tests/test_cpu_boundary.py).  On a box each side's areas sum to 1 and the normals
are +-e to 1e-13.  The closed-surface sum |sum area normal| is asked of the kernel only where the restatement itself holds
it to 1e-12 (tests/test_cpu_boundary.py establishes the meshes), and then to 1.3e-10: the restatement's 1e-12 plus the two
bounds above over a surface of total area 6.
"""
import numpy as np
import pytest
import torch

import boundary_checks as B
import field_checks as F
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

pytestmark = pytest.mark.gpu

# the degrees and meshes of tests/test_gpu_field_ops.py: every degree on the smallest Kershaw mesh it has, and a box
KINKED = (2, 4, 6, 10, 14)
CASES = [("kershaw", (2, 2, 2) if N in KINKED else (2, 1, 1), N) for N in range(1, 16)] + [("box", (3, 3, 1), 7)]
IDS = ["%s-%dx%dx%d-N%d" % ((kind,) + E + (N,)) for kind, E, N in CASES]


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class Device:
    def __init__(self, mesh, gpu):
        _, w, D = S.gll(mesh.N)
        self.xyz = [dev(c, gpu) for c in (mesh.x, mesh.y, mesh.z)]
        self.D, self.w = dev(D, gpu), dev(w, gpu)
        self.E, self.N, self.nn = mesh.num_local_elements, mesh.N, (mesh.N + 1) ** 2


def outputs(count, n, gpu, fill=0.0):
    pairs = [S.guarded(np.full(n, fill), torch.float64, gpu) for _ in range(count)]
    return [w for w, _ in pairs], [v for _, v in pairs]


def run(d, gpu, elem, side, normal=True):
    """(area, normal or None) of the listed faces, flat, from whole buffers between guard words"""
    m = len(elem)
    whole, out = outputs(4 if normal else 1, m * d.nn, gpu)
    k("fdd_field_surface", out[0], out[1:] if normal else None, d.xyz, d.D, d.w, dev(np.asarray(elem, np.int32), gpu), dev(np.asarray(side, np.int32), gpu), m, d.E, d.N)
    got = [host(t) for t in out]
    assert all(S.guards_stand(w) for w in whole)
    return got[0], (np.stack(got[1:]) if normal else None)


@pytest.mark.parametrize("kind,E,N", CASES, ids=IDS)
def test_kernel_against_the_long_double_restatement(gpu, kind, E, N):
    mesh = F.mesh_of(kind, E, N)
    ref = B.restated_surface(mesh)
    d = Device(mesh, gpu)
    m, n = len(ref["elem"]), N + 1
    want_a, want_n = ref["area"].reshape(-1), ref["normal"].reshape(3, -1)

    # every face of the surface in one call: many workgroups, all six sides
    area, normal = run(d, gpu, ref["elem"], ref["side"])
    rel, err = float(np.abs(area / want_a - 1).max()), float(np.abs(normal - want_n).max())
    print("area %.2e relative, normal %.2e" % (rel, err))
    assert set(ref["side"].tolist()) == set(range(6)) and rel <= 1e-11 and err <= 1e-11 and (area > 0).all()

    # one face per call, one of every side, with and without the normal: the bits of the call over all
    for s in range(6):
        f = int(np.flatnonzero(ref["side"] == s)[-1])
        one_a, one_n = run(d, gpu, ref["elem"][f : f + 1], ref["side"][f : f + 1])
        sl = slice(f * n * n, (f + 1) * n * n)
        assert np.array_equal(one_a, area[sl]) and np.array_equal(one_n, normal[:, sl]), s
        assert np.array_equal(run(d, gpu, ref["elem"][f : f + 1], ref["side"][f : f + 1], normal=False)[0], area[sl]), s

    closed_ref = max(abs(float((ref["area"] * ref["normal"][c]).sum())) for c in range(3))
    if closed_ref <= 1e-12:
        closed = max(abs(float((area * normal[c]).sum())) for c in range(3))
        print("closed surface: %.2e (restatement %.1e)" % (closed, closed_ref))
        assert closed <= 1.3e-10
    if kind == "box":
        sides = np.repeat(ref["side"], n * n)
        assert max(abs(float(area[sides == s].sum()) - 1.0) for s in range(6)) <= 1e-13
        want = np.zeros_like(normal)
        for s in range(6):
            want[s // 2, sides == s] = 1.0 if s % 2 else -1.0
        assert np.abs(normal - want).max() <= 1e-13


def test_a_face_outside_the_arrays_is_skipped(gpu):
    """the caller validates the list; an element or side out of range is left alone, not read"""
    mesh = F.mesh_of("kershaw", (2, 1, 1), 3)
    d = Device(mesh, gpu)
    whole, out = outputs(4, 4 * d.nn, gpu, fill=5.0)
    k("fdd_field_surface", out[0], out[1:], d.xyz, d.D, d.w, dev(np.array([0, 2, -1, 1], np.int32), gpu), dev(np.array([6, 0, 0, -1], np.int32), gpu), 4, d.E, d.N)
    assert all(bool((host(t) == 5.0).all()) for t in out) and all(S.guards_stand(w) for w in whole)


def refused(code, *args):
    with pytest.raises(lib.FddError) as exc:
        k("fdd_field_surface", *args)
    assert "failed with code %d:" % code in str(exc.value), str(exc.value)


def test_refusals_touch_nothing(gpu):
    mesh = F.mesh_of("kershaw", (2, 1, 1), 3)
    ref = B.restated_surface(mesh)
    d = Device(mesh, gpu)
    m = len(ref["elem"])
    fe, fs = dev(ref["elem"], gpu), dev(ref["side"], gpu)
    whole, o = outputs(4, m * d.nn, gpu, fill=5.0)
    UNSUPPORTED, INVALID = -2, -1
    for N_bad in (0, 16, -3):  # the degree first: every other bound divides by it
        refused(UNSUPPORTED, o[0], o[1:], d.xyz, d.D, d.w, fe, fs, m, d.E, N_bad)
        refused(UNSUPPORTED, None, None, None, None, None, None, None, -1, -1, N_bad)
    refused(INVALID, o[0], o[1:], d.xyz, d.D, d.w, fe, fs, -1, d.E, d.N)
    refused(INVALID, o[0], o[1:], d.xyz, d.D, d.w, fe, fs, m, -1, d.N)
    refused(INVALID, o[0], o[1:], d.xyz, d.D, d.w, fe, fs, m, 0, d.N)  # faces of no element
    refused(INVALID, o[0], o[1:], d.xyz, d.D, d.w, fe, fs, 2**31 // 16, d.E, d.N)
    for missing in range(7):
        args = [o[0], o[1:], d.xyz, d.D, d.w, fe, fs]
        if missing == 1:
            args[1] = [o[1], None, o[3]]
        elif missing == 2:
            args[2] = [d.xyz[0], None, d.xyz[2]]
        else:
            args[missing] = None
        refused(INVALID, *args, m, d.E, d.N)
    # an output that is an input, or another output
    refused(INVALID, d.xyz[1], o[1:], d.xyz, d.D, d.w, fe, fs, m, d.E, d.N)
    refused(INVALID, o[0], [o[1], d.xyz[2], o[3]], d.xyz, d.D, d.w, fe, fs, m, d.E, d.N)
    refused(INVALID, o[0], [o[1], o[2], o[1]], d.xyz, d.D, d.w, fe, fs, m, d.E, d.N)
    refused(INVALID, o[0], [o[1], o[0], o[3]], d.xyz, d.D, d.w, fe, fs, m, d.E, d.N)
    refused(INVALID, d.D, None, d.xyz, d.D, d.w, fe, fs, m, d.E, d.N)
    refused(INVALID, o[0], [o[1], o[2], d.w], d.xyz, d.D, d.w, fe, fs, m, d.E, d.N)
    refused(INVALID, fe, None, d.xyz, d.D, d.w, fe, fs, m, d.E, d.N)
    # no faces: nothing to do, nothing read
    k("fdd_field_surface", o[0], o[1:], d.xyz, d.D, d.w, fe, fs, 0, d.E, d.N)
    k("fdd_field_surface", None, None, None, None, None, None, None, 0, 0, d.N)
    assert all(S.guards_stand(w) for w in whole) and all(bool((host(t) == 5.0).all()) for t in o)
    assert np.array_equal(host(d.xyz[1]), mesh.y) and np.array_equal(host(fe), ref["elem"]) and np.array_equal(host(d.D), S.gll(3)[2])
