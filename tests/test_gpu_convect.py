"""The convection term c . grad u on the solver's mesh: the kernel entries (include/fdd_hip.h: fdd_field_convect,
fdd_field_weak_convect) against the np.longdouble restatement of tests/convect_checks.py, and the host entries
(include/fdd_host.h: fddh_convect, fddh_weak_convect, fddh_convect_quadrature; Problem.convect / weak_convect / quadrature).

Bounds: 1e-11 T_c and 1e-11 T_wc, the project's bar for the field operators (tests/test_cpu_convect.py: the restatement in
float64 stays within 2.9e-14 T_c and 3.3e-16 T_wc of the long double one; a wrong slot of P', a dropped direction or the
collocated form is an error of 1e-3 T and more), |convect(c, a.X + b) - c.a| 1e-10, the skew-symmetry sums 1e-13 of the sum of
the absolute terms (the project's bar for dots).

Worst figures measured on an MI355X (each test prints its own): convect 6.7e-14 T_c, against c . gradient 2.0e-16 T_c, linear
field 4.7e-13, weak_convect 5.8e-17 T_wc against the restatement and against the exact integral on the box, skew symmetry
3.9e-17 and the sum 2.1e-16 of the absolute terms.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import convect_checks as C
import field_checks as F
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

pytestmark = pytest.mark.gpu

# Every mesh at N = 1, 2, 7 (a wave is an element), 8 (the first past a wave) and 15: one element, and a count above what a
# workgroup holds that is no multiple of it (256 lanes hold 64 elements at N = 1, 4 at N = 7, 1 at N = 15).  The Kershaw map
# has no one-element mesh at N = 2 -- its kink falls on the centre node, where the isoparametric Jacobian is not positive, and
# support.KershawMesh refuses it --, so that case takes (2,2,2).  Then the remaining degrees on two Kershaw elements ((2,2,2)
# at the degrees with a centre node across the kink), so that every instance of both kernels runs
KINKED = (2, 4, 6, 10, 14)
COUNTS = {1: (4, 4, 5), 7: (3, 1, 3), 15: (3, 1, 1)}
CASES = [(kind, (2, 2, 2) if (kind, N) == ("kershaw", 2) else (1, 1, 1), N) for kind in ("box", "kershaw", "deformed") for N in (1, 2, 7, 8, 15)]
CASES += [(kind, COUNTS[N], N) for kind in ("box", "kershaw", "deformed") for N in (1, 7, 15)]
CASES += [("kershaw", (2, 2, 2) if N in KINKED else (2, 1, 1), N) for N in range(1, 16) if N not in (1, 2, 7, 8, 15)]
IDS = ["%s-%dx%dx%d-N%d" % ((kind,) + E + (N,)) for kind, E, N in CASES]
# fdd_field_weak_convect has an instance at every degree: none is refused, so none is left out here
assert sorted({N for _, _, N in CASES}) == list(range(1, 16))


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def output(n, gpu):
    whole, vec = S.guarded(np.zeros(n), torch.float64, gpu)
    return whole, vec


@functools.lru_cache(maxsize=None)
def reference(kind, E, N):
    """the mesh, its long double geometry, the seeded fields, the two operators of the restatement and their scales"""
    mesh = F.mesh_of(kind, E, N)
    ref = F.geometry(mesh, np.longdouble)
    c, u = C.fields(mesh, 700 + N)
    return mesh, ref, c, u, C.convect(ref, c, u), C.convect_scale(ref, c, u), C.weak_convect(ref, c, u), C.weak_convect_scale(ref, c, u)


class Device:
    """a mesh's coordinates, D_hat and the quadrature tables (the long double ones, rounded) on the GPU"""

    def __init__(self, mesh, gpu, D=None):
        D = S.gll(mesh.N)[2] if D is None else D
        z, w, P, Pd = C.tables(mesh.N, np.longdouble, D)
        self.xyz = [dev(a, gpu) for a in (mesh.x, mesh.y, mesh.z)]
        self.D, self.P, self.Pd, self.w, self.M = dev(D, gpu), dev(P, gpu), dev(Pd, gpu), dev(w, gpu), len(w)
        self.E, self.N, self.n = mesh.num_local_elements, mesh.N, mesh.num_local_points

    def convect(self, out, c, u):
        k("fdd_field_convect", out, c, u, self.xyz, self.D, self.E, self.N)

    def weak_convect(self, out, c, u):
        k("fdd_field_weak_convect", out, c, u, self.xyz, self.D, self.P, self.Pd, self.w, self.M, self.E, self.N)


@pytest.mark.parametrize("kind,E,N", CASES, ids=IDS)
def test_kernel_entries_against_the_long_double_restatement(gpu, kind, E, N):
    mesh, ref, c, u, want, Tc, want_weak, Twc = reference(kind, E, N)
    d = Device(mesh, gpu)
    cd, ud = [dev(a, gpu) for a in c], dev(u, gpu)

    whole, out = output(d.n, gpu)
    d.convect(out, cd, ud)
    got = host(out)
    err = float(np.abs(got - want).max())
    print("convect: %.2e T_c" % (err / Tc))
    assert S.guards_stand(whole) and err <= 1e-11 * Tc

    # the same from the gradient kernel's components
    grad = [torch.zeros(d.n, dtype=torch.float64, device=gpu) for _ in range(3)]
    k("fdd_field_gradient", grad, ud, d.xyz, d.D, d.E, N)
    by_gradient = sum(np.asarray(c[a], dtype=np.longdouble) * host(grad[a]) for a in range(3))
    err = float(np.abs(got - by_gradient).max())
    print("convect against c . gradient: %.2e T_c" % (err / Tc))
    assert err <= 1e-11 * Tc

    # a linear field: c . a at every point of any mesh whose map the elements represent
    whole, out = output(d.n, gpu)
    d.convect(out, cd, dev(F.linear_field(mesh), gpu))
    err = float(np.abs(host(out) - sum(F.LINEAR[a] * c[a] for a in range(3))).max())
    print("convect of a linear field: %.2e" % err)
    assert S.guards_stand(whole) and err <= 1e-10

    whole, out = output(d.n, gpu)
    d.weak_convect(out, cd, ud)
    err = float(np.abs(host(out) - want_weak).max())
    print("weak_convect: %.2e T_wc" % (err / Twc))
    assert S.guards_stand(whole) and err <= 1e-11 * Twc


@pytest.mark.parametrize("kind,E,N", [c for c in CASES if c[0] == "box"], ids=[i for c, i in zip(CASES, IDS) if c[0] == "box"])
def test_weak_convect_is_the_exact_integral_on_the_box(gpu, kind, E, N):
    """against 2n+2 Gauss points in long double; by tests/test_cpu_convect.py the collocated form misses that by 4e-3 T_wc and more"""
    mesh, ref, c, u, _, _, _, Twc = reference(kind, E, N)
    exact = C.weak_convect(ref, c, u, M=2 * (N + 1) + 2)
    d = Device(mesh, gpu)
    whole, out = output(d.n, gpu)
    d.weak_convect(out, [dev(a, gpu) for a in c], dev(u, gpu))
    err = float(np.abs(host(out) - exact).max())
    print("weak_convect against the exact integral: %.2e T_wc" % (err / Twc))
    assert S.guards_stand(whole) and err <= 1e-11 * Twc


def refused(name, code, *args):
    with pytest.raises(lib.FddError) as exc:
        k(name, *args)
    assert "failed with code %d:" % code in str(exc.value), str(exc.value)


def test_kernel_entries_refuse_before_they_touch_an_output(gpu):
    mesh = F.mesh_of("kershaw", (2, 1, 1), 3)
    d = Device(mesh, gpu)
    c0, u0 = C.fields(mesh, 5)
    c, u = [dev(a, gpu) for a in c0], dev(u0, gpu)
    whole, out = output(d.n, gpu)
    out.fill_(5.0)
    UNSUPPORTED, INVALID = -2, -1
    for N_bad in (0, 16):
        refused("fdd_field_convect", UNSUPPORTED, out, c, u, d.xyz, d.D, d.E, N_bad)
        refused("fdd_field_weak_convect", UNSUPPORTED, out, c, u, d.xyz, d.D, d.P, d.Pd, d.w, (3 * (N_bad + 1) + 1) // 2, d.E, N_bad)
    # the degree is looked at before the count
    refused("fdd_field_convect", UNSUPPORTED, out, c, u, d.xyz, d.D, -1, 16)
    refused("fdd_field_convect", INVALID, out, c, u, d.xyz, d.D, -1, d.N)
    refused("fdd_field_weak_convect", INVALID, out, c, u, d.xyz, d.D, d.P, d.Pd, d.w, d.M, -1, d.N)
    # a wrong number of quadrature points
    for M_bad in (d.M - 1, d.M + 1, d.n, 0):
        refused("fdd_field_weak_convect", INVALID, out, c, u, d.xyz, d.D, d.P, d.Pd, d.w, M_bad, d.E, d.N)
    # an output that is an input
    for o in (c[1], u, d.xyz[2], d.D):
        refused("fdd_field_convect", INVALID, o, c, u, d.xyz, d.D, d.E, d.N)
    for o in (c[0], u, d.xyz[1], d.D, d.P, d.Pd, d.w):
        refused("fdd_field_weak_convect", INVALID, o, c, u, d.xyz, d.D, d.P, d.Pd, d.w, d.M, d.E, d.N)
    # a null pointer
    refused("fdd_field_convect", INVALID, None, c, u, d.xyz, d.D, d.E, d.N)
    refused("fdd_field_convect", INVALID, out, [c[0], None, c[2]], u, d.xyz, d.D, d.E, d.N)
    refused("fdd_field_convect", INVALID, out, c, None, d.xyz, d.D, d.E, d.N)
    refused("fdd_field_convect", INVALID, out, c, u, [d.xyz[0], d.xyz[1], None], d.D, d.E, d.N)
    refused("fdd_field_convect", INVALID, out, c, u, d.xyz, None, d.E, d.N)
    for at in range(8):
        args = [out, c, u, d.xyz, d.D, d.P, d.Pd, d.w]
        args[at] = None
        refused("fdd_field_weak_convect", INVALID, *args, d.M, d.E, d.N)
    # no elements: nothing to do, nothing read
    k("fdd_field_convect", out, c, u, d.xyz, d.D, 0, d.N)
    k("fdd_field_weak_convect", out, c, u, d.xyz, d.D, d.P, d.Pd, d.w, d.M, 0, d.N)
    assert S.guards_stand(whole) and bool((out == 5.0).all())
    assert np.array_equal(host(d.xyz[1]), mesh.y) and np.array_equal(host(u), u0) and np.array_equal(host(c[1]), c0[1])


# ---- through the problem ----
@pytest.fixture(scope="module")
def setup(gpu):
    H.init(0)
    H.comm_single()
    H.set_print(False)
    return True


def golden_tables(p):
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])


@pytest.mark.parametrize("N", (2, 7, 8))
def test_weak_convect_is_skew_symmetric_for_a_solenoidal_velocity(setup, N):
    """c = (y - 1/2, 1/2 - x, 0) on the 2^3-element box, u and phi continuous and zero on the boundary: the integral of
    phi c . grad u + u c . grad phi = c . grad(u phi) vanishes, and so does the integral of c . grad u"""
    p = H.Problem.box((2, 2, 2), (1, 1, 1), N, 2, False)
    try:
        golden_tables(p)
        x, y = p.mesh_array("x"), p.mesh_array("y")
        c = (y - 0.5, 0.5 - x, np.zeros(p.n))
        u, phi = (p.dssum(S.seeded_uniform(p.n, seed) - 0.5, mask=True, weight=True) for seed in (21, 22))
        wu, wphi = p.weak_convect(*c, u), p.weak_convect(*c, phi)
        both, scale = float((phi * wu).sum() + (u * wphi).sum()), float(np.abs(phi * wu).sum() + np.abs(u * wphi).sum())
        total, total_scale = float(wu.sum()), float(np.abs(wu).sum())
        print("N = %d: skew symmetry %.2e of the absolute terms, sum %.2e" % (N, abs(both) / scale, abs(total) / total_scale))
        assert scale > 0 and abs(both) <= 1e-13 * scale
        assert total_scale > 0 and abs(total) <= 1e-13 * total_scale
    finally:
        p.close()


@pytest.mark.parametrize("kind", ("box", "kershaw"))
def test_both_operators_follow_set_D_hat(setup, kind):
    p = H.Problem.box((2, 3, 2), (1, 1, 1), 7, 2, False) if kind == "box" else H.Problem.kershaw((6, 2, 2), (1, 1, 1), 7, 2, with_subdomain=False)
    try:
        golden_tables(p)
        mesh = S.ArrayMesh.from_problem(p)
        c, u = C.fields(mesh, 40)
        D = np.asarray(S.gll(mesh.N)[2])
        other = D * (1.0 + 1e-3 * (S.seeded_uniform(len(D), 9) - 0.5))
        p.weak_convect(*c, u)  # the tables of the first table are in place when it changes
        p.set_D_hat(0, other)
        ref, moved = F.geometry(mesh, np.longdouble), F.geometry(mesh, np.longdouble, D_hat=other)
        for name, op, scale in (("convect", C.convect, C.convect_scale), ("weak_convect", C.weak_convect, C.weak_convect_scale)):
            T = scale(moved, c, u)
            want, before = op(moved, c, u), op(ref, c, u)
            err = float(np.abs(getattr(p, name)(*c, u) - want).max())
            print("%s after set_D_hat: %.2e T, the tables differ by %.2e T" % (name, err / T, float(np.abs(want - before).max()) / T))
            assert err <= 1e-11 * T
            assert float(np.abs(want - before).max()) >= 1e-6 * T  # the two tables are told apart
        # and back
        p.set_D_hat(0, D)
        assert float(np.abs(p.weak_convect(*c, u) - C.weak_convect(ref, c, u)).max()) <= 1e-11 * C.weak_convect_scale(ref, c, u)
    finally:
        p.close()


def test_two_dimensional_problem_is_refused_and_stays_usable(setup, tmp_path):
    E, N = (3, 2), 4
    S.write_mesh_files(str(tmp_path), S.QuadMesh(E, N, amplitude=0.05))
    p = H.Problem.from_directory(str(tmp_path), N, 2, with_subdomain=False)
    try:
        golden_tables(p)
        u = S.seeded_uniform(p.n, 3)
        before = p.stiffness(u)
        for call in (lambda: p.convect(u, u, u, u), lambda: p.weak_convect(u, u, u, u)):
            with pytest.raises(lib.FddError) as exc:
                call()
            assert "3-D only" in str(exc.value) and "2-D" in str(exc.value)
        assert np.array_equal(p.stiffness(u), before) and np.abs(before).max() > 0
    finally:
        p.close()


def test_quadrature_is_the_cpu_host_librarys_bit_for_bit(setup):
    """the tables need no kernel: the host layer built on the CPU stand-in of the kernel library hands out the same ones"""
    shim = os.path.join(S.HERE, "cpu_shim")
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", shim, "-s"])
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "convect_refusals.py"), os.path.join(shim, "_build", "libfdd_host_cpu.so")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    tables = json.loads(out.stdout.strip().splitlines()[-1])["tables"]
    for N in (1, 2, 7, 8, 15):
        p = H.Problem.box((1, 1, 1), (1, 1, 1), N, 1, False)
        try:
            assert np.array_equal(p.get_D_hat(0), np.array(tables[str(N)]["D"]))
            for name, got in zip(("z", "w", "P", "Pd"), p.quadrature()):
                assert np.array_equal(got.reshape(-1), np.array(tables[str(N)][name])), (N, name)
        finally:
            p.close()
