"""Neumann and Robin faces of the generated meshes (include/fdd_host.h: fddh_boundary_*, fddh_problem_create_box_faces; DESIGN
section 15): the restatements the tests share, and the checks that run on the CPU stand-in of the kernel C-ABI as
`python tests/boundary_checks.py <libfdd_host_cpu.so> <check>` (tests/test_cpu_boundary.py), one child process each;
`... write <dir> <Ex,Ey,Ez> <Px,Py,Pz> <N> <rank> <faces|-> <eps>` writes one rank's mesh files through the host layer.

Restatements
  face_list / face_points  every element face on the surface of the box, sorted by (side, element), from the coordinates alone,
                           and the index of its points in a point vector ((a, b) = (j, k), (i, k), (i, j) on x-, y-, z-faces)
  surface                  area = w_a w_b |Nvec| and normal = +-Nvec / |Nvec| from the Jacobian of field_checks.geometry, in
                           any float type: np.longdouble is what fdd_field_surface is held to
  Reference                the assembled SEM matrix of a mesh with its mask, kappa, lambda and a Robin diagonal over ALL nodes
                           (scipy sparse; dense below 3 000 nodes), the solve with Dirichlet and flux data, and the maps between
                           point and node vectors.  Nodes are the distinct glo_num, in ascending order
The manufactured solution is u = sin(4x + 3y + 2z + 0.3): no symmetry of the box, no face on which u or its flux vanishes.

The preconditioner's pieces on natural faces (check_inner_operator, check_level0_matrix, check_against_oracle, further down)
are held to Reference.K_free(), to the restatements of tests/amg_setup_restatements.py and to the oracle; the GPU runs them
with every term (tests/test_gpu_boundary_preconditioner.py), the CPU stand-in without lambda and alpha.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

TAU = 1e-10
MAX_ITERATIONS = 500
DENSE_BELOW = 3000


def api():
    import support as S
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

    return S, H, lib


# ---------------------------------------------------------------- the mask and the faces
def face_mask(mesh, faces):
    """p_mask of the codes: 0 on every point of a 'D' face (the coordinates of the cube's faces are exact)"""
    assert len(faces) == 6 and set(faces) <= {"D", "N"}
    on = [mesh.x == 0.0, mesh.x == 1.0, mesh.y == 0.0, mesh.y == 1.0, mesh.z == 0.0, mesh.z == 1.0]
    masked = np.zeros(len(mesh.x), bool)
    for s in range(6):
        if faces[s] == "D":
            masked |= on[s]
    return np.where(masked, 0.0, 1.0)


def face_points(elem, side, n):
    """(m, n, n) indices [f, b, a] of the face points in a point vector"""
    elem, side = np.asarray(elem, np.int64), np.asarray(side, np.int64)
    b, a = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    fixed = np.where(side % 2 == 1, n - 1, 0)[:, None, None]
    axis = (side // 2)[:, None, None]
    in_elem = np.where(axis == 0, fixed + n * (a + n * b), np.where(axis == 1, a + n * (fixed + n * b), a + n * (b + n * fixed)))
    return elem[:, None, None] * n**3 + in_elem


def face_list(mesh):
    """(elem, side) of every element face that lies in a face of the unit cube, sorted by (side, element)"""
    n = mesh.N + 1
    elem, side = [], []
    coords = (mesh.x, mesh.y, mesh.z)
    for s in range(6):
        c, want = coords[s // 2], float(s % 2)
        for e in range(mesh.num_local_elements):
            pts = face_points([e], [s], n).reshape(-1)
            if np.abs(c[pts] - want).max() <= 1e-12:
                elem.append(e), side.append(s)
    return np.array(elem, np.int32), np.array(side, np.int32)


def surface(g, elem, side):
    """(area (m, n, n), normal (3, m, n, n)) in g.dtype from the Jacobian of field_checks.geometry: Nvec = X_s x X_t on
    r-faces, X_t x X_r on s-faces, X_r x X_s on t-faces; + on the upper side"""
    n = g.n
    pts = face_points(elem, side, n)
    col = lambda b: [g.J[a][b].reshape(-1)[pts] for a in range(3)]  # X_r, X_s, X_t at the face points
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    Xr, Xs, Xt = col(0), col(1), col(2)
    per_axis = [cross(Xs, Xt), cross(Xt, Xr), cross(Xr, Xs)]
    axis = (np.asarray(side) // 2)[:, None, None]
    N = [np.where(axis == 0, per_axis[0][c], np.where(axis == 1, per_axis[1][c], per_axis[2][c])) for c in range(3)]
    mag = np.sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2])
    ww = (g.w[:, None] * g.w[None, :])[None, :, :]
    sign = np.where(np.asarray(side) % 2 == 1, 1.0, -1.0).astype(g.dtype)[:, None, None]
    return ww * mag, np.stack([sign * N[c] / mag for c in range(3)])


def restated_surface(mesh, dtype=np.longdouble):
    """the dict of Problem.surface() from the restatement (area and normal in dtype)"""
    import field_checks as F

    elem, side = face_list(mesh)
    area, normal = surface(F.geometry(mesh, dtype), elem, side)
    return {"elem": elem, "side": side, "points": face_points(elem, side, mesh.N + 1), "area": area, "normal": normal}


# ---------------------------------------------------------------- the manufactured solution
def exact(x, y, z):
    return np.sin(4.0 * x + 3.0 * y + 2.0 * z + 0.3)


def exact_gradient(x, y, z):
    c = np.cos(4.0 * x + 3.0 * y + 2.0 * z + 0.3)
    return [4.0 * c, 3.0 * c, 2.0 * c]


def kappa_smooth(x, y, z):
    return 1.0 + x + 2.0 * y * y


def source(x, y, z, lam=0.0, kappa=False):
    """-div(kappa grad u) + lam u; kappa False: 1, True: kappa_smooth, whose gradient is (1, 4y, 0)"""
    u, c = exact(x, y, z), np.cos(4.0 * x + 3.0 * y + 2.0 * z + 0.3)
    if not kappa:
        return (29.0 + lam) * u
    return 29.0 * kappa_smooth(x, y, z) * u - (4.0 + 12.0 * y) * c + lam * u


def exact_flux(surf, x, y, z, alpha=None, kappa=None):
    """kappa du/dn + alpha u at the face points, (m, n, n): the natural datum of the exact solution"""
    pts = surf["points"]
    g = exact_gradient(x[pts], y[pts], z[pts])
    dudn = sum(np.asarray(surf["normal"][a], np.float64) * g[a] for a in range(3))
    if kappa is not None:
        dudn = kappa[pts] * dudn
    return dudn + (0.0 if alpha is None else alpha * exact(x[pts], y[pts], z[pts]))


def side_alpha(surf, mask, values):
    """alpha (m, n, n): values[side] on the free points of the faces of that side, 0 elsewhere"""
    alpha = np.zeros(surf["points"].shape)
    for side, v in values.items():
        alpha[surf["side"] == side] = v
    return alpha * (mask[surf["points"]] != 0.0)


# ---------------------------------------------------------------- the assembled matrix
class Reference:
    """K = Qt D^T [kappa G] D Q + diag(Qt (lam B + r)) over all nodes of `mesh` (its arrays g, glo_num, p_mask; D the golden
    table of its degree), r[q] = sum alpha area over the face entries at q"""

    def __init__(self, mesh, kappa=None, lam=0.0, alpha=None, surf=None):
        import scipy.sparse as sp

        import diffusivity_checks as DC
        import field_checks as F
        import support as S

        self.mesh, n = mesh, mesh.N + 1
        ids, self.node = np.unique(mesh.glo_num, return_inverse=True)
        self.nn = len(ids)
        D = np.asarray(S.gll(mesh.N)[2], np.float64).reshape(n, n)
        G = [np.asarray(a, np.float64) * (1.0 if kappa is None else kappa) for a in mesh.g]
        self.B = np.asarray(F.mass(F.geometry(mesh, np.float64)), np.float64)
        self.r = np.zeros(len(self.node))
        if alpha is not None:
            np.add.at(self.r, surf["points"].reshape(-1), (alpha * np.asarray(surf["area"], np.float64)).reshape(-1))
        self.cbar = np.bincount(self.node, weights=lam * self.B + self.r, minlength=self.nn)
        self.K = (DC.assemble(G, D, n, self.node, self.nn) + sp.diags(self.cbar)).tocsr()
        self.free = np.bincount(self.node, weights=np.asarray(mesh.p_mask, np.float64), minlength=self.nn) > 0
        self.lam = lam
        xyz = [np.zeros(self.nn) for _ in range(3)]
        for c, a in zip(xyz, (mesh.x, mesh.y, mesh.z)):
            c[self.node] = a
        self.exact = exact(*xyz)

    def assembled(self, f):
        return np.bincount(self.node, weights=f, minlength=self.nn)

    def on_nodes(self, u):
        out = np.zeros(self.nn)
        out[self.node] = u
        return out

    def rhs(self, f, u_D=None, flux=None, surf=None):
        """the node right-hand side on the free nodes: f^ - K u_D^ + Qt scatter(area flux)"""
        fh = self.assembled(f)
        if flux is not None:
            t = np.zeros(len(self.node))
            np.add.at(t, surf["points"].reshape(-1), (np.asarray(surf["area"], np.float64) * flux).reshape(-1))
            fh = fh + self.assembled(t)
        if u_D is not None:
            fh = fh - self.K @ self.on_nodes(u_D)
        return fh[self.free]

    def K_free(self):
        return self.K[self.free][:, self.free]

    def solve(self, fh_free, u_D=None):
        """the node solution over all nodes"""
        Kf = self.K_free()
        if self.nn < DENSE_BELOW:
            uf = np.linalg.solve(Kf.toarray(), fh_free)
        else:
            import scipy.sparse.linalg as spl

            uf = spl.spsolve(Kf.tocsc(), fh_free)
        u = np.zeros(self.nn) if u_D is None else self.on_nodes(u_D)
        u[self.free] = uf
        return u


def problem_data(mesh, surf, lam=0.0, alpha=None, kappa=None):
    """(f, u_D, flux) of the exact solution at the points of `mesh`: f = B s, u_D = u on the masked points, flux = kappa du/dn
    + alpha u on every face point (what falls on masked points is never read)"""
    import field_checks as F

    x, y, z = mesh.x, mesh.y, mesh.z
    B = np.asarray(F.mass(F.geometry(mesh, np.float64)), np.float64)
    f = B * source(x, y, z, lam, kappa is not None)
    u_D = np.where(np.asarray(mesh.p_mask) == 0.0, exact(x, y, z), 0.0)
    return f, u_D, exact_flux(surf, x, y, z, alpha, kappa)


def dense_error(N, faces, alpha_sides=None, E=(2, 2, 2), lam=0.0):
    """max |u_h - u| over the nodes of the dense solve on the E box at degree N with the face codes and a Robin coefficient
    per side, all data from the exact solution: the discretisation's own error"""
    import support as S

    mesh = S.BoxMesh(E, N)
    mesh.p_mask = face_mask(mesh, faces)
    surf = restated_surface(mesh)
    alpha = side_alpha(surf, mesh.p_mask, alpha_sides) if alpha_sides else None
    ref = Reference(mesh, None, lam, alpha, surf)
    f, u_D, flux = problem_data(mesh, surf, lam, alpha)
    u = ref.solve(ref.rhs(f, u_D, flux, surf), u_D)
    return float(np.abs(u - ref.exact).max())


# ---------------------------------------------------------------- checks on the CPU stand-in (child processes)
SETTINGS = {"none": 0, "jacobi": 2, "vcycle": 1}  # flag sub_use_preconditioner: the inner GMRES alone, with Jacobi, with the V-cycle


def new_problem(E, N, faces, kind="box", **kw):
    S, H, _ = api()
    p = (H.Problem.box if kind == "box" else H.Problem.kershaw)(E, (1, 1, 1), poly_degree=N, poly_reduction=2 if N > 2 else 1, with_subdomain=True, faces=faces, **kw)
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
    return p


def check_solves(N):
    """DNDNDN on the 2^3 box with inhomogeneous Dirichlet and Neumann data, the surface weights from the restatement (the
    stand-in has no fdd_field_surface): the three preconditioner settings and both outer methods against the dense matrix"""
    S, H, _ = api()
    faces = "DNDNDN"
    p = new_problem((2, 2, 2), N, faces)
    try:
        p.set_options(max_iterations=MAX_ITERATIONS, tolerance=TAU)
        mesh = S.ArrayMesh.from_problem(p)
        assert np.array_equal(mesh.p_mask, face_mask(mesh, faces))
        surf = restated_surface(mesh)
        ref = Reference(mesh)
        f, u_D, flux = problem_data(mesh, surf)
        scattered = np.zeros(p.n)
        np.add.at(scattered, surf["points"].reshape(-1), (np.asarray(surf["area"], np.float64) * flux).reshape(-1))
        f_prime = f - p.stiffness(u_D) + scattered
        fh = ref.rhs(f, u_D, flux, surf)
        dense = ref.solve(fh, u_D)
        dense_err = float(np.abs(dense - ref.exact).max())
        print("solves N = %d: error of the dense solve against the exact solution %.6e" % (N, dense_err))
        Kf = ref.K_free()
        for setting, value in SETTINGS.items():
            p.set_flag("sub_use_preconditioner", value)
            for method in ("fcg", "gmres"):
                u, its, hist = p.solve(f_prime, method)
                un = ref.on_nodes(u + u_D)
                ratio = float(np.linalg.norm(fh - Kf @ un[ref.free]) / (TAU * np.linalg.norm(fh)))
                err = float(np.abs(un - ref.exact).max())
                print("solves N = %d %s %s: %d iterations, true residual %.3f tau |f^|, error %.6f x the dense solve's" % (N, setting, method, its, ratio, err / dense_err))
                assert its < MAX_ITERATIONS and hist[-1] <= TAU * hist[0], (setting, method, its)
                assert ratio <= 10.0 and err <= 1.05 * dense_err, (setting, method, ratio, err / dense_err)
    finally:
        p.close()


def check_singular():
    """NNNNNN can be created; solve, pcg_begin and precond_apply refuse it, naming the remedies; the operator still applies"""
    S, H, lib = api()
    p = new_problem((2, 2, 2), 3, "NNNNNN")
    try:
        assert p.boundary_info()["faces"] == "NNNNNN" and p.mesh_array("p_mask").min() == 1.0
        u = S.seeded_uniform(p.n, 3)
        before = p.stiffness(u)
        f = p.stiffness(p.dssum(u, mask=False, weight=True))
        for call in (lambda: p.solve(f), lambda: p.solve(f, "gmres"), lambda: p.solve_timed(f), lambda: p.solve_projected(f), lambda: p.pcg_begin(f), lambda: p.precond_apply(f)):
            try:
                call()
            except lib.FddError as exc:
                text = str(exc)
                assert "singular" in text and "'D' face" in text and "fddh_helmholtz_set" in text and "fddh_boundary_robin_set" in text, text
                print("refused:", text.split(": ", 1)[1][:60])
            else:
                raise AssertionError("a singular problem was solved")
        assert np.array_equal(p.stiffness(u), before) and np.abs(before).max() > 0
        ones = p.stiffness(np.ones(p.n))
        print("singular: |A 1| = %.2e max|A u|" % (np.abs(ones).max() / np.abs(before).max()))
        assert np.abs(ones).max() <= 1e-12 * np.abs(before).max()  # the constants are in the null space: why it is refused
    finally:
        p.close()


def check_missing_entries():
    """the stand-in has no fdd_field_surface: surface and robin_set say so and the problem stays usable"""
    S, H, lib = api()
    import ctypes

    p = new_problem((2, 2, 2), 3, "DNDNDN")
    try:
        info = p.boundary_info()
        assert info["num_faces"] == 24 and not info["robin_active"] and info["shift_support"] == 0, info
        m, n = info["num_faces"], 4
        elem, side = np.zeros(m, np.int32), np.zeros(m, np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        lib.host().call("fddh_boundary_faces", p.h, elem.ctypes.data_as(ip), side.ctypes.data_as(ip), m)
        want = face_list(S.ArrayMesh.from_problem(p))
        assert np.array_equal(elem, want[0]) and np.array_equal(side, want[1])
        area, alpha = np.zeros((m, n, n)), np.zeros((m, n, n))
        alpha[side == 1] = 2.0
        L = lib.host()
        for name, args in (("fddh_boundary_surface", (p.h, area.ctypes.data, None, None, None, ctypes.c_longlong(area.size))), ("fddh_boundary_robin_set", (p.h, alpha.ctypes.data))):
            rc = L.raw(name)(*args)
            text = L.raw("fddh_last_error")().decode()
            print("refused: %s: %s" % (name, text))
            assert rc != 0 and "fdd_field_surface" in text and "does not export" in text, (name, rc, text)
        rc = L.raw("fddh_problem_set_flag")(p.h, b"indexed_shift", 1)
        text = L.raw("fddh_last_error")().decode()
        print("refused: indexed_shift=1: %s" % text)
        assert rc != 0 and "fdd_shift_add_indexed" in text and "does not export" in text
        p.set_flag("indexed_shift", 0)
        p.robin(None)  # clearing what was never set is accepted
        assert not p.boundary_info()["robin_active"] and not p.helmholtz_info()["active"] and np.abs(p.helmholtz_shift()).max() == 0.0
        p.set_options(max_iterations=MAX_ITERATIONS, tolerance=TAU)
        u_star, f = p.make_rhs(0, 7)
        u, its, hist = p.solve(f)
        assert its < MAX_ITERATIONS and hist[-1] <= TAU * hist[0]
    finally:
        p.close()


# ---------------------------------------------------------------- the preconditioner's pieces on natural faces
# Shared by tests/test_gpu_boundary_preconditioner.py (all of a case) and, as child processes on the CPU stand-in, by
# tests/test_cpu_boundary.py (standin=True: that kernel library has neither fdd_shift_add nor fdd_field_surface, so lambda
# and alpha are left out on both sides; the face codes and kappa stay).  Every bound is one the project already had.
ROBIN = dict(kappa="smooth", lam=10.0, alpha={1: 2.0, 3: 0.5})
OPERATOR_CASES = {
    "box_N3_DNNNDN_all_terms": dict(kind="box", N=3, faces="DNNNDN", **ROBIN),
    "kershaw_N5_DNNNDN_all_terms": dict(kind="kershaw", N=5, faces="DNNNDN", **ROBIN),
    "box_N7_DNNNDN_all_terms": dict(kind="box", N=7, faces="DNNNDN", **ROBIN),
    "box_N7_NNDDDN": dict(kind="box", N=7, faces="NNDDDN"),  # natural x-faces: the line kernel with assemble_in_stiffness
    "box_N11_DNDNDN": dict(kind="box", N=11, faces="DNDNDN"),
    "box_N4_NNNNNN_robin": dict(kind="box", N=4, faces="NNNNNN", alpha={1: 2.0}),  # no masked point at all
}
HIERARCHY_CASES = {
    "box_N3_DNNDND": dict(kind="box", N=3, faces="DNNDND", device=True),
    "box_N4_DNNNNN_robin": dict(kind="box", N=4, faces="DNNNNN", alpha={1: 2.0}),
    "kershaw_N4_NNNNNN_shift": dict(kind="kershaw", N=4, faces="NNNNNN", lam=10.0),
    "box_N4_DNNDNN_kappa_robin": dict(kind="box", N=4, faces="DNNDNN", kappa="random", alpha={1: 2.0, 4: 0.5}),
    # degree 7: level 0 is coarsened on the lattice (8 -> 4 nodes per direction and element), whose end planes now carry dofs
    "box_N7_DNNDND_lattice": dict(kind="box", N=7, faces="DNNDND", device=True, lattice=True),
}
ORACLE_CASES = {
    "product_N7_DNNDND": dict(E=(3, 2, 2), N=7, faces="DNNDND", builder="product"),  # reaches the matrix-free transfer
    "product_N3_NDNNND": dict(E=(4, 4, 4), N=3, faces="NDNNND", builder="product"),
    "scipy_N5_DNNNNN": dict(E=(3, 2, 2), N=5, faces="DNNNNN", builder="scipy"),
    "float_N5_DNNNNN": dict(E=(3, 2, 2), N=5, faces="DNNNNN", builder="float"),
}


def set_coefficients(p, mesh, spec, standin):
    """kappa, lambda and alpha of the case on the problem; returns (kappa, lam, alpha, restated surface) as Reference takes
    them.  alpha is only returned: the caller sets it through p.robin where its check wants it (before or after a build)"""
    import diffusivity_checks as DC

    kappa = {None: None, "smooth": kappa_smooth(mesh.x, mesh.y, mesh.z), "random": DC.kappa_random(p.n, 5)}[spec.get("kappa")]
    lam = 0.0 if standin else spec.get("lam", 0.0)
    sides = None if standin else spec.get("alpha")
    if kappa is not None:
        p.diffusivity(kappa)
    if lam:
        p.helmholtz(lam)
    rs = restated_surface(mesh) if sides else None
    alpha = side_alpha(rs, mesh.p_mask, sides) if sides else None
    return kappa, lam, alpha, rs


def reference_order_of_dofs(p, ref):
    """perm[d] = the row of ref.K_free() that dof d of the Subdomain is.  One rank: the region is the rank's own points, so
    point q of the Subdomain is point q of the mesh; a point has a dof exactly where its node is free, and all points of a
    node share the dof"""
    dof, nd = p.sub_point_dofs(), p.sub_info()["unique_dofs"]
    assert len(dof) == len(ref.node) and nd == int(ref.free.sum()) == dof.max() + 1
    has = dof >= 0
    assert np.array_equal(has, ref.free[ref.node])
    row = np.cumsum(ref.free) - 1
    perm = np.full(nd, -1, np.int64)
    perm[dof[has]] = row[ref.node[has]]
    assert np.array_equal(perm[dof[has]], row[ref.node[has]]) and np.array_equal(np.sort(perm), np.arange(nd))
    return perm


def shift_on_dofs(p):
    """cbar in the Subdomain's dof order (helmholtz::dofs_of_nodes): the node vector through Q's column of a dof's points"""
    dof = p.sub_point_dofs()
    _, _, qcol, _ = p.csr(0)
    c = np.zeros(p.sub_info()["unique_dofs"])
    c[dof[dof >= 0]] = p.helmholtz_shift()[qcol[dof >= 0]]
    return c


def check_inner_operator(case, standin=False):
    """Qt A_L Q + diag(c) over the dofs is Reference.K_free() in the numbering of sub_point_dofs: sub_dof_operator within
    1e-12 max|want| and sub_jacobi_diagonal within 1e-12 relative (the bounds of test_node_operator_is_the_matrix and
    diffusivity_checks.check_operator), under preconditioner_precision 64 and 32 -- neither entry takes the flag (both run
    the double operator, tests/test_gpu_helmholtz.py), so both settings are held to the double bound and to each other"""
    S, _, _ = api()
    spec = OPERATOR_CASES[case]
    p = new_problem((2, 2, 2), spec["N"], spec["faces"], spec["kind"])
    try:
        mesh = S.ArrayMesh.from_problem(p)
        assert np.array_equal(mesh.p_mask, face_mask(mesh, spec["faces"]))
        kappa, lam, alpha, rs = set_coefficients(p, mesh, spec, standin)
        if alpha is not None:
            p.robin(spec["alpha"])
        ref = Reference(mesh, kappa, lam, alpha, rs)
        perm = reference_order_of_dofs(p, ref)
        K = ref.K_free()[perm][:, perm].tocsr()
        natural = int((ref.free & (np.bincount(ref.node, weights=on_surface(mesh), minlength=ref.nn) > 0)).sum())
        assert natural > 0  # dofs on the surface: what a Dirichlet box does not have
        x = S.seeded_uniform(len(perm), 17) - 0.5
        want, dwant = K @ x, K.diagonal()
        out = {}
        for bits in (64, 32):
            p.set_flag("preconditioner_precision", bits)
            y, d = p.sub_dof_operator(x), p.sub_jacobi_diagonal()
            e_op, e_diag = float(np.abs(y - want).max() / np.abs(want).max()), float((np.abs(d - dwant) / dwant).max())
            print("inner operator %s, precision %d: operator %.3e, diagonal %.3e (%d dofs, %d on natural faces)%s" % (case, bits, e_op, e_diag, len(perm), natural, " [lambda, alpha left out]" if standin and (spec.get("lam") or spec.get("alpha")) else ""))
            assert e_op <= 1e-12 and e_diag <= 1e-12, (case, bits, e_op, e_diag)
            out[bits] = (y, d)
        assert np.array_equal(out[32][0], out[64][0]) and np.array_equal(out[32][1], out[64][1])
        p.set_flag("preconditioner_precision", 64)
    finally:
        p.close()


def on_surface(mesh):
    """1.0 at the points on the surface of the unit cube"""
    on = np.zeros(len(mesh.x), bool)
    for c in (mesh.x, mesh.y, mesh.z):
        on |= (c == 0.0) | (c == 1.0)
    return on.astype(np.float64)


def check_level0_matrix(case, standin=False):
    """level-0 A of the host-built hierarchy is the restatement of low_order::assemble_fem on the problem's point -> dof
    array plus cbar on the diagonal (amg_setup_restatements.add_diagonal_ref), pattern and bits, as
    diffusivity_checks.check_hierarchy_matrix; it has unique_dofs rows, more than the all-Dirichlet twin by the free nodes on
    the surface; robin(None) gives back the bits of the hierarchy that never saw alpha; where nothing makes the device build
    step aside (no shift, no kappa) the device build gives the same levels; at degree 7 level-0 P is the restatement of
    low_order::geometric_level on that array, as bits, with the coarse dofs counted by hand"""
    import amg_setup_restatements as R
    import diffusivity_checks as DC

    S, _, _ = api()
    spec = HIERARCHY_CASES[case]
    E, N = (2, 2, 2), spec["N"]
    p = new_problem(E, N, spec["faces"], spec["kind"])
    try:
        mesh = S.ArrayMesh.from_problem(p)
        kappa, lam, alpha, _ = set_coefficients(p, mesh, spec, standin)
        if standin and spec["faces"] == "NNNNNN" and not lam:
            raise AssertionError("%s has no twin on the stand-in: without its shift the matrix is singular" % case)
        p.amg_build(device=False)
        never = p.amg_levels()
        if alpha is not None:
            p.robin(spec["alpha"])  # a hierarchy that amg_build made is built again
        assert p.amg_setup_info()["levels_built_on_device"] == 0
        levels = p.amg_levels()
        A = levels[0]["A"]
        pd, nd = p.sub_point_dofs(), p.sub_info()["unique_dofs"]
        assert nd == p.info["sub_num_dofs"] == A.shape[0] == A.shape[1]
        if kappa is None:
            ptr, col, val = R.assemble_fem_ref(mesh.x, mesh.y, mesh.z, pd, nd, N)[2]
        else:
            ptr, col, val = DC.assemble_fem_kappa(mesh.x, mesh.y, mesh.z, pd, nd, N, kappa)
        c = shift_on_dofs(p)
        assert c.any() == bool(lam or alpha is not None)
        if c.any():
            val = R.add_diagonal_ref(ptr, col, val, c)
        assert np.array_equal(ptr, A.indptr) and np.array_equal(col, A.indices), "pattern of A"
        assert np.array_equal(DC.bits(val), DC.bits(A.data)), "values of A: %d of %d differ" % ((DC.bits(val) != DC.bits(A.data)).sum(), len(val))
        twin = new_problem(E, N, "DDDDDD", spec["kind"])
        try:
            nd_twin = twin.sub_info()["unique_dofs"]
        finally:
            twin.close()
        node = np.unique(mesh.glo_num, return_inverse=True)[1]
        free = np.bincount(node, weights=mesh.p_mask) > 0
        natural = int((free & (np.bincount(node, weights=on_surface(mesh)) > 0)).sum())
        print("level-0 matrix %s: %d rows (%d in the all-Dirichlet twin, %d free nodes on the surface), %d entries, as bits%s" % (case, nd, nd_twin, natural, len(val), " [lambda, alpha left out]" if standin and (spec.get("lam") or spec.get("alpha")) else ""))
        assert natural > 0 and nd == nd_twin + natural
        if spec.get("lattice"):
            # low_order::geometric_level on the same point -> dof array (test_cpu_amg_setup_restatements.py holds it to the
            # all-Dirichlet boxes): P as bits; the coarse lattice has 3 E + 1 = 7 nodes per direction, each direction loses the
            # one on its single 'D' face: 6^3 coarse dofs, where the all-Dirichlet twin has 5^3; applied matrix-free
            n = N + 1
            keep = R.coarse_nodes_ref(n, S.gll(N)[0])
            g = R.geometric_level_ref(pd, nd, n, keep, *R.interp_tables_ref(S.gll(N)[0], keep))
            P = levels[0]["P"]
            assert spec["faces"] == "DNNDND" and not g["refused"] and g["unplaced"] == 0 and P.shape == (nd, g["num_coarse"]) == (nd, 6**3)
            assert np.array_equal(g["P"][0], P.indptr) and np.array_equal(g["P"][1], P.indices), "pattern of P"
            assert np.array_equal(DC.bits(g["P"][2]), DC.bits(P.data)), "values of P"
            assert p.amg_level_transfer(0)
            print("level-0 matrix %s: P %d x %d on the lattice, as bits" % (case, nd, P.shape[1]))
        if alpha is not None:
            assert not np.array_equal(DC.bits(A.data), DC.bits(never[0]["A"].data))
            p.robin(None)
            DC.same_levels(p.amg_levels(), never)
        if spec.get("device") and not standin:
            p.amg_build(device=True)
            built = p.amg_setup_info()["levels_built_on_device"]
            print("level-0 matrix %s: %d level(s) built on the device" % (case, built))
            assert built >= 1
            DC.same_levels(p.amg_levels(), levels)
    finally:
        p.close()


def check_against_oracle(case):
    """amg_checks.check_amg / check_amg_f32 as they stand on a problem with natural faces (the oracle reads p_mask from the
    mesh it is given): V-cycle 1e-11, inner histories 1e-9, outer history 1e-8, the oracle's iteration count, the matrix-free
    transfer against the CSR one 1e-13 / 2e-5.  Prints the count (no cap: equality with the oracle's is the condition)"""
    import amg_checks

    spec = ORACLE_CASES[case]
    p = new_problem(spec["E"], spec["N"], spec["faces"])
    try:
        p.set_flag("sub_use_preconditioner", 0)  # switched on by the checks once the hierarchy under test is attached
        if spec["builder"] == "float":
            its = amg_checks.check_amg_f32(p, spec["N"], 2)
            print("oracle %s: %d outer iterations with the float cycle (within one of the double cycle's)" % (case, its))
        else:
            its = amg_checks.check_amg(p, spec["N"], 2, builder=spec["builder"])
            assert its is not None
            print("oracle %s: %d outer iterations, product and oracle" % (case, its))
            if spec["builder"] == "product":
                assert p.amg_level_transfer(0) == (spec["N"] == 7)
    finally:
        p.close()


CHECKS = {"solves_N3": lambda: check_solves(3), "solves_N5": lambda: check_solves(5), "singular": check_singular, "missing_entries": check_missing_entries}
CHECKS.update({"operator_" + c: (lambda c=c: check_inner_operator(c, standin=True)) for c in OPERATOR_CASES})
CHECKS.update({"level0_" + c: (lambda c=c: check_level0_matrix(c, standin=True)) for c in HIERARCHY_CASES})
CHECKS.update({"oracle_" + c: (lambda c=c: check_against_oracle(c)) for c in ORACLE_CASES})


def write_files(L, directory, E, P, N, rank, faces, eps):
    """one rank's mesh files through the host layer's writer (it needs no device): faces "-" takes the writer that was
    there before the codes.  Prints the return code and fddh_last_error()"""
    import ctypes

    arr3 = lambda v: (ctypes.c_int * 3)(*[int(t) for t in v.split(",")])
    eps = ctypes.c_double(float(eps))
    if faces == "-":
        rc = L.raw("fddh_write_kershaw_mesh_files")(os.fsencode(directory), arr3(E), arr3(P), int(N), int(rank), eps, eps)
    else:
        rc = L.raw("fddh_write_box_faces_mesh_files")(os.fsencode(directory), arr3(E), arr3(P), int(N), int(rank), eps, eps, faces.strip("'").encode())
    print("%d\t%s" % (rc, L.raw("fddh_last_error")().decode() if rc else ""))


def main(lib_path, name, *args):
    S, H, lib = api()
    lib._host = lib._Lib(lib_path, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
    if name == "write":
        return write_files(lib.host(), *args)
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    CHECKS[name]()
    print("ok")


if __name__ == "__main__":
    main(*sys.argv[1:])
