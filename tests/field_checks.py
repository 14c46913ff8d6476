"""Numpy restatement of the field operators (include/fdd_hip.h: fdd_field_mass, _gradient, _weak_divergence) on the arrays of
a support.BoxMesh / KershawMesh / DeformedMesh, in any float type: np.longdouble is the reference the kernels are held to,
float64 the cross-check that says what double arithmetic can deliver (tests/test_cpu_field_ops.py).

Arrays are element-major, x fastest: a field is viewed as [e, k, j, i].  D[i, p] = D_hat[p + i n].  With X = (x, y, z):
  J[a][b] = dX_a / dr_b   D applied to X_a along r (i), s (j), t (k)
  I       = J^-1          by cofactors over det J
  mass    = w_i w_j w_k det J
  grad_a  = sum_b du/dr_b I[b][a]
  wdiv    = D_r^T F_r + D_s^T F_s + D_t^T F_t,  F_b = mass sum_a I[b][a] v_a
T and T_w are the sums of the absolute values of the terms of a gradient component and of a weak divergence, largest over
the points: what a rounding error of the operators is measured against.
"""
import numpy as np

import support as S


def along(D, c):
    """(D c along r, along s, along t) of c[e, k, j, i]"""
    return [np.einsum("ip,ekjp->ekji", D, c), np.einsum("jp,ekpi->ekji", D, c), np.einsum("kp,epji->ekji", D, c)]


def along_transposed(D, F):
    """D_r^T F[0] + D_s^T F[1] + D_t^T F[2]"""
    return np.einsum("pi,ekjp->ekji", D, F[0]) + np.einsum("pj,ekpi->ekji", D, F[1]) + np.einsum("pk,epji->ekji", D, F[2])


class Geometry:
    pass


def geometry(mesh, dtype, D_hat=None):
    """D, the weights and, per point, J, det J, I = J^-1 and the mass of `mesh` in `dtype`; D_hat: another table than the
    golden one of the mesh's degree"""
    g = Geometry()
    n = mesh.N + 1
    _, w, D = S.gll(mesh.N)
    g.n, g.ne, g.dtype = n, mesh.num_local_elements, dtype
    g.D = np.asarray(D if D_hat is None else D_hat, dtype=dtype).reshape(n, n)
    g.w = np.asarray(w, dtype=dtype)
    g.shape = (g.ne, n, n, n)
    X = [np.asarray(c, dtype=dtype).reshape(g.shape) for c in (mesh.x, mesh.y, mesh.z)]
    J = [along(g.D, c) for c in X]  # J[a][b]
    cof = lambda a, b, c, d: J[a[0]][a[1]] * J[b[0]][b[1]] - J[c[0]][c[1]] * J[d[0]][d[1]]
    C = [[cof((1, 1), (2, 2), (1, 2), (2, 1)), cof((0, 2), (2, 1), (0, 1), (2, 2)), cof((0, 1), (1, 2), (0, 2), (1, 1))],
         [cof((1, 2), (2, 0), (1, 0), (2, 2)), cof((0, 0), (2, 2), (0, 2), (2, 0)), cof((0, 2), (1, 0), (0, 0), (1, 2))],
         [cof((1, 0), (2, 1), (1, 1), (2, 0)), cof((0, 1), (2, 0), (0, 0), (2, 1)), cof((0, 0), (1, 1), (0, 1), (1, 0))]]
    g.det = J[0][0] * C[0][0] + J[0][1] * C[1][0] + J[0][2] * C[2][0]
    g.J = J
    g.I = [[C[b][a] / g.det for a in range(3)] for b in range(3)]  # I[b][a] = dr_b / dX_a
    g.www = g.w[None, :, None, None] * g.w[None, None, :, None] * g.w[None, None, None, :]
    g.mass = g.www * g.det
    return g


def mass(g):
    return g.mass.reshape(-1)


def gradient(g, u):
    """[gx, gy, gz] of u (flat)"""
    du = along(g.D, np.asarray(u, dtype=g.dtype).reshape(g.shape))
    return [(du[0] * g.I[0][a] + du[1] * g.I[1][a] + du[2] * g.I[2][a]).reshape(-1) for a in range(3)]


def gradient_scale(g, u):
    """T: the largest sum of the absolute terms of a gradient component"""
    du = along(np.abs(g.D), np.abs(np.asarray(u, dtype=g.dtype).reshape(g.shape)))
    return max(float((du[0] * np.abs(g.I[0][a]) + du[1] * np.abs(g.I[1][a]) + du[2] * np.abs(g.I[2][a])).max()) for a in range(3))


def weak_divergence(g, v):
    v = [np.asarray(c, dtype=g.dtype).reshape(g.shape) for c in v]
    F = [g.mass * (g.I[b][0] * v[0] + g.I[b][1] * v[1] + g.I[b][2] * v[2]) for b in range(3)]
    return along_transposed(g.D, F).reshape(-1)


def weak_divergence_scale(g, v):
    """T_w: the same for the weak divergence"""
    v = [np.abs(np.asarray(c, dtype=g.dtype).reshape(g.shape)) for c in v]
    F = [np.abs(g.mass) * (np.abs(g.I[b][0]) * v[0] + np.abs(g.I[b][1]) * v[1] + np.abs(g.I[b][2]) * v[2]) for b in range(3)]
    return float(along_transposed(np.abs(g.D), F).max())


def adjoint_sides(g, out, v, phi, grad_phi):
    """(sum out phi, sum B v . grad phi, the sum of the absolute values of the terms of both): out = wdiv(v) makes the first
    two equal"""
    out, phi = np.asarray(out, dtype=g.dtype), np.asarray(phi, dtype=g.dtype)
    B = g.mass.reshape(-1)
    terms = [B * np.asarray(v[a], dtype=g.dtype) * np.asarray(grad_phi[a], dtype=g.dtype) for a in range(3)]
    return (out * phi).sum(), sum(t.sum() for t in terms), np.abs(out * phi).sum() + sum(np.abs(t).sum() for t in terms)


LINEAR = (0.7, -1.3, 0.4)


def linear_field(mesh, c=0.25):
    """u = a . X + c with a = LINEAR: its gradient is a at every point of any mesh whose map the elements represent"""
    return LINEAR[0] * mesh.x + LINEAR[1] * mesh.y + LINEAR[2] * mesh.z + c


def mesh_of(kind, E, N, **kw):
    return {"box": S.BoxMesh, "kershaw": S.KershawMesh, "deformed": S.DeformedMesh}[kind](E, N, **kw)


def fields(mesh, seed):
    """seeded u, (vx, vy, vz), phi of the mesh's points: element-local values, as the operators are element-local"""
    n = mesh.num_local_points
    return S.seeded_uniform(n, seed) - 0.5, [S.seeded_uniform(n, seed + 1 + a) - 0.5 for a in range(3)], S.seeded_uniform(n, seed + 7) - 0.5


# ---- -laplace(u) = s on the unit cube from the source term, in numpy alone ----
def source(x, y, z):
    return 3.0 * np.pi**2 * np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)


def exact(x, y, z):
    return np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)


def source_solve_error(N, E=2):
    """max |u_h - u| over the nodes of the E^3-element box at degree N, u_h from f = B s (B: mass() of the restatement, summed
    over the copies of a node) and a dense solve with the assembled stiffness matrix, which on this mesh is the sum of three
    Kronecker products of the 1-D stiffness and mass matrices"""
    mesh = S.BoxMesh((E, E, E), N)
    n = N + 1
    z, w, D = S.gll(N)
    D = np.asarray(D).reshape(n, n)
    h = 1.0 / E
    G = E * N + 1
    K1, M1 = np.zeros((G, G)), np.zeros(G)
    for e in range(E):
        sl = slice(e * N, e * N + n)
        K1[sl, sl] += (2.0 / h) * (D.T * w) @ D
        M1[sl] += 0.5 * h * w
    xs = np.concatenate([(e + 0.5 * (z[:N] + 1.0)) * h for e in range(E)] + [[1.0]])
    index = lambda c: np.abs(c[:, None] - xs[None, :]).argmin(axis=1)
    node = index(mesh.x) + G * (index(mesh.y) + G * index(mesh.z))
    f = np.bincount(node, weights=mass(geometry(mesh, np.float64)) * source(mesh.x, mesh.y, mesh.z), minlength=G**3)
    inner = np.arange(1, G - 1)
    Ki, Mi = K1[np.ix_(inner, inner)], np.diag(M1[inner])
    A = np.kron(Mi, np.kron(Mi, Ki)) + np.kron(Mi, np.kron(Ki, Mi)) + np.kron(Ki, np.kron(Mi, Mi))  # x fastest
    keep = (inner[:, None, None] * G * G + inner[None, :, None] * G + inner[None, None, :]).reshape(-1)
    u = np.linalg.solve(A, f[keep])
    zz, yy, xx = np.meshgrid(xs[inner], xs[inner], xs[inner], indexing="ij")
    return float(np.abs(u - exact(xx, yy, zz).reshape(-1)).max())
