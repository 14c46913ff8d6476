"""Numpy restatement of the Helmholtz problem (-laplace + lam) u = s on the unit cube with E^3 elements of degree N: the
dense reference the solves of tests/test_gpu_helmholtz.py are held to, and what it gives on its own
(tests/test_cpu_helmholtz.py).  The construction is field_checks.source_solve_error's -- the assembled stiffness matrix as
the sum of three Kronecker products of the 1-D stiffness and mass matrices, x fastest, Dirichlet nodes removed -- with
lam * kron(M, M, M) added; the mass matrix is diagonal, so the term is a vector.

  exact     u = sin(pi x) sin(pi y) sin(pi z)
  source    s = (3 pi^2 + lam) u
  f         B s at the points (B: the diagonal mass matrix), summed over the copies of a node
"""
import functools
import math

import numpy as np

import field_checks as F
import support as S


class Box:
    """The E^3-element box at degree N.  K: the dense stiffness matrix over the interior nodes; m: the diagonal of the mass
    matrix there; node: lattice index of every point of the mesh (x fastest, G = E N + 1 per direction); keep: the lattice
    indices of the interior nodes, in the order of K's rows; exact: u at those nodes."""

    def __init__(self, N, E=2):
        self.N, self.E = N, E
        self.mesh = mesh = S.BoxMesh((E, E, E), N)
        n = N + 1
        z, w, D = S.gll(N)
        D = np.asarray(D).reshape(n, n)
        h = 1.0 / E
        self.G = G = E * N + 1
        K1, M1 = np.zeros((G, G)), np.zeros(G)
        for e in range(E):
            sl = slice(e * N, e * N + n)
            K1[sl, sl] += (2.0 / h) * (D.T * w) @ D
            M1[sl] += 0.5 * h * w
        xs = np.concatenate([(e + 0.5 * (z[:N] + 1.0)) * h for e in range(E)] + [[1.0]])
        index = lambda c: np.abs(c[:, None] - xs[None, :]).argmin(axis=1)
        self.node = index(mesh.x) + G * (index(mesh.y) + G * index(mesh.z))
        inner = np.arange(1, G - 1)
        Ki, Mi = K1[np.ix_(inner, inner)], np.diag(M1[inner])
        self.K = np.kron(Mi, np.kron(Mi, Ki)) + np.kron(Mi, np.kron(Ki, Mi)) + np.kron(Ki, np.kron(Mi, Mi))
        mi = M1[inner]
        self.m = np.kron(mi, np.kron(mi, mi))
        self.keep = (inner[:, None, None] * G * G + inner[None, :, None] * G + inner[None, None, :]).reshape(-1)
        zz, yy, xx = np.meshgrid(xs[inner], xs[inner], xs[inner], indexing="ij")
        self.exact = F.exact(xx, yy, zz).reshape(-1)

    def matrix(self, lam):
        """the assembled Helmholtz matrix over the interior nodes"""
        A = self.K.copy()
        A[np.diag_indices_from(A)] += lam * self.m
        return A

    def source(self, lam):
        """s at the points of the mesh"""
        return (3.0 * np.pi**2 + lam) * F.exact(self.mesh.x, self.mesh.y, self.mesh.z)

    def assembled(self, f_points):
        """the sums of a point vector over the copies of every interior node"""
        return np.bincount(self.node, weights=f_points, minlength=self.G**3)[self.keep]

    def on_nodes(self, u_points):
        """a continuous point vector at the interior nodes"""
        lattice = np.zeros(self.G**3)
        lattice[self.node] = u_points
        return lattice[self.keep]

    def rhs(self, lam):
        """f = B s of the restatement, assembled"""
        return self.assembled(F.mass(F.geometry(self.mesh, np.float64)) * self.source(lam))

    def solve_error(self, lam):
        """max |u_h - u| over the interior nodes, u_h from the dense solve"""
        return float(np.abs(np.linalg.solve(self.matrix(lam), self.rhs(lam)) - self.exact).max())

    def jacobi_condition(self, lam):
        """the condition number of D^-1/2 A D^-1/2, D the diagonal of A (both ends of the spectrum by Lanczos: a full
        eigendecomposition of the 2197 rows at N = 7 takes several seconds, this a fraction of one, to 1e-10)"""
        from scipy.sparse.linalg import eigsh

        A = self.matrix(lam)
        s = 1.0 / np.sqrt(np.diag(A))
        ev = eigsh(s[:, None] * A * s[None, :], k=2, which="BE", tol=1e-10, ncv=min(len(s) - 1, 80), return_eigenvectors=False)
        return float(ev.max() / ev.min())


@functools.lru_cache(maxsize=None)
def box(N, E=2):
    return Box(N, E)


def cg_bound(kappa, tau):
    """iterations after which the energy-norm error bound 2 ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k of CG is below tau"""
    rk = math.sqrt(kappa)
    return int(math.ceil(math.log(2.0 / tau) / math.log((rk + 1.0) / (rk - 1.0))))
