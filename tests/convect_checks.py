"""Numpy restatement of the convection term (include/fdd_hip.h: fdd_field_convect, fdd_field_weak_convect) on the geometry of
tests/field_checks.py, in any float type: np.longdouble is the reference the kernels are held to, float64 says what double
arithmetic can deliver (tests/test_cpu_convect.py).

With C = adj J = I det J and chat_b = sum_a C[b][a] c_a:
  convect       = (sum_b chat_b du/dr_b) / det J
  weak_convect  = (P^T x P^T x P^T) [omega omega omega sum_b ((P x P x P) chat_b) (u,_b on the fine grid)]
on M Gauss-Legendre points per direction (M = None: the kernel's (3n+1)/2), P the interpolation from the GLL points to them
by the barycentric formula, P' = P D.  The nodes of both grids are Newton-refined in the working type.
T_c and T_wc are the sums of the absolute values of the terms of the two, largest over the points.
"""
import numpy as np

import field_checks as F
import support as S


def legendre(z, m):
    """(P_m, P_m') at z"""
    p0, p1 = np.ones_like(z), z.copy()
    for k in range(1, m):
        p0, p1 = p1, ((2 * k + 1) * z * p1 - k * p0) / (k + 1)
    return p1, m * (z * p1 - p0) / (z * z - 1)


def gauss(M, dtype):
    """M Gauss-Legendre nodes (ascending) and weights in dtype"""
    z = np.asarray(np.polynomial.legendre.leggauss(M)[0], dtype=dtype)
    for _ in range(3):
        p, dp = legendre(z, M)
        z = z - p / dp
    z = (z - z[::-1]) / 2  # symmetric, the centre of an odd rule exactly 0
    dp = legendre(z, M)[1]
    return z, 2 / ((1 - z * z) * dp * dp)


def lobatto(N, dtype):
    """the N+1 GLL nodes in dtype: the golden ones, their interior refined by Newton on P_N'"""
    z = np.asarray(S.gll(N)[0], dtype=dtype)
    x = z[1:-1].copy()
    for _ in range(3 if N > 1 else 0):
        p, dp = legendre(x, N)
        x = x - dp / ((2 * x * dp - N * (N + 1) * p) / (1 - x * x))
    z[1:-1] = (x - x[::-1]) / 2
    return z


def interpolation(z, x):
    """P[q, i] = l_i(x_q) for the nodes z, barycentric; a point that is a node gives the unit row"""
    n = len(z)
    lam = np.array([1 / np.prod([z[i] - z[j] for j in range(n) if j != i]) for i in range(n)], dtype=z.dtype)
    diff = x[:, None] - z[None, :]
    hit = diff == 0
    P = lam[None, :] / np.where(hit, 1, diff)
    P = P / P.sum(axis=1)[:, None]
    rows = hit.any(axis=1)
    P[rows] = hit[rows].astype(z.dtype)
    return P


def tables(N, dtype, D, M=None):
    """(z, w, P, P') of the rule with M points (None: (3n+1)/2) for the degree-N GLL grid and the derivative matrix D"""
    n = N + 1
    z, w = gauss((3 * n + 1) // 2 if M is None else M, dtype)
    P = interpolation(lobatto(N, dtype), z)
    return z, w, P, P @ np.asarray(D, dtype=dtype).reshape(n, n)


def tensor3(At, As, Ar, f):
    """(At x As x Ar) f for f[e, k, j, i]: Ar along i, As along j, At along k"""
    f = np.einsum("ai,ekji->ekja", Ar, f)
    f = np.einsum("bj,ekja->ekba", As, f)
    return np.einsum("ck,ekba->ecba", At, f)


def _fields(g, c, u):
    return [np.asarray(a, dtype=g.dtype).reshape(g.shape) for a in c], np.asarray(u, dtype=g.dtype).reshape(g.shape)


def chat(g, c):
    """chat_b = sum_a C[b][a] c_a, C = adj J = I det J"""
    return [(g.I[b][0] * c[0] + g.I[b][1] * c[1] + g.I[b][2] * c[2]) * g.det for b in range(3)]


def chat_abs(g, c):
    return [(np.abs(g.I[b][0]) * np.abs(c[0]) + np.abs(g.I[b][1]) * np.abs(c[1]) + np.abs(g.I[b][2]) * np.abs(c[2])) * np.abs(g.det) for b in range(3)]


def convect(g, c, u):
    c, u = _fields(g, c, u)
    du, ch = F.along(g.D, u), chat(g, c)
    return ((ch[0] * du[0] + ch[1] * du[1] + ch[2] * du[2]) / g.det).reshape(-1)


def convect_scale(g, c, u):
    """T_c"""
    c, u = _fields(g, c, u)
    du, ch = F.along(np.abs(g.D), np.abs(u)), chat_abs(g, c)
    return float(((ch[0] * du[0] + ch[1] * du[1] + ch[2] * du[2]) / np.abs(g.det)).max())


def _weak(P, Pd, w, ch, u):
    fine = [tensor3(P, P, P, b) for b in ch]
    du = [tensor3(P, P, Pd, u), tensor3(P, Pd, P, u), tensor3(Pd, P, P, u)]
    www = w[None, :, None, None] * w[None, None, :, None] * w[None, None, None, :]
    s = www * (fine[0] * du[0] + fine[1] * du[1] + fine[2] * du[2])
    return tensor3(P.T, P.T, P.T, s)


def weak_convect(g, c, u, M=None, quadrature=None):
    """quadrature: (z, w, P, P') to use instead of tables(N, g.dtype, g.D, M)"""
    c, u = _fields(g, c, u)
    _, w, P, Pd = tables(g.n - 1, g.dtype, g.D, M) if quadrature is None else [np.asarray(t, dtype=g.dtype) for t in quadrature]
    return _weak(P, Pd, w, chat(g, c), u).reshape(-1)


def weak_convect_scale(g, c, u, M=None):
    """T_wc"""
    c, u = _fields(g, c, u)
    _, w, P, Pd = tables(g.n - 1, g.dtype, g.D, M)
    return float(_weak(np.abs(P), np.abs(Pd), np.abs(w), chat_abs(g, c), np.abs(u)).max())


def collocated_weak(g, c, u):
    """mass . convect: the weak form on the GLL points themselves, which aliases"""
    return F.mass(g) * convect(g, c, u)


def fields(mesh, seed):
    """seeded (cx, cy, cz), u of the mesh's points: element-local values, each a polynomial of degree N per element"""
    u, c, _ = F.fields(mesh, seed)
    return c, u
