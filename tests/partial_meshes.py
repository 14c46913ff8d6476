"""Meshes on which only some elements meet a condition that the host layer establishes per element list, and numpy
restatements of those conditions (host/element_operator.hpp: detect_zero_factors, detect_shared_blocks, detect_affine).
This module knows nothing of the kernel library: it builds BoxMesh-like objects that support.write_mesh_files accepts, and
reads their arrays.

Builders (elems: global element numbers ix + Ex (iy + Ey iz) of the box; a rank's part holds the ones that fall into it)
  bumped    the listed elements get the interior bump 0.05 h (1, -0.7, 0.5) prod_a sin^2(pi t_a), t the element's own unit
            coordinates, h its shortest edge: zero with zero slope on the element's faces, so the mesh stays conforming and no
            other element moves.  The bumped elements get the isoparametric factors of their own points; EVERY OTHER element
            keeps the base mesh's blocks bit for bit (recomputing them isoparametrically would leave rounding noise of 1e-17
            in g_4..g_6, since D * const is not exactly 0).  At degree 1 an element has no interior point: the base mesh
  graded    g_1..g_3 of the listed elements times a smooth positive function of the point, another one per element;
            g_4..g_6 stay 0.0: a diagonal list that is neither affine nor repeating
  sheared   the box under x += 0.25 y + 0.1 z, y -= 0.15 z, factors in the analytic form c_f ((w_i w_j) w_k) with constant
            non-zero c_4..c_6 (the isoparametric factors of such a mesh do not meet affine_tolerance above degree 2)
  edited    one entry of one factor array replaced

Restated verdicts, on the elements of a list given by their local numbers (None: all)
  offdiag_zero      every entry of g_4..g_6 is +-0.0
  factor_classes    the number of bit-distinct blocks of g_1..g_3; shared: at most half as many as elements, within
                    SHARED_FACTOR_BYTES_LIMIT, and only where offdiag_zero holds
  affine_deviation  c_f = G_f(p0) / W(p0) at the middle point p0, the largest |G_f(p) - c_f W(p)| / (max_f |c_f| W(p)),
                    W(p) = (w_i w_j) w_k; affine: at most AFFINE_TOLERANCE = 64 eps
  list_state        the tuple stiffness_choice_rules takes, from the three above and the verdict on the degree's table
"""
import copy

import numpy as np

import support as S

AFFINE_TOLERANCE = 64.0 * np.finfo(np.float64).eps
SHARED_FACTOR_BYTES_LIMIT = 1 << 20
BUMP = (0.05, (1.0, -0.7, 0.5))
SHEAR = np.array([[1.0, 0.25, 0.1], [0.0, 1.0, -0.15], [0.0, 0.0, 1.0]])
PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


def _own(mesh):
    """a copy whose arrays can be written without touching the mesh it was made from"""
    m = copy.copy(mesh)
    m.x, m.y, m.z = mesh.x.copy(), mesh.y.copy(), mesh.z.copy()
    m.g = [a.copy() for a in mesh.g]
    return m


def local_elements(mesh, elems):
    """the local numbers, ascending, of the global elements `elems` that this rank's part holds"""
    Ex, Ey, _ = mesh.E
    lx, ly, lz = mesh.local_E
    ox, oy, oz = mesh.origin
    out = []
    for g in elems:
        ix, iy, iz = g % Ex - ox, (g // Ex) % Ey - oy, g // (Ex * Ey) - oz
        if 0 <= ix < lx and 0 <= iy < ly and 0 <= iz < lz:
            out.append(ix + lx * (iy + ly * iz))
    return sorted(out)


def sheared(E, N, P=(1, 1, 1), rank=0):
    m = _own(S.BoxMesh(E, N, P, rank))
    n = N + 1
    _, w, _ = S.gll(N)
    h = 1.0 / np.asarray(E, np.float64)
    J = SHEAR * (0.5 * h)[None, :]  # dx/dr of every element
    Ji = np.linalg.inv(J)
    c = np.linalg.det(J) * (Ji @ Ji.T)
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    W = ((w[i] * w[j]) * w[k]).reshape(-1)  # the product in the order the affine kernel forms it
    m.g = [np.ascontiguousarray(np.tile(c[a, b] * W, m.num_local_elements)) for a, b in PAIRS]
    x, y, z = m.x, m.y, m.z
    m.x, m.y, m.z = x + 0.25 * y + 0.1 * z, y - 0.15 * z, z.copy()
    m.shear_constants = [c[a, b] for a, b in PAIRS]
    return m


def bumped(E, N, elems, P=(1, 1, 1), rank=0, base="box"):
    m = sheared(E, N, P, rank) if base == "sheared" else _own(S.BoxMesh(E, N, P, rank))
    m.bumped_elements = local_elements(m, elems) if N >= 2 else []
    if not m.bumped_elements:
        return m
    n = N + 1
    n3 = n**3
    z, _, _ = S.gll(N)
    t = 0.5 * (np.asarray(z) + 1.0)
    s = np.sin(np.pi * t) ** 2
    s[0] = s[-1] = 0.0  # sin(pi) is 1.2e-16 in double: the faces stay where they are, exactly
    shape = (s[:, None, None] * s[None, :, None] * s[None, None, :]).reshape(-1)  # symmetric in k, j, i
    amplitude = BUMP[0] * min(1.0 / e for e in E)
    for e in m.bumped_elements:
        at = slice(e * n3, (e + 1) * n3)
        one = copy.copy(m)
        one.num_local_elements = 1
        S.DeformedMesh._isoparametric(one, [c[at] + amplitude * d * shape for c, d in zip((m.x, m.y, m.z), BUMP[1])])
        m.x[at], m.y[at], m.z[at] = one.x, one.y, one.z
        for f in range(6):
            m.g[f][at] = one.g[f]
    return m


def grading(mesh, e):
    """the factor of element e's points: smooth, within [0.7, 1.3], and another function for every element"""
    n3 = mesh.num_elem_points
    at = slice(e * n3, (e + 1) * n3)
    return 1.0 + 0.3 * np.cos(0.7 * e + 2.0 * mesh.x[at] + 3.0 * mesh.y[at] + 5.0 * mesh.z[at])


def graded(E, N, elems, P=(1, 1, 1), rank=0):
    m = _own(S.BoxMesh(E, N, P, rank))
    n3 = m.num_elem_points
    m.graded_elements = local_elements(m, elems)
    for e in m.graded_elements:
        at = slice(e * n3, (e + 1) * n3)
        for f in range(3):
            m.g[f][at] = m.g[f][at] * grading(m, e)
    return m


def edited(mesh, f, element, point, value):
    """f: "g_1" .. "g_6"; point: within the element (negative: from its end)"""
    m = _own(mesh)
    n3 = m.num_elem_points
    m.g[int(f[2:]) - 1][element * n3 + (point % n3)] = value
    return m


class collected:
    """the factor blocks of a list whose elements come from several meshes of one degree (a composite region's list: a
    rank's own elements, or ring elements pulled from its peers); parts: (mesh, local element) in the list's order"""

    def __init__(self, parts):
        first = parts[0][0]
        self.N, self.num_elem_points, self.num_local_elements = first.N, first.num_elem_points, len(parts)
        assert all(m.N == self.N for m, _ in parts)
        n3 = self.num_elem_points
        self.g = [np.concatenate([m.g[f][e * n3 : (e + 1) * n3] for m, e in parts]) for f in range(6)]


# ---------------------------------------------------------------- restated verdicts
def _blocks(mesh, f, elems):
    a = np.ascontiguousarray(mesh.g[f], np.float64).reshape(mesh.num_local_elements, mesh.num_elem_points)
    return a if elems is None else a[np.asarray(elems, np.int64)]


def offdiag_zero(mesh, elems=None):
    """-0.0 passes, a denormal does not"""
    return all(not (_blocks(mesh, f, elems).view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)).any() for f in (3, 4, 5))


def factor_classes(mesh, elems=None):
    rows = np.concatenate([_blocks(mesh, f, elems) for f in range(3)], axis=1)
    return len({row.tobytes() for row in rows})


def shared(mesh, elems=None):
    if not offdiag_zero(mesh, elems):
        return False
    ne = mesh.num_local_elements if elems is None else len(elems)
    classes = factor_classes(mesh, elems)
    return 2 * classes <= ne and classes * 3 * mesh.num_elem_points * 8 <= SHARED_FACTOR_BYTES_LIMIT


def affine_deviation(mesh, elems=None, per_element=False):
    n = mesh.N + 1
    _, w, _ = S.gll(mesh.N)
    w = np.asarray(w, np.float64)
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    W = ((w[i] * w[j]) * w[k]).reshape(-1)
    mid = n // 2
    p0 = mid + mid * n + mid * n * n
    G = np.stack([_blocks(mesh, f, elems) for f in range(6)])  # [f, e, p]
    c = G[:, :, p0] / ((w[mid] * w[mid]) * w[mid])
    scale = np.abs(c).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = (np.abs(G - c[:, :, None] * W[None, None, :]) / (scale[None, :, None] * W[None, None, :])).max(axis=(0, 2))
    worst = np.where(scale > 0.0, worst, 1.0)
    worst = np.where(np.isnan(worst), 1.0, worst)
    return worst if per_element else float(worst.max())


def list_state(mesh, elems=None, affine_requested=False, lean=(False, False)):
    """(dim, degree, affine in use, offdiag_zero, shared_blocks, lean verdict on the double table, on the float table) of a
    3-D list of degree <= 15: the argument of stiffness_choice_rules.choose / info.  lean: the verdicts on the degree-7 table"""
    zero = offdiag_zero(mesh, elems)
    return (3, mesh.N, bool(affine_requested) and affine_deviation(mesh, elems) <= AFFINE_TOLERANCE, zero, zero and shared(mesh, elems), mesh.N == 7 and lean[0], mesh.N == 7 and lean[1])
