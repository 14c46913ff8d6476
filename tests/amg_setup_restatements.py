"""Plain numpy restatements of the host setup routines of host/low_order.hpp that the device kernels of
csrc/fdd_amg_setup.hip must reproduce bit for bit: coarse_nodes and the 1-D interpolation tables, geometric_level (on a
conforming lattice given as its point -> dof array), assemble_fem with from_triplets.

Every floating-point statement is the host's own, in the host's order, evaluated in IEEE double (np.float64 scalars, or
np.float64 arrays where one statement is applied to all tetrahedra at once: numpy neither contracts nor reorders, so each
element sees the scalar statement).  Sums whose order matters -- the 27-slot stencils, the merge of equal columns -- run
as scalar loops in the order of arrival.  test_cpu_amg_setup_restatements.py holds these to the host build itself; the GPU
tests (test_gpu_amg_setup_kernels.py) then use them as the reference of the kernels."""
import numpy as np

INT_MAX = 2**31 - 1
f64 = np.float64

# vertex offsets (i, j, k) of the 6 tetrahedra of a cell: the table of low_order::assemble_fem
TETS = np.array([[[0, 0, 0], [0, 1, 0], [1, 0, 0], [1, 0, 1]], [[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 1]], [[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 1]],
                 [[1, 0, 1], [1, 1, 0], [1, 1, 1], [0, 1, 0]], [[0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 1, 0]], [[1, 0, 1], [1, 1, 1], [0, 1, 1], [0, 1, 0]]])


# ----------------------------------------------------------------------------------------------------------------------
# the lattice
# ----------------------------------------------------------------------------------------------------------------------
def coarse_nodes_ref(n, ref):
    """low_order::coarse_nodes (uniform targets)"""
    if n <= 4:
        return [0, n - 1]
    m = (n + 1) // 2
    if n % 2 == 0 and m % 2 == 1:
        m += 1
    taken = [False] * n
    for q in range((m + 1) // 2):
        target = f64(-1.0) + f64(2.0) * f64(q) / f64(m - 1)
        best = -1
        for i in range((n - 1) // 2 + 1):
            if not taken[i] and (best < 0 or abs(f64(ref[i]) - target) < abs(f64(ref[best]) - target) - f64(1e-14)):
                best = i
        taken[best] = taken[n - 1 - best] = True
    return [i for i in range(n) if taken[i]]


def interp_tables_ref(ref, keep):
    """lo, hi, wl of low_order::geometric_level: node i from the kept nodes keep[lo[i]], keep[hi[i]] with weights wl[i], 1 - wl[i]"""
    n, m = len(ref), len(keep)
    pos = [-1] * n
    for a in range(m):
        pos[keep[a]] = a
    lo, hi, wl = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    a = 0
    for i in range(n):
        if pos[i] >= 0:
            lo[i] = hi[i] = pos[i]
            wl[i] = 1.0
            a = pos[i]
            continue
        lo[i], hi[i] = a, a + 1
        wl[i] = (f64(ref[keep[a + 1]]) - f64(ref[i])) / (f64(ref[keep[a + 1]]) - f64(ref[keep[a]]))
    return lo, hi, wl


def interp_rows_ref(cmap, first, point_dof, n, keep, lo, hi, wl):
    """The rows of P from cmap / first: per dof a list of (coarse column, value), columns ascending (stable) and equal
    columns summed in arrival order; None for a row that is refused because a kept node's dof is not kept.  Also returns
    how many entries were merged into an equal column."""
    np3 = n * n * n
    rows, merged = [], 0
    for d in range(len(cmap)):
        if cmap[d] >= 0:
            rows.append([(int(cmap[d]), f64(1.0))])
            continue
        q = int(first[d])
        e, v = q // np3, q % np3
        idx = [v % n, (v // n) % n, v // (n * n)]
        row, refused = [], False
        for corner in range(8):
            w = f64(1.0)
            cq, stride, skip = 0, 1, False
            for a in range(3):
                side, i = (corner >> a) & 1, idx[a]
                if lo[i] == hi[i]:
                    if side:
                        skip = True
                    cq += int(keep[lo[i]]) * stride
                else:
                    w = w * ((f64(1.0) - f64(wl[i])) if side else f64(wl[i]))
                    cq += int(keep[hi[i] if side else lo[i]]) * stride
                stride *= n
            if skip:
                continue
            fd = int(point_dof[e * np3 + cq])
            if fd < 0:
                continue
            assert fd < len(cmap), "a kept lattice node carries a dof outside the matrix: not a valid input"
            c = int(cmap[fd])
            if c < 0:
                refused = True
                break
            row.append((c, w * f64(1.0)))
        if refused:
            rows.append(None)
            continue
        row.sort(key=lambda t: t[0])  # stable
        out = []
        for t, (c, w) in enumerate(row):
            if t > 0 and c == row[t - 1][0]:
                out[-1] = (c, f64(out[-1][1] + w))
                merged += 1
            else:
                out.append((c, w))
        rows.append(out)
    return rows, merged


def geometric_level_ref(point_dof, num_dofs, n, keep, lo, hi, wl):
    """low_order::geometric_level on a conforming lattice: every point carries one dof with a unit entry (point_dof[q] in
    [0, num_dofs)) or none (anything else: -1, or a value >= num_dofs, which the dof scan ignores).  Returns a dict:
    first (INT_MAX: the dof has no point), kept, flag, cmap, owner_dof, unplaced, P = (ptr, col, val) or None when refused,
    row_len (-1 on the refused rows), refused, merged, coarse_point_dof."""
    point_dof = np.asarray(point_dof, np.int64)
    m, np3 = len(keep), n * n * n
    total = len(point_dof)
    E = total // np3
    pos = np.full(n, -1)
    for a in range(m):
        pos[keep[a]] = a
    v = np.arange(np3)
    node_kept = (pos[v % n] >= 0) & (pos[(v // n) % n] >= 0) & (pos[v // (n * n)] >= 0)
    first = np.full(num_dofs, INT_MAX, np.int64)
    kept = np.zeros(num_dofs, np.int32)
    for q in range(total):  # the serial scan
        d = point_dof[q]
        if d < 0 or d >= num_dofs:
            continue
        if first[d] == INT_MAX:
            first[d] = q
        if node_kept[q % np3]:
            kept[d] = 1
    flag = ((first == INT_MAX) | (kept != 0)).astype(np.int32)
    cmap = np.full(num_dofs, -1, np.int32)
    nc = 0
    for d in range(num_dofs):
        if flag[d]:
            cmap[d] = nc
            nc += 1
    owner_dof = np.full(total, -1, np.int32)
    placed = first != INT_MAX
    owner_dof[first[placed]] = np.nonzero(placed)[0]
    rows, merged = interp_rows_ref(cmap, first, point_dof, n, keep, lo, hi, wl)
    refused = any(r is None for r in rows)
    row_len = np.array([-1 if r is None else len(r) for r in rows], np.int32).reshape(num_dofs)
    P = None
    if not refused:
        ptr = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int32)
        col = np.array([c for r in rows for c, _ in r], np.int32)
        val = np.array([w for r in rows for _, w in r], np.float64)
        P = (ptr, col, val)
    cv = np.arange(m * m * m)
    keep = np.asarray(keep)
    fine_node = keep[cv % m] + keep[(cv // m) % m] * n + keep[cv // (m * m)] * n * n
    fq = (np.arange(E)[:, None] * np3 + fine_node[None, :]).ravel()
    fd = point_dof[fq]
    assert not (fd >= num_dofs).any(), "a kept lattice node carries a dof outside the matrix: not a valid input"
    coarse_point_dof = np.where(fd >= 0, cmap[np.maximum(fd, 0)] if num_dofs else -1, -1).astype(np.int32)
    return dict(first=first.astype(np.int32), kept=kept, flag=flag, cmap=cmap, owner_dof=owner_dof, unplaced=int((~placed).any()), P=P, row_len=row_len,
                refused=refused, merged=merged, coarse_point_dof=coarse_point_dof, num_coarse=nc)


# ----------------------------------------------------------------------------------------------------------------------
# the low-order FEM matrix
# ----------------------------------------------------------------------------------------------------------------------
def tet_matrices_ref(xs, ys, zs):
    """A_tet of low_order::assemble_fem for arrays of tetrahedra: xs, ys, zs of shape (4, T) -> At (4, 4, T) and det (T).
    One numpy statement per host statement."""
    H = [xs[0] - xs[3], xs[1] - xs[3], xs[2] - xs[3], ys[0] - ys[3], ys[1] - ys[3], ys[2] - ys[3], zs[0] - zs[3], zs[1] - zs[3], zs[2] - zs[3]]
    det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6])
    i_d = f64(1.0) / det
    iH = [i_d * (H[4] * H[8] - H[7] * H[5]), i_d * (H[2] * H[7] - H[8] * H[1]), i_d * (H[1] * H[5] - H[4] * H[2]),
          i_d * (H[5] * H[6] - H[8] * H[3]), i_d * (H[0] * H[8] - H[6] * H[2]), i_d * (H[2] * H[3] - H[5] * H[0]),
          i_d * (H[3] * H[7] - H[6] * H[4]), i_d * (H[1] * H[6] - H[7] * H[0]), i_d * (H[0] * H[4] - H[3] * H[1])]
    G = [[None] * 3 for _ in range(3)]
    for m in range(3):
        for nn in range(3):
            g = np.zeros_like(det)
            for k in range(3):
                g = g + (det / f64(24.0)) * iH[m * 3 + k] * iH[nn * 3 + k]
            G[m][nn] = g
    At = np.zeros((4, 4) + det.shape)
    for i in range(4):
        for j in range(4):
            a = np.zeros_like(det)
            m0, m1 = (i, i + 1) if i < 3 else (0, 3)
            n0, n1 = (j, j + 1) if j < 3 else (0, 3)
            minus = (i < 3) != (j < 3)
            for m in range(m0, m1):
                for nn in range(n0, n1):
                    g = -G[m][nn] if minus else G[m][nn]
                    for _ in range(4):
                        a = a + g
            At[i, j] = a
    return At, det


def fem_stencils_ref(x, y, z, point_dof, N, epsilon=1.0e-12):
    """The per-point K[27] and touched bits of low_order::assemble_fem, summed in the order sz, sy, sx, t (then i, j).
    Returns K (points, 27), mask (points, uint32) and the determinants of all tetrahedra (elements, cells, 6)."""
    n = N + 1
    n3 = n * n * n
    x, y, z = (np.asarray(a, np.float64) for a in (x, y, z))
    point_dof = np.asarray(point_dof)
    E = len(x) // n3
    sz, sy, sx = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")  # cells in the order sz, sy, sx
    sx, sy, sz = sx.ravel(), sy.ravel(), sz.ravel()
    # local index of vertex v of tetrahedron t of every cell: (cells, 6, 4)
    loc = (sx[:, None, None] + TETS[None, :, :, 0]) + (sy[:, None, None] + TETS[None, :, :, 1]) * n + (sz[:, None, None] + TETS[None, :, :, 2]) * n * n
    K = np.zeros((E * n3, 27))
    mask = np.zeros(E * n3, np.uint32)
    dets = np.zeros((E, len(sx), 6))
    d = TETS[:, None, :, :] - TETS[:, :, None, :]  # d[t, i, j] = tets[t][j] - tets[t][i]
    slot = (d[..., 0] + 1) + 3 * (d[..., 1] + 1) + 9 * (d[..., 2] + 1)
    slot = np.broadcast_to(slot[None], (len(sx), 6, 4, 4))
    for e in range(E):
        g = e * n3 + loc  # (cells, 6, 4)
        xs, ys, zs = (np.moveaxis(a[g], 2, 0) for a in (x, y, z))  # (4, cells, 6)
        At, det = tet_matrices_ref(xs, ys, zs)
        dets[e] = det
        At = np.moveaxis(At, (0, 1), (2, 3))  # (cells, 6, i, j)
        has = point_dof[g] >= 0
        sel = has[:, :, :, None] & has[:, :, None, :] & (np.abs(At) > epsilon)
        gi = np.broadcast_to(g[:, :, :, None], sel.shape)
        # K[slot] += At[i][j] in the host's order: ufunc.at is unbuffered and takes its operands one after the other, and
        # the boolean selection lists them in C order (cell = sz, sy, sx; then t, i, j)
        np.add.at(K, (gi[sel], slot[sel]), At[sel])
        np.bitwise_or.at(mask, gi[sel], np.uint32(1) << slot[sel].astype(np.uint32))
    return K, mask, dets


def from_triplets_ref(rows, ti, tj, tv):
    """low_order::from_triplets: per row the entries in arrival order, sorted stably by column, equal columns summed from
    the first one on."""
    ti, tj, tv = np.asarray(ti, np.int64), np.asarray(tj, np.int64), np.asarray(tv, np.float64)
    order = np.lexsort((np.arange(len(ti)), tj, ti))  # by row, then column, then arrival
    ptr = np.zeros(rows + 1, np.int64)
    col, val = [], []
    last_r, last_c = -1, -1
    for p in order:
        r, c = ti[p], tj[p]
        if r == last_r and c == last_c:
            val[-1] = f64(val[-1] + tv[p])
        else:
            col.append(c)
            val.append(f64(tv[p]))
            ptr[r + 1] += 1
        last_r, last_c = r, c
    return np.cumsum(ptr).astype(np.int32), np.array(col, np.int32), np.array(val, np.float64)


def assemble_fem_ref(x, y, z, point_dof, num_dofs, N, epsilon=1.0e-12):
    """low_order::assemble_fem: returns K, mask (per point), the merged CSR rows (ptr, col, val) and the determinants."""
    n = N + 1
    point_dof = np.asarray(point_dof, np.int64)
    K, mask, dets = fem_stencils_ref(x, y, z, point_dof, N, epsilon)
    # the element's merged entries, row by row, neighbours in ascending local index: points ascending, slots ascending
    g, s = np.nonzero((mask[:, None] >> np.arange(27, dtype=np.uint32)[None, :]) & np.uint32(1))
    assert (point_dof[g] >= 0).all()
    nb = g + (s % 3 - 1) + ((s // 3) % 3 - 1) * n + (s // 9 - 1) * n * n
    ptr, col, val = from_triplets_ref(num_dofs, point_dof[g], point_dof[nb], K[g, s])
    return K, mask, (ptr, col, val), dets


def add_diagonal_ref(ptr, col, val, shift):
    """Subdomain::amg_build after assemble_fem: the diagonal entry of row d plus shift[d], once, one double sum (the
    Helmholtz and Robin terms of the level-0 matrix; the coarse operators are Galerkin products of it)"""
    ptr, col, val = np.asarray(ptr), np.asarray(col), np.array(val, np.float64)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    on = np.nonzero(rows == col)[0]
    assert np.array_equal(rows[on], np.arange(len(ptr) - 1)), "a row without a diagonal entry"
    val[on] = val[on] + np.asarray(shift, np.float64)
    return val


def dof_points_ref(point_dof, num_dofs):
    """dof_ptr / dof_points: the ascending points of every dof, the transpose of point_dof"""
    point_dof = np.asarray(point_dof, np.int64)
    pts = np.nonzero((point_dof >= 0) & (point_dof < num_dofs))[0]
    order = np.argsort(point_dof[pts], kind="stable")
    counts = np.bincount(point_dof[pts], minlength=num_dofs)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), pts[order].astype(np.int32)
