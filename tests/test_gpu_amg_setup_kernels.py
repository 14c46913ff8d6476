"""The device AMG-setup entries that test_gpu_amg_device_setup.py reaches only through whole hierarchy builds, called one by
one on inputs built here: the six lattice entries, the three FEM entries, inv_sqrt_diagonal and unit_values
(csrc/fdd_amg_setup.hip) against the restatements of host/low_order.hpp in tests/amg_setup_restatements.py, which
test_cpu_amg_setup_restatements.py holds to the host build.  Integers must be equal, doubles equal as uint64 bits.

Every index array handed to a kernel is in range for the buffers it indexes (a point_dof value >= num_dofs sits only on
lattice nodes that no entry uses as an index, and never exceeds the guard band of the dof arrays); the refusals are those
an entry makes on the host before any launch.  Every output buffer lies between guard values that must survive."""
import ctypes

import numpy as np
import pytest
import torch

import amg_setup_restatements as R
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

pytestmark = pytest.mark.gpu

PAD = 8            # guard elements on either side of every output
GUARD_I = -777     # guard value of int buffers
FILL_I = -555      # what an int output holds before the call ("untouched" = still this)
GUARD_F, FILL_F = 777.0, -555.0
OUT_OF_RANGE = 4   # point_dof values in [num_dofs, num_dofs + OUT_OF_RANGE): within PAD of the dof arrays' ends


class Buf:
    """an output buffer of n elements between two guard bands"""

    def __init__(self, n, dtype):
        self.n = n
        self.guard, self.fill = (GUARD_F, FILL_F) if dtype == torch.float64 else (GUARD_I, FILL_I)
        self.whole = torch.full((n + 2 * PAD,), self.guard, dtype=dtype, device="cuda")
        self.view = self.whole[PAD : PAD + n]
        self.view.fill_(self.fill)

    @property
    def p(self):
        return lib.ptr(self.view) if self.n > 0 else lib.ptr(self.whole[PAD:])

    def get(self):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert (w[:PAD] == self.guard).all() and (w[PAD + self.n :] == self.guard).all(), "a guard value was overwritten"
        return w[PAD : PAD + self.n].copy()

    def untouched(self):
        return bool((self.get() == self.fill).all())


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def call(name, *args):
    return lib.hip().call(name, *args, lib.current_stream())


# ----------------------------------------------------------------------------------------------------------------------
# lattice entries
# ----------------------------------------------------------------------------------------------------------------------
def tables(n, keep):
    """lo / hi / wl of a kept set on Chebyshev-spaced nodes (weights that are no dyadic fractions); the kept sets below are
    not what low_order::coarse_nodes would choose"""
    ref = -np.cos(np.pi * np.arange(n) / (n - 1))
    lo, hi, wl = R.interp_tables_ref(ref, list(keep))
    return np.array(keep, np.int32), lo, hi, wl


def node_kept(n, keep):
    pos = np.zeros(n, bool)
    pos[list(keep)] = True
    v = np.arange(n**3)
    return pos[v % n] & pos[(v // n) % n] & pos[v // (n * n)]


def conforming_box(E, n):
    """(E, 1, 1) elements joined across their x faces, the nodes numbered on the global grid, a Dirichlet shell of -1 (where
    the shell would leave nothing -- n = 2 -- only the three lower faces)"""
    gx, gy, gz = E * (n - 1) + 1, n, n
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")  # k slowest ... x fastest below
    lz, ly, lx = i.ravel(), j.ravel(), k.ravel()
    e = np.arange(E)[:, None]
    X, Y, Z = e * (n - 1) + lx[None], 0 * e + ly[None], 0 * e + lz[None]
    shell = (X == 0) | (Y == 0) | (Z == 0) | (X == gx - 1) | (Y == gy - 1) | (Z == gz - 1)
    if shell.all():
        shell = (X == 0) | (Y == 0) | (Z == 0)
    node = X + gx * (Y + gy * Z)
    ids = np.unique(node[~shell])
    number = np.full(gx * gy * gz, -1)
    number[ids] = np.arange(len(ids))
    return np.where(shell, -1, number[node]).ravel().astype(np.int32), len(ids)


def random_sharing(E, n, keep, seed):
    """a dof on many points of many elements; the kept nodes draw from six dofs, so two kept nodes of one element share one
    (the equal-column merge); every seventh dof has no point (unplaced); values >= num_dofs on some nodes that are not kept"""
    rng = np.random.default_rng(seed)
    points = E * n**3
    nd = max(8, points // 3)
    pool = np.array([d for d in range(nd) if d % 7 != 3])
    pd = np.where(rng.random(points) < 0.1, -1, pool[rng.integers(0, len(pool), points)])
    kept_node = np.tile(node_kept(n, keep), E)
    few = np.array([-1, 0, 1, 2, 4, 5, 6])
    pd[kept_node] = few[rng.integers(0, len(few), int(kept_node.sum()))]
    outside = ~kept_node & (rng.random(points) < 0.03)
    pd[outside] = nd + rng.integers(0, OUT_OF_RANGE, int(outside.sum()))
    return pd.astype(np.int32), nd


class LatticeChain:
    """the six entries in the header's order, every output in a guarded buffer"""

    def __init__(self, pd, nd, E, n, keep, lo, hi, wl):
        self.nd, self.E, self.n, self.m = nd, E, n, len(keep)
        self.points = E * n**3
        self.tab = (n, self.m, lib.ptr(keep), lib.ptr(lo), lib.ptr(hi), lib.ptr(wl))
        self._host = (keep, lo, hi, wl)  # the host tables outlive the calls
        self.pd = dev(pd if len(pd) else np.full(1, -1), np.int32)  # no element: still a pointer, never read
        i32 = torch.int32
        self.first, self.kept, self.flag, self.cmap, self.row_len = (Buf(nd, i32) for _ in range(5))
        self.cstart, self.P_ptr = Buf(nd + 1, i32), Buf(nd + 1, i32)
        self.owner, self.unplaced = Buf(self.points, i32), Buf(1, i32)
        self.coarse = Buf(E * self.m**3, i32)

    def to_row_lengths(self, interp_pd=None):
        nd = self.nd
        call("fdd_amg_setup_lattice_dofs", self.first.p, self.kept.p, lib.ptr(self.pd), self.E, nd, *self.tab)
        call("fdd_amg_setup_lattice_coarse_flags", self.flag.p, self.first.p, self.kept.p, nd)
        self.cstart_h = np.zeros(nd + 1, np.int32)
        call("fdd_amg_setup_row_pointers", self.cstart.p, lib.ptr(self.cstart_h), self.flag.p, nd)
        call("fdd_amg_setup_lattice_cmap", self.cmap.p, self.owner.p, self.unplaced.p, self.cstart.p, self.first.p, self.kept.p, self.points, nd)
        self.interp_pd = self.pd if interp_pd is None else dev(interp_pd, np.int32)
        call("fdd_amg_setup_lattice_interp_count", self.row_len.p, self.cmap.p, self.first.p, lib.ptr(self.interp_pd), nd, *self.tab)

    def to_the_end(self):
        nd = self.nd
        self.P_ptr_h = np.zeros(nd + 1, np.int32)
        call("fdd_amg_setup_row_pointers", self.P_ptr.p, lib.ptr(self.P_ptr_h), self.row_len.p, nd)  # refuses a row length of -1
        nnz = int(self.P_ptr_h[-1])
        self.P_col, self.P_val = Buf(nnz, torch.int32), Buf(nnz, torch.float64)
        call("fdd_amg_setup_lattice_interp_fill", self.P_col.p, self.P_val.p, self.P_ptr.p, self.cmap.p, self.first.p, lib.ptr(self.interp_pd), nd, *self.tab)
        call("fdd_amg_setup_lattice_coarse_points", self.coarse.p, lib.ptr(self.pd), self.cmap.p, self.E, *self.tab)


def check_level(pd, nd, E, n, keep):
    keep, lo, hi, wl = tables(n, keep)
    g = R.geometric_level_ref(pd, nd, n, list(keep), lo, hi, wl)
    assert not g["refused"]
    # in range: what the entries index the dof arrays with lies in [0, nd) or, unused as an index, within the guard band
    assert pd.min() >= -1 and pd.max() < nd + OUT_OF_RANGE <= nd + PAD and (pd[np.tile(node_kept(n, keep), E)] < nd).all()
    c = LatticeChain(pd, nd, E, n, keep, lo, hi, wl)
    c.to_row_lengths()
    for name, buf in (("first", c.first), ("kept", c.kept), ("flag", c.flag), ("cmap", c.cmap), ("owner_dof", c.owner), ("row_len", c.row_len)):
        assert np.array_equal(buf.get(), g[name]), name
    assert int(c.unplaced.get()[0]) == g["unplaced"]
    assert np.array_equal(c.cstart.get(), c.cstart_h) and c.cstart_h[-1] == g["num_coarse"]
    c.to_the_end()
    ptr, col, val = g["P"]
    assert np.array_equal(c.P_ptr.get(), ptr) and np.array_equal(c.P_ptr_h, ptr)
    assert np.array_equal(c.P_col.get(), col)
    assert np.array_equal(bits(c.P_val.get()), bits(val))
    assert np.array_equal(c.coarse.get(), g["coarse_point_dof"])
    return g, c


# (n, keep, the second E).  Points of one element: n^3; for n = 8, 16, 32 that is a multiple of the 256 lanes of a
# workgroup whatever E is, so there the ragged last workgroup is that of the launches over dofs and over coarse points
# (n = 32: already at E = 1, 27000 dofs and 125 coarse points; a second element only doubles the restatement's time).
LATTICES = [(2, (0, 1), 37), (3, (0, 2), 11), (5, (0, 2, 4), 3), (8, (0, 3, 4, 7), 3), (8, (0, 1, 2, 3, 7), 3), (16, (0, 15), 2), (32, (0, 5, 16, 26, 31), 1)]
LATTICE_IDS = ["n%d_keep%s" % (n, "-".join(map(str, k))) for n, k, _ in LATTICES]


@pytest.mark.parametrize("n,keep,E2", LATTICES, ids=LATTICE_IDS)
def test_lattice_chain_on_a_conforming_box(gpu, n, keep, E2):
    """family (a): a box numbered here, not by the host layer, with its Dirichlet shell of -1.  n = 2, 3, 5, 32 are lattice
    sizes no hierarchy build runs (branch: n other than 16, 8, 5, 4, up to the declared 32), and none of the kept sets is
    low_order::coarse_nodes' choice for its n except {0, n - 1} at n <= 4 (branch: kept sets that are not the host's own)."""
    for E in sorted({1, E2}):
        pd, nd = conforming_box(E, n)
        g, c = check_level(pd, nd, E, n, keep)
        assert g["unplaced"] == 0 and g["merged"] == 0
        if E == E2:
            assert any(size % 256 for size in (c.points, nd, E * len(keep) ** 3)), "no ragged workgroup in this case"


@pytest.mark.parametrize("n,keep,E2", LATTICES, ids=LATTICE_IDS)
def test_lattice_chain_on_randomly_shared_dofs(gpu, n, keep, E2):
    """family (b).  Branches: `unplaced` set (dofs without a point); the merge of equal coarse columns in a row
    (rc[k] == rc[k - 1]: two kept nodes of one element on one dof); a point_dof value >= num_dofs ignored by the dof scan."""
    merged = outside = 0
    for E in sorted({1, E2}):
        pd, nd = random_sharing(E, n, keep, 100 * n + E)
        g, c = check_level(pd, nd, E, n, keep)
        assert g["unplaced"] == 1                     # branch: unplaced
        merged += g["merged"]
        outside += int((pd >= nd).sum())
        # corrupt nothing: the dofs' own arrays are what the restatement gives (checked above) and the guards stand
    if len(keep) < n:  # n = 2 keeps every node: no interpolated row, no node that is not kept
        assert merged > 0                             # branch: rc[k] == rc[k - 1]
        assert outside > 0                            # branch: d >= num_dofs in the dof scan


def test_lattice_row_of_a_kept_node_whose_dof_is_not_kept_is_refused(gpu):
    """family (c), branch row_len = -1.  Inside one chain a kept node's dof is always kept, so the rows are handed another
    point_dof than the one the dof scan saw: the lower kept corner of a dof that is not kept now carries a second dof that
    is not kept (in range, and a valid point -> dof array of its own).  interp_count writes -1 on that row, the second
    row_pointers call raises, and nothing later is called."""
    n, keep, E = 8, (0, 3, 4, 7), 3
    pd, nd = random_sharing(E, n, keep, 5)
    keep_a, lo, hi, wl = tables(n, keep)
    g = R.geometric_level_ref(pd, nd, n, list(keep), lo, hi, wl)
    dropped = np.nonzero(g["cmap"] < 0)[0]
    d0, d1 = int(dropped[0]), int(dropped[1])
    q = int(g["first"][d0])
    e, v = q // n**3, q % n**3
    corner = sum(int(keep_a[lo[(v // n**a) % n]]) * n**a for a in range(3))
    other = pd.copy()
    other[e * n**3 + corner] = d1
    assert 0 <= other.min() + 1 and (other[np.tile(node_kept(n, keep), E)] < nd).all()
    rows, _ = R.interp_rows_ref(g["cmap"], g["first"], other, n, list(keep), lo, hi, wl)
    expect = np.array([-1 if r is None else len(r) for r in rows], np.int32)
    assert expect[d0] == -1
    c = LatticeChain(pd, nd, E, n, keep_a, lo, hi, wl)
    c.to_row_lengths(interp_pd=other)
    assert np.array_equal(c.cmap.get(), g["cmap"])
    assert np.array_equal(c.row_len.get(), expect)
    with pytest.raises(lib.FddError) as exc:
        c.to_the_end()
    assert "fdd_amg_setup_row_pointers" in str(exc.value)
    assert c.P_ptr.untouched() and c.coarse.untouched()


def lattice_entries(c, nd, E):
    """the four entries that take the tables, on valid buffers"""
    return {
        "fdd_amg_setup_lattice_dofs": ((c.first, c.kept), lambda tab: (c.first.p, c.kept.p, lib.ptr(c.pd), E, nd) + tab),
        "fdd_amg_setup_lattice_interp_count": ((c.row_len,), lambda tab: (c.row_len.p, c.cmap.p, c.first.p, lib.ptr(c.pd), nd) + tab),
        "fdd_amg_setup_lattice_interp_fill": ((c.P_col, c.P_val), lambda tab: (c.P_col.p, c.P_val.p, c.P_ptr.p, c.cmap.p, c.first.p, lib.ptr(c.pd), nd) + tab),
        "fdd_amg_setup_lattice_coarse_points": ((c.coarse,), lambda tab: (c.coarse.p, lib.ptr(c.pd), c.cmap.p, E) + tab),
    }


def test_lattice_tables_are_refused_before_any_launch(gpu):
    """n = 1, n = 33, m = 1, m = n + 1, keep[a], lo or hi out of range, a NULL table: every entry that takes the tables
    raises and leaves its sentinel-filled outputs as they were"""
    n, E = 4, 1
    pd, nd = conforming_box(E, n)
    big = 40  # the tables are long enough for every n tried, whatever the entry reads before it refuses
    keep, lo, hi = np.zeros(big, np.int32), np.zeros(big, np.int32), np.zeros(big, np.int32)
    keep[1] = n - 1
    hi[1:] = 1
    lo[n - 1] = 1
    wl = np.full(big, 0.5)

    def variant(n_=n, m_=2, keep_=keep, lo_=lo, hi_=hi, wl_=wl, edit=None):
        arrays = [a.copy() if a is not None else None for a in (keep_, lo_, hi_, wl_)]
        if edit:
            edit(*arrays)
        return (n_, m_) + tuple(arrays)

    def put(which, index, value):
        def edit(*arrays):
            arrays[which][index] = value
        return edit

    bad = {
        "n=1": variant(n_=1, m_=1), "n=33": variant(n_=33), "m=1": variant(m_=1), "m=n+1": variant(m_=n + 1),
        "keep<0": variant(edit=put(0, 1, -1)), "keep=n": variant(edit=put(0, 1, n)),
        "lo<0": variant(edit=put(1, 2, -1)), "lo=m": variant(edit=put(1, 2, 2)), "hi<0": variant(edit=put(2, 2, -1)), "hi=m": variant(edit=put(2, 2, 2)),
        "keep NULL": variant(keep_=None), "lo NULL": variant(lo_=None), "hi NULL": variant(hi_=None), "wl NULL": variant(wl_=None),
    }
    c = LatticeChain(pd, nd, E, n, keep[:2].copy(), lo[:n].copy(), hi[:n].copy(), wl[:n].copy())
    c.P_col, c.P_val = Buf(8 * nd, torch.int32), Buf(8 * nd, torch.float64)
    for name, (outs, args) in lattice_entries(c, nd, E).items():
        for what, (n_, m_, k_, l_, h_, w_) in bad.items():
            tab = (n_, m_, lib.ptr(k_), lib.ptr(l_), lib.ptr(h_), lib.ptr(w_))
            with pytest.raises(lib.FddError) as exc:
                call(name, *args(tab))
            assert name in str(exc.value) and "lattice tables" in str(exc.value), (name, what)
            assert all(o.untouched() for o in outs), (name, what)
    # the good tables are good: the same calls pass
    c.to_row_lengths()
    c.to_the_end()
    torch.cuda.synchronize()


def test_lattice_zero_sizes_launch_nothing(gpu):
    n, keep = 4, (0, 3)
    keep, lo, hi, wl = tables(n, keep)
    # num_dofs = 0 (every point without a dof): nothing is written but the cmap entry's own clears (owner_dof = -1 on every
    # point, unplaced = 0), the two one-entry row pointers and the coarse lattice's -1
    c = LatticeChain(np.full(2 * n**3, -1, np.int32), 0, 2, n, keep, lo, hi, wl)
    c.to_row_lengths()
    c.to_the_end()
    assert c.cstart_h[0] == 0 and c.P_ptr_h[0] == 0 and list(c.cstart.get()) == [0] and list(c.P_ptr.get()) == [0]
    assert (c.owner.get() == -1).all() and list(c.unplaced.get()) == [0]
    assert (c.coarse.get() == -1).all()
    for empty in (c.first, c.kept, c.flag, c.cmap, c.row_len, c.P_col, c.P_val):
        assert empty.n == 0 and len(empty.get()) == 0  # .get() checks the guards on either side of nothing
    # num_elements = 0 with dofs: the dof scan clears its outputs (no point: INT_MAX, not kept), the rest follows, no point is read
    nd = 5
    c = LatticeChain(np.zeros(0, np.int32), nd, 0, n, keep, lo, hi, wl)
    c.to_row_lengths()
    c.to_the_end()
    assert (c.first.get() == R.INT_MAX).all() and not c.kept.get().any() and (c.flag.get() == 1).all()
    assert list(c.cmap.get()) == list(range(nd)) and list(c.unplaced.get()) == [1] and (c.row_len.get() == 1).all()
    assert list(c.P_col.get()) == list(range(nd)) and (c.P_val.get() == 1.0).all()
    assert c.owner.n == 0 and c.coarse.n == 0 and len(c.owner.get()) == 0 and len(c.coarse.get()) == 0


# ----------------------------------------------------------------------------------------------------------------------
# FEM entries
# ----------------------------------------------------------------------------------------------------------------------
def element_coordinates(E, N, perturbed):
    """elements side by side in x on Chebyshev-spaced nodes under a sheared affine map (every entry of a tetrahedron's H
    is non-zero); perturbed: plus a smooth displacement small enough that every determinant stays positive"""
    n = N + 1
    r = 0.5 * (1.0 - np.cos(np.pi * np.arange(n) / N))
    k, j, i = np.meshgrid(r, r, r, indexing="ij")
    X = (np.arange(E)[:, None] + i.ravel()[None]).ravel()
    Y, Z = np.tile(j.ravel(), E), np.tile(k.ravel(), E)
    if perturbed:
        s = 0.04 * np.sin(2.1 * X + 0.3) * np.sin(1.7 * Y + 0.2) * np.sin(2.6 * Z + 0.1)
        X, Y, Z = X + s, Y - 0.7 * s, Z + 0.5 * s
    return 1.1 * X + 0.2 * Y + 0.1 * Z, 0.15 * X + 0.9 * Y - 0.1 * Z, -0.05 * X + 0.25 * Y + 1.3 * Z


def fem_point_dofs(variant, E, N, seed):
    n = N + 1
    rng = np.random.default_rng(seed)
    if variant == "conforming":
        return conforming_box(E, n)
    if variant == "shared":  # a handful of dofs on all the points: some dof owns more than 8 of them
        nd = max(2, E * n**3 // 12)
        return rng.integers(0, nd, E * n**3).astype(np.int32), nd
    pd, nd = conforming_box(E, n)  # "holes": -1 points scattered inside; the dofs that lose all their points keep an empty row
    pd[rng.random(len(pd)) < 0.2] = -1
    return pd, nd


def device_fem(x, y, z, pd, nd, N, E, eps):
    points = len(pd)
    K, mask = Buf(points * 27, torch.float64), Buf(points, torch.int32)
    dpd, dx, dy, dz = dev(pd, np.int32), dev(x, np.float64), dev(y, np.float64), dev(z, np.float64)
    call("fdd_amg_setup_fem_stencils", K.p, mask.p, lib.ptr(dx), lib.ptr(dy), lib.ptr(dz), lib.ptr(dpd), N, E, ctypes.c_double(eps))
    dof_ptr, dof_points = R.dof_points_ref(pd, nd)
    assert len(dof_points) == 0 or (dof_points.min() >= 0 and dof_points.max() < points)
    dp, dq = dev(dof_ptr, np.int32), dev(dof_points if len(dof_points) else np.zeros(1), np.int32)
    row_len = Buf(nd, torch.int32)
    call("fdd_amg_setup_fem_count", row_len.p, lib.ptr(dp), lib.ptr(dq), mask.p, lib.ptr(dpd), N, nd)
    A_ptr, A_ptr_h = Buf(nd + 1, torch.int32), np.zeros(nd + 1, np.int32)
    call("fdd_amg_setup_row_pointers", A_ptr.p, lib.ptr(A_ptr_h), row_len.p, nd)
    nnz = int(A_ptr_h[-1])
    A_col, A_val = Buf(nnz, torch.int32), Buf(nnz, torch.float64)
    call("fdd_amg_setup_fem_fill", A_col.p, A_val.p, A_ptr.p, lib.ptr(dp), lib.ptr(dq), mask.p, K.p, lib.ptr(dpd), N, nd)
    assert np.array_equal(A_ptr.get(), A_ptr_h)
    return K.get().reshape(points, 27), mask.get().view(np.uint32), (A_ptr_h, A_col.get(), A_val.get()), dof_ptr


@pytest.mark.parametrize("perturbed", [False, True], ids=["affine", "perturbed"])
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("N", [1, 2, 3, 7])
def test_fem_chain_equals_assemble_fem(gpu, N, E, perturbed):
    """fem_stencils -> fem_count -> row_pointers -> fem_fill against assemble_fem_ref: K as bits, mask equal, rows equal in
    ptr and col and as bits in val; with epsilon = 1e-12 and with one that drops entries (mask bits, the
    not(fabs(a) > epsilon) branch)"""
    x, y, z = element_coordinates(E, N, perturbed)
    dropped_something = False
    for variant in ("conforming", "shared", "holes"):
        pd, nd = fem_point_dofs(variant, E, N, 10 * N + E)
        ref_default = None
        for eps in (1.0e-12, None):
            if eps is None:  # between the small and the large entries of the default stencils: some are dropped, not all
                mags = np.abs(ref_default[0][ref_default[0] != 0.0])
                if len(mags) == 0:
                    continue
                eps = float(np.quantile(mags, 0.3))
            Kr, maskr, (ptr, col, val), dets = R.assemble_fem_ref(x, y, z, pd, nd, N, eps)
            assert dets.min() > 0.0, "a tetrahedron of the test's own mesh is inverted"
            if ref_default is None:
                ref_default = (Kr, maskr)
            elif not np.array_equal(maskr, ref_default[1]):
                dropped_something = True
            K, mask, (dptr, dcol, dval), dof_ptr = device_fem(x, y, z, pd, nd, N, E, eps)
            case = (variant, eps)
            assert np.array_equal(mask, maskr), case
            assert np.array_equal(bits(K), bits(Kr)), case
            assert np.array_equal(dptr, ptr) and np.array_equal(dcol, col), case
            assert np.array_equal(bits(dval), bits(val)), case
            if variant == "shared" and E * (N + 1) ** 3 >= 27:
                assert np.diff(dof_ptr).max() > 8, case  # branch: a dof on more than 8 points in fem_row_kernel
    assert dropped_something  # the large epsilon really drops entries


# ----------------------------------------------------------------------------------------------------------------------
# the two small entries
# ----------------------------------------------------------------------------------------------------------------------
def csr_with_diagonal_cases(rows, seed):
    """row i by i % 4: no diagonal entry | the diagonal stored last | stored first | an explicitly stored 0.0 diagonal"""
    rng = np.random.default_rng(seed)
    ptr, col, val, diag = [0], [], [], []
    for i in range(rows):
        others = [c for c in rng.choice(rows + 3, size=int(rng.integers(0, 5)), replace=False) if c != i]
        vals = list(rng.uniform(0.5, 2.0, len(others)))
        kind, d = i % 4, float(rng.uniform(0.1, 9.0))
        if kind == 0:
            d = 0.0  # what low_order::diagonal leaves where no entry is stored
        else:
            d = 0.0 if kind == 3 else d
            at = len(others) if kind == 1 else 0 if kind == 2 else len(others) // 2
            others.insert(at, i)
            vals.insert(at, d)
        col += others
        val += vals
        diag.append(d)
        ptr.append(len(col))
    return np.array(ptr, np.int32), np.array(col, np.int32), np.array(val), np.array(diag)


SINGLE_ROWS = [([1, 2], [0.7, 1.9], 0.0), ([1, 2, 0], [0.7, 1.9, 3.3], 3.3), ([0, 1, 2], [3.3, 0.7, 1.9], 3.3), ([1, 0, 2], [0.7, 0.0, 1.9], 0.0)]  # the four kinds as one row each


@pytest.mark.parametrize("rows", [1, 255, 257])
def test_inv_sqrt_diagonal(gpu, rows):
    """bits of 1.0 / np.sqrt(d).  Branch: a row without a diagonal entry (d stays 0.0, D = inf, as the header states); the
    diagonal stored last, first, and stored as 0.0"""
    if rows == 1:
        matrices = [(np.array([0, len(c)], np.int32), np.array(c, np.int32), np.array(v), np.array([d])) for c, v, d in SINGLE_ROWS]
    else:
        matrices = [csr_with_diagonal_cases(rows, 40)]
    for ptr, col, val, diag in matrices:
        D = Buf(rows, torch.float64)
        dptr, dcol, dval = dev(ptr, np.int32), dev(col, np.int32), dev(val, np.float64)
        call("fdd_amg_setup_inv_sqrt_diagonal", D.p, lib.ptr(dptr), lib.ptr(dcol), lib.ptr(dval), rows)
        with np.errstate(divide="ignore"):
            expect = 1.0 / np.sqrt(diag)
        assert np.array_equal(bits(D.get()), bits(expect)), (rows, list(col[:4]))
        if rows > 1:
            assert np.isinf(expect[0::4]).all() and np.isinf(expect[3::4]).all() and np.isfinite(expect[1::4]).all() and np.isfinite(expect[2::4]).all()


def test_unit_values(gpu):
    """flag = 1 iff every value is exactly 1.0.  The kernel is a grid-stride loop on fdd_stream_grid(nnz, 256) workgroups,
    at most FDD_REDUCE_MAX_BLOCKS = 2048 of them: the loop runs a second trip from nnz = 2048 * 256 + 1 = 524289 on, the
    smallest such nnz, and then the very last value is read on that second trip (branch: a non-unit value at the very end
    of a long value array)."""
    second_trip = 2048 * 256 + 1
    flag = Buf(1, torch.int32)
    call("fdd_amg_setup_unit_values", flag.p, lib.ptr(None), 0)
    assert list(flag.get()) == [1]
    for nnz in (1, 1000, second_trip):
        val = torch.ones(nnz, dtype=torch.float64, device="cuda")
        flag = Buf(1, torch.int32)
        call("fdd_amg_setup_unit_values", flag.p, lib.ptr(val), nnz)
        assert list(flag.get()) == [1], nnz
        for other in (1.0 + 2.0**-52, -1.0, 0.0, float("nan")):
            for at in sorted({0, nnz // 2, nnz - 1}):
                val[at] = other
                flag = Buf(1, torch.int32)
                call("fdd_amg_setup_unit_values", flag.p, lib.ptr(val), nnz)
                assert list(flag.get()) == [0], (nnz, other, at)
                val[at] = 1.0
