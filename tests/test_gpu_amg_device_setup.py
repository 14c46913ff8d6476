"""The low-order AMG hierarchy built on the device ("amg_device_setup", csrc/fdd_amg_setup.hip) against the host build.

The host setup (host/low_order.hpp) fixes the order of every sum, so the device build must reproduce it bit for bit.
Held here: spgemm_count / _fill (against gustavson() below), transpose_count / _fill (against scipy), row_pointers (its
overflow refusal), and whole hierarchies against the host's, level by level, as uint64 bits.  The other eleven setup
entries -- fem_stencils / _count / _fill, inv_sqrt_diagonal, unit_values, the six lattice_* -- run here only inside those
hierarchy builds; entry by entry they are held in test_gpu_amg_setup_kernels.py, against the restatements of
tests/amg_setup_restatements.py."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def own_stream(gpu):
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    yield True
    H.init(0)


# ----------------------------------------------------------------------------------------------------------------------
# kernel entries
# ----------------------------------------------------------------------------------------------------------------------
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _sync():
    torch.cuda.synchronize()


def device_spgemm(A, B):
    L = lib.hip()
    s = lib.current_stream()
    ap, ac, av = _dev(A.indptr, np.int32), _dev(A.indices, np.int32), _dev(A.data, np.float64)
    bp, bc, bv = _dev(B.indptr, np.int32), _dev(B.indices, np.int32), _dev(B.data, np.float64)
    n = A.shape[0]
    length = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    cursor = torch.zeros(max(A.nnz, 1), dtype=torch.int32, device="cuda")
    L.call("fdd_amg_setup_spgemm_count", lib.ptr(length), lib.ptr(cursor), lib.ptr(ap), lib.ptr(ac), lib.ptr(bp), lib.ptr(bc), n, B.shape[0], s)
    cp = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    cp_h = np.zeros(n + 1, np.int32)
    L.call("fdd_amg_setup_row_pointers", lib.ptr(cp), lib.ptr(cp_h), lib.ptr(length), n, s)
    nnz = int(cp_h[-1])
    cc = torch.zeros(max(nnz, 1), dtype=torch.int32, device="cuda")
    cv = torch.zeros(max(nnz, 1), dtype=torch.float64, device="cuda")
    L.call("fdd_amg_setup_spgemm_fill", lib.ptr(cc), lib.ptr(cv), lib.ptr(cursor), lib.ptr(cp), lib.ptr(ap), lib.ptr(ac), lib.ptr(av), lib.ptr(bp), lib.ptr(bc), lib.ptr(bv), n, B.shape[0], s)
    _sync()
    return cp_h, cc.cpu().numpy()[:nnz], cv.cpu().numpy()[:nnz]


def device_transpose(A, drop_tol=-1.0):
    L = lib.hip()
    s = lib.current_stream()
    ap, ac, av = _dev(A.indptr, np.int32), _dev(A.indices, np.int32), _dev(A.data, np.float64)
    rows, cols = A.shape
    length = torch.zeros(max(cols, 1), dtype=torch.int32, device="cuda")
    L.call("fdd_amg_setup_transpose_count", lib.ptr(length), lib.ptr(ap), lib.ptr(ac), lib.ptr(av), rows, cols, ctypes.c_double(drop_tol), s)
    tp = torch.zeros(cols + 1, dtype=torch.int32, device="cuda")
    tp_h = np.zeros(cols + 1, np.int32)
    L.call("fdd_amg_setup_row_pointers", lib.ptr(tp), lib.ptr(tp_h), lib.ptr(length), cols, s)
    nnz = int(tp_h[-1])
    tc = torch.zeros(max(nnz, 1), dtype=torch.int32, device="cuda")
    tv = torch.zeros(max(nnz, 1), dtype=torch.float64, device="cuda")
    cursor = torch.zeros(max(cols, 1), dtype=torch.int32, device="cuda")
    src = torch.zeros(max(nnz, 1), dtype=torch.int32, device="cuda")
    L.call("fdd_amg_setup_transpose_fill", lib.ptr(tc), lib.ptr(tv), lib.ptr(cursor), lib.ptr(src), lib.ptr(tp), lib.ptr(ap), lib.ptr(ac), lib.ptr(av), rows, cols, nnz, ctypes.c_double(drop_tol), s)
    _sync()
    return tp_h, tc.cpu().numpy()[:nnz], tv.cpu().numpy()[:nnz]


def gustavson(A, B):
    """low_order::multiply restated: acc[j] = 0.0, then += a*b in the order of A's row, then B's row; columns sorted."""
    ptr, col, val = [0], [], []
    for i in range(A.shape[0]):
        acc = {}
        for p in range(A.indptr[i], A.indptr[i + 1]):
            k, a = A.indices[p], A.data[p]
            for q in range(B.indptr[k], B.indptr[k + 1]):
                j = B.indices[q]
                if j not in acc:
                    acc[j] = np.float64(0.0)
                acc[j] = np.float64(acc[j] + np.float64(a) * np.float64(B.data[q]))
        for j in sorted(acc):
            col.append(j)
            val.append(acc[j])
        ptr.append(len(col))
    return np.array(ptr, np.int32), np.array(col, np.int32), np.array(val, np.float64)


def random_csr(rng, rows, cols, density, long_rows=()):
    M = sp.random(rows, cols, density=density, format="lil", random_state=rng, data_rvs=lambda k: rng.standard_normal(k))
    for r in long_rows:
        M[r, :] = rng.standard_normal(cols)
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def test_spgemm_is_bitwise_gustavson(own_stream):
    rng = np.random.default_rng(7)
    cases = [
        (random_csr(rng, 60, 40, 0.08), random_csr(rng, 40, 50, 0.1)),
        (random_csr(rng, 30, 250, 0.02, long_rows=(3, 17)), random_csr(rng, 250, 80, 0.05)),  # rows of > 200 products
        (sp.csr_matrix((20, 30)), random_csr(rng, 30, 10, 0.2)),                               # all rows empty
    ]
    A0, B0 = cases[0]
    A0 = A0.tolil()
    A0[5, :] = 0  # an empty row among full ones
    cases[0] = (sp.csr_matrix(A0), B0)
    cases[0][0].eliminate_zeros()
    for A, B in cases:
        A.sort_indices()
        B.sort_indices()
        hp, hc, hv = gustavson(A, B)
        dp, dc, dv = device_spgemm(A, B)
        assert np.array_equal(hp, dp) and np.array_equal(hc, dc)
        assert np.array_equal(hv.view(np.uint64), dv.view(np.uint64))
    long = cases[1][0]
    assert max(sum(np.diff(cases[1][1].indptr)[long.indices[long.indptr[r]:long.indptr[r + 1]]]) for r in (3, 17)) > 200


def test_transpose_equals_scipy(own_stream):
    rng = np.random.default_rng(11)
    for A in (random_csr(rng, 70, 45, 0.1), random_csr(rng, 5, 300, 0.3), sp.csr_matrix((4, 6))):
        A.sort_indices()
        T = A.T.tocsr()
        T.sort_indices()
        tp, tc, tv = device_transpose(A)
        assert np.array_equal(tp, T.indptr) and np.array_equal(tc, T.indices)
        assert np.array_equal(tv.view(np.uint64), T.data.view(np.uint64))
    # drop_tol >= 0: entries of magnitude <= drop_tol are left out, as CSR_Matrix::transpose does
    A = sp.csr_matrix(np.array([[1.0, 1e-14, 0.0], [0.0, 2.0, -1e-13], [3.0, 0.0, 4.0]]))
    tp, tc, tv = device_transpose(A, 1e-12)
    assert list(tp) == [0, 2, 3, 4] and list(tc) == [0, 2, 1, 2] and list(tv) == [1.0, 3.0, 2.0, 4.0]


def test_row_pointer_overflow_is_an_error(own_stream):
    L = lib.hip()
    length = _dev(np.array([2**30, 2**30, 2**30], np.int32), np.int32)
    ptr = torch.zeros(4, dtype=torch.int32, device="cuda")
    ptr_h = np.zeros(4, np.int32)
    with pytest.raises(lib.FddError) as exc:
        L.call("fdd_amg_setup_row_pointers", lib.ptr(ptr), lib.ptr(ptr_h), lib.ptr(length), 3, lib.current_stream())
    assert "int range" in str(exc.value)


# ----------------------------------------------------------------------------------------------------------------------
# hierarchies: device build against host build
# ----------------------------------------------------------------------------------------------------------------------
def make_box(E, N, red=2, faces="DDDDDD"):
    p = H.Problem.box(E, (1, 1, 1), N, red, True, faces=faces)
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
    return p


def make_kershaw(E, N, eps, red=2, faces="DDDDDD"):
    p = H.Problem.kershaw(E, (1, 1, 1), N, red, eps, faces=faces)
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
    return p


def make_curved(directory, E=(3, 2, 2), N=7, red=6):
    for deg in S.level_degrees(N, red):
        S.write_mesh_files(directory, S.DeformedMesh(E, deg, 0.05))
    return H.Problem.from_directory(directory, N, red)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same_hierarchy(ph, pd):
    Lh, Ld = ph.amg_levels(), pd.amg_levels()
    assert len(Lh) == len(Ld)
    for l, (h, d) in enumerate(zip(Lh, Ld)):
        for key in ("A", "P"):
            if h[key] is None:
                assert d[key] is None, (l, key)
                continue
            assert h[key].shape == d[key].shape, (l, key)
            assert np.array_equal(h[key].indptr, d[key].indptr), (l, key)
            assert np.array_equal(h[key].indices, d[key].indices), (l, key)
            assert np.array_equal(bits(h[key].data), bits(d[key].data)), (l, key)
        assert np.array_equal(bits(h["D"]), bits(d["D"])), (l, "D")
        assert np.array_equal(bits(h["coefs"]), bits(d["coefs"])), (l, "coefs")
        assert ph.amg_level_transfer(l) == pd.amg_level_transfer(l), l
    return len(Lh)


def build_pair(make, device_min_levels):
    ph, pd = make(), make()
    nh = ph.amg_build(device=False)
    nd = pd.amg_build(device=True)
    assert nh == nd
    assert ph.amg_setup_info()["levels_built_on_device"] == 0
    info = pd.amg_setup_info()
    assert info["levels_built_on_device"] >= device_min_levels, info
    assert info["setup_seconds"] > 0.0
    return ph, pd


@pytest.mark.parametrize(
    "E,N,device_min_levels",
    [((4, 3, 5), 7, 3), ((3, 3, 3), 15, 3), ((4, 4, 4), 4, 1), ((3, 3, 3), 3, 1)],
    ids=["box435_N7", "box3_N15", "box4_N4", "box3_N3_handoff_at_0"],
)
def test_device_hierarchy_is_the_host_hierarchy(own_stream, E, N, device_min_levels):
    ph, pd = build_pair(lambda: make_box(E, N), device_min_levels)
    try:
        assert_same_hierarchy(ph, pd)
        if N == 3:
            assert pd.amg_setup_info()["levels_built_on_device"] == 1  # no lattice level: the device FEM matrix is handed over at level 0
        r = S.seeded_uniform(ph.n, 5) - 0.5
        assert np.array_equal(bits(ph.amg_apply(r)), bits(pd.amg_apply(r)))
    finally:
        ph.close()
        pd.close()


@pytest.mark.parametrize(
    "kind,E,N,faces,device_min_levels",
    [("box", (4, 3, 5), 7, "DNNDND", 3), ("box", (3, 3, 3), 3, "NDNNNN", 1), ("kershaw", (3, 3, 3), 7, "DNDDND", 1)],
    ids=["box435_N7_DNNDND", "box3_N3_NDNNNN_handoff_at_0", "kershaw3_N7_DNDDND"],
)
def test_device_hierarchy_is_the_host_hierarchy_with_natural_faces(own_stream, kind, E, N, faces, device_min_levels):
    """Face codes alone do not make the device build step aside (Subdomain::amg_build: only a shift, a kappa or a composite
    do): the end points of the lattice lines are dofs, the dof lattice has a plane more per natural face and the node order
    changes.  The same levels as the host build, as bits, the same number of device levels as the all-Dirichlet mesh of
    that size, the same bits from a V-cycle in double and in float"""
    make = (lambda f: make_box(E, N, faces=f)) if kind == "box" else (lambda f: make_kershaw(E, N, 0.3, faces=f))
    ph, pd = build_pair(lambda: make(faces), device_min_levels)
    try:
        twin = make("DDDDDD")
        try:
            twin.amg_build(device=True)
            twin_built, twin_rows = twin.amg_setup_info()["levels_built_on_device"], twin.amg_levels()[0]["A"].shape[0]
        finally:
            twin.close()
        built = pd.amg_setup_info()["levels_built_on_device"]
        print("%s %s N = %d %s: %d levels built on the device (%d on the all-Dirichlet mesh), %d rows (%d)" % (kind, E, N, faces, built, twin_built, pd.amg_levels()[0]["A"].shape[0], twin_rows))
        assert built == twin_built and pd.amg_levels()[0]["A"].shape[0] > twin_rows
        if N == 3:
            assert built == 1  # no lattice level: the device FEM matrix is handed over at level 0
        assert_same_hierarchy(ph, pd)
        r = S.seeded_uniform(ph.n, 5) - 0.5
        zh, zd = ph.amg_apply(r), pd.amg_apply(r)
        assert np.array_equal(bits(zh), bits(zd)) and np.abs(zh).max() > 0.0
        for p in (ph, pd):
            p.set_flag("amg_precision", 32)
        zh32, zd32 = ph.amg_apply(r), pd.amg_apply(r)
        assert np.array_equal(bits(zh32), bits(zd32)) and np.abs(zh32).max() > 0.0 and not np.array_equal(zh32, zh)
    finally:
        ph.close()
        pd.close()


def test_kershaw_hierarchy(own_stream):
    ph, pd = build_pair(lambda: make_kershaw((4, 4, 4), 7, 0.3), 1)
    try:
        assert np.diff(ph.amg_levels()[0]["A"].indptr).max() > 7  # deformed cells couple more than the 7-point neighbours
        assert_same_hierarchy(ph, pd)
    finally:
        ph.close()
        pd.close()


def test_curved_mesh_from_files(own_stream):
    with tempfile.TemporaryDirectory() as d:
        ph, pd = build_pair(lambda: make_curved(d), 1)
        try:
            assert np.diff(ph.amg_levels()[0]["A"].indptr).max() > 7
            assert_same_hierarchy(ph, pd)
        finally:
            ph.close()
            pd.close()


def test_float_vcycle_on_device_levels(own_stream):
    """amg_precision = 32: the f32 copies of the device-built levels come from HBM; the cycle gives the same bits."""
    ph, pd = build_pair(lambda: make_box((4, 3, 5), 7), 3)
    try:
        r = S.seeded_uniform(ph.n, 8) - 0.5
        for p in (ph, pd):
            p.set_flag("amg_precision", 32)
        zh, zd = ph.amg_apply(r), pd.amg_apply(r)
        assert np.array_equal(bits(zh), bits(zd))
        assert np.abs(zh).max() > 0.0
    finally:
        ph.close()
        pd.close()


@pytest.mark.parametrize("method", ["fcg", "gmres"])
def test_solver_histories_identical(own_stream, method):
    out = []
    for device in (False, True):
        p = make_box((4, 3, 5), 7)
        try:
            p.set_flag("sub_use_preconditioner", 1)
            p.set_flag("amg_device_setup", 1 if device else 0)  # the implicit build on first use follows the flag
            _, f = p.make_rhs_from(S.seeded_uniform(p.n, 21))
            u, its, hist = p.solve(f, method)
            out.append((its, hist, u, p.amg_setup_info()["levels_built_on_device"]))
        finally:
            p.close()
    (ih, hh, uh, dh), (idv, hd, ud, dd) = out
    assert dh == 0 and dd >= 3
    assert ih == idv
    assert np.array_equal(bits(hh), bits(hd))
    assert np.array_equal(bits(uh), bits(ud))


def test_composite_region_builds_on_the_host(own_stream):
    def make():
        p = H.Problem.box((3, 3, 3), (1, 1, 1), 7, 2, True, force_composite=True)
        for lvl in range(p.info["num_levels"]):
            p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
        return p

    ph, pd = make(), make()
    try:
        ph.amg_build(device=False)
        pd.amg_build(device=True)
        assert pd.amg_setup_info()["levels_built_on_device"] == 0
        assert_same_hierarchy(ph, pd)
    finally:
        ph.close()
        pd.close()


def test_full_size_c2_hierarchy(own_stream):
    """C2: 32^3 elements, N = 7.  The two builds' times are printed, not asserted."""
    ph, pd = build_pair(lambda: make_box((32, 32, 32), 7), 3)
    try:
        n = assert_same_hierarchy(ph, pd)
        print(f"C2 hierarchy ({n} levels): host setup {ph.amg_setup_info()['setup_seconds']:.3f} s, device setup {pd.amg_setup_info()['setup_seconds']:.3f} s "
              f"({pd.amg_setup_info()['levels_built_on_device']} levels on the device)")
    finally:
        ph.close()
        pd.close()
