"""GPU parity: every HIP kernel entry of libfdd_hip.so, called through the
C-ABI, against the CPU oracle on the same seeded inputs.

Bar (include/fdd_hip.h): element-wise kernels, thread-per-row and LDS-staged
SpMV, stiffness (two-launch and fused) and restriction keep the reference's
per-output operation order and must be BIT-IDENTICAL to the oracle
(both sides compiled with -ffp-contract=off).  Reductions use a different
summation tree: |gpu - oracle| <= 1e-13 * sum|terms| (a 1e-13 relative bound
on the conditioning-free scale; SURVEY.md section 8(d) asks 1e-11*sqrt(n/1e6)).
"""
import ctypes

import numpy as np
import pytest
import torch

import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k, reduce_workspace

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
P = S._p


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rnd(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


SIZES = [1, 2, 3, 127, 128, 129, 4097, 1000003]


# ------------------------------------------------------------------ math.okl
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", [0, 1])
def test_set_to_value(gpu, n, offset):
    L = S.oracle()
    ref = rnd(n + offset + 3, 1)
    u = dev(ref, gpu)
    L.orc_set_to_value(P(ref), ctypes.c_double(0.375), n, offset)
    k("fdd_set_to_value", u, 0.375, n, offset)
    assert np.array_equal(host(u), ref)


@pytest.mark.parametrize("n", SIZES)
def test_invert(gpu, n):
    L = S.oracle()
    ref = rnd(n, 2) + 2.0
    u = dev(ref, gpu)
    L.orc_invert_vector_elements(P(ref), n)
    k("fdd_invert_vector_elements", u, n)
    assert np.array_equal(host(u), ref)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alias", ["none", "u", "v"])
@pytest.mark.parametrize("shift", [0, 1])
def test_axpby(gpu, n, alias, shift):
    L = S.oracle()
    a, b = 1.25, -0.7
    u = rnd(n + shift, 3)[shift:]
    v = rnd(n + shift, 4)[shift:]
    du_full = dev(rnd(n + shift, 3), gpu)
    dv_full = dev(rnd(n + shift, 4), gpu)
    du, dv = du_full[shift:], dv_full[shift:]
    u = np.ascontiguousarray(u)
    v = np.ascontiguousarray(v)
    if alias == "none":
        out = np.zeros(n)
        dout_full = torch.zeros(n + shift, dtype=torch.float64, device=gpu)
        dout = dout_full[shift:]
    elif alias == "u":
        out, dout = u, du
    else:
        out, dout = v, dv
    L.orc_vector_vector_addition(P(out), ctypes.c_double(a), P(u), ctypes.c_double(b), P(v), n)
    k("fdd_vector_vector_addition", dout, a, du, b, dv, n)
    assert np.array_equal(host(dout), out)


@pytest.mark.parametrize("n", SIZES)
def test_scale(gpu, n):
    L = S.oracle()
    u = rnd(n, 5)
    out = np.zeros(n)
    L.orc_vector_scaling(P(out), ctypes.c_double(1.0 / 3.0), P(u), n)
    dout = torch.zeros(n, dtype=torch.float64, device=gpu)
    k("fdd_vector_scaling", dout, 1.0 / 3.0, dev(u, gpu), n)
    assert np.array_equal(host(dout), out)


def test_zero_length_is_noop(gpu):
    z = torch.zeros(4, dtype=torch.float64, device=gpu)
    k("fdd_set_to_value", z, 1.0, 0, 0)
    k("fdd_vector_scaling", z, 2.0, z, 0)
    k("fdd_csr_multiply", z, None, None, None, z, 0)
    assert host(z).sum() == 0.0


def test_invalid_argument_is_reported(gpu):
    z = torch.zeros(4, dtype=torch.float64, device=gpu)
    with pytest.raises(lib.FddError):
        k("fdd_vector_scaling", z, 2.0, z, -1)
    with pytest.raises(lib.FddError):
        k("fdd_csr_multiply_range", z, z, z, z, z, 3, 2)  # csr_matrix.tpp:322-326


# --------------------------------------------------- fused vector updates
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", ["dom", "sub"])
def test_vector_updates(gpu, n, family):
    L = S.oracle()
    u, r, p, q, z, f = (rnd(n, s) for s in range(10, 16))
    alpha, beta = 0.618, -1.7

    # initialize_arrays
    u0, r0 = u.copy(), r.copy()
    getattr(L, f"orc_{family}_initialize_arrays")(P(u0), P(r0), P(f), n)
    du, dr = dev(u, gpu), dev(r, gpu)
    k(f"fdd_{family}_initialize_arrays", du, dr, dev(f, gpu), n)
    assert np.array_equal(host(du), u0) and np.array_equal(host(dr), r0)

    # solution_and_residual_update
    u1, r1 = u.copy(), np.zeros(n)
    getattr(L, f"orc_{family}_solution_and_residual_update")(P(u1), P(r1), P(r), P(p), P(q), ctypes.c_double(alpha), n)
    du, dr1 = dev(u, gpu), torch.zeros(n, dtype=torch.float64, device=gpu)
    k(f"fdd_{family}_solution_and_residual_update", du, dr1, dev(r, gpu), dev(p, gpu), dev(q, gpu), alpha, n)
    assert np.array_equal(host(du), u1) and np.array_equal(host(dr1), r1)

    # residual_and_search_update
    p2, r2 = p.copy(), r.copy()
    getattr(L, f"orc_{family}_residual_and_search_update")(P(p2), P(r2), P(z), P(r1), ctypes.c_double(beta), n)
    dp, dr = dev(p, gpu), dev(r, gpu)
    k(f"fdd_{family}_residual_and_search_update", dp, dr, dev(z, gpu), dr1, beta, n)
    assert np.array_equal(host(dp), p2) and np.array_equal(host(dr), r2)


def test_vector_updates_device_scalars(gpu):
    """alpha = num/den read on the device: same bits as the host-side division."""
    L = S.oracle()
    n = 100003
    u, r, p, q, z = (rnd(n, s) for s in range(20, 25))
    num, den = 0.37, 1.9
    alpha = num / den
    u1, r1 = u.copy(), np.zeros(n)
    L.orc_dom_solution_and_residual_update(P(u1), P(r1), P(r), P(p), P(q), ctypes.c_double(alpha), n)
    sc = dev(np.array([num, den]), gpu)
    du, dr1 = dev(u, gpu), torch.zeros(n, dtype=torch.float64, device=gpu)
    k("fdd_dom_solution_and_residual_update_dev", du, dr1, dev(r, gpu), dev(p, gpu), dev(q, gpu), sc[0:], sc[1:], n)
    assert np.array_equal(host(du), u1) and np.array_equal(host(dr1), r1)
    p2, r2 = p.copy(), r.copy()
    L.orc_dom_residual_and_search_update(P(p2), P(r2), P(z), P(r1), ctypes.c_double(alpha), n)
    dp, dr = dev(p, gpu), dev(r, gpu)
    k("fdd_dom_residual_and_search_update_dev", dp, dr, dev(z, gpu), dr1, sc[0:], sc[1:], n)
    assert np.array_equal(host(dp), p2) and np.array_equal(host(dr), r2)


def test_cast_copies(gpu):
    L = S.oracle()
    n = 70001
    v = rnd(n, 30)
    out = np.zeros(n)
    L.orc_sub_copy_f64_f64(P(out), P(v), n)
    d = torch.zeros(n, dtype=torch.float64, device=gpu)
    k("fdd_sub_copy_f64_f64", d, dev(v, gpu), n)
    assert np.array_equal(host(d), out)

    out32 = np.zeros(n, np.float32)
    L.orc_sub_copy_f32_f64(P(out32), P(v), n)
    d32 = torch.zeros(n, dtype=torch.float32, device=gpu)
    k("fdd_sub_copy_f32_f64", d32, dev(v, gpu), n)
    assert np.array_equal(host(d32), out32)

    back = np.zeros(n)
    L.orc_sub_copy_f64_f32(P(back), P(out32), n)
    k("fdd_sub_copy_f64_f32", d, d32, n)
    assert np.array_equal(host(d), back)


# ------------------------------------------------------------ reductions
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 4097, 1000003, 5000001])
def test_reductions(gpu, n):
    L = S.oracle()
    nb = (n + 127) // 128
    ws = reduce_workspace(gpu)
    out = torch.zeros(2, dtype=torch.float64, device=gpu)
    a, b, c, d, w = (rnd(n, s) for s in range(40, 45))
    w = np.abs(w)
    block = np.zeros(2 * nb)

    def check(got, ref, scale):
        assert abs(got - ref) <= 1e-13 * scale + 1e-300, (got, ref, scale)

    # domain.okl:109-138 and :235-264
    L.orc_dom_residual_norm(P(block), P(a), P(b), P(w), n, nb)
    ref = L.orc_block_sum(P(block), nb)
    k("fdd_dom_residual_norm", out, ws, dev(a, gpu), dev(b, gpu), dev(w, gpu), n)
    check(host(out)[0], ref, np.abs(a * b * w).sum())
    k("fdd_dom_inner_product", out, ws, dev(a, gpu), dev(b, gpu), dev(w, gpu), n)
    L.orc_dom_inner_product(P(block), P(a), P(b), P(w), n, nb)
    check(host(out)[0], L.orc_block_sum(P(block), nb), np.abs(a * b * w).sum())

    # domain.okl:140-184
    L.orc_dom_projection_inner_products(P(block), P(a), P(b), P(c), P(d), n, nb)
    g = L.orc_block_sum(P(block), nb)
    t = L.orc_block_sum(P(block[nb:]), nb)
    k("fdd_dom_projection_inner_products", out, ws, dev(a, gpu), dev(b, gpu), dev(c, gpu), dev(d, gpu), n)
    o = host(out)
    check(o[0], g, np.abs(a * b).sum())
    check(o[1], t, np.abs(c * d).sum())

    # domain.okl:195-224
    L.orc_dom_inner_product_flexible(P(block), P(a), P(b), P(c), n, nb)
    k("fdd_dom_inner_product_flexible", out, ws, dev(a, gpu), dev(b, gpu), dev(c, gpu), n)
    check(host(out)[0], L.orc_block_sum(P(block), nb), np.abs((b - a) * c).sum())

    # subdomain.okl:103-258
    L.orc_sub_inner_product(P(block), P(a), P(b), n, nb)
    k("fdd_sub_inner_product", out, ws, dev(a, gpu), dev(b, gpu), n)
    check(host(out)[0], L.orc_block_sum(P(block), nb), np.abs(a * b).sum())
    k("fdd_amg_dot", out, ws, dev(a, gpu), dev(b, gpu), n)
    check(host(out)[0], L.orc_block_sum(P(block), nb), np.abs(a * b).sum())

    L.orc_sub_weighted_inner_product(P(block), P(a), P(b), P(w), n, nb)
    k("fdd_sub_weighted_inner_product", out, ws, dev(a, gpu), dev(b, gpu), dev(w, gpu), n)
    check(host(out)[0], L.orc_block_sum(P(block), nb), np.abs(a * b * w).sum())

    L.orc_sub_projection_inner_products(P(block), P(a), P(b), P(c), P(d), P(w), n, nb)
    k("fdd_sub_projection_inner_products", out, ws, dev(a, gpu), dev(b, gpu), dev(c, gpu), dev(d, gpu), dev(w, gpu), n)
    o = host(out)
    check(o[0], L.orc_block_sum(P(block), nb), np.abs(a * b * w).sum())
    check(o[1], L.orc_block_sum(P(block[nb:]), nb), np.abs(c * d * w).sum())

    L.orc_sub_search_update_inner_product(P(block), P(a), P(b), P(c), P(w), n, nb)
    k("fdd_sub_search_update_inner_product", out, ws, dev(a, gpu), dev(b, gpu), dev(c, gpu), dev(w, gpu), n)
    check(host(out)[0], L.orc_block_sum(P(block), nb), np.abs((b - a) * c * w).sum())


def test_reduction_is_deterministic_and_empty_is_zero(gpu):
    n = 3000001
    ws = reduce_workspace(gpu)
    a, b = dev(rnd(n, 50), gpu), dev(rnd(n, 51), gpu)
    o1 = torch.zeros(1, dtype=torch.float64, device=gpu)
    o2 = torch.ones(1, dtype=torch.float64, device=gpu)
    k("fdd_sub_inner_product", o1, ws, a, b, n)
    k("fdd_sub_inner_product", o2, ws, a, b, n)
    assert host(o1)[0] == host(o2)[0]
    k("fdd_sub_inner_product", o2, ws, a, b, 0)
    assert host(o2)[0] == 0.0


# ----------------------------------------------------------------- CSR
def csr_random(rows, cols, row_lens, seed):
    rng = np.random.default_rng(seed)
    ptr = np.zeros(rows + 1, np.int32)
    ptr[1:] = np.cumsum(row_lens)
    nnz = int(ptr[-1])
    col = np.zeros(nnz, np.int32)
    for i in range(rows):
        L = row_lens[i]
        if L:
            col[ptr[i]:ptr[i + 1]] = np.sort(rng.choice(cols, size=L, replace=(L > cols)))
    val = rng.uniform(-1, 1, nnz)
    return ptr, col, val


def stencil27(m):
    """27-point stencil CSR on an m^3 node grid (stand-in for A_fem[0] / the
    superdomain operator)."""
    idx = np.arange(m**3).reshape(m, m, m)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                z0, z1 = max(0, -dz), m - max(0, dz)
                y0, y1 = max(0, -dy), m - max(0, dy)
                x0, x1 = max(0, -dx), m - max(0, dx)
                r = idx[z0:z1, y0:y1, x0:x1].reshape(-1)
                c = idx[z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx].reshape(-1)
                rows.append(r)
                cols.append(c)
    rows = np.concatenate(rows)
    cols = np.concatenate(cols)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    ptr = np.zeros(m**3 + 1, np.int32)
    np.add.at(ptr, rows + 1, 1)
    ptr = np.cumsum(ptr).astype(np.int32)
    val = np.random.default_rng(7).uniform(-1, 1, len(cols))
    return ptr, cols.astype(np.int32), val


def run_csr_case(gpu, ptr, col, val, ncols, expect_kind=None, exact=True):
    L = S.oracle()
    rows = len(ptr) - 1
    u = rnd(ncols, 60)
    w = rnd(rows, 61)
    dptr, dcol, dval, du, dw = dev(ptr, gpu), dev(col, gpu), dev(val, gpu), dev(u, gpu), dev(w, gpu)

    ref = np.zeros(rows)
    L.orc_csr_multiply(P(ref), P(ptr), P(col), P(val), P(u), rows)
    refw = np.zeros(rows)
    L.orc_csr_multiply_weight(P(refw), P(ptr), P(col), P(val), P(u), P(w), rows)

    def same(got, want):
        if exact:
            assert np.array_equal(got, want)
        else:
            scale = np.abs(want).max() + 1e-300
            assert np.abs(got - want).max() <= 1e-13 * max(scale, 1.0) * 64

    out = torch.full((rows,), 7.0, dtype=torch.float64, device=gpu)
    k("fdd_csr_multiply", out, dptr, dcol, dval, du, rows)
    same(host(out), ref)
    k("fdd_csr_multiply_weight", out, dptr, dcol, dval, du, dw, rows)
    same(host(out), refw)

    # inclusive row range (csr_matrix.okl:20-33)
    if rows >= 5:
        r0, r1 = rows // 3, rows - 2
        out.fill_(7.0)
        k("fdd_csr_multiply_range", out, dptr, dcol, dval, du, r0, r1)
        want = np.full(rows, 7.0)
        L.orc_csr_multiply_range(P(want), P(ptr), P(col), P(val), P(u), r0, r1)
        same(host(out), want)

    # planned SpMV
    plan = vp()
    lib.hip().call("fdd_csr_plan_create", ctypes.byref(plan), P(ptr), rows, ncols, int(ptr[-1]))
    try:
        kind = ctypes.c_int(-1)
        lib.hip().call("fdd_csr_plan_kind", plan, ctypes.byref(kind))
        if expect_kind is not None:
            assert kind.value == expect_kind
        out.fill_(7.0)
        k("fdd_csr_plan_multiply", plan, out, dptr, dcol, dval, du, None)
        same(host(out), ref)
        k("fdd_csr_plan_multiply", plan, out, dptr, dcol, dval, du, dw)
        same(host(out), refw)
        if len(val) and not np.all(val == 1.0) and expect_kind == 1:
            # short even rows: the sliced-ELL copy of the matrix (one lane per row, column-major slices of 64 rows)
            attached = ctypes.c_int(0)
            k("fdd_csr_plan_attach_sell", plan, P(ptr), dptr, dcol, dval, ctypes.c_double(1.5), ctypes.byref(attached))
            widths = np.diff(ptr)
            padded = sum(int(widths[i:i + 64].max()) * 64 for i in range(0, rows, 64))
            assert attached.value == int(padded <= 1.5 * len(val) and len(val) <= 16 * rows)  # one lane per row pays up to 16 entries per row (27-entry rows measured faster on the row-block kernel)
            if attached.value:
                slices, compact = ctypes.c_int(-1), ctypes.c_int(-1)
                lib.hip().call("fdd_csr_plan_sell_info", plan, ctypes.byref(slices), ctypes.byref(compact))
                assert slices.value > 0
                # fdd_csr_plan_multiply does not look at the sliced-ELL copy: attaching one leaves that entry on the
                # row-block kernel, with the same bits as before.  Of the calls below only fdd_csr_plan_matvec runs
                # sell_kernel (every entry that does, bit for bit: test_gpu_sell_entries.py)
                out.fill_(7.0)
                k("fdd_csr_plan_multiply", plan, out, dptr, dcol, dval, du, None)
                same(host(out), ref)
                k("fdd_csr_plan_multiply", plan, out, dptr, dcol, dval, du, dw)
                same(host(out), refw)
                yy = rnd(rows, 63)
                dyy = dev(yy, gpu)
                L.orc_amg_matvec(P(yy), P(ptr), P(col), P(val), P(u), ctypes.c_double(-1.0), ctypes.c_double(0.5), rows)
                k("fdd_csr_plan_matvec", plan, dyy, dptr, dcol, dval, du, -1.0, 0.5)
                same(host(dyy), yy)
        if len(val) and np.all(val == 1.0):
            # boolean matrix: the plan may skip the val array, same bits
            lib.hip().call("fdd_csr_plan_set_unit_values", plan, 1)
            out.fill_(7.0)
            k("fdd_csr_plan_multiply", plan, out, dptr, dcol, None, du, None)
            same(host(out), ref)
            k("fdd_csr_plan_multiply", plan, out, dptr, dcol, None, du, dw)
            same(host(out), refw)
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)

    # y = alpha*A*x + beta*y (AMG/csr_matrix.cpp:112-134)
    y = rnd(rows, 62)
    dy = dev(y, gpu)
    L.orc_amg_matvec(P(y), P(ptr), P(col), P(val), P(u), ctypes.c_double(-1.0), ctypes.c_double(1.0), rows)
    k("fdd_amg_matvec", dy, dptr, dcol, dval, du, -1.0, 1.0, rows)
    same(host(dy), y)


def test_csr_boolean_gather_scatter(gpu):
    """Q and Qt of a box-mesh Domain (domain.tpp:287-294): 1 and 1..8 nnz/row."""
    m = S.BoxMesh((6, 6, 6), 5)
    W = S.OracleWorld([m], 5)
    try:
        ptr, col, val = W.Q(0)
        run_csr_case(gpu, ptr, col, val, W.num_nodes(0), expect_kind=0)
        ptr, col, val = W.Qt(0)
        assert np.diff(ptr).max() == 8
        run_csr_case(gpu, ptr, col, val, m.num_local_points, expect_kind=1)  # ragged rows: LDS row staging
    finally:
        W.close()


def test_csr_stencil27_lds_staged(gpu):
    ptr, col, val = stencil27(41)
    run_csr_case(gpu, ptr, col, val, 41**3, expect_kind=1)


def test_csr_ragged_rows(gpu):
    """Empty rows, rows of every length up to a block, and rows longer than a
    block (workgroup-reduced: tolerance instead of bit equality)."""
    rng = np.random.default_rng(9)
    rows = 3000
    lens = rng.integers(0, 40, rows)
    lens[rng.integers(0, rows, 200)] = 0
    lens[5] = 2048
    lens[6] = 2047
    lens[700] = 1
    ptr, col, val = csr_random(rows, 5000, lens, 10)
    run_csr_case(gpu, ptr, col, val, 5000, expect_kind=1)

    lens2 = lens.copy()
    lens2[17] = 2049
    lens2[18] = 10000
    lens2[rows - 1] = 4100
    ptr, col, val = csr_random(rows, 5000, lens2, 11)
    run_csr_case(gpu, ptr, col, val, 5000, expect_kind=1, exact=False)


def test_csr_runs_of_empty_rows(gpu):
    """Leading, inner and trailing runs of empty rows longer than a row block (a block whose rows hold no entry at
    all: its first-entry index may sit one past the end of col / val), next to rows wide enough that the LDS-staged
    kernel is chosen -- the shape of the composite region's non-conforming Q (Dirichlet points have no entry, hanging
    points have (N_j + 1)^2 of them)."""
    rng = np.random.default_rng(12)
    rows = 9000
    lens = rng.integers(0, 3, rows)
    lens[:2600] = 0       # leading
    lens[4000:6700] = 0   # inner
    lens[-2300:] = 0      # trailing: base == nnz for these blocks
    lens[3000:3040] = 36
    ptr, col, val = csr_random(rows, 4000, lens, 13)
    assert ptr[-1] > rows // 8
    run_csr_case(gpu, ptr, col, val, 4000)
    lens[3000:3400] = 64  # more entries than rows: row-block kernel for sure
    ptr, col, val = csr_random(rows, 4000, lens, 14)
    run_csr_case(gpu, ptr, col, val, 4000, expect_kind=1)
    # boolean variant (unit values, dssum-style gather plans)
    lens = np.zeros(rows, np.int64)
    lens[2500:5000] = rng.integers(1, 9, 2500)
    ptr, col, _ = csr_random(rows, 4000, lens, 15)
    run_csr_case(gpu, ptr, col, np.ones(len(col)), 4000, expect_kind=1)


def test_sell_with_a_few_wide_slices(gpu):
    """Short even rows and, at the end, two hundred rows of 150-400 entries (the interface and superdomain rows of a
    composite's low-order operator): the sliced-ELL copy is still attached, its wide slices are visited first, and
    the row sums keep the column order (same bits as the row-block kernel)."""
    rows, ncols = 20000, 20000
    lens = np.full(rows, 7, np.int64)
    lens[5000:5064] = 3
    lens[-200:] = np.random.default_rng(3).integers(150, 400, 200)
    ptr, col, val = csr_random(rows, ncols, lens, 21)
    run_csr_case(gpu, ptr, col, val, ncols, expect_kind=1)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("shape", ["lattice", "lattice15", "far_columns", "mixed"])
def test_sell_compact_columns(gpu, shape, precision):
    """The sliced-ELL copy's compact column form (a wave-uniform base per slot + a 16-bit offset per row) where a slice's
    slots allow it, 32-bit columns in the other slices of the same matrix: the bits of the 32-bit form
    (FDD_TUNE_CSR_SELL_COL16=0), the row-block kernel's values to rounding, in double and in single precision; row
    lengths 7 / 15 / 1-9 exercise every tail (0-3 entries after the groups of four), the ragged last slice and empty rows."""
    import os

    import scipy.sparse as sp

    rng = np.random.default_rng(230)
    if shape in ("lattice", "lattice15"):
        m = 47  # 103 823 rows: columns of a slice spread over 2*47*47 + 64 << 65536, but the matrix has more than 65536 columns
        T = sp.diags([1.0, -2.0, 1.0], [-1, 0, 1], shape=(m, m))
        I = sp.eye(m)
        A = sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(I, sp.kron(I, T))
        if shape == "lattice15":
            A = A + 0.25 * sp.kron(sp.kron(T, T), I) + 0.125 * sp.kron(I, sp.kron(T, T))
        A = A.tocsr()
        A.sort_indices()
        ptr, col = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        rows = cols = A.shape[0]
        expect = "all"
    else:
        rows, cols = 40000 + 37, 400000
        lens = rng.integers(1, 10, rows)
        lens[777] = 0
        lens[64 * 100 : 64 * 101] = 0  # a slice of empty rows
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        near = ((np.repeat(np.arange(rows, dtype=np.int64), lens) * cols) // rows + rng.integers(0, 30000, int(ptr[-1]))).clip(0, cols - 1)
        far = rng.integers(0, cols, int(ptr[-1]))
        if shape == "far_columns":
            pick, expect = far, "few"
        else:
            pick, expect = np.where(np.repeat(np.arange(rows) % 2048 < 1024, lens), near, far), "some"
        col = np.concatenate([np.sort(pick[ptr[r] : ptr[r + 1]]) for r in range(rows)]).astype(np.int32)
    nnz = int(ptr[-1])
    ft = np.float64 if precision == 64 else np.float32
    tt = torch.float64 if precision == 64 else torch.float32
    val = rng.uniform(-1, 1, nnz).astype(ft)
    x, y0 = rng.uniform(-1, 1, cols).astype(ft), rng.uniform(-1, 1, rows).astype(ft)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    dp, dc, dv, dx = t(ptr), t(col), t(val), t(x)
    create = "fdd_csr_plan_create" if precision == 64 else "fdd_csr_plan_create_f32"

    def run(plan, alpha, beta):
        y = t(y0) if (beta != 0.0 and precision == 64) else torch.full((rows,), float("nan"), dtype=tt, device=gpu)
        if precision == 64:
            k("fdd_csr_plan_matvec", plan, y, dp, dc, dv, dx, alpha, beta)
        else:
            k("fdd_csr_plan_matvec_to_f32", plan, y, t(y0) if beta != 0.0 else None, dp, dc, dv, dx, alpha, beta)
        return host(y)

    plans, results = {}, {}
    try:
        for form in ("blocks", "col32", "col16"):
            plans[form] = vp()
            lib.hip().call(create, ctypes.byref(plans[form]), vp(ptr.ctypes.data), rows, cols, nnz)
            if form != "blocks":
                os.environ["FDD_TUNE_CSR_SELL_COL16"] = "0" if form == "col32" else "1"
                attached = ctypes.c_int(0)
                k("fdd_csr_plan_attach_sell", plans[form], vp(ptr.ctypes.data), dp, dc, dv, ctypes.c_double(2.5), ctypes.byref(attached))
                assert attached.value == 1, form
                slices, compact = ctypes.c_int(-1), ctypes.c_int(-1)
                lib.hip().call("fdd_csr_plan_sell_info", plans[form], ctypes.byref(slices), ctypes.byref(compact))
                assert slices.value == (rows + 63) // 64
                if form == "col32":
                    assert compact.value == 0
                elif expect == "all":
                    assert compact.value == slices.value
                elif expect == "some":
                    assert slices.value // 3 < compact.value < slices.value
                else:
                    assert compact.value < slices.value // 10
            results[form] = [run(plans[form], a, b) for a, b in ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0))]
        for got, want, blocks in zip(results["col16"], results["col32"], results["blocks"]):
            assert np.isfinite(got).all() and np.array_equal(got, want), (shape, precision)
            # the row-block kernel adds a wide row's products with several lanes (the entry stands in for cusparseSpMV,
            # whose order is undefined): same values to rounding
            assert np.allclose(want, blocks, rtol=1e-12 if precision == 64 else 1e-4, atol=1e-13 if precision == 64 else 1e-5), (shape, precision)
    finally:
        os.environ.pop("FDD_TUNE_CSR_SELL_COL16", None)
        for plan in plans.values():
            lib.hip().call("fdd_csr_plan_destroy", plan)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n,keep,E", [(8, (0, 3, 4, 7), 37), (8, (0, 2, 5, 7), 1), (16, (0, 2, 4, 7, 8, 11, 13, 15), 9), (16, (0, 15), 5), (8, (0, 1, 2, 3, 7), 6)])
def test_lattice_transfer_equals_the_csr_interpolator(gpu, n, keep, E, precision):
    """fdd_lattice_prolong / fdd_lattice_restrict (the matrix-free interpolator of a geometric AMG level, host/low_order.hpp
    geometric_level) against the same operator as a scipy CSR matrix built entry by entry from the weight table: random
    ownership (later occurrences and Dirichlet points own nothing), coarse nodes shared between elements or without a
    dof; uneven and minimal kept sets, a single element, a workgroup's ragged last elements."""
    import scipy.sparse as sp

    rng = np.random.default_rng(300 + n + E)
    m = len(keep)
    ref = np.sort(np.concatenate([[-1.0, 1.0], rng.uniform(-0.95, 0.95, n - 2)]))
    pos = {k: a for a, k in enumerate(keep)}
    lo, hi, wl = np.zeros(n, np.int32), np.zeros(n, np.int32), np.ones(n)
    a = 0
    for i in range(n):
        if i in pos:
            lo[i] = hi[i] = a = pos[i]
            continue
        lo[i], hi[i] = a, a + 1
        wl[i] = (ref[keep[a + 1]] - ref[i]) / (ref[keep[a + 1]] - ref[keep[a]])
    np3, mc = n**3, m**3
    owns = rng.uniform(size=E * np3) < 0.8
    nfine = int(owns.sum())
    owner = np.full(E * np3, -1, np.int32)
    owner[owns] = rng.permutation(nfine).astype(np.int32)
    nc = max(E * mc // 2, 3)
    coarse = rng.integers(0, nc, E * mc).astype(np.int32)
    coarse[rng.uniform(size=E * mc) < 0.1] = -1
    # the operator entry by entry: owned point (e, i, j, k) -> the kept nodes around it
    pts = np.nonzero(owns)[0]
    e, v = pts // np3, pts % np3
    ii, jj, kk = v % n, (v // n) % n, v // (n * n)
    rows, kept_node, wts = [], [], []
    for corner in range(8):
        sx, sy, sz = corner & 1, (corner >> 1) & 1, corner >> 2
        ok = ~((sx & (lo[ii] == hi[ii])) | (sy & (lo[jj] == hi[jj])) | (sz & (lo[kk] == hi[kk]))).astype(bool)
        ca, cb, cc = np.where(sx, hi[ii], lo[ii]), np.where(sy, hi[jj], lo[jj]), np.where(sz, hi[kk], lo[kk])
        w = np.where(sx, 1 - wl[ii], wl[ii]) * np.where(sy, 1 - wl[jj], wl[jj]) * np.where(sz, 1 - wl[kk], wl[kk])
        rows.append(owner[pts][ok])
        kept_node.append((e * mc + (cc * m + cb) * m + ca)[ok])
        wts.append(w[ok])
    rows, kept_node, wts = np.concatenate(rows), np.concatenate(kept_node), np.concatenate(wts)
    S_el = sp.csr_matrix((wts, (kept_node, rows)), shape=(E * mc, nfine))  # element-local restriction
    has = coarse[kept_node] >= 0
    P = sp.csr_matrix((wts[has], (rows[has], coarse[kept_node][has])), shape=(nfine, nc))
    assert np.allclose(np.asarray(S_el.sum(axis=0)).ravel(), 1.0)  # a partition of unity: the weights of a fine point add up to 1
    ft, tt = (np.float64, torch.float64) if precision == 64 else (np.float32, torch.float32)
    tol = 1e-13 if precision == 64 else 2e-6
    u0, ec, fine = (rng.uniform(-1, 1, sz).astype(ft) for sz in (nfine, nc, nfine))
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(gpu)
    suffix = "" if precision == 64 else "_f32"
    vpi = lambda arr: vp(arr.ctypes.data)
    supported = ctypes.c_int(0)
    lib.hip().call("fdd_lattice_supported", n, m, ctypes.byref(supported))
    assert supported.value == 1
    du = t(u0)
    k("fdd_lattice_prolong" + suffix, du, t(ec), t(owner), t(coarse), n, m, vpi(lo), vpi(hi), vpi(wl), ctypes.c_longlong(E))
    want = u0.astype(np.float64) + P @ ec.astype(np.float64)
    assert np.abs(host(du) - want).max() <= tol * max(np.abs(want).max(), 1.0)
    partial = torch.full((E * mc,), float("nan"), dtype=tt, device=gpu)
    k("fdd_lattice_restrict" + suffix, partial, t(fine), t(owner), n, m, vpi(lo), vpi(hi), vpi(wl), ctypes.c_longlong(E))
    want = S_el @ fine.astype(np.float64)
    assert np.abs(host(partial) - want).max() <= tol * max(np.abs(want).max(), 1.0) * n
    # zero elements: nothing is launched; an unsupported lattice is refused
    k("fdd_lattice_prolong" + suffix, du, t(ec), t(owner), t(coarse), n, m, vpi(lo), vpi(hi), vpi(wl), ctypes.c_longlong(0))
    lib.hip().call("fdd_lattice_supported", 6, 3, ctypes.byref(supported))
    assert supported.value == 0
    with pytest.raises(lib.FddError):
        k("fdd_lattice_prolong" + suffix, du, t(ec), t(owner), t(coarse), 6, 3, vpi(lo), vpi(hi), vpi(wl), ctypes.c_longlong(1))


@pytest.mark.parametrize("suffix", ["", "_f32"])
def test_lattice_transfer_refuses_bad_sizes_before_any_launch(gpu, suffix):
    """fdd_lattice_prolong / fdd_lattice_restrict and their _f32 forms check the lattice (n, m: exactly what
    fdd_lattice_supported accepts) and then the element count, before n divides anything and before any launch: n = 0 was a
    host integer division by zero.  Every refused call raises and leaves the output buffer, pre-filled with a sentinel, alone."""
    tt = torch.float64 if suffix == "" else torch.float32
    sentinel = -12345.5
    vpi = lambda arr: vp(arr.ctypes.data)
    lo, hi, wl = np.zeros(17, np.int32), np.zeros(17, np.int32), np.ones(17)
    size = 2 * 17**3
    src = torch.zeros(size, dtype=tt, device=gpu)
    owner = torch.full((size,), -1, dtype=torch.int32, device=gpu)
    coarse = torch.full((size,), -1, dtype=torch.int32, device=gpu)
    cases = [(n, 2, 1) for n in (0, -1, 1, 7, 9, 17)]                                  # lattices that are not built
    cases += [(n, m, 1) for n in (0, -1, 1, 7, 9, 17, 8, 16) for m in (0, n + 1)]      # kept counts out of range
    cases += [(8, 6, 1), (16, 10, 1)]                                                  # one more than n / 2 + 1
    cases += [(n, 2, E) for n in (8, 16) for E in (-1, -(2**40), 2**31 // n**3, 2**31, 2**40)]  # E < 0 and E at and past the 2^31 bound
    for n, m, E in cases:
        supported = ctypes.c_int(-1)
        lib.hip().call("fdd_lattice_supported", n, m, ctypes.byref(supported))
        assert supported.value == (1 if (n in (8, 16) and 2 <= m <= n // 2 + 1) else 0), (n, m)
        if E == 1:
            assert supported.value == 0, (n, m)
        for name, args in (("fdd_lattice_prolong", (src, owner, coarse)), ("fdd_lattice_restrict", (src, owner))):
            out = torch.full((size,), sentinel, dtype=tt, device=gpu)
            with pytest.raises(lib.FddError):
                k(name + suffix, out, *args, n, m, vpi(lo), vpi(hi), vpi(wl), ctypes.c_longlong(E))
            torch.cuda.synchronize()
            assert bool((out == sentinel).all()), (name, n, m, E)
    # accepted sizes with no element launch nothing and succeed
    for n in (8, 16):
        out = torch.full((size,), sentinel, dtype=tt, device=gpu)
        k("fdd_lattice_prolong" + suffix, out, src, owner, coarse, n, 2, vpi(lo), vpi(hi), vpi(wl), ctypes.c_longlong(0))
        k("fdd_lattice_restrict" + suffix, out, src, owner, n, 2, vpi(lo), vpi(hi), vpi(wl), ctypes.c_longlong(0))
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())


def test_csr_empty_matrix(gpu):
    ptr = np.zeros(11, np.int32)
    run_csr_case(gpu, ptr, np.zeros(0, np.int32), np.zeros(0), 7, expect_kind=0)


# ------------------------------------------------------------ stiffness
def stiffness_inputs(E, N, seed, dim=3):
    n = N + 1
    npts = E * n**dim
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1, 1, npts)
    G = [rng.uniform(0.1, 1.0, npts) if g < dim else rng.uniform(-0.3, 0.3, npts) for g in range(6)]
    _, _, D = S.gll(N)
    return u, G, np.ascontiguousarray(D)


def oracle_stiffness(u, G, D, N, dim):
    L = S.oracle()
    npts = len(u)
    GDu = [np.zeros(npts) for _ in range(3)]
    Au = np.zeros(npts)
    gd = (vp * 3)(*[a.ctypes.data for a in GDu])
    gg = (vp * 6)(*[a.ctypes.data for a in G])
    L.orc_dom_stiffness_matrix_1(gd, P(u), P(D), gg, npts, N, dim)
    L.orc_dom_stiffness_matrix_2(P(Au), gd, P(D), npts, N, dim)
    return Au, GDu


@pytest.mark.parametrize("N", [1, 2, 3, 5, 7, 15])
@pytest.mark.parametrize("dim", [2, 3])
def test_stiffness_two_launch_form(gpu, N, dim):
    E = 37 if dim == 3 else 101
    u, G, D = stiffness_inputs(E, N, 70 + N, dim)
    Au, GDu = oracle_stiffness(u, G, D, N, dim)
    npts = len(u)
    dG = [dev(g, gpu) for g in G]
    dGDu = [torch.zeros(npts, dtype=torch.float64, device=gpu) for _ in range(3)]
    dAu = torch.zeros(npts, dtype=torch.float64, device=gpu)
    k("fdd_dom_stiffness_matrix_1", dGDu, dev(u, gpu), dev(D, gpu), dG, npts, N, dim)
    k("fdd_dom_stiffness_matrix_2", dAu, dGDu, dev(D, gpu), npts, N, dim)
    for d in range(dim):
        assert np.array_equal(host(dGDu[d]), GDu[d])
    assert np.array_equal(host(dAu), Au)


@pytest.mark.parametrize("N", list(range(1, 16)))
def test_stiffness_fused_bit_exact(gpu, N):
    """Fused D^T G D u == oracle two-kernel arithmetic, bit for bit, with all
    six geometric factors non-zero; element counts that do not fill the last
    workgroup."""
    for E in (1, 7, 130):
        u, G, D = stiffness_inputs(E, N, 90 + N)
        Au, _ = oracle_stiffness(u, G, D, N, 3)
        dAu = torch.full((len(u),), 3.0, dtype=torch.float64, device=gpu)
        k("fdd_dom_stiffness_matrix", dAu, dev(u, gpu), dev(D, gpu), [dev(g, gpu) for g in G], E, N)
        assert np.array_equal(host(dAu), Au), (N, E)


@pytest.mark.parametrize("N", list(range(1, 16)))
def test_stiffness_fused_two_dimensional_bit_exact(gpu, N):
    """The fused 2-D kernel (domain.okl's DIM == 2 branches in one launch) == the oracle's two-kernel arithmetic,
    bit for bit; element counts that do not fill the last workgroup, an offset list in reverse order, in place."""
    n2 = (N + 1) ** 2
    # the last size makes every workgroup walk 8 groups of elements (launch_fused_2d), the last one ragged
    walking = [(256 // n2) * (8 * 4096 + 3) + 1] if N in (1, 3, 7, 10, 15) else []
    for E in [1, 9, 1030] + walking:
        u, G, D = stiffness_inputs(E, N, 490 + N, 2)
        Au, _ = oracle_stiffness(u, G, D, N, 2)
        dG = [dev(g, gpu) for g in G]
        dAu = torch.full((len(u),), 3.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_matrix_2d", dAu, dev(u, gpu), dev(D, gpu), dG, None, E, N)
        assert np.array_equal(host(dAu), Au), (N, E)
        eo = (np.arange(E)[::-1] * n2).astype(np.int32)
        du = dev(u, gpu)
        k("fdd_stiffness_matrix_2d", du, du, dev(D, gpu), dG, dev(eo, gpu), E, N)
        assert np.array_equal(host(du), Au), (N, E)
    with pytest.raises(lib.FddError):
        k("fdd_stiffness_matrix_2d", dAu, dev(u, gpu), dev(D, gpu), dG, None, 1, 16)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 6, 7, 9, 15])
def test_stiffness_fused_gather_on_load(gpu, N):
    """fdd_sub_stiffness_matrix_gather: u[p] = v[point_dof[p]] (0 where the point
    has no dof) fused into the load == scatter on the host, then the oracle's
    two-kernel arithmetic, bit for bit; contiguous and offset-list element order."""
    n3 = (N + 1) ** 3
    for E in (1, 6, 41):
        _, G, D = stiffness_inputs(E, N, 190 + N)
        rng = np.random.default_rng(300 + N + E)
        ndof = max(1, (E * n3) // 3)
        pd = rng.integers(-1, ndof, E * n3).astype(np.int32)
        v = rng.uniform(-1, 1, ndof)
        u = np.where(pd >= 0, v[np.maximum(pd, 0)], 0.0)
        Au, _ = oracle_stiffness(u, G, D, N, 3)
        dG = [dev(g, gpu) for g in G]
        dAu = torch.full((E * n3,), 3.0, dtype=torch.float64, device=gpu)
        k("fdd_sub_stiffness_matrix_gather", dAu, dev(v, gpu), dev(pd, gpu), dev(D, gpu), dG, None, E, N)
        assert np.array_equal(host(dAu), Au), (N, E)
        # the same elements visited through an offset list in reverse order
        eo = (np.arange(E)[::-1] * n3).astype(np.int32)
        dAu2 = torch.full((E * n3,), 5.0, dtype=torch.float64, device=gpu)
        k("fdd_sub_stiffness_matrix_gather", dAu2, dev(v, gpu), dev(pd, gpu), dev(D, gpu), dG, dev(eo, gpu), E, N)
        assert np.array_equal(host(dAu2), Au), (N, E)


@pytest.mark.parametrize("N", [8, 9, 11, 12, 14, 15])
def test_stiffness_mfma(gpu, N):
    """fp64-MFMA path (config C3, N = 15; lower degrees zero-padded to 16): MFMA
    fuses multiply-add and sums in its own order, so the bar is a tolerance,
    1e-12 * max|Au| (observed ~1e-15), against the oracle AND against the
    bit-exact fused kernel; element lists with offsets and counts that do not
    divide the grid."""
    for E in (1, 5, 300):
        u, G, D = stiffness_inputs(E, N, 200 + N)
        Au, _ = oracle_stiffness(u, G, D, N, 3)
        du, dD, dG = dev(u, gpu), dev(D, gpu), [dev(g, gpu) for g in G]
        out = torch.full((len(u),), 3.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_matrix_mfma", out, du, dD, dG, None, E, N)
        got = host(out)
        assert np.abs(got - Au).max() <= 1e-12 * np.abs(Au).max(), (N, E, np.abs(got - Au).max() / np.abs(Au).max())
    # element offsets: every other element of a larger vector
    n3 = (N + 1) ** 3
    E = 40
    u, G, D = stiffness_inputs(2 * E, N, 300 + N)
    eo = (np.arange(E) * 2 * n3).astype(np.int32)
    ref = torch.full((len(u),), 7.0, dtype=torch.float64, device=gpu)
    out = torch.full((len(u),), 7.0, dtype=torch.float64, device=gpu)
    du, dD, dG, deo = dev(u, gpu), dev(D, gpu), [dev(g, gpu) for g in G], dev(eo, gpu)
    k("fdd_sub_stiffness_matrix", ref, du, dD, dG, deo, E, N)
    k("fdd_stiffness_matrix_mfma", out, du, dD, dG, deo, E, N)
    r, o = host(ref), host(out)
    assert np.abs(o - r).max() <= 1e-12 * np.abs(r).max()
    assert np.all(o.reshape(2 * E, n3)[1::2] == 7.0)  # untouched elements


@pytest.mark.parametrize("N", [8, 11, 13, 15])
def test_stiffness_mfma_gather_on_load(gpu, N):
    """The matrix-core kernel reading u through the point -> dof index array (and an optional
    device scale) against the bit-exact scalar kernel fed the same values: MFMA tolerance."""
    n3 = (N + 1) ** 3
    E = 5
    _, G, D = stiffness_inputs(E, N, 400 + N)
    rng = np.random.default_rng(410 + N)
    ndof = (E * n3) // 2
    pd = rng.integers(-1, ndof, E * n3).astype(np.int32)
    v = rng.uniform(-1, 1, ndof)
    scale = np.array([0.37])
    u = np.where(pd >= 0, scale[0] * v[np.maximum(pd, 0)], 0.0)
    Au, _ = oracle_stiffness(u, G, D, N, 3)
    dG = [dev(g, gpu) for g in G]
    for sc in (None, dev(scale, gpu)):
        ref = Au if sc is not None else oracle_stiffness(np.where(pd >= 0, v[np.maximum(pd, 0)], 0.0), G, D, N, 3)[0]
        out = torch.full((E * n3,), 7.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_matrix_mfma_gather", out, dev(v, gpu), sc, dev(pd, gpu), dev(D, gpu), dG, None, E, N)
        assert np.abs(host(out) - ref).max() <= 1e-12 * np.abs(ref).max(), N


def test_stiffness_fused_unsupported_degree(gpu):
    z = torch.zeros(8, dtype=torch.float64, device=gpu)
    with pytest.raises(lib.FddError):
        k("fdd_dom_stiffness_matrix", z, z, z, [z] * 6, 1, 16)


def mixed_level_inputs(seed):
    """A Subdomain-like element list with mixed degrees (subdomain.tpp:558-566,
    1603-1630): levels N = 7, 5, 3, 1 interleaved."""
    rng = np.random.default_rng(seed)
    degs = [7, 5, 3, 1]
    elems = rng.integers(0, 4, 90)
    offset, vert, level = [], [], []
    elem_offsets = {l: [] for l in range(4)}
    o = 0
    for l in elems:
        n3 = (degs[l] + 1) ** 3
        offset += [o] * n3
        vert += list(range(n3))
        level += [l] * n3
        elem_offsets[int(l)].append(o)
        o += n3
    npts = o
    u = rng.uniform(-1, 1, npts)
    G = [rng.uniform(0.1, 1.0, npts) if g < 3 else rng.uniform(-0.3, 0.3, npts) for g in range(6)]
    D = [np.ascontiguousarray(S.gll(d)[2]) for d in degs]
    return degs, np.array(offset, np.int32), np.array(vert, np.int32), np.array(level, np.int32), elem_offsets, u, G, D


def test_sub_stiffness_mixed_degree(gpu):
    L = S.oracle()
    degs, offset, vert, level, elem_offsets, u, G, D = mixed_level_inputs(5)
    npts = len(u)
    GDu = [np.zeros(npts) for _ in range(3)]
    Au = np.zeros(npts)
    gd = (vp * 3)(*[a.ctypes.data for a in GDu])
    gg = (vp * 6)(*[a.ctypes.data for a in G])
    Dp = (vp * 4)(*[a.ctypes.data for a in D])
    pd = (ctypes.c_int * 4)(*degs)
    L.orc_sub_stiffness_matrix_1(gd, P(u), Dp, P(offset), P(vert), P(level), pd, gg, npts, 3)
    L.orc_sub_stiffness_matrix_2(P(Au), gd, Dp, P(offset), P(vert), P(level), pd, npts, 3)

    dD = [dev(d, gpu) for d in D]
    dG = [dev(g, gpu) for g in G]
    du = dev(u, gpu)
    dGDu = [torch.zeros(npts, dtype=torch.float64, device=gpu) for _ in range(3)]
    dAu = torch.zeros(npts, dtype=torch.float64, device=gpu)
    doff, dvert, dlev = dev(offset, gpu), dev(vert, gpu), dev(level, gpu)
    k("fdd_sub_stiffness_matrix_1", dGDu, du, dD, doff, dvert, dlev, pd, 4, dG, npts, 3)
    k("fdd_sub_stiffness_matrix_2", dAu, dGDu, dD, doff, dvert, dlev, pd, 4, npts, 3)
    assert np.array_equal(host(dAu), Au)

    # level-sorted fused form: one launch per level over that level's elements
    dAu2 = torch.zeros(npts, dtype=torch.float64, device=gpu)
    for l, d in enumerate(degs):
        eo = np.array(elem_offsets[l], np.int32)
        if len(eo):
            k("fdd_sub_stiffness_matrix", dAu2, du, dD[l], dG, dev(eo, gpu), len(eo), d)
    assert np.array_equal(host(dAu2), Au)


# ---------------------------------------------------------- restriction
@pytest.mark.parametrize("Nf,Nc", [(7, 1), (7, 5), (7, 4), (6, 3), (5, 3), (3, 1), (15, 9), (15, 1), (2, 1)])
def test_restriction(gpu, Nf, Nc):
    L = S.oracle()
    E = 53
    n_f, n_c = Nf + 1, Nc + 1
    J = np.ascontiguousarray(S.J_cf(Nc, Nf))
    u = rnd(E * n_f**3, 100 + Nf)
    w1 = np.zeros(E * n_f * n_f * n_c)
    w2 = np.zeros(E * n_f * n_c * n_c)
    uc = np.zeros(E * n_c**3)
    L.orc_sub_restriction_1(P(w1), P(J), P(u), len(w1), n_f, n_c, 3)
    L.orc_sub_restriction_2(P(w2), P(J), P(w1), len(w2), n_f, n_c, 3)
    L.orc_sub_restriction_3(P(uc), P(J), P(w2), len(uc), n_f, n_c)

    dJ, du = dev(J, gpu), dev(u, gpu)
    d1 = torch.zeros(len(w1), dtype=torch.float64, device=gpu)
    d2 = torch.zeros(len(w2), dtype=torch.float64, device=gpu)
    dc = torch.zeros(len(uc), dtype=torch.float64, device=gpu)
    k("fdd_sub_restriction_1", d1, dJ, du, len(w1), n_f, n_c, 3)
    k("fdd_sub_restriction_2", d2, dJ, d1, len(w2), n_f, n_c, 3)
    k("fdd_sub_restriction_3", dc, dJ, d2, len(uc), n_f, n_c)
    assert np.array_equal(host(d1), w1)
    assert np.array_equal(host(d2), w2)
    assert np.array_equal(host(dc), uc)

    dc2 = torch.zeros(len(uc), dtype=torch.float64, device=gpu)
    k("fdd_sub_restriction", dc2, dJ, du, E, n_f, n_c)
    assert np.array_equal(host(dc2), uc)


def test_restriction_2d(gpu):
    L = S.oracle()
    E, Nf, Nc = 77, 7, 3
    n_f, n_c = Nf + 1, Nc + 1
    J = np.ascontiguousarray(S.J_cf(Nc, Nf))
    u = rnd(E * n_f**2, 111)
    w1 = np.zeros(E * n_f * n_c)
    uc = np.zeros(E * n_c * n_c)
    L.orc_sub_restriction_1(P(w1), P(J), P(u), len(w1), n_f, n_c, 2)
    L.orc_sub_restriction_2(P(uc), P(J), P(w1), len(uc), n_f, n_c, 2)
    d1 = torch.zeros(len(w1), dtype=torch.float64, device=gpu)
    dc = torch.zeros(len(uc), dtype=torch.float64, device=gpu)
    k("fdd_sub_restriction_1", d1, dev(J, gpu), dev(u, gpu), len(w1), n_f, n_c, 2)
    k("fdd_sub_restriction_2", dc, dev(J, gpu), d1, len(uc), n_f, n_c, 2)
    assert np.array_equal(host(d1), w1) and np.array_equal(host(dc), uc)
    # both `dim == 2` launches as one (fdd_sub_restriction_2d), bit for bit, over the reference's level pairs and beyond
    for E2, Nf2, Nc2 in ((77, 7, 3), (1, 7, 1), (300, 3, 1), (41, 15, 7), (9, 5, 4), (1000, 2, 1)):
        nf, nc = Nf2 + 1, Nc2 + 1
        J2 = np.ascontiguousarray(S.J_cf(Nc2, Nf2))
        u2 = rnd(E2 * nf * nf, 112 + Nf2)
        t2, ref2 = np.zeros(E2 * nf * nc), np.zeros(E2 * nc * nc)
        L.orc_sub_restriction_1(P(t2), P(J2), P(u2), len(t2), nf, nc, 2)
        L.orc_sub_restriction_2(P(ref2), P(J2), P(t2), len(ref2), nf, nc, 2)
        out2 = torch.full((len(ref2),), 3.0, dtype=torch.float64, device=gpu)
        k("fdd_sub_restriction_2d", out2, dev(J2, gpu), dev(u2, gpu), E2, nf, nc)
        assert np.array_equal(host(out2), ref2), (E2, Nf2, Nc2)


# ------------------------------------------------------------------ AMG
def test_amg_elementwise(gpu):
    L = S.oracle()
    n = 99991
    f, Sv, r, D, w, v, u = (rnd(n, s) for s in range(120, 127))
    alpha = 0.83

    Sr, ww = np.zeros(n), np.zeros(n)
    L.orc_amg_main_scaled_residual(P(Sr), P(ww), P(f), P(Sv), ctypes.c_double(alpha), n)
    dSr = torch.zeros(n, dtype=torch.float64, device=gpu)
    dw = torch.zeros(n, dtype=torch.float64, device=gpu)
    k("fdd_amg_main_scaled_residual", dSr, dw, dev(f, gpu), dev(Sv, gpu), alpha, n)
    assert np.array_equal(host(dSr), Sr) and np.array_equal(host(dw), ww)

    w2, v2 = w.copy(), v.copy()
    L.orc_amg_main_polynomial_evaluation(P(w2), P(v2), P(r), P(D), ctypes.c_double(alpha), n)
    dw, dv = dev(w, gpu), dev(v, gpu)
    k("fdd_amg_main_polynomial_evaluation", dw, dv, dev(r, gpu), dev(D, gpu), alpha, n)
    assert np.array_equal(host(dw), w2) and np.array_equal(host(dv), v2)

    u2 = u.copy()
    L.orc_amg_main_update_field(P(u2), P(w), P(D), n)
    du = dev(u, gpu)
    k("fdd_amg_main_update_field", du, dev(w, gpu), dev(D, gpu), n)
    assert np.array_equal(host(du), u2)

    uv = np.zeros(n)
    L.orc_amg_vector_multiplication(P(uv), P(u), P(v), n)
    duv = torch.zeros(n, dtype=torch.float64, device=gpu)
    k("fdd_amg_vector_multiplication", duv, dev(u, gpu), dev(v, gpu), n)
    assert np.array_equal(host(duv), uv)

    k("fdd_amg_vector_set_to_value", duv, -2.5, n)
    assert np.all(host(duv) == -2.5)


# ------------------------------------- fused dssum / multi-vector forms
def boolean_gather(nodes, points, seed, empty_points=0):
    """Qt of a boolean scatter: every point belongs to exactly one node (or, for
    `empty_points` of them, to none: Dirichlet points of a Subdomain Q)."""
    rng = np.random.default_rng(seed)
    owner = rng.integers(0, nodes, points)
    owner[:nodes] = np.arange(nodes)  # every node has at least one point
    rng.shuffle(owner)
    keep = np.ones(points, bool)
    keep[rng.choice(points, empty_points, replace=False)] = False
    order = np.argsort(owner[keep], kind="stable")
    pts = np.nonzero(keep)[0][order].astype(np.int32)
    ptr = np.zeros(nodes + 1, np.int32)
    np.add.at(ptr, owner[keep] + 1, 1)
    ptr = np.cumsum(ptr).astype(np.int32)
    return ptr, pts, np.nonzero(~keep)[0].astype(np.int32)


@pytest.mark.parametrize("weighted,masked", [(False, False), (True, False), (False, True), (True, True)])
def test_dssum_fused_equals_two_spmvs(gpu, weighted, masked):
    L = S.oracle()
    nodes, points = 40000, 90000
    tptr, tcol, _ = boolean_gather(nodes, points, 1)
    tval = np.ones(points)
    # Q = Qt^T: one entry per point
    qcol = np.zeros(points, np.int32)
    for nd in range(nodes):
        qcol[tcol[tptr[nd]:tptr[nd + 1]]] = nd
    qptr = np.arange(points + 1, dtype=np.int32)
    u, w, m = rnd(points, 2), rnd(nodes, 3) + 2, (rnd(points, 4) > 0).astype(float)

    t = np.zeros(nodes)
    if weighted:
        L.orc_csr_multiply_weight(P(t), P(tptr), P(tcol), P(tval), P(u), P(w), nodes)
    else:
        L.orc_csr_multiply(P(t), P(tptr), P(tcol), P(tval), P(u), nodes)
    ref = np.zeros(points)
    if masked:
        L.orc_csr_multiply_weight(P(ref), P(qptr), P(qcol), P(tval), P(t), P(m), points)
    else:
        L.orc_csr_multiply(P(ref), P(qptr), P(qcol), P(tval), P(t), points)

    dptr, dcol, du = dev(tptr, gpu), dev(tcol, gpu), dev(u, gpu)
    dw = dev(w, gpu) if weighted else None
    dm = dev(m, gpu) if masked else None
    out = torch.full((points,), 9.0, dtype=torch.float64, device=gpu)
    dt = torch.zeros(nodes, dtype=torch.float64, device=gpu)
    k("fdd_dssum_fused", out, dt, dptr, dcol, du, dw, dm, 0, nodes)
    assert np.array_equal(host(out), ref) and np.array_equal(host(dt), t)

    # in place, and split into gather(prefix) / fused(rest) / scatter(prefix)
    nb = 1234
    inplace = dev(u, gpu)
    k("fdd_dssum_gather", dt, dptr, dcol, inplace, dw, 0, nb)
    k("fdd_dssum_fused", inplace, None, dptr, dcol, inplace, dw, dm, nb, nodes)
    k("fdd_dssum_scatter", inplace, dt, dptr, dcol, dm, 0, nb)
    assert np.array_equal(host(inplace), ref)

    # the same on the row blocks of Qt's SpMV plan (LDS-staged, balanced)
    plan = vp()
    lib.hip().call("fdd_csr_plan_create", ctypes.byref(plan), P(tptr), nodes, points, points)
    lib.hip().call("fdd_csr_plan_set_unit_values", plan, 1)
    try:
        kind = ctypes.c_int(-1)
        lib.hip().call("fdd_csr_plan_kind", plan, ctypes.byref(kind))
        assert kind.value == 1
        out.fill_(9.0)
        dt.zero_()
        k("fdd_csr_plan_dssum", plan, out, dt, dptr, dcol, du, dw, dm, 0, nodes, 0)
        assert np.array_equal(host(out), ref) and np.array_equal(host(dt), t)
        for nb2 in (1234, 2048 * 3, 1):  # prefix boundaries inside and on row-block edges
            inplace = dev(u, gpu)
            dt.zero_()
            k("fdd_csr_plan_dssum", plan, None, dt, dptr, dcol, inplace, dw, None, 0, nb2, 1)
            assert np.array_equal(host(dt)[:nb2], t[:nb2]) and not host(dt)[nb2:].any()
            k("fdd_csr_plan_dssum", plan, inplace, None, dptr, dcol, inplace, dw, dm, nb2, nodes, 0)
            k("fdd_csr_plan_dssum", plan, inplace, dt, dptr, dcol, None, None, dm, 0, nb2, 2)
            assert np.array_equal(host(inplace), ref)
        if weighted:
            ws = reduce_workspace(gpu)
            o1 = torch.zeros(1, dtype=torch.float64, device=gpu)
            o2 = torch.zeros(1, dtype=torch.float64, device=gpu)
            k("fdd_gather_weighted_norm2", o1, ws, dptr, dcol, du, dw, nodes)
            k("fdd_csr_plan_gather_weighted_norm2", plan, o2, ws, dptr, dcol, du, dw)
            assert abs(host(o1)[0] - host(o2)[0]) <= 1e-13 * abs(host(o1)[0])
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)


def test_dssum_fused_with_points_without_dof(gpu):
    """Subdomain Q has empty rows on Dirichlet points (subdomain.tpp:1517-1520):
    they receive the 0.0 the SpMV writes."""
    L = S.oracle()
    nodes, points = 30000, 70000
    tptr, tcol, no_dof = boolean_gather(nodes, points, 5, empty_points=5000)
    nnz = len(tcol)
    qptr = np.zeros(points + 1, np.int32)
    qcol = np.zeros(nnz, np.int32)
    has = np.ones(points, bool)
    has[no_dof] = False
    qptr[1:] = np.cumsum(has)
    owner = np.zeros(points, np.int32)
    for nd in range(nodes):
        owner[tcol[tptr[nd]:tptr[nd + 1]]] = nd
    qcol[:] = owner[has]
    u = rnd(points, 6)
    ones = np.ones(nnz)
    t, ref = np.zeros(nodes), np.full(points, 5.0)
    L.orc_csr_multiply(P(t), P(tptr), P(tcol), P(ones), P(u), nodes)
    L.orc_csr_multiply(P(ref), P(qptr), P(qcol), P(ones), P(t), points)
    out = torch.full((points,), 5.0, dtype=torch.float64, device=gpu)
    k("fdd_dssum_fused", out, None, dev(tptr, gpu), dev(tcol, gpu), dev(u, gpu), None, None, 0, nodes)
    k("fdd_fill_indexed", out, dev(no_dof, gpu), 0.0, len(no_dof))
    assert np.array_equal(host(out), ref)


@pytest.mark.parametrize("m", [1, 2, 5, 8])
def test_multi_axpy_equals_successive_axpys(gpu, m):
    L = S.oracle()
    for n in (1, 1001, 400003):
        q = rnd(n, 7)
        V = [rnd(n, 10 + i) for i in range(m)]
        c = rnd(m, 8)
        ref = q.copy()
        for i in range(m):
            L.orc_vector_vector_addition(P(ref), ctypes.c_double(1.0), P(ref), ctypes.c_double(c[i]), P(V[i]), n)
        dq = dev(q, gpu)
        k("fdd_multi_axpy", dq, (ctypes.c_double * m)(*c), [dev(v, gpu) for v in V], m, n)
        assert np.array_equal(host(dq), ref)


@pytest.mark.parametrize("m", [1, 3, 5, 8])
def test_multi_weighted_inner_product(gpu, m):
    L = S.oracle()
    n = 700001
    nb = (n + 127) // 128
    a, w = rnd(n, 20), np.abs(rnd(n, 21))
    B = [rnd(n, 30 + i) for i in range(m)]
    ws = reduce_workspace(gpu)
    out = torch.zeros(8, dtype=torch.float64, device=gpu)
    k("fdd_multi_weighted_inner_product", out, ws, dev(a, gpu), [dev(b, gpu) for b in B], m, dev(w, gpu), n)
    got = host(out)
    block = np.zeros(nb)
    for i in range(m):
        L.orc_sub_weighted_inner_product(P(block), P(a), P(B[i]), P(w), n, nb)
        ref = L.orc_block_sum(P(block), nb)
        assert abs(got[i] - ref) <= 1e-13 * np.abs(a * B[i] * w).sum()


def test_gather_weighted_norm2(gpu):
    L = S.oracle()
    nodes, points = 50000, 120000
    tptr, tcol, _ = boolean_gather(nodes, points, 9)
    u, w = rnd(points, 40), (rnd(nodes, 41) > -0.5).astype(float)
    t = np.zeros(nodes)
    ones = np.ones(points)
    L.orc_csr_multiply_weight(P(t), P(tptr), P(tcol), P(ones), P(u), P(w), nodes)
    nb = (nodes + 127) // 128
    block = np.zeros(nb)
    L.orc_sub_weighted_inner_product(P(block), P(t), P(t), P(w), nodes, nb)
    ref = L.orc_block_sum(P(block), nb)
    ws = reduce_workspace(gpu)
    out = torch.zeros(1, dtype=torch.float64, device=gpu)
    k("fdd_gather_weighted_norm2", out, ws, dev(tptr, gpu), dev(tcol, gpu), dev(u, gpu), dev(w, gpu), nodes)
    assert abs(host(out)[0] - ref) <= 1e-13 * ref


@pytest.mark.parametrize("m", [1, 2, 4, 8])
def test_multi_axpy_norm2_with_device_coefficients(gpu, m):
    """Gram-Schmidt update + norm in one pass: the update is the arithmetic of
    fdd_multi_axpy with coefficients sign*c[k] read from device memory (bit-exact),
    the norm is the weighted dot of the result (reduction tolerance)."""
    L = S.oracle()
    ws = reduce_workspace(gpu)
    for n in (1, 1001, 400003):
        y, w = rnd(n, 50), np.abs(rnd(n, 51))
        X = [rnd(n, 60 + i) for i in range(m)]
        c = rnd(m, 52)
        ref = y.copy()
        for i in range(m):
            L.orc_vector_vector_addition(P(ref), ctypes.c_double(1.0), P(ref), ctypes.c_double(-c[i]), P(X[i]), n)
        nb = (n + 127) // 128
        block = np.zeros(nb)
        L.orc_sub_weighted_inner_product(P(block), P(ref), P(ref), P(w), n, nb)
        norm2 = L.orc_block_sum(P(block), nb)
        dy = dev(y, gpu)
        out = torch.zeros(1, dtype=torch.float64, device=gpu)
        k("fdd_multi_axpy_norm2_dev", out, ws, dy, dev(c, gpu), -1.0, [dev(x, gpu) for x in X], m, dev(w, gpu), n)
        assert np.array_equal(host(dy), ref)
        assert abs(host(out)[0] - norm2) <= 1e-13 * norm2
        # x = (1 / sqrt(norm2_dev)) * y: the host sequence alpha = sqrt(s); scaling by 1.0 / alpha
        dx = torch.zeros(n, dtype=torch.float64, device=gpu)
        k("fdd_vector_scaling_rsqrt_dev", dx, out, dy, n)
        s = host(out)[0]
        sref = np.zeros(n)
        L.orc_vector_scaling(P(sref), ctypes.c_double(1.0 / np.sqrt(s)), P(ref), n)
        assert np.array_equal(host(dx), sref)


def test_scaled_forms_equal_scaling_first(gpu):
    """The *_scaled entries read inv[k] * x_k[d] on load: exactly the values vector_scaling
    would have stored, so each must equal (bit for bit / to reduction rounding) its unscaled
    sibling applied to pre-scaled vectors."""
    L = S.oracle()
    ws = reduce_workspace(gpu)
    m, n = 4, 300001
    X = [rnd(n, 200 + i) for i in range(m)]
    inv = np.abs(rnd(m, 210)) + 0.5
    Xs = []
    for i in range(m):
        t = np.zeros(n)
        L.orc_vector_scaling(P(t), ctypes.c_double(inv[i]), P(X[i]), n)
        Xs.append(t)
    a, w, c = rnd(n, 220), np.abs(rnd(n, 221)), rnd(m, 222)
    dX, dXs, dinv = [dev(x, gpu) for x in X], [dev(x, gpu) for x in Xs], dev(inv, gpu)
    # multi-dot
    o1, o2 = torch.zeros(8, dtype=torch.float64, device=gpu), torch.zeros(8, dtype=torch.float64, device=gpu)
    k("fdd_multi_weighted_inner_product_scaled", o1, ws, dev(a, gpu), dX, dinv, m, dev(w, gpu), n)
    k("fdd_multi_weighted_inner_product", o2, ws, dev(a, gpu), dXs, m, dev(w, gpu), n)
    assert np.array_equal(host(o1), host(o2))
    # Gram-Schmidt update into a separate destination + norm
    dy, dst1 = dev(a, gpu), torch.zeros(n, dtype=torch.float64, device=gpu)
    n1, n2 = torch.zeros(1, dtype=torch.float64, device=gpu), torch.zeros(1, dtype=torch.float64, device=gpu)
    k("fdd_multi_axpy_norm2_scaled_dev", n1, ws, dst1, dy, dev(c, gpu), -1.0, dX, dinv, m, dev(w, gpu), n)
    assert np.array_equal(host(dy), a)  # the source is left alone
    dy2 = dev(a, gpu)
    k("fdd_multi_axpy_norm2_dev", n2, ws, dy2, dev(c, gpu), -1.0, dXs, m, dev(w, gpu), n)
    assert np.array_equal(host(dst1), host(dy2)) and np.array_equal(host(n1), host(n2))
    # solution update
    q1, q2 = dev(a, gpu), dev(a, gpu)
    k("fdd_multi_axpy_scaled_dev", q1, dev(c, gpu), dX, dinv, m, n)
    k("fdd_multi_axpy_dev", q2, dev(c, gpu), dXs, m, n)
    assert np.array_equal(host(q1), host(q2))
    # scaling by a device scalar
    out = torch.zeros(n, dtype=torch.float64, device=gpu)
    k("fdd_vector_scaling_dev", out, dinv, dX[0], n)
    assert np.array_equal(host(out), Xs[0])
    # gather-on-load stiffness of a scaled dof vector
    N, E = 7, 9
    n3 = (N + 1) ** 3
    _, G, D = stiffness_inputs(E, N, 230)
    rng = np.random.default_rng(231)
    ndof = 2000
    pd = rng.integers(-1, ndof, E * n3).astype(np.int32)
    v = rng.uniform(-1, 1, ndof)
    vs = np.zeros(ndof)
    L.orc_vector_scaling(P(vs), ctypes.c_double(inv[1]), P(v), ndof)
    dG = [dev(g, gpu) for g in G]
    A1, A2 = torch.zeros(E * n3, dtype=torch.float64, device=gpu), torch.zeros(E * n3, dtype=torch.float64, device=gpu)
    k("fdd_sub_stiffness_matrix_gather_scaled", A1, dev(v, gpu), dinv[1:], dev(pd, gpu), dev(D, gpu), dG, None, E, N)
    k("fdd_sub_stiffness_matrix_gather", A2, dev(vs, gpu), dev(pd, gpu), dev(D, gpu), dG, None, E, N)
    assert np.array_equal(host(A1), host(A2))


def test_limited_linear_combination_and_small_device_ops(gpu):
    """fdd_multi_lincomb_limited_dev (solution update whose column count never left the device; q taken as 0
    without being read), fdd_xpby_ratio_dev (p = z + (num/den) p), fdd_sqrt_sum_dev."""
    L = S.oracle()
    m, n = 5, 200003
    V = [rnd(n, 300 + i) for i in range(m)]
    c, inv = rnd(m, 310), np.abs(rnd(m, 311)) + 0.5
    dV, dc, dinv = [dev(v, gpu) for v in V], dev(c, gpu), dev(inv, gpu)
    for last in (0, 2, 4):
        ref = np.zeros(n)
        for i in range(last + 1):
            t = np.zeros(n)
            L.orc_vector_scaling(P(t), ctypes.c_double(inv[i]), P(V[i]), n)
            L.orc_vector_vector_addition(P(ref), ctypes.c_double(1.0), P(ref), ctypes.c_double(c[i]), P(t), n)
        q = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)  # garbage in: must not be read
        k("fdd_multi_lincomb_limited_dev", q, 1, dc, dV, dinv, dev(np.array([float(last)]), gpu), m, n)
        assert np.array_equal(host(q), ref), last
        # accumulate on top of an existing q, no limit
        q2 = dev(rnd(n, 320), gpu)
        ref2 = rnd(n, 320)
        for i in range(m):
            L.orc_vector_vector_addition(P(ref2), ctypes.c_double(1.0), P(ref2), ctypes.c_double(c[i]), P(V[i]), n)
        k("fdd_multi_lincomb_limited_dev", q2, 0, dc, dV, None, None, m, n)
        assert np.array_equal(host(q2), ref2)
    z, p = rnd(n, 330), rnd(n, 331)
    num, den = np.array([0.37]), np.array([-1.9])
    dp = dev(p, gpu)
    k("fdd_xpby_ratio_dev", dp, dev(z, gpu), dev(num, gpu), dev(den, gpu), dp, n)
    assert np.array_equal(host(dp), z + (num[0] / den[0]) * p)
    parts = np.array([2.25, 4.0])
    out = torch.zeros(1, dtype=torch.float64, device=gpu)
    k("fdd_sqrt_sum_dev", out, dev(parts, gpu), 2)
    assert host(out)[0] == 2.5


@pytest.mark.parametrize("n", [1, 2, 129, 4097])
def test_xmay_ratio_dev(gpu, n):
    """fdd_xmay_ratio_dev: out = x - (*num / *den) * y against numpy, as bits; out separate and out == x; every pointer on
    a 16-byte boundary and every pointer 8 bytes off one (the one-value-per-lane path); guard values around out"""
    x, y = rnd(n, 340 + n), rnd(n, 341 + n)
    num, den = np.array([0.37]), np.array([-1.9])
    expect = x - (num[0] / den[0]) * y
    dnum, dden = dev(num, gpu), dev(den, gpu)
    for shift in (0, 1):
        for alias in (False, True):
            X, Y, O = (torch.full((n + shift + 3,), 777.0, dtype=torch.float64, device=gpu) for _ in range(3))
            dx, dy = X[shift : shift + n], Y[shift : shift + n]
            dx.copy_(dev(x, gpu))
            dy.copy_(dev(y, gpu))
            out = dx if alias else O[shift : shift + n]
            assert out.data_ptr() % 16 == 8 * shift and dy.data_ptr() % 16 == 8 * shift
            k("fdd_xmay_ratio_dev", out, dx, dnum, dden, dy, n)
            case = (n, shift, alias)
            assert np.array_equal(host(out).view(np.uint64), expect.view(np.uint64)), case
            assert np.array_equal(host(dy), y) and (alias or np.array_equal(host(dx), x)), case
            for whole in (X, Y, O):
                w = host(whole)
                assert (w[:shift] == 777.0).all() and (w[shift + n :] == 777.0).all(), case
            if alias:
                assert (host(O) == 777.0).all(), case


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("m", [1, 5, 8])
def test_multi_lincomb_scaled_dev(gpu, m, scaled):
    """fdd_multi_lincomb_scaled_dev: the bits of fdd_multi_axpy_scaled_dev on a zeroed q and of
    fdd_multi_lincomb_limited_dev without a limit; with q_is_zero = 1 a q full of NaN is not read"""
    n = 4099
    V = [dev(rnd(n, 350 + i), gpu) for i in range(m)]
    dc = dev(rnd(m, 360), gpu)
    dinv = dev(np.abs(rnd(m, 361)) + 0.5, gpu) if scaled else None
    q_axpy = torch.zeros(n, dtype=torch.float64, device=gpu)
    k("fdd_multi_axpy_scaled_dev", q_axpy, dc, V, dinv, m, n)
    assert np.abs(host(q_axpy)).max() > 0.0
    for q_is_zero in (1, 0):
        start = float("nan") if q_is_zero else 0.0
        Q1, Q2 = (torch.full((n + 16,), 777.0, dtype=torch.float64, device=gpu) for _ in range(2))
        q1, q2 = Q1[8 : 8 + n], Q2[8 : 8 + n]
        q1.fill_(start)
        q2.fill_(start)
        k("fdd_multi_lincomb_scaled_dev", q1, q_is_zero, dc, V, dinv, m, n)
        k("fdd_multi_lincomb_limited_dev", q2, q_is_zero, dc, V, dinv, None, m, n)
        case = (m, scaled, q_is_zero)
        assert np.array_equal(host(q1).view(np.uint64), host(q_axpy).view(np.uint64)), case
        assert np.array_equal(host(q1).view(np.uint64), host(q2).view(np.uint64)), case
        assert (host(Q1)[:8] == 777.0).all() and (host(Q1)[8 + n :] == 777.0).all(), case


def test_gather_indexed(gpu):
    n_in, n_out = 5000, 7001
    x, sc = rnd(n_in, 70), rnd(n_out, 71)
    idx = np.random.default_rng(72).integers(-1, n_in, n_out).astype(np.int32)
    base = np.where(idx >= 0, x[np.maximum(idx, 0)], 0.0)
    out = torch.full((n_out,), 9.0, dtype=torch.float64, device=gpu)
    k("fdd_gather_indexed", out, dev(x, gpu), dev(idx, gpu), None, n_out)
    assert np.array_equal(host(out), base)
    k("fdd_gather_indexed", out, dev(x, gpu), dev(idx, gpu), dev(sc, gpu), n_out)
    assert np.array_equal(host(out), base * sc)


def test_gather_from_two_sources_and_scatter_add(gpu):
    """The two small kernels of the composite's exchange and hanging-point stages: a gather whose source vector has its
    head in one buffer and its tail in another (unshifted indices), and y[index[i]] += t[i] on distinct indices."""
    n_lo, n_hi, n_out = 4000, 9000, 7001
    lo, hi = rnd(n_lo, 170), rnd(n_hi, 171)  # hi is addressed by the same index as the whole vector: entries below n_lo unused
    idx = np.random.default_rng(172).integers(-1, n_hi, n_out).astype(np.int32)
    want = np.where(idx < 0, 0.0, np.where(idx < n_lo, lo[np.clip(idx, 0, n_lo - 1)], hi[np.maximum(idx, 0)]))
    out = torch.full((n_out,), 9.0, dtype=torch.float64, device=gpu)
    k("fdd_gather_indexed_split", out, dev(lo, gpu), dev(hi, gpu), n_lo, dev(idx, gpu), n_out)
    assert np.array_equal(host(out), want)
    y, t = rnd(n_hi, 173), rnd(3000, 174)
    rows = np.random.default_rng(175).choice(n_hi, size=3000, replace=False).astype(np.int32)
    ref = y.copy()
    ref[rows] = ref[rows] + t
    dy = dev(y, gpu)
    k("fdd_scatter_add_indexed", dy, dev(rows, gpu), dev(t, gpu), 3000)
    assert np.array_equal(host(dy), ref)
    y32, t32 = y.astype(np.float32), t.astype(np.float32)
    ref32 = y32.copy()
    ref32[rows] = ref32[rows] + t32
    dy32 = dev(y32, gpu)
    k("fdd_scatter_add_indexed_f32", dy32, dev(rows, gpu), dev(t32, gpu), 3000)
    assert np.array_equal(host(dy32), ref32)


@pytest.mark.parametrize("shape", ["boolean", "stencil", "dense"])
def test_csr_plan_matvec_axpby(gpu, shape):
    """y = alpha*A*x + beta*y on the plan (cusparseSpMV's role in the AMG V-cycle);
    beta = 0 must not read y (NaN in, numbers out)."""
    L = S.oracle()
    rng = np.random.default_rng(80)
    if shape == "boolean":
        ptr, col, _ = boolean_gather(3000, 9000, 81)
        val = np.ones(len(col))
        rows, cols = 3000, 9000
    elif shape == "stencil":
        import scipy.sparse as sp

        m = 17
        T = sp.diags([1.0, -2.0, 1.0], [-1, 0, 1], shape=(m, m))
        A = (sp.kron(sp.kron(T, sp.eye(m)), sp.eye(m)) + sp.kron(sp.kron(sp.eye(m), T), sp.eye(m)) + sp.kron(sp.eye(m), sp.kron(sp.eye(m), T))).tocsr()
        A.sort_indices()
        ptr, col, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
        rows = cols = m**3
    else:
        rows = cols = 37
        ptr = (np.arange(rows + 1) * cols).astype(np.int32)
        col = np.tile(np.arange(cols), rows).astype(np.int32)
        val = rng.uniform(-1, 1, rows * cols)
    x, y0 = rnd(cols, 82), rnd(rows, 83)
    plan = vp()
    lib.hip().call("fdd_csr_plan_create", ctypes.byref(plan), vp(ptr.ctypes.data), rows, cols, len(col))
    try:
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (1.0, 1.0), (0.5, -2.0)):
            ref = y0.copy()
            L.orc_amg_matvec(P(ref), P(ptr), P(col), P(val), P(x), ctypes.c_double(alpha), ctypes.c_double(beta), rows)
            y_in = np.full(rows, np.nan) if beta == 0.0 else y0
            dy = dev(y_in, gpu)
            k("fdd_csr_plan_matvec", plan, dy, dev(ptr, gpu), dev(col, gpu), dev(val, gpu), dev(x, gpu), alpha, beta)
            # the entry stands in for cusparseSpMV, whose summation order is undefined: row blocks with few, wide rows
            # are summed by several lanes per row (boolean short-row matrices keep the column order)
            if shape == "boolean":
                assert np.array_equal(host(dy), ref), (shape, alpha, beta)
            else:
                assert np.allclose(host(dy), ref, rtol=1e-12, atol=1e-13), (shape, alpha, beta)
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)


@pytest.mark.parametrize("shape", ["boolean", "stencil", "dense", "long_row"])
def test_amg_smoother_fused_into_spmv(gpu, shape):
    """The Chebyshev smoother's element-wise kernels as SpMV epilogues: the oracle's unfused
    sequence matvec -> scaled_residual / polynomial_evaluation / update_field ->
    vector_multiplication (subdomain.tpp:19-83), on every plan kind; bit-identical where the
    row sums keep the column order."""
    L = S.oracle()
    rng = np.random.default_rng(90)
    if shape == "boolean":
        n = 3000
        ptr, col, _ = boolean_gather(n, n, 91)
        val = rng.uniform(-1, 1, len(col))
    elif shape == "stencil":
        import scipy.sparse as sp

        m = 15
        T = sp.diags([1.0, -2.0, 1.0], [-1, 0, 1], shape=(m, m))
        A = (sp.kron(sp.kron(T, sp.eye(m)), sp.eye(m)) + sp.kron(sp.kron(sp.eye(m), T), sp.eye(m)) + sp.kron(sp.eye(m), sp.kron(sp.eye(m), T))).tocsr()
        A.sort_indices()
        ptr, col, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
        n = m**3
    elif shape == "dense":
        n = 41
        ptr = (np.arange(n + 1) * n).astype(np.int32)
        col = np.tile(np.arange(n), n).astype(np.int32)
        val = rng.uniform(-1, 1, n * n)
    else:  # one row longer than a row block among short ones
        n = 3000
        lens = np.full(n, 3)
        lens[1234] = 2500
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        col = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens]).astype(np.int32)
        val = rng.uniform(-1, 1, len(col))
    u, f, D, w_in = rnd(n, 92), rnd(n, 93), rnd(n, 94) + 1.5, rnd(n, 95)
    coef = -0.37
    # a row longer than a block is summed by the whole workgroup (shuffle tree) and the rows of a block with few, wide
    # rows by several lanes each: same values, other order (the reference's cusparseSpMV defines none)
    same = np.array_equal if shape == "boolean" else (lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-13))
    c = ctypes.c_double
    plan = vp()
    lib.hip().call("fdd_csr_plan_create", ctypes.byref(plan), vp(ptr.ctypes.data), n, n, len(col))
    dp, dc, dv, dD = dev(ptr, gpu), dev(col, gpu), dev(val, gpu), dev(D, gpu)
    try:
        # residual: work = f - A u; Sr = D*work, w = coef*Sr; out = D*w
        work = f.copy()
        L.orc_amg_matvec(P(work), P(ptr), P(col), P(val), P(u), c(-1.0), c(1.0), n)
        Sr, w, out = np.zeros(n), np.zeros(n), np.zeros(n)
        L.orc_amg_main_scaled_residual(P(Sr), P(w), P(work), P(D), c(coef), n)
        L.orc_amg_vector_multiplication(P(out), P(D), P(w), n)
        dwork = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
        dSr = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
        k("fdd_amg_smooth_residual_matvec", plan, dwork, dSr, dp, dc, dv, dev(u, gpu), dev(f, gpu), dD, coef)
        assert same(host(dSr), Sr) and same(host(dwork), out), shape

        # start (u = 0): Sr = D*f, out = D*(coef*Sr)
        Sr0, w0, out0 = np.zeros(n), np.zeros(n), np.zeros(n)
        L.orc_amg_main_scaled_residual(P(Sr0), P(w0), P(f), P(D), c(coef), n)
        L.orc_amg_vector_multiplication(P(out0), P(D), P(w0), n)
        dwork0 = torch.zeros(n, dtype=torch.float64, device=gpu)
        dSr0 = torch.zeros(n, dtype=torch.float64, device=gpu)
        k("fdd_amg_smooth_start", dwork0, dSr0, dev(f, gpu), dD, coef, n)
        assert same(host(dSr0), Sr0) and same(host(dwork0), out0), shape

        # polynomial: v = A work_in; v *= D; w = coef*Sr + v; out = D*w
        v = np.zeros(n)
        L.orc_amg_matvec(P(v), P(ptr), P(col), P(val), P(w_in), c(1.0), c(0.0), n)
        w1, out1 = np.zeros(n), np.zeros(n)
        L.orc_amg_main_polynomial_evaluation(P(w1), P(v), P(Sr), P(D), c(coef), n)
        L.orc_amg_vector_multiplication(P(out1), P(D), P(w1), n)
        dout = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
        k("fdd_amg_smooth_polynomial_matvec", plan, dout, dp, dc, dv, dev(w_in, gpu), dev(Sr, gpu), dD, coef)
        assert same(host(dout), out1), shape

        # update: the same w, then u += D*w
        u2 = u.copy()
        L.orc_amg_main_update_field(P(u2), P(w1), P(D), n)
        du = dev(u, gpu)
        k("fdd_amg_smooth_update_matvec", plan, du, dp, dc, dv, dev(w_in, gpu), dev(Sr, gpu), dD, coef)
        assert same(host(du), u2), shape

        # the same from u = 0 (pre-smoothing): u is written, not read -- the bits of the update on a zeroed vector
        u0 = np.zeros(n)
        L.orc_amg_main_update_field(P(u0), P(w1), P(D), n)
        du0 = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
        k("fdd_amg_smooth_update_matvec_from_zero", plan, du0, dp, dc, dv, dev(w_in, gpu), dev(Sr, gpu), dD, coef)
        assert same(host(du0), u0), shape
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)


@pytest.mark.parametrize("shape", ["short_rows", "stencil"])
def test_f32_spmv_and_fused_smoother(gpu, shape):
    """`Float = float` entries (AMG/config.hpp:4): f32 SpMV y = alpha*A*x + beta*y_in and the fused smoother
    epilogues, bit-exact against an IEEE-single restatement (numpy float32 scalars, products added in
    column order, no contraction), on both row-block sizes."""
    f32 = np.float32
    rng = np.random.default_rng(97)
    if shape == "short_rows":
        n = 700
        lens = rng.integers(0, 4, n)  # includes empty rows: the small row blocks
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        col = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens] + [np.zeros(0, int)]).astype(np.int32)
    else:
        import scipy.sparse as sp

        m = 9
        T = sp.diags([1.0, -2.0, 1.0], [-1, 0, 1], shape=(m, m))
        A = (sp.kron(sp.kron(T, sp.eye(m)), sp.eye(m)) + sp.kron(sp.kron(sp.eye(m), T), sp.eye(m)) + sp.kron(sp.eye(m), sp.kron(sp.eye(m), T))).tocsr()
        A.sort_indices()
        ptr, col = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        n = m**3
    val = rng.uniform(-1, 1, len(col)).astype(f32)
    x, yin, fv, Sr_in = (rng.uniform(-1, 1, n).astype(f32) for _ in range(4))
    D = (rng.uniform(0.5, 1.5, n)).astype(f32)
    u0 = rng.uniform(-1, 1, n).astype(f32)
    coef, alpha, beta = f32(-0.37), f32(0.75), f32(-1.25)

    def rowsum(v):
        out = np.zeros(n, f32)
        for r in range(n):
            s_ = f32(0)
            for j in range(ptr[r], ptr[r + 1]):
                s_ = f32(s_ + f32(val[j] * v[col[j]]))
            out[r] = s_
        return out

    Ax = rowsum(x)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    nan = lambda: torch.full((n,), float("nan"), dtype=torch.float32, device=gpu)
    plan = vp()
    lib.hip().call("fdd_csr_plan_create_f32", ctypes.byref(plan), vp(ptr.ctypes.data), n, n, len(col))
    dp, dc, dv, dD, dx = dev(ptr, gpu), dev(col, gpu), t32(val), t32(D), t32(x)
    try:
        kind = ctypes.c_int()
        lib.hip().call("fdd_csr_plan_kind", plan, ctypes.byref(kind))
        assert kind.value == 1
        # y = alpha*A*x + beta*y_in; beta = 0 never reads y
        y = nan()
        k("fdd_csr_plan_matvec_to_f32", plan, y, t32(yin), dp, dc, dv, dx, float(alpha), float(beta))
        assert np.array_equal(y.cpu().numpy(), (alpha * Ax + beta * yin).astype(f32))
        y = nan()
        k("fdd_csr_plan_matvec_to_f32", plan, y, None, dp, dc, dv, dx, float(alpha), 0.0)
        assert np.array_equal(y.cpu().numpy(), (alpha * Ax).astype(f32))
        # residual: work = -A x + f; Sr = D*work; w = coef*Sr; out = w*D
        work = (f32(-1) * Ax + f32(1) * fv).astype(f32)
        Sr = (D * work).astype(f32)
        out = ((coef * Sr).astype(f32) * D).astype(f32)
        dwork, dSr = nan(), nan()
        k("fdd_amg_smooth_residual_matvec_f32", plan, dwork, dSr, dp, dc, dv, dx, t32(fv), dD, float(coef))
        assert np.array_equal(dSr.cpu().numpy(), Sr) and np.array_equal(dwork.cpu().numpy(), out)
        # start: Sr = D*f; out = D*(coef*Sr)
        Sr0 = (D * fv).astype(f32)
        out0 = (D * (coef * Sr0).astype(f32)).astype(f32)
        dwork, dSr = nan(), nan()
        k("fdd_amg_smooth_start_f32", dwork, dSr, t32(fv), dD, float(coef), n)
        assert np.array_equal(dSr.cpu().numpy(), Sr0) and np.array_equal(dwork.cpu().numpy(), out0)
        # polynomial / update: v = (A x)*D; w = coef*Sr + v; out = w*D | u += D*w
        v = (Ax * D).astype(f32)
        w = ((coef * Sr_in).astype(f32) + v).astype(f32)
        dout = nan()
        k("fdd_amg_smooth_polynomial_matvec_f32", plan, dout, dp, dc, dv, dx, t32(Sr_in), dD, float(coef))
        assert np.array_equal(dout.cpu().numpy(), (w * D).astype(f32))
        du = t32(u0)
        k("fdd_amg_smooth_update_matvec_f32", plan, du, dp, dc, dv, dx, t32(Sr_in), dD, float(coef))
        assert np.array_equal(du.cpu().numpy(), (u0 + (D * w).astype(f32)).astype(f32))
        dz = torch.full((n,), float("nan"), dtype=torch.float32, device=gpu)
        k("fdd_amg_smooth_update_matvec_from_zero_f32", plan, dz, dp, dc, dv, dx, t32(Sr_in), dD, float(coef))
        assert np.array_equal(dz.cpu().numpy(), (f32(0) + (D * w).astype(f32)).astype(f32))
        # set
        d = nan()
        k("fdd_amg_vector_set_to_value_f32", d, 0.25, n)
        assert np.array_equal(d.cpu().numpy(), np.full(n, 0.25, f32))
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)


def test_graph_capture_and_replay(gpu):
    """fdd_graph_*: a captured launch sequence replays with the same result;
    the default stream is refused (it cannot be captured)."""
    L = lib.hip()
    n = 100003
    a, b = rnd(n, 90), rnd(n, 91)
    st = vp()
    L.call("fdd_stream_create", ctypes.byref(st))
    da, db, dc = dev(a, gpu), dev(b, gpu), torch.zeros(n, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    with pytest.raises(lib.FddError):
        L.call("fdd_graph_begin_capture", None)
    L.call("fdd_graph_begin_capture", st)
    L.call("fdd_vector_vector_addition", vp(dc.data_ptr()), 1.0, vp(da.data_ptr()), 2.0, vp(db.data_ptr()), n, st)
    L.call("fdd_vector_scaling", vp(dc.data_ptr()), 0.5, vp(dc.data_ptr()), n, st)
    g = vp()
    L.call("fdd_graph_end_capture", st, ctypes.byref(g))
    L.call("fdd_stream_sync", st)
    assert not host(dc).any()  # capture records, it does not run
    for _ in range(2):
        L.call("fdd_graph_launch", g, st)
        L.call("fdd_stream_sync", st)
        assert np.array_equal(host(dc), 0.5 * (1.0 * a + 2.0 * b))
        dc.zero_()
        torch.cuda.synchronize()
    L.call("fdd_graph_destroy", g)
    L.call("fdd_stream_destroy", st)


def _host_gmres_cycle(norm2, cols, m, iters_before, max_iterations, tol, use_relative, r0=None):
    """The reference's scalar bookkeeping of one restart cycle (subdomain.tpp:4396-4477) in Python floats."""
    import math

    H = [[0.0] * m for _ in range(m)]
    c, s, gamma = [0.0] * m, [0.0] * m, [0.0] * (m + 1)
    gamma[0] = math.sqrt(norm2)
    r0 = gamma[0] if r0 is None else r0
    hist = [gamma[0]]
    it = iters_before
    converged = False
    j = 0
    while j < m:
        it += 1
        dots = cols[j]
        for i in range(j + 1):
            H[i][j] = dots[i]
        for i in range(j):
            h = H[i][j]
            H[i][j] = c[i] * h + s[i] * H[i + 1][j]
            H[i + 1][j] = -s[i] * h + c[i] * H[i + 1][j]
        alpha = math.sqrt(dots[j + 1])
        if abs(alpha) == 0.0:
            converged = True
            break
        beta = math.sqrt(H[j][j] * H[j][j] + alpha * alpha)
        g = 1.0 / beta
        c[j] = H[j][j] * g
        s[j] = alpha * g
        H[j][j] = beta
        gamma[j + 1] = -s[j] * gamma[j]
        gamma[j] = c[j] * gamma[j]
        r = abs(gamma[j + 1])
        hist.append(r)
        if (r / r0 < tol) if use_relative else (r < tol):
            converged = True
            break
        if it >= max_iterations:
            converged = True
            break
        j += 1
    if j == m:
        j -= 1
    for k in range(j, -1, -1):
        gk = gamma[k]
        for i in range(j, k, -1):
            gk -= H[k][i] * c[i]
        c[k] = gk / H[k][k]
    return c[: j + 1], hist, j, it - iters_before, converged


@pytest.mark.parametrize("case", ["full", "tolerance", "max_iterations", "breakdown"])
def test_gmres_bookkeeping_on_device(gpu, case):
    """fdd_gmres_*_dev against the host statements they replace, bit for bit; a stop inside
    the cycle is recorded while the later steps are still fed (with garbage) and ignored."""
    L = lib.hip()
    m = 5
    rng = np.random.default_rng({"full": 1, "tolerance": 2, "max_iterations": 3, "breakdown": 4}[case])
    cols = [np.concatenate([rng.uniform(-1, 1, j + 1), [rng.uniform(0.1, 1.0)]]) for j in range(m)]
    norm2, tol, max_it, before, rel = 3.7, 1e-30, 100, 0, 0
    if case == "tolerance":
        full = _host_gmres_cycle(norm2, cols, m, 0, 100, 1e-30, True)[1]  # monotone: stop exactly at column 2
        tol, rel = 0.5 * (full[2] + full[3]) / full[0], 1
    elif case == "max_iterations":
        max_it, before = 7, 4
    elif case == "breakdown":
        cols[2][3] = 0.0
    y, hist, j_last, steps, conv = _host_gmres_cycle(norm2, cols, m, before, max_it, tol, bool(rel))
    if case != "full":
        assert j_last < m - 1 and conv

    nbytes = L.raw("fdd_gmres_state_bytes")()
    st = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=gpu)
    d_norm = dev(np.array([norm2]), gpu)
    stream = lib.current_stream()
    L.call("fdd_gmres_begin_dev", vp(st.data_ptr()), vp(d_norm.data_ptr()), 1, stream)
    keep = []
    for j in range(m):
        d = dev(cols[j] if j <= j_last or case == "full" else np.full(j + 2, np.nan), gpu)  # garbage after the stop
        keep.append(d)
        L.call("fdd_gmres_step_dev", vp(st.data_ptr()), vp(d.data_ptr()), j, before, max_it, ctypes.c_double(tol), rel, stream)
    L.call("fdd_gmres_finish_dev", vp(st.data_ptr()), m, stream)
    gy, gh = np.zeros(8), np.zeros(9)
    nh, jl, stp, cv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.call("fdd_gmres_fetch", vp(st.data_ptr()), P(gy), P(gh), ctypes.byref(nh), ctypes.byref(jl), ctypes.byref(stp), ctypes.byref(cv), stream)
    assert (jl.value, stp.value, bool(cv.value), nh.value) == (j_last, steps, conv, len(hist))
    assert np.array_equal(gh[: nh.value], np.array(hist))
    assert np.array_equal(gy[: j_last + 1], np.array(y)) and not gy[j_last + 1 :].any()
    # the coefficient pointer the update kernel reads
    yp = vp()
    L.call("fdd_gmres_coefficients", vp(st.data_ptr()), ctypes.byref(yp))
    n = 1001
    q = rnd(n, 5)
    V = [rnd(n, 10 + i) for i in range(j_last + 1)]
    ref = q.copy()
    O = S.oracle()
    for i in range(j_last + 1):
        O.orc_vector_vector_addition(P(ref), ctypes.c_double(1.0), P(ref), ctypes.c_double(y[i]), P(V[i]), n)
    dq = dev(q, gpu)
    k("fdd_multi_axpy_dev", dq, yp, [dev(v, gpu) for v in V], j_last + 1, n)
    assert np.array_equal(host(dq), ref)
    if case in ("full", "tolerance"):
        # fdd_gmres_scales / fdd_gmres_last_column: the device addresses the *_scaled and *_limited entries read, inside the
        # state; inv[0] = 1 / gamma_0, inv[j + 1] = 1 / ||q_j|| of the columns that were taken, j_last as a double
        ip, jp = vp(), vp()
        L.call("fdd_gmres_scales", vp(st.data_ptr()), ctypes.byref(ip))
        L.call("fdd_gmres_last_column", vp(st.data_ptr()), ctypes.byref(jp))
        lo, hi = st.data_ptr(), st.data_ptr() + nbytes
        assert lo <= ip.value and ip.value + 8 * (m + 1) <= hi and lo <= jp.value and jp.value + 8 <= hi
        inv, jl_dev = np.zeros(m + 1), np.zeros(1)
        L.call("fdd_fetch_scalars", P(inv), ip, 8 * (m + 1), stream)
        L.call("fdd_fetch_scalars", P(jl_dev), jp, 8, stream)
        expect = 1.0 / np.sqrt(np.array([norm2] + [cols[j][j + 1] for j in range(j_last + 1)]))
        assert np.array_equal(inv[: j_last + 2].view(np.uint64), expect.view(np.uint64))
        assert jl_dev[0] == float(jl.value) == float(j_last)


def test_fetch_scalars(gpu):
    L = lib.hip()
    a = rnd(32, 95)
    da = dev(a, gpu)
    torch.cuda.synchronize()
    out = np.zeros(32)
    L.call("fdd_fetch_scalars", P(out), vp(da.data_ptr()), 256, None)
    assert np.array_equal(out, a)
    with pytest.raises(lib.FddError):
        L.call("fdd_fetch_scalars", P(out), vp(da.data_ptr()), 8192, None)


# -------------------------------------------------------------- runtime
def test_runtime_memory_roundtrip(gpu):
    L = lib.hip()
    p = vp()
    L.call("fdd_malloc", ctypes.byref(p), 8 * 1000)
    a = rnd(1000, 130)
    b = np.zeros(1000)
    q = vp()
    L.call("fdd_malloc", ctypes.byref(q), 8 * 1000)
    L.call("fdd_memcpy_h2d", p, P(a), 8000, None)
    L.call("fdd_memcpy_d2d", q, p, 8000, None)
    L.call("fdd_device_sync")
    L.call("fdd_memcpy_d2h", P(b), q, 8000, None)
    assert np.array_equal(a, b)
    L.call("fdd_memset", q, 0, 8000, None)
    L.call("fdd_memcpy_d2h", P(b), q, 8000, None)
    assert not b.any()
    L.call("fdd_free", p)
    L.call("fdd_free", q)
    name = ctypes.create_string_buffer(128)
    L.call("fdd_device_name", name, 128)
    assert b"gfx950" in name.value


# ------------------------------------- affine elements (an option of the build)
def affine_factor_arrays(c, w, E, N, dtype=np.float64):
    """G_f(e; i, j, k) = c[e, f] * ((w_i * w_j) * w_k), associated as the kernel forms it"""
    n = N + 1
    w = w.astype(dtype)
    W = ((w[None, None, :] * w[None, :, None]) * w[:, None, None]).astype(dtype)  # [k, j, i], x fastest
    return [np.ascontiguousarray((c[:, f, None].astype(dtype) * W.reshape(1, -1)).astype(dtype).ravel()) for f in range(6)]


@pytest.mark.parametrize("N", [1, 2, 3, 5, 7, 8, 10, 15])
def test_stiffness_affine_equals_the_streamed_kernel(gpu, N):
    """fdd_stiffness_matrix_affine forms the six factors of a point from six numbers per element and the GLL weights
    instead of reading them: on factor arrays that ARE c_f(e) (w_i w_j) w_k it is the oracle's arithmetic bit for bit
    (plain and gathered with a scale, contiguous and offset-list order), and fdd_stiffness_affine_detect recognises
    such arrays and points at the one element that is not of that form."""
    n3 = (N + 1) ** 3
    w = S.gll(N)[1]
    for E in (1, 6, 41):
        rng = np.random.default_rng(900 + 7 * N + E)
        c = np.concatenate([rng.uniform(0.5, 1.5, (E, 3)), rng.uniform(-0.2, 0.2, (E, 3))], axis=1)
        G = affine_factor_arrays(c, w, E, N)
        u, _, D = stiffness_inputs(E, N, 901 + N)
        Au, _ = oracle_stiffness(u, G, D, N, 3)
        dc, dw, dD = dev(c.ravel(), gpu), dev(w, gpu), dev(D, gpu)
        out = torch.full((E * n3,), 3.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_matrix_affine", out, dev(u, gpu), None, None, dD, dc, dw, None, E, N)
        assert np.array_equal(host(out), Au), (N, E)
        # gathered through an index array with holes, scaled, elements through an offset list in reverse order
        ndof = max(1, (E * n3) // 3)
        pd = rng.integers(-1, ndof, E * n3).astype(np.int32)
        v = rng.uniform(-1, 1, ndof)
        scale = 0.37251
        ug = np.where(pd >= 0, (scale * v)[np.maximum(pd, 0)], 0.0)
        Aug, _ = oracle_stiffness(ug, G, D, N, 3)
        eo = (np.arange(E)[::-1] * n3).astype(np.int32)
        # the list's k-th element sits at eo[k]: its six numbers are those of element E-1-k of the arrays
        dcr = dev(c[::-1].ravel(), gpu)
        out2 = torch.full((E * n3,), 5.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_matrix_affine", out2, dev(v, gpu), dev(np.array([scale]), gpu), dev(pd, gpu), dD, dcr, dw, dev(eo, gpu), E, N)
        assert np.array_equal(host(out2), Aug), (N, E, "gather")
        # detection: the arrays built above pass; one factor of one point of the last element nudged by 1e-9 does not
        dG = [dev(g, gpu) for g in G]
        cd = torch.zeros(E * 6, dtype=torch.float64, device=gpu)
        dv = torch.full((E,), -1.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_affine_detect", cd, dv, dG, None, dw, E, N)
        assert host(dv).max() <= 8 * np.finfo(float).eps and np.abs(host(cd).reshape(E, 6) - c).max() <= 4 * np.finfo(float).eps * np.abs(c).max()
        G2 = [g.copy() for g in G]
        G2[0][(E - 1) * n3 + n3 - 1] *= 1.0 + 1e-9  # a diagonal factor: between a third of and the whole of the largest one
        k("fdd_stiffness_affine_detect", cd, dv, [dev(g, gpu) for g in G2], None, dw, E, N)
        d = host(dv)
        assert d[: E - 1].max(initial=0.0) <= 8 * np.finfo(float).eps and 1e-10 < d[E - 1] < 1e-8, (N, E, d)
    if N == 7:
        with pytest.raises(lib.FddError):
            k("fdd_stiffness_matrix_affine", out, dev(u, gpu), None, None, dD, dc, dw, None, E, 16)


@pytest.mark.parametrize("N", [8, 11, 14, 15])
def test_stiffness_mfma_affine(gpu, N):
    """The matrix-core kernel with the factors formed from six numbers per element (fdd_stiffness_matrix_mfma_affine):
    on factor arrays of exactly that form it is the streamed matrix-core kernel bit for bit (the same products feed
    the same matrix instructions) and the oracle to the matrix-core tolerance; plain, and gathered with a scale
    through an offset list (more elements than workgroups, so the persistent loop runs)."""
    n3 = (N + 1) ** 3
    w = S.gll(N)[1]
    for E in (1, 5, 300):
        rng = np.random.default_rng(970 + 7 * N + E)
        c = np.concatenate([rng.uniform(0.5, 1.5, (E, 3)), rng.uniform(-0.2, 0.2, (E, 3))], axis=1)
        G = affine_factor_arrays(c, w, E, N)
        u, _, D = stiffness_inputs(E, N, 971 + N)
        Au, _ = oracle_stiffness(u, G, D, N, 3)
        dc, dw, dD, dG = dev(c.ravel(), gpu), dev(w, gpu), dev(D, gpu), [dev(g, gpu) for g in G]
        ref = torch.full((E * n3,), 3.0, dtype=torch.float64, device=gpu)
        out = torch.full((E * n3,), 5.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_matrix_mfma", ref, dev(u, gpu), dD, dG, None, E, N)
        k("fdd_stiffness_matrix_mfma_affine", out, dev(u, gpu), None, None, dD, dc, dw, None, E, N)
        assert np.array_equal(host(out), host(ref)), (N, E)
        assert np.abs(host(out) - Au).max() <= 1e-12 * np.abs(Au).max()
        ndof = max(1, (E * n3) // 3)
        pd = rng.integers(-1, ndof, E * n3).astype(np.int32)
        v = rng.uniform(-1, 1, ndof)
        sc = dev(np.array([0.37251]), gpu)
        eo = (np.arange(E)[::-1] * n3).astype(np.int32)
        ref2 = torch.full((E * n3,), 3.0, dtype=torch.float64, device=gpu)
        out2 = torch.full((E * n3,), 5.0, dtype=torch.float64, device=gpu)
        k("fdd_stiffness_matrix_mfma_gather", ref2, dev(v, gpu), sc, dev(pd, gpu), dD, dG, dev(eo, gpu), E, N)
        k("fdd_stiffness_matrix_mfma_affine", out2, dev(v, gpu), sc, dev(pd, gpu), dD, dev(c[::-1].ravel(), gpu), dw, dev(eo, gpu), E, N)
        assert np.array_equal(host(out2), host(ref2)), (N, E, "gather")


@pytest.mark.parametrize("n", [1, 7, 4097, 1_000_001])
def test_flexible_dot_with_the_next_gamma(gpu, n):
    """fdd_dom_inner_product_flexible_gamma = {<z, r+>, <r+ - r, z>} from one pass over the three vectors: the same bits
    as the flexible dot and as the first sum of the projection kernel on (z, r+)."""
    ws = reduce_workspace(gpu)
    r, r1, z = dev(rnd(n, 1), gpu), dev(rnd(n, 2), gpu), dev(rnd(n, 3), gpu)
    out2 = torch.zeros(2, dtype=torch.float64, device=gpu)
    flex = torch.zeros(1, dtype=torch.float64, device=gpu)
    proj = torch.zeros(2, dtype=torch.float64, device=gpu)
    k("fdd_dom_inner_product_flexible_gamma", out2, ws, r, r1, z, n)
    k("fdd_dom_inner_product_flexible", flex, ws, r, r1, z, n)
    k("fdd_dom_projection_inner_products", proj, ws, z, r1, z, r1, n)
    assert host(out2)[1] == host(flex)[0] and host(out2)[0] == host(proj)[0]


# ------------------------------------------------------------------ the interface exchange's kernels (gs_add on the boundary prefix, domain.tpp:590-594)
@pytest.mark.parametrize("nb,peers", [(1, 1), (37, 2), (5000, 3), (152000, 7)])
def test_interface_exchange_kernels(gpu, nb, peers):
    """Both forms of gs(gs_add) on a rank's boundary prefix.  Dense form: pack into / unpack from the interface-slot vector.
    Neighbour form: gather (own copies + the parts each sharing rank gets, one or two interleaved vectors), and after the
    exchange the sum of every node's copies IN THE ORDER ITS ROW LISTS THEM (ascending rank: all sharers must form the same
    bits) -- against plain numpy loops of the same statements, bit for bit."""
    rng = np.random.default_rng(1000 + nb)
    a, b = rnd(nb + 13, 1), rnd(nb + 13, 2)
    # dense form
    slots_n = 3 * nb + 5
    slot_of = rng.permutation(slots_n)[:nb].astype(np.int32)
    slots = torch.zeros(slots_n, dtype=torch.float64, device=gpu)
    k("fdd_interface_pack", slots, dev(slot_of, gpu), dev(a, gpu), nb)
    ref = np.zeros(slots_n)
    ref[slot_of] = a[:nb]
    assert np.array_equal(host(slots), ref)
    back = torch.full((nb,), 9.0, dtype=torch.float64, device=gpu)
    k("fdd_interface_unpack", back, slots, dev(slot_of, gpu), nb)
    assert np.array_equal(host(back), a[:nb])
    # neighbour form: every peer shares a random subset of the prefix
    shared = [np.sort(rng.choice(nb, size=max(1, nb // (p + 2)), replace=False)).astype(np.int32) for p in range(peers)]
    index = np.concatenate([np.arange(nb, dtype=np.int32)] + shared)
    total = sum(len(x) for x in shared)
    first = np.cumsum([0] + [len(x) for x in shared])
    me = peers // 2  # this rank's place among the sharers: peers 0..me-1 come before it, the rest after
    ptr, col = [0], []
    for node in range(nb):
        for p in range(peers + 1):
            if p == me:
                col.append(node)
                continue
            q = p if p < me else p - 1
            pos = np.searchsorted(shared[q], node)
            if pos < len(shared[q]) and shared[q][pos] == node:
                col.append(nb + total + first[q] + pos)
        ptr.append(len(col))
    ptr, col = np.array(ptr, np.int32), np.array(col, np.int32)
    for nc in (1, 2):
        buf = torch.full((nc * (nb + 2 * total),), -7.0, dtype=torch.float64, device=gpu)
        k("fdd_interface_gather", buf, dev(index, gpu), nb + total, dev(a, gpu), dev(b, gpu) if nc == 2 else None)
        got = host(buf).copy()
        want = np.full(nc * (nb + 2 * total), -7.0)
        want[0:nc * (nb + total):nc] = a[index]
        if nc == 2:
            want[1:nc * (nb + total):nc] = b[index]
        assert np.array_equal(got, want), nc
        recv = rnd(nc * total, 30 + nc)  # what the peers would have sent
        want[nc * (nb + total):] = recv
        buf = dev(want, gpu)
        oa, ob = dev(a, gpu).clone(), dev(b, gpu).clone()
        k("fdd_interface_sum", oa, ob if nc == 2 else None, dev(ptr, gpu), dev(col, gpu), nb, buf)
        ra, rb = a.copy(), b.copy()
        for node in range(nb):
            sa = sb = 0.0
            for c in col[ptr[node]:ptr[node + 1]]:
                sa += want[c * nc]
                if nc == 2:
                    sb += want[c * nc + 1]
            ra[node] = sa
            if nc == 2:
                rb[node] = sb
        assert np.array_equal(host(oa), ra), nc  # entries past the prefix untouched
        if nc == 2:
            assert np.array_equal(host(ob), rb)
