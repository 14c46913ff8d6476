"""The persistent kernels past the first trip of every workgroup.

Several hot-path kernels run a capped grid: a workgroup walks a list of elements or row blocks and carries state from one
trip to the next (values prefetched one element ahead, indices two ahead, descriptors two blocks ahead, LDS buffers reused
behind a wave-level or a single workgroup barrier).  The kernel-level tests of the other files stop before that loop goes
round more than once; here every size is past its cap often enough that the steady state runs, and each part asserts that
precondition itself, so that a later change of a cap makes the test fail and not go quiet:

  1. the matrix-core stiffness kernel (csrc/fdd_stiffness_mfma.hip, grid min(E, 256)) at E = 3 * 256 + 37: three and four
     trips per workgroup; every entry against the oracle's two-kernel arithmetic (1e-12 * max|Au|, the bar of the existing
     matrix-core tests) AND, bit for bit, against the same entry launched on the same list in chunks of at most 256
     elements -- one trip per workgroup, the path the other files cover;
  2. the short-row CSR kernel (csr_short_pipelined_kernel, csrc/fdd_csr.hip, grid min(4 * 256, blocks)) on a plan of more
     than 3 * 1024 row blocks, every instance with an epilogue, in both precisions, bit for bit against the oracle entries
     the small-plan tests use; row ranges whose ends lie in blocks of different trips; the gather-norm reduction past its
     grid cap of 2048;
  3. the restriction kernels (csrc/fdd_restrict.hip): every compiled pair of the wave form and two that take the generic
     instance at E = 53, and each form past its cap, bit for bit against the oracle's three launches.

Guard words stand in front of every output, behind it and in its gaps, and the data differs from element to element (row to
row), so that an element served from another's registers cannot pass.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import support as S
from support import GUARD, Plan, boolean_gather_matrix, guarded, guards_stand, row_sums_in_column_order
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k, reduce_workspace

pytestmark = pytest.mark.gpu

P = S._p
c_double = ctypes.c_double

# FDD_CU_COUNT of csrc/fdd_common.h: the compute units of an MI355X.  Every cap below is a multiple of it.
CU_COUNT = 256


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------------------------------------------------------------
# 1. matrix-core stiffness
# ------------------------------------------------------------------------------------------------------------------------
# grid = min(E, 256) workgroups of one element each per trip; with the grid / 8 window order 37 workgroups take four trips
# and the others three, and the first index prefetch of every workgroup (element e + 256) names a real element
MFMA_GRID = CU_COUNT
E_STEADY = 3 * MFMA_GRID + 37
DEVICE_BYTES_LIMIT = 0.5e9  # a case whose device copy would be larger drops its 2E-vector variant


class ElementList:
    """E elements of n3 points in list order, stored either one after the other (elem_offset NULL) or in shuffled slots of a
    vector of 2E elements (an offset list with gaps)."""

    def __init__(self, E, n3, spread, seed):
        self.E, self.n3, self.spread = E, n3, spread
        self.nslots = 2 * E if spread else E
        self.slots = np.random.default_rng(seed).permutation(self.nslots)[:E] if spread else np.arange(E)
        self.offsets = (self.slots * n3).astype(np.int32)
        if spread:
            assert (np.diff(self.slots) < 0).any() and len(np.unique(self.slots)) == E

    def place(self, a, fill):
        """the list-ordered array in the vector's layout; the slots of no element hold `fill`"""
        if not self.spread:
            return a
        whole = np.full((self.nslots, self.n3), fill, a.dtype)
        whole[self.slots] = a.reshape(self.E, self.n3)
        return whole.ravel()

    def output(self, gpu):
        whole = torch.full((self.nslots * self.n3 + 16,), GUARD, dtype=torch.float64, device=gpu)
        return whole, whole[8:-8]

    def collect(self, whole, what):
        """the outputs in list order; guard words in front, behind and in the slots of no element"""
        torch.cuda.synchronize()
        h = whole.cpu().numpy()
        assert (h[:8] == GUARD).all() and (h[-8:] == GUARD).all(), (what, "guard words around the output")
        body = h[8:-8].reshape(self.nslots, self.n3)
        unused = np.ones(self.nslots, bool)
        unused[self.slots] = False
        assert (body[unused] == GUARD).all(), (what, "elements that are not in the list were written")
        return body[self.slots].ravel()


def stiffness_data(E, N, seed, diag=False, affine=False):
    """u, the six factor arrays (list order, different at every point) and D.  diag: arrays 3..5 all 0.0; affine: the arrays
    are c_f(e) (w_i w_j) w_k with six numbers per element that differ from element to element."""
    n3 = (N + 1) ** 3
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.0, 1.0, E * n3)
    c = None
    if affine:
        c = np.concatenate([rng.uniform(0.5, 1.5, (E, 3)), rng.uniform(-0.2, 0.2, (E, 3))], axis=1)
        w = S.gll(N)[1]
        W = ((w[None, None, :] * w[None, :, None]) * w[:, None, None]).reshape(1, -1)  # [k, j, i], x fastest: (w_i w_j) w_k
        G = [np.ascontiguousarray((c[:, f, None] * W).ravel()) for f in range(6)]
    elif diag:
        G = [rng.uniform(0.5, 1.5, E * n3) if g < 3 else np.zeros(E * n3) for g in range(6)]
    else:
        G = [rng.uniform(0.1, 1.0, E * n3) if g < 3 else rng.uniform(-0.3, 0.3, E * n3) for g in range(6)]
    return u, G, np.ascontiguousarray(S.gll(N)[2]), c


def gather_data(E, N, seed):
    """v on about half as many dofs as there are points, and a point -> dof array with about a third of its entries -1"""
    n3 = (N + 1) ** 3
    rng = np.random.default_rng(seed)
    ndof = (E * n3) // 2
    pd = rng.integers(0, ndof, E * n3).astype(np.int32)
    pd[rng.random(E * n3) < 1.0 / 3.0] = -1
    assert 0.3 < (pd < 0).mean() < 0.37
    return rng.uniform(-1.0, 1.0, ndof), pd


def gathered(v, pd, scale):
    """u[p] = scale * v[pd[p]], 0 where the point has no dof: the products the kernel forms on load"""
    return np.where(pd >= 0, (v if scale is None else scale * v)[np.maximum(pd, 0)], 0.0)


def launch_mfma(entry, N, out, vec, scale, pd, D, G, eo, count, factors=None, weights=None):
    if entry == "fdd_stiffness_matrix_mfma":
        k(entry, out, vec, D, G, eo, count, N)
    elif entry == "fdd_stiffness_matrix_mfma_affine":
        k(entry, out, vec, scale, pd, D, factors, weights, eo, count, N)
    else:  # _gather, _diag
        k(entry, out, vec, scale, pd, D, G, eo, count, N)


def steady_state_case(gpu, entry, N, elements, Au, vec, scale, pd, D, G, factors=None, weights=None):
    """One launch over the whole list against (a) the oracle's Au (list order) and (b) the same entry on the same list in
    chunks of at most MFMA_GRID elements, as bits.  Returns the ratio of (a)."""
    E = elements.E
    assert E > 3 * MFMA_GRID and E % MFMA_GRID != 0, "every workgroup must take a third element, some a fourth"
    what = (entry, N, "offset list" if elements.spread else "contiguous", "gather" if pd is not None else "local", "scale" if scale is not None else "no scale")
    deo = dev(elements.offsets, gpu)
    whole, out = elements.output(gpu)
    launch_mfma(entry, N, out, vec, scale, pd, D, G, deo if elements.spread else None, E, factors, weights)
    got = elements.collect(whole, what)
    whole2, out2 = elements.output(gpu)
    for first in range(0, E, MFMA_GRID):
        count = min(MFMA_GRID, E - first)
        launch_mfma(entry, N, out2, vec, scale, pd, D, G, deo[first : first + count], count, None if factors is None else factors[6 * first : 6 * (first + count)], weights)
    chunked = elements.collect(whole2, what + ("in chunks",))
    ratio = np.abs(got - Au).max() / np.abs(Au).max()
    print("%s: max|Au - oracle| / max|Au| = %.3e" % (" ".join(str(w) for w in what), ratio))
    assert np.abs(Au).max() > 0.0 and np.isfinite(got).all()
    differing = np.nonzero((bits(got) != bits(chunked)).reshape(E, -1).any(axis=1))[0]
    assert len(differing) == 0, (what, "list positions whose bits depend on the trip they are computed in", differing[:20], "oracle ratio %.3e" % ratio)
    assert ratio <= 1e-12, (what, "against the oracle: %.3e" % ratio)
    return ratio


def layouts(N, arrays):
    """contiguous, and the shuffled offset list over 2E elements where its device copy stays under the limit"""
    n3 = (N + 1) ** 3
    spread_bytes = arrays * 2 * E_STEADY * n3 * 8
    return [False, True] if spread_bytes <= DEVICE_BYTES_LIMIT else [False]


@pytest.mark.parametrize("N", [8, 15])
def test_mfma_local_steady_state(gpu, N):
    """fdd_stiffness_matrix_mfma: elem_offset NULL, and a shuffled offset list with gaps over a vector of 2E elements"""
    n3 = (N + 1) ** 3
    u, G, D, _ = stiffness_data(E_STEADY, N, 7100 + N)
    Au, _ = S.oracle_stiffness(u, G, D, N, 3)
    dD = dev(D, gpu)
    for spread in layouts(N, arrays=6 + 1 + 2):
        elements = ElementList(E_STEADY, n3, spread, 7200 + N)
        du = dev(elements.place(u, np.nan), gpu)
        dG = [dev(elements.place(g, np.nan), gpu) for g in G]
        steady_state_case(gpu, "fdd_stiffness_matrix_mfma", N, elements, Au, du, None, None, dD, dG)
        del du, dG


@pytest.mark.parametrize("N", [8, 11, 15])
def test_mfma_gather_steady_state(gpu, N):
    """fdd_stiffness_matrix_mfma_gather, scale NULL and given: the dof indices run two elements ahead of the element that is
    computed, so from the second trip on every index register has been refilled inside the loop"""
    n3 = (N + 1) ** 3
    _, G, D, _ = stiffness_data(E_STEADY, N, 7300 + N)
    v, pd = gather_data(E_STEADY, N, 7400 + N)
    dD, dv = dev(D, gpu), dev(v, gpu)
    for spread in layouts(N, arrays=6 + 1 + 2 + 1):
        elements = ElementList(E_STEADY, n3, spread, 7500 + N)
        dG = [dev(elements.place(g, np.nan), gpu) for g in G]
        dpd = dev(elements.place(pd, -1), gpu)
        for scale in (None, 0.37251):
            Au, _ = S.oracle_stiffness(gathered(v, pd, scale), G, D, N, 3)
            steady_state_case(gpu, "fdd_stiffness_matrix_mfma_gather", N, elements, Au, dv, None if scale is None else dev(np.array([scale]), gpu), dpd, dD, dG)
        del dG, dpd


@pytest.mark.parametrize("N", [8, 11])
def test_mfma_diag_steady_state(gpu, N):
    """fdd_stiffness_matrix_mfma_diag, local and gather form, G[3..5] NULL; the oracle runs on the six arrays the form stands
    for (3..5 all 0.0).  N = 11 is the lowest degree the host layer sends to the matrix cores."""
    n3 = (N + 1) ** 3
    u, G, D, _ = stiffness_data(E_STEADY, N, 7600 + N, diag=True)
    v, pd = gather_data(E_STEADY, N, 7700 + N)
    Au_local, _ = S.oracle_stiffness(u, G, D, N, 3)
    Au_gather, _ = S.oracle_stiffness(gathered(v, pd, 0.37251), G, D, N, 3)
    dD, dv, dscale = dev(D, gpu), dev(v, gpu), dev(np.array([0.37251]), gpu)
    for spread in layouts(N, arrays=3 + 1 + 2 + 1):
        elements = ElementList(E_STEADY, n3, spread, 7800 + N)
        dG = [dev(elements.place(g, np.nan), gpu) for g in G[:3]] + [None, None, None]
        steady_state_case(gpu, "fdd_stiffness_matrix_mfma_diag", N, elements, Au_local, dev(elements.place(u, np.nan), gpu), None, None, dD, dG)
        steady_state_case(gpu, "fdd_stiffness_matrix_mfma_diag", N, elements, Au_gather, dv, dscale, dev(elements.place(pd, -1), gpu), dD, dG)


def test_mfma_affine_steady_state(gpu):
    """fdd_stiffness_matrix_mfma_affine at N = 8, local and gather form: the six numbers of an element are read by list
    position in every trip (the chunks take slices of elem_factors); the oracle runs on the arrays c_f(e) (w_i w_j) w_k"""
    N = 8
    n3 = (N + 1) ** 3
    u, G, D, c = stiffness_data(E_STEADY, N, 7900, affine=True)
    assert len(np.unique(c[:, 0])) == E_STEADY
    v, pd = gather_data(E_STEADY, N, 7901)
    Au_local, _ = S.oracle_stiffness(u, G, D, N, 3)
    Au_gather, _ = S.oracle_stiffness(gathered(v, pd, 0.37251), G, D, N, 3)
    dD, dv, dscale, dc, dw = dev(D, gpu), dev(v, gpu), dev(np.array([0.37251]), gpu), dev(c.ravel(), gpu), dev(S.gll(N)[1], gpu)
    for spread in (False, True):
        elements = ElementList(E_STEADY, n3, spread, 7902)
        steady_state_case(gpu, "fdd_stiffness_matrix_mfma_affine", N, elements, Au_local, dev(elements.place(u, np.nan), gpu), None, None, dD, None, dc, dw)
        steady_state_case(gpu, "fdd_stiffness_matrix_mfma_affine", N, elements, Au_gather, dv, dscale, dev(elements.place(pd, -1), gpu), dD, None, dc, dw)


@pytest.mark.parametrize("E", [5, 300])
@pytest.mark.parametrize("N", [10, 13])
def test_mfma_local_six_arrays_at_the_degrees_never_run(gpu, N, E):
    """the n = 11 and n = 14 instances of the local six-array form, which no other kernel-level test launches"""
    n3 = (N + 1) ** 3
    u, G, D, _ = stiffness_data(E, N, 8000 + 10 * N + E)
    Au, _ = S.oracle_stiffness(u, G, D, N, 3)
    elements = ElementList(E, n3, False, 0)
    whole, out = elements.output(gpu)
    k("fdd_stiffness_matrix_mfma", out, dev(u, gpu), dev(D, gpu), [dev(g, gpu) for g in G], None, E, N)
    got = elements.collect(whole, (N, E))
    ratio = np.abs(got - Au).max() / np.abs(Au).max()
    print("fdd_stiffness_matrix_mfma N=%d E=%d: max|Au - oracle| / max|Au| = %.3e" % (N, E, ratio))
    assert np.abs(Au).max() > 0.0 and ratio <= 1e-12, (N, E, "against the oracle: %.3e" % ratio)


# ------------------------------------------------------------------------------------------------------------------------
# 2. short-row CSR kernel with epilogues
# ------------------------------------------------------------------------------------------------------------------------
# min(4 * 256, blocks) workgroups take the row blocks b, b + 1024, ... with three blocks in flight
PIPELINED_WORKGROUPS = 4 * CU_COUNT
REDUCE_MAX_BLOCKS = 2048  # FDD_REDUCE_MAX_BLOCKS of include/fdd_hip.h: the grid cap of gather_norm2_block_kernel
SHORT_BLOCK_NNZ = 1024    # FDD_CSR_BLOCK_NNZ / 2: entries, and rows, a short-row block holds at most
CSR_ROWS = 2_000_000


def short_row_blocks(ptr):
    """the row blocks plan_create cuts a short-row matrix into (no row longer than a block): as many rows as fit into
    SHORT_BLOCK_NNZ entries and SHORT_BLOCK_NNZ rows.  One step per block."""
    rows = len(ptr) - 1
    starts = [0]
    while starts[-1] < rows:
        r = starts[-1]
        e = min(r + SHORT_BLOCK_NNZ, int(np.searchsorted(ptr, ptr[r] + SHORT_BLOCK_NNZ, side="right")) - 1)
        assert e > r
        starts.append(e)
    return np.array(starts)


@pytest.fixture(scope="module")
def csr(gpu):
    """one boolean-gather-shaped matrix of more than 3 * 1024 row blocks, its device arrays and a plan of either precision
    with random values and with unit values; no sliced-ELL copy is attached.  Made once and left unchanged."""
    ptr, col, cols = boolean_gather_matrix(CSR_ROWS, CSR_ROWS)
    rng = np.random.default_rng(CSR_ROWS + 1)
    m = types.SimpleNamespace(ptr=ptr, col=col, rows=CSR_ROWS, cols=cols, nnz=len(col))
    m.val = rng.uniform(-1.0, 1.0, m.nnz)
    m.val32 = rng.uniform(-1.0, 1.0, m.nnz).astype(np.float32)
    m.ones, m.ones32 = np.ones(m.nnz), np.ones(m.nnz, np.float32)
    m.x, m.y0, m.f, m.Sr, m.u0, m.weight = (rng.uniform(-1.0, 1.0, n) for n in (cols, CSR_ROWS, CSR_ROWS, CSR_ROWS, CSR_ROWS, CSR_ROWS))
    m.D = rng.uniform(0.5, 1.5, CSR_ROWS)
    m.dptr, m.dcol, m.dval, m.dval32, m.dones32 = (dev(a, gpu) for a in (ptr, col, m.val, m.val32, m.ones32))
    m.blocks = short_row_blocks(ptr)
    m.plans = {(f32, unit): Plan(ptr, cols, f32=f32, unit=unit) for f32 in (False, True) for unit in (False, True)}
    try:
        for plan in m.plans.values():
            nb = plan.query("num_blocks")
            assert nb > 3 * PIPELINED_WORKGROUPS and nb % PIPELINED_WORKGROUPS != 0 and nb > REDUCE_MAX_BLOCKS, nb
            assert nb == len(m.blocks) - 1, (nb, len(m.blocks) - 1)
            assert plan.query("kind") == 1 and plan.query("pipelined") == 1
        yield m
    finally:
        torch.cuda.synchronize()
        for plan in m.plans.values():
            plan.close()


def values_of(m, values, f32=False):
    """(the plan, the device value array handed to the entry, the host values of the reference)"""
    unit = values == "unit"
    if f32:  # the f32 entries may read the 1.0 values of a unit-value plan (include/fdd_hip.h)
        return m.plans[(True, unit)], (m.dones32 if unit else m.dval32), (m.ones32 if unit else m.val32)
    return m.plans[(False, unit)], (None if unit else m.dval), (m.ones if unit else m.val)


def check_output(whole, part, ref, what):
    torch.cuda.synchronize()
    got = part.cpu().numpy()
    differing = np.nonzero(bits(got) != bits(ref))[0]
    assert len(differing) == 0, (what, "rows that differ", differing[:20], len(differing))
    assert guards_stand(whole), (what, "guard words")


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weight"])
@pytest.mark.parametrize("values", ["random", "unit"])
def test_csr_plan_multiply_steady_state(gpu, csr, values, weighted):
    """fdd_csr_plan_multiply, weight NULL and given, random values and unit values with A_val NULL, against
    orc_csr_multiply[_weight] as bits"""
    m = csr
    plan, dval, val = values_of(m, values)
    L = S.oracle()
    ref = np.zeros(m.rows)
    if weighted:
        L.orc_csr_multiply_weight(P(ref), P(m.ptr), P(m.col), P(val), P(m.x), P(m.weight), m.rows)
    else:
        L.orc_csr_multiply(P(ref), P(m.ptr), P(m.col), P(val), P(m.x), m.rows)
    assert np.abs(ref).max() > 0.0
    whole, out = guarded(np.full(m.rows, GUARD), torch.float64, gpu)
    k("fdd_csr_plan_multiply", plan.h, out, m.dptr, m.dcol, dval, dev(m.x, gpu), dev(m.weight, gpu) if weighted else None)
    check_output(whole, out, ref, (values, weighted))


@pytest.mark.parametrize("values", ["random", "unit"])
def test_csr_plan_matvec_steady_state(gpu, csr, values):
    """fdd_csr_plan_matvec and _matvec_to (y_in NULL, y_in a separate vector) for three (alpha, beta), against orc_amg_matvec
    as bits; beta = 0 reads neither y nor y_in (NaN in, numbers out); y_in is left as it was"""
    m = csr
    plan, dval, val = values_of(m, values)
    L = S.oracle()
    dx = dev(m.x, gpu)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)):
        ref = m.y0.copy()
        L.orc_amg_matvec(P(ref), P(m.ptr), P(m.col), P(val), P(m.x), c_double(alpha), c_double(beta), m.rows)
        start = np.full(m.rows, np.nan) if beta == 0.0 else m.y0
        whole, y = guarded(start, torch.float64, gpu)
        k("fdd_csr_plan_matvec", plan.h, y, m.dptr, m.dcol, dval, dx, alpha, beta)
        check_output(whole, y, ref, (values, alpha, beta, "matvec"))
        whole, y = guarded(start, torch.float64, gpu)
        k("fdd_csr_plan_matvec_to", plan.h, y, None, m.dptr, m.dcol, dval, dx, alpha, beta)
        check_output(whole, y, ref, (values, alpha, beta, "matvec_to, y_in NULL"))
        whole, y = guarded(np.full(m.rows, np.nan), torch.float64, gpu)
        whole_in, y_in = guarded(start, torch.float64, gpu)
        k("fdd_csr_plan_matvec_to", plan.h, y, y_in, m.dptr, m.dcol, dval, dx, alpha, beta)
        check_output(whole, y, ref, (values, alpha, beta, "matvec_to, y_in separate"))
        assert np.array_equal(bits(y_in.cpu().numpy()), bits(start)) and guards_stand(whole_in)


@pytest.mark.parametrize("values", ["random", "unit"])
def test_amg_smoother_entries_steady_state(gpu, csr, values):
    """the four fused smoother entries against the oracle's unfused sequence matvec -> scaled_residual /
    polynomial_evaluation / update_field -> vector_multiplication, as bits (the pipelined kernel sums a row in column
    order); their operands f, Sr, D_val, u are the ones loaded one row block ahead"""
    m = csr
    plan, dval, val = values_of(m, values)
    L = S.oracle()
    n, coef = m.rows, -0.37
    dx, dD, df, dSr_in = (dev(a, gpu) for a in (m.x, m.D, m.f, m.Sr))
    nan = np.full(n, np.nan)
    # residual: work = f - A x; Sr = D*work, w = coef*Sr; out = D*w
    work = m.f.copy()
    L.orc_amg_matvec(P(work), P(m.ptr), P(m.col), P(val), P(m.x), c_double(-1.0), c_double(1.0), n)
    Sr, w, out = np.zeros(n), np.zeros(n), np.zeros(n)
    L.orc_amg_main_scaled_residual(P(Sr), P(w), P(work), P(m.D), c_double(coef), n)
    L.orc_amg_vector_multiplication(P(out), P(m.D), P(w), n)
    (Wwork, dwork), (WSr, dSr) = guarded(nan, torch.float64, gpu), guarded(nan, torch.float64, gpu)
    k("fdd_amg_smooth_residual_matvec", plan.h, dwork, dSr, m.dptr, m.dcol, dval, dx, df, dD, coef)
    check_output(WSr, dSr, Sr, (values, "residual: Sr"))
    check_output(Wwork, dwork, out, (values, "residual: work"))
    # polynomial: v = A x; v *= D; w = coef*Sr + v; out = D*w
    v = np.zeros(n)
    L.orc_amg_matvec(P(v), P(m.ptr), P(m.col), P(val), P(m.x), c_double(1.0), c_double(0.0), n)
    w1, out1 = np.zeros(n), np.zeros(n)
    L.orc_amg_main_polynomial_evaluation(P(w1), P(v), P(m.Sr), P(m.D), c_double(coef), n)
    L.orc_amg_vector_multiplication(P(out1), P(m.D), P(w1), n)
    Wout, dout = guarded(nan, torch.float64, gpu)
    k("fdd_amg_smooth_polynomial_matvec", plan.h, dout, m.dptr, m.dcol, dval, dx, dSr_in, dD, coef)
    check_output(Wout, dout, out1, (values, "polynomial"))
    # update: the same w, then u += D*w, in place
    u2 = m.u0.copy()
    L.orc_amg_main_update_field(P(u2), P(w1), P(m.D), n)
    Wu, du = guarded(m.u0, torch.float64, gpu)
    k("fdd_amg_smooth_update_matvec", plan.h, du, m.dptr, m.dcol, dval, dx, dSr_in, dD, coef)
    check_output(Wu, du, u2, (values, "update"))
    # the same from u = 0: u is written, not read
    uz = np.zeros(n)
    L.orc_amg_main_update_field(P(uz), P(w1), P(m.D), n)
    Wz, dz = guarded(nan, torch.float64, gpu)
    k("fdd_amg_smooth_update_matvec_from_zero", plan.h, dz, m.dptr, m.dcol, dval, dx, dSr_in, dD, coef)
    check_output(Wz, dz, uz, (values, "update from zero"))
    assert np.abs(out).max() > 0.0 and np.abs(out1).max() > 0.0 and not np.array_equal(u2, m.u0)


def row_sums_of_products_f32(ptr, col, val, x):
    """s = 0; s += val[j] * x[col[j]] entry after entry, every product and every sum rounded to IEEE single"""
    s = np.zeros(len(ptr) - 1, np.float32)
    length = np.diff(ptr)
    for j in range(int(length.max())):
        on = length > j
        at = ptr[:-1][on] + j
        s[on] = s[on] + val[at] * x[col[at]]
    assert s.dtype == np.float32
    return s


@pytest.mark.parametrize("values", ["random", "unit"])
def test_f32_entries_steady_state(gpu, csr, values):
    """fdd_csr_plan_matvec_to_f32 and the four _f32 smoother entries against the IEEE-single restatement of
    test_f32_spmv_and_fused_smoother (numpy float32, products added in column order, no contraction), as bits"""
    m = csr
    f32 = np.float32
    plan, dval, val = values_of(m, values, f32=True)
    n = m.rows
    x, yin, fv, Sr_in, u0, D = (a.astype(f32) for a in (m.x, m.y0, m.f, m.Sr, m.u0, m.D))
    coef, alpha, beta = f32(-0.37), f32(0.75), f32(-1.25)
    Ax = row_sums_of_products_f32(m.ptr, m.col, val, x)
    assert np.abs(Ax).max() > 0.0
    dx, dD, dSr_in = dev(x, gpu), dev(D, gpu), dev(Sr_in, gpu)
    nan = np.full(n, np.nan, f32)
    # y = alpha*A*x + beta*y_in; beta = 0 never reads y
    W, y = guarded(nan, torch.float32, gpu)
    k("fdd_csr_plan_matvec_to_f32", plan.h, y, dev(yin, gpu), m.dptr, m.dcol, dval, dx, float(alpha), float(beta))
    check_output(W, y, alpha * Ax + beta * yin, (values, "matvec_to_f32"))
    W, y = guarded(nan, torch.float32, gpu)
    k("fdd_csr_plan_matvec_to_f32", plan.h, y, None, m.dptr, m.dcol, dval, dx, float(alpha), 0.0)
    check_output(W, y, alpha * Ax, (values, "matvec_to_f32, beta = 0"))
    W, y = guarded(yin, torch.float32, gpu)
    k("fdd_csr_plan_matvec_to_f32", plan.h, y, None, m.dptr, m.dcol, dval, dx, float(alpha), float(beta))
    check_output(W, y, alpha * Ax + beta * yin, (values, "matvec_to_f32 in place"))
    # residual: work = -A x + f; Sr = D*work; w = coef*Sr; out = w*D
    work = f32(-1) * Ax + f32(1) * fv
    Sr = D * work
    out = (coef * Sr) * D
    (Wwork, dwork), (WSr, dSr) = guarded(nan, torch.float32, gpu), guarded(nan, torch.float32, gpu)
    k("fdd_amg_smooth_residual_matvec_f32", plan.h, dwork, dSr, m.dptr, m.dcol, dval, dx, dev(fv, gpu), dD, float(coef))
    check_output(WSr, dSr, Sr, (values, "residual_f32: Sr"))
    check_output(Wwork, dwork, out, (values, "residual_f32: work"))
    # polynomial / update: v = (A x)*D; w = coef*Sr + v; out = w*D | u += D*w | u = 0 + D*w
    v = (f32(1) * Ax) * D
    w = coef * Sr_in + v
    Wout, dout = guarded(nan, torch.float32, gpu)
    k("fdd_amg_smooth_polynomial_matvec_f32", plan.h, dout, m.dptr, m.dcol, dval, dx, dSr_in, dD, float(coef))
    check_output(Wout, dout, w * D, (values, "polynomial_f32"))
    Wu, du = guarded(u0, torch.float32, gpu)
    k("fdd_amg_smooth_update_matvec_f32", plan.h, du, m.dptr, m.dcol, dval, dx, dSr_in, dD, float(coef))
    check_output(Wu, du, u0 + D * w, (values, "update_f32"))
    Wz, dz = guarded(nan, torch.float32, gpu)
    k("fdd_amg_smooth_update_matvec_from_zero_f32", plan.h, dz, m.dptr, m.dcol, dval, dx, dSr_in, dD, float(coef))
    check_output(Wz, dz, f32(0) + D * w, (values, "update_from_zero_f32"))
    for a in (work, Sr, out, v, w):
        assert a.dtype == f32


def test_row_ranges_across_trips(gpu, csr):
    """fdd_csr_plan_dssum mode 1 and fdd_csr_plan_gather_f32 on row ranges whose two ends lie inside row blocks of
    different trips of the persistent kernel: the rows of the range are the sums in column order, as bits, and every other
    row keeps the guard value"""
    m = csr
    G = PIPELINED_WORKGROUPS
    inside = lambda b: int((m.blocks[b] + m.blocks[b + 1]) // 2)
    ranges = [(inside(5), inside(2 * G + 9)), (inside(G + 1), m.rows), (inside(7), inside(G + 7)), (inside(3 * G + 2), inside(3 * G + 2) + 1)]
    plan = m.plans[(False, True)]
    for dtype, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        u = m.x.astype(npdt)
        du = dev(u, gpu)
        sums = row_sums_in_column_order(m.ptr, m.col, u)
        assert sums.dtype == npdt and np.abs(sums).max() > 0.0
        for lo, hi in ranges:
            b_lo, b_hi = (int(np.searchsorted(m.blocks, r, side="right")) - 1 for r in (lo, hi - 1))
            assert m.blocks[b_lo] < lo < m.blocks[b_lo + 1], "the range starts inside a block"
            assert hi == m.rows or m.blocks[b_hi] < hi < m.blocks[b_hi + 1], "the range ends inside a block"
            if hi - lo > 1:
                assert (b_hi - b_lo) // G >= 1, "the ends lie in blocks of different trips"
            whole, t = guarded(np.full(m.rows, GUARD, npdt), dtype, gpu)
            if dtype == torch.float64:
                k("fdd_csr_plan_dssum", plan.h, None, t, m.dptr, m.dcol, du, None, None, lo, hi, 1)
            else:
                k("fdd_csr_plan_gather_f32", plan.h, t, m.dptr, m.dcol, du, lo, hi)
            expect = np.full(m.rows, GUARD, npdt)
            expect[lo:hi] = sums[lo:hi]
            check_output(whole, t, expect, (str(npdt), lo, hi))


def test_gather_weighted_norm2_past_the_grid_cap(gpu, csr):
    """fdd_csr_plan_gather_weighted_norm2 on more row blocks than gather_norm2_block_kernel has workgroups (its LDS is reused
    from trip to trip) against fdd_gather_weighted_norm2 and against the sum of the same terms in numpy.longdouble, to the
    1e-13 of test_gather_weighted_norm2; two calls give the same bits"""
    m = csr
    plan = m.plans[(False, True)]
    assert plan.query("num_blocks") > REDUCE_MAX_BLOCKS
    w = np.random.default_rng(77).uniform(0.25, 1.0, m.rows)
    s = row_sums_in_column_order(m.ptr, m.col, m.x) * w
    ref = float(np.sum((s * s * w).astype(np.longdouble)))
    assert ref > 0.0
    ws = reduce_workspace(gpu)
    du, dw = dev(m.x, gpu), dev(w, gpu)
    results = []
    for entry in ("plan", "plan", "rows"):
        whole = torch.full((3,), GUARD, dtype=torch.float64, device=gpu)
        if entry == "plan":
            k("fdd_csr_plan_gather_weighted_norm2", plan.h, whole[1:2], ws, m.dptr, m.dcol, du, dw)
        else:
            k("fdd_gather_weighted_norm2", whole[1:2], ws, m.dptr, m.dcol, du, dw, m.rows)
        torch.cuda.synchronize()
        h = whole.cpu().numpy()
        assert h[0] == GUARD and h[2] == GUARD
        results.append(h[1])
    first, second, rows_form = results
    print("gather_weighted_norm2: plan %.17e rows %.17e longdouble %.17e: relative %.3e / %.3e" % (first, rows_form, ref, abs(first - ref) / ref, abs(rows_form - ref) / ref))
    assert np.float64(first).view(np.uint64) == np.float64(second).view(np.uint64), (first, second)
    assert abs(first - ref) <= 1e-13 * ref, (first, ref)
    assert abs(first - rows_form) <= 1e-13 * ref, (first, rows_form)


# ------------------------------------------------------------------------------------------------------------------------
# 3. restriction
# ------------------------------------------------------------------------------------------------------------------------
WAVE_FORM_CAP = 16 * CU_COUNT * 4  # elements per sweep of the wave form: 16 * 256 workgroups of four waves, one element each
FUSED_FORM_CAP = 8 * CU_COUNT      # elements per sweep of the fused form (n_f > 8): one per workgroup
GROUPS_2D_CAP = 16 * CU_COUNT      # groups of 256 / n_f^2 elements per sweep of the 2-D form
# FDD_RESTRICT_CASE in fdd_sub_restriction, as (Nf, Nc) = (n_f - 1, n_c - 1)
COMPILED_PAIRS = [(7, 1), (7, 5), (7, 4), (7, 3), (7, 6), (6, 1), (6, 4), (5, 1), (5, 3), (4, 1), (4, 2), (3, 1), (2, 1)]
GENERIC_PAIRS = [(6, 3), (1, 1)]  # restriction_wave_kernel<0, 0>


def restriction_reference(u, E, Nf, Nc, dim):
    """the oracle's launches (three in 3-D, two in 2-D) on E elements"""
    L = S.oracle()
    n_f, n_c = Nf + 1, Nc + 1
    if Nc < Nf:
        J = np.ascontiguousarray(S.J_cf(Nc, Nf))
    else:  # no interpolation table of the fixtures has equal degrees; the kernels take any n_f x n_c table
        J = np.random.default_rng(8900 + Nf).uniform(-1.0, 1.0, n_f * n_c)
    if dim == 3:
        w1, w2, uc = np.zeros(E * n_f * n_f * n_c), np.zeros(E * n_f * n_c * n_c), np.zeros(E * n_c**3)
        L.orc_sub_restriction_1(P(w1), P(J), P(u), len(w1), n_f, n_c, 3)
        L.orc_sub_restriction_2(P(w2), P(J), P(w1), len(w2), n_f, n_c, 3)
        L.orc_sub_restriction_3(P(uc), P(J), P(w2), len(uc), n_f, n_c)
    else:
        w1, uc = np.zeros(E * n_f * n_c), np.zeros(E * n_c * n_c)
        L.orc_sub_restriction_1(P(w1), P(J), P(u), len(w1), n_f, n_c, 2)
        L.orc_sub_restriction_2(P(uc), P(J), P(w1), len(uc), n_f, n_c, 2)
    return J, uc


def restriction_case(gpu, E, Nf, Nc, dim):
    n_f, n_c = Nf + 1, Nc + 1
    u = np.random.default_rng(9000 + 100 * Nf + Nc + dim).uniform(-1.0, 1.0, E * n_f**dim)
    J, ref = restriction_reference(u, E, Nf, Nc, dim)
    assert np.abs(ref).max() > 0.0
    whole, out = guarded(np.full(len(ref), GUARD), torch.float64, gpu)
    k("fdd_sub_restriction" if dim == 3 else "fdd_sub_restriction_2d", out, dev(J, gpu), dev(u, gpu), E, n_f, n_c)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    differing = np.nonzero((bits(got) != bits(ref)).reshape(E, -1).any(axis=1))[0]
    assert len(differing) == 0, ((E, Nf, Nc, dim), "elements that differ", differing[:20], len(differing))
    assert guards_stand(whole), (E, Nf, Nc, dim)


@pytest.mark.parametrize("Nf,Nc", COMPILED_PAIRS + GENERIC_PAIRS)
def test_restriction_every_instance(gpu, Nf, Nc):
    """fdd_sub_restriction at E = 53 for each of the thirteen compiled restriction_wave_kernel<NF, NC> and two pairs that take
    the instance with its sizes in arguments, as bits"""
    assert Nf + 1 <= 8 and len(set(COMPILED_PAIRS)) == 13 and not set(COMPILED_PAIRS) & set(GENERIC_PAIRS)
    restriction_case(gpu, 53, Nf, Nc, 3)


@pytest.mark.parametrize("Nf,Nc", [(7, 1), (2, 1)])
def test_restriction_wave_form_past_its_cap(gpu, Nf, Nc):
    """every wave takes a second element and five a third: the wave-level syncs in front of the LDS rewrite are all that
    orders an element's stores behind the reads of the element before"""
    E = 2 * WAVE_FORM_CAP + 5
    assert Nf + 1 <= 8 and E > 2 * WAVE_FORM_CAP and E % WAVE_FORM_CAP != 0
    restriction_case(gpu, E, Nf, Nc, 3)


@pytest.mark.parametrize("Nf,Nc", [(8, 1), (15, 9)])
def test_restriction_fused_form_past_its_cap(gpu, Nf, Nc):
    E = 2 * FUSED_FORM_CAP + 5
    assert Nf + 1 > 8 and E > 2 * FUSED_FORM_CAP and E % FUSED_FORM_CAP != 0
    restriction_case(gpu, E, Nf, Nc, 3)


@pytest.mark.parametrize("Nf,Nc,E", [(15, 7, 2 * GROUPS_2D_CAP + 3), (2, 1, 28 * 2 * GROUPS_2D_CAP + 5)])
def test_restriction_2d_past_its_cap(gpu, Nf, Nc, E):
    """fdd_sub_restriction_2d with one element per workgroup and trip (n_f = 16) and with 28 (n_f = 3), the last group ragged"""
    epb = 256 // (Nf + 1) ** 2
    assert epb == (1 if Nf == 15 else 28)
    groups = -(-E // epb)
    assert groups > 2 * GROUPS_2D_CAP and groups % GROUPS_2D_CAP != 0 and (epb == 1 or E % epb != 0)
    restriction_case(gpu, E, Nf, Nc, 2)
