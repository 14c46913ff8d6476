"""Successive-right-hand-side projection on the GPU: the three entries of csrc/fdd_projection.hip against numpy float64,
the single-launch path against the host layer's composition of the same passes from the multi-vector entries (flag
"fused_projection"), and the solver-level checks of tests/projection_checks.py (the basis is A-orthonormal and its images
are the operator's, a right-hand side in its span costs no iteration, a slowly varying sequence needs fewer iterations
with both outer solvers, the lifecycle, two ranks).

Bars of the kernel checks (the project's own for reductions and element-wise sums): a sum within 1e-13 x the sum of the
absolute values of its terms, an entry of x / b within 1e-13 x (|x_in| + sum_k |c_k row_k|) -- the start value is a term
of the sum like the others: without it an entry whose products happen to be tiny would be held below the rounding of the
one addition that forms it."""

import numpy as np
import pytest
import torch

import projection_checks as C
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k, reduce_workspace

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 40_001]
BASES = [0, 1, 2, 7, 8, 9, 16]
GUARD = 777.0
LABELS = {"projection_dots_kernel", "projection_apply_kernel", "projection_store_kernel"}


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rnd(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def lds(n):
    even = n + (n & 1)
    return (even, even + 6)


def slab(K, ld, n, seed, device):
    """K rows of ld doubles; the padding behind the n values of a row is NaN: a kernel that walks ld instead of n shows"""
    a = np.full((max(K, 1), ld), np.nan)
    a[:, :n] = rnd(max(K, 1) * n, seed).reshape(max(K, 1), n)
    return a, dev(a, device)


def off(a, base, device):
    """the vector on the device, `base` doubles off a 16-byte boundary"""
    return dev(np.concatenate([np.zeros(base), a]), device)[base:]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K", BASES)
def test_dots_against_numpy(gpu, n, K):
    """out[k] = <X_k, f> for every ld and both alignments of f; nothing behind out[K] or behind the workspace is touched,
    K = 0 writes nothing at all, and two calls give the same bits"""
    ws_all = torch.full((len(reduce_workspace(gpu)) + 64,), GUARD, dtype=torch.float64, device=gpu)
    ws = ws_all[:-64]
    for ld in lds(n):
        X, dX = slab(K, ld, n, 3, gpu)
        for base in (0, 1):
            f = rnd(n, 4 + base)
            df = off(f, base, gpu)
            out = torch.full((K + 4,), GUARD, dtype=torch.float64, device=gpu)
            k("fdd_projection_dots", out, ws, dX, ld, K, df, n)
            got = host(out).copy()
            k("fdd_projection_dots", out, ws, dX, ld, K, df, n)
            assert np.array_equal(host(out).view(np.int64), got.view(np.int64)), (ld, base)
            assert np.all(got[K:] == GUARD) and np.all(host(ws_all)[-64:] == GUARD), (ld, base)
            for kk in range(K):
                terms = X[kk, :n] * f
                assert abs(got[kk] - terms.sum()) <= 1e-13 * np.abs(terms).sum(), (ld, base, kk, got[kk], terms.sum())


def test_dots_of_nothing_are_zero(gpu):
    ws = reduce_workspace(gpu)
    _, dX = slab(3, 8, 8, 1, gpu)
    out = torch.full((5,), GUARD, dtype=torch.float64, device=gpu)
    k("fdd_projection_dots", out, ws, dX, 8, 3, None, 0)
    assert host(out).tolist() == [0.0, 0.0, 0.0, GUARD, GUARD]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K", BASES)
def test_apply_against_numpy(gpu, n, K):
    """x = x_in + sign_x X c, b = b_in + sign_b AX c and <x, b>, for every ld, both alignments, both sign pairs the host
    layer uses, x_in given and absent (x then holds NaN on entry and must come out finite), with and without the dot; the
    in-place call gives the bits of the out-of-place one"""
    ws = reduce_workspace(gpu)
    c = rnd(max(K, 1), 9)
    dc = dev(c, gpu)
    for ld in lds(n):
        X, dX = slab(K, ld, n, 5, gpu)
        AX, dAX = slab(K, ld, n, 6, gpu)
        for base in (0, 1):
            x_in, b_in = rnd(n, 7), rnd(n, 8)
            for sx, sb in ((1.0, -1.0), (-1.0, -1.0)):
                for with_x_in in (True, False):
                    x0 = x_in if with_x_in else np.zeros(n)
                    want_x = x0 + sx * sum((c[kk] * X[kk, :n] for kk in range(K)), np.zeros(n))
                    want_b = b_in + sb * sum((c[kk] * AX[kk, :n] for kk in range(K)), np.zeros(n))
                    tol_x = 1e-13 * (np.abs(x0) + sum((np.abs(c[kk] * X[kk, :n]) for kk in range(K)), np.zeros(n)))
                    tol_b = 1e-13 * (np.abs(b_in) + sum((np.abs(c[kk] * AX[kk, :n]) for kk in range(K)), np.zeros(n)))
                    what = (ld, base, sx, sb, with_x_in)
                    # out of place, with the dot
                    dx, db = off(np.full(n, np.nan), base, gpu), off(np.full(n, np.nan), base, gpu)
                    dx_in, db_in = (off(x_in, base, gpu) if with_x_in else None), off(b_in, base, gpu)
                    nu2 = torch.full((3,), GUARD, dtype=torch.float64, device=gpu)
                    k("fdd_projection_apply", dx, db, nu2, ws, dx_in, db_in, dX, dAX, ld, K, dc, sx, sb, n)
                    gx, gb, g2 = host(dx).copy(), host(db).copy(), host(nu2).copy()
                    assert np.isfinite(gx).all() and np.isfinite(gb).all(), what
                    assert np.all(np.abs(gx - want_x) <= tol_x) and np.all(np.abs(gb - want_b) <= tol_b), what
                    assert abs(g2[0] - np.dot(gx, gb)) <= 1e-13 * np.abs(gx * gb).sum() and g2[1] == GUARD, (what, g2[0], np.dot(gx, gb))
                    # in place (b always, x where it has a start value), without the dot: the same bits
                    ix = off(x_in if with_x_in else np.full(n, np.nan), base, gpu)
                    ib = off(b_in, base, gpu)
                    k("fdd_projection_apply", ix, ib, None, None, ix if with_x_in else None, ib, dX, dAX, ld, K, dc, sx, sb, n)
                    assert np.array_equal(host(ix).view(np.int64), gx.view(np.int64)) and np.array_equal(host(ib).view(np.int64), gb.view(np.int64)), what


@pytest.mark.parametrize("n", SIZES)
def test_store_scales_both_rows(gpu, n):
    for ld in lds(n):
        for base in (0, 1):
            x, b = rnd(n, 1), rnd(n, 2)
            nu2 = np.array([2.7])
            rows = torch.full((2, ld), GUARD, dtype=torch.float64, device=gpu)
            k("fdd_projection_store", rows[0], rows[1], off(x, base, gpu), off(b, base, gpu), dev(nu2, gpu), n)
            got = host(rows)
            inv = 1.0 / np.sqrt(nu2[0])
            assert np.all(np.abs(got[0, :n] - inv * x) <= 1e-15 * np.abs(x)) and np.all(np.abs(got[1, :n] - inv * b) <= 1e-15 * np.abs(b)), (ld, base)
            assert np.all(got[:, n:] == GUARD)


def test_entries_refuse_too_many_rows_and_an_odd_row_length(gpu):
    ws = reduce_workspace(gpu)
    n = 64
    _, dX = slab(17, n + 2, n, 1, gpu)
    v, w, c = dev(rnd(n, 2), gpu), dev(rnd(n, 3), gpu), dev(rnd(17, 4), gpu)
    out = torch.zeros(32, dtype=torch.float64, device=gpu)
    for K, ld in ((17, n), (2, n + 1), (2, n - 2), (-1, n)):
        with pytest.raises(lib.FddError):
            k("fdd_projection_dots", out, ws, dX, ld, K, v, n)
        with pytest.raises(lib.FddError):
            k("fdd_projection_apply", v, w, None, ws, v, w, dX, dX, ld, K, c, 1.0, 1.0, n)


@pytest.fixture
def setup(gpu):
    H.init(0)
    H.comm_single()
    H.set_print(False)
    return True


def test_single_launches_agree_with_the_composed_passes(setup):
    """four right-hand sides through solve_projected at capacity 4, once with "fused_projection" 1 and once with 0, each
    from an empty basis: the same iteration counts, solutions within 1e-10 |u|_inf, bases within 1e-10 |X_k|_inf entry by
    entry -- and the profile shows the new kernels with the flag on, never with it off"""
    import support as S

    p = C.new_box()
    try:
        p.projection(4)
        fs = [p.make_rhs_from(S.seeded_uniform(p.n, 40 + i))[1] for i in range(4)]
        runs = {}
        for flag in (1, 0):
            p.set_flag("fused_projection", flag)
            p.projection_clear()
            sols, labels = S.profiled(lambda: [p.solve_projected(f, "fcg") for f in fs])
            assert (LABELS <= labels) if flag else not (LABELS & labels), (flag, sorted(labels))
            runs[flag] = (sols, C.basis_of(p))
        p.set_flag("fused_projection", 1)
        assert [s[1] for s in runs[1][0]] == [s[1] for s in runs[0][0]], ([s[1] for s in runs[1][0]], [s[1] for s in runs[0][0]])
        for (ua, _, _, pa), (ub, _, _, pb) in zip(*[r[0] for r in runs.values()]):
            assert np.abs(ua - ub).max() <= 1e-10 * np.abs(ub).max()
            assert pa[2:].tolist() == pb[2:].tolist()
        assert len(runs[1][1]) == len(runs[0][1]) == 4
        for (xa, axa), (xb, axb) in zip(runs[1][1], runs[0][1]):
            dx, dax = np.abs(xa - xb).max() / np.abs(xb).max(), np.abs(axa - axb).max() / np.abs(axb).max()
            print("fused against composed: |dX| %.3e |dAX| %.3e" % (dx, dax))
            assert dx <= 1e-10 and dax <= 1e-10
    finally:
        p.close()


def test_basis_is_a_orthonormal_and_a_rhs_in_its_span_costs_nothing(setup):
    """Three independent seeded right-hand sides solved at 1e-10 into a basis of capacity 4: A X_k (fddh_problem_stiffness)
    equals the stored image within 1e-12 |AX_k|_inf, and X^T (AX), summed in numpy, is the identity within 1e-10 (a cap:
    one classical Gram-Schmidt sweep on three independent fields loses about n eps cond; observed 2.2e-16 on the MI355X and
    4.4e-16 on the CPU build of the host layer, the drift of the images 4.4e-16 and 3.5e-16).  Then 0.7 f_0 - 1.3 f_1 + 0.4 f_2 at 1e-5: no iteration,
    |f - A x0| <= 1e-5 |f| as the solve reports it and as the operator gives it, while the plain solve iterates.  The
    margin between the two tolerances is what makes this hold: an exact float64 projection leaves 9.1e-11 |f| on the CPU
    build, 1.1e5 times below the bar (tests/test_cpu_projection.py asserts the factor 100)."""
    p = C.new_box()
    try:
        fs = C.span_setup(p)
        C.check_basis_properties(p, fs)
        C.check_in_span(p, fs)
    finally:
        p.close()


@pytest.mark.parametrize("method", ["fcg", "gmres"])
@pytest.mark.parametrize("vcycle", [0, 1])
def test_sequence_needs_fewer_iterations_and_meets_the_tolerance(setup, method, vcycle):
    """u*_t = cos(0.2 t) phi_0 + sin(0.2 t) phi_1 + 0.05 t phi_2 + 1e-3 psi_t, t < 8, at capacity 4 (a restart inside the
    sequence): every projected solve meets |f - A u| <= tolerance |f| and agrees with the plain solve of the same f within
    10 tolerance |u|_inf (why the phi are smooth: projection_checks.sequence_fields), the basis never exceeds its capacity,
    and the iterations add up to strictly fewer than the plain sequence's"""
    p = C.new_box()
    try:
        C.check_sequence(p, method, vcycle)
    finally:
        p.close()


def test_lifecycle(setup):
    """capacity 0 is the plain solve bit for bit; clear, set_D_hat and "affine_geometry" empty a live basis, options and
    other flags do not; capacities 17 and -1 are refused and change nothing; f = 0 and a zero-iteration solve store nothing"""
    p = C.new_box()
    try:
        C.check_lifecycle(p)
    finally:
        p.close()


def test_two_ranks_agree_with_one(gpu):
    """8x4x4 elements over 2x1x1 ranks of this process at N = 3, the span test's four solves (the fields are seeded per
    GLOBAL node, so that both decompositions solve the same problem): proj and the iteration counts identical on both
    ranks, no iteration in the span, and every gathered solution within 10 x the span test's tolerance (1e-10, 1e-5 for the
    combination) x |u|_inf of the one-rank run's.  The three solves run at 1e-12, not 1e-10: solved at 1e-10 the one-rank and
    the two-rank PLAIN solve already differ by 20 to 29 tolerances (projection_checks.check_two_ranks has the figures and
    the reason); at 1e-12 the observed distance is 0.17 to 0.32 of a tolerance."""
    C.check_two_ranks()
