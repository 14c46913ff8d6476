"""Chebyshev-Jacobi inner solve (flag "inner_solver" = 1) on the GPU: the element-wise step kernels fdd_cheby_step / _f32
against the composition from vector_vector_addition and vector_diagonal_scaling_dev they must equal bit for bit (odd
lengths, pointers off a 16-byte boundary, guard values around every output), the three forms of a step through the host
layer -- fused gather epilogue, gather + step kernel, composed -- on the same input, the float path against the double
one, and the solver-level checks of tests/chebyshev_checks.py (the recurrence against numpy, the eigenvalue bound, M as a
fixed linear symmetric positive map, the preconditioner and both outer solvers against the oracle, two ranks on the
composite, the refusals, the invalidation)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import chebyshev_checks as C
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

pytestmark = pytest.mark.gpu

GUARD = 777.0
FUSED_LABELS = {"csr_short_pipelined_kernel<gather, ChebyStep>", "csr_short_pipelined_kernel<gather, ChebyStep, f32>"}
STEP_LABELS = {"ew_vec2_kernel<ChebyStep>", "cheby_step_f32_kernel"}


@pytest.fixture(scope="module")
def setup(gpu):
    H.init(0)
    H.comm_single()
    H.set_print(False)
    return True


def profiled(fn):
    lib.host().call("fddh_profile_enable", 1)
    out = fn()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.host().call("fddh_profile_collect", buf, len(buf))
    lib.host().call("fddh_profile_enable", 0)
    return out, set(json.loads(buf.value.decode()))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1, 2, 3, 125, 1027, 600_001])
def test_step_kernel_equals_its_composition(gpu, n, dtype):
    """first, middle and last step for every n and for vectors on and off a 16-byte boundary: the bits of the composition
    from the existing entries, x in place, r_out in place, nothing written behind the n values, and on the last step
    neither d nor r_out written at all"""
    f32 = dtype == torch.float32
    sfx = "_f32" if f32 else ""
    c_d, c_r = 0.37, 1.83
    rng = np.random.default_rng(n)

    def vec(base):
        t = torch.full((n + base + 3,), GUARD, dtype=dtype, device=gpu)
        t[base : base + n] = torch.from_numpy(rng.uniform(-1.0, 1.0, n)).to(dtype).to(gpu)
        return t, t[base : base + n]

    for base in (0, 1):
        for first, last in ((1, 0), (0, 0), (0, 1), (1, 1)):
            (X, x), (D, d), (R, r), (Q, q), (Di, dinv) = (vec(base) for _ in range(5))
            dinv.abs_().add_(0.5)
            x0, d0, r0 = x.clone(), d.clone(), r.clone()
            # the composition (include/fdd_hip.h)
            t, rr, dn, xn = (torch.empty(n, dtype=dtype, device=gpu) for _ in range(4))
            if first:
                k("fdd_vector_diagonal_scaling_dev" + sfx, t, dinv, None, r0, n)
                k("fdd_vector_vector_addition" + sfx, dn, c_r, t, 0.0, t, n)
                xn.copy_(dn)
            else:
                k("fdd_vector_vector_addition" + sfx, rr, 1.0, r0, -1.0, q, n)
                k("fdd_vector_diagonal_scaling_dev" + sfx, t, dinv, None, rr, n)
                k("fdd_vector_vector_addition" + sfx, dn, c_d, d0, c_r, t, n)
                k("fdd_vector_vector_addition" + sfx, xn, 1.0, x0, 1.0, dn, n)
            k("fdd_cheby_step" + sfx, x, d, r, r, q, dinv, c_d, c_r, first, last, n)
            torch.cuda.synchronize()
            case = (n, base, first, last)
            assert torch.equal(x, xn), case
            assert torch.equal(d, d0 if last else dn), case
            assert torch.equal(r, r0 if (last or first) else rr), case
            for whole, part in ((X, x), (D, d), (R, r)):
                assert bool((whole[:base] == GUARD).all()) and bool((whole[base + n :] == GUARD).all()), case


@pytest.mark.parametrize("shape", ["E2N3", "E3N3", "E3N7"])
def test_recurrence_bound_map_and_outer_solves(setup, shape):
    """tests/chebyshev_checks.py run_shape on the product libraries (what it holds: test_cpu_chebyshev.py)"""
    C.run_shape(shape)


@pytest.mark.parametrize("shape", ["E2N3", "E3N3", "E3N7"])
def test_same_bits_in_every_form(setup, shape):
    """check 4: the fused gather epilogue, gather + step kernel and the composition from existing entries give the same bits
    for the same input, in double and in float; float is within 1e-5 of double and not equal to it.  On the shape with
    several row blocks the fused kernel must really have run."""
    p = C.new_box(shape)
    try:
        n = p.sub_info()["unique_dofs"]
        fa = C.rnd(n, 31)
        for order in (2, 4, 7):
            p.inner_chebyshev(order=order)
            got = {}
            for bits in (64, 32):
                p.set_flag("preconditioner_precision", bits)
                for form, (kernels, fused) in {"fused": (1, 1), "step": (1, 0), "composed": (0, 0)}.items():
                    p.set_flag("chebyshev_kernels", kernels)
                    p.set_flag("fused_chebyshev", fused)
                    got[(bits, form)], labels = profiled(lambda: p.sub_dof_solve(fa))
                    if form == "fused" and shape == "E3N7":
                        assert FUSED_LABELS & labels, sorted(labels)
                    if form == "step":
                        assert STEP_LABELS & labels and not (FUSED_LABELS & labels), sorted(labels)
                    if form == "composed":
                        assert not ((STEP_LABELS | FUSED_LABELS) & labels), sorted(labels)
                p.set_flag("chebyshev_kernels", 1)
                p.set_flag("fused_chebyshev", 1)
                assert np.array_equal(got[(bits, "fused")], got[(bits, "step")]), (order, bits)
                assert np.array_equal(got[(bits, "composed")], got[(bits, "step")]), (order, bits)
            z64, z32 = got[(64, "step")], got[(32, "step")]
            err = np.abs(z32 - z64).max() / np.abs(z64).max()
            print("forms %s order %d: float against double %.3e" % (shape, order, err))
            assert err <= 1e-5 and not np.array_equal(z32, z64)
        p.set_flag("preconditioner_precision", 64)
    finally:
        p.close()


def test_two_rank_composite(gpu):
    C.check_composite()
    H.init(0, use_torch_stream=True)
    H.comm_single()


def test_refusals_leave_the_problem_usable(setup):
    C.check_refusals()
