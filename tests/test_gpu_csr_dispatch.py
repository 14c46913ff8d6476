"""Which kernel a CSR plan's entries run on (plan_launch and the gather entries of csrc/fdd_csr.hip), rung by rung:
the smallest plans at which each rung of the ladder is taken and a row range can straddle a row block, on
fdd_csr_plan_multiply, fdd_csr_plan_dssum (mode 1), fdd_csr_plan_gather_f32 and fdd_csr_plan_matvec_to, against the
oracle entries the other CSR tests call (csr_matrix.okl in double, its DType = float gather, AMG/csr_matrix.cpp's
matvec).

Bar: BIT-IDENTICAL wherever the entry keeps the column order of a row's sum.  The plans are shaped so that this is
every row but two kinds:
  * the one row longer than a row block ("long" plan) is reduced by the whole workgroup: the 1e-13 bar that
    test_csr_ragged_rows holds such rows to;
  * the f32 plan of 40-60 entries per row: fdd_csr_plan_matvec_to_f32 stands in for cusparseSpMV, whose summation
    order is undefined, and adds the few wide rows of a block with several lanes each.  Two orders of a sum of n
    float products differ by at most 2 n u sum|a_j x_j| (u = 2^-24), then alpha * s + beta * y rounds twice more.
The double plans of 5-9 entries per row have more than 128 rows in every block, where the several-lanes form of the
free-order entries does not apply (csr_block_kernel: nrows * lanes * 2 <= 256), so the matvec there is in column order.

The library reads FDD_TUNE_GATHER_PIPELINED once per process: the one-block-per-workgroup forms are checked by a child
process started with it set to 0 (this file run as a script), which also sees fdd_csr_plan_pipelined report 0.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]

import pytest
import torch

import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
P = S._p
f32 = np.float32
c_double = ctypes.c_double


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def csr_from_lens(lens, ncols, seed):
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(ncols, size=int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, col, rng.uniform(-1, 1, len(col))


def short_boolean_plan():
    """Rows of 0-3 entries, 2*1024 + 37 rows: row blocks of 1024 non-zeros, several of them, an all-empty leading block
    and runs of empty rows further on.  (More entries than rows, or the plan takes one lane per row: the stored rows hold 2-3.)"""
    rng = np.random.default_rng(21)
    rows = 2 * 1024 + 37
    lens = rng.integers(2, 4, rows)
    lens[:1024] = 0
    lens[1500:1530] = 0
    lens[rng.integers(1024, rows, 60)] = rng.integers(0, 2, 60)
    lens[-2:] = 0
    assert lens.sum() > rows and lens.max() == 3
    ptr, col, _ = csr_from_lens(lens, 3000, 22)
    return ptr, col, np.ones(len(col)), 3000


def wide_plan(long_row):
    """Rows of 5-9 stored values, 3 * 256 + 177 of them (about 3 * 2048 non-zeros): row blocks of 2048 non-zeros holding
    256, 256, 256 and 177 rows.  long_row: one more row, of 2048 + 5 entries, between the first block and the second."""
    rng = np.random.default_rng(23)
    lens = rng.integers(5, 10, 3 * 256 + 177)
    if long_row:
        lens = np.concatenate([lens[:256], [2048 + 5], lens[256:]])
    ptr, col, val = csr_from_lens(lens, 4000, 24)
    return ptr, col, val, 4000


def split_row_plan():
    """Rows of 40-60 values, 300 of them: the few wide rows of a block are added by several lanes each (free-order entries)."""
    lens = np.random.default_rng(25).integers(40, 61, 300)
    ptr, col, val = csr_from_lens(lens, 2000, 26)
    return ptr, col, val, 2000


def row_ranges(rows):
    return ((0, rows), (17, rows - 5), (rows - 3, rows), (rows // 2, rows // 2))


def make_plan(ptr, ncols, entry="fdd_csr_plan_create"):
    plan = vp()
    lib.hip().call(entry, ctypes.byref(plan), P(ptr), len(ptr) - 1, ncols, int(ptr[-1]))
    return plan


def plan_int(plan, entry):
    out = ctypes.c_int(-1)
    lib.hip().call(entry, plan, ctypes.byref(out))
    return out.value


def check_double_plan(gpu, name, ptr, col, val, ncols, boolean, blocks):
    L = S.oracle()
    rows = len(ptr) - 1
    lens = np.diff(ptr)
    long_rows = np.nonzero(lens > 2048)[0]
    rng = np.random.default_rng(31)
    u, w, y0, yin = rng.uniform(-1, 1, ncols), rng.uniform(0.5, 2, rows), rng.uniform(-1, 1, rows), rng.uniform(-1, 1, rows)
    ones = np.ones(len(col))
    dptr, dcol, dval, du, dw = dev(ptr, gpu), dev(col, gpu), dev(val, gpu), dev(u, gpu), dev(w, gpu)

    def same(got, want, what):
        exact = np.ones(rows, bool)
        exact[long_rows] = False
        assert np.array_equal(got[exact], want[exact]), (name, what)
        if len(long_rows):  # reduced by the whole workgroup: the bar of test_csr_ragged_rows
            scale = np.abs(want).max() + 1e-300
            assert np.abs(got[long_rows] - want[long_rows]).max() <= 1e-13 * max(scale, 1.0) * 64, (name, what)

    plan = make_plan(ptr, ncols)
    try:
        assert plan_int(plan, "fdd_csr_plan_kind") == 1 and plan_int(plan, "fdd_csr_plan_num_blocks") == blocks, name
        ref, refw = np.zeros(rows), np.zeros(rows)
        L.orc_csr_multiply(P(ref), P(ptr), P(col), P(val), P(u), rows)
        L.orc_csr_multiply_weight(P(refw), P(ptr), P(col), P(val), P(u), P(w), rows)
        for unit in ([False, True] if boolean else [False]):
            if unit:
                lib.hip().call("fdd_csr_plan_set_unit_values", plan, 1)
            out = torch.full((rows,), 7.0, dtype=torch.float64, device=gpu)
            k("fdd_csr_plan_multiply", plan, out, dptr, dcol, None if unit else dval, du, None)
            same(host(out), ref, ("multiply", unit))
            k("fdd_csr_plan_multiply", plan, out, dptr, dcol, None if unit else dval, du, dw)
            same(host(out), refw, ("multiply_weight", unit))

            # y = alpha*A*x + beta*y: beta = 0 (y is not read), beta != 0 in place, and from another vector y_in
            for alpha, beta, src in ((1.0, 0.0, None), (-1.0, 0.5, None), (0.75, -1.25, yin)):
                want = np.zeros(rows) if beta == 0.0 else (y0 if src is None else src).copy()
                L.orc_amg_matvec(P(want), P(ptr), P(col), P(val), P(u), c_double(alpha), c_double(beta), rows)
                dy = dev(np.full(rows, np.nan) if beta == 0.0 else y0, gpu)
                k("fdd_csr_plan_matvec_to", plan, dy, None if src is None else dev(src, gpu), dptr, dcol, None if unit else dval, du, alpha, beta)
                same(host(dy), want, ("matvec_to", unit, alpha, beta))

        # the gathers see the matrix as boolean: t = sum of u over the row's entries (* weight), rows [lo, hi) only
        tref, trefw = np.zeros(rows), np.zeros(rows)
        L.orc_csr_multiply(P(tref), P(ptr), P(col), P(ones), P(u), rows)
        L.orc_csr_multiply_weight(P(trefw), P(ptr), P(col), P(ones), P(u), P(w), rows)
        u32 = u.astype(f32)
        du32 = dev(u32, gpu)
        lib.hip().call("fdd_csr_plan_set_unit_values", plan, 1)
        for lo, hi in row_ranges(rows):
            for weight, want_all in ((None, tref), (dw, trefw)):
                want = np.full(rows, 9.0)
                want[lo:hi] = want_all[lo:hi]
                t = torch.full((rows,), 9.0, dtype=torch.float64, device=gpu)
                k("fdd_csr_plan_dssum", plan, None, t, dptr, dcol, du, weight, None, lo, hi, 1)
                assert np.array_equal(host(t), want), (name, "dssum gather", weight is not None, lo, hi)  # a long row too: one lane per row there
            want32 = np.full(rows, 9.0, f32)
            L.orc_f32_csr_gather(P(want32), P(ptr), P(col), P(u32), lo, hi)
            t32 = torch.full((rows,), 9.0, dtype=torch.float32, device=gpu)
            k("fdd_csr_plan_gather_f32", plan, t32, dptr, dcol, du32, lo, hi)
            assert np.array_equal(host(t32), want32), (name, "gather_f32", lo, hi)
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)


def check_f32_plan(gpu, name, ptr, col, val, ncols, column_order):
    L = S.oracle()
    rows = len(ptr) - 1
    lens = np.diff(ptr)
    rng = np.random.default_rng(41)
    val32 = val.astype(f32) if not np.all(val == 1.0) else rng.uniform(-1, 1, len(col)).astype(f32)
    x, yin = rng.uniform(-1, 1, ncols).astype(f32), rng.uniform(-1, 1, rows).astype(f32)
    # IEEE-single row sums in column order, all rows at once: entry j of every row that has one
    Ax, absAx = np.zeros(rows, f32), np.zeros(rows)
    for j in range(int(lens.max())):
        on = np.nonzero(lens > j)[0]
        prod = val32[ptr[on] + j] * x[col[ptr[on] + j]]
        Ax[on] = Ax[on] + prod
        absAx[on] += np.abs(prod.astype(np.float64))
    assert Ax.dtype == f32
    dptr, dcol, dval, dx = dev(ptr, gpu), dev(col, gpu), dev(val32, gpu), dev(x, gpu)
    plan = make_plan(ptr, ncols, "fdd_csr_plan_create_f32")
    try:
        assert plan_int(plan, "fdd_csr_plan_kind") == 1
        for alpha, beta, src in ((f32(1.0), f32(0.0), None), (f32(0.75), f32(-1.25), yin)):
            want = (alpha * Ax).astype(f32) if src is None else ((alpha * Ax).astype(f32) + (beta * src).astype(f32)).astype(f32)
            y = torch.full((rows,), float("nan"), dtype=torch.float32, device=gpu)
            k("fdd_csr_plan_matvec_to_f32", plan, y, None if src is None else dev(src, gpu), dptr, dcol, dval, dx, float(alpha), float(beta))
            if column_order:
                assert np.array_equal(host(y), want), (name, "matvec_to_f32", alpha, beta)
            else:
                u = 2.0**-24
                bound = u * (2.0 * lens * abs(alpha) * absAx + 4.0 * (abs(alpha) * absAx + (0.0 if src is None else np.abs(beta * src.astype(np.float64)))))
                assert np.all(np.abs(host(y).astype(np.float64) - want.astype(np.float64)) <= bound), (name, "matvec_to_f32", alpha, beta)
        for lo, hi in row_ranges(rows):
            want32 = np.full(rows, 9.0, f32)
            L.orc_f32_csr_gather(P(want32), P(ptr), P(col), P(x), lo, hi)
            t32 = torch.full((rows,), 9.0, dtype=torch.float32, device=gpu)
            k("fdd_csr_plan_gather_f32", plan, t32, dptr, dcol, dx, lo, hi)
            assert np.array_equal(host(t32), want32), (name, "gather_f32", lo, hi)
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)


def check_everything(gpu):
    short, wide, long_, split = short_boolean_plan(), wide_plan(False), wide_plan(True), split_row_plan()
    assert np.diff(short[0])[:1024].max() == 0 and np.diff(long_[0])[256] == 2048 + 5
    check_double_plan(gpu, "short", *short, boolean=True, blocks=plan_blocks(short[0], 1024, 1024))
    check_double_plan(gpu, "wide", *wide, boolean=False, blocks=4)
    check_double_plan(gpu, "long", *long_, boolean=False, blocks=5)
    check_f32_plan(gpu, "short f32", *short, column_order=True)
    check_f32_plan(gpu, "wide f32", *wide, column_order=True)
    check_f32_plan(gpu, "split f32", *split, column_order=False)


def plan_blocks(ptr, block_nnz, row_cap):
    """The plan's row blocks as include/fdd_hip.h describes them: consecutive rows, at most block_nnz entries and row_cap rows."""
    blocks, r, rows = 0, 0, len(ptr) - 1
    while r < rows:
        e = r
        while e < rows and e - r < row_cap and ptr[e + 1] - ptr[r] <= block_nnz:
            e += 1
        r = max(e, r + 1)
        blocks += 1
    return blocks


def short_plan_is_pipelined():
    ptr, _, _, ncols = short_boolean_plan()
    plan = make_plan(ptr, ncols)
    try:
        return plan_int(plan, "fdd_csr_plan_pipelined")
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)


def test_every_rung_against_the_oracle(gpu):
    assert plan_blocks(short_boolean_plan()[0], 1024, 1024) >= 4
    check_everything(gpu)
    assert short_plan_is_pipelined() == int(int(os.environ.get("FDD_TUNE_GATHER_PIPELINED") or 4) > 0)  # 1 unless the caller turned it off


def test_one_block_per_workgroup_forms_in_a_child_process(gpu):
    """FDD_TUNE_GATHER_PIPELINED=0: no plan runs on the persistent pipelined kernel, the same results."""
    env = dict(os.environ, FDD_TUNE_GATHER_PIPELINED="0")
    done = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "dispatch child ok" in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


if __name__ == "__main__":
    assert torch.cuda.is_available()
    device = torch.device("cuda:0")
    assert short_plan_is_pipelined() == 0
    check_everything(device)
    print("dispatch child ok")
