"""The column-order restatements of tests/sell_entry_checks.py against references that are not the kernels, without a GPU:
in double precision the oracle's unfused sequence (orc_amg_matvec, then the smoother's element-wise kernels, as
test_amg_smoother_fused_into_spmv composes them), in single precision the scalar numpy.float32 row loop of
test_f32_spmv_and_fused_smoother -- bit for bit.  And the conditions the cases are built for, asserted: they are what
puts test_gpu_sell_entries.py on the paths it names."""
import ctypes

import numpy as np
import pytest

import sell_entry_checks as C
import support as S

P = S._p
c = ctypes.c_double


def oracle_f64(entry, ptr, col, v):
    """The oracle's unfused launch sequence for `entry`: name -> array"""
    L = S.oracle()
    n = len(ptr) - 1
    ptr, col = np.ascontiguousarray(ptr), np.ascontiguousarray(col)
    val, x, D = (np.ascontiguousarray(v[key]) for key in ("val", "x", "D"))

    def matvec(y, alpha, beta):
        L.orc_amg_matvec(P(y), P(ptr), P(col), P(val), P(x), c(alpha), c(beta), n)
        return y

    if entry == "matvec_beta0":
        return {"y": matvec(np.full(n, np.nan), C.ALPHA, 0.0)}
    if entry in ("matvec_in_place", "matvec_from_y_in"):
        return {"y": matvec(v["y0"].copy(), C.ALPHA, C.BETA)}
    if entry == "residual":
        work = matvec(v["f"].copy(), -1.0, 1.0)
        Sr, w, out = np.zeros(n), np.zeros(n), np.zeros(n)
        L.orc_amg_main_scaled_residual(P(Sr), P(w), P(work), P(D), c(C.COEF), n)
        L.orc_amg_vector_multiplication(P(out), P(D), P(w), n)
        return {"work": out, "Sr": Sr}
    vv = matvec(np.zeros(n), 1.0, 0.0)
    w = np.zeros(n)
    L.orc_amg_main_polynomial_evaluation(P(w), P(vv), P(np.ascontiguousarray(v["Sr"])), P(D), c(C.COEF), n)
    if entry == "polynomial":
        out = np.zeros(n)
        L.orc_amg_vector_multiplication(P(out), P(D), P(w), n)
        return {"work": out}
    u = v["u0"].copy() if entry == "update" else np.zeros(n)
    L.orc_amg_main_update_field(P(u), P(w), P(D), n)
    return {"u": u}


def scalar_f32(entry, ptr, col, v):
    """The IEEE-single restatement of test_f32_spmv_and_fused_smoother: numpy.float32 scalars row by row, products added in
    column order, the epilogue's statements element-wise"""
    f32 = np.float32
    n = len(ptr) - 1
    val, x, D = v["val"], v["x"], v["D"]
    Ax = np.zeros(n, f32)
    for r in range(n):
        s_ = f32(0)
        for j in range(ptr[r], ptr[r + 1]):
            s_ = f32(s_ + f32(val[j] * x[col[j]]))
        Ax[r] = s_
    alpha, beta, coef = f32(C.ALPHA), f32(C.BETA), f32(C.COEF)
    if entry == "matvec_beta0":
        return {"y": (alpha * Ax).astype(f32)}
    if entry in ("matvec_in_place", "matvec_from_y_in"):
        return {"y": ((alpha * Ax).astype(f32) + (beta * v["y0"]).astype(f32)).astype(f32)}
    if entry == "residual":
        work = ((f32(-1) * Ax).astype(f32) + (f32(1) * v["f"]).astype(f32)).astype(f32)
        Sr = (D * work).astype(f32)
        return {"work": ((coef * Sr).astype(f32) * D).astype(f32), "Sr": Sr}
    vv = (Ax * D).astype(f32)
    w = ((coef * v["Sr"]).astype(f32) + vv).astype(f32)
    if entry == "polynomial":
        return {"work": (w * D).astype(f32)}
    if entry == "update":
        return {"u": (v["u0"] + (D * w).astype(f32)).astype(f32)}
    return {"u": (f32(0) + (D * w).astype(f32)).astype(f32)}


@pytest.mark.parametrize("name", C.CASES + C.OTHER_RUNGS)
def test_f64_restatements_are_the_oracle_sequence(name):
    ptr, col, n_rows, n_cols = C.case(name)
    v = C.inputs(name, np.float64)
    for entry, outputs in C.ENTRIES.items():
        got, want = C.restate(entry, np.float64, ptr, col, v), oracle_f64(entry, ptr, col, v)
        assert tuple(got) == tuple(want) == outputs
        for key in outputs:
            assert got[key].dtype == np.float64 and np.isfinite(want[key]).all()
            assert np.array_equal(C.bits(got[key]), C.bits(want[key])), (name, entry, key, int((C.bits(got[key]) != C.bits(want[key])).sum()))


@pytest.mark.parametrize("name", ["every_width", "single_partial_slice"])
def test_f32_restatements_are_the_scalar_row_loop(name):
    ptr, col, n_rows, n_cols = C.case(name)
    v = C.inputs(name, np.float32)
    for entry, outputs in C.ENTRIES.items():
        got, want = C.restate(entry, np.float32, ptr, col, v), scalar_f32(entry, ptr, col, v)
        assert tuple(got) == tuple(want) == outputs
        for key in outputs:
            assert got[key].dtype == np.float32 and np.isfinite(want[key]).all()
            assert np.array_equal(C.bits(got[key]), C.bits(want[key])), (name, entry, key, int((C.bits(got[key]) != C.bits(want[key])).sum()))


def test_case_invariants():
    """Conditions, not measurements: the seeds are chosen so that they hold."""
    for name in C.CASES + C.OTHER_RUNGS:
        ptr, col, n_rows, n_cols = C.case(name)
        lens = np.diff(ptr)
        assert n_rows == n_cols == len(ptr) - 1 and ptr[0] == 0 and ptr[-1] == len(col)
        assert col.min() >= 0 and col.max() < n_cols
        inside = np.ones(len(col), bool)
        inside[ptr[1:-1][ptr[1:-1] < len(col)]] = False  # first entries of the rows after row 0
        step = np.diff(col)[inside[1:]]  # ascending inside every row; drawn columns may repeat in mixed_columns, as in its recipe
        assert (step >= 0).all() if name == "mixed_columns" else (step > 0).all(), name
        assert 0 < ptr[-1] <= 16 * n_rows  # what fdd_csr_plan_attach_sell takes
        for dtype in (np.float64, np.float32):
            v = C.inputs(name, dtype)
            assert all(np.abs(v[key]).max() < 1 for key in ("val", "x", "y0", "f", "Sr", "u0")) and 0.5 <= v["D"].min() and v["D"].max() <= 1.5
            assert not np.all(v["val"] == 1)  # not a unit-value plan

    ptr, col, n, _ = C.case("lattice7")
    lens, widths = np.diff(ptr), C.slice_widths(ptr)
    assert n == 2197 and len(widths) == 35 and n - 34 * C.SLICE == 21 and lens.min() == 4 and lens.max() == 7
    # 7 wide but for the slices that lie wholly in the first or the last plane of 169 nodes, which miss one neighbour: the
    # remainder of 6 or 7 entries is the sell_batch<8, false> tail, and most rows are padded inside it
    assert list(widths) == [6, 6] + [7] * 30 + [6, 6, 6] and (lens < np.repeat(widths, C.SLICE)[:n]).sum() > n // 4
    assert C.expected_compact_slices(ptr, col, n) == len(widths)
    assert not C.twin_splits_rows(ptr)

    ptr, col, n, _ = C.case("every_width")
    lens, widths = np.diff(ptr), C.slice_widths(ptr)
    assert n == C.SLICE * 17 + 5 and list(widths) == list(range(17)) + [3]
    for s in range(1, 17):
        assert lens[s * C.SLICE : (s + 1) * C.SLICE].min() == 0
    assert lens[17 * C.SLICE :].min() >= 1
    assert widths.max() > 4 * max(widths.min(), 1)  # widest-first slice order in force
    assert ptr[-1] <= 16 * n
    assert C.expected_compact_slices(ptr, col, n) == len(widths)
    assert not C.twin_splits_rows(ptr)

    ptr, col, n, n_cols = C.case("mixed_columns")
    lens, widths = np.diff(ptr), C.slice_widths(ptr)
    assert n == 70037 and n_cols > 65535 and lens.max() == 9 and (lens == 0).sum() == C.SLICE + 1 and widths[100] == 0
    assert len(widths) // 3 < C.expected_compact_slices(ptr, col, n) < len(widths)
    assert widths.max() > 4 * max(widths.min(), 1)  # the empty slice puts the widest-first order in force here too

    ptr, col, n, _ = C.case("sparse_rows")  # the plan of one lane per row: no more entries than rows, not one in every row
    lens = np.diff(ptr)
    assert n == 2 * 512 + 37 and n // 2 < ptr[-1] <= n and set(lens) == {0, 1, 2}

    ptr, col, n, _ = C.case("single_entry_rows")  # the plan that does not read the row pointers
    assert n == 2 * 1024 + 37 and list(ptr) == list(range(n + 1))

    ptr, col, n, _ = C.case("single_partial_slice")
    lens, widths = np.diff(ptr), C.slice_widths(ptr)
    assert n == 37 and list(widths) == [5] and lens.min() == 0
    assert C.expected_compact_slices(ptr, col, n) == 1
    assert not C.twin_splits_rows(ptr)


def test_expected_compact_slices_on_slices_worked_out_by_hand():
    """Two rows, one slot: spread 65535 is compact, 65536 is not; a short row repeats its last column in the padded slot;
    an empty row does not count."""
    one = lambda cols: (np.array([0, 1, 2], np.int32), np.array(cols, np.int32), 2)
    assert C.expected_compact_slices(*one([0, 65535])) == 1
    assert C.expected_compact_slices(*one([0, 65536])) == 0
    # row 0 = {5}, row 1 = {5, 70000}: slot 1 holds 5 (repeated) and 70000
    assert C.expected_compact_slices(np.array([0, 1, 3], np.int32), np.array([5, 5, 70000], np.int32), 2) == 0
    # row 0 = {69000}, row 1 = {5, 70000}: slot 0 is wide
    assert C.expected_compact_slices(np.array([0, 1, 3], np.int32), np.array([69000, 5, 70000], np.int32), 2) == 0
    # row 0 = {69000, 69001}, row 1 empty, row 2 = {69500}: the empty row's stand-in column does not count
    assert C.expected_compact_slices(np.array([0, 2, 2, 3], np.int32), np.array([69000, 69001, 69500], np.int32), 3) == 1
    # second slice: rows 64.. ; the first slice stays compact
    ptr = np.concatenate([np.arange(65), [65, 66]]).astype(np.int32)
    col = np.concatenate([np.arange(64), [0, 70000]]).astype(np.int32)
    assert C.expected_compact_slices(ptr, col, 66) == 1


def test_twin_splits_rows_on_plans_worked_out_by_hand():
    rows7 = lambda n: np.arange(n + 1) * 7
    assert not C.twin_splits_rows(np.arange(101) * 3)  # fewer than four entries per row: the small row block, one lane per row
    assert not C.twin_splits_rows(rows7(256 + 149))  # blocks of 256 and 149 rows: more than 128
    assert C.twin_splits_rows(rows7(256 + 128))  # the last block's 128 rows get two lanes each
    assert C.twin_splits_rows(rows7(37))
    assert C.twin_splits_rows(np.concatenate([[0], 2048 - 7 * 20 + rows7(20)]))  # one row of 1908 entries, then 20 of 7: a block of 21 rows
