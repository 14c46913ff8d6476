"""Every SpMV entry of a plan on its sliced-ELL copy (`sell_kernel<T, Epi>`, csrc/fdd_csr.hip), bit for bit against the
column-order restatements of tests/sell_entry_checks.py (held to the oracle in test_cpu_sell_restatement.py): the axpby
entry with beta = 0, in place and from a separate y_in, and the four smoother epilogues with the side output Sr, in
both precisions, with 16-bit and with 32-bit columns, on slices of every width 0 ... 16, a plan that mixes compact and
wide slices, the widest-first slice order and a single ragged slice.  `fdd_csr_plan_sell_info` says that the plan runs
on sell_kernel; a second plan of the same matrix without the copy (the row-block twin) must give the same values."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sell_entry_checks as C
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
GUARD_ENTRIES = 64
SENTINEL = 777.0
# the twin adds no row of these with several lanes (sell_entry_checks.twin_splits_rows, asserted below and without a GPU):
# same bits; mixed_columns: the bar of test_sell_compact_columns
TWIN_AS_BITS = ("lattice7", "every_width", "single_partial_slice")


def run_entries(gpu, plan, precision, ptr, v, d):
    """Every entry of C.ENTRIES on `plan`: entry -> {output name: host array}.  Outputs are allocated with a guard of 64
    sentinel entries behind them and passed at their true length; an output the entry does not read is NaN-filled."""
    n = len(ptr) - 1
    tt = torch.float64 if precision == 64 else torch.float32
    sfx = "" if precision == 64 else "_f32"
    t = lambda a: torch.from_numpy(np.array(a)).to(gpu)  # a copy: the cases are read-only
    wholes = []

    def output(start=None):
        whole = torch.full((n + GUARD_ENTRIES,), SENTINEL, dtype=tt, device=gpu)
        whole[:n] = float("nan") if start is None else t(start)
        wholes.append(whole)
        return whole[:n]

    matrix = (d["ptr"], d["col"], d["val"])
    results = {}
    y = output()
    k("fdd_csr_plan_matvec_to" + sfx, plan, y, None, *matrix, d["x"], C.ALPHA, 0.0)
    results["matvec_beta0"] = {"y": y}
    y = output(v["y0"])
    k("fdd_csr_plan_matvec_to" + sfx, plan, y, None, *matrix, d["x"], C.ALPHA, C.BETA)
    results["matvec_in_place"] = {"y": y}
    y, y_in = output(), t(v["y0"])
    k("fdd_csr_plan_matvec_to" + sfx, plan, y, y_in, *matrix, d["x"], C.ALPHA, C.BETA)
    results["matvec_from_y_in"] = {"y": y}
    work, Sr = output(), output()
    k("fdd_amg_smooth_residual_matvec" + sfx, plan, work, Sr, *matrix, d["x"], d["f"], d["D"], C.COEF)
    results["residual"] = {"work": work, "Sr": Sr}
    work = output()
    k("fdd_amg_smooth_polynomial_matvec" + sfx, plan, work, *matrix, d["x"], d["Sr"], d["D"], C.COEF)
    results["polynomial"] = {"work": work}
    u = output(v["u0"])
    k("fdd_amg_smooth_update_matvec" + sfx, plan, u, *matrix, d["x"], d["Sr"], d["D"], C.COEF)
    results["update"] = {"u": u}
    u = output()
    k("fdd_amg_smooth_update_matvec_from_zero" + sfx, plan, u, *matrix, d["x"], d["Sr"], d["D"], C.COEF)
    results["update_from_zero"] = {"u": u}
    torch.cuda.synchronize()
    for whole in wholes:
        assert bool((whole[n:] == SENTINEL).all()), "an entry wrote past its output"
    assert np.array_equal(C.bits(y_in.cpu().numpy()), C.bits(v["y0"])), "matvec_to changed y_in"
    for key in ("x", "f", "Sr", "D", "val"):
        assert np.array_equal(C.bits(d[key].cpu().numpy()), C.bits(v[key])), "an entry changed its input " + key
    return {entry: {key: a.cpu().numpy() for key, a in outs.items()} for entry, outs in results.items()}


@pytest.mark.parametrize("form", ["col16", "col32"])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", C.CASES)
def test_sell_entries_are_their_column_order_restatements(gpu, name, precision, form):
    ptr, col, n, n_cols = C.case(name)
    dtype = np.float64 if precision == 64 else np.float32
    v = C.inputs(name, dtype)
    t = lambda a: torch.from_numpy(np.array(a)).to(gpu)  # a copy: the cases are read-only
    d = {key: t(a) for key, a in v.items()}
    d["ptr"], d["col"] = t(ptr), t(col)
    create = "fdd_csr_plan_create" if precision == 64 else "fdd_csr_plan_create_f32"
    slices_expected = (n + C.SLICE - 1) // C.SLICE
    plans = {}
    try:
        for which in ("sell", "twin"):
            plans[which] = vp()
            lib.hip().call(create, ctypes.byref(plans[which]), vp(ptr.ctypes.data), n, n_cols, int(ptr[-1]))
        os.environ["FDD_TUNE_CSR_SELL_COL16"] = "0" if form == "col32" else "1"
        attached = ctypes.c_int(0)
        k("fdd_csr_plan_attach_sell", plans["sell"], vp(ptr.ctypes.data), d["ptr"], d["col"], d["val"], ctypes.c_double(1e9), ctypes.byref(attached))
        assert attached.value == 1
        for which, want_slices, want_compact in (("sell", slices_expected, C.expected_compact_slices(ptr, col, n) if form == "col16" else 0), ("twin", 0, 0)):
            slices, compact = ctypes.c_int(-1), ctypes.c_int(-1)
            lib.hip().call("fdd_csr_plan_sell_info", plans[which], ctypes.byref(slices), ctypes.byref(compact))
            assert (slices.value, compact.value) == (want_slices, want_compact), (which, slices.value, compact.value)

        got = run_entries(gpu, plans["sell"], precision, ptr, v, d)
        twin = run_entries(gpu, plans["twin"], precision, ptr, v, d)
    finally:
        os.environ.pop("FDD_TUNE_CSR_SELL_COL16", None)
        for plan in plans.values():
            lib.hip().call("fdd_csr_plan_destroy", plan)

    failures, away = [], 0.0
    for entry, outputs in C.ENTRIES.items():
        want = C.restate(entry, dtype, ptr, col, v)
        assert tuple(got[entry]) == tuple(want) == outputs
        for key in outputs:
            differ = C.bits(got[entry][key]) != C.bits(want[key])
            if differ.any():
                failures.append("%s.%s: %d of %d rows differ from the restatement, first row %d" % (entry, key, differ.sum(), n, np.flatnonzero(differ)[0]))
            if name in TWIN_AS_BITS:
                assert not C.twin_splits_rows(ptr)
                same = np.array_equal(C.bits(twin[entry][key]), C.bits(got[entry][key]))
            else:
                # the row-block kernel may add a row's products with several lanes (the entries stand in for cusparseSpMV,
                # whose order is undefined): same values to rounding, the relative bar of test_sell_compact_columns without its
                # absolute term (measured distance on this case: 0 in both precisions)
                same = np.allclose(got[entry][key], twin[entry][key], rtol=1e-12 if precision == 64 else 1e-4, atol=0.0)
            away = max(away, float((np.abs(got[entry][key] - twin[entry][key]) / np.maximum(np.abs(twin[entry][key]), np.finfo(dtype).tiny)).max()))
            if not same:
                failures.append("%s.%s: the plan without a sliced-ELL copy gives other values" % (entry, key))
    print("%s %d %s: largest relative distance of a row from the twin's, over all entries: %.3e" % (name, precision, form, away))
    assert not failures, (name, precision, form, failures)


@pytest.mark.parametrize("name", C.OTHER_RUNGS)
def test_entries_on_the_plans_without_row_blocks(gpu, name):
    """The same entries on the two rungs of plan_launch that have no row blocks (double precision only): no more entries than
    rows (`sparse_rows`: csr_row_kernel, one lane per row) and exactly one entry in every row (`single_entry_rows`:
    csr_one_per_row_kernel, which does not read the row pointers).  Both keep the column order: the same restatements, as
    bits.  No sliced-ELL copy here -- no other test calls the axpby entry on these two rungs, or the smoothers on the first."""
    ptr, col, n, n_cols = C.case(name)
    v = C.inputs(name, np.float64)
    t = lambda a: torch.from_numpy(np.array(a)).to(gpu)
    d = {key: t(a) for key, a in v.items()}
    d["ptr"], d["col"] = t(ptr), t(col)
    plan = vp()
    lib.hip().call("fdd_csr_plan_create", ctypes.byref(plan), vp(ptr.ctypes.data), n, n_cols, int(ptr[-1]))
    try:
        kind = ctypes.c_int(-1)
        lib.hip().call("fdd_csr_plan_kind", plan, ctypes.byref(kind))
        assert kind.value == 0 and (set(np.diff(ptr)) == {1}) == (name == "single_entry_rows")
        got = run_entries(gpu, plan, 64, ptr, v, d)
    finally:
        lib.hip().call("fdd_csr_plan_destroy", plan)
    for entry, outputs in C.ENTRIES.items():
        want = C.restate(entry, np.float64, ptr, col, v)
        for key in outputs:
            differ = C.bits(got[entry][key]) != C.bits(want[key])
            assert not differ.any(), (name, entry, key, int(differ.sum()), int(np.flatnonzero(differ)[0]))
