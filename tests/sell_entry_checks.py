"""Cases and column-order restatements for the SpMV entries of a plan on its sliced-ELL copy (`sell_kernel<T, Epi>`,
csrc/fdd_csr.hip).  Plain numpy; test_cpu_sell_restatement.py holds the restatements to the oracle without a GPU,
test_gpu_sell_entries.py holds the kernel to them bit for bit.

On the sliced-ELL copy one lane owns a row and adds its products in column order, starting from +0.0; a padded slot
adds 0 * x[c] for a column the row already reads, which on finite input leaves the sum's bits alone.  So every entry
can be restated slot by slot: acc = acc + val[:, k] * x[col[:, k]] on the rows that have a k-th entry, product and sum
rounded separately in the entry's own type, then the epilogue's statements in the order csrc/fdd_csr.hip quotes them."""
import functools

import numpy as np

SLICE = 64  # rows of a slice: one wavefront
COEF = -0.37
ALPHA, BETA = 0.75, -1.25
CASES = ("lattice7", "every_width", "mixed_columns", "single_partial_slice")
# entry -> the outputs it writes, the first being the vector the C entry takes as y / work / u
ENTRIES = {
    "matvec_beta0": ("y",),
    "matvec_in_place": ("y",),
    "matvec_from_y_in": ("y",),
    "residual": ("work", "Sr"),
    "polynomial": ("work",),
    "update": ("u",),
    "update_from_zero": ("u",),
}


def _from_lengths(lens, cols_of_row):
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    parts = [np.sort(cols_of_row(r, int(L))) for r, L in enumerate(lens) if L] + [np.zeros(0, np.int64)]
    return ptr, np.concatenate(parts).astype(np.int32)


def _lattice7():
    m = 13
    idx = np.arange(m**3).reshape(m, m, m)
    rows, cols = [], []
    for dz, dy, dx in ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
        z0, z1, y0, y1, x0, x1 = max(0, -dz), m - max(0, dz), max(0, -dy), m - max(0, dy), max(0, -dx), m - max(0, dx)
        rows.append(idx[z0:z1, y0:y1, x0:x1].reshape(-1))
        cols.append(idx[z0 + dz : z1 + dz, y0 + dy : y1 + dy, x0 + dx : x1 + dx].reshape(-1))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m**3))]).astype(np.int32)
    return ptr, cols[order].astype(np.int32), m**3, m**3


def _every_width():
    rng = np.random.default_rng(411)
    n = SLICE * 17 + 5
    lens = np.zeros(n, np.int64)
    for s in range(1, 17):
        part = rng.integers(0, s + 1, SLICE)
        a, b = rng.choice(SLICE, size=2, replace=False)
        part[a], part[b] = s, 0
        lens[s * SLICE : (s + 1) * SLICE] = part
    tail = rng.integers(1, 4, 5)
    tail[rng.integers(0, 5)] = 3
    lens[17 * SLICE :] = tail
    ptr, col = _from_lengths(lens, lambda r, L: rng.choice(n, size=L, replace=False))
    return ptr, col, n, n


def _mixed_columns():
    rng = np.random.default_rng(412)
    n = 70000 + 37
    lens = rng.integers(1, 10, n)
    lens[777] = 0
    lens[SLICE * 100 : SLICE * 101] = 0  # a slice of empty rows
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(ptr[-1])
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    # the "mixed" recipe of test_sell_compact_columns: stripes of 1024 rows, columns near the diagonal / anywhere
    near = (row_of + rng.integers(0, 30000, nnz)).clip(0, n - 1)
    far = rng.integers(0, n, nnz)
    pick = np.where(row_of % 2048 < 1024, near, far)
    col = pick[np.lexsort((pick, row_of))].astype(np.int32)  # ascending inside every row
    return ptr, col, n, n


def _single_partial_slice():
    rng = np.random.default_rng(413)
    n = 37
    lens = rng.integers(0, 6, n)
    lens[3], lens[20] = 0, 5
    ptr, col = _from_lengths(lens, lambda r, L: rng.choice(n, size=L, replace=False))
    return ptr, col, n, n


def _sparse_rows():
    """Not a sliced-ELL case: rows of 0, 1 or 2 entries, no more entries than rows -- the double-precision plan of one lane
    per row (csr_row_kernel, two rows per lane: 2 * 512 + 37 rows are three workgroups, the last one ragged)"""
    rng = np.random.default_rng(414)
    n = 2 * 512 + 37
    lens = rng.choice([0, 1, 2], size=n, p=[0.4, 0.35, 0.25])
    lens[:3], lens[-2:] = (2, 0, 1), (0, 2)
    ptr, col = _from_lengths(lens, lambda r, L: rng.choice(n, size=L, replace=False))
    return ptr, col, n, n


def _single_entry_rows():
    """Not a sliced-ELL case either: exactly one entry in every row -- the double-precision plan that does not read the row
    pointers (csr_one_per_row_kernel, four rows per lane: 2 * 1024 + 37 rows are three workgroups, the last one ragged)"""
    rng = np.random.default_rng(415)
    n = 2 * 1024 + 37
    return np.arange(n + 1, dtype=np.int32), rng.integers(0, n, n).astype(np.int32), n, n


OTHER_RUNGS = ("sparse_rows", "single_entry_rows")
_BUILDERS = {"lattice7": _lattice7, "every_width": _every_width, "mixed_columns": _mixed_columns, "single_partial_slice": _single_partial_slice, "sparse_rows": _sparse_rows, "single_entry_rows": _single_entry_rows}
assert tuple(_BUILDERS)[: len(CASES)] == CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """ptr, col, n_rows, n_cols of a case (square: the smoother entries take vectors of both lengths); read-only"""
    ptr, col, n_rows, n_cols = _BUILDERS[name]()
    ptr.setflags(write=False)
    col.setflags(write=False)
    return ptr, col, n_rows, n_cols


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """The case's values in (-1, 1), its vectors in (-1, 1) and D in (0.5, 1.5), from a fixed seed, in `dtype`; read-only"""
    ptr, _, n_rows, n_cols = case(name)
    rng = np.random.default_rng(500 + list(_BUILDERS).index(name))
    v = {"val": rng.uniform(-1, 1, int(ptr[-1]))}
    for key in ("x", "y0", "f", "Sr", "u0"):
        v[key] = rng.uniform(-1, 1, n_cols if key == "x" else n_rows)
    v["D"] = rng.uniform(0.5, 1.5, n_rows)
    v = {key: a.astype(dtype) for key, a in v.items()}
    for a in v.values():
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return v


def slice_widths(ptr):
    lens = np.diff(ptr)
    return np.array([int(lens[i : i + SLICE].max()) for i in range(0, len(lens), SLICE)])


def expected_compact_slices(ptr, col, n_rows):
    """How many slices take the 16-bit column form: the rule of sell_probe_kernel.  A slice is compact when in every slot
    the largest and the smallest column differ by at most 65535; a row shorter than the slice repeats its last column in
    the padded slots; empty rows do not count."""
    lens = np.diff(ptr).astype(np.int64)
    slices = (n_rows + SLICE - 1) // SLICE
    width = slice_widths(ptr)
    first = np.asarray(ptr[:-1], np.int64)
    live = np.zeros(slices * SLICE, bool)
    live[:n_rows] = lens > 0
    wide = np.zeros(slices, bool)
    for k in range(int(lens.max())):
        c = np.zeros(slices * SLICE, np.int64)
        c[:n_rows][lens > 0] = col[(first + np.minimum(k, lens - 1))[lens > 0]]
        lo = np.where(live, c, np.iinfo(np.int64).max).reshape(slices, SLICE).min(axis=1)
        hi = np.where(live, c, -1).reshape(slices, SLICE).max(axis=1)
        wide |= (k < width) & (hi >= 0) & (hi - lo > 65535)
    return int(slices - wide.sum())


def twin_splits_rows(ptr, block_nnz_max=2048, workgroup=256):
    """Whether the plan of the same matrix without a sliced-ELL copy adds some row with several lanes (plan_create and
    csr_block_kernel restated): only plans of the large row block (nnz >= 4 * rows; at most 256 rows and 2048 entries per
    block, cut greedily) do, in the blocks with at most 128 rows, two lanes or more per row.  Rows of up to two entries
    keep their bits under any split (a + b = b + a)."""
    ptr = np.asarray(ptr, np.int64)
    rows = len(ptr) - 1
    if ptr[-1] < 4 * rows:
        return False
    r = 0
    while r < rows:
        e = r
        while e < rows and e - r < workgroup and ptr[e + 1] - ptr[r] <= block_nnz_max:
            e += 1
        e = max(e, r + 1)
        if (e - r) * 2 <= workgroup and np.diff(ptr[r : e + 1]).max() > 2:
            return True
        r = e
    return False


def row_sums(ptr, col, val, x):
    """acc = 0; acc = acc + val[k] * x[col[k]] slot after slot, each product and each sum rounded in val's type"""
    T = val.dtype
    assert x.dtype == T
    lens = np.diff(ptr)
    first = np.asarray(ptr[:-1], np.int64)
    acc = np.zeros(len(lens), T)
    for k in range(int(lens.max()) if len(lens) else 0):
        on = lens > k
        j = first[on] + k
        prod = (val[j] * x[col[j]]).astype(T)
        acc[on] = (acc[on] + prod).astype(T)
    return acc


def restate(entry, dtype, ptr, col, v):
    """The outputs of `entry` (a key of ENTRIES) on the matrix (ptr, col, v["val"]) and the vectors of v, all of `dtype`:
    name -> array.  The statements are the epilogues' (EpiAxpbyT ... EpiSmoothUpdateZeroT), one rounding per operation."""
    T = np.dtype(dtype).type
    for a in v.values():
        assert a.dtype == T
    s = row_sums(ptr, col, v["val"], v["x"])
    D, coef = v["D"], T(COEF)
    if entry == "matvec_beta0":  # alpha * s, y is not read
        return {"y": T(ALPHA) * s}
    if entry in ("matvec_in_place", "matvec_from_y_in"):  # alpha * s + beta * y
        return {"y": T(ALPHA) * s + T(BETA) * v["y0"]}
    if entry == "residual":
        work = T(-1) * s + T(1) * v["f"]
        sr = D * work
        w = coef * sr
        return {"work": w * D, "Sr": sr}
    vv = (T(1) * s) * D
    w = coef * v["Sr"] + vv
    if entry == "polynomial":
        return {"work": w * D}
    if entry == "update":
        return {"u": v["u0"] + D * w}
    if entry == "update_from_zero":
        return {"u": T(0) + D * w}
    raise KeyError(entry)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
