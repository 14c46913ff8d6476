"""The zeroth-order term on the support of its coefficient alone (include/fdd_hip.h):
  fdd_shift_add_indexed[_f32](y, c_values, index, m, scale_dev, x, n)    y[index[k]] = y[index[k]] + c_values[k] * (s * x[index[k]])
against numpy in the same precision: the statement is a multiply and an add (the library is compiled with -ffp-contract=off,
the float entry rounds s to float first, as fdd_shift_add_f32 does), so on the support the bits are numpy's -- and with them
the dense entry's, which tests/test_gpu_helmholtz_kernels.py holds to the same statement -- and everything else of y, the guard
words around it included, keeps its raw bits (a -0.0 and a NaN payload among them: the dense entry's y + 0 * x would turn
the former into +0.0).
"""
import numpy as np
import pytest
import torch

import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

pytestmark = pytest.mark.gpu

# no entry, one, a wavefront less one / whole / and one, and more workgroups than one (256 lanes each) with a ragged last
SIZES = (0, 1, 63, 64, 65, 4097)


def raw(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def data(m, dtype, seed):
    """n = 3 m + 11 values, m distinct ascending indices with the first and the last value of the vector among them"""
    rng = np.random.default_rng(seed)
    n = 3 * m + 11
    index = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
    if m >= 2:
        index[0], index[-1] = 0, n - 1
    y, x, c = (rng.uniform(-1.0, 1.0, size).astype(dtype) for size in (n, n, m))
    off = np.setdiff1d(np.arange(n), index)
    y[off[0]] = -0.0
    raw(y)[off[1]] = raw(np.array([np.nan], dtype))[0] | 0x1234  # a NaN with a payload
    return n, index, y, x, c


@pytest.mark.parametrize("scaled", (False, True), ids=("plain", "scaled"))
@pytest.mark.parametrize("offset", (0, 1), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("m", SIZES)
def test_bits_on_the_support_and_nothing_else(gpu, m, dtype, offset, scaled):
    n, index, y, x, c = data(m, dtype, 100 + m)
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    pad = lambda a: np.concatenate([np.zeros(offset, a.dtype), a])  # bases one element off the allocation's alignment
    whole, dy = S.guarded(pad(y), tdtype, gpu)
    dx, dc = (torch.from_numpy(pad(a)).to(gpu) for a in (x, c))
    di = torch.from_numpy(pad(index)).to(gpu)
    s = 0.37
    ds = torch.tensor([s], dtype=torch.float64, device=gpu) if scaled else None
    before = whole.cpu().numpy().copy()
    k("fdd_shift_add_indexed" if dtype is np.float64 else "fdd_shift_add_indexed_f32", dy[offset:], dc[offset:], di[offset:], m, ds, dx[offset:], n)
    torch.cuda.synchronize()
    after = whole.cpu().numpy()
    first = 8 + offset
    want = before[first : first + n].copy()  # what the device held, bit for bit
    assert np.array_equal(want[index], y[index]) and np.signbit(want[np.setdiff1d(np.arange(n), index)[0]])
    xs = dtype(s) * x[index] if scaled else x[index]
    want[index] = y[index] + c * xs
    assert want.dtype == dtype
    assert np.array_equal(raw(after[first : first + n]), raw(want))
    assert np.array_equal(raw(after[:first]), raw(before[:first])) and np.array_equal(raw(after[first + n :]), raw(before[first + n :]))
    assert np.array_equal(dx.cpu().numpy(), pad(x)) and np.array_equal(dc.cpu().numpy(), pad(c)) and np.array_equal(di.cpu().numpy(), pad(index))


def test_an_index_outside_the_vector_is_skipped(gpu):
    n, index, y, x, c = data(65, np.float64, 7)
    index[3], index[-1] = -1, n
    whole, dy = S.guarded(y, torch.float64, gpu)
    k("fdd_shift_add_indexed", dy, torch.from_numpy(c).to(gpu), torch.from_numpy(index).to(gpu), 65, None, torch.from_numpy(x).to(gpu), n)
    torch.cuda.synchronize()
    ok = (index >= 0) & (index < n)
    want = y.copy()
    want[index[ok]] = y[index[ok]] + c[ok] * x[index[ok]]
    assert np.array_equal(raw(dy.cpu().numpy()), raw(want)) and S.guards_stand(whole)


def refused(name, *args):
    with pytest.raises(lib.FddError) as exc:
        k(name, *args)
    assert "failed with code -1:" in str(exc.value), str(exc.value)


def test_refusals_touch_nothing(gpu):
    n, m = 96, 12
    buf = torch.full((4 * n,), 5.0, dtype=torch.float64, device=gpu)
    A, Bo, dx, dc = buf[:n], buf[n // 2 : n // 2 + n], buf[2 * n : 3 * n], buf[3 * n : 3 * n + m]
    di = torch.arange(m, dtype=torch.int32, device=gpu)
    fbuf = torch.full((4 * n,), 5.0, dtype=torch.float32, device=gpu)
    FA, FB, fx, fc = fbuf[:n], fbuf[n // 2 : n // 2 + n], fbuf[2 * n : 3 * n], fbuf[3 * n : 3 * n + m]
    as_index = buf[: m // 2 + 1].view(torch.int32)[:m]  # an index list inside y
    for name, y, over, x, c, inside in (("fdd_shift_add_indexed", A, Bo, dx, dc, as_index), ("fdd_shift_add_indexed_f32", FA, FB, fx, fc, fbuf[:m].view(torch.int32))):
        refused(name, y, c, di, m, None, y, n)  # y is x
        refused(name, over, c, di, m, None, y, n)  # y overlaps x
        refused(name, y, y[n - m :], di, m, None, x, n)  # c_values inside y
        refused(name, y, c, inside, m, None, x, n)  # index inside y
        refused(name, y, c, di, -1, None, x, n)
        refused(name, y, c, di, m, None, x, -1)
        refused(name, y, c, di, n + 1, None, x, n)  # more entries than values
        refused(name, None, c, di, m, None, x, n)
        refused(name, y, None, di, m, None, x, n)
        refused(name, y, c, None, m, None, x, n)
        refused(name, y, c, di, m, None, None, n)
        k(name, None, None, None, 0, None, None, n)  # no entry: nothing to do, nothing read
        k(name, None, None, None, 0, None, None, 0)
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all()) and bool((fbuf == 5.0).all()) and bool((di == torch.arange(m, dtype=torch.int32, device=gpu)).all())
