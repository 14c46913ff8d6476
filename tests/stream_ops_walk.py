"""The bits of the streaming vector entries: every extern "C" entry of csrc/fdd_blas1.hip and csrc/fdd_reduce.hip (but
fdd_reduce_workspace_doubles) and fdd_cheby_step_f32, called at the smallest sizes at which one of their paths can go wrong,
one record per call.  `python tests/stream_ops_walk.py <libfdd_hip.so> gpu [--record FILE]` prints the records (or writes
FILE); tests/stream_ops_expected.tsv is that output of the library before each operation's arithmetic was stated once over
a lane accessor (csrc/fdd_stream.h), and tests/test_gpu_stream_ops_bits.py holds the package's library to it row for row.

A record is  entry/variant (empty: the row above's) <tab> n <tab> shifts <tab> results : reduction outputs and other device scalars as the hex of
their doubles, and one SHA-256 over the bytes of every vector the entry may write, guard elements in front and behind included.

  sizes    n = 1 (the tail alone), 2 (one pair), 3 (a pair and the tail), 515 (a second workgroup of pairs, and a tail)
  shifts   every size with all vector pointers aligned ("-") and with all of them one element further ("all+1": the
           one-element path); at n = 3 each vector pointer shifted alone ("name+1": one misaligned pointer must send the
           call to the one-element path, which the reductions' sums show); entries with float vectors at n = 515 also two
           elements further ("all+2": 8 bytes, enough for a pair of floats, not for four)
  options  every entry has a base case that gets all of the above (entries with m vectors: m = 5, every optional argument
           given); m = 1 and 8, every optional argument absent (scales, `last_dev` = m - 2, `q_is_zero`, `w`, `dst`), the
           solver's aliasings (dst == y, out == x, out == y, uv == u, r_out == r_in, r_kp1 == r_k, b[0] == a), the first,
           later (r_out == r_in) and last forms of the Chebyshev step beside its base case (the second step) and
           fdd_dom_lincomb_flexible_gamma on a slice of odd start, with v[0] = r_kp1 + slice_begin and on an empty slice
           run at n = 515, all aligned and all shifted
  past the grid cap (a second trip of the grid-stride loop; these and no others): fdd_vector_vector_addition at
           n = 2*256*32768 + 515, fdd_sub_inner_product and fdd_multi_axpy_norm2_scaled_dev (m = 2) at n = 2*256*2048 + 515

Inputs come from numpy.random.default_rng seeded by entry and n (the same for every shift); weights and diagonals lie in
[0.5, 1.5), the rest in [-1, 1); device scalars are fixed.  Every return code is checked and the walk stops at the first
error: nothing is launched after it.

mode cpu: the library is the CPU stand-in (tests/cpu_shim) on host memory, a rehearsal of the walk itself; entries it
lacks are recorded as "absent", and its reductions sum in another order than the GPU's.
"""
import ctypes
import hashlib
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F64, F32 = np.float64, np.float32
SEED = 18
SIZES = (1, 2, 3, 515)
EW_PAST_CAP = 2 * 256 * 32768 + 515   # kEwMaxBlocks workgroups of 256 lanes, two values each, and more
RED_PAST_CAP = 2 * 256 * 2048 + 515   # FDD_REDUCE_MAX_BLOCKS
MS = (1, 5, 8)
GUARD = 2          # elements behind every vector
GUARD_VALUE = -7.0
UNWRITTEN = 3.0    # what an output vector holds before the call
ALPHA, BETA, NUM, DEN, SCALE, S2, C_D, C_R, SIGN = 0.75, -1.25, 0.75, -1.5, 1.375, 2.5, 0.3125, 1.625, -1.0
COEFFS = [0.5 - 0.1875 * k for k in range(8)]
SCALES = [1.0 + 0.09375 * k for k in range(8)]


class HostMemory:
    def put(self, host):
        raw = np.empty(host.nbytes + 64, np.uint8)
        off = (-raw.ctypes.data) % 64
        a = raw[off:off + host.nbytes].view(host.dtype)
        a[:] = host
        return a, a.ctypes.data

    def get(self, keep):
        return keep

    def sync(self):
        pass


class DeviceMemory:
    def __init__(self):
        import torch

        assert torch.cuda.is_available(), "mode gpu needs a GPU"
        self.torch = torch

    def put(self, host):
        t = self.torch.from_numpy(host).cuda()
        assert t.data_ptr() % 64 == 0
        return t, t.data_ptr()

    def get(self, keep):
        return keep.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize()  # raises on an asynchronous HIP error: the walk ends there


class Buf:
    """`values` in memory the library can reach, `shift` elements behind an aligned address, guard elements around."""

    def __init__(self, mem, values, shift):
        self.mem, self.itemsize = mem, values.itemsize
        host = np.full(shift + len(values) + GUARD, GUARD_VALUE, values.dtype)
        host[shift:shift + len(values)] = values
        self.keep, base = mem.put(host)
        self.address = base + shift * self.itemsize

    def at(self, k):
        return ctypes.c_void_p(self.address + k * self.itemsize)

    def bytes(self):
        return self.mem.get(self.keep).tobytes()


class Absent(Exception):
    pass


class Case:
    def __init__(self, walk, label, n, shifts):
        self.w, self.label, self.n, self.shifts = walk, label, n, shifts
        self.rng = np.random.default_rng([SEED, zlib.crc32(label.split("/")[0].encode()), n])
        self.names, self.written, self.scalar_outs = [], [], []

    def _buf(self, name, values):
        self.names.append(name)
        shift = self.shifts.get(name, self.shifts.get("all", 0))
        return Buf(self.w.mem, values, shift)

    def vec(self, name, dtype=F64, positive=False, n=None):
        """an input vector"""
        v = self.rng.random(self.n if n is None else n)
        return self._buf(name, (v + 0.5 if positive else 2.0 * v - 1.0).astype(dtype))

    def io(self, name, dtype=F64, positive=False, n=None):
        """a vector the entry reads and writes"""
        b = self.vec(name, dtype, positive, n)
        self.written.append((name, b))
        return b

    def out(self, name, dtype=F64, n=None):
        """a vector the entry writes"""
        b = self._buf(name, np.full(self.n if n is None else n, UNWRITTEN, dtype))
        self.written.append((name, b))
        return b

    def dev(self, values):
        """device scalars: aligned, not a vector pointer"""
        return Buf(self.w.mem, np.asarray(values, F64), 0)

    def result(self, nv, name="out"):
        b = Buf(self.w.mem, np.full(nv, UNWRITTEN, F64), 0)
        self.scalar_outs.append((name, b, nv))
        return b

    def call(self, name, *args):
        fn = self.w.entry(name)
        if fn is None:
            raise Absent(name)
        conv, keep = [], []
        for a in args:
            if isinstance(a, Buf):
                conv.append(ctypes.c_void_p(a.address))
            elif isinstance(a, (list, tuple)):  # a host array of pointers
                arr = (ctypes.c_void_p * len(a))(*[x.address if isinstance(x, Buf) else x.value for x in a])
                keep.append(arr)
                conv.append(ctypes.cast(arr, ctypes.c_void_p))
            elif isinstance(a, np.ndarray):  # a host array of values
                keep.append(a)
                conv.append(ctypes.c_void_p(a.ctypes.data))
            else:
                conv.append(a)
        conv.append(None)  # the default stream
        rc = fn(*conv)
        if rc != 0:
            raise RuntimeError("%s returned %d at %s n=%d: %s" % (name, rc, self.label, self.n, self.w.last_error()))
        self.w.mem.sync()

    def record(self):
        parts = []
        for name, b, nv in self.scalar_outs:
            got = np.frombuffer(b.bytes(), F64)
            assert np.all(got[nv:] == GUARD_VALUE), (self.label, name, "wrote behind its %d values" % nv)
            parts.append("%s=%s" % (name, ",".join(float(x).hex() for x in got[:nv])))
        if self.written:
            h = hashlib.sha256()
            for name, b in self.written:
                h.update(b.bytes())
            parts.append("%s:%s" % ("+".join(name for name, b in self.written), h.hexdigest()))
        return " ".join(parts)


def shift_text(shifts):
    return ",".join("%s+%d" % kv for kv in shifts.items()) or "-"


# ---------------------------------------------------------------------------------------------------- the entries
# f(c, **options) builds its vectors in a fixed order and makes ONE call

def set_to_value(c, name="fdd_set_to_value", offset=None, dtype=F64):
    u = c.out("u", dtype, n=c.n + (offset or 0))
    c.call(name, u, ALPHA, c.n, *(() if offset is None else (offset,)))


def invert(c):
    c.call("fdd_invert_vector_elements", c.io("u", positive=True), c.n)


def axpby(c, alias=None):
    u, v = c.io("u"), c.vec("v")
    c.call("fdd_vector_vector_addition", u if alias else c.out("uv"), ALPHA, u, BETA, v, c.n)


def scaling(c, kind="value", alias=False):
    u = c.io("u")
    au = u if alias else c.out("au")
    if kind == "value":
        c.call("fdd_vector_scaling", au, ALPHA, u, c.n)
    elif kind == "dev":
        c.call("fdd_vector_scaling_dev", au, c.dev([SCALE]), u, c.n)
    else:
        c.call("fdd_vector_scaling_rsqrt_dev", au, c.dev([S2]), u, c.n)


def sqrt_sum(c):
    c.call("fdd_sqrt_sum_dev", c.result(1), c.dev([0.5 + 0.25 * k for k in range(c.n)]), c.n)


def ratio(c, name, alias=None):
    x, y = c.io("x"), c.io("y")
    c.call(name, {"x": x, "y": y}.get(alias) or c.out("out"), x, c.dev([NUM]), c.dev([DEN]), y, c.n)


def diagonal_scaling(c, scale=True):
    c.call("fdd_vector_diagonal_scaling_dev", c.out("z"), c.vec("d", positive=True), c.dev([SCALE]) if scale else None, c.vec("u"), c.n)


def cheby_step(c, step, name="fdd_cheby_step", dtype=F64):
    x = c.out("x", dtype) if step == "first" else c.io("x", dtype)
    d = {"first": c.out, "middle": c.io, "last": c.vec}[step]("d", dtype)
    r = c.io("r", dtype) if step == "middle" else c.vec("r", dtype)  # r_out == r_in, as the solver has it from the third step on
    q = None if step == "first" else c.vec("q", dtype)
    c.call(name, x, d, r if step == "middle" else None, r, q, c.vec("dinv", dtype, positive=True), C_D, C_R, int(step == "first"), int(step == "last"), c.n)


def cheby_step_apart(c, name="fdd_cheby_step", dtype=F64):  # the second step: r_in is the right-hand side, r_out its own vector
    c.call(name, c.io("x", dtype), c.io("d", dtype), c.out("r_out", dtype), c.vec("r_in", dtype), c.vec("q", dtype), c.vec("dinv", dtype, positive=True), C_D, C_R, 0, 0, c.n)


def initialize(c, name):
    c.call(name, c.out("u_k"), c.out("r_k"), c.vec("f"), c.n)


def update_ur(c, name, dev=False, alias=False):
    u, r = c.io("u_k"), c.io("r_k")
    alpha = (c.dev([NUM]), c.dev([DEN])) if dev else (ALPHA,)
    c.call(name, u, r if alias else c.out("r_kp1"), r, c.vec("p_k"), c.vec("q_k"), *alpha, c.n)


def update_pr(c, name, dev=False):
    beta = (c.dev([NUM]), c.dev([DEN])) if dev else (BETA,)
    c.call(name, c.io("p_k"), c.out("r_k"), c.vec("z_k"), c.vec("r_kp1"), *beta, c.n)


def copy(c, name, to, frm):
    c.call(name, c.out("u", to), c.vec("v", frm), c.n)


def multi_axpy(c, m):
    c.call("fdd_multi_axpy", c.io("q"), np.asarray(COEFFS[:m], F64), [c.vec("v%d" % k) for k in range(m)], m, c.n)


def multi_lincomb(c, name, m, scales=False, zero=None, last=None):
    q = c.io("q")
    v = [c.vec("v%d" % k) for k in range(m)]
    args = [q] + ([] if zero is None else [int(zero)]) + [c.dev(COEFFS[:m]), v]
    if name != "fdd_multi_axpy_dev":
        args.append(c.dev(SCALES[:m]) if scales else None)
    if last is not None:
        args.append(c.dev([m - 2.0]) if last else None)
    c.call(name, *args, m, c.n)


def scaled_residual(c):
    c.call("fdd_amg_main_scaled_residual", c.out("Sr"), c.out("w"), c.vec("f_m_Au"), c.vec("S", positive=True), ALPHA, c.n)


def smooth_start(c, name, dtype):
    c.call(name, c.out("work", dtype), c.out("Sr", dtype), c.vec("f", dtype), c.vec("D_val", dtype, positive=True), ALPHA, c.n)


def polynomial_evaluation(c):
    c.call("fdd_amg_main_polynomial_evaluation", c.out("w"), c.io("v"), c.vec("r"), c.vec("D_val", positive=True), ALPHA, c.n)


def update_field(c):
    c.call("fdd_amg_main_update_field", c.io("u"), c.vec("w"), c.vec("D_val", positive=True), c.n)


def vector_multiplication(c):
    c.call("fdd_amg_vector_multiplication", c.out("uv"), c.vec("u"), c.vec("v"), c.n)


def dot(c, name, vectors, nv=1, positive_last=False):
    vs = [c.vec(v, positive=positive_last and v == vectors[-1]) for v in vectors]
    c.call(name, c.result(nv), c.w.ws, *vs, c.n)


def lincomb_flexible_gamma(c, m, odd=False, v0_is_r1=False, scales=True, last=False, zero=False, empty=False):
    n = c.n
    begin = min(100 + odd, n - 1) if n > 3 else (1 if odd and n > 1 else 0)
    size = 0 if empty else (min(201, n - begin) if n > 3 else min(2, n - begin))
    r, r1, z = c.vec("r_k"), c.vec("r_kp1"), c.io("z_k")
    v = [c.vec("v%d" % k, n=max(size, 1)) for k in range(m)]
    if v0_is_r1:
        v[0] = r1.at(begin)
    c.call("fdd_dom_lincomb_flexible_gamma", c.result(2), c.w.ws, r, r1, z, n, begin, size, int(zero), c.dev(COEFFS[:m]), v, c.dev(SCALES[:m]) if scales else None,
           c.dev([m - 2.0]) if last else None, m)


def multi_dot(c, name, m, scales=False, weights=True, a_among_b=False, dtype=F64):
    a = c.vec("a", dtype)
    b = [c.vec("b%d" % k, dtype) for k in range(m)]
    if a_among_b:
        b[0] = a
    args = [c.result(m), c.w.ws, a, b]
    if "scaled" in name:
        args.append(c.dev(SCALES[:m]) if scales else None)
    args.append(m)
    if dtype is F64:
        args.append(c.vec("w", positive=True) if weights else None)
    c.call(name, *args, c.n)


def multi_axpy_norm(c, name, m, dst="y", scales=False, weights=True, dtype=F64):
    y = c.io("y", dtype)
    x = [c.vec("x%d" % k, dtype) for k in range(m)]
    args = [c.result(1), c.w.ws]
    if "scaled" in name:
        args.append(y if dst == "y" else c.out("dst", dtype) if dst == "apart" else None)
    args += [y, c.dev(COEFFS[:m]), SIGN, x]
    if "scaled" in name:
        args.append(c.dev(SCALES[:m]) if scales else None)
    args.append(m)
    if dtype is F64:
        args.append(c.vec("w", positive=True) if weights else None)
    c.call(name, *args, c.n)


def gather_weighted_norm2(c):  # rows of one to three boolean entries
    n = c.n
    lens = 1 + (np.arange(n) % 3)
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    col = c.rng.integers(0, 2 * n, size=int(ptr[-1])).astype(np.int32)
    c.call("fdd_gather_weighted_norm2", c.result(1), c.w.ws, Buf(c.w.mem, ptr, 0), Buf(c.w.mem, col, 0), c.vec("u", n=2 * n), c.vec("node_weight", positive=True), n)


def table():
    """(label, function, options, an entry's base case?, float vectors?).  A base case runs at every size and with each
    pointer shifted alone; a further option or m of the same entry at n = 515, all aligned and all shifted."""
    T = []

    def add(label, f, floats=False, **opts):
        T.append((label, f, opts, True, floats))

    def more(label, f, floats=False, **opts):
        T.append((label, f, opts, False, floats))

    add("fdd_set_to_value", set_to_value, offset=0)
    more("fdd_set_to_value/offset1", set_to_value, offset=1)
    add("fdd_amg_vector_set_to_value", set_to_value, name="fdd_amg_vector_set_to_value")
    add("fdd_amg_vector_set_to_value_f32", set_to_value, floats=True, name="fdd_amg_vector_set_to_value_f32", dtype=F32)
    add("fdd_invert_vector_elements", invert)
    add("fdd_vector_vector_addition", axpby)
    more("fdd_vector_vector_addition/uv=u", axpby, alias="u")
    add("fdd_vector_scaling", scaling)
    more("fdd_vector_scaling/au=u", scaling, alias=True)
    add("fdd_vector_scaling_dev", scaling, kind="dev")
    more("fdd_vector_scaling_dev/au=u", scaling, kind="dev", alias=True)
    add("fdd_vector_scaling_rsqrt_dev", scaling, kind="rsqrt")
    more("fdd_sqrt_sum_dev", sqrt_sum)
    for name, alias in (("fdd_xpby_ratio_dev", "y"), ("fdd_xmay_ratio_dev", "x")):
        add(name, ratio, name=name)
        more("%s/out=%s" % (name, alias), ratio, name=name, alias=alias)
    add("fdd_vector_diagonal_scaling_dev", diagonal_scaling)
    more("fdd_vector_diagonal_scaling_dev/noscale", diagonal_scaling, scale=False)
    for name, dtype in (("fdd_cheby_step", F64), ("fdd_cheby_step_f32", F32)):
        add(name + "/second", cheby_step_apart, floats=dtype is F32, name=name, dtype=dtype)
        for step in ("first", "middle", "last"):
            more("%s/%s" % (name, step), cheby_step, floats=dtype is F32, step=step, name=name, dtype=dtype)
    for name in ("fdd_dom_initialize_arrays", "fdd_sub_initialize_arrays"):
        add(name, initialize, name=name)
    for name in ("fdd_dom_solution_and_residual_update", "fdd_sub_solution_and_residual_update", "fdd_dom_solution_and_residual_update_dev"):
        add(name, update_ur, name=name, dev=name.endswith("_dev"))
        more(name + "/r_kp1=r_k", update_ur, name=name, dev=name.endswith("_dev"), alias=True)
    for name in ("fdd_dom_residual_and_search_update", "fdd_sub_residual_and_search_update", "fdd_dom_residual_and_search_update_dev"):
        add(name, update_pr, name=name, dev=name.endswith("_dev"))
    add("fdd_sub_copy_f64_f64", copy, name="fdd_sub_copy_f64_f64", to=F64, frm=F64)
    add("fdd_sub_copy_f32_f64", copy, floats=True, name="fdd_sub_copy_f32_f64", to=F32, frm=F64)
    add("fdd_sub_copy_f64_f32", copy, floats=True, name="fdd_sub_copy_f64_f32", to=F64, frm=F32)
    add("fdd_amg_main_scaled_residual", scaled_residual)
    add("fdd_amg_smooth_start", smooth_start, name="fdd_amg_smooth_start", dtype=F64)
    add("fdd_amg_smooth_start_f32", smooth_start, floats=True, name="fdd_amg_smooth_start_f32", dtype=F32)
    add("fdd_amg_main_polynomial_evaluation", polynomial_evaluation)
    add("fdd_amg_main_update_field", update_field)
    add("fdd_amg_vector_multiplication", vector_multiplication)
    for name, vectors, nv, positive_last in (
            ("fdd_dom_residual_norm", ("r_k", "QQt_r_k", "mask"), 1, True), ("fdd_dom_inner_product", ("u_k", "v_k", "mask"), 1, True),
            ("fdd_dom_projection_inner_products", ("z_k", "r_k", "p_k", "q_k"), 2, False), ("fdd_dom_inner_product_flexible", ("r_k", "r_kp1", "z_k"), 1, False),
            ("fdd_dom_inner_product_flexible_gamma", ("r_k", "r_kp1", "z_k"), 2, False), ("fdd_sub_inner_product", ("u", "v"), 1, False),
            ("fdd_sub_weighted_inner_product", ("u", "v", "w"), 1, True), ("fdd_sub_projection_inner_products", ("z_k", "r_k", "p_k", "q_k", "weight"), 2, True),
            ("fdd_sub_search_update_inner_product", ("r_k", "r_kp1", "z_k", "weight"), 1, True), ("fdd_amg_dot", ("x", "y"), 1, False)):
        add(name, dot, name=name, vectors=vectors, nv=nv, positive_last=positive_last)
    more("fdd_gather_weighted_norm2", gather_weighted_norm2)

    # the entries with m vectors: the base case at m = 5 with every optional argument given; m = 1 and 8, and each option the other way
    def with_m(label, f, floats=False, **opts):
        add(label + "/m5", f, floats=floats, m=5, **opts)
        more(label + "/m1", f, floats=floats, m=1, **opts)
        more(label + "/m8", f, floats=floats, m=8, **opts)

    with_m("fdd_multi_axpy", multi_axpy)
    with_m("fdd_multi_axpy_dev", multi_lincomb, name="fdd_multi_axpy_dev")
    with_m("fdd_multi_axpy_scaled_dev/scales", multi_lincomb, name="fdd_multi_axpy_scaled_dev", scales=True)
    more("fdd_multi_axpy_scaled_dev/m5", multi_lincomb, name="fdd_multi_axpy_scaled_dev", m=5)
    with_m("fdd_multi_lincomb_scaled_dev/scales", multi_lincomb, name="fdd_multi_lincomb_scaled_dev", scales=True, zero=False)
    more("fdd_multi_lincomb_scaled_dev/zero/m5", multi_lincomb, name="fdd_multi_lincomb_scaled_dev", m=5, zero=True)
    with_m("fdd_multi_lincomb_limited_dev/scales/last", multi_lincomb, name="fdd_multi_lincomb_limited_dev", scales=True, zero=False, last=True)
    more("fdd_multi_lincomb_limited_dev/scales/m5", multi_lincomb, name="fdd_multi_lincomb_limited_dev", m=5, scales=True, zero=False, last=False)
    more("fdd_multi_lincomb_limited_dev/last/zero/m5", multi_lincomb, name="fdd_multi_lincomb_limited_dev", m=5, zero=True, last=True)
    with_m("fdd_dom_lincomb_flexible_gamma/even", lincomb_flexible_gamma)
    more("fdd_dom_lincomb_flexible_gamma/odd/m5", lincomb_flexible_gamma, m=5, odd=True)
    more("fdd_dom_lincomb_flexible_gamma/even/v0=r1/m5", lincomb_flexible_gamma, m=5, v0_is_r1=True)
    more("fdd_dom_lincomb_flexible_gamma/odd/v0=r1/last/zero/m5", lincomb_flexible_gamma, m=5, odd=True, v0_is_r1=True, last=True, zero=True)
    more("fdd_dom_lincomb_flexible_gamma/even/noscales/last/m5", lincomb_flexible_gamma, m=5, scales=False, last=True)
    more("fdd_dom_lincomb_flexible_gamma/empty/m5", lincomb_flexible_gamma, m=5, empty=True)
    with_m("fdd_multi_weighted_inner_product", multi_dot, name="fdd_multi_weighted_inner_product")
    more("fdd_multi_weighted_inner_product/w=NULL/m5", multi_dot, name="fdd_multi_weighted_inner_product", m=5, weights=False)
    with_m("fdd_multi_weighted_inner_product_scaled/scales/b0=a", multi_dot, name="fdd_multi_weighted_inner_product_scaled", scales=True, a_among_b=True)
    more("fdd_multi_weighted_inner_product_scaled/w=NULL/m5", multi_dot, name="fdd_multi_weighted_inner_product_scaled", m=5, weights=False)
    with_m("fdd_multi_inner_product_scaled_f32/scales/b0=a", multi_dot, floats=True, name="fdd_multi_inner_product_scaled_f32", scales=True, a_among_b=True, dtype=F32)
    more("fdd_multi_inner_product_scaled_f32/m5", multi_dot, floats=True, name="fdd_multi_inner_product_scaled_f32", m=5, dtype=F32)
    with_m("fdd_multi_axpy_norm2_dev", multi_axpy_norm, name="fdd_multi_axpy_norm2_dev")
    more("fdd_multi_axpy_norm2_dev/w=NULL/m5", multi_axpy_norm, name="fdd_multi_axpy_norm2_dev", m=5, weights=False)
    for name, dtype in (("fdd_multi_axpy_norm2_scaled_dev", F64), ("fdd_multi_axpy_norm2_scaled_dev_f32", F32)):
        with_m(name + "/dst=apart/scales", multi_axpy_norm, floats=dtype is F32, name=name, dst="apart", scales=True, dtype=dtype)
        more(name + "/dst=y/scales/m5", multi_axpy_norm, floats=dtype is F32, name=name, m=5, dst="y", scales=True, dtype=dtype)
        more(name + "/dst=null/scales/m5", multi_axpy_norm, floats=dtype is F32, name=name, m=5, dst="null", scales=True, dtype=dtype)
        more(name + "/dst=y/w=NULL/m5", multi_axpy_norm, floats=dtype is F32, name=name, m=5, weights=False, dtype=dtype)
    return T


PAST_CAP = (
    ("fdd_vector_vector_addition", axpby, {}, EW_PAST_CAP),
    ("fdd_sub_inner_product", dot, {"name": "fdd_sub_inner_product", "vectors": ("u", "v")}, RED_PAST_CAP),
    ("fdd_multi_axpy_norm2_scaled_dev/m2/dst=y/scales", multi_axpy_norm, {"name": "fdd_multi_axpy_norm2_scaled_dev", "m": 2, "scales": True}, RED_PAST_CAP),
)


class Walk:
    def __init__(self, lib_path, mode):
        from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

        assert mode in ("cpu", "gpu"), mode
        self.mem = DeviceMemory() if mode == "gpu" else HostMemory()  # gpu: torch has loaded the HIP runtime before the library is
        self.cdll = ctypes.CDLL(lib_path, mode=ctypes.RTLD_GLOBAL)
        self.decls = lib.parse_header(os.path.join(lib.INCLUDE_DIR, "fdd_hip.h"))
        self.fns = {}
        self.ws = Buf(self.mem, np.zeros(8 * 2048, F64), 0)  # FDD_MULTI_MAX * FDD_REDUCE_MAX_BLOCKS doubles
        self.lines, self.last_label = [], None

    def entry(self, name):
        if name not in self.fns:
            fn = getattr(self.cdll, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = self.decls[name]
            self.fns[name] = fn
        return self.fns[name]

    def last_error(self):
        fn = self.cdll.fdd_last_error
        fn.restype = ctypes.c_char_p
        return (fn() or b"").decode()

    def one(self, label, f, opts, n, shifts):
        c = Case(self, label, n, shifts)
        try:
            f(c, **opts)
            text = c.record()
        except Absent:
            text = "absent"
        self.lines.append("%s\t%d\t%s\t%s" % ("" if label == self.last_label else label, n, shift_text(shifts), text))
        self.last_label = label
        return c.names

    def run(self):
        for label, f, opts, base, floats in table():
            for n in SIZES if base else SIZES[3:]:
                names = self.one(label, f, opts, n, {})
                self.one(label, f, opts, n, {"all": 1})
                if floats and n == SIZES[-1]:
                    self.one(label, f, opts, n, {"all": 2})
                if n == 3 and base:
                    for name in dict.fromkeys(names):
                        self.one(label, f, opts, n, {name: 1})
        for label, f, opts, n in PAST_CAP:
            self.one(label, f, opts, n, {})
            self.one(label, f, opts, n, {"all": 1})
        return self.lines


def main(argv):
    lib_path, mode = argv[0], argv[1]
    text = "\n".join(Walk(lib_path, mode).run()) + "\n"
    if "--record" in argv:
        with open(argv[argv.index("--record") + 1], "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
