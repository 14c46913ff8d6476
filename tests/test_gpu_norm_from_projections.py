"""The last Arnoldi step of an inner GMRES cycle with its norm taken from the projections (include/fdd_norm_estimate.h;
flag "last_norm_from_projections"): |q - sum h_k v_k|^2 = <q, q> - sum h_k^2 up to rounding while the difference keeps at
least 2^-10 of <q, q>, the exact pass behind a gate otherwise.

Kernel level: fdd_multi_weighted_inner_product_self, fdd_multi_axpy_norm2_scaled_gated_dev and fdd_gmres_step_last_dev
against the entries they stand beside (equal bits), against numpy in double, and against a Python restatement of the function
and of gmres_step_kernel.  n = 1, 2, 3, 513 and 2*2048*256 + 3 (every workgroup of the capped grid makes a second trip and
there is an odd tail), aligned pointers and one pointer offset by 8 bytes (the single-element path), m = 1..7, with and
without weights, with and without basis scales.

Solver level: box (4, 3, 3), degree 5, reduction 4, flag 1 against flag 0 -- the parent's sequence -- within 1e-12 where the
rounding differs and bit for bit where the flag must not reach.  The tolerance is the header's design bound: ten of 53 bits
lost leave 2^-43 ~ 1.1e-13 relative in the last norm of a cycle.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k, reduce_workspace
from test_gpu_kernels import _host_gmres_cycle

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
P = S._p
MMAX = 7  # FDD_MULTI_MAX - 1
SIZES = [1, 2, 3, 513, 2 * 2048 * 256 + 3]
SENTINEL = -7.25
GATED_LABEL = "reduce_vec2_gated_kernel<MultiAxpyNorm>"
EXACT_LABEL = "reduce_vec2_kernel<MultiAxpyNorm>"
FUSED_LABEL = "reduce_vec2_kernel<LincombFlexGamma>"


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def norm2_from_projections(aa, h):
    """fdd_norm2_from_projections in Python floats (IEEE doubles, every product rounded before it is subtracted)"""
    aa = float(aa)
    e = aa
    for x in h:
        hh = float(x) * float(x)
        e = e - hh
    finite = (aa - aa == 0.0) and (e - e == 0.0)
    return e, bool(finite and e >= aa * 2.0 ** -10)


_DATA = {}


def data(n):
    """per n, made once and never written: a generic vector, positive weights, MMAX vectors orthonormal in the weighted
    product (as far as n allows: at n < MMAX the trailing ones are only normalised), their scales, and noise"""
    if n not in _DATA:
        rng = np.random.default_rng(1000 + n)
        w = rng.uniform(0.5, 1.5, n)
        q = np.linalg.qr(rng.uniform(-1.0, 1.0, (n, MMAX)))[0] if n >= MMAX else rng.uniform(-1.0, 1.0, (n, MMAX))
        B = [np.ascontiguousarray(q[:, i]) for i in range(MMAX)]
        if n < MMAX:
            B = [b / np.sqrt((b * b).sum()) for b in B]
        _DATA[n] = {"a": rng.uniform(-1.0, 1.0, n), "w": w, "B": B, "scales": rng.uniform(0.5, 2.0, MMAX), "noise": rng.uniform(-1.0, 1.0, n)}
    return _DATA[n]


class Vectors:
    """the device copies of one (n, offset, weights, scales) setting: with offset 1 the vector `a` (and y) starts 8 bytes
    behind a 16-byte boundary, which sends every launch down the single-element path"""

    def __init__(self, gpu, n, offset, weights, scales):
        d = data(n)
        self.n, self.gpu = n, gpu
        self.w_h = d["w"] if weights else None
        self.s_h = d["scales"] if scales else None
        root = np.sqrt(d["w"]) if weights else 1.0
        self.b_h = [b / root for b in d["B"]]  # orthonormal in the product the entries form
        stored = [b / d["scales"][i] if scales else b for i, b in enumerate(self.b_h)]  # s_k * stored_k stands for b_k
        self.b_h = [(d["scales"][i] * x if scales else x) for i, x in enumerate(stored)]  # the values the kernel forms on load
        self.B = [dev(x, gpu) for x in stored]
        self.w = dev(d["w"], gpu) if weights else None
        self.s = dev(d["scales"], gpu) if scales else None
        self.offset = offset
        self.generic = self.place(d["a"])
        self.near_b0 = self.place(3.0 * self.b_h[0] + 1e-9 * d["noise"])

    def place(self, values):
        full = torch.zeros(self.n + self.offset + 2, dtype=torch.float64, device=self.gpu)
        view = full[self.offset : self.offset + self.n]
        view.copy_(dev(values, self.gpu))
        assert (view.data_ptr() % 16 == 8) == (self.offset == 1)
        return view


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_dots_with_the_self_product(gpu, n, offset):
    """out[0..m-1] have the bits of fdd_multi_weighted_inner_product_scaled, out[m] the bits of that entry on b[0] = a
    without a scale, and all of them are the sums numpy forms in double (1e-13 of the sum of the terms' magnitudes)"""
    ws = reduce_workspace(gpu)
    for weights in (False, True):
        for scales in (False, True):
            V = Vectors(gpu, n, offset, weights, scales)
            a = V.generic
            a_h, w_h = host(a), (V.w_h if weights else np.ones(n))
            self_ref = torch.full((8,), SENTINEL, dtype=torch.float64, device=gpu)
            k("fdd_multi_weighted_inner_product_scaled", self_ref, ws, a, [a], None, 1, V.w, n)
            for m in range(1, MMAX + 1):
                got = torch.full((10,), SENTINEL, dtype=torch.float64, device=gpu)
                ref = torch.full((10,), SENTINEL, dtype=torch.float64, device=gpu)
                k("fdd_multi_weighted_inner_product_self", got, ws, a, V.B[:m], V.s, m, V.w, n)
                k("fdd_multi_weighted_inner_product_scaled", ref, ws, a, V.B[:m], V.s, m, V.w, n)
                g, r = host(got), host(ref)
                case = (n, offset, weights, scales, m)
                assert np.array_equal(g[:m], r[:m]), case
                assert np.array_equal(g[m : m + 1], host(self_ref)[:1]), case
                assert np.all(g[m + 1 :] == SENTINEL), case  # m + 1 sums and not one word more
                for i in range(m):
                    assert abs(g[i] - (a_h * V.b_h[i] * w_h).sum()) <= 1e-13 * np.abs(a_h * V.b_h[i] * w_h).sum(), case
                assert abs(g[m] - (a_h * a_h * w_h).sum()) <= 1e-13 * (a_h * a_h * w_h).sum(), case


def test_dots_with_the_self_product_refuse_eight_vectors(gpu):
    ws = reduce_workspace(gpu)
    V = Vectors(gpu, 513, 0, False, False)
    out = torch.zeros(10, dtype=torch.float64, device=gpu)
    with pytest.raises(lib.FddError):
        k("fdd_multi_weighted_inner_product_self", out, ws, V.generic, V.B + [V.generic], None, 8, None, 513)
    with pytest.raises(lib.FddError):
        k("fdd_multi_axpy_norm2_scaled_gated_dev", out, ws, None, V.generic, out, -1.0, V.B + [V.generic], None, 8, None, 513, out)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_gated_norm_pass(gpu, n, offset):
    """Gate closed (orthonormal b, generic a: the function allows the estimate): out, dst and the workspace keep their
    sentinels.  Gate open (a = 3 b_0 + 1e-9 noise: est / aa < 2^-10): out and dst have the bits of the ungated entry.  Which
    of the two a launch must be is the Python restatement of the function on the entry's own dots; from n = 513 on the two
    constructions must give what they were built for."""
    for weights in (False, True):
        for scales in (False, True):
            V = Vectors(gpu, n, offset, weights, scales)
            for m in range(1, MMAX + 1):
                for name, y in (("closed", V.generic), ("open", V.near_b0)):
                    case = (n, offset, weights, scales, m, name)
                    ws = torch.full_like(reduce_workspace(gpu), SENTINEL)
                    dots = torch.full((10,), SENTINEL, dtype=torch.float64, device=gpu)
                    k("fdd_multi_weighted_inner_product_self", dots, ws, y, V.B[:m], V.s, m, V.w, n)
                    d = host(dots)
                    est, usable = norm2_from_projections(d[m], d[:m])
                    if name == "open":
                        assert not usable, case
                    elif n >= 513:
                        assert usable and est / d[m] > 0.5, case
                    for store in (False, True):
                        ws.fill_(SENTINEL)
                        out = torch.full((1,), SENTINEL, dtype=torch.float64, device=gpu)
                        dst = torch.full((n,), SENTINEL, dtype=torch.float64, device=gpu) if store else None
                        k("fdd_multi_axpy_norm2_scaled_gated_dev", out, ws, dst, y, dots, -1.0, V.B[:m], V.s, m, V.w, n, dots)
                        if usable:
                            assert host(out)[0] == SENTINEL and np.all(host(ws) == SENTINEL), case
                            assert dst is None or np.all(host(dst) == SENTINEL), case
                            continue
                        ref_out = torch.full((1,), SENTINEL, dtype=torch.float64, device=gpu)
                        ref_dst = torch.full((n,), SENTINEL, dtype=torch.float64, device=gpu) if store else None
                        k("fdd_multi_axpy_norm2_scaled_dev", ref_out, ws, ref_dst, y, dots, -1.0, V.B[:m], V.s, m, V.w, n)
                        assert np.array_equal(host(out).view(np.int64), host(ref_out).view(np.int64)), case
                        assert dst is None or np.array_equal(host(dst).view(np.int64), host(ref_dst).view(np.int64)), case
                        # and against numpy: the vector in the entry's own order of operations, its norm to reduction rounding
                        yy = host(y).copy()
                        for i in range(m):
                            yy = 1.0 * yy + (-1.0 * d[i]) * V.b_h[i]
                        assert dst is None or np.array_equal(host(dst), yy), case
                        terms = yy * yy * (V.w_h if weights else 1.0)
                        assert abs(host(out)[0] - terms.sum()) <= 1e-13 * terms.sum(), case


def fetch_counters(st, stream):
    e, x, r = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_double()
    lib.hip().call("fdd_gmres_fetch_norm_counters", vp(st.data_ptr()), ctypes.byref(e), ctypes.byref(x), ctypes.byref(r), stream)
    return e.value, x.value, r.value


@pytest.mark.parametrize("m", [1, 4, 7])
def test_last_step_on_device(gpu, m):
    """fdd_gmres_step_last_dev against gmres_step_kernel's Python restatement fed with the norm the function chooses, bit for
    bit on both branches, over cycles on one state: the estimate (the exact slot holds a NaN nobody may read), the fall-back
    below the bound, a negative difference, an infinite self product and an exact zero; the counters and the smallest ratio
    follow."""
    L = lib.hip()
    stream = lib.current_stream()
    rng = np.random.default_rng(40 + m)
    st = torch.zeros(L.raw("fdd_gmres_state_bytes")() // 8 + 1, dtype=torch.float64, device=gpu)
    counted, ratios = [0, 0], []
    keep = []
    for case in ("estimate", "below_bound", "negative", "infinite", "zero", "estimate"):
        cols = [np.concatenate([rng.uniform(-1, 1, j + 1), [rng.uniform(0.1, 1.0)]]) for j in range(m)]
        h = cols[m - 1][:m].copy()
        hh = float(sum(float(x) * float(x) for x in h))
        aa, exact = {"estimate": (hh + rng.uniform(0.5, 2.0), np.nan), "below_bound": (hh * (1.0 + 2.0 ** -12), 0.37), "negative": (0.5 * hh, 0.21),
                     "infinite": (np.inf, 0.4), "zero": (0.0, 0.3)}[case]
        if case == "zero":
            h[:] = 0.0
        est, usable = norm2_from_projections(aa, h)
        assert usable == (case in ("estimate", "zero"))
        cols[m - 1] = np.concatenate([h, [est if usable else exact]])
        y, hist, j_last, steps, conv = _host_gmres_cycle(3.7, cols, m, 0, 100, 1e-30, False)
        counted[0 if usable else 1] += 1
        with np.errstate(all="ignore"):
            ratio = float(np.float64(est) / np.float64(aa))
        if ratio == ratio:  # 0 / 0 and inf / inf are not recorded
            ratios.append(ratio)

        d_norm = dev(np.array([3.7]), gpu)
        L.call("fdd_gmres_begin_dev", vp(st.data_ptr()), vp(d_norm.data_ptr()), 1, stream)
        for j in range(m - 1):
            keep.append(dev(cols[j], gpu))
            L.call("fdd_gmres_step_dev", vp(st.data_ptr()), vp(keep[-1].data_ptr()), j, 0, 100, ctypes.c_double(1e-30), 0, stream)
        keep.append(dev(np.concatenate([h, [aa, exact]]), gpu))
        L.call("fdd_gmres_step_last_dev", vp(st.data_ptr()), vp(keep[-1].data_ptr()), m - 1, 0, 100, ctypes.c_double(1e-30), 0, stream)
        L.call("fdd_gmres_finish_dev", vp(st.data_ptr()), m, stream)
        gy, gh = np.zeros(8), np.zeros(9)
        nh, jl, stp, cv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.call("fdd_gmres_fetch", vp(st.data_ptr()), P(gy), P(gh), ctypes.byref(nh), ctypes.byref(jl), ctypes.byref(stp), ctypes.byref(cv), stream)
        assert (jl.value, stp.value, bool(cv.value), nh.value) == (j_last, steps, conv, len(hist)), case
        assert np.array_equal(gh[: nh.value], np.array(hist)), case
        # "zero" stops on alpha = 0 with a zero column: the back-substitution divides by it on both sides alike
        assert np.array_equal(gy[: j_last + 1], np.array(y), equal_nan=True) and not gy[j_last + 1 :].any(), case
        got = fetch_counters(st, stream)
        assert got[:2] == tuple(counted) and got[2] == min(ratios), (case, got, counted, ratios)
    with pytest.raises(lib.FddError):  # a slot has no room for column 7's three extra words
        L.call("fdd_gmres_step_last_dev", vp(st.data_ptr()), vp(keep[-1].data_ptr()), 7, 0, 100, ctypes.c_double(1e-30), 0, stream)


# ---------------------------------------------------------------- solver level
E, N, RED = (4, 3, 3), 5, 4
FLAG = "last_norm_from_projections"


@pytest.fixture(scope="module")
def setup(gpu):
    H.init(0)
    H.comm_single()
    H.set_print(False)
    return True


@pytest.fixture(scope="module")
def problem(setup):
    p = H.Problem.box(E, (1, 1, 1), N, RED, True)
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
    p.set_flag("sub_use_preconditioner", 0)
    p.amg_build()
    _, f = p.make_rhs_from(S.seeded_uniform(p.n, 2468))
    r = S.seeded_uniform(p.n, 5) - 0.5
    yield p, f, r
    p.close()


def configure(p, nv=4, it=4, slot=0):
    p.set_options(sub_num_vectors=nv, sub_max_iterations=it)
    p.set_flag("sub_use_preconditioner", slot)


def both_settings(p, r, what=None):
    """(flag 0, flag 1) of precond_apply -- or of what(p) --, and the counters' advance under flag 1"""
    out = []
    for flag in (0, 1):
        p.set_flag(FLAG, flag)
        before = p.inner_norm_counters()
        out.append(p.precond_apply(r, "gmres") if what is None else what(p))
        after = p.inner_norm_counters()
        moved = (after["estimated"] - before["estimated"], after["exact"] - before["exact"])
        if flag == 0:
            assert moved == (0, 0)
    p.set_flag(FLAG, 1)
    return out[0], out[1], moved, after["min_ratio"]


def close_to_parent(a, b, what):
    (z0, h0), (z1, h1) = a, b
    dz, dh = np.abs(z1 - z0).max() / np.abs(z0).max(), (np.abs(h1 - h0).max() / h0[0] if len(h0) == len(h1) else np.inf)
    print("%s: max|z1 - z0| / max|z0| = %.3e, max|hist1 - hist0| / hist0[0] = %.3e" % (what, dz, dh))
    assert len(h0) == len(h1), what
    assert dz <= 1e-12 and dh <= 1e-12, (what, dz, dh)


@pytest.mark.parametrize("nv,it", [(1, 1), (2, 5), (4, 4), (7, 7)])
def test_preconditioner_stays_within_rounding_of_the_parent(problem, nv, it):
    p, f, r = problem
    configure(p, nv, it)
    a, b, moved, ratio = both_settings(p, r)
    print("GMRES(%d) x %d: last steps (estimated, exact) = %s, smallest est/aa so far %.3e" % (nv, it, moved, ratio))
    assert 1 <= moved[0] + moved[1] <= -(-it // nv)  # one last step per cycle enqueued, fewer only if the solve stops early
    close_to_parent(a, b, "GMRES(%d) x %d" % (nv, it))


def test_outer_solve_keeps_its_iteration_count(problem):
    p, f, r = problem
    configure(p)
    (u0, its0, hist0), (u1, its1, hist1), moved, _ = both_settings(p, r, lambda q: q.solve(f, "fcg"))
    print("fcg: %d / %d iterations, last steps (estimated, exact) = %s, max|u1 - u0| / max|u0| = %.3e" % (its0, its1, moved, np.abs(u1 - u0).max() / np.abs(u0).max()))
    assert its0 == its1 and moved[0] + moved[1] >= its1


@pytest.mark.parametrize("setting", ["eight_vectors", "float_inner_solve"])
def test_the_flag_does_not_reach_the_old_paths(problem, setting):
    """GMRES(8) (a slot has no room for the ninth sum) and the float inner solve keep every bit and count nothing"""
    p, f, r = problem
    configure(p, 8, 8) if setting == "eight_vectors" else configure(p)
    if setting == "float_inner_solve":
        p.set_flag("preconditioner_precision", 32)
    try:
        (z0, h0), (z1, h1), moved, _ = both_settings(p, r)
        assert moved == (0, 0) and np.array_equal(z0, z1) and np.array_equal(h0, h1)
    finally:
        p.set_flag("preconditioner_precision", 64)


@pytest.mark.parametrize("other", ["device_bookkeeping", "skip_last_basis_store"])
def test_the_other_switches_keep_their_bits_with_the_flag_on(problem, other):
    """host against device bookkeeping, and the last basis vector stored or not: which norm the last step takes depends on
    the flag alone, so each pair still agrees bit for bit"""
    p, f, r = problem
    configure(p)
    p.set_flag(FLAG, 1)
    got = {}
    try:
        for value in (0, 1):
            p.set_flag(other, value)
            before = p.inner_norm_counters()
            got[value] = (p.precond_apply(r, "gmres"), p.sub_dof_solve(p.sub_dof_rhs(r)))
            after = p.inner_norm_counters()
            assert after["estimated"] + after["exact"] - before["estimated"] - before["exact"] == 2, (other, value)
    finally:
        p.set_flag(other, 1)
    assert np.array_equal(got[0][0][0], got[1][0][0]) and np.array_equal(got[0][0][1], got[1][0][1]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("slot", [1, 2])
def test_with_a_preconditioner_in_the_slot(problem, slot):
    """the V-cycle (1) and point-Jacobi (2) inside the inner solve: the Arnoldi basis is orthonormal there as well"""
    p, f, r = problem
    configure(p, 4, 4, slot)
    try:
        a, b, moved, ratio = both_settings(p, r)
        print("slot %d: last steps (estimated, exact) = %s, smallest est/aa so far %.3e" % (slot, moved, ratio))
        assert moved[0] + moved[1] == 1
        close_to_parent(a, b, "slot %d" % slot)
    finally:
        p.set_flag("sub_use_preconditioner", 0)


def labels_of_steps(p, steps):
    """the profile labels of `steps` outer iterations"""
    lib.host().call("fddh_profile_enable", 1)
    p.pcg_steps(steps)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.host().call("fddh_profile_collect", buf, len(buf))
    lib.host().call("fddh_profile_enable", 0)
    return set(json.loads(buf.value.decode()))


def test_lazy_steps_take_the_gated_pass_without_a_synchronisation(problem):
    """three lazy outer steps: one estimate per application of the preconditioner and no fall-back; the gated launch is in the
    sequence and the deferred update, which only the lazy single cycle hands over, still is -- nothing waits on the host.
    With the flag at 0 the gated launch is gone and nothing is counted."""
    p, f, r = problem
    configure(p)
    try:
        for flag in (1, 0):
            p.set_flag(FLAG, flag)
            p.pcg_begin(f)
            p.pcg_steps(1)
            before = p.inner_norm_counters()
            labels = labels_of_steps(p, 3)
            after = p.inner_norm_counters()
            moved = (after["estimated"] - before["estimated"], after["exact"] - before["exact"])
            assert moved == ((3, 0) if flag else (0, 0)), (flag, moved)
            assert (GATED_LABEL in labels) == (flag == 1), (flag, sorted(labels))
            assert FUSED_LABEL in labels and EXACT_LABEL in labels, (flag, sorted(labels))  # lazy path; steps 0..2 keep the exact pass
    finally:
        p.set_flag(FLAG, 1)
