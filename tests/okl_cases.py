"""The reference's OKL kernels, case by case: ONE closed table that names, per row, the reference kernel file and
kernel(s), the `orc_*` restatement in oracle/ and the HIP entries that the kernel-level GPU tests hold bit for bit to
that restatement (test_gpu_kernels.py, test_gpu_kernels_f32.py, test_gpu_persistent_trips.py).

Three sides run the same inputs:
  ref   code compiled from the reference's own kernel files (oracle/_ref/libokl_*.so, `make -C oracle ref`: the four
        OKL files rewritten to their OCCA-Serial loop nests by oracle/okl_serial.sed, g++ -O2 -ffp-contract=off)
  orc   oracle/_build/libfdd_oracle.so, the hand restatement
  hip   libfdd_hip.so on the GPU
and every output array is identified by the SHA-256 of its bytes.  tests/golden/okl_kernels.json records the `ref`
hashes (tests/golden/make_okl_golden.py); test_cpu_okl_reference.py holds `orc` to them and test_gpu_okl_reference.py
holds `hip` to them, so both are pinned to reference-compiled code and not to each other.

Inputs come from the integer generator below, written out here so that the recorded hashes depend on no library's
random numbers: multiples of 2^-20 in (-1, 1), exact in double and in float.

Not in the table (the only exclusions):
  * the float builds of the eight block reductions: the float inner solve of this project keeps DOUBLE accumulators
    over float data (documented deviation, oracle/fdd_oracle_f32.c:15-18), so there is no float restatement to hold;
  * AMG/kernels.cu: `<<< >>>` launches need a device compiler, and its five bodies are one-line element-wise statements.
Float kernels without an `orc_f32_*` twin (set_to_value, invert_vector_elements, the fused vector updates, the three
restrictions with DType = float) have no row of their own: the product never runs them in float.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import zlib

import numpy as np

import support as S

GOLDEN = os.path.join(S.GOLDEN_DIR, "okl_kernels.json")

vp = ctypes.c_void_p
c_double, c_float = ctypes.c_double, ctypes.c_float
f32, f64 = np.float32, np.float64
BLOCK = 128                             # config.hpp:38-40
SUB_DEGREES = list(range(15, 0, -1))    # the POLY_DEGREE table of the reference-compiled subdomain libraries: level l is degree 15 - l

# reference-compiled library -> the kernel file it is built from (oracle/Makefile, target ref)
REF_LIBS = {
    "domain_d2_f64": "domain.okl", "domain_d3_f64": "domain.okl",
    "subdomain_d2_f64": "subdomain.okl", "subdomain_d3_f64": "subdomain.okl", "subdomain_d2_f32": "subdomain.okl", "subdomain_d3_f32": "subdomain.okl",
    "math_f64": "math.okl", "math_f32": "math.okl",
    "csr_matrix_f64": "csr_matrix.okl", "csr_matrix_f32": "csr_matrix.okl",
}


def ref_built():
    return all(os.path.exists(S.okl_ref_so(t)) for t in REF_LIBS)


ref_lib = S.okl_ref_lib


# ------------------------------------------------------------------ inputs
def draws(n, label):
    """n integers in [-(2^20 - 1), 2^20 - 1]: SplitMix64 of the counters 1..n on a stream named by `label` (64-bit
    integer arithmetic with wrap-around, the top 21 bits of each word)."""
    stream = (zlib.crc32(label.encode()) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(stream)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(43)).astype(np.int64) % (2**21 - 1) - (2**20 - 1)


def unit(n, label, dtype=f64):
    """multiples of 2^-20 in (-1, 1)"""
    return (draws(n, label) * 2.0**-20).astype(dtype)


def nonzero_unit(n, label, dtype=f64):
    d = draws(n, label)
    return (np.where(d == 0, 1, d) * 2.0**-20).astype(dtype)


def positive(n, label, dtype=f64):
    """multiples of 2^-22 in (0.25, 0.75): exact in float as well"""
    return (0.5 + 0.25 * unit(n, label)).astype(dtype)


def factors(npts, label, dim, dtype=f64):
    """six geometric factor arrays: the diagonal ones positive, the cross terms (G[3..5]; G[2] in 2-D) non-zero"""
    diag = range(dim)
    return [positive(npts, "%s/G%d" % (label, g), dtype) if g in diag else (0.25 * nonzero_unit(npts, "%s/G%d" % (label, g))).astype(dtype) for g in range(6)]


def P(a):
    return vp(a.ctypes.data)


def ptrs(arrays):
    return (vp * len(arrays))(*[a.ctypes.data for a in arrays])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def num_blocks(n):
    return (n + BLOCK - 1) // BLOCK


class Case:
    """One run of a row's kernel(s): `id`, the reference-compiled library it runs in and the parameters."""

    def __init__(self, id, lib, **params):
        self.id, self.lib, self.p = id, lib, params

    def __repr__(self):
        return self.id


class Row:
    """A table row.  Subclasses state: source (kernel file), kernels, orc (restatements), hip_forms (tuples of HIP entry
    names that together restate the row: a two-launch form is one tuple, a fused form another), cases, and
    inputs(case) -> dict, ref(lib, case, x) / run_orc(L, case, x) / run_hip(form, case, x, T) -> {output name: array}.
    run_orc and run_hip may return a subset of the reference's outputs (a fused kernel stores no intermediates)."""

    source = None
    kernels = ()
    orc = ()
    hip_forms = ()
    cases = ()

    def forms(self, case):
        return self.hip_forms


# ------------------------------------------------------------------ stiffness
class DomStiffness(Row):
    source, kernels = "domain.okl", ("stiffness_matrix_1", "stiffness_matrix_2")
    orc = ("orc_dom_stiffness_matrix_1", "orc_dom_stiffness_matrix_2")
    hip_forms = (("fdd_dom_stiffness_matrix_1", "fdd_dom_stiffness_matrix_2"), ("fdd_dom_stiffness_matrix",), ("fdd_sub_stiffness_matrix",), ("fdd_sub_stiffness_matrix_gather",), ("fdd_stiffness_matrix_2d",))
    cases = [Case("dom_stiffness/3d/N%d" % N, "domain_d3_f64", dim=3, N=N, E=3) for N in range(1, 16)] + [Case("dom_stiffness/2d/N%d" % N, "domain_d2_f64", dim=2, N=N, E=3) for N in (1, 5, 7, 15)]

    def forms(self, case):
        two_launch = self.hip_forms[0]
        return (two_launch,) + (self.hip_forms[1:4] if case.p["dim"] == 3 else self.hip_forms[4:])

    def inputs(self, case):
        dim, N, E = case.p["dim"], case.p["N"], case.p["E"]
        n = N + 1
        npts = E * n**dim
        return {"u": unit(npts, case.id + "/u"), "D": unit(n * n, case.id + "/D"), "G": factors(npts, case.id, dim), "npts": npts}

    def ref(self, lib, case, x):
        dim, N, npts = case.p["dim"], case.p["N"], x["npts"]
        GDu = [np.zeros(npts) for _ in range(3)]
        Au = np.zeros(npts)
        lib.stiffness_matrix_1(ptrs(GDu), P(x["u"]), P(x["D"]), ptrs(x["G"]), npts, N)
        lib.stiffness_matrix_2(P(Au), ptrs(GDu), P(x["D"]), npts, N)
        return dict([("GDu%d" % d, GDu[d]) for d in range(dim)] + [("Au", Au)])

    def run_orc(self, L, case, x):
        dim, N, npts = case.p["dim"], case.p["N"], x["npts"]
        GDu = [np.zeros(npts) for _ in range(3)]
        Au = np.zeros(npts)
        L.orc_dom_stiffness_matrix_1(ptrs(GDu), P(x["u"]), P(x["D"]), ptrs(x["G"]), npts, N, dim)
        L.orc_dom_stiffness_matrix_2(P(Au), ptrs(GDu), P(x["D"]), npts, N, dim)
        return dict([("GDu%d" % d, GDu[d]) for d in range(dim)] + [("Au", Au)])

    def run_hip(self, form, case, x, T):
        dim, N, E, npts = case.p["dim"], case.p["N"], case.p["E"], x["npts"]
        du, dD, dG = T.dev(x["u"]), T.dev(x["D"]), [T.dev(g) for g in x["G"]]
        dAu = T.full(npts, 3.0)
        if len(form) == 2:
            dGDu = [T.full(npts, 3.0) for _ in range(3)]
            T.k(form[0], dGDu, du, dD, dG, npts, N, dim)
            T.k(form[1], dAu, dGDu, dD, npts, N, dim)
            return dict([("GDu%d" % d, T.host(dGDu[d])) for d in range(dim)] + [("Au", T.host(dAu))])
        if form[0] == "fdd_dom_stiffness_matrix":
            T.k(form[0], dAu, du, dD, dG, E, N)
        elif form[0] == "fdd_sub_stiffness_matrix_gather":
            T.k(form[0], dAu, du, T.dev(np.arange(npts, dtype=np.int32)), dD, dG, None, E, N)
        else:  # fdd_sub_stiffness_matrix, fdd_stiffness_matrix_2d: the elements through an offset list in reverse order
            eo = (np.arange(E)[::-1] * (N + 1) ** dim).astype(np.int32)
            T.k(form[0], dAu, du, dD, dG, T.dev(eo), E, N)
        return {"Au": T.host(dAu)}


MIXED_DEGREES = [7, 1, 15, 3, 5, 1, 7, 5, 3]  # nine elements over the levels of degree 15, 7, 5, 3, 1, shuffled


def element_list(degrees, dim):
    """offset, vert and level of every point of a Subdomain element list (subdomain.tpp:558-566, 1603-1630)"""
    offset, vert, level, starts = [], [], [], []
    o = 0
    for d in degrees:
        m = (d + 1) ** dim
        starts.append(o)
        offset.append(np.full(m, o, np.int32))
        vert.append(np.arange(m, dtype=np.int32))
        level.append(np.full(m, SUB_DEGREES.index(d), np.int32))
        o += m
    return np.concatenate(offset), np.concatenate(vert), np.concatenate(level), starts, o


class SubStiffness(Row):
    source, kernels = "subdomain.okl", ("stiffness_matrix_1", "stiffness_matrix_2")
    orc = ("orc_sub_stiffness_matrix_1", "orc_sub_stiffness_matrix_2")
    hip_forms = (("fdd_sub_stiffness_matrix_1", "fdd_sub_stiffness_matrix_2"), ("fdd_sub_stiffness_matrix",), ("fdd_stiffness_matrix_2d",))
    cases = [Case("sub_stiffness/3d/mixed", "subdomain_d3_f64", dim=3), Case("sub_stiffness/2d/mixed", "subdomain_d2_f64", dim=2)]

    def forms(self, case):
        return (self.hip_forms[0], self.hip_forms[1] if case.p["dim"] == 3 else self.hip_forms[2])

    def inputs(self, case):
        dim = case.p["dim"]
        offset, vert, level, starts, npts = element_list(MIXED_DEGREES, dim)
        D = [unit((d + 1) ** 2, "%s/D%d" % (case.id, d)) for d in SUB_DEGREES]
        return {"offset": offset, "vert": vert, "level": level, "starts": starts, "npts": npts, "D": D, "u": unit(npts, case.id + "/u"), "G": factors(npts, case.id, dim)}

    def ref(self, lib, case, x):
        dim, npts = case.p["dim"], x["npts"]
        GDu = [np.zeros(npts) for _ in range(3)]
        Au = np.zeros(npts)
        lib.stiffness_matrix_1(ptrs(GDu), P(x["u"]), ptrs(x["D"]), P(x["offset"]), P(x["vert"]), P(x["level"]), ptrs(x["G"]), npts)
        lib.stiffness_matrix_2(P(Au), ptrs(GDu), ptrs(x["D"]), P(x["offset"]), P(x["vert"]), P(x["level"]), npts)
        return dict([("GDu%d" % d, GDu[d]) for d in range(dim)] + [("Au", Au)])

    def run_orc(self, L, case, x):
        dim, npts = case.p["dim"], x["npts"]
        GDu = [np.zeros(npts) for _ in range(3)]
        Au = np.zeros(npts)
        pd = (ctypes.c_int * len(SUB_DEGREES))(*SUB_DEGREES)
        L.orc_sub_stiffness_matrix_1(ptrs(GDu), P(x["u"]), ptrs(x["D"]), P(x["offset"]), P(x["vert"]), P(x["level"]), pd, ptrs(x["G"]), npts, dim)
        L.orc_sub_stiffness_matrix_2(P(Au), ptrs(GDu), ptrs(x["D"]), P(x["offset"]), P(x["vert"]), P(x["level"]), pd, npts, dim)
        return dict([("GDu%d" % d, GDu[d]) for d in range(dim)] + [("Au", Au)])

    def run_hip(self, form, case, x, T):
        dim, npts = case.p["dim"], x["npts"]
        du, dD, dG = T.dev(x["u"]), [T.dev(d) for d in x["D"]], [T.dev(g) for g in x["G"]]
        dAu = T.full(npts, 3.0)
        if len(form) == 2:
            pd = (ctypes.c_int * len(SUB_DEGREES))(*SUB_DEGREES)
            doff, dvert, dlev = T.dev(x["offset"]), T.dev(x["vert"]), T.dev(x["level"])
            dGDu = [T.full(npts, 3.0) for _ in range(3)]
            T.k(form[0], dGDu, du, dD, doff, dvert, dlev, pd, len(SUB_DEGREES), dG, npts, dim)
            T.k(form[1], dAu, dGDu, dD, doff, dvert, dlev, pd, len(SUB_DEGREES), npts, dim)
            return dict([("GDu%d" % d, T.host(dGDu[d])) for d in range(dim)] + [("Au", T.host(dAu))])
        for d in sorted(set(MIXED_DEGREES)):  # level-sorted fused form: one launch per level over that level's elements
            eo = np.array([s for s, deg in zip(x["starts"], MIXED_DEGREES) if deg == d], np.int32)
            T.k(form[0], dAu, du, dD[SUB_DEGREES.index(d)], dG, T.dev(eo), len(eo), d)
        return {"Au": T.host(dAu)}


class SubStiffnessF32(Row):
    """subdomain.okl with DType = float at one degree; orc_f32_sub_stiffness and the HIP entry are the fused forms
    (the gather through an identity index, no scale)"""
    source, kernels = "subdomain.okl", ("stiffness_matrix_1", "stiffness_matrix_2")
    orc = ("orc_f32_sub_stiffness",)
    hip_forms = (("fdd_sub_stiffness_matrix_gather_scaled_f32",),)
    cases = [Case("sub_stiffness_f32/3d/N%d" % N, "subdomain_d3_f32", N=N, E=3) for N in (3, 7)]

    def inputs(self, case):
        N, E = case.p["N"], case.p["E"]
        offset, vert, level, _, npts = element_list([N] * E, 3)
        D = [unit((d + 1) ** 2, "%s/D%d" % (case.id, d), f32) for d in SUB_DEGREES]
        return {"offset": offset, "vert": vert, "level": level, "npts": npts, "D": D, "u": unit(npts, case.id + "/u", f32), "G": factors(npts, case.id, 3, f32)}

    def ref(self, lib, case, x):
        npts = x["npts"]
        GDu = [np.zeros(npts, f32) for _ in range(3)]
        Au = np.zeros(npts, f32)
        lib.stiffness_matrix_1(ptrs(GDu), P(x["u"]), ptrs(x["D"]), P(x["offset"]), P(x["vert"]), P(x["level"]), ptrs(x["G"]), npts)
        lib.stiffness_matrix_2(P(Au), ptrs(GDu), ptrs(x["D"]), P(x["offset"]), P(x["vert"]), P(x["level"]), npts)
        return {"GDu0": GDu[0], "GDu1": GDu[1], "GDu2": GDu[2], "Au": Au}

    def run_orc(self, L, case, x):
        N, E = case.p["N"], case.p["E"]
        Au = np.zeros(x["npts"], f32)
        L.orc_f32_sub_stiffness(P(Au), P(x["u"]), None, None, P(x["D"][SUB_DEGREES.index(N)]), ptrs(x["G"]), E, N)
        return {"Au": Au}

    def run_hip(self, form, case, x, T):
        N, E, npts = case.p["N"], case.p["E"], x["npts"]
        dAu = T.full(npts, 3.0, f32)
        T.k(form[0], dAu, T.dev(x["u"]), None, T.dev(np.arange(npts, dtype=np.int32)), T.dev(x["D"][SUB_DEGREES.index(N)]), [T.dev(g) for g in x["G"]], None, E, N)
        return {"Au": T.host(dAu)}


# ------------------------------------------------------------------ restriction
class Restriction(Row):
    source, kernels = "subdomain.okl", ("restriction_1", "restriction_2", "restriction_3")
    orc = ("orc_sub_restriction_1", "orc_sub_restriction_2", "orc_sub_restriction_3")
    hip_forms = (("fdd_sub_restriction_1", "fdd_sub_restriction_2", "fdd_sub_restriction_3"), ("fdd_sub_restriction",), ("fdd_sub_restriction_2d",))
    # (n_f, n_c): the level pairs of the reference's degree lists
    cases = [Case("restriction/3d/%d_%d" % nn, "subdomain_d3_f64", dim=3, n_f=nn[0], n_c=nn[1], E=5) for nn in ((8, 2), (8, 6), (8, 5), (8, 4), (6, 4), (5, 3), (4, 2), (3, 2), (2, 2), (16, 10), (16, 2))] + [
        Case("restriction/2d/%d_%d" % nn, "subdomain_d2_f64", dim=2, n_f=nn[0], n_c=nn[1], E=5) for nn in ((8, 4), (6, 5), (16, 8))]

    def forms(self, case):
        return (self.hip_forms[0], self.hip_forms[1] if case.p["dim"] == 3 else self.hip_forms[2])

    def inputs(self, case):
        dim, n_f, n_c, E = (case.p[key] for key in ("dim", "n_f", "n_c", "E"))
        sizes = [E * n_f ** (dim - s) * n_c**s for s in range(dim + 1)]  # fine, after each launch ..., coarse
        return {"J": unit(n_f * n_c, case.id + "/J"), "u": unit(sizes[0], case.id + "/u"), "sizes": sizes}

    def _names(self, dim):
        return ["Ju_1", "Ju_2", "Ju_3"][: dim - 1] + ["u_c"]

    def ref(self, lib, case, x):
        dim, n_f, n_c = case.p["dim"], case.p["n_f"], case.p["n_c"]
        out, src = {}, x["u"]
        for s, name in enumerate(self._names(dim)):
            dst = np.zeros(x["sizes"][s + 1])
            getattr(lib, "restriction_%d" % (s + 1))(P(dst), P(x["J"]), P(src), len(dst), n_f, n_c)
            out[name] = src = dst
        return out

    def run_orc(self, L, case, x):
        dim, n_f, n_c = case.p["dim"], case.p["n_f"], case.p["n_c"]
        out, src = {}, x["u"]
        for s, name in enumerate(self._names(dim)):
            dst = np.zeros(x["sizes"][s + 1])
            if s < 2:
                getattr(L, "orc_sub_restriction_%d" % (s + 1))(P(dst), P(x["J"]), P(src), len(dst), n_f, n_c, dim)
            else:
                L.orc_sub_restriction_3(P(dst), P(x["J"]), P(src), len(dst), n_f, n_c)
            out[name] = src = dst
        return out

    def run_hip(self, form, case, x, T):
        dim, n_f, n_c, E = (case.p[key] for key in ("dim", "n_f", "n_c", "E"))
        dJ, du = T.dev(x["J"]), T.dev(x["u"])
        if len(form) == 1:
            dc = T.full(x["sizes"][-1], 3.0)
            T.k(form[0], dc, dJ, du, E, n_f, n_c)
            return {"u_c": T.host(dc)}
        out, src = {}, du
        for s, name in enumerate(self._names(dim)):
            dst = T.full(x["sizes"][s + 1], 3.0)
            if s < 2:
                T.k(form[s], dst, dJ, src, x["sizes"][s + 1], n_f, n_c, dim)
            else:
                T.k(form[s], dst, dJ, src, x["sizes"][s + 1], n_f, n_c)
            out[name] = T.host(dst)
            src = dst
        return out


# ------------------------------------------------------------------ vector kernels
VECTOR_SIZES = (1, 127, 128, 129, 1000)


class SetToValue(Row):
    source, kernels, orc, hip_forms = "math.okl", ("set_to_value",), ("orc_set_to_value",), (("fdd_set_to_value",),)
    cases = [Case("set_to_value/n%d/offset%d" % (n, o), "math_f64", n=n, offset=o) for n in VECTOR_SIZES for o in (0, 1)]
    alpha = 0.375

    def inputs(self, case):
        return {"u": unit(case.p["n"] + case.p["offset"] + 3, case.id + "/u")}

    def ref(self, lib, case, x):
        u = x["u"].copy()
        lib.set_to_value(P(u), c_double(self.alpha), case.p["n"], case.p["offset"])
        return {"u": u}

    def run_orc(self, L, case, x):
        u = x["u"].copy()
        L.orc_set_to_value(P(u), c_double(self.alpha), case.p["n"], case.p["offset"])
        return {"u": u}

    def run_hip(self, form, case, x, T):
        du = T.dev(x["u"])
        T.k(form[0], du, self.alpha, case.p["n"], case.p["offset"])
        return {"u": T.host(du)}


class Invert(Row):
    source, kernels, orc, hip_forms = "math.okl", ("invert_vector_elements",), ("orc_invert_vector_elements",), (("fdd_invert_vector_elements",),)
    cases = [Case("invert/n%d" % n, "math_f64", n=n) for n in VECTOR_SIZES]

    def inputs(self, case):
        return {"u": 1.5 + 0.5 * unit(case.p["n"], case.id + "/u")}

    def ref(self, lib, case, x):
        u = x["u"].copy()
        lib.invert_vector_elements(P(u), case.p["n"])
        return {"u": u}

    def run_orc(self, L, case, x):
        u = x["u"].copy()
        L.orc_invert_vector_elements(P(u), case.p["n"])
        return {"u": u}

    def run_hip(self, form, case, x, T):
        du = T.dev(x["u"])
        T.k(form[0], du, case.p["n"])
        return {"u": T.host(du)}


class Axpby(Row):
    """uv = alpha u + beta v; `uv` a third vector, u itself or v itself (domain.tpp:767)"""
    source, kernels = "math.okl", ("vector_vector_addition",)
    orc, hip_forms = ("orc_vector_vector_addition",), (("fdd_vector_vector_addition",),)
    dtype, scalar, fn = f64, c_double, "orc_vector_vector_addition"
    cases = [Case("axpby/n%d/alias_%s" % (n, a), "math_f64", n=n, alias=a) for n in VECTOR_SIZES for a in ("none", "u", "v")]
    alpha, beta = 1.25, -0.7

    def inputs(self, case):
        n = case.p["n"]
        return {"u": unit(n, case.id + "/u", self.dtype), "v": unit(n, case.id + "/v", self.dtype)}

    def _host(self, call, case, x):
        u, v = x["u"].copy(), x["v"].copy()
        uv = {"none": np.zeros(case.p["n"], self.dtype), "u": u, "v": v}[case.p["alias"]]
        call(P(uv), self.scalar(self.alpha), P(u), self.scalar(self.beta), P(v), case.p["n"])
        return {"uv": uv}

    def ref(self, lib, case, x):
        return self._host(lib.vector_vector_addition, case, x)

    def run_orc(self, L, case, x):
        return self._host(getattr(L, self.fn), case, x)

    def run_hip(self, form, case, x, T):
        du, dv = T.dev(x["u"]), T.dev(x["v"])
        duv = {"none": T.full(case.p["n"], 3.0, self.dtype), "u": du, "v": dv}[case.p["alias"]]
        T.k(form[0], duv, float(self.dtype(self.alpha)), du, float(self.dtype(self.beta)), dv, case.p["n"])
        return {"uv": T.host(duv)}


class AxpbyF32(Axpby):
    orc, hip_forms = ("orc_f32_vector_vector_addition",), (("fdd_vector_vector_addition_f32",),)
    dtype, scalar, fn = f32, c_float, "orc_f32_vector_vector_addition"
    cases = [Case("axpby_f32/n%d/alias_%s" % (n, a), "math_f32", n=n, alias=a) for n in VECTOR_SIZES for a in ("none", "u", "v")]


class Scaling(Row):
    source, kernels, orc, hip_forms = "math.okl", ("vector_scaling",), ("orc_vector_scaling",), (("fdd_vector_scaling",),)
    cases = [Case("scaling/n%d" % n, "math_f64", n=n) for n in VECTOR_SIZES]
    alpha = 1.0 / 3.0

    def inputs(self, case):
        return {"u": unit(case.p["n"], case.id + "/u")}

    def ref(self, lib, case, x):
        au = np.zeros(case.p["n"])
        lib.vector_scaling(P(au), c_double(self.alpha), P(x["u"]), case.p["n"])
        return {"au": au}

    def run_orc(self, L, case, x):
        au = np.zeros(case.p["n"])
        L.orc_vector_scaling(P(au), c_double(self.alpha), P(x["u"]), case.p["n"])
        return {"au": au}

    def run_hip(self, form, case, x, T):
        dau = T.full(case.p["n"], 3.0)
        T.k(form[0], dau, self.alpha, T.dev(x["u"]), case.p["n"])
        return {"au": T.host(dau)}


class ScalingF32(Row):
    """DType = float: the float build holds alpha = float(1/3); the restatement and the HIP entry take the double and
    round it once"""
    source, kernels, orc, hip_forms = "math.okl", ("vector_scaling",), ("orc_f32_vector_scaling",), (("fdd_vector_scaling_dev_f32",),)
    cases = [Case("scaling_f32/n%d" % n, "math_f32", n=n) for n in VECTOR_SIZES]
    alpha = 1.0 / 3.0

    def inputs(self, case):
        return {"u": unit(case.p["n"], case.id + "/u", f32)}

    def ref(self, lib, case, x):
        au = np.zeros(case.p["n"], f32)
        lib.vector_scaling(P(au), c_float(self.alpha), P(x["u"]), case.p["n"])
        return {"au": au}

    def run_orc(self, L, case, x):
        au = np.zeros(case.p["n"], f32)
        L.orc_f32_vector_scaling(P(au), c_double(self.alpha), P(x["u"]), case.p["n"])
        return {"au": au}

    def run_hip(self, form, case, x, T):
        dau = T.full(case.p["n"], 3.0, f32)
        T.k(form[0], dau, T.dev(np.array([self.alpha])), T.dev(x["u"]), case.p["n"])
        return {"au": T.host(dau)}


class VectorUpdates(Row):
    """initialize_arrays, solution_and_residual_update and residual_and_search_update of one kernel file, chained as the
    flexible CG chains them; `_dev` entries read alpha = num / den on the device (den = 1: the same bits)"""
    alpha, beta = 0.618, -1.7

    def __init__(self, family, source, lib):
        self.family, self.source = family, source
        self.kernels = ("initialize_arrays", "solution_and_residual_update", "residual_and_search_update")
        self.orc = tuple("orc_%s_%s" % (family, kn) for kn in self.kernels)
        direct = tuple("fdd_%s_%s" % (family, kn) for kn in self.kernels)
        self.hip_forms = (direct,) + (((direct[0], direct[1] + "_dev", direct[2] + "_dev"),) if family == "dom" else ())
        self.cases = [Case("%s_vector_updates/n%d" % (family, n), lib, n=n) for n in VECTOR_SIZES]

    def inputs(self, case):
        return {name: unit(case.p["n"], "%s/%s" % (case.id, name)) for name in ("u", "r", "p", "q", "z", "f")}

    def _host(self, fns, case, x):
        n = case.p["n"]
        u0, r0 = x["u"].copy(), x["r"].copy()
        fns[0](P(u0), P(r0), P(x["f"]), n)
        u1, r1 = x["u"].copy(), np.zeros(n)
        fns[1](P(u1), P(r1), P(x["r"]), P(x["p"]), P(x["q"]), c_double(self.alpha), n)
        p2, r2 = x["p"].copy(), x["r"].copy()
        fns[2](P(p2), P(r2), P(x["z"]), P(r1), c_double(self.beta), n)
        return {"init_u": u0, "init_r": r0, "update_u": u1, "update_r_kp1": r1, "search_p": p2, "search_r": r2}

    def ref(self, lib, case, x):
        return self._host([getattr(lib, kn) for kn in self.kernels], case, x)

    def run_orc(self, L, case, x):
        return self._host([getattr(L, fn) for fn in self.orc], case, x)

    def run_hip(self, form, case, x, T):
        n = case.p["n"]
        scalars = lambda a: (a,) if not form[1].endswith("_dev") else (T.dev(np.array([a])), T.dev(np.array([1.0])))
        u0, r0 = T.dev(x["u"]), T.dev(x["r"])
        T.k(form[0], u0, r0, T.dev(x["f"]), n)
        u1, r1 = T.dev(x["u"]), T.full(n, 3.0)
        T.k(form[1], u1, r1, T.dev(x["r"]), T.dev(x["p"]), T.dev(x["q"]), *scalars(self.alpha), n)
        p2, r2 = T.dev(x["p"]), T.dev(x["r"])
        T.k(form[2], p2, r2, T.dev(x["z"]), r1, *scalars(self.beta), n)
        return {"init_u": T.host(u0), "init_r": T.host(r0), "update_u": T.host(u1), "update_r_kp1": T.host(r1), "search_p": T.host(p2), "search_r": T.host(r2)}


class Copies(Row):
    """copy_from_domain_data (DType <- EType) and copy_to_domain_data (EType <- DType), EType = double.  The values carry
    more than 24 significant bits, so that the rounding of the float build is live."""
    source, kernels = "subdomain.okl", ("copy_from_domain_data", "copy_to_domain_data")

    def __init__(self, tag, lib, dtype, names):
        self.dtype = dtype
        self.orc = tuple("orc_sub_copy_" + nm for nm in names)
        self.hip_forms = (tuple("fdd_sub_copy_" + nm for nm in names),)
        self.cases = [Case("copies_%s/n%d" % (tag, n), lib, n=n) for n in VECTOR_SIZES]

    def inputs(self, case):
        n = case.p["n"]
        return {"v": unit(n, case.id + "/hi") + unit(n, case.id + "/lo") * 2.0**-30}

    def _host(self, fns, case, x):
        n = case.p["n"]
        inner = np.zeros(n, self.dtype)
        fns[0](P(inner), P(x["v"]), n)
        back = np.zeros(n)
        fns[1](P(back), P(inner), n)
        return {"from_domain": inner, "to_domain": back}

    def ref(self, lib, case, x):
        return self._host([lib.copy_from_domain_data, lib.copy_to_domain_data], case, x)

    def run_orc(self, L, case, x):
        return self._host([getattr(L, fn) for fn in self.orc], case, x)

    def run_hip(self, form, case, x, T):
        n = case.p["n"]
        inner, back = T.full(n, 3.0, self.dtype), T.full(n, 3.0)
        T.k(form[0], inner, T.dev(x["v"]), n)
        T.k(form[1], back, inner, n)
        return {"from_domain": T.host(inner), "to_domain": T.host(back)}


# ------------------------------------------------------------------ block reductions
REDUCTION_SIZES = (1, 128, 129, 1000)


class Reduction(Row):
    """One 128-wide block reduction: `operands` vectors in, (n + 127) / 128 block partials out (two sets of them for the
    projection kernels); the last block is partial.  No HIP entry: the HIP reductions group their sums differently by
    design and keep their 1e-13 * sum|terms| bar against these restatements (test_gpu_kernels.py::test_reductions)."""

    def __init__(self, family, kernel, operands, lib, source, sets=1):
        self.source, self.kernels, self.orc, self.hip_forms = source, (kernel,), ("orc_%s_%s" % (family, kernel),), ()
        self.operands, self.sets = operands, sets
        self.cases = [Case("%s_%s/n%d" % (family, kernel, n), lib, n=n) for n in REDUCTION_SIZES]

    def inputs(self, case):
        return {"v": [unit(case.p["n"], "%s/%d" % (case.id, j)) for j in range(self.operands)]}

    def _host(self, fn, case, x):
        n = case.p["n"]
        nb = num_blocks(n)
        block = np.full(self.sets * nb, 3.0)
        fn(P(block), *[P(v) for v in x["v"]], n, nb)
        return {"block": block}

    def ref(self, lib, case, x):
        return self._host(getattr(lib, self.kernels[0]), case, x)

    def run_orc(self, L, case, x):
        return self._host(getattr(L, self.orc[0]), case, x)


# ------------------------------------------------------------------ CSR
CSR_ROWS, CSR_COLS = 50, 40
CSR_RANGES = ((0, 49), (7, 7), (10, 31))  # inclusive ends (csr_matrix.okl:20-33)


def csr_matrix(label, dtype=f64, boolean=False):
    """50 rows of 0..6 entries, runs of empty rows (the first rows, a run in the middle that crosses a range end, the
    last rows), distinct ascending columns"""
    length = np.abs(draws(CSR_ROWS, label + "/length")) % 7
    for lo, hi in ((0, 2), (29, 34), (48, 50)):
        length[lo:hi] = 0
    length[7], length[10] = 6, 5
    ptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int32)
    col = np.zeros(int(ptr[-1]), np.int32)
    for i in range(CSR_ROWS):
        order = np.argsort(draws(CSR_COLS, "%s/row%d" % (label, i)), kind="stable")
        col[ptr[i] : ptr[i + 1]] = np.sort(order[: length[i]])
    val = np.ones(len(col), dtype) if boolean else nonzero_unit(len(col), label + "/val", dtype)
    return ptr, col, val


class Csr(Row):
    source, kernels = "csr_matrix.okl", ("multiply", "multiply_weight", "multiply_range")
    orc = ("orc_csr_multiply", "orc_csr_multiply_weight", "orc_csr_multiply_range")
    hip_forms = (("fdd_csr_multiply", "fdd_csr_multiply_weight", "fdd_csr_multiply_range"), ("fdd_csr_plan_multiply",))
    cases = [Case("csr/f64", "csr_matrix_f64")]

    def inputs(self, case):
        ptr, col, val = csr_matrix(case.id)
        return {"ptr": ptr, "col": col, "val": val, "u": unit(CSR_COLS, case.id + "/u"), "w": unit(CSR_ROWS, case.id + "/w")}

    def _host(self, fns, case, x):
        out = {"multiply": np.full(CSR_ROWS, 7.0), "multiply_weight": np.full(CSR_ROWS, 7.0)}
        fns[0](P(out["multiply"]), P(x["ptr"]), P(x["col"]), P(x["val"]), P(x["u"]), CSR_ROWS)
        fns[1](P(out["multiply_weight"]), P(x["ptr"]), P(x["col"]), P(x["val"]), P(x["u"]), P(x["w"]), CSR_ROWS)
        for lo, hi in CSR_RANGES:
            out["range_%d_%d" % (lo, hi)] = t = np.full(CSR_ROWS, 7.0)
            fns[2](P(t), P(x["ptr"]), P(x["col"]), P(x["val"]), P(x["u"]), lo, hi)
        return out

    def ref(self, lib, case, x):
        return self._host([lib.multiply, lib.multiply_weight, lib.multiply_range], case, x)

    def run_orc(self, L, case, x):
        return self._host([getattr(L, fn) for fn in self.orc], case, x)

    def run_hip(self, form, case, x, T):
        dptr, dcol, dval, du, dw = (T.dev(x[name]) for name in ("ptr", "col", "val", "u", "w"))
        out = {"multiply": T.full(CSR_ROWS, 7.0), "multiply_weight": T.full(CSR_ROWS, 7.0)}
        if len(form) == 1:
            plan = T.plan(x["ptr"], CSR_COLS)
            try:
                T.k(form[0], plan.h, out["multiply"], dptr, dcol, dval, du, None)
                T.k(form[0], plan.h, out["multiply_weight"], dptr, dcol, dval, du, dw)
                return {name: T.host(t) for name, t in out.items()}
            finally:
                plan.close()
        T.k(form[0], out["multiply"], dptr, dcol, dval, du, CSR_ROWS)
        T.k(form[1], out["multiply_weight"], dptr, dcol, dval, du, dw, CSR_ROWS)
        for lo, hi in CSR_RANGES:
            out["range_%d_%d" % (lo, hi)] = t = T.full(CSR_ROWS, 7.0)
            T.k(form[2], t, dptr, dcol, dval, du, lo, hi)
        return {name: T.host(t) for name, t in out.items()}


class CsrF32(Row):
    """csr_matrix.okl with DType = float on a boolean matrix (every value 1.0f): the gathers of the float inner solve.
    orc_f32_csr_gather and the HIP gathers take the half-open row range [lo, hi + 1)."""
    source, kernels = "csr_matrix.okl", ("multiply", "multiply_range")
    orc = ("orc_f32_csr_gather",)
    hip_forms = (("fdd_gather_rows_f32",), ("fdd_csr_plan_gather_f32",))
    cases = [Case("csr/f32_boolean", "csr_matrix_f32")]

    def inputs(self, case):
        ptr, col, val = csr_matrix(case.id, f32, boolean=True)
        return {"ptr": ptr, "col": col, "val": val, "u": unit(CSR_COLS, case.id + "/u", f32)}

    def ref(self, lib, case, x):
        out = {"multiply": np.full(CSR_ROWS, 7.0, f32)}
        lib.multiply(P(out["multiply"]), P(x["ptr"]), P(x["col"]), P(x["val"]), P(x["u"]), CSR_ROWS)
        for lo, hi in CSR_RANGES:
            out["range_%d_%d" % (lo, hi)] = t = np.full(CSR_ROWS, 7.0, f32)
            lib.multiply_range(P(t), P(x["ptr"]), P(x["col"]), P(x["val"]), P(x["u"]), lo, hi)
        return out

    def _ranges(self):
        return [("multiply", 0, CSR_ROWS)] + [("range_%d_%d" % (lo, hi), lo, hi + 1) for lo, hi in CSR_RANGES]

    def run_orc(self, L, case, x):
        out = {}
        for name, lo, end in self._ranges():
            out[name] = t = np.full(CSR_ROWS, 7.0, f32)
            L.orc_f32_csr_gather(P(t), P(x["ptr"]), P(x["col"]), P(x["u"]), lo, end)
        return out

    def run_hip(self, form, case, x, T):
        dptr, dcol, du = T.dev(x["ptr"]), T.dev(x["col"]), T.dev(x["u"])
        plan = T.plan(x["ptr"], CSR_COLS) if "plan" in form[0] else None
        try:
            out = {}
            for name, lo, end in self._ranges():
                t = T.full(CSR_ROWS, 7.0, f32)
                T.k(form[0], *([plan.h] if plan else []), t, dptr, dcol, du, lo, end)
                out[name] = T.host(t)
            return out
        finally:
            if plan:
                plan.close()


# ------------------------------------------------------------------ the table
TABLE = [
    DomStiffness(),
    SubStiffness(),
    SubStiffnessF32(),
    Restriction(),
    SetToValue(),
    Invert(),
    Axpby(),
    AxpbyF32(),
    Scaling(),
    ScalingF32(),
    VectorUpdates("dom", "domain.okl", "domain_d3_f64"),
    VectorUpdates("sub", "subdomain.okl", "subdomain_d3_f64"),
    Copies("f64", "subdomain_d3_f64", f64, ("f64_f64", "f64_f64")),
    Copies("f32", "subdomain_d3_f32", f32, ("f32_f64", "f64_f32")),
    Reduction("dom", "residual_norm", 3, "domain_d3_f64", "domain.okl"),
    Reduction("dom", "projection_inner_products", 4, "domain_d3_f64", "domain.okl", sets=2),
    Reduction("dom", "inner_product_flexible", 3, "domain_d3_f64", "domain.okl"),
    Reduction("dom", "inner_product", 3, "domain_d3_f64", "domain.okl"),
    Reduction("sub", "inner_product", 2, "subdomain_d3_f64", "subdomain.okl"),
    Reduction("sub", "weighted_inner_product", 3, "subdomain_d3_f64", "subdomain.okl"),
    Reduction("sub", "projection_inner_products", 5, "subdomain_d3_f64", "subdomain.okl", sets=2),
    Reduction("sub", "search_update_inner_product", 4, "subdomain_d3_f64", "subdomain.okl"),
    Csr(),
    CsrF32(),
]

CASES = [(row, case) for row in TABLE for case in row.cases]
CASE_IDS = [case.id for _, case in CASES]
HIP_CASES = [(row, case, form) for row, case in CASES for form in row.forms(case)]
HIP_CASE_IDS = ["%s-%s" % (case.id, "+".join(form)) for _, case, form in HIP_CASES]


def covered_kernels():
    """(kernel file, kernel name) of every row"""
    return {(row.source, kn) for row in TABLE for kn in row.kernels}


def first_difference(a, b):
    """index and both values of the first entry in which two arrays of one shape differ as bits, or None"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bits = "u%d" % a.dtype.itemsize
    diff = np.nonzero(a.view(bits) != b.view(bits))[0]
    if len(diff) == 0:
        return None
    i = int(diff[0])
    return "first difference at [%d]: %r against %r (%d of %d entries differ)" % (i, a[i].item(), b[i].item(), len(diff), len(a))


def check_against_golden(golden_cases, case, got, other=None, who="result"):
    """every array of `got` carries the recorded hash of its name; on a mismatch, where the reference's own arrays are at
    hand (`other`), the first differing index and both values go into the message"""
    want = golden_cases[case.id]
    assert set(got) <= set(want), (case.id, sorted(got), sorted(want))
    for name, a in got.items():
        if sha(a) != want[name]:
            detail = first_difference(a, other[name]) if other is not None else "reference-compiled libraries not built here: hashes only"
            raise AssertionError("%s: %s of %s differs from the reference-compiled kernel; %s" % (case.id, name, who, detail))
