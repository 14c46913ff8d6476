"""Which stiffness kernel an element list runs, restated in Python from the project's documents (the flags' descriptions,
DESIGN.md's table of profile labels) and not from the C++ of host/element_operator.hpp: the precedence of the families, the
profile label and bytes per point of every choice, and what the five fddh_problem_*_info entries count.
test_cpu_stiffness_choice.py holds the host layer's decision to it over every reachable combination;
test_gpu_stiffness_choice.py holds a real solve's profile labels and info answers to it.

A list: dim, degree, and what was established about its arrays -- affine (in use), offdiag_zero, shared_blocks, and the lean
verdicts on its double and float derivative tables.  Flags: a dict name -> bool."""
import itertools
import struct

FLAGS = ("mfma_stiffness", "skip_zero_factors", "line_stiffness", "mfma_skip_zero_factors", "shared_factor_blocks", "lean_line_stiffness")
FAMILIES = ("two_launch", "fused_2d", "fused", "diag", "lines", "mfma", "mfma_diag", "affine", "mfma_affine")


def reachable(dim, degree, affine, offdiag_zero, shared_blocks, lean64, lean32):
    """offdiag_zero and affine are established for 3-D lists of degree <= 15 only, shared_blocks only where offdiag_zero
    holds, and a table passes the lean check only at degree 7"""
    fused_3d = dim == 3 and degree <= 15
    return (fused_3d or not (affine or offdiag_zero)) and (offdiag_zero or not shared_blocks) and (degree == 7 or not (lean64 or lean32))


def choose(lst, flags, f32, form, in_place=False):
    """(family, shared, lean) for form "local" (double only; in_place: Au is u) or "gather" """
    dim, degree, affine, offdiag_zero, shared_blocks, lean64, lean32 = lst
    on = lambda name: bool(flags[name])
    plain = lambda family: (family, False, False)
    # the matrix-core kernels: double, 3-D, degree 11..15; a float list never runs on them
    cores = on("mfma_stiffness") and not f32 and dim == 3 and 11 <= degree <= 15
    # three arrays: the flag, zero off-diagonal arrays, not affine; "skip_zero_factors" = 0 means six arrays everywhere
    three = on("skip_zero_factors") and offdiag_zero and not affine
    if form == "gather":
        if affine:  # first, whatever the other flags say
            return plain("mfma_affine" if cores else "affine")
        if cores:
            return plain("mfma_diag" if three and on("mfma_skip_zero_factors") else "mfma")
    else:
        assert not f32, "the local form exists in double only"
        if cores and not in_place:  # the local matrix-core kernels need Au != u; there is no local affine kernel
            return plain("mfma_diag" if three and on("mfma_skip_zero_factors") else "mfma")
    if three and not cores:  # a list that counts as a matrix-core list runs six arrays where it cannot run there (in place)
        if on("line_stiffness") and dim == 3 and degree == 7:
            # shared exactly where the shared instance would run; lean by the verdict on this precision's own table
            return ("lines", on("shared_factor_blocks") and shared_blocks, on("lean_line_stiffness") and (lean32 if f32 else lean64))
        return plain("diag")
    if form == "gather" or (dim == 3 and degree <= 15):
        return plain("fused")
    return plain("fused_2d" if dim == 2 and degree <= 15 else "two_launch")


# (form, family, shared, lean) -> ((label f64, label f32), (bytes per point f64, f32)); None: no such instance
_LINE = "line_stiffness_kernel"
PROFILE = {
    ("local", "mfma_diag", False, False): (("mfma_diag_stiffness_kernel", None), (40, None)),
    ("local", "mfma", False, False): (("mfma_stiffness_kernel", None), (64, None)),
    ("local", "lines", False, False): ((_LINE, None), (40, None)),
    ("local", "lines", True, False): ((_LINE + "<shared>", None), (16, None)),
    ("local", "lines", False, True): ((_LINE + "<lean>", None), (40, None)),
    ("local", "lines", True, True): ((_LINE + "<shared,lean>", None), (16, None)),
    ("local", "diag", False, False): (("diag_stiffness_kernel", None), (40, None)),
    ("local", "fused", False, False): (("fused_stiffness_kernel", None), (64, None)),
    ("local", "fused_2d", False, False): (("fused_stiffness_2d_kernel", None), (40, None)),
    ("local", "two_launch", False, False): ((None, None), (None, None)),  # no scope
    ("gather", "affine", False, False): (("fused_stiffness_kernel<gather,affine>", "fused_stiffness_kernel<gather,f32,affine>"), (12, 8)),
    ("gather", "mfma_affine", False, False): (("mfma_stiffness_kernel<gather,affine>", None), (12, None)),
    ("gather", "mfma_diag", False, False): (("mfma_diag_stiffness_kernel<gather>", None), (36, None)),
    ("gather", "lines", False, False): ((_LINE + "<gather>", _LINE + "<gather,f32>"), (36, 20)),
    ("gather", "lines", True, False): ((_LINE + "<gather,shared>", _LINE + "<gather,shared,f32>"), (12, 8)),
    ("gather", "lines", False, True): ((_LINE + "<gather,lean>", _LINE + "<gather,f32,lean>"), (36, 20)),
    ("gather", "lines", True, True): ((_LINE + "<gather,shared,lean>", _LINE + "<gather,shared,f32,lean>"), (12, 8)),
    ("gather", "diag", False, False): (("diag_stiffness_kernel<gather>", "diag_stiffness_kernel<gather,f32>"), (36, 20)),
    ("gather", "fused", False, False): (("fused_stiffness_kernel<gather>", "fused_stiffness_kernel<gather,f32>"), (60, 32)),
    ("gather", "mfma", False, False): (("mfma_stiffness_kernel<gather>", None), (60, None)),
}
ALL_LABELS = {label for labels, _ in PROFILE.values() for label in labels if label}


def profile(form, choice, f32):
    """(label, bytes per point); the gather form adds sizeof(Real) * gathered values to points * bytes per point"""
    labels, nbytes = PROFILE[(form,) + tuple(choice)]
    return labels[f32], nbytes[f32]


def info(lst, flags, f32):
    """what the five fddh_problem_*_info entries say of a list: from the gather form in the precision in use.  Three arrays
    includes the line lists and excludes the matrix-core instance; shared and lean are attributes of the line form"""
    family, shared, lean = choose(lst, flags, f32, "gather")
    return {"diag": family in ("diag", "lines"), "mfma_diag": family == "mfma_diag", "lines": family == "lines", "shared": family == "lines" and shared, "lean": family == "lines" and lean}


def composite_info(lists, flags, f32):
    """what the entries say of a Subdomain with several level lists (a composite region: the rank's own elements at degree N,
    rings at the reduced degrees, the degree-1 far field): every list is chosen for on its own, from its own degree and
    arrays, and an entry counts the lists of its kind -- a degree-7 line list stands next to slab lists at 5, 3 and 1"""
    each = [info(lst, flags, f32) for lst in lists]
    return {kind: sum(one[kind] for one in each) for kind in ("diag", "mfma_diag", "lines", "shared", "lean")}


def lean_table_ok(D, f32=False):
    """the lean line instance's conditions on an 8 x 8 derivative table (the flag's description), bit for bit: the interior
    diagonal is +-0.0 and everywhere else entry 63 - m has the bits of the negation of entry m; f32: on the table cast to
    float, which is the one the float lists read"""
    code, sign = ("<f", 1 << 31) if f32 else ("<d", 1 << 63)
    values = [float(x) for row in D for x in (row if hasattr(row, "__len__") else [row])]
    if len(values) != 64:
        return False
    w = [int.from_bytes(struct.pack(code, x), "little") for x in values]
    if any(w[9 * i] & ~sign for i in range(1, 7)):
        return False
    return all(w[63 - m] == w[m] ^ sign for m in range(32) if m not in (9, 18, 27))


# 2, 3 and 5: the intermediate degrees of the composites tests/local_world_checks.py runs (7, 5, 3, 1; 5, 3, 1; 3, 2, 1)
DEGREES = (1, 2, 3, 5, 7, 8, 11, 15, 16)


def combinations():
    """every reachable (list, flags, f32, form, in_place)"""
    for dim, degree in itertools.product((2, 3), DEGREES):
        for state in itertools.product((False, True), repeat=5):
            lst = (dim, degree) + state
            if not reachable(*lst):
                continue
            for bits in itertools.product((False, True), repeat=len(FLAGS)):
                flags = dict(zip(FLAGS, bits))
                yield lst, flags, False, "local", False
                yield lst, flags, False, "local", True
                yield lst, flags, False, "gather", False
                yield lst, flags, True, "gather", False
