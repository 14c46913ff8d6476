"""What every fddh_problem_* entry of the host C API (include/fdd_host.h) answers to a call it has to refuse, and what
fddh_problem_set_flag answers to every flag: `python tests/capi_refusals.py <libfdd_host*.so> <cpu|gpu>` prints one line per
call -- situation, name, return code, fddh_last_error() -- separated by tabs.  tests/capi_refusals_expected.tsv is that
output of the library before the entries' common openings were folded into one guard (host/fdd_host_capi.cpp), on the CPU
stand-in of the kernel library; tests/test_cpu_capi_refusals.py and tests/test_gpu_capi_refusals.py hold a library to it.

The entries are taken from the header, so one added later is walked without an edit here: every fddh_problem_* except
the create_* entries and destroy, with NULL for every pointer and 0 for every scalar, in four situations:
  uninit   a thread that never called fddh_init
  null     the initialised rank, NULL problem
  foreign  a second initialised thread that is handed the first thread's live problem
  nosub    the owner, on a problem built without a Subdomain
and fddh_problem_set_flag with every flag the host layer knows and one it does not, values 0 and 1 and, for the flags with
a range, one value below and one above it, on the problem without a Subdomain (flags_nosub) and on one with (flags_sub).
The problems are boxes of 2x2x2 elements, degree 2, reduction 1.

mode cpu: the library is the CPU build of the host layer (tests/cpu_shim) and takes the place of the package's own; gpu:
the package's own libraries, on the GPU.
"""
import ctypes
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

# fddh_problem_set_flag: the on/off flags, the flags that choose between the stiffness kernels and the flags with a range,
# with one value below and one above it
FLAGS = (
    "affine_geometry", "amg_device_setup", "amg_fused_smoother", "amg_graph", "amg_matrix_free_transfer", "assembled_inner_solve", "assembled_outer_solve",
    "chebyshev_kernels", "device_bookkeeping", "early_gamma", "fold_coarse_exchange", "fused_chebyshev", "fused_dssum", "fused_projection",
    "fused_update_flexible_dot", "lazy_steps", "neighbour_interface_exchange", "restructured_inner_solve", "shared_residual_norm", "skip_last_basis_store",
    "sub_use_preconditioner", "unit_stitch_in_place",
    "mfma_stiffness", "skip_zero_factors", "mfma_skip_zero_factors", "line_stiffness", "shared_factor_blocks", "lean_line_stiffness", "assemble_in_stiffness",
)
RANGED = {
    "inner_solver": (-1, 2),
    "inner_chebyshev_order": (0, 17),
    "inner_chebyshev_lower_permille": (0, 1000),
    "amg_num_vcycles": (0, 17),
    "amg_cheby_order": (0, 5),
    "preconditioner_precision": (31, 65),
    "amg_precision": (31, 65),
}
UNKNOWN = "no_such_flag"


def main(lib_path, mode):
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

    if mode == "cpu":
        lib._host = lib._Lib(lib_path, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
    else:
        assert mode == "gpu" and os.path.samefile(lib_path, lib.host().path), (mode, lib_path)
    L = lib.host()
    entries = sorted(n for n in lib.parse_header(os.path.join(lib.INCLUDE_DIR, "fdd_host.h")) if n.startswith("fddh_problem_") and not n.startswith("fddh_problem_create_") and n != "fddh_problem_destroy")
    assert len(entries) >= 54, entries
    lines = []

    def report(situation, name, rc):
        lines.append("%s\t%s\t%d\t%s" % (situation, name, rc, L.raw("fddh_last_error")().decode() if rc else ""))

    def walk(situation, problem):
        for name in entries:
            args = [None if t is ctypes.c_void_p else t(0) for t in L.decls[name][1]]
            args[0] = problem
            report(situation, name, L.raw(name)(*args))

    def on_a_thread(body):
        failure = []

        def run():
            try:
                body()
            except BaseException as exc:  # an assertion of the walk itself: the main thread raises it again
                failure.append(exc)

        t = threading.Thread(target=run)
        t.start()
        t.join()
        if failure:
            raise failure[0]

    def init_rank(first):
        H.init(0, use_torch_stream=first and mode == "gpu")
        H.comm_single()
        H.set_print(False)

    on_a_thread(lambda: walk("uninit", None))
    init_rank(True)
    walk("null", None)
    bare = H.Problem.box((2, 2, 2), (1, 1, 1), 2, 1, False)
    full = H.Problem.box((2, 2, 2), (1, 1, 1), 2, 1, True)

    def foreign():
        init_rank(False)
        try:
            walk("foreign", full.h)
        finally:
            L.call("fddh_rank_finalize")

    on_a_thread(foreign)
    walk("nosub", bare.h)

    for situation, p in (("flags_nosub", bare), ("flags_sub", full)):
        for flag in sorted(FLAGS + tuple(RANGED) + (UNKNOWN,)):
            for value in dict.fromkeys((0, 1) + RANGED.get(flag, ())):  # each value once: 0 is below some ranges
                report(situation, "%s=%d" % (flag, value), L.raw("fddh_problem_set_flag")(p.h, flag.encode(), value))
    full.close()
    bare.close()
    sys.stdout.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
