"""What fddh_diffusivity_set refuses (include/fdd_host.h): more than one rank, a composite region, a 2-D problem, a wrong
length, a value that is not finite or not > 0 -- each with a message that names its reason (the first offending point for a
value), nothing touched: the problem answers as it did before, bit for bit, with a kappa that was set before still in place.
And the flag "coefficient_in_kernel" on a kernel library without the coefficient entries.

run(stand_in) is called by tests/test_gpu_diffusivity.py (stand_in = False: the product's kernel library has the entries, the
flag is accepted) and, as `python tests/diffusivity_refusals.py <libfdd_host_cpu.so> <libfdd_cpu_shim.so>`, by
tests/test_cpu_diffusivity.py on the CPU stand-in of the kernel library, which has none of the three: the flag is refused
there, naming the first, and the stand-in is asked for each of them by name.  Prints `refused: ...` per refusal."""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

COEF_ENTRIES = ("fdd_stiffness_matrix_lines_coef", "fdd_stiffness_matrix_lines_coef_f32", "fdd_stiffness_matrix_lines_coef_direct")


def run(stand_in):
    import diffusivity_checks as C

    S, H, lib = C.api()

    def refused(call, *words):
        try:
            call()
        except lib.FddError as e:
            print("refused:", e)
            assert all(w in str(e) for w in words), (str(e), words)
        else:
            raise AssertionError("accepted: %s" % (words,))

    # more than one rank
    def body(rank, size):
        p = H.Problem.box((2, 1, 1), (2, 1, 1), 2, 1, False)
        try:
            u = S.seeded_uniform(p.n, 3)
            before = p.stiffness(u)
            refused(lambda: p.diffusivity(2.0), "one rank")
            assert not p.diffusivity_info()["active"] and np.array_equal(p.stiffness(u), before)
            return 1
        finally:
            p.close()

    assert sum(H.run_local_ranks(2, body)) == 2

    # a composite region
    p = H.Problem.box((3, 3, 3), (1, 1, 1), 3, 2, True, force_composite=True)
    try:
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 51))
        before = p.solve(f)
        refused(lambda: p.diffusivity(2.0), "composite")
        after = p.solve(f)
        assert not p.diffusivity_info()["active"] and before[1] == after[1] > 0 and np.array_equal(C.bits(before[0]), C.bits(after[0]))
    finally:
        p.close()

    # a 2-D problem
    with tempfile.TemporaryDirectory() as tmp:
        S.write_mesh_files(tmp, S.QuadMesh((3, 2), 4, amplitude=0.05))
        p = H.Problem.from_directory(tmp, 4, 2, with_subdomain=False)
        try:
            u = S.seeded_uniform(p.n, 3)
            before = p.stiffness(u)
            refused(lambda: p.diffusivity(2.0), "3-D only", "2-D")
            assert np.array_equal(p.stiffness(u), before) and np.abs(before).max() > 0
        finally:
            p.close()

    # a wrong length, bad values: with a kappa in place, which stays
    p = C.new_problem("box", (2, 2, 2), 3)
    try:
        kappa = C.kappa_random(p.n, 8)
        p.diffusivity(kappa)
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 52))
        before = p.solve(f)
        info = p.diffusivity_info()
        refused(lambda: p.diffusivity(np.ones(p.n + 1)), "one value per point", str(p.n), str(p.n + 1))
        refused(lambda: p.diffusivity(np.ones(p.n - 1)), "one value per point")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(lambda: p.diffusivity(bad), "finite and > 0", "point 0")
            k = np.ones(p.n)
            k[5], k[9] = bad, bad
            refused(lambda: p.diffusivity(k), "finite and > 0", "point 5")
        assert p.diffusivity_info() == info and info["active"]
        after = p.solve(f)
        assert before[1] == after[1] > 0 and np.array_equal(C.bits(before[0]), C.bits(after[0])) and np.array_equal(C.bits(before[2]), C.bits(after[2]))

        # the flag
        if stand_in:
            refused(lambda: p.set_flag("coefficient_in_kernel", 1), "coefficient_in_kernel", COEF_ENTRIES[0], "does not export")
        else:
            p.set_flag("coefficient_in_kernel", 1)
        p.set_flag("coefficient_in_kernel", 0)
        assert not p.diffusivity_info()["fine_domain_in_kernel"]
        after = p.solve(f)
        assert np.array_equal(C.bits(before[0]), C.bits(after[0]))
    finally:
        p.close()


if __name__ == "__main__":
    import diffusivity_checks as C

    _, H, lib = C.api()
    lib._host = lib._Lib(sys.argv[1], os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
    shim = ctypes.CDLL(sys.argv[2])
    for name in COEF_ENTRIES:
        print("missing:" if not hasattr(shim, name) else "exported:", name)
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    run(True)
    print("ok")
