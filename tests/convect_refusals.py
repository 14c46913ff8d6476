"""What the convection entries of the host C API (fddh_convect, fddh_weak_convect, fddh_convect_quadrature) answer on the CPU
build of the host layer (tests/cpu_shim), whose stand-in of the kernel library has no fdd_field_* entries:
`python tests/convect_refusals.py <libfdd_host_cpu.so>` prints one JSON object.  In a process of its own, as
tests/field_refusals.py is: the stand-in library must not stay loaded in the test process.
  uninit / null / box   situation -> operator entry -> [return code, fddh_last_error()], as in tests/field_refusals.py
  tables                degree -> {"D": the level's D_hat, "z", "w", "P", "Pd": what fddh_convect_quadrature hands out}
  moved                 at degree 7: Pd after fddh_problem_set_D_hat with 2 D_hat
"""
import ctypes
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

OPERATORS = ("fddh_convect", "fddh_weak_convect")
DEGREES = (1, 2, 7, 8, 15)


def main(lib_path):
    import numpy as np

    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

    lib._host = lib._Lib(lib_path, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")  # binds every entry the header declares
    L = lib.host()
    report = {}

    def call(name, problem, vectors):
        rc = L.raw(name)(problem, *[H._dp(v) if v is not None else None for v in vectors])
        return [rc, L.raw("fddh_last_error")().decode() if rc else ""]

    def walk(situation, problem, vectors):
        report[situation] = {name: call(name, problem, vectors) for name in OPERATORS}

    none = [None] * 5
    t = threading.Thread(target=lambda: walk("uninit", None, none))
    t.start()
    t.join()
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    walk("null", None, none)
    p = H.Problem.box((2, 2, 2), (1, 1, 1), 2, 1, False)
    walk("box", p.h, [np.zeros(p.n) for _ in range(5)])
    p.close()

    report["tables"] = {}
    for N in DEGREES:
        p = H.Problem.box((1, 1, 1), (1, 1, 1), N, 1, False)
        z, w, P, Pd = p.quadrature()
        report["tables"][str(N)] = {"D": p.get_D_hat(0).tolist(), "z": z.tolist(), "w": w.tolist(), "P": P.reshape(-1).tolist(), "Pd": Pd.reshape(-1).tolist()}
        if N == 7:
            p.set_D_hat(0, 2.0 * p.get_D_hat(0))
            report["moved"] = p.quadrature()[3].reshape(-1).tolist()
        p.close()
    sys.stdout.write(json.dumps(report) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
