"""What the flag "last_norm_from_projections" and fddh_inner_norm_counters answer on the CPU build of the host layer
(tests/cpu_shim), whose stand-in of the kernel library has none of the entries behind them:
`python tests/norm_estimate_cpu_walk.py <libfdd_host_cpu.so>` prints one JSON object.  In a process of its own: the stand-in
library must not stay loaded in the test process.
  set_1 / set_0     [return code, fddh_last_error()] of fddh_problem_set_flag with 1 and with 0
  counters          Problem.inner_norm_counters() after an application of the preconditioner: the flag is off there
  nosub             [return code, text] of fddh_inner_norm_counters on a problem without a Subdomain
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main(lib_path):
    import numpy as np

    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

    lib._host = lib._Lib(lib_path, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
    L = lib.host()
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    report = {}

    def answer(rc):
        return [rc, L.raw("fddh_last_error")().decode() if rc else ""]

    p = H.Problem.box((2, 2, 2), (1, 1, 1), 2, 1, True)
    p.set_flag("sub_use_preconditioner", 0)
    report["set_1"] = answer(L.raw("fddh_problem_set_flag")(p.h, b"last_norm_from_projections", 1))
    report["set_0"] = answer(L.raw("fddh_problem_set_flag")(p.h, b"last_norm_from_projections", 0))
    z, hist = p.precond_apply(np.linspace(-1.0, 1.0, p.n), "gmres")
    report["finite"] = bool(np.isfinite(z).all() and len(hist) > 1)
    report["counters"] = p.inner_norm_counters()
    p.close()
    bare = H.Problem.box((2, 2, 2), (1, 1, 1), 2, 1, False)
    report["nosub"] = answer(L.raw("fddh_inner_norm_counters")(bare.h, None, None, None))
    bare.close()
    sys.stdout.write(json.dumps(report) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
