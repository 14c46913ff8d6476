"""What a Helmholtz shift costs per outer PCG step: C2 (32^3 elements, N = 7), one process, the headline
configuration (inner GMRES(4), double, no V-cycle), lam = 0 against lam = 1 alternated off / on three times, pcg_steps
20 after 3, a host clock around a device synchronise.

    python tools/helmholtz_step_time.py [OUT.json]      the step times (profiles/r19_helmholtz/step_times.json)
    python tools/helmholtz_step_time.py --trace         one short off / on pair, to run under a kernel trace
                                                        (profiles/r19_helmholtz/kernel_stats.csv)
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H  # noqa: E402


def main(argv):
    trace = "--trace" in argv
    out = [a for a in argv if not a.startswith("--")]
    H.init(0)
    H.comm_single()
    H.set_print(False)
    t = time.perf_counter()
    p = H.Problem.box((32, 32, 32), (1, 1, 1), 7, 6, with_subdomain=True)
    p.set_flag("sub_use_preconditioner", 0)
    p.set_flag("preconditioner_precision", 64)
    _, f = p.make_rhs(function_id=4, seed=1234)
    print("setup %.1f s, %d nodes" % (time.perf_counter() - t, p.info["num_local_nodes"]), flush=True)
    steps, warmup = (5, 2) if trace else (20, 3)
    rows = []
    for lam in (0.0, 1.0) if trace else (0.0, 1.0, 0.0, 1.0, 0.0, 1.0):
        t = time.perf_counter()
        p.helmholtz(lam)
        t_set = time.perf_counter() - t
        p.pcg_begin(f)
        p.pcg_steps(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = p.pcg_steps(steps)
        torch.cuda.synchronize()
        rows.append({"lambda": lam, "ms_per_step": 1e3 * (time.perf_counter() - t0) / steps, "last_residual": last, "helmholtz_set_seconds": t_set})
        print(json.dumps(rows[-1]), flush=True)
    p.close()
    if trace:
        return
    off = [r["ms_per_step"] for r in rows if r["lambda"] == 0.0]
    on = [r["ms_per_step"] for r in rows if r["lambda"] != 0.0]
    summary = {"config": "C2 32^3 N=7, headline (inner GMRES(4), double, no V-cycle), pcg_steps 20 after 3", "runs": rows, "off_ms_min": min(off), "on_ms_min": min(on), "off_ms_all": off, "on_ms_all": on}
    if out:
        with open(out[0], "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"off_ms_min": min(off), "on_ms_min": min(on)}))


if __name__ == "__main__":
    main(sys.argv[1:])
