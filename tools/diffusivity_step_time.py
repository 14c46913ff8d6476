"""What a diffusivity per point costs per outer PCG step, and what the coefficient instance of the line kernel buys (DESIGN
section 14): C2 (32^3 elements, N = 7), one process, the headline configuration (inner GMRES(4), double, no V-cycle),
kappa = 1 + 1/2 sin(2 pi x) sin(2 pi y) sin(2 pi z).  Three settings alternated three times each -- no kappa; kappa with
"coefficient_in_kernel" = 0 (every list streams its scaled arrays, the kernel that was there before); kappa with it = 1 --
pcg_steps 20 after 3, a host clock around a device synchronise.  The time of fddh_diffusivity_set at that size is recorded
with every change of kappa.

    python tools/diffusivity_step_time.py [OUT.json]      the step times (profiles/r20_diffusivity/step_times.json)
    python tools/diffusivity_step_time.py --trace         one short triple, to run under a kernel trace
                                                          (profiles/r20_diffusivity/kernel_stats.csv)
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H  # noqa: E402

SETTINGS = ("none", "streamed", "in_kernel")


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
    x, y, z = (p.mesh_array(c) for c in "xyz")
    kappa = 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y) * np.sin(2 * np.pi * z)
    del x, y, z
    print("setup %.1f s, %d nodes" % (time.perf_counter() - t, p.info["num_local_nodes"]), flush=True)
    steps, warmup = (5, 2) if trace else (20, 3)
    rows = []
    for setting in SETTINGS * (1 if trace else 3):
        p.set_flag("coefficient_in_kernel", 1 if setting == "in_kernel" else 0)
        t = time.perf_counter()
        p.diffusivity(None if setting == "none" else kappa)
        t_set = time.perf_counter() - t
        info = p.diffusivity_info()
        p.pcg_begin(f)
        p.pcg_steps(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = p.pcg_steps(steps)
        torch.cuda.synchronize()
        rows.append({"setting": setting, "ms_per_step": 1e3 * (time.perf_counter() - t0) / steps, "last_residual": last, "last_residual_hex": float(last).hex(),
                     "diffusivity_set_seconds": t_set, "fine_domain_in_kernel": info["fine_domain_in_kernel"], "sub_lists_in_kernel": info["sub_lists_in_kernel"]})
        print(json.dumps(rows[-1]), flush=True)
    p.close()
    if trace:
        return
    ms = {s: [r["ms_per_step"] for r in rows if r["setting"] == s] for s in SETTINGS}
    summary = {"config": "C2 32^3 N=7, headline (inner GMRES(4), double, no V-cycle), pcg_steps 20 after 3, kappa = 1 + sin sin sin / 2", "runs": rows,
               "ms_all": ms, "ms_min": {s: min(v) for s, v in ms.items()}, "spread_ms": {s: max(v) - min(v) for s, v in ms.items()}}
    if out:
        with open(out[0], "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"ms_min": summary["ms_min"], "spread_ms": summary["spread_ms"]}))


if __name__ == "__main__":
    main(sys.argv[1:])
