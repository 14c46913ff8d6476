"""What a Robin coefficient costs per outer PCG step, and what the indexed shift saves of it: C2 (32^3
elements, N = 7) with the face codes DDNNNN, one process, the headline configuration (inner GMRES(4), double, no V-cycle),
three settings alternated three times -- no Robin coefficient, alpha = 1 on the four natural faces with "indexed_shift" 0,
the same with "indexed_shift" 1 --, pcg_steps 20 after 3, a host clock around a device synchronise.

    python tools/boundary_step_time.py [OUT.json]      the step times (profiles/r21_boundary/step_times.json)

The yardstick of the indexed kernel is the dense pass in this same process: the flag's default is 1 only if its step is faster
by more than the largest spread between the runs of one setting.
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H  # noqa: E402

SETTINGS = ("none", "dense", "indexed")


def main(argv):
    out = [a for a in argv if not a.startswith("--")]
    H.init(0)
    H.comm_single()
    H.set_print(False)
    t = time.perf_counter()
    p = H.Problem.box((32, 32, 32), (1, 1, 1), 7, 6, with_subdomain=True, faces="DDNNNN")
    p.set_flag("sub_use_preconditioner", 0)
    p.set_flag("preconditioner_precision", 64)
    _, f = p.make_rhs(function_id=4, seed=1234)
    s = p.surface(normal=False)
    alpha = (p.mesh_array("p_mask")[s["points"]] != 0.0) * (s["side"] >= 2)[:, None, None] * 1.0
    nodes = p.info["num_local_nodes"]
    print("setup %.1f s, %d nodes, %d faces" % (time.perf_counter() - t, nodes, len(s["elem"])), flush=True)
    steps, warmup = 20, 3
    rows = []
    for setting in SETTINGS * 3:
        t = time.perf_counter()
        p.set_flag("indexed_shift", int(setting == "indexed"))
        p.robin(None if setting == "none" else alpha)
        t_set = time.perf_counter() - t
        info = p.boundary_info()
        assert info["robin_active"] == (setting != "none") and info["indexed_inner"] == (setting == "indexed"), info
        p.pcg_begin(f)
        p.pcg_steps(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = p.pcg_steps(steps)
        torch.cuda.synchronize()
        rows.append({"setting": setting, "ms_per_step": 1e3 * (time.perf_counter() - t0) / steps, "last_residual": last, "robin_set_seconds": t_set, "shift_support": info["shift_support"]})
        print(json.dumps(rows[-1]), flush=True)
    p.close()
    ms = {k: [r["ms_per_step"] for r in rows if r["setting"] == k] for k in SETTINGS}
    spread = max(max(v) - min(v) for v in ms.values())
    gain = min(ms["dense"]) - min(ms["indexed"])
    support = max(r["shift_support"] for r in rows)
    summary = {"config": "C2 32^3 N=7 DDNNNN, alpha = 1 on the four natural faces, headline (inner GMRES(4), double, no V-cycle), pcg_steps 20 after 3", "nodes": nodes, "shift_support": support,
               "support_share": support / nodes, "runs": rows, "ms_all": ms, "ms_min": {k: min(v) for k, v in ms.items()}, "largest_spread_ms": spread, "indexed_gain_ms": gain, "indexed_is_faster": bool(gain > spread)}
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out[0])), exist_ok=True)
        with open(out[0], "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({k: summary[k] for k in ("ms_min", "largest_spread_ms", "indexed_gain_ms", "indexed_is_faster", "support_share")}))


if __name__ == "__main__":
    main(sys.argv[1:])
