#!/usr/bin/env python
"""The Chebyshev-Jacobi inner solve (flag "inner_solver" = 1) against the inner GMRES(4), one rank, outer fcg to a tolerance.

Meshes: the box and the Kershaw map (eps = 0.3) of the same size.  Inner solves: GMRES(4) without a preconditioner in its
slot ("sub_use_preconditioner" 0, the headline configuration) and with point-Jacobi there (2), and Chebyshev-Jacobi at
orders 2, 3, 4, 5, 8 on the same diagonal.  For each: iterations and device seconds to the tolerance (solve_timed, after
one warm-up solve), milliseconds per outer step, and whether it converged within the iteration cap.  The order-4 leg is
run with "fused_chebyshev" off / on / off / on, so that the fused gather's gain can be told from the run-to-run spread.
One JSON line.

    python tools/inner_solver_compare.py --elements 32 --degree 7 > profiles/r07_inner_chebyshev.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--elements", type=int, default=32, help="elements per direction (32 at degree 7 = config C2)")
    ap.add_argument("--degree", type=int, default=7)
    ap.add_argument("--reduction", type=int, default=6)
    ap.add_argument("--orders", default="2,3,4,5,8")
    ap.add_argument("--kershaw-eps", type=float, default=0.3)
    ap.add_argument("--tolerance", type=float, default=1e-7)
    ap.add_argument("--max-iterations", type=int, default=500)
    args = ap.parse_args()

    import torch

    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H

    H.init(0)
    H.comm_single()
    H.set_print(False)
    E = (args.elements,) * 3
    orders = [int(o) for o in args.orders.split(",") if o]
    result = {"what": "inner solves compared under outer fcg; seconds are device time of the whole solve (stream synchronised before and after), after one warm-up solve of the same right-hand side",
              "device": torch.cuda.get_device_name(0), "elements": list(E), "degree": args.degree, "reduction": args.reduction, "tolerance": args.tolerance, "max_iterations": args.max_iterations, "meshes": {}}

    for mesh in ("box", "kershaw"):
        p = H.Problem.box(E, (1, 1, 1), args.degree, args.reduction, True) if mesh == "box" else H.Problem.kershaw(E, (1, 1, 1), args.degree, args.reduction, eps=args.kershaw_eps)
        p.set_options(max_iterations=args.max_iterations, tolerance=args.tolerance)
        f = p.make_rhs_from(np.random.default_rng(1234).uniform(0.0, 1.0, p.n))[1]

        def leg():
            p.solve_timed(f, "fcg")
            its, hist, sec = p.solve_timed(f, "fcg")
            return {"iterations": int(its), "seconds": float(sec), "ms_per_step": 1e3 * float(sec) / max(int(its), 1), "converged": bool(hist[-1] <= args.tolerance * hist[0]), "final_relative_residual": float(hist[-1] / hist[0])}

        legs = {}
        for pre in (0, 2):
            p.set_flag("inner_solver", 0)
            p.set_flag("sub_use_preconditioner", pre)
            legs["gmres4_sub_use_preconditioner_%d" % pre] = leg()
        p.set_flag("inner_solver", 1)
        info = p.inner_chebyshev_info()
        legs["chebyshev_settings"] = info
        for m in orders:
            p.inner_chebyshev(order=m)
            legs["chebyshev_order_%d" % m] = leg()
        p.inner_chebyshev(order=4)
        legs["chebyshev_order_4_fused_off_on_off_on"] = []
        for fused in (0, 1, 0, 1):
            p.set_flag("fused_chebyshev", fused)
            legs["chebyshev_order_4_fused_off_on_off_on"].append(leg())
        result["meshes"][mesh] = legs
        p.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
