#!/usr/bin/env python
"""What successive-right-hand-side projection (Problem.solve_projected) buys on a slowly varying sequence, one rank.

T right-hand sides f_t = A u*(t),
    u*(t) = cos(w t) phi_0 + sin(w t) phi_1 + d t phi_2 + eps psi_t,
phi_i fixed seeded mixes of the lowest Dirichlet modes of the unit box (what a time stepper's solutions look like), psi_t
a fresh seeded rough field per step.  The sequence goes through solve_timed (every solve from u = 0) and through
solve_projected at capacities 4, 8 and 16, in the headline configuration (inner GMRES alone) and in the reference's
default one (the low-order V-cycle inside every inner step).  One JSON line: iterations and device seconds per step of
each; the seconds of the projected solves include the projection's own passes.

    python tools/projection_sequence.py --elements 32 --degree 7 --steps 12 > profiles/projection_sequence_c2.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ((1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 1), (1, 2, 2), (2, 1, 2), (2, 2, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--elements", type=int, default=32, help="elements per direction (32 at degree 7 = config C2)")
    ap.add_argument("--degree", type=int, default=7)
    ap.add_argument("--reduction", type=int, default=6)
    ap.add_argument("--steps", type=int, default=12, help="T, right-hand sides in the sequence")
    ap.add_argument("--omega", type=float, default=0.2)
    ap.add_argument("--drift", type=float, default=0.05)
    ap.add_argument("--fresh", type=float, default=1e-3, help="amplitude of the fresh rough part of every step")
    ap.add_argument("--capacities", default="4,8,16")
    ap.add_argument("--method", choices=["fcg", "gmres"], default="fcg")
    ap.add_argument("--tolerance", type=float, default=1e-7)
    ap.add_argument("--no-reference-default", action="store_true", help="headline configuration only (no hierarchy build)")
    args = ap.parse_args()

    import torch

    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H

    H.init(0)
    H.comm_single()
    H.set_print(False)
    E = (args.elements,) * 3
    p = H.Problem.box(E, (1, 1, 1), args.degree, args.reduction, True)
    p.set_options(max_iterations=500, tolerance=args.tolerance)
    x, y, z = (p.mesh_array(c) for c in "xyz")

    def smooth(seed):
        w = np.random.default_rng(seed).uniform(0.5, 1.0, len(MODES)) / np.array([a * a + b * b + c * c for a, b, c in MODES]) * 3.0
        out = np.zeros(p.n)
        for wk, (a, b, c) in zip(w, MODES):
            out += wk * np.sin(a * np.pi * x) * np.sin(b * np.pi * y) * np.sin(c * np.pi * z)
        return out

    phi = [smooth(100 + i) for i in range(3)]
    del x, y, z
    rhs = []
    for t in range(args.steps):
        u_star = np.cos(args.omega * t) * phi[0] + np.sin(args.omega * t) * phi[1] + args.drift * t * phi[2]
        u_star += args.fresh * np.random.default_rng(1000 + t).uniform(0.0, 1.0, p.n)
        rhs.append(p.make_rhs_from(u_star)[1])
    del phi

    capacities = [int(c) for c in args.capacities.split(",") if c]
    result = {"what": "successive-right-hand-side projection against the plain solve on one slowly varying sequence; seconds are device time per solve (stream synchronised before and after), the projection's own passes included",
              "device": torch.cuda.get_device_name(0), "elements": list(E), "degree": args.degree, "reduction": args.reduction, "points": p.n,
              "steps": args.steps, "omega": args.omega, "drift": args.drift, "fresh": args.fresh, "outer": args.method, "tolerance": args.tolerance, "configurations": {}}

    def run_sequence(capacity):
        its, sec, start = [], [], []
        p.projection(capacity)
        for f in rhs:
            if capacity == 0:
                i, hist, s = p.solve_timed(f, args.method)
                start.append(1.0)
            else:
                _, i, hist, proj = p.solve_projected(f, args.method, timed=True)
                s = proj[4]
                start.append(float(proj[1] / proj[0]))
            its.append(int(i))
            sec.append(float(s))
        p.projection(0)
        return {"iterations": its, "seconds": sec, "start_residual_over_f": start, "total_iterations": int(sum(its)), "total_seconds": float(sum(sec))}

    for name, vcycle in (("headline", 0), ("reference_default", 1)):
        if vcycle and args.no_reference_default:
            continue
        if vcycle:
            p.amg_build()
        p.set_flag("sub_use_preconditioner", vcycle)
        p.solve_timed(rhs[0], args.method)  # warm-up: first-use allocations and graph capture stay out of the figures
        entry = {"plain": run_sequence(0)}
        for cap in capacities:
            entry["capacity_%d" % cap] = run_sequence(cap)
        result["configurations"][name] = entry
    p.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
