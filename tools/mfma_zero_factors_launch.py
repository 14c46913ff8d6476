#!/usr/bin/env python3
"""Per-launch time of the matrix-core stiffness kernel on six factor arrays (fdd_stiffness_matrix_mfma_gather) and on three
(fdd_stiffness_matrix_mfma_diag), gather form with a box's own point -> node numbering, back to back in one process.
Default shape: C3 (32^3 elements, N = 15), where the algorithmic bytes are 8.93 GB and 5.71 GB per launch.

    python tools/mfma_zero_factors_launch.py [--E 32] [--N 15] [--launches 30] [--rounds 2] [--lib PATH] [--json OUT]

Each launch is timed by its own pair of device events; per round and entry the line gives minimum and median.  --lib loads
another build of the kernel library (a development variant of the kernel) in place of the package's own.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from microbench import PEAK, box_Q, gll  # noqa: E402
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib  # noqa: E402


def launch_times(fn, launches, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1e-3 for e0, e1 in pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--N", type=int, default=15)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert 8 <= args.N <= 15, "the matrix-core kernel covers degree 8..15"
    dev = torch.device("cuda:0")
    if args.lib:
        import torch as _t  # noqa: F401  (the HIP runtime first, as lib.hip() does)

        lib._hip = lib._Lib(os.path.abspath(args.lib), os.path.join(lib.INCLUDE_DIR, "fdd_hip.h"), "fdd_last_error")
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k

    E, N = args.E, args.N
    n = N + 1
    (_, col, _), _, P, nodes = box_Q(E, N, dev)
    torch.manual_seed(7)
    G = [torch.rand(P, dtype=torch.float64, device=dev) + 0.5 for _ in range(3)] + [torch.zeros(P, dtype=torch.float64, device=dev) for _ in range(3)]
    Dh = torch.tensor(gll(N)[2], dtype=torch.float64, device=dev)
    v = torch.rand(nodes, dtype=torch.float64, device=dev) - 0.5
    six = torch.empty(P, dtype=torch.float64, device=dev)
    three = torch.empty(P, dtype=torch.float64, device=dev)
    entries = {
        "six arrays (fdd_stiffness_matrix_mfma_gather)": (60 * P + 8 * nodes, lambda: k("fdd_stiffness_matrix_mfma_gather", six, v, None, col, Dh, G, None, E**3, N)),
        "three arrays (fdd_stiffness_matrix_mfma_diag)": (36 * P + 8 * nodes, lambda: k("fdd_stiffness_matrix_mfma_diag", three, v, None, col, Dh, G, None, E**3, N)),
    }
    print(f"library {lib.hip().path}\n{E}^3 elements, N = {N}: {P} points, {nodes} nodes, {args.launches} launches per entry and round", flush=True)
    results = {"library": lib.hip().path, "E": E, "N": N, "points": P, "nodes": nodes, "rounds": []}
    for r in range(args.rounds):
        row = {}
        for name, (nbytes, fn) in entries.items():
            t = launch_times(fn, args.launches)
            lo, med = min(t), statistics.median(t)
            print(f"round {r + 1}  {name:48s} min {lo * 1e6:8.1f} us  median {med * 1e6:8.1f} us  {nbytes / 1e9:5.2f} GB  {nbytes / med / 1e12:5.2f} TB/s = {nbytes / med / PEAK:4.2f} of peak at the median", flush=True)
            row[name] = {"min_us": lo * 1e6, "median_us": med * 1e6, "bytes": nbytes, "all_us": [x * 1e6 for x in t]}
        results["rounds"].append(row)
    same = bool(torch.equal(six, three))  # -0.0 == 0.0: values, not bits
    print(f"outputs equal as values: {same}; max|Au| = {float(six.abs().max()):.6e}", flush=True)
    results["outputs_equal"] = same
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)
    if not same:
        raise SystemExit("the two entries differ")


if __name__ == "__main__":
    main()
