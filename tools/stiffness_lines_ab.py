#!/usr/bin/env python3
"""Per-launch time of the gather-form stiffness kernels at config C2 (32^3 elements, N = 7, box numbering): the slab
form (fdd_stiffness_matrix_diag[_f32], fdd_sub_stiffness_matrix_gather_scaled[_f32]) against the line form
(fdd_stiffness_matrix_lines[_f32]) in one process, and whether the two give the same bits there.

    python tools/stiffness_lines_ab.py [--lib other/libfdd_hip.so] [--launches 30 --warmup 5 --rounds 2]
    python tools/stiffness_lines_ab.py --counters old|new     # a few launches of one double three-array instance, for rocprofv3 --pmc
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib  # noqa: E402
from microbench import box_Q, gll  # noqa: E402


def per_launch_us(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return t.min(), float(np.median(t)), t.max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="kernel library to time (default: the package's)")
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--counters", choices=("old", "new"), default=None)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    decls = lib.parse_header(os.path.join(lib.INCLUDE_DIR, "fdd_hip.h"))
    path = args.lib or lib.hip().path
    cdll = lib.hip().cdll if args.lib is None else ctypes.CDLL(path)
    tag = os.path.basename(path)

    def entry(name):
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = decls[name]
        return fn

    E, N = args.E, 7
    n3, ne = 512, E**3
    P = ne * n3
    (_, col, _), _, _, nodes = box_Q(E, N, dev)
    D64 = torch.tensor(gll(N)[2], dtype=torch.float64, device=dev)
    torch.manual_seed(7)
    G64 = [torch.rand(P, dtype=torch.float64, device=dev) + 0.5 for _ in range(6)]
    v64 = torch.rand(nodes, dtype=torch.float64, device=dev) - 0.5
    stream = lib.current_stream()

    def family(real, diag):
        f32 = real == 32
        dt = torch.float32 if f32 else torch.float64
        D, G, v = D64.to(dt), [g.to(dt) for g in G64], v64.to(dt)
        sfx = "_f32" if f32 else ""
        old = entry(("fdd_stiffness_matrix_diag" if diag else "fdd_sub_stiffness_matrix_gather_scaled") + sfx)
        new = entry("fdd_stiffness_matrix_lines" + sfx)
        out_old, out_new = torch.zeros(P, dtype=dt, device=dev), torch.zeros(P, dtype=dt, device=dev)
        Gp = lib.ptr_array(G)

        def run_old():
            rc = old(lib.ptr(out_old), lib.ptr(v), None, lib.ptr(col), lib.ptr(D), Gp, None, ne, N, stream)
            assert rc == 0, rc

        def run_new():
            return new(lib.ptr(out_new), lib.ptr(v), None, lib.ptr(col), lib.ptr(D), Gp, None, ne, N, diag, stream)

        return run_old, run_new, out_old, out_new, new is not None

    if args.counters:
        run_old, run_new, _, _, have = family(64, 1)
        for _ in range(3):
            if args.counters == "old":
                run_old()
            else:
                assert have and run_new() == 0
        torch.cuda.synchronize()
        return

    for real in (64, 32):
        for diag in (1, 0):
            name = f"{'three' if diag else 'six'}-array {'float' if real == 32 else 'double'}"
            run_old, run_new, out_old, out_new, have = family(real, diag)
            built = have and run_new() == 0
            torch.cuda.synchronize()
            if built:
                run_old()
                torch.cuda.synchronize()
                same = torch.equal(out_old.view(torch.int32), out_new.view(torch.int32))
                print(f"{tag} {name}: line form bits == slab form bits at {E}^3 elements: {same}", flush=True)
            for r in range(args.rounds):
                o = per_launch_us(run_old, args.launches, args.warmup)
                line = f"{tag} round {r} {name} slab form us (min, median, max): {o[0]:.1f} {o[1]:.1f} {o[2]:.1f}"
                if built:
                    w = per_launch_us(run_new, args.launches, args.warmup)
                    line += f"  line form us: {w[0]:.1f} {w[1]:.1f} {w[2]:.1f}"
                else:
                    line += "  line form: not built"
                print(line, flush=True)
            del out_old, out_new


if __name__ == "__main__":
    main()
