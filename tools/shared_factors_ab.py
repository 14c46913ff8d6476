#!/usr/bin/env python3
"""Per-launch time of the line stiffness kernel at config C2's shape (32^3 elements, N = 7, box numbering) on factor arrays
whose blocks repeat from element to element: the streamed instance (fdd_stiffness_matrix_lines[_f32], every element its own
copy) against the shared instance (fdd_stiffness_matrix_lines_shared[_f32], the few distinct blocks) in one process,
double and float, gather and local form.  The two must give the same bits: asserted.

    python tools/shared_factors_ab.py [--classes 1] [--launches 30 --warmup 5 --rounds 2]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib  # noqa: E402
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k  # noqa: E402
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
    return t.min(), float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--classes", type=int, default=1, help="distinct factor blocks; element e holds block e mod classes")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    E, N, n3 = args.E, 7, 512
    ne = E**3
    P = ne * n3
    (_, col, _), _, _, nodes = box_Q(E, N, dev)
    D64 = torch.tensor(gll(N)[2], dtype=torch.float64, device=dev)
    torch.manual_seed(7)
    rep = (torch.arange(ne, device=dev) % args.classes).to(torch.int32)
    G64 = [(torch.rand(args.classes, n3, dtype=torch.float64, device=dev) + 0.5)[rep.long()].reshape(-1).contiguous() for _ in range(3)]
    v64 = torch.rand(nodes, dtype=torch.float64, device=dev) - 0.5
    u64 = torch.rand(P, dtype=torch.float64, device=dev) - 0.5

    mism = torch.ones(1, dtype=torch.int32, device=dev)
    k("fdd_stiffness_factor_block_verify", mism, G64 + [None] * 3, None, rep, ne, N)
    assert int(mism.item()) == 0
    print(f"{ne} elements, {args.classes} distinct factor block(s), {os.path.basename(lib.hip().path)}", flush=True)

    for real in (64, 32):
        dt = torch.float32 if real == 32 else torch.float64
        sfx = "_f32" if real == 32 else ""
        D, G = D64.to(dt), [g.to(dt) for g in G64] + [None] * 3
        for form in ("gather", "local"):
            src, idx = (v64.to(dt), col) if form == "gather" else (u64.to(dt), None)
            out_a, out_b = torch.zeros(P, dtype=dt, device=dev), torch.zeros(P, dtype=dt, device=dev)

            def streamed():
                k("fdd_stiffness_matrix_lines" + sfx, out_a, src, None, idx, D, G, None, ne, N, 1)

            def shared():
                k("fdd_stiffness_matrix_lines_shared" + sfx, out_b, src, None, idx, D, G, None, rep, ne, N, 1)

            streamed()
            shared()
            torch.cuda.synchronize()
            assert torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)) and float(out_a.abs().max()) > 0.0, (real, form)
            name = f"{'float' if real == 32 else 'double'} {form}"
            for r in range(args.rounds):
                a = per_launch_us(streamed, args.launches, args.warmup)
                b = per_launch_us(shared, args.launches, args.warmup)
                print(f"round {r} {name}: same bits; streamed us (min, median): {a[0]:.1f} {a[1]:.1f}  shared us: {b[0]:.1f} {b[1]:.1f}", flush=True)
            del out_a, out_b


if __name__ == "__main__":
    main()
