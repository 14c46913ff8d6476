#!/usr/bin/env python3
"""Per-launch time of the shared line stiffness kernel at config C2's shape (32^3 elements, N = 7, box numbering, one factor
block repeated): the parent instance (fdd_stiffness_matrix_lines_shared[_f32]) against the lean one
(fdd_stiffness_matrix_lines_lean[_f32] with the same factor_elem) in one process, double and float, gather and local form.
The two must give the same values (the sign of a zero may differ): asserted.

    python tools/lean_line_ab.py [--lib other/libfdd_hip.so] [--launches 30 --warmup 5 --rounds 2]
    python tools/lean_line_ab.py --counters parent|lean     # a few launches of the double gather instance, for rocprofv3 --pmc

A development build of the kernel library (csrc compiled with -DFDD_LEAN_LINE_DEV) also holds each part of the lean kernel
alone and exports fdd_dev_lean_line_parts to choose among them; given such a library with --lib, every part it holds is
timed against the parent as well: 1 = the zero terms and the sums that start from a product, 3 = that with D_hat resident
in scalar registers; the build that was measured for HISTORY also had 4 = the factor loads requested ahead of the gather
alone and 7 = all three.
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

PARTS = {1: "zero terms", 3: "zero terms + resident D_hat", 4: "hoisted factor loads", 7: "all three"}


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
    ap.add_argument("--lib", default=None, help="kernel library to time (default: the package's)")
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--counters", choices=("parent", "lean"), default=None)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    decls = lib.parse_header(os.path.join(lib.INCLUDE_DIR, "fdd_hip.h"))
    path = args.lib or lib.hip().path
    cdll = lib.hip().cdll if args.lib is None else ctypes.CDLL(path)
    set_parts = getattr(cdll, "fdd_dev_lean_line_parts", None)

    def entry(name):
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = decls[name]
        return fn

    E, N, n3 = args.E, 7, 512
    ne = E**3
    P = ne * n3
    (_, col, _), _, _, nodes = box_Q(E, N, dev)
    D64 = torch.tensor(gll(N)[2], dtype=torch.float64, device=dev)
    torch.manual_seed(7)
    rep = torch.zeros(ne, dtype=torch.int32, device=dev)
    G64 = [(torch.rand(n3, dtype=torch.float64, device=dev) + 0.5).repeat(ne).contiguous() for _ in range(3)]
    v64 = torch.rand(nodes, dtype=torch.float64, device=dev) - 0.5
    u64 = torch.rand(P, dtype=torch.float64, device=dev) - 0.5
    stream = lib.current_stream()
    print(f"{ne} elements, one factor block, {os.path.basename(path)}{' (development build: parts)' if set_parts else ''}", flush=True)

    def family(real, form):
        dt = torch.float32 if real == 32 else torch.float64
        sfx = "_f32" if real == 32 else ""
        D, G = D64.to(dt), [g.to(dt) for g in G64]
        src, idx = (v64.to(dt), col) if form == "gather" else (u64.to(dt), None)
        out_a, out_b = torch.zeros(P, dtype=dt, device=dev), torch.zeros(P, dtype=dt, device=dev)
        Gp = lib.ptr_array(G + [None] * 3)
        parent_fn, lean_fn = entry("fdd_stiffness_matrix_lines_shared" + sfx), entry("fdd_stiffness_matrix_lines_lean" + sfx)
        keep = (D, G, src, Gp)

        def parent():
            rc = parent_fn(lib.ptr(out_a), lib.ptr(src), None, lib.ptr(idx), lib.ptr(D), Gp, None, lib.ptr(rep), ne, N, 1, stream)
            assert rc == 0, rc

        def lean():
            rc = lean_fn(lib.ptr(out_b), lib.ptr(src), None, lib.ptr(idx), lib.ptr(D), Gp, None, lib.ptr(rep), ne, N, 1, stream)
            assert rc == 0, rc

        return parent, lean, out_a, out_b, keep

    if args.counters:
        parent, lean, _, _, keep = family(64, "gather")
        for _ in range(3):
            (parent if args.counters == "parent" else lean)()
        torch.cuda.synchronize()
        return

    for real in (64, 32):
        for form in ("gather", "local"):
            parent, lean, out_a, out_b, keep = family(real, form)
            name = f"{'float' if real == 32 else 'double'} {form}"
            parent()
            choices = [c for c in PARTS if set_parts(c) == 0] if set_parts else [None]  # a part the build does not hold is refused
            for parts in choices:
                if set_parts:
                    assert set_parts(parts) == 0
                out_b.zero_()
                lean()
                torch.cuda.synchronize()
                assert torch.equal(out_a, out_b) and float(out_a.abs().max()) > 0.0, (real, form, parts)  # -0.0 == 0.0
            # within a round the parent and every choice follow one another, so that a drift of the clock meets them all
            for r in range(args.rounds):
                a = per_launch_us(parent, args.launches, args.warmup)
                line = f"round {r} {name}: same values; parent us (min, median): {a[0]:.1f} {a[1]:.1f}"
                for parts in choices:
                    if set_parts:
                        assert set_parts(parts) == 0
                    b = per_launch_us(lean, args.launches, args.warmup)
                    line += f"  lean{'' if parts is None else ' [' + PARTS[parts] + ']'} us: {b[0]:.1f} {b[1]:.1f}"
                print(line, flush=True)
            if set_parts:
                set_parts(0)  # back to the release build's choice
            del out_a, out_b, keep


if __name__ == "__main__":
    main()
