#!/usr/bin/env python3
"""Per-launch time of one application of Qt A_L Q at config C2's shape (32^3 elements, N = 7, one factor block repeated):
the old pair of kernels -- the lean shared line kernel into the point buffer (fdd_stiffness_matrix_lines_lean), then the
whole boolean gather Qt (fdd_csr_plan_dssum, mode 1) -- against the new pair -- the same instance completing the single and
pair rows itself (fdd_stiffness_matrix_lines_direct), then the gather of the general rows (fdd_csr_plan_gather_mapped) -- in
one process.  The classes of Qt's rows are the host layer's (fddh_problem_assembly_arrays).  Both pairs must write the same
bits into every dof: asserted.

    python tools/assemble_ab.py [--E 32 --launches 30 --warmup 5 --rounds 2]
    FDD_TUNE_ASSEMBLE_NT_STORE=1 python tools/assemble_ab.py     # non-temporal stores of the rows the kernel completes
    python tools/assemble_ab.py --counters old|new                # a few launches of one pair, for rocprofv3 --pmc
    python tools/assemble_ab.py --instance parent                 # the shared instance that is not lean (lean_line_stiffness = 0)
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

from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H, lib  # noqa: E402
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd.kernels import k  # noqa: E402
from lean_line_ab import per_launch_us  # noqa: E402
from microbench import gll  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--counters", choices=("old", "new"), default=None)
    ap.add_argument("--instance", choices=("lean", "parent"), default="lean", help="which shared instance of the line kernel both pairs run")
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    H.init(0)
    H.comm_single()
    H.set_print(False)
    E, N, n3 = args.E, 7, 512
    p = H.Problem.box((E, E, E), (1, 1, 1), N, 6, True)
    pd = p.sub_point_dofs()
    pcd, rptr, rcol, rmap = p.assembly_arrays()
    info = p.assembly_info()
    p.close()
    ne, npts, nd = E**3, len(pd), int(pd.max()) + 1
    pts = np.flatnonzero(pd >= 0)
    order = np.argsort(pd[pts], kind="stable")
    ptr = np.zeros(nd + 1, np.int64)
    np.add.at(ptr, pd[pts] + 1, 1)
    ptr, col = np.cumsum(ptr).astype(np.int32), pts[order].astype(np.int32)

    def plan_of(row_ptr):
        h = ctypes.c_void_p()
        lib.hip().call("fdd_csr_plan_create", ctypes.byref(h), lib.ptr(row_ptr), len(row_ptr) - 1, npts, int(row_ptr[-1]))
        lib.hip().call("fdd_csr_plan_set_unit_values", h, 1)
        blocks = ctypes.c_int()
        lib.hip().call("fdd_csr_plan_num_blocks", h, ctypes.byref(blocks))
        return h, blocks.value

    plan, blocks = plan_of(ptr)
    rplan, rblocks = plan_of(rptr)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dpd, dpcd, dptr, dcol, drptr, drcol, drmap = (t(a) for a in (pd, pcd, ptr, col, rptr, rcol, rmap))
    torch.manual_seed(7)
    D = torch.tensor(gll(N)[2], dtype=torch.float64, device=dev)
    G = [(torch.rand(n3, dtype=torch.float64, device=dev) + 0.5).repeat(ne).contiguous() for _ in range(3)] + [None] * 3
    rep = torch.zeros(ne, dtype=torch.int32, device=dev)
    v = torch.rand(nd, dtype=torch.float64, device=dev) - 0.5
    q_old, q_new = torch.zeros(npts, dtype=torch.float64, device=dev), torch.zeros(npts, dtype=torch.float64, device=dev)
    y_old, y_new = torch.zeros(nd, dtype=torch.float64, device=dev), torch.full((nd,), float("nan"), dtype=torch.float64, device=dev)
    print(f"{ne} elements, {nd} dofs; rows {info['rows']}, points {info['points']}; row blocks {blocks} -> {rblocks}; "
          f"{args.instance} shared instance; non-temporal stores of y: {os.environ.get('FDD_TUNE_ASSEMBLE_NT_STORE', '0')}", flush=True)
    lean = args.instance == "lean"

    def old_stiffness():
        k("fdd_stiffness_matrix_lines_lean" if lean else "fdd_stiffness_matrix_lines_shared", q_old, v, None, dpd, D, G, None, rep, ne, N, 1)

    def old_gather():
        k("fdd_csr_plan_dssum", plan, None, y_old, dptr, dcol, q_old, None, None, 0, nd, 1)

    def new_stiffness():
        k("fdd_stiffness_matrix_lines_direct", q_new, y_new, v, None, dpcd, D, G, None, rep, int(lean), ne, N, 1)

    def new_gather():
        k("fdd_csr_plan_gather_mapped", rplan, y_new, drmap, drptr, drcol, q_new)

    def old_pair():
        old_stiffness()
        old_gather()

    def new_pair():
        new_stiffness()
        new_gather()

    if args.counters:
        for _ in range(3):
            (old_pair if args.counters == "old" else new_pair)()
        torch.cuda.synchronize()
        return

    old_pair()
    new_pair()
    torch.cuda.synchronize()
    assert torch.equal(y_old.view(torch.int64), y_new.view(torch.int64)) and float(y_old.abs().max()) > 0.0, "the two pairs differ"
    # within a round the six timings follow one another, so that a drift of the clock meets them all
    for r in range(args.rounds):
        line = f"round {r}: same bits; us per launch (min, median):"
        for name, fn in (("old stiffness", old_stiffness), ("old gather", old_gather), ("old pair", old_pair), ("new stiffness", new_stiffness), ("new gather", new_gather), ("new pair", new_pair)):
            a = per_launch_us(fn, args.launches, args.warmup)
            line += f"  {name} {a[0]:.1f} {a[1]:.1f}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
