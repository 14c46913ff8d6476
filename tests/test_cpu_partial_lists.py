"""Meshes on which only some elements qualify for a three-array, shared or affine kernel, on the CPU build of the host layer
(tests/cpu_shim): the builders of tests/partial_meshes.py against figures worked out beforehand, and of every case of
tests/partial_list_checks.py what does not need the product's kernels -- the written bits, stiffness, inner operator and its
diagonal against numpy on the written arrays (1e-12), the same restatement under the wrong verdict (off by at least 1e-3, the
figure that tells test_gpu_partial_lists.py's 1e-12 apart from a kernel that skipped arrays it needed), and on the bumped boxes
the outer solve against the oracle.  The stand-in has none of the three-array or line entries, so of the verdicts only the
affine one can switch a list here; one child process per check (the stand-in library must not stay loaded in the test process).

Figures on the stand-in (each check prints its own): operator against numpy at most 3.4e-16 max|ref|, inner operator 1.4e-15,
its diagonal 6.0e-16; under the wrong verdict the restatement is off by 5.0e-3 (one bumped element of 80 at degree 3; the
inner operator by 2.6e-3) to 2.2e-1 max|ref| (fourteen graded elements of 27); on the affine kernel the inner operator is
within 2.1e-15 and two PCG steps within 5.6e-15 of the streamed ones; outer FCG iterations equal the oracle's in all eight
solves (20, 33, 35), and in the two-rank case (FCG 67, GMRES 73)."""
import os
import subprocess
import sys

import pytest

import partial_list_checks as C
import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


@pytest.fixture(scope="module")
def cpu_host_lib():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    assert os.path.exists(HOST_CPU_SO)
    return HOST_CPU_SO


def run_check(lib_path, name):
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "partial_list_checks.py"), lib_path, name], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-6000:] + out.stderr[-4000:]
    return out.stdout


def test_builders_give_the_figures_worked_out_beforehand(cpu_host_lib):
    """one bumped element: the only one with non-zero g_4..g_6 (4 - 15 % of max|g_1|) and off the affine form (0.10 - 0.30, the
    others at most 5.2e-16), two blocks, the box at degree 1; the sheared box passes the affine bar in its analytic form at
    every degree and in isoparametric form only up to degree 2; 2 and 15 classes on the graded lists"""
    out = run_check(cpu_host_lib, "builders")
    assert out.count("bumped (3,3,3) N =") == 5 and out.count("sheared (3,2,2) N =") == 4


def _two_rank_worker(rank, world, rdzv, mesh_dir):
    import torch.distributed as dist

    import rendezvous
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

    # test-only: serve include/fdd_host.h from the CPU build of the host layer
    lib._host = lib._Lib(HOST_CPU_SO, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
    rendezvous.init_gloo(rank, world, rdzv)
    try:
        H.init(0, use_torch_stream=False)
        H.set_print(False)
        H.comm_torch_callbacks(on_gpu=False)
        C.two_ranks(H, rank, world, mesh_dir, dist.barrier, product=False)
    finally:
        dist.destroy_process_group()


def test_the_offender_is_a_ring_element_pulled_from_the_other_rank(cpu_host_lib, tmp_path):
    """the two-rank composite of tests/test_gpu_comm.py's case under `gloo` on the stand-in: region, the restated verdicts of
    the region's three lists (nothing switches here), operators and outer solves against the oracle's world"""
    import rendezvous
    import torch.multiprocessing as mp

    mp.spawn(_two_rank_worker, args=(2, rendezvous.new(), str(tmp_path / "bumped")), nprocs=2, join=True)


@pytest.mark.parametrize("case", list(C.CASES))
def test_case_on_the_stand_in(cpu_host_lib, case):
    spec = C.CASES[case]
    out = run_check(cpu_host_lib, case)
    assert out.count("|Au - ref| / max|ref|") == 1 and out.count("under the wrong verdict") == (spec["wrong"] is not None) and out.count("outer FCG") == spec["oracle"]
