"""Reconfiguring a live problem equals building a fresh one, on the CPU build of the host layer (tests/cpu_shim): every
walk of reconfigure_walks.py in a child process of its own.  The outputs of each step of a problem walked through a list
of configurations are the bits a fresh problem gives at that configuration -- a stale buffer, a cache that outlives its
setting or a captured sequence that no longer matches shows as a named transition.  tests/run_asan.sh runs this file with
the host layer under AddressSanitizer: that is what sees a host heap overwrite reliably (the outer GMRES arrays sized for
another num_vectors were one).

The workload's inputs change with the step, so that kept state cannot coincide with what the new step computes.

Left out here by name (reconfigure_walks.CPU_LEFT_OUT): the walk whose hierarchy is built with "amg_device_setup", which
the CPU stand-in of the kernel library has no entries for; test_gpu_reconfigure.py runs it."""
import os
import subprocess
import sys

import pytest

import reconfigure_walks as R
import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


@pytest.fixture(scope="module")
def cpu_host_lib():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    assert os.path.exists(HOST_CPU_SO)
    return HOST_CPU_SO


def test_the_walk_tables_cover_what_they_claim():
    """every family grows and shrinks a size, ends on a configuration of its own (configurations() asserts it) and has a walk
    whose last step is also held to the oracle; the refusals name steps that exist; only the device-built hierarchy is
    left out on the CPU"""
    for name, walk in R.WALKS.items():
        assert walk["family"] in R.FAMILIES
        assert len(R.configurations(walk, name)) == len(walk["steps"]) >= 3, name
    assert all(R.families_have_an_oracle_walk().values()), R.families_have_an_oracle_walk()
    for w, label, option in R.REFUSED:
        assert label in [s[0] for s in R.WALKS[w]["steps"]] and option in R.BASE
    assert sorted(set(R.WALKS) - set(R.walk_names(cpu=True))) == ["vcycle_device"]
    for key, sizes in (("num_vectors", [20, 10, 20, 3]), ("sub_num_vectors", [4, 8, 1, 7, 2]), ("sub_max_iterations", [9, 11, 1, 7, 5]), ("amg_cheby_order", [1, 4, 2, 3])):
        walk = {"num_vectors": "outer_basis_advice", "amg_cheby_order": "vcycle_host"}.get(key, "inner_krylov")
        seen = [c[key] for _, c in R.configurations(R.WALKS[walk], walk)]  # the values in force
        seen = [v for i, v in enumerate(seen) if i == 0 or v != seen[i - 1]]
        assert seen[: len(sizes)] == sizes, (key, seen)


@pytest.mark.parametrize("walk", R.walk_names(cpu=True))
def test_reconfigured_problem_equals_a_fresh_one(cpu_host_lib, walk):
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "reconfigure_walks.py"), cpu_host_lib, walk], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-4000:] + out.stderr[-4000:]


@pytest.mark.parametrize("name", sorted(R.ABANDONED))
def test_an_abandoned_stepwise_run_leaves_nothing_behind(cpu_host_lib, name):
    """reconfigure_walks.run_abandoned_stepwise: pcg_begin and pcg_steps(2) without pcg_solution, then two solves and a
    preconditioner application with another right-hand side, against a fresh problem given the same three calls"""
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "reconfigure_walks.py"), cpu_host_lib, name], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-4000:] + out.stderr[-4000:]
