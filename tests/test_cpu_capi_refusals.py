"""What the host C API refuses, entry by entry and flag by flag, on the CPU build of the host layer (tests/cpu_shim): the
walk of tests/capi_refusals.py, in a child process (the stand-in library must not stay loaded in the test process), held
line for line to tests/capi_refusals_expected.tsv.

The table is the walk's output on the library as it was before the entries' openings were folded into one guard
(on_problem, host/fdd_host_capi.cpp), not on the code under test.  Six of its rows were then set by hand: fddh_problem_csr,
_assembled_weight and _amg_level_arrays did not ask whose thread was calling, and answered a thread that never ran
fddh_init with "null argument", "null argument" and "no Subdomain", and a second rank that was handed the first one's problem
with 0, "null argument" and "the hierarchy has 0 levels"; they now give the two texts of the rank check like every other entry."""
import os
import subprocess
import sys

import pytest

import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")
EXPECTED = os.path.join(S.HERE, "capi_refusals_expected.tsv")


@pytest.fixture(scope="module")
def cpu_host_lib():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    assert os.path.exists(HOST_CPU_SO)
    return HOST_CPU_SO


def test_every_refusal_and_every_flag_answers_as_before(cpu_host_lib):
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "capi_refusals.py"), cpu_host_lib, "cpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    got = out.stdout.splitlines()
    with open(EXPECTED) as fh:
        want = fh.read().splitlines()
    differing = [(w, g) for w, g in zip(want, got) if w != g]
    assert len(got) == len(want) and not differing, "%d lines, expected %d; first differing (expected, got): %r" % (len(got), len(want), differing[:5])
    # the table covers what it is meant to: the four situations over every entry, both flag walks
    for situation in ("uninit", "null", "foreign", "nosub", "flags_nosub", "flags_sub"):
        assert sum(line.startswith(situation + "\t") for line in want) >= 54, situation
