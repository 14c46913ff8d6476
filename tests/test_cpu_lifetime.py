"""Who owns the host layer's device memory, on the CPU build (tests/cpu_shim): cpu_shim/lifetime_main.cpp walks problems
through every owner -- hierarchy and its rebuilds, float and Chebyshev-Jacobi inner solves, stepped and projected solves, a
forced composite -- and requires fdd_live_objects back at its baseline after each destroy.  The program, the host layer, the
stand-in and the oracle's kernels are one executable under AddressSanitizer, so a use after free, a double free or an
out-of-bounds read of a "device" block, and a host leak at exit, are its reports.  Nothing is preloaded."""
import os
import subprocess

import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
PROGRAM = os.path.join(SHIM_DIR, "_build", "lifetime_asan")


def test_every_owner_gives_back_what_it_took():
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s", "_build/lifetime_asan"])
    out = subprocess.run([PROGRAM], capture_output=True, text=True, timeout=600)
    report = out.stdout[-3000:] + out.stderr[-6000:]
    assert out.returncode == 0, report
    assert out.stdout.rstrip().split("\n")[-1] == "ok", report
    assert "AddressSanitizer" not in out.stderr, report
