"""The switch "amg_device_setup" on the CPU build of the host layer (tests/cpu_shim): the C-ABI stand-in there does not
define the fdd_amg_setup_* entries, the host layer references them weakly, so it still loads -- and refuses the switch,
naming the entry it lacks, instead of failing later inside a build."""
import os
import subprocess
import sys

import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


def test_device_setup_flag_names_the_missing_entry_on_the_cpu_shim():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    code = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H, lib
lib._host = lib._Lib(%r, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
H.init(0, use_torch_stream=False); H.comm_single(); H.set_print(False)
p = H.Problem.box((2, 2, 2), (1, 1, 1), 3, 2, True)
p.set_flag("amg_device_setup", 0)  # off: accepted, nothing changes
assert p.amg_setup_info() == {"levels_built_on_device": 0, "setup_seconds": 0.0}, p.amg_setup_info()
try:
    p.set_flag("amg_device_setup", 1)
except lib.FddError as e:
    print("refused:", e)
else:
    raise SystemExit("the switch was accepted without the kernel entries")
""" % (S.ROOT, S.HERE, HOST_CPU_SO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused:" in out.stdout and "fdd_amg_setup_" in out.stdout, out.stdout
    assert "amg_device_setup" in out.stdout
