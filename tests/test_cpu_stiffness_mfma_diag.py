"""The flag "mfma_skip_zero_factors" on the CPU build of the host layer (tests/cpu_shim): the C-ABI stand-in there does not
define fdd_stiffness_matrix_mfma_diag, the host layer references it weakly, so it still loads, switches no list -- and refuses
the flag, naming the entry it lacks."""
import os
import subprocess
import sys

import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")


def test_mfma_zero_factor_flag_is_off_and_names_the_missing_entry_on_the_cpu_shim():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    code = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H, lib
lib._host = lib._Lib(%r, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
H.init(0, use_torch_stream=False); H.comm_single(); H.set_print(False)
p = H.Problem.box((1, 1, 2), (1, 1, 1), 11, 5, True)
assert p.level_degree(0) == 11
info = p.mfma_zero_factor_info()
assert info == {"enabled": False, "fine_domain": False, "sub_lists_mfma_diag": 0, "sub_lists": info["sub_lists"]} and info["sub_lists"] >= 1, info
p.set_flag("mfma_skip_zero_factors", 0)  # off: accepted, nothing changes
try:
    p.set_flag("mfma_skip_zero_factors", 1)
except lib.FddError as e:
    print("refused:", e)
else:
    raise SystemExit("the flag was accepted without the kernel entry")
assert p.mfma_zero_factor_info() == info
# a small degree-11 solve runs as before, on six arrays
u_star, f = p.make_rhs_from(S.seeded_uniform(p.n, 11))
u, its, hist = p.solve(f, "fcg")
assert 0 < its < 100 and hist[-1] < 1e-6 * hist[0], (its, hist)
assert np.abs(u - u_star).max() <= 1e-6 * np.abs(u_star).max()
print("solved in", its)
""" % (S.ROOT, S.HERE, HOST_CPU_SO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused:" in out.stdout and "fdd_stiffness_matrix_mfma_diag" in out.stdout, out.stdout
    assert "mfma_skip_zero_factors" in out.stdout and "solved in" in out.stdout
