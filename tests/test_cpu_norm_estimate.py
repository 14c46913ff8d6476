"""The one statement of the norm from the projections (include/fdd_norm_estimate.h), without a GPU: the header compiled as
plain C against a Python restatement in IEEE doubles, at and around its bound, and what the host layer answers about the
flag "last_norm_from_projections" where the kernel library lacks the entries (tests/norm_estimate_cpu_walk.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import support as S

SHIM_DIR = os.path.join(S.HERE, "cpu_shim")
HOST_CPU_SO = os.path.join(SHIM_DIR, "_build", "libfdd_host_cpu.so")

WRAPPER = """
#include "fdd_norm_estimate.h"
int norm2_from_projections(double aa, const double *h, int m, double *est) { return fdd_norm2_from_projections(aa, h, m, est); }
"""


def restated(aa, h):
    aa = float(aa)
    e = aa
    for x in h:
        hh = float(x) * float(x)
        e = e - hh
    finite = (aa - aa == 0.0) and (e - e == 0.0)
    return e, int(finite and e >= aa * 2.0 ** -10)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    d = tmp_path_factory.mktemp("norm_estimate")
    src, so = d / "wrapper.c", d / "libwrapper.so"
    src.write_text(WRAPPER)
    subprocess.check_call(["cc", "-O2", "-std=gnu99", "-shared", "-fPIC", "-I", os.path.join(S.ROOT, "include"), "-o", str(so), str(src)])
    fn = ctypes.CDLL(str(so)).norm2_from_projections
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return fn


def ask(fn, aa, h):
    h = np.ascontiguousarray(h, dtype=np.float64)
    est = ctypes.c_double(-1.0)
    ok = fn(ctypes.c_double(aa), h.ctypes.data, len(h), ctypes.byref(est))
    return est.value, ok


def test_the_function_is_its_restatement(compiled):
    rng = np.random.default_rng(7)
    for m in range(0, 8):
        for _ in range(200):
            h = rng.uniform(-1.0, 1.0, m)
            hh = float((h * h).sum())
            aa = hh + 10.0 ** rng.uniform(-20, 1) * rng.choice([1.0, 1.0, 1.0, -1.0])
            got, want = ask(compiled, aa, h), restated(aa, h)
            assert got == want or (got[1] == want[1] == 0 and got[0] != got[0] and want[0] != want[0]), (aa, h, got, want)


def test_the_bound_and_what_is_not_finite(compiled):
    h = np.array([0.5, -0.25])  # squares 0.25 and 0.0625: every number below is exact
    hh = 0.3125
    at = hh / (1.0 - 2.0 ** -10)  # est = aa * 2^-10 up to the rounding of the division
    # usable from aa = hh (1 + x) with x = 2^-10 / (1 - 2^-10) = 0.0009775... on
    for aa, usable in ((1.0, 1), (hh * 1.0009, 0), (hh * 1.001, 1), (hh, 0), (0.5 * hh, 0), (np.inf, 0), (-1.0, 0)):
        est, ok = ask(compiled, aa, h)
        assert ok == usable and (est, ok) == restated(aa, h), (aa, est, ok)
    assert ask(compiled, np.nan, h)[1] == 0
    assert abs(ask(compiled, at, h)[0] / at - 2.0 ** -10) < 1e-15
    assert ask(compiled, 0.0, np.zeros(3)) == (0.0, 1)  # a zero vector: the step stops on alpha = 0 as it did
    assert ask(compiled, 1.0, np.array([np.nan]))[1] == 0 and ask(compiled, 1.0, np.array([np.inf]))[1] == 0
    assert ask(compiled, 2.0, np.array([1.0]))[0] == 1.0 and ask(compiled, 1.0, [])[0] == 1.0


def test_the_cpu_build_keeps_the_exact_pass():
    subprocess.check_call(["make", "-C", S.ORACLE_DIR, "-s"])
    subprocess.check_call(["make", "-C", SHIM_DIR, "-s"])
    out = subprocess.run([sys.executable, os.path.join(S.HERE, "norm_estimate_cpu_walk.py"), HOST_CPU_SO], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["set_1"][0] != 0 and "fdd_multi_weighted_inner_product_self" in report["set_1"][1]
    assert report["set_0"] == [0, ""] and report["finite"]
    assert report["counters"] == {"estimated": 0, "exact": 0, "min_ratio": 0.0}
    assert report["nosub"][0] != 0 and "Subdomain" in report["nosub"][1]
