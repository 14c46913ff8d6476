"""What the host C API refuses, on the package's own libfdd_host.so: the walk of tests/capi_refusals.py, once, in one child
process, against the rows of tests/capi_refusals_expected.tsv whose return code is not 0 (tests/test_cpu_capi_refusals.py
says where the table comes from).  Each of those calls is refused before it reaches the device.

The table was recorded on the CPU stand-in of the kernel library, which lacks the entries some flags need: a row whose
refusal is "... which the loaded kernel library does not export" cannot be asked of the product's library, which build()
makes with every entry.  Those calls must be accepted here."""
import os
import subprocess
import sys

import pytest

import support as S

pytestmark = pytest.mark.gpu

NOT_EXPORTED = "which the loaded kernel library does not export"


def test_every_refusal_answers_as_on_the_cpu_build(gpu):
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

    out = subprocess.run([sys.executable, os.path.join(S.HERE, "capi_refusals.py"), lib.host().path, "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    got = out.stdout.splitlines()
    with open(os.path.join(S.HERE, "capi_refusals_expected.tsv")) as fh:
        want = fh.read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    refused = 0
    for w, g in zip(want, got):
        situation, name, rc, text = w.split("\t")
        if rc == "0":
            assert g.split("\t")[:2] == [situation, name], (w, g)  # the same call: the walk's order is the table's
        elif text.endswith(NOT_EXPORTED):
            assert g == "\t".join((situation, name, "0", "")), (w, g)
        else:
            refused += 1
            assert w == g, (w, g)
    assert refused >= 4 * 54, refused  # at least the three situations that refuse every entry, and a fourth's worth beside them
