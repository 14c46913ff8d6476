#!/usr/bin/env python3
"""Generate tests/golden/okl_kernels.json from the REFERENCE's own OKL kernels.

Runs only where oracle/_ref is built (`make -C oracle ref`: the reference's domain.okl, subdomain.okl, math.okl and
csr_matrix.okl rewritten to their OCCA-Serial loop nests by oracle/okl_serial.sed and compiled with g++ -O2
-ffp-contract=off, ten libraries).  For every case of tests/okl_cases.py the fixture records the SHA-256 of each
output array that the reference-compiled kernel returns, and for every library the kernel names it exports: recorded
results and a list of names, no program text.

    python tests/golden/make_okl_golden.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import okl_cases as C  # noqa: E402
import support as S  # noqa: E402


def exported(tag):
    """the functions a library defines and exports (nm -D), without the linker's own _init / _fini"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.okl_ref_so(tag)], text=True)
    return sorted(w[2] for w in (line.split() for line in out.splitlines()) if len(w) == 3 and w[1] == "T" and not w[2].startswith("_"))


def main():
    assert C.ref_built(), "oracle/_ref is not built: run `make -C oracle ref` where the reference is readable"
    golden = {
        "source": "domain.okl, subdomain.okl, math.okl, csr_matrix.okl through oracle/okl_serial.sed, g++ -O2 -ffp-contract=off, BLOCK_SIZE = 128, POLY_DEGREE = 15..1",
        "exports": {tag: exported(tag) for tag in sorted(C.REF_LIBS)},
        "cases": {},
    }
    for row, case in C.CASES:
        got = row.ref(C.ref_lib(case.lib), case, row.inputs(case))
        golden["cases"][case.id] = {name: C.sha(a) for name, a in sorted(got.items())}
    with open(C.GOLDEN, "w") as fh:
        json.dump(golden, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", C.GOLDEN, os.path.getsize(C.GOLDEN), "bytes,", len(golden["cases"]), "cases")


if __name__ == "__main__":
    main()
