"""The verdicts the host layer reaches per element list (host/element_operator.hpp: detect_zero_factors, detect_shared_blocks,
detect_affine, direct_lines_apply) on meshes where only some elements qualify: one bumped element in a box -- first, last,
past the first workgroup of the detection pass --, lists that qualify on one level and not on another, graded diagonal lists,
a sheared box whose off-diagonal constants are not zero, and single edited entries.  The meshes and the numpy restatements
of the verdicts are tests/partial_meshes.py, the cases and the library-independent checks tests/partial_list_checks.py (the
CPU twin is tests/test_cpu_partial_lists.py); the table of cases, with measured figures, is in tests/README.md.

Per case, on one rank, in double and with the float preconditioner:
 1. the problem's mesh arrays have the bits that were written;
 2. every fddh_problem_*_info answer is what stiffness_choice_rules gives for the restated verdicts of the lists, and the
    profile labels of a short solve are among the labels the rules allow for the lists of the levels, at the bytes per
    launch of those lists (test_gpu_stiffness_choice.check_step, given the per-level states), with all flags on, and with
    "affine_geometry" asked for;
 3. - 5. stiffness, inner operator and its diagonal against numpy on the written arrays to 1e-12, and the same restatement
    under the wrong verdict off by at least 1e-3 (partial_list_checks.operator);
 6. stiffness, preconditioner application and stepped PCG with the six flags that act on a verdict all off and all on
    ("skip_zero_factors", "mfma_skip_zero_factors", "line_stiffness", "shared_factor_blocks", "lean_line_stiffness",
    "assemble_in_stiffness": the ones documented to leave the operator's values alone; "mfma_stiffness" stays on, it acts on
    the degree and changes rounding): bit-identical where no list of any level holds a three-array verdict, equal as values
    (up to the sign of a zero) where one does;
 7. on the bumped boxes, whose factors belong to their coordinates, a full outer FCG solve against the CPU oracle.
"""
import time

import numpy as np
import pytest

import partial_list_checks as C
import partial_meshes as M
import stiffness_choice_rules as R
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from test_gpu_stiffness_choice import check_step
from test_gpu_stiffness_diag import same_values
from test_gpu_stiffness_shared_factors import same_bits, two_steps

pytestmark = pytest.mark.gpu

VERDICT_FLAGS = ("skip_zero_factors", "mfma_skip_zero_factors", "line_stiffness", "shared_factor_blocks", "lean_line_stiffness", "assemble_in_stiffness")
NO_LINE_FORM = "a list does not run the degree-7 line form"
EPS64 = 64 * np.finfo(float).eps


@pytest.fixture(scope="module")
def setup(gpu):
    H.init(0)
    H.comm_single()
    H.set_print(False)
    return True


def expected_by_the_issue(case, p, plain, asked, N):
    """what the table of cases states outright, next to the restated verdicts: all flags on, double"""
    zero, lines, shared, mfma = p.zero_factor_info(), p.line_stiffness_info(), p.shared_factor_info(), p.mfma_zero_factor_info()
    three = lambda info, key: (info["fine_domain"], info[key])
    if case.startswith("bumped_") and "sheared" not in case:
        # the finest list does not qualify, the degree-1 list of the same problem does
        assert not plain[N][3] and plain[1][3] and plain[1][4] and all(not plain[d][3] for d in plain if d > 1), plain
        assert three(zero, "sub_lists_diag") == three(lines, "sub_lists_lines") == three(shared, "sub_lists_shared") == three(mfma, "sub_lists_mfma_diag") == (False, 0)
        assert shared["fine_domain_classes"] == 0  # not looked for
        assert three(p.lean_line_info(), "sub_lists_lean") == (False, 0)
        ai = p.assembly_info()
        assert ai["enabled"] and not ai["in_effect"] and ai["why_not"] == NO_LINE_FORM, ai
        assert not asked[N][2] and asked[1][2]  # "affine_geometry" would switch the degree-1 list alone
    elif case == "graded_333_N7_e26":
        assert three(zero, "sub_lists_diag") == three(lines, "sub_lists_lines") == three(shared, "sub_lists_shared") == (True, 1) and shared["fine_domain_classes"] == 2
        assert not asked[N][2]
    elif case == "graded_333_N7_e13_to_26":
        assert three(zero, "sub_lists_diag") == three(lines, "sub_lists_lines") == (True, 1) and three(shared, "sub_lists_shared") == (False, 0) and shared["fine_domain_classes"] == 15
    elif case.startswith("sheared_"):
        assert all(not st[3] for st in plain.values()) and all(st[2] for st in asked.values())
        assert three(zero, "sub_lists_diag") == three(lines, "sub_lists_lines") == three(mfma, "sub_lists_mfma_diag") == (False, 0)
    elif case.startswith("bumped_sheared"):
        assert all(not st[3] for st in plain.values()) and not asked[N][2]
        assert three(zero, "sub_lists_diag") == (False, 0)
    elif case.endswith("denormal"):
        assert not plain[N][3] and three(zero, "sub_lists_diag") == three(lines, "sub_lists_lines") == (False, 0) and p.assembly_info()["why_not"] == NO_LINE_FORM
    elif case.endswith("minus_zero"):
        assert three(zero, "sub_lists_diag") == three(lines, "sub_lists_lines") == three(shared, "sub_lists_shared") == (True, 1) and shared["fine_domain_classes"] == 1
    else:
        raise AssertionError(case)


@pytest.mark.parametrize("case", list(C.CASES))
def test_lists_of_which_only_some_elements_qualify(setup, tmp_path, case):
    spec = C.CASES[case]
    N, red = spec["N"], spec["red"]
    t0 = time.time()
    p, meshes = C.open_problem(H, case, str(tmp_path / "mesh"))
    try:
        elements = meshes[N].E
        C.written_bits(p, meshes)
        lean = (R.lean_table_ok(S.gll(7)[2], False), R.lean_table_ok(S.gll(7)[2], True))
        plain = {d: M.list_state(mesh, None, False, lean) for d, mesh in meshes.items()}
        asked = {d: M.list_state(mesh, None, True, lean) for d, mesh in meshes.items()}
        assert all(R.reachable(*st) for st in list(plain.values()) + list(asked.values()))
        any_verdict = any(st[3] for st in plain.values())
        flags = {name: True for name in R.FLAGS}
        for name in R.FLAGS + ("assemble_in_stiffness",):
            p.set_flag(name, 1)
        expected_by_the_issue(case, p, plain, asked, N)
        deviation = M.affine_deviation(meshes[N])
        for precision in (64, 32):
            p.set_flag("preconditioner_precision", precision)
            # 2. the info answers and the labels of a short solve, as the lists stand and with the affine form asked for
            check_step(p, N, case, precision, flags, False, 80, state=plain.__getitem__, elements=elements, reduction=red)
            assert p.shared_factor_info()["fine_domain_classes"] == (M.factor_classes(meshes[N]) if plain[N][3] else 0)
            ai, sub_lines = p.assembly_info(), R.info(plain[N], flags, precision == 32)["lines"]
            want_why = "the inner solve runs in float" if precision == 32 else "" if sub_lines else NO_LINE_FORM
            assert (ai["enabled"], ai["in_effect"], ai["why_not"]) == (True, want_why == "", want_why), (ai, plain[N])
            p.set_flag("affine_geometry", 1)
            check_step(p, N, case, precision, flags, False, 81, state=asked.__getitem__, elements=elements, reduction=red)
            info = p.affine_info()
            if asked[N][2]:
                assert 0.0 <= info["max_deviation"] <= EPS64 and deviation <= EPS64, (info, deviation)
            else:
                assert abs(info["max_deviation"] - deviation) <= 1e-9 * deviation and deviation > 1e-6, (info, deviation)
            p.set_flag("affine_geometry", 0)
            # 6. the flags that act on a verdict: all on against all off
            on = two_steps(p, 90)
            for name in VERDICT_FLAGS:
                p.set_flag(name, 0)
            off_flags = {name: name == "mfma_stiffness" for name in R.FLAGS}
            check_step(p, N, case, precision, off_flags, False, 82, state=plain.__getitem__, elements=elements, reduction=red)
            off = two_steps(p, 90)
            for name in VERDICT_FLAGS:
                p.set_flag(name, 1)
            (same_values if any_verdict else same_bits)(on, off)
            assert np.abs(on["stiffness"]).max() > 0.0 and on["r2"][0] > 0.0
        p.set_flag("preconditioner_precision", 64)
        print("%s: affine deviation %.3e; a list of some level holds a three-array verdict: %s" % (case, deviation, any_verdict))
        # 3. - 5.
        C.operator(p, meshes[N], spec["wrong"], case, asked[N][2])
        # 7.
        if spec["oracle"]:
            C.oracle_solve(p, N, red, case)
    finally:
        p.close()
    print("%s: %.2f s" % (case, time.time() - t0))
