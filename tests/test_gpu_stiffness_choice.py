"""The host layer's choice of stiffness kernel reaches the launch: on small problems whose lists between them run every family,
the flags are walked one after the other, and after a short solve at each step the profile labels recorded
(fddh_profile_enable / _collect) are held to the restatement in stiffness_choice_rules.py -- a subset of what the rules give
for the problem's lists in both forms, containing the gather label of the degree-N lists, with the bytes per launch of the
rules' table -- and so are the answers of the fddh_problem_*_info entries.  Bits are not compared here: the
test_gpu_stiffness_* files and the reconfigure walks do that.

Eight equal elements are one class of factor blocks (2 * classes <= elements: the shared instance applies), degree 11 is the
lowest on the matrix cores, and the Kershaw mesh keeps six arrays whatever the flags say."""
import numpy as np
import pytest

import stiffness_choice_rules as R
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H

pytestmark = pytest.mark.gpu

E, REDUCTION = (2, 2, 2), 6
FAMILY_PREFIXES = ("fused_stiffness", "diag_stiffness_kernel", "line_stiffness_kernel", "mfma_stiffness_kernel", "mfma_diag_stiffness_kernel")
WALK = [("lean_line_stiffness", 0), ("shared_factor_blocks", 0), ("line_stiffness", 0), ("skip_zero_factors", 0), ("affine_geometry", 1)]
WALK_11 = WALK[:3] + [("mfma_skip_zero_factors", 0)] + WALK[3:] + [("mfma_stiffness", 0)]


@pytest.fixture(scope="module")
def setup(gpu):
    H.init(0)
    H.comm_single()
    H.set_print(False)
    return True


def short_solve(p, seed):
    _, f = p.make_rhs_from(S.seeded_uniform(p.n, seed + 1))
    p.stiffness(S.seeded_uniform(p.n, seed))  # the local form
    p.precond_apply(f)  # the Subdomain's gather form, in the precision in use
    p.pcg_begin(f)
    assert p.pcg_steps(2) > 0.0  # the fine Domain's gather form


def bytes_fit(total, count, candidates):
    """is total exactly the sum of count launches, each of one of the candidate sizes?"""
    c = sorted(set(candidates))
    if not count * c[0] <= total <= count * c[-1]:
        return False
    if len(c) == 1:
        return True
    return any(bytes_fit(total - n * c[-1], count - n, c[:-1]) for n in range(count + 1))


def check_step(p, N, box, precision, flags, affine, seed, state=None, elements=E, reduction=REDUCTION):
    """state(d): what was established about the list of degree d (stiffness_choice_rules), for meshes whose lists differ from
    level to level (test_gpu_partial_lists.py); None: a box or a Kershaw mesh of `elements`, every level alike"""
    f32 = precision == 32
    n_elems = int(np.prod(elements))
    nodes = lambda d: int(np.prod([e * d + 1 for e in elements]))
    # the lists: one per Domain level (all of the same elements), and the Subdomain's one list of the rank's own elements
    state = state or (lambda d: (3, d, affine, box, box, box and d == 7, box and d == 7))
    sub_list, sub_gathered = state(N), p.sub_info()["sub_ext_dofs"]
    assert p.zero_factor_info()["sub_lists"] == 1
    sizes = {}

    def add(lst, form, in_place, single, gathered):
        label, per_point = R.profile(form, R.choose(lst, flags, single, form, in_place), single)
        if label:
            points = n_elems * (lst[1] + 1) ** 3
            sizes.setdefault(label, []).append(per_point * points + (0 if form == "local" else (4 if single else 8) * gathered))
        return label

    for d in S.level_degrees(N, reduction):
        for in_place in (False, True):
            add(state(d), "local", in_place, False, 0)
        add(state(d), "gather", False, False, nodes(d))  # the nodes of the box of elements of degree d
    for in_place in (False, True):
        add(sub_list, "local", in_place, False, 0)
    must = {add(state(N), "gather", False, False, p.info["num_local_nodes"]), add(sub_list, "gather", False, f32, sub_gathered)}
    assert nodes(N) == p.info["num_local_nodes"]

    _, record = S.profiled(lambda: short_solve(p, seed), records=True)
    got = {label for label in record if label.startswith(FAMILY_PREFIXES)}
    print(N, "box" if box else "kershaw", precision, flags, "affine" if affine else "", sorted(got))
    assert got <= set(sizes) and must <= got, (sorted(got), sorted(sizes), sorted(must))
    for label in got:
        assert bytes_fit(int(record[label]["bytes"]), record[label]["count"], sizes[label]) and record[label]["bytes"] == int(record[label]["bytes"]), (label, record[label], sizes[label])

    # the info entries: the fine Domain's list in double, the Subdomain's in the precision in use
    dom, sub = R.info(state(N), flags, False), R.info(sub_list, flags, f32)
    for name, kind, flag, key in ((p.zero_factor_info, "diag", "skip_zero_factors", "sub_lists_diag"), (p.mfma_zero_factor_info, "mfma_diag", "mfma_skip_zero_factors", "sub_lists_mfma_diag"),
                                  (p.line_stiffness_info, "lines", "line_stiffness", "sub_lists_lines"), (p.shared_factor_info, "shared", "shared_factor_blocks", "sub_lists_shared"),
                                  (p.lean_line_info, "lean", "lean_line_stiffness", "sub_lists_lean")):
        answer = name()
        assert (answer["enabled"], answer["fine_domain"], answer[key], answer["sub_lists"]) == (flags[flag], dom[kind], int(sub[kind]), 1), (flag, answer, dom, sub)
    answer = p.affine_info()
    assert (answer["fine_domain"], answer["sub_lists_affine"], answer["sub_lists"]) == (state(N)[2], int(sub_list[2]), 1), answer


@pytest.mark.parametrize("N,box,precision", [(7, True, 64), (7, True, 32), (11, True, 64), (7, False, 64)])
def test_the_choice_reaches_the_launch_at_every_step_of_the_flag_walk(setup, N, box, precision):
    p = H.Problem.box(E, (1, 1, 1), N, REDUCTION, True) if box else H.Problem.kershaw(E, (1, 1, 1), N, REDUCTION, 0.3, True)
    try:
        p.set_flag("preconditioner_precision", precision)
        flags = {name: True for name in R.FLAGS}
        for name in R.FLAGS:
            p.set_flag(name, 1)
        affine = False
        check_step(p, N, box, precision, flags, affine, 60)
        for step, (name, value) in enumerate(WALK_11 if N == 11 else WALK):
            p.set_flag(name, value)
            if name == "affine_geometry":
                affine = box  # only where the mesh's own factor arrays have that form: not on the Kershaw mesh
            else:
                flags[name] = bool(value)
            check_step(p, N, box, precision, flags, affine, 61 + step)
    finally:
        p.close()
