"""The outer PCG step with its residual norm and its solution update folded into neighbouring passes: the host layer's flags
"fused_residual_norm" and "solution_in_direction_pass" (each on by default), 0 against 1, bit for bit.

Each flag only moves statements between launches, so the bar is np.array_equal of the residual history and of the solution,
and the profile labels say that the path under test really ran (or, where its conditions do not hold, that it stayed out):

  fused_residual_norm           residual_update_norm_kernel: only on one rank with a preconditioner (the norm is the dof
                                slice's plain sum)
  solution_in_direction_pass    ew_kernel<SolutionDirectionDev>: wherever the node-space flexible CG keeps its scalars on the
                                device; the owed update is flushed by whatever reads the solution first

Shapes: 5x2x2 at degree 7 (pairs inside and across workgroups of the line kernel, a last workgroup with one element), 2x2x2
at degree 7, 3x3x3 at degree 3, Kershaw 4x2x2 at degree 7 (six factor arrays); two ranks of one process on 4x2x2."""
import ctypes

import numpy as np
import pytest

import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

pytestmark = pytest.mark.gpu

NORM, DIRECTION = "residual_update_norm_kernel", "ew_kernel<SolutionDirectionDev>"
FLAGS = {"fused_residual_norm": NORM, "solution_in_direction_pass": DIRECTION}


@pytest.fixture(scope="module")
def setup(gpu):
    H.init(0)
    H.comm_single()
    H.set_print(False)
    return True


def problem(shape):
    kind, E, N, red = shape
    p = H.Problem.kershaw(E, (1, 1, 1), N, red, 0.3, True) if kind == "kershaw" else H.Problem.box(E, (1, 1, 1), N, red, True)
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
    return p


def set_flags(p, values):
    for name, value in values.items():
        p.set_flag(name, value)


def five_steps(p, f):
    """(history of five single steps, the solution behind them, the norm and the solution of five lazy steps, labels)"""
    p.pcg_begin(f)
    single = [p.pcg_steps(1) for _ in range(5)]
    u_single = p.pcg_solution()
    p.pcg_begin(f)
    (last, u_lazy), labels = S.profiled(lambda: (p.pcg_steps(5), p.pcg_solution()))
    return {"history": np.array(single), "solution": u_single, "lazy_last": np.array([last]), "lazy_solution": u_lazy}, labels


def same_bits(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(np.asarray(a[key]).view(np.uint64), np.asarray(b[key]).view(np.uint64)), (what, key)


SHAPES = {
    "box_5x2x2_N7": ("box", (5, 2, 2), 7, 6),
    "box_2x2x2_N7": ("box", (2, 2, 2), 7, 6),
    "box_3x3x3_N3": ("box", (3, 3, 3), 3, 2),
    "kershaw_4x2x2_N7": ("kershaw", (4, 2, 2), 7, 6),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_each_flag_and_all_of_them_keep_every_bit(setup, name):
    p = problem(SHAPES[name])
    try:
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 97))
        set_flags(p, {flag: 0 for flag in FLAGS})
        base, labels = five_steps(p, f)
        assert not (set(FLAGS.values()) & labels), labels
        assert np.isfinite(base["solution"]).all() and (base["history"] > 0.0).all() and base["history"][-1] < base["history"][0]
        assert base["lazy_last"][0] == base["history"][-1] and np.array_equal(base["lazy_solution"], base["solution"])
        settings = [{flag: 1} for flag in FLAGS] + [{flag: 1 for flag in FLAGS}]
        for on in settings:
            set_flags(p, on)
            got, labels = five_steps(p, f)
            same_bits(got, base, (name, on))
            for flag, label in FLAGS.items():
                assert (label in labels) == (flag in on), (name, on, flag, sorted(labels))
            set_flags(p, {flag: 0 for flag in on})
    finally:
        p.close()


def test_the_owed_solution_update_is_not_lost(setup):
    """one step, then the solution: the update the residual half left to the direction half has been made; a solution
    read between further steps leaves them their bits"""
    p = problem(("box", (2, 2, 2), 7, 6))
    try:
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 98))
        got = {}
        for flag in (0, 1):
            p.set_flag("solution_in_direction_pass", flag)
            p.pcg_begin(f)
            r1 = p.pcg_steps(1)
            u1 = p.pcg_solution()
            u1_again = p.pcg_solution()
            r3 = p.pcg_steps(2)
            u3 = p.pcg_solution()
            assert np.array_equal(u1, u1_again)
            got[flag] = {"r": np.array([r1, r3]), "u1": u1, "u3": u3}
        assert np.abs(got[0]["u1"]).max() > 0.0 and not np.array_equal(got[0]["u1"], got[0]["u3"])
        same_bits(got[1], got[0], "owed")
    finally:
        p.close()


@pytest.mark.parametrize("lazy", [0, 1])
def test_a_solve_that_stops_behind_a_speculative_direction_half(setup, lazy):
    """solve_timed to 1e-7: the stopping test is read behind a direction half that already carried the solution update of the
    iteration it tests.  Iteration count, history and solution with the flags on equal those with them off."""
    p = problem(("box", (2, 2, 2), 7, 6))
    try:
        p.set_options(tolerance=1e-7)
        p.set_flag("lazy_steps", lazy)
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 99))
        got = {}
        for value in (0, 1):
            set_flags(p, {flag: value for flag in FLAGS})
            got[value] = solve_with_solution(p, f)
        assert got[0][0] == got[1][0] and got[0][0] > 1
        assert got[0][1][-1] <= 1e-7 * got[0][1][0] and np.abs(got[0][2]).max() > 0.0
        assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])
    finally:
        p.close()


def solve_with_solution(p, f):
    """(iterations, history, solution) of fddh_problem_solve_timed with the flexible CG"""
    u, hist = np.zeros(p.n), np.zeros(4096)
    nh, its, sec = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    dp = lambda a: ctypes.c_void_p(a.ctypes.data)
    f = np.ascontiguousarray(f)
    lib.host().call("fddh_problem_solve_timed", p.h, 0, dp(f), dp(u), dp(hist), len(hist), ctypes.byref(nh), ctypes.byref(its), ctypes.byref(sec))
    return its.value, hist[: nh.value].copy(), u


@pytest.mark.parametrize("setting", [("sub_use_preconditioner", 1), ("sub_use_preconditioner", 2), ("preconditioner_precision", 32)])
def test_the_vector_passes_do_not_depend_on_the_inner_solve(setup, setting):
    p = problem(("box", (2, 2, 2), 7, 6))
    try:
        name, value = setting
        if name == "sub_use_preconditioner" and value == 1:
            p.amg_build()
        p.set_flag(name, value)
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 100))
        set_flags(p, {flag: 0 for flag in FLAGS})
        base, labels = five_steps(p, f)
        assert not (set(FLAGS.values()) & labels)
        set_flags(p, {flag: 1 for flag in FLAGS})
        got, labels = five_steps(p, f)
        assert NORM in labels and DIRECTION in labels, sorted(labels)
        same_bits(got, base, setting)
    finally:
        p.close()


def test_two_ranks_keep_their_bits_and_the_norm_fusion_stays_out(gpu):
    """two ranks of this process on 4x2x2 at degree 7: the norm has two parts and an exchange (no fusion), the solution
    update still rides in the direction pass"""

    def body(rank, world):
        p = H.Problem.box((4, 2, 2), (2, 1, 1), 7, 6, True)
        try:
            p.set_flag("sub_use_preconditioner", 0)
            for lvl in range(p.info["num_levels"]):
                p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
            _, f = p.make_rhs_from(S.seeded_uniform(p.n, 101 + rank))
            out = {}
            for value in (0, 1):
                set_flags(p, {flag: value for flag in FLAGS})
                p.pcg_begin(f)
                single = [p.pcg_steps(1) for _ in range(3)]
                u_single = p.pcg_solution()
                p.pcg_begin(f)
                (last, u_lazy), labels = S.profiled(lambda: (p.pcg_steps(3), p.pcg_solution()))
                out[value] = ({"history": np.array(single), "solution": u_single, "lazy_last": np.array([last]), "lazy_solution": u_lazy}, labels)
            return out
        finally:
            p.close()

    try:
        results = H.run_local_ranks(2, body)
    finally:
        H.init(0, use_torch_stream=True)
        H.comm_single()
    for rank, out in enumerate(results):
        (off, labels_off), (on, labels_on) = out[0], out[1]
        same_bits(on, off, rank)
        assert np.isfinite(on["solution"]).all() and on["history"][-1] < on["history"][0]
        assert not (set(FLAGS.values()) & labels_off), (rank, sorted(labels_off))
        assert NORM not in labels_on and DIRECTION in labels_on, (rank, sorted(labels_on))
