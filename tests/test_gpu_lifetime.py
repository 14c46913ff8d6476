"""Who owns the device memory of a problem, on the GPU (host/fdd_device.hpp: fdd::memory shares its block, a plan and a
captured graph have one owner each): a closed problem gives back every block, plan and graph it took,
and a rebuilt hierarchy replaces the one before it.

Counted with fdd_live_objects (include/fdd_hip.h) -- what the kernel library itself has handed out and not got back; the
card's free memory is other processes' too.  Every test reads its baseline first (earlier modules of the session may hold
problems of their own) and requires the figures to have RISEN before it requires them back, so a dead counter cannot pass.
The sanitized walk of the same owners on the CPU build is tests/test_cpu_lifetime.py.

Shapes: box (2,2,2) at N = 7, r = 2 is the smallest that reaches the line-kernel lists, factor_elem, the assembly classes
and the coefficient arrays.  The host layer runs on a stream of its own so that the V-cycle is captured (graphs)."""
import ctypes

import pytest

import reconfigure_walks as R
import support as S
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

pytestmark = pytest.mark.gpu

FIGURES = ("blocks", "bytes", "peak", "plans", "graphs", "mallocs")
HELD = ("blocks", "bytes", "plans", "graphs")


def live():
    out = (ctypes.c_longlong * len(FIGURES))()
    lib.hip().call("fdd_live_objects", out, len(FIGURES))
    return dict(zip(FIGURES, out))


def held(figures):
    return tuple(figures[k] for k in HELD)


def rose(now, before, *keys):
    return all(now[k] > before[k] for k in keys)


@pytest.fixture(scope="module")
def own_stream(gpu):
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    yield True
    H.init(0)  # back to torch's current stream for the other modules


def new_problem(N=7, **kw):
    p = H.Problem.box((2, 2, 2), (1, 1, 1), N, 2, True, **kw)
    p.set_options(max_iterations=3, preconditioner_type=1)
    return p


def test_default_build_host_and_device_hierarchy(own_stream):
    """default flags, amg_build on the host and then on the device, a solve, close(): back to the baseline, twice, with the
    same peak"""
    base = live()
    peaks = []
    for _ in range(2):
        lib.hip().call("fdd_live_objects_reset_peak")
        p = new_problem()
        created = live()
        assert rose(created, base, "blocks", "bytes", "plans", "mallocs"), (created, base)
        p.amg_build(device=False)
        on_host = live()
        assert rose(on_host, created, "blocks", "bytes", "plans"), (on_host, created)
        p.amg_build(device=True)
        assert p.amg_setup_info()["levels_built_on_device"] >= 1
        on_device = live()
        assert rose(on_device, on_host, "mallocs") and rose(on_device, created, "blocks", "plans"), (on_device, on_host)
        _, f = p.make_rhs()
        p.solve(f)
        solved = live()
        assert rose(solved, on_device, "blocks", "graphs"), (solved, on_device)
        p.close()
        after = live()
        assert held(after) == held(base), (after, base)
        peaks.append(after["peak"])
    assert peaks[0] == peaks[1] and peaks[0] > base["bytes"], peaks


def test_every_rebuild_replaces_the_hierarchy_before_it(own_stream):
    """the four ways a live problem builds its hierarchy again, three times each, a solve after every one"""
    base = live()
    p = new_problem(faces="DNNDND")
    try:
        p.amg_build(device=False)
        _, f = p.make_rhs()
        p.solve(f)
        built = live()
        assert rose(built, base, "blocks", "bytes", "plans", "graphs"), (built, base)
        kappas = [1.0 + S.seeded_uniform(p.n, 50 + k) for k in range(3)]
        ways = {
            "diffusivity": [lambda k=k: p.diffusivity(k) for k in kappas],
            "helmholtz": [lambda v=v: p.helmholtz(v) for v in (1.0, 2.0, 3.0)],
            "robin": [lambda v=v: p.robin({1: v}) for v in (1.0, 2.0, 3.0)],
            "amg_cheby_order": [lambda v=v: p.set_flag("amg_cheby_order", v) for v in (3, 2, 3)],
        }
        for name, calls in ways.items():
            first = None
            for call in calls:
                before = live()
                call()
                rebuilt = live()
                assert rose(rebuilt, before, "mallocs"), (name, rebuilt, before)
                p.solve(f)
                now = live()
                assert now["graphs"] > 0
                first = first or now
                assert held(now) == held(first), (name, now, first)
    finally:
        p.close()
    assert held(live()) == held(base), (live(), base)


def test_the_other_owners(own_stream):
    """float inner solve with the V-cycle (captured graphs), Chebyshev-Jacobi inner solve, a projection basis with two
    projected solves, the surface weights"""
    base = live()
    p = new_problem(faces="DNNDND")
    try:
        p.amg_build(device=False)
        _, f = p.make_rhs()
        _, g = p.make_rhs(seed=1)
        p.set_flag("preconditioner_precision", 32)
        p.solve(f)
        float_solve = live()
        assert rose(float_solve, base, "blocks", "bytes", "plans", "graphs"), (float_solve, base)
        p.set_flag("sub_use_preconditioner", 2)
        p.set_flag("inner_solver", 1)
        p.solve(f)
        p.set_flag("preconditioner_precision", 64)
        p.solve(f)
        chebyshev = live()
        assert rose(chebyshev, float_solve, "blocks", "bytes"), (chebyshev, float_solve)
        p.set_flag("inner_solver", 0)
        p.set_flag("sub_use_preconditioner", 1)
        p.projection(4)
        p.solve_projected(f)
        p.solve_projected(g)
        projected = live()
        assert rose(projected, chebyshev, "blocks", "bytes"), (projected, chebyshev)
        p.surface()
        assert rose(live(), projected, "blocks", "bytes")
    finally:
        p.close()
    assert held(live()) == held(base), (live(), base)


def test_a_forced_composite(own_stream):
    base = live()
    p = new_problem(force_composite=True)
    try:
        p.amg_build(device=False)
        _, f = p.make_rhs()
        p.solve(f)
        assert rose(live(), base, "blocks", "bytes", "plans", "graphs")
    finally:
        p.close()
    assert held(live()) == held(base), (live(), base)


def test_two_ranks(own_stream):
    """box (4,2,2) as two blocks of (2,2,2) at N = 3: composites with rings and exchange buffers, closed and finalized"""
    base = live()

    def body(rank, size):
        p = H.Problem.box((4, 2, 2), (2, 1, 1), 3, 2, True)
        try:
            p.set_options(max_iterations=3)
            p.amg_build(device=False)
            _, f = p.make_rhs()
            p.solve(f)
            return live()
        finally:
            p.close()

    for during in H.run_local_ranks(2, body):
        assert rose(during, base, "blocks", "bytes", "plans"), (during, base)
    assert held(live()) == held(base), (live(), base)


@pytest.mark.parametrize("walk", [n for n in R.walk_names(cpu=False) if R.WALKS[n]["family"] == "operator"])
def test_a_reconfigure_walk_closes_what_it_opened(own_stream, walk):
    """the walks of the family "operator" through their own driver, which closes every problem it builds; the walk's
    assertions are its own"""
    lib.hip().call("fdd_live_objects_reset_peak")
    base = live()
    R.run_walk(R.Driver(H, S, lib), walk)
    after = live()
    assert rose(after, base, "mallocs") and after["peak"] > base["bytes"], (after, base)
    assert held(after) == held(base), (after, base)
