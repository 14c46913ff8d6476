"""The checks of the successive-right-hand-side projection (fddh_problem_solve_projected, host/projection.hpp) that do
not care which kernel library is underneath: the defining properties of the basis, a right-hand side in the span, a
slowly varying sequence through both outer solvers, the lifecycle, and two ranks of one process.

Used by tests/test_gpu_projection.py on the GPU (product libraries, the kernels of csrc/fdd_projection.hip) and, with the
CPU stand-in of the kernel C-ABI -- which lacks those entries, so the host layer composes the passes from the multi-vector
entries -- by tests/test_cpu_projection.py as `python tests/projection_checks.py <libfdd_host_cpu.so> <check>`.

Every check prints the figures it asserts on before it asserts.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

BOX = ((4, 4, 4), (1, 1, 1), 3, 2)
CAPACITY = 4
TIGHT, LOOSE = 1e-10, 1e-5  # the three solves that make the basis / the solve of their combination
SPAN_COEFFS = (0.7, -1.3, 0.4)


def api():
    import support as S
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import lib

    return S, H, lib


def new_box(E=BOX[0], P=BOX[1], N=BOX[2], red=BOX[3]):
    S, H, _ = api()
    p = H.Problem.box(E, P, N, red, True)
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
    p.set_flag("sub_use_preconditioner", 0)
    return p


def true_residual(p, f, u):
    """|f - A u| / |f| with the operator and the norm of the public interface"""
    return p.residual_norm(f - p.stiffness(u)) / p.residual_norm(f)


def basis_of(p):
    return [p.projection_basis(k) for k in range(p.projection_info()["size"])]


def span_setup(p, seeds=(11, 22, 33), field=None, tolerance=TIGHT):
    """three independent right-hand sides solved at TIGHT (or tighter) into an empty basis of CAPACITY; returns them"""
    S, _, _ = api()
    p.projection(CAPACITY)
    p.set_options(tolerance=tolerance)
    fs = []
    for s in seeds:
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, s) if field is None else field(s))
        u, its, hist, proj = p.solve_projected(f, "fcg")
        res = true_residual(p, f, u)
        print("span_setup: seed %d its %d proj %s residual %.3e" % (s, its, proj.tolist(), res))
        assert its >= 1 and res <= TIGHT
        fs.append(f)
    assert p.projection_info()["size"] == len(seeds)
    return fs


def check_basis_properties(p, fs=None):
    """A X_k is what the operator gives for X_k, and X^T A X = I.  Returns (drift, gram deviation)."""
    if fs is None:
        fs = span_setup(p)
    basis = basis_of(p)
    assert len(basis) == 3
    drift = 0.0
    for k, (x, ax) in enumerate(basis):
        d = np.abs(p.stiffness(x) - ax).max() / np.abs(ax).max()
        print("basis_properties: row %d |A X_k - AX_k|_inf / |AX_k|_inf = %.3e" % (k, d))
        drift = max(drift, d)
    gram = np.array([[float(np.dot(xj, axk)) for (_, axk) in basis] for (xj, _) in basis])
    dev = np.abs(gram - np.eye(len(basis))).max()
    print("basis_properties: max |X^T AX - I| = %.3e" % dev)
    assert drift <= 1e-12, drift
    assert dev <= 1e-10, dev
    return drift, dev


def check_in_span(p, fs=None, exact=False):
    """f in the span of the three solved right-hand sides: no iteration at LOOSE, while the plain solve iterates.
    exact: also the residual an exact float64 projection in numpy leaves, against the bar (the CPU check of the margin)."""
    if fs is None:
        fs = span_setup(p)
    f = sum(c * fj for c, fj in zip(SPAN_COEFFS, fs))
    ratio = None
    if exact:
        basis = basis_of(p)
        alpha = [float(np.dot(x, f)) for (x, _) in basis]
        r = f - sum(a * ax for a, (_, ax) in zip(alpha, basis))
        ratio = p.residual_norm(r) / p.residual_norm(f)
        print("in_span: exact projection leaves |f - AX X^T f| / |f| = %.3e, bar / that = %.3e" % (ratio, LOOSE / ratio))
        assert ratio * 100.0 <= LOOSE, ratio
    p.set_options(tolerance=LOOSE)
    before = p.projection_info()
    u, its, hist, proj = p.solve_projected(f, "fcg")
    res = true_residual(p, f, u)
    print("in_span: its %d proj %s residual %.3e history %s" % (its, proj.tolist(), res, hist.tolist()))
    assert its == 0 and len(hist) == 1 and hist[0] == proj[1]
    assert proj[1] <= LOOSE * proj[0]
    assert res <= LOOSE
    assert p.projection_info() == before and proj[2] == proj[3] == before["size"]  # a zero-iteration solve stores nothing
    _, its_plain, _ = p.solve(f, "fcg")
    print("in_span: plain solve its %d" % its_plain)
    assert its_plain >= 1
    return its, proj, ratio


def smooth_field(p, seed):
    """a seeded mix of the four lowest Dirichlet modes of the unit box, sin(a pi x) sin(b pi y) sin(c pi z), a + b + c <= 4"""
    x, y, z = (p.mesh_array(c) for c in "xyz")
    w = np.random.default_rng(seed).uniform(0.5, 1.0, 4)
    modes = ((1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2))
    return sum(wk * np.sin(a * np.pi * x) * np.sin(b * np.pi * y) * np.sin(c * np.pi * z) for wk, (a, b, c) in zip(w, modes))


def sequence_fields(p, T=8):
    """u*_t = cos(0.2 t) phi_0 + sin(0.2 t) phi_1 + 0.05 t phi_2 + 1e-3 psi_t: phi fixed seeded smooth fields (what a time
    stepper's solutions are), psi_t a fresh seeded rough part.

    Why smooth: the check below holds two solutions of the same f, each with |r| <= tol |f|, to 10 tol |u|_inf of each
    other.  Their difference is A^-1 (r_1 - r_2); for u* in the span of modes with eigenvalues in [l, L] and a residual in
    the lowest of them that is at most 2 tol |f| / l <= 2 (L / l) tol |u|.  The four modes used have L / l = 6 / 3 = 2: a
    bound of 4 tol, 2.5 times inside the bar, which the rough part (1e-3 of the amplitude) does not use up.  For rough
    fields L / l is the condition number of the operator and no solver could promise the bar."""
    S, _, _ = api()
    phi = [smooth_field(p, 100 + i) for i in range(3)]
    return [np.cos(0.2 * t) * phi[0] + np.sin(0.2 * t) * phi[1] + 0.05 * t * phi[2] + 1e-3 * S.seeded_uniform(p.n, 1000 + t) for t in range(T)]


def check_sequence(p, method, vcycle, tolerance=1e-7):
    """eight slowly varying right-hand sides through solve_projected at CAPACITY against the plain solve of each"""
    if vcycle:
        p.amg_build()
    p.set_flag("sub_use_preconditioner", 1 if vcycle else 0)
    p.set_options(tolerance=tolerance)
    p.projection(CAPACITY)
    total, total_plain = 0, 0
    for t, u_star in enumerate(sequence_fields(p)):
        _, f = p.make_rhs_from(u_star)
        u, its, hist, proj = p.solve_projected(f, method)
        up, its_plain, _ = p.solve(f, method)
        info = p.projection_info()
        res = true_residual(p, f, u)
        diff = np.abs(u - up).max() / np.abs(up).max()
        print("sequence %s vcycle %d t %d: its %d plain %d proj %s residual %.3e |u - u_plain|/|u| %.3e info %s" % (method, vcycle, t, its, its_plain, proj.tolist(), res, diff, info))
        assert res <= tolerance, (t, res)
        assert diff <= 10 * tolerance, (t, diff)
        assert info["size"] <= CAPACITY and proj[3] == info["size"]
        total += its
        total_plain += its_plain
    print("sequence %s vcycle %d: %d iterations projected, %d plain, restarts %d" % (method, vcycle, total, total_plain, info["restarts"]))
    assert info["restarts"] >= 1
    assert total < total_plain, (total, total_plain)
    p.set_flag("sub_use_preconditioner", 0)
    return total, total_plain


def check_lifecycle(p):
    S, _, lib = api()
    p.set_options(tolerance=1e-7)
    _, f = p.make_rhs_from(S.seeded_uniform(p.n, 7))
    _, g = p.make_rhs_from(S.seeded_uniform(p.n, 8))
    # off: the plain solve, bit for bit
    p.projection(0)
    u, its, hist = p.solve(f, "fcg")
    up, itsp, histp, proj = p.solve_projected(f, "fcg")
    assert itsp == its and np.array_equal(up, u) and np.array_equal(histp, hist) and proj[2] == proj[3] == 0
    assert p.projection_info() == {"capacity": 0, "size": 0, "restarts": 0}
    # refused capacities leave the state alone
    p.projection(CAPACITY)
    p.solve_projected(f, "fcg")
    state = p.projection_info()
    assert state == {"capacity": CAPACITY, "size": 1, "restarts": 0}
    x_before = p.projection_basis(0)[0]
    for bad in (17, -1):
        try:
            p.projection(bad)
        except lib.FddError as e:
            assert "capacity" in str(e), e
        else:
            raise AssertionError("capacity %d was accepted" % bad)
        assert p.projection_info() == state and np.array_equal(p.projection_basis(0)[0], x_before)
    # f = 0: u = 0, nothing stored
    u0, its0, hist0, proj0 = p.solve_projected(np.zeros(p.n), "fcg")
    assert its0 == 0 and not u0.any() and proj0[0] == 0.0 and p.projection_info() == state
    # the same f again: its solution is in the basis, no iteration, nothing stored
    u2, its2, _, proj2 = p.solve_projected(f, "fcg")
    assert its2 == 0 and p.projection_info() == state and true_residual(p, f, u2) <= 1e-7
    # clear empties the basis
    p.projection_clear()
    assert p.projection_info() == {"capacity": CAPACITY, "size": 0, "restarts": 0}
    try:
        p.projection_basis(0)
    except lib.FddError:
        pass
    else:
        raise AssertionError("row 0 of an empty basis was handed out")
    # set_D_hat on a live basis empties it; solver options and other flags do not
    p.solve_projected(f, "fcg")
    p.solve_projected(g, "fcg")
    assert p.projection_info()["size"] == 2
    p.set_options(tolerance=1e-8, num_vectors=10)
    p.set_flag("fused_dssum", 0)
    p.set_flag("fused_dssum", 1)
    assert p.projection_info()["size"] == 2
    p.set_D_hat(0, S.gll(p.level_degree(0))[2])
    assert p.projection_info()["size"] == 0
    p.solve_projected(f, "fcg")
    p.set_flag("affine_geometry", 1)
    assert p.projection_info()["size"] == 0
    p.set_flag("affine_geometry", 0)
    # configure(0) frees the slabs and a later solve is the plain one again
    p.projection(0)
    up, itsp, histp, _ = p.solve_projected(f, "fcg")
    u, its, hist = p.solve(f, "fcg")
    assert itsp == its and np.array_equal(up, u) and np.array_equal(histp, hist)
    # without a Subdomain: the same wrapper on the unpreconditioned solvers
    p.set_options(use_preconditioner=0, tolerance=1e-7)
    p.projection(2)
    for method in ("fcg", "gmres"):
        p.projection_clear()
        ua, itsa, _, _ = p.solve_projected(f, method)
        ub, itsb, _, projb = p.solve_projected(f, method)
        print("lifecycle: no preconditioner %s its %d then %d" % (method, itsa, itsb))
        assert itsa >= 1 and itsb == 0 and true_residual(p, f, ub) <= 1e-7
    p.set_options(use_preconditioner=1)
    p.projection(0)


def nodal_field(p, seed):
    """a seeded value per GLOBAL node, so that every rank (and the one-rank problem) sees the same function"""
    glo = p.mesh_array("glo_num")
    table = np.random.default_rng(seed).uniform(0.0, 1.0, 200_003)
    return table[glo % len(table)]


def check_two_ranks(solve_tolerance=TIGHT / 100.0):
    """(8,4,4) over (2,1,1) at N = 3 in one process: the span test's four solves on two ranks against one rank.

    The bar on the solutions is the span test's: 10 TIGHT |u|_inf for the three solves that make the basis, 10 LOOSE |u|_inf
    for their combination.  Solved AT TIGHT the three miss it, and not because of the projection: the first of them starts
    from an empty basis and is the plain solve, which one rank (one subdomain) and two ranks (the composite) end at different
    iterates of residual <= 1e-10 |f|; the two differ by A^-1 (r_1 - r_2), for these rough fields 2.0e-9, 2.4e-9 and
    2.9e-9 |u|_inf -- 20 to 29 tolerances, on the CPU build and on the MI355X alike.  As in the span test the remedy is to
    tighten the solves, not the bar: at TIGHT / 100 the same amplification leaves 0.3 of a tolerance."""
    _, H, _ = api()
    E, N, red = (8, 4, 4), 3, 2

    def run(P):
        def body(rank, size):
            p = new_box(E, P, N, red)
            fs = span_setup(p, field=lambda s: nodal_field(p, s), tolerance=solve_tolerance)
            its, proj, _ = check_in_span(p, fs)
            f = sum(c * fj for c, fj in zip(SPAN_COEFFS, fs))
            p.projection_clear()
            us = []
            for g, tol in zip(fs + [f], [solve_tolerance] * 3 + [LOOSE]):
                p.set_options(tolerance=tol)
                u, i, _, pr = p.solve_projected(g, "fcg")
                us.append((u, i, pr.tolist()))
            out = (p.mesh_array("glo_num"), us, its, proj.tolist())
            p.close()
            return out

        return H.run_local_ranks(P[0] * P[1] * P[2], body)

    one = run((1, 1, 1))[0]
    two = run((2, 1, 1))
    assert two[0][2] == two[1][2] == 0 and two[0][3] == two[1][3]  # in span: no iteration, the same figures on both ranks
    by_node = {}
    for k, (u, i, pr) in enumerate(one[1]):
        by_node[k] = dict(zip(one[0].tolist(), u.tolist()))
    tolerances = [TIGHT] * 3 + [LOOSE]  # of the four solves
    worst = []
    for k in range(len(one[1])):
        assert two[0][1][k][1:] == two[1][1][k][1:], (k, two[0][1][k][1:], two[1][1][k][1:])  # iterations and proj identical
        scale = np.abs(one[1][k][0]).max()
        diff = 0.0
        for glo, us, _, _ in two:
            ref = np.array([by_node[k][g] for g in glo.tolist()])
            diff = max(diff, np.abs(us[k][0] - ref).max() / scale)
        print("two_ranks: solve %d its %d (one rank %d) basis %d -> %d |u - u_one|_inf / |u|_inf = %.3e = %.2f x its tolerance" % (k, two[0][1][k][1], one[1][k][1], two[0][1][k][2][2], two[0][1][k][2][3], diff, diff / tolerances[k]))
        worst.append(diff / tolerances[k])
    assert two[0][1][3][1] == 0  # the combination again, after the three: no iteration
    assert max(worst) <= 10.0, worst
    return True


def run_basis_and_span(exact=False):
    p = new_box()
    try:
        fs = span_setup(p)
        return check_basis_properties(p, fs), check_in_span(p, fs, exact=exact)
    finally:
        p.close()


def run_sequence(method):
    p = new_box()
    try:
        return check_sequence(p, method, 0), check_sequence(p, method, 1)
    finally:
        p.close()


def run_lifecycle():
    p = new_box()
    try:
        check_lifecycle(p)
    finally:
        p.close()


CHECKS = {
    "basis_and_span": lambda: run_basis_and_span(exact=True),
    "sequence_fcg": lambda: run_sequence("fcg"),
    "sequence_gmres": lambda: run_sequence("gmres"),
    "lifecycle": run_lifecycle,
    "two_ranks": check_two_ranks,
}


if __name__ == "__main__":
    _, H, lib = api()
    # test-only: serve include/fdd_host.h from the CPU build of the host layer (tests/cpu_shim)
    lib._host = lib._Lib(sys.argv[1], os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
    name = sys.argv[2]
    if name != "two_ranks":
        H.init(0, use_torch_stream=False)
        H.comm_single()
        H.set_print(False)
    if name == "fused_flag":
        p = new_box((2, 2, 2))
        p.set_flag("fused_projection", 0)
        try:
            p.set_flag("fused_projection", 1)
        except lib.FddError as e:
            print("refused:", e)
        else:
            raise SystemExit("the flag was accepted without the kernel entries")
        p.close()
    else:
        CHECKS[name]()
    print("ok")
