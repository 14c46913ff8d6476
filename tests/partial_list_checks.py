"""Problems on meshes where only some elements meet a condition the host layer establishes per element list
(tests/partial_meshes.py): the cases, and the checks that do not care which kernel library is underneath.

  written_bits     every level's factor arrays and coordinates come back from the problem with the bits that were written
  operator         p.stiffness(u) against diffusivity_checks.local_stiffness on the written arrays, 1e-12 max|ref|;
                   sub_dof_operator and sub_jacobi_diagonal against diffusivity_checks.assemble on them, 1e-12; and the
                   same restatement under the WRONG verdict -- the offending elements' g_4..g_6 zeroed, or a graded element
                   given its representative's block -- must differ from the reference by at least 1e-3 max|ref|, so that
                   the 1e-12 tells a kernel that skipped arrays it needed from one that read them
  oracle_solve     a full outer FCG solve with the preconditioner on against the CPU oracle on the problem's own arrays:
                   equal iteration counts, histories to 1e-8 r0, solution to 1e-9 (meshes whose factors belong to their
                   coordinates only)
  nothing_switches the answers of a kernel library without the three-array and line entries
  affine_answers   with "affine_geometry" asked for, exactly the lists within AFFINE_TOLERANCE of the affine form switch; where
                   one does, operator also holds the inner operator on the affine kernel to the matrix (1e-12) and two PCG
                   steps to the streamed ones (1e-12)
  two_ranks        the composite of two ranks in which the offending element is a ring element pulled from the other rank

Used by tests/test_gpu_partial_lists.py on the GPU and, with the CPU stand-in of the kernel C-ABI, by
tests/test_cpu_partial_lists.py as `python tests/partial_list_checks.py <libfdd_host_cpu.so> <check>`.  Every check prints the
figures it asserts on first.
"""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import diffusivity_checks as DC  # noqa: E402
import partial_meshes as M  # noqa: E402
import support as S  # noqa: E402

BOX = (3, 3, 3)
LAST = 26


def _box_at_fine_degree_only(N, edit):
    return lambda deg: edit(S.BoxMesh(BOX, deg)) if deg == N else S.BoxMesh(BOX, deg)


# name -> mesh(degree), N, reduction; offenders(mesh): the elements whose arrays a wrong verdict would misread; wrong:
# "offdiag" (their g_4..g_6 taken for zero) or "representative" (their g_1..g_3 blocks taken for the lowest element's), None:
# the case is held by the verdicts and the flag comparison alone; oracle: the factors belong to the coordinates
CASES = {}
for _e in (0, 79, 41):  # 80 elements of 64 points: the detection pass has more than one workgroup; first, last, in the middle
    CASES["bumped_544_N3_e%d" % _e] = dict(mesh=lambda deg, e=_e: M.bumped((5, 4, 4), deg, [e]), N=3, red=2, wrong="offdiag", oracle=True)
for _name, _elems in (("e26", [26]), ("e0_e26", [0, 26])):
    for _red in (6, 2):  # levels 7, 1 and 7, 5, 3, 1: only the last list qualifies
        CASES["bumped_333_N7_%s_r%d" % (_name, _red)] = dict(mesh=lambda deg, el=_elems: M.bumped(BOX, deg, el), N=7, red=_red, wrong="offdiag", oracle=True)
CASES["bumped_222_N11_e7"] = dict(mesh=lambda deg: M.bumped((2, 2, 2), deg, [7]), N=11, red=5, wrong="offdiag", oracle=True)
CASES["graded_333_N7_e26"] = dict(mesh=lambda deg: M.graded(BOX, deg, [LAST]), N=7, red=6, wrong="representative", oracle=False)
CASES["graded_333_N7_e13_to_26"] = dict(mesh=lambda deg: M.graded(BOX, deg, range(13, 27)), N=7, red=6, wrong="representative", oracle=False)
for _N in (3, 7, 11):
    CASES["sheared_322_N%d" % _N] = dict(mesh=lambda deg: M.sheared((3, 2, 2), deg), N=_N, red=_N - 1, wrong="offdiag", oracle=False)
CASES["bumped_sheared_322_N7_e11"] = dict(mesh=lambda deg: M.bumped((3, 2, 2), deg, [11], base="sheared"), N=7, red=6, wrong="offdiag", oracle=False)
CASES["edited_333_N7_denormal"] = dict(mesh=_box_at_fine_degree_only(7, lambda m: M.edited(m, "g_6", LAST, -1, 5e-324)), N=7, red=6, wrong=None, oracle=False)
CASES["edited_333_N7_minus_zero"] = dict(mesh=_box_at_fine_degree_only(7, lambda m: M.edited(m, "g_6", LAST, -1, -0.0)), N=7, red=6, wrong=None, oracle=False)


def offenders(mesh, wrong):
    n3 = mesh.num_elem_points
    if wrong == "offdiag":
        return [e for e in range(mesh.num_local_elements) if not M.offdiag_zero(mesh, [e])]
    lowest = [a.reshape(-1, n3)[0] for a in mesh.g[:3]]
    return [e for e in range(mesh.num_local_elements) if any(not np.array_equal(a.reshape(-1, n3)[e], b) for a, b in zip(mesh.g[:3], lowest))]


def wrong_factors(mesh, wrong):
    """the arrays a kernel would in effect read under the wrong verdict"""
    n3 = mesh.num_elem_points
    G = [a.copy() for a in mesh.g]
    for e in offenders(mesh, wrong):
        at = slice(e * n3, (e + 1) * n3)
        for f in ((3, 4, 5) if wrong == "offdiag" else (0, 1, 2)):
            G[f][at] = 0.0 if wrong == "offdiag" else G[f][:n3]
    return G


def level_meshes(case):
    spec = CASES[case]
    return {deg: spec["mesh"](deg) for deg in S.level_degrees(spec["N"], spec["red"])}


def open_problem(H, case, directory, meshes=None):
    """the case's meshes written once per level degree and read back by the host layer"""
    spec = CASES[case]
    meshes = meshes or level_meshes(case)
    for mesh in meshes.values():
        S.write_mesh_files(directory, mesh)
    p = H.Problem.from_directory(directory, spec["N"], spec["red"])
    p.set_flag("sub_use_preconditioner", 0)  # the inner solves without the V-cycle, as the oracle side runs them
    for lvl in range(p.info["num_levels"]):
        p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
    return p, meshes


def written_bits(p, meshes):
    for lvl in range(p.info["num_levels"]):
        mesh = meshes[p.level_degree(lvl)]
        for name, want in [("x", mesh.x), ("y", mesh.y), ("z", mesh.z)] + [("g_%d" % (f + 1), mesh.g[f]) for f in range(6)]:
            assert np.array_equal(DC.bits(p.mesh_array(name, lvl)), DC.bits(want)), (lvl, name)


def operator(p, mesh, wrong, label, affine=False):
    N = mesh.N
    n, D = N + 1, np.asarray(S.gll(N)[2], np.float64).reshape(N + 1, N + 1)
    u = DC.rnd(p.n, 1)
    ref = DC.local_stiffness(u, mesh.g, D, n)
    err = np.abs(p.stiffness(u) - ref).max() / np.abs(ref).max()
    pd, nd = p.sub_point_dofs().astype(np.int64), p.sub_info()["unique_dofs"]
    K = DC.assemble(mesh.g, D, n, pd, nd)
    xa = DC.rnd(nd, 4)
    want, dwant = K @ xa, K.diagonal()
    e_op = np.abs(p.sub_dof_operator(xa) - want).max() / np.abs(want).max()
    e_diag = (np.abs(p.sub_jacobi_diagonal() - dwant) / dwant).max()
    print("%s: |Au - ref| / max|ref| = %.3e, inner operator %.3e, its diagonal %.3e (%d dofs)" % (label, err, e_op, e_diag, nd))
    assert err <= 1e-12 and e_op <= 1e-12 and e_diag <= 1e-12, (err, e_op, e_diag)
    if affine:
        # the list switches to the affine kernel: the inner operator against the same matrix, and the fine Domain's
        # gather form through two PCG steps against the streamed ones (the bars of test_gpu_host.test_affine_geometry_option)
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 7))
        p.pcg_begin(f)
        r_streamed, u_streamed = p.pcg_steps(2), p.pcg_solution()
        p.set_flag("affine_geometry", 1)
        try:
            assert p.affine_info()["fine_domain"] and p.affine_info()["sub_lists_affine"] == 1
            e_aff = np.abs(p.sub_dof_operator(xa) - want).max() / np.abs(want).max()
            p.pcg_begin(f)
            r_affine, u_affine = p.pcg_steps(2), p.pcg_solution()
        finally:
            p.set_flag("affine_geometry", 0)
        d_r, d_u = abs(r_affine - r_streamed) / r_streamed, np.abs(u_affine - u_streamed).max() / np.abs(u_streamed).max()
        print("%s: on the affine kernel the inner operator %.3e; two PCG steps against the streamed ones: residual %.3e, iterate %.3e" % (label, e_aff, d_r, d_u))
        assert e_aff <= 1e-12 and d_r <= 1e-12 and d_u <= 1e-12, (e_aff, d_r, d_u)
    if wrong is None:
        return
    Gw = wrong_factors(mesh, wrong)
    bite = np.abs(DC.local_stiffness(u, Gw, D, n) - ref).max() / np.abs(ref).max()
    bite_op = np.abs(DC.assemble(Gw, D, n, pd, nd) @ xa - want).max() / np.abs(want).max()
    print("%s: under the wrong verdict (%s, elements %s) the restatement is off by %.3e max|ref|, the inner operator by %.3e" % (label, wrong, offenders(mesh, wrong), bite, bite_op))
    assert bite >= 1e-3 and bite_op >= 1e-3, (bite, bite_op)


def oracle_solve(p, N, red, label):
    W = S.OracleWorld([S.ArrayMesh.from_problem(p)], N)
    sd = S.OracleSubdomain(None, N, red, meshes=[S.ArrayMesh.from_problem(p, lvl) for lvl in range(p.info["num_levels"])])
    try:
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 1234))
        u, its, hist = p.solve(f, "fcg")

        def pre(zz, rr):
            out, _, _ = sd.solve(rr[0], "gmres")
            zz[0][:] = out

        ou, oits, ohist = W.solve([f], "fcg", precond=pre)
        d_hist = np.abs(hist[: len(ohist)] - ohist[: len(hist)]).max() / ohist[0]
        d_u = np.abs(u - ou[0]).max() / np.abs(ou[0]).max()
        print("%s: outer FCG %d iterations, the oracle %d; histories differ by %.3e r0, solutions by %.3e" % (label, its, oits, d_hist, d_u))
        assert its == oits and len(hist) == len(ohist), (its, oits)
        assert d_hist <= 1e-8 and d_u <= 1e-9, (d_hist, d_u)
    finally:
        W.close()
        sd.close()


def nothing_switches(p):
    """a kernel library without the optional stiffness entries: no flag is on, no list on a three-array or line kernel"""
    for answer in (p.zero_factor_info(), p.mfma_zero_factor_info(), p.line_stiffness_info(), p.shared_factor_info(), p.lean_line_info()):
        on = {k: v for k, v in answer.items() if k not in ("sub_lists", "fine_domain_table_ok", "fine_domain_classes")}
        assert not any(on.values()) and answer["sub_lists"] == 1, answer


def affine_answers(p, meshes, N):
    """with "affine_geometry" asked for: exactly the lists whose restated deviation is within AFFINE_TOLERANCE switch, and the
    deviation reported is the restated one of the fine level (the Domain's list and the Subdomain's are the same elements)"""
    dev = M.affine_deviation(meshes[N])
    want = dev <= M.AFFINE_TOLERANCE
    p.set_flag("affine_geometry", 1)
    info = p.affine_info()
    p.set_flag("affine_geometry", 0)
    print("affine: restated deviation %.3e, reported %.3e, switched %s" % (dev, info["max_deviation"], info["fine_domain"]))
    assert (info["fine_domain"], info["sub_lists_affine"], info["sub_lists"]) == (want, int(want), 1), (info, dev)
    if want:
        assert 0.0 <= info["max_deviation"] <= M.AFFINE_TOLERANCE, info
    else:
        assert abs(info["max_deviation"] - dev) <= 1e-9 * dev and dev > 1e-6, (info, dev)
    off = p.affine_info()
    assert not off["fine_domain"] and off["sub_lists_affine"] == 0, off
    return want


# ---------------------------------------------------------------- two ranks: the offender is a ring element of the other rank
TWO_RANKS = dict(E=(8, 2, 2), N=5, red=2, P=(2, 1, 1), bumped=[4])  # global element (4, 0, 0): rank 1's first, on the rank interface
INFO_KEYS = (("zero_factor_info", "diag", "skip_zero_factors", "sub_lists_diag"), ("mfma_zero_factor_info", "mfma_diag", "mfma_skip_zero_factors", "sub_lists_mfma_diag"),
             ("line_stiffness_info", "lines", "line_stiffness", "sub_lists_lines"), ("shared_factor_info", "shared", "shared_factor_blocks", "sub_lists_shared"),
             ("lean_line_info", "lean", "lean_line_stiffness", "sub_lists_lean"))


def two_ranks(H, rank, world, mesh_dir, barrier, product=True):
    """One of two ranks of the composite on bumped((8,2,2), 5, [4]), reduction 2, overlaps (1, 1): the bumped element is rank
    1's own (its degree-5 lists do not qualify) and a ring element of rank 0, where the first ring keeps degree 5 -- rank 0's
    Domain lists all qualify, and of its Subdomain's three lists exactly the degree-5 one (own elements and first ring),
    disqualified by an element pulled from its peer, runs six arrays: another verdict than the Domain's list of that degree.
    The expected counts come from p.sub_region() and the restated verdicts on the written arrays; region,
    operators (1e-12) and outer solves (equal counts, histories to 1e-8 r0) are held to the oracle's two-rank world.
    product: the kernel library has the optional stiffness entries (the CPU stand-in has none)."""
    import stiffness_choice_rules as R

    E, N, red, Pg, bump = (TWO_RANKS[k] for k in ("E", "N", "red", "P", "bumped"))
    degs = S.level_degrees(N, red)
    cache = {}

    def mesh_of(deg, r):
        if (deg, r) not in cache:
            cache[(deg, r)] = M.bumped(E, deg, bump, Pg, r)
        return cache[(deg, r)]

    assert mesh_of(N, 1).bumped_elements == [0] and mesh_of(N, 0).bumped_elements == [] and mesh_of(1, 1).bumped_elements == []
    for deg in degs:
        S.write_mesh_files(mesh_dir, mesh_of(deg, rank), proc_id=rank)
    barrier()
    p = H.Problem.from_directory(mesh_dir, N, red, 1, 1, with_subdomain=True)
    try:
        p.set_flag("sub_use_preconditioner", 0)
        for lvl in range(p.info["num_levels"]):
            p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
            assert all(np.array_equal(DC.bits(p.mesh_array("g_%d" % (f + 1), lvl)), DC.bits(mesh_of(degs[lvl], rank).g[f])) for f in range(6))
        meshes = [mesh_of(N, r) for r in range(world)]
        W = S.OracleWorld(meshes, N)
        F = S.OracleFdd(E, N, red, Pg, meshes=[[mesh_of(d, r) for d in degs] for r in range(world)])
        si, oi = p.sub_info(), F.info[rank]
        assert si["is_composite"] == 1 and si["num_values"] == oi["num_values"] and si["unique_dofs"] == oi["unique_dofs"]
        ids, lv = p.sub_region()
        assert np.array_equal(ids, F.region(rank)[0]) and np.array_equal(lv, F.region(rank)[1])

        # the lists of the region, from the written arrays: elements are numbered rank after rank
        per_rank = meshes[0].num_local_elements
        region_levels = sorted(set(lv.tolist()))
        assert region_levels == [0, 1, 2]
        parts = {l: [(mesh_of(degs[l], int(e) // per_rank), int(e) % per_rank) for e in ids[lv == l]] for l in region_levels}
        lists = [M.list_state(M.collected(parts[l])) for l in region_levels]
        bumped_global = per_rank  # rank 1's local element 0
        holds_it = [l for l in region_levels if bumped_global in ids[lv == l].tolist()]
        # with overlap 1 the first ring keeps degree N: rank 0's level-0 list is its own elements and that ring, so the
        # Subdomain's list of degree 5 fails where the Domain's list of the same degree holds
        assert holds_it == [0] and (bumped_global // per_rank != rank) == (rank == 0), (rank, holds_it)
        assert [st[3] for st in lists] == [l not in holds_it for l in region_levels], lists  # exactly the list that holds it fails
        own = M.list_state(mesh_of(N, rank))
        assert own[3] == (rank == 0)
        flags = {name: product or name == "mfma_stiffness" for name in R.FLAGS}
        for precision in (64, 32):
            p.set_flag("preconditioner_precision", precision)
            want = R.composite_info(lists, flags, precision == 32)
            for entry, kind, flag, key in INFO_KEYS:
                answer = getattr(p, entry)()
                assert (answer["enabled"], answer["fine_domain"], answer[key], answer["sub_lists"]) == (flags[flag], R.info(own, flags, False)[kind], want[kind], 3), (rank, precision, flag, answer, want)
            if product:  # two of the three lists stream three arrays, the one with the bumped element six
                assert want["diag"] == 2 and p.zero_factor_info()["fine_domain"] == (rank == 0)
        p.set_flag("preconditioner_precision", 64)
        print("rank %d: levels of the region's lists %s, off-diagonal arrays zero %s, the bumped element in list %s" % (rank, region_levels, [st[3] for st in lists], holds_it))

        us = [np.sin(3 * mm.x + 1) * np.cos(2 * mm.y) + mm.z * mm.x for mm in meshes]
        v = np.random.default_rng(5 + rank).standard_normal(si["num_values"])
        for op in ("stiffness", "dssum"):
            ref = getattr(F, op)(rank, v)
            err = np.abs(p.sub_op(op, v) - ref).max() / np.abs(ref).max()
            print("rank %d: sub_op %s against the oracle %.3e" % (rank, op, err))
            assert err <= 1e-12, op
        ref = F.tree(us)[rank]
        err = np.abs(p.sub_op("tree", us[rank]) - ref).max() / np.abs(ref).max()
        print("rank %d: sub_op tree against the oracle %.3e" % (rank, err))
        assert err <= 1e-12
        o_f = W.stiffness(W.dssum(us, True, True))
        _, f = p.make_rhs_from(us[rank])
        assert np.abs(f - o_f[rank]).max() <= 1e-13 * np.abs(o_f[rank]).max()

        def pre(z, r):
            out, _ = F.precondition(r, "gmres")
            for k in range(world):
                z[k][:] = out[k]

        for method in ("fcg", "gmres"):
            u, its, hist = p.solve(f, method)
            ou, oits, ohist = W.solve(o_f, method, precond=pre)
            d_hist = np.abs(hist[: len(ohist)] - ohist[: len(hist)]).max() / ohist[0]
            print("rank %d: outer %s %d iterations, the oracle %d; histories differ by %.3e r0, solutions by %.3e" % (rank, method, its, oits, d_hist, np.abs(u - ou[rank]).max() / np.abs(ou[rank]).max()))
            assert its == oits, (method, its, oits)
            assert d_hist <= 1e-8, (method, d_hist)
        W.close()
        F.close()
    finally:
        p.close()


# ---------------------------------------------------------------- the builders against figures worked out beforehand
def check_builders():
    """one bumped element in the (3,3,3) box, the sheared box in its analytic and isoparametric forms, the graded lists"""
    for N in (1, 2, 3, 5, 7, 11):
        m, box = M.bumped(BOX, N, [13]), S.BoxMesh(BOX, N)
        n3 = (N + 1) ** 3
        blocks = lambda mesh, f: np.asarray(mesh.g[f]).reshape(27, n3)
        same = [e for e in range(27) if all(np.array_equal(DC.bits(blocks(m, f)[e]), DC.bits(blocks(box, f)[e])) for f in range(6))]
        moved = [e for e in range(27) if not np.array_equal(DC.bits(m.x.reshape(27, n3)[e]), DC.bits(box.x.reshape(27, n3)[e]))]
        if N == 1:  # no interior point: the box itself, which qualifies
            assert len(same) == 27 and moved == [] and M.offdiag_zero(m) and M.shared(m) and M.factor_classes(m) == 1
            continue
        off = max(np.abs(blocks(m, f)[13]).max() for f in (3, 4, 5)) / np.abs(m.g[0]).max()
        dev = M.affine_deviation(m, per_element=True)
        print("bumped (3,3,3) N = %d: max|g_4..6| / max|g_1| = %.3f in element 13, deviation from the affine form %.3f there and at most %.2e elsewhere, %d classes" % (N, off, dev[13], np.delete(dev, 13).max(), M.factor_classes(m)))
        assert same == [e for e in range(27) if e != 13] and moved == [13]
        assert [e for e in range(27) if not M.offdiag_zero(m, [e])] == [13] and not M.offdiag_zero(m) and M.offdiag_zero(m, same)
        assert 0.03 <= off <= 0.16 and 0.05 <= dev[13] <= 0.35 and np.delete(dev, 13).max() <= 5.2e-16
        # two blocks for 27 elements: a missed off-diagonal verdict would also make the list shared
        assert M.factor_classes(m) == 2 and 2 * 2 <= 27 and not M.shared(m)
        # the faces of the bumped element stay where they are, bit for bit
        n = N + 1
        face = np.zeros((n, n, n), bool)
        face[[0, -1]] = face[:, [0, -1]] = face[:, :, [0, -1]] = True
        for c in "xyz":
            assert np.array_equal(DC.bits(getattr(m, c).reshape(27, n3)[13][face.reshape(-1)]), DC.bits(getattr(box, c).reshape(27, n3)[13][face.reshape(-1)]))
    for N in (2, 3, 7, 11):
        m = M.sheared((3, 2, 2), N)
        iso = M._own(m)
        S.DeformedMesh._isoparametric(iso, [m.x, m.y, m.z])
        ratio = abs(m.shear_constants[3]) / abs(m.shear_constants[0])
        d_analytic, d_iso = M.affine_deviation(m), M.affine_deviation(iso)
        print("sheared (3,2,2) N = %d: |c_4| / |c_1| = %.3f, deviation %.2e in the analytic form, %.2e isoparametric (bar %.2e); the two forms differ by %.1e max|g|"
              % (N, ratio, d_analytic, d_iso, M.AFFINE_TOLERANCE, max(np.abs(a - b).max() for a, b in zip(m.g, iso.g)) / np.abs(m.g[0]).max()))
        assert abs(ratio - 0.17) < 0.005 and d_analytic <= M.AFFINE_TOLERANCE and not M.offdiag_zero(m) and all(c != 0.0 for c in m.shear_constants)
        assert (d_iso <= M.AFFINE_TOLERANCE) == (N <= 2)  # what the option asks of an isoparametric sheared mesh: degree <= 2
        assert max(np.abs(a - b).max() for a, b in zip(m.g, iso.g)) <= 1e-13 * np.abs(m.g[0]).max()  # the analytic factors are the geometry's
    m = M.bumped((3, 2, 2), 7, [11], base="sheared")
    dev = M.affine_deviation(m, per_element=True)
    assert dev[:11].max() <= M.AFFINE_TOLERANCE and dev[11] > 0.05 and not M.offdiag_zero(m, [0])
    one, many = M.graded(BOX, 7, [LAST]), M.graded(BOX, 7, range(13, 27))
    print("graded: %d and %d classes, deviations %.3f and %.3f" % (M.factor_classes(one), M.factor_classes(many), M.affine_deviation(one), M.affine_deviation(many)))
    assert M.offdiag_zero(one) and M.factor_classes(one) == 2 and M.shared(one) and M.affine_deviation(one) > 1e-6
    assert M.offdiag_zero(many) and M.factor_classes(many) == 15 and 2 * 15 > 27 and not M.shared(many)
    assert all(min(a.min() for a in mesh.g[:3]) > 0.0 for mesh in (one, many))
    box = S.BoxMesh(BOX, 7)
    denormal, minus = M.edited(box, "g_6", LAST, -1, 5e-324), M.edited(box, "g_6", LAST, -1, -0.0)
    assert not M.offdiag_zero(denormal) and M.offdiag_zero(denormal, range(26)) and M.offdiag_zero(minus) and np.signbit(minus.g[5][-1]) and M.offdiag_zero(box)
    # a rank's part holds the global elements that fall into it
    assert M.bumped((8, 2, 2), 5, [4], P=(2, 1, 1), rank=1).bumped_elements == [0] and M.bumped((8, 2, 2), 5, [4], P=(2, 1, 1), rank=0).bumped_elements == []


def check_case(case):
    """what of a case does not need the product's kernels: the written bits, the operator and its biting figure, the oracle
    solve; the stand-in of the kernel library switches nothing but the affine lists"""
    _, H, _ = DC.api()
    spec = CASES[case]
    directory = tempfile.mkdtemp(prefix="fdd_partial_")
    t0 = time.time()
    try:
        p, meshes = open_problem(H, case, directory)
        try:
            written_bits(p, meshes)
            nothing_switches(p)
            affine = affine_answers(p, meshes, spec["N"])
            operator(p, meshes[spec["N"]], spec["wrong"], case, affine)
            if spec["oracle"]:
                oracle_solve(p, spec["N"], spec["red"], case)
        finally:
            p.close()
    finally:
        shutil.rmtree(directory, ignore_errors=True)
    print("%s: %.2f s" % (case, time.time() - t0))


CHECKS = {"builders": check_builders}
CHECKS.update({c: (lambda c=c: check_case(c)) for c in CASES})


if __name__ == "__main__":
    _, H, lib = DC.api()
    # test-only: serve include/fdd_host.h from the CPU build of the host layer (tests/cpu_shim)
    lib._host = lib._Lib(sys.argv[1], os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    for name in sys.argv[2:]:
        CHECKS[name]()
    print("ok")
