"""Reconfiguring a live problem equals building a fresh one: the walk tables and the `fresh` / `walked` drivers shared by
test_cpu_reconfigure.py (the CPU build of the host layer, tests/cpu_shim, in a child process) and test_gpu_reconfigure.py.

A configuration is a complete set of options (fddh_problem_set_options), flags (fddh_problem_set_flag) and seven keys of
this module: "amg" (how the low-order hierarchy comes to be: None = the problem never has one, "first_use" = the
inner solve builds it, "host" / "device" = fddh_problem_amg_build with "amg_device_setup" 0 / 1, "attached" = handed in
level by level), "inner" (the method precond_apply is called with), "pcg_steps" (K > 0: pcg_begin / pcg_steps(K) /
pcg_solution join the workload) and the operator's terms: "D_hat" (None = the GLL table `build` sets, "perturbed" = a table
of the fine level that fails lean_table_ok), "helmholtz" (None, a constant, or "field": seeded, >= 0, with exact zeros) and
"diffusivity" (None, "smooth", or "jump": 1 : 1000 across an element face, diffusivity_checks.kappa_jump), and, on a mesh
with natural faces (a fifth entry of the mesh tuple: the face codes), "robin" (None or {side: alpha}, set after the shift
and before kappa at every step; on the other meshes the entry is never called).  `apply` sets
every key, always in the same order, so that fresh(c) and the last step of walked(..., c) differ in one thing only: what
the problem did before.  Two exceptions, the table and the flag "affine_geometry": every call of either empties all that
hangs on the operator (basis, diagonal, Chebyshev bound), made again only at the next use, so a call at every step would
stand in for whatever the shift or kappa owe at that step.  `apply` therefore sets these two only where they differ from
what the problem holds (`build`'s GLL table and the library's affine_geometry = 0 on a new problem; the driver keeps
track), and no step of a walk changes the table together with another term.  The shift and kappa are set at every step, in that order, after the flags: clearing one
that is not set returns before it touches anything, and one that is set is set again ("set twice in a row" is every such
pair of steps), which empties again -- so the walks change the affine flag and the shift also at steps where no kappa
is set, and kappa, set last, is never followed by another emptying.

The property (every step, not only the last): the outputs of step i of walked(c0, ..., ck) equal those of fresh(ci) bit
for bit -- vectors, residual histories, iteration counts.  Both sides run the same code on the same inputs and the suite
already relies on run-to-run repeatability; the control (two fresh(ck) runs) is asserted first.

A walk is a named list of (label, changes) steps; changes are relative to the step before.  A failure names the walk,
the step and its label, i.e. the transition.

Besides the walks: a stepwise run abandoned while it is live, then other solves (ABANDONED, run_abandoned_stepwise).

The CPU build: the walk whose hierarchy is built on the device is left out by name (CPU_LEFT_OUT).  The stand-in of the
kernel library also has no fdd_shift_add* and no coefficient instance of the line kernel, so fddh_helmholtz_set answers
"does not export" for any value and "coefficient_in_kernel" = 1 is refused.  No walk is left out for that: there every
walk runs with "helmholtz" None and "coefficient_in_kernel" 0 at every step (CPU_SUBSTITUTED, on_cpu), i.e. the table,
kappa and affine transitions of the family "operator" on a problem without a shift, and each step's printed label says so;
the shift's transitions are test_gpu_reconfigure.py's alone.

Run as a program (the CPU test does): reconfigure_walks.py <libfdd_host_cpu.so> <walk name, or a name of ABANDONED>.
"""
import sys

import numpy as np

import diffusivity_checks as K

# every option and flag a configuration sets, in the order `apply` sets them (values: the library's defaults, except the
# iteration cap, which keeps the solves short, and "sub_use_preconditioner", off where the walk has no hierarchy)
BASE = {
    # fddh_problem_set_options
    "max_iterations": 12,
    "tolerance": 1e-7,
    "num_vectors": 20,
    "use_preconditioner": 1,
    "preconditioner_type": 1,
    "sub_num_vectors": 4,
    "sub_max_iterations": 4,
    # fddh_problem_set_flag: launch sequences and kernel selection
    "fused_dssum": 1,
    "restructured_inner_solve": 1,
    "assembled_outer_solve": 1,
    "assembled_inner_solve": 1,
    "device_bookkeeping": 1,
    "skip_last_basis_store": 1,
    "shared_residual_norm": 1,
    "early_gamma": 1,
    "unit_stitch_in_place": 1,
    "lazy_steps": 1,
    "mfma_stiffness": 1,
    "affine_geometry": 0,
    "coefficient_in_kernel": 1,
    "inner_solver": 0,
    # the V-cycle
    "sub_use_preconditioner": 0,
    "amg_cheby_order": 2,
    "amg_num_vcycles": 1,
    "amg_graph": 1,
    "amg_fused_smoother": 1,
    "amg_matrix_free_transfer": 1,
    "preconditioner_precision": 64,
    "amg_precision": 64,
    # this module's keys
    "amg": None,
    "inner": "gmres",
    "pcg_steps": 0,
    "D_hat": None,
    "helmholtz": None,
    "robin": None,
    "diffusivity": None,
}
OPTION_KEYS = ("max_iterations", "tolerance", "num_vectors", "use_preconditioner", "preconditioner_type", "sub_num_vectors", "sub_max_iterations")
MODULE_KEYS = ("amg", "inner", "pcg_steps", "D_hat", "helmholtz", "robin", "diffusivity")
FLAG_KEYS = tuple(k for k in BASE if k not in OPTION_KEYS and k not in MODULE_KEYS)

# The CPU stand-in of the kernel library has no fdd_amg_setup_* entry: the host layer refuses "amg_device_setup" = 1 there
# (test_cpu_amg_device_setup.py), so walks whose hierarchy is built on the device are left out of the CPU file by name.
# "mfma_stiffness" and "amg_graph" are accepted there (one stiffness routine serves both kernels; a capture that the
# stand-in declines runs the same launches eagerly) and stay in.
# "affine_geometry" empties all that hangs on the operator at every call, whatever the value (like fddh_problem_set_D_hat, the
# module's docstring): `apply` sets it only where it differs from what the problem holds (BASE's 0, the library's default, on a
# new problem)
SET_ON_CHANGE = ("affine_geometry",)

CPU_LEFT_OUT = {"amg": ("device",)}
# Nor has it fdd_shift_add* or the coefficient instance of the line kernel: no walk is left out for that, these keys take the
# value given here at every step of every walk, and the label of a step they change says so (cpu_label).
CPU_SUBSTITUTED = {"helmholtz": None, "robin": None, "coefficient_in_kernel": 0}  # "robin": nor has it fdd_field_surface


def on_cpu(c):
    return dict(c, **CPU_SUBSTITUTED)


def cpu_label(label, changes):
    """the label of a step as the CPU build runs it: what the step asks for and the stand-in cannot do is named"""
    dropped = [k for k in CPU_SUBSTITUTED if k in changes]
    return label + (" [CPU build: without its change of %s]" % ", ".join(dropped) if dropped else "")


# Transitions the library refuses, as (walk, step label, option): a closed list, matched line for line by include/fdd_host.h
# (the comment on fddh_problem_set_flag).  The error text must name the option, the option keeps its earlier value and the
# property goes on holding.  No other transition of any walk may be refused.
REFUSED = (
    ("vcycle_attached", "order 3 on a handed-in hierarchy", "amg_cheby_order"),
    ("vcycle_host", "order 1 under the float cycle", "amg_cheby_order"),
)

BOX_SMALL = ("box", (4, 4, 4), 3, 2)   # BASELINE C1
BOX_N7 = ("box", (3, 3, 3), 7, 6)
BOX_N11 = ("box", (2, 2, 2), 11, 5)    # degrees 11, 6, 1: the fine level's stiffness runs on the matrix cores when "mfma_stiffness" is on
KERSHAW = ("kershaw", (4, 4, 4), 3, 2)
COMPOSITE = ("composite", (4, 4, 4), 3, 2)  # FDDH_FORCE_COMPOSITE on one rank
BOX_N7_NATURAL = ("box", (2, 2, 2), 7, 6, "DNNNDN")  # face codes: x+, y-, y+ and z+ natural, their end points are dofs

ADVICE = "the sequence of ADVICE.md: point-space GMRES(20), node-space GMRES(10), point-space GMRES(20)"

WALKS = {
    # ---- outer GMRES basis: num_vectors 20 -> 10 -> 20 -> 3, point space <-> node space, reference-shaped <-> restructured
    "outer_basis_advice": dict(mesh=BOX_SMALL, family="outer", oracle=True, base={"max_iterations": 25}, steps=[
        ("point-space GMRES(20)", {"num_vectors": 20, "assembled_outer_solve": 0, "restructured_inner_solve": 0}),
        ("node-space GMRES(10)", {"num_vectors": 10, "assembled_outer_solve": 1, "restructured_inner_solve": 1}),
        ("point-space GMRES(20) again: " + ADVICE, {"num_vectors": 20, "assembled_outer_solve": 0}),
        ("node-space GMRES(3)", {"num_vectors": 3, "assembled_outer_solve": 1}),
        ("point-space GMRES(3), reference-shaped", {"assembled_outer_solve": 0, "restructured_inner_solve": 0}),
        ("point-space GMRES(10), restructured", {"num_vectors": 10, "restructured_inner_solve": 1}),
        ("node-space GMRES(7) capped inside its second cycle", {"num_vectors": 7, "assembled_outer_solve": 1, "max_iterations": 9}),
    ]),
    "outer_basis_n7": dict(mesh=BOX_N7, family="outer", base={"max_iterations": 8}, steps=[
        ("node-space GMRES(20)", {}),
        ("point-space GMRES(10)", {"num_vectors": 10, "assembled_outer_solve": 0}),
        ("node-space GMRES(20)", {"num_vectors": 20, "assembled_outer_solve": 1}),
        ("point-space GMRES(3), reference-shaped", {"num_vectors": 3, "assembled_outer_solve": 0, "restructured_inner_solve": 0}),
    ]),
    "outer_basis_composite": dict(mesh=COMPOSITE, family="outer", base={"max_iterations": 8}, steps=[
        ("node-space GMRES(20)", {}),
        ("node-space GMRES(10)", {"num_vectors": 10}),
        ("point-space GMRES(20)", {"num_vectors": 20, "assembled_outer_solve": 0}),
        ("node-space GMRES(3)", {"num_vectors": 3, "assembled_outer_solve": 1}),
    ]),
    # ---- inner Krylov: (sub_num_vectors, sub_max_iterations) (4,9) -> (8,11) -> (1,1) -> (7,7) -> (2,5)
    "inner_krylov": dict(mesh=BOX_SMALL, family="inner", oracle=True, base={"amg": "host", "max_iterations": 6}, steps=[
        ("GMRES(4) x 9 with the V-cycle", {"sub_num_vectors": 4, "sub_max_iterations": 9, "sub_use_preconditioner": 1}),
        ("GMRES(8) x 11, identity, host bookkeeping", {"sub_num_vectors": 8, "sub_max_iterations": 11, "sub_use_preconditioner": 0, "device_bookkeeping": 0}),
        ("GMRES(1) x 1, point-Jacobi, point-space inner solve", {"sub_num_vectors": 1, "sub_max_iterations": 1, "sub_use_preconditioner": 2, "device_bookkeeping": 1, "assembled_inner_solve": 0}),
        ("inner FCG x 7, reference-shaped", {"sub_num_vectors": 7, "sub_max_iterations": 7, "inner": "fcg", "preconditioner_type": 0, "restructured_inner_solve": 0}),
        ("GMRES(7) x 7 with the V-cycle, last basis vector stored", {"inner": "gmres", "preconditioner_type": 1, "sub_use_preconditioner": 1, "assembled_inner_solve": 1, "restructured_inner_solve": 1, "skip_last_basis_store": 0}),
        ("GMRES(2) x 5, point space, host bookkeeping", {"sub_num_vectors": 2, "sub_max_iterations": 5, "assembled_inner_solve": 0, "device_bookkeeping": 0, "skip_last_basis_store": 1}),
        ("GMRES(2) x 5, identity, dof space: the oracle's configuration", {"sub_use_preconditioner": 0, "assembled_inner_solve": 1, "device_bookkeeping": 1}),
    ]),
    "inner_krylov_kershaw": dict(mesh=KERSHAW, family="inner", base={"max_iterations": 6}, steps=[
        ("GMRES(4) x 9", {"sub_num_vectors": 4, "sub_max_iterations": 9}),
        ("GMRES(8) x 11, point-Jacobi", {"sub_num_vectors": 8, "sub_max_iterations": 11, "sub_use_preconditioner": 2}),
        ("GMRES(1) x 1, host bookkeeping", {"sub_num_vectors": 1, "sub_max_iterations": 1, "device_bookkeeping": 0}),
        ("GMRES(7) x 7, identity, reference-shaped", {"sub_num_vectors": 7, "sub_max_iterations": 7, "sub_use_preconditioner": 0, "restructured_inner_solve": 0, "assembled_inner_solve": 0}),
        ("GMRES(2) x 5, dof space", {"sub_num_vectors": 2, "sub_max_iterations": 5, "restructured_inner_solve": 1, "assembled_inner_solve": 1, "device_bookkeeping": 1}),
    ]),
    "inner_krylov_composite": dict(mesh=COMPOSITE, family="inner", base={"max_iterations": 5}, steps=[
        ("GMRES(4) x 9", {"sub_num_vectors": 4, "sub_max_iterations": 9}),
        ("GMRES(8) x 11", {"sub_num_vectors": 8, "sub_max_iterations": 11}),
        ("GMRES(1) x 1, host bookkeeping", {"sub_num_vectors": 1, "sub_max_iterations": 1, "device_bookkeeping": 0}),
        ("GMRES(7) x 7, point-Jacobi", {"sub_num_vectors": 7, "sub_max_iterations": 7, "device_bookkeeping": 1, "sub_use_preconditioner": 2}),
        ("GMRES(2) x 5, point space", {"sub_num_vectors": 2, "sub_max_iterations": 5, "assembled_inner_solve": 0}),
    ]),
    # ---- V-cycle: (order, cycles) (1,1) -> (4,2) -> (2,2) -> (3,1); graph, smoother, transfer and both precisions toggled
    "vcycle_host": dict(mesh=BOX_N7, family="vcycle", oracle=True, oracle_vcycle_step=6, base={"amg": "host", "sub_use_preconditioner": 1, "max_iterations": 5, "sub_num_vectors": 2, "sub_max_iterations": 2}, steps=[
        ("order 1, 1 cycle", {"amg_cheby_order": 1, "amg_num_vcycles": 1}),
        ("order 4, 2 cycles, eager launches", {"amg_cheby_order": 4, "amg_num_vcycles": 2, "amg_graph": 0}),
        ("order 2, 2 cycles, float V-cycle, reference-shaped smoother", {"amg_cheby_order": 2, "amg_graph": 1, "amg_precision": 32, "amg_fused_smoother": 0}),
        ("float inner solve, CSR interpolators", {"preconditioner_precision": 32, "amg_fused_smoother": 1, "amg_matrix_free_transfer": 0}),
        ("order 1 under the float cycle", {"amg_cheby_order": 1, "sub_num_vectors": 3, "sub_max_iterations": 3}),
        ("double again", {"preconditioner_precision": 64, "amg_precision": 64}),
        ("order 3, 1 cycle, matrix-free interpolators", {"amg_cheby_order": 3, "amg_num_vcycles": 1, "amg_matrix_free_transfer": 1}),
        ("identity in the inner solve: the oracle's configuration", {"sub_use_preconditioner": 0, "sub_num_vectors": 4, "sub_max_iterations": 4}),
    ]),
    "vcycle_device": dict(mesh=BOX_N7, family="vcycle", base={"amg": "device", "sub_use_preconditioner": 1, "max_iterations": 5, "sub_num_vectors": 2, "sub_max_iterations": 2}, steps=[
        ("order 1, 1 cycle", {"amg_cheby_order": 1, "amg_num_vcycles": 1}),
        ("order 4, 2 cycles, eager launches", {"amg_cheby_order": 4, "amg_num_vcycles": 2, "amg_graph": 0}),
        ("order 2, 2 cycles, float inner solve", {"amg_cheby_order": 2, "amg_graph": 1, "preconditioner_precision": 32, "amg_precision": 32}),
        ("double, CSR interpolators", {"preconditioner_precision": 64, "amg_precision": 64, "amg_matrix_free_transfer": 0}),
        ("order 3, 1 cycle", {"amg_cheby_order": 3, "amg_num_vcycles": 1, "amg_fused_smoother": 0}),
    ]),
    "vcycle_first_use": dict(mesh=BOX_SMALL, family="vcycle", oracle_vcycle_step=3, base={"amg": "first_use", "sub_use_preconditioner": 1, "max_iterations": 5}, steps=[
        ("double, built by the first inner solve", {}),
        ("float V-cycle, eager launches, 2 cycles: a fresh problem sets these before anything is built", {"amg_precision": 32, "amg_graph": 0, "amg_num_vcycles": 2}),
        ("double, graph", {"amg_precision": 64, "amg_graph": 1}),
        ("order 3", {"amg_cheby_order": 3, "amg_num_vcycles": 1}),
    ]),
    "vcycle_attached": dict(mesh=BOX_SMALL, family="vcycle", base={"amg": "attached", "sub_use_preconditioner": 1, "max_iterations": 5}, steps=[
        ("order 2, 1 cycle", {}),
        ("2 cycles, eager launches", {"amg_num_vcycles": 2, "amg_graph": 0}),
        ("order 3 on a handed-in hierarchy", {"amg_cheby_order": 3, "amg_graph": 1}),
        ("float V-cycle, 1 cycle", {"amg_precision": 32, "amg_num_vcycles": 1}),
    ]),
    "vcycle_composite": dict(mesh=COMPOSITE, family="vcycle", base={"amg": "host", "sub_use_preconditioner": 1, "max_iterations": 4}, steps=[
        ("order 2, 1 cycle", {}),
        ("2 cycles, eager launches", {"amg_num_vcycles": 2, "amg_graph": 0}),
        ("order 3, graph", {"amg_cheby_order": 3, "amg_graph": 1}),
        ("order 2, 1 cycle, reference-shaped smoother", {"amg_cheby_order": 2, "amg_num_vcycles": 1, "amg_fused_smoother": 0}),
    ]),
    # ---- kernel selection: each switch 1 -> 0 -> 1 with a solve between
    "kernel_selection": dict(mesh=BOX_SMALL, family="kernels", oracle=True, base={"max_iterations": 6, "pcg_steps": 3}, steps=[
        ("all on", {}),
        ("fused_dssum off", {"fused_dssum": 0}),
        ("fused_dssum on, early_gamma off", {"fused_dssum": 1, "early_gamma": 0}),
        ("early_gamma on, unit_stitch_in_place off", {"early_gamma": 1, "unit_stitch_in_place": 0}),
        ("unit_stitch_in_place on, lazy_steps off", {"unit_stitch_in_place": 1, "lazy_steps": 0}),
        ("lazy_steps on, shared_residual_norm off", {"lazy_steps": 1, "shared_residual_norm": 0}),
        ("shared_residual_norm on, affine_geometry on", {"shared_residual_norm": 1, "affine_geometry": 1}),
        ("affine_geometry off, 5 steps", {"affine_geometry": 0, "pcg_steps": 5}),
    ]),
    "kernel_selection_n11": dict(mesh=BOX_N11, family="kernels", base={"max_iterations": 4, "pcg_steps": 2, "sub_num_vectors": 2, "sub_max_iterations": 2}, steps=[
        ("matrix cores", {}),
        ("scalar stiffness", {"mfma_stiffness": 0}),
        ("matrix cores, affine elements", {"mfma_stiffness": 1, "affine_geometry": 1}),
        ("scalar stiffness, affine elements, 3 steps", {"mfma_stiffness": 0, "pcg_steps": 3}),
    ]),
    "kernel_selection_composite": dict(mesh=COMPOSITE, family="kernels", base={"max_iterations": 4, "pcg_steps": 2}, steps=[
        ("all on", {}),
        ("fused_dssum off, lazy_steps off", {"fused_dssum": 0, "lazy_steps": 0}),
        ("fused_dssum on, early_gamma off", {"fused_dssum": 1, "lazy_steps": 1, "early_gamma": 0}),
        ("host bookkeeping, 3 steps", {"early_gamma": 1, "device_bookkeeping": 0, "pcg_steps": 3}),
    ]),
    # ---- tolerance and caps: a stop on the cap in the middle of a restart cycle, then a stop on the tolerance
    "tolerance_and_caps": dict(mesh=BOX_SMALL, family="caps", oracle=True, base={"num_vectors": 5, "pcg_steps": 4}, steps=[
        ("cap 7 inside the second cycle of GMRES(5)", {"max_iterations": 7, "tolerance": 0.0}),
        ("tolerance 1e-3 reached first", {"max_iterations": 60, "tolerance": 1e-3}),
        ("cap 3 inside the first cycle, point space", {"max_iterations": 3, "tolerance": 1e-12, "assembled_outer_solve": 0}),
        ("tolerance 1e-7", {"max_iterations": 60, "tolerance": 1e-7}),
        ("cap 11, node space, 2 steps", {"max_iterations": 11, "tolerance": 1e-30, "assembled_outer_solve": 1, "pcg_steps": 2}),
    ]),
    # ---- preconditioner on and off, and its type
    "preconditioner_on_off": dict(mesh=BOX_SMALL, family="precond", oracle=True, base={"max_iterations": 8}, steps=[
        ("inner GMRES", {"use_preconditioner": 1, "preconditioner_type": 1}),
        ("none", {"use_preconditioner": 0}),
        ("inner FCG", {"use_preconditioner": 1, "preconditioner_type": 0, "inner": "fcg"}),
        ("none, point space", {"use_preconditioner": 0, "assembled_outer_solve": 0}),
        ("inner GMRES(3) x 6", {"use_preconditioner": 1, "preconditioner_type": 1, "inner": "gmres", "assembled_outer_solve": 1, "sub_num_vectors": 3, "sub_max_iterations": 6}),
    ]),
    "preconditioner_on_off_kershaw": dict(mesh=KERSHAW, family="precond", base={"max_iterations": 8}, steps=[
        ("inner GMRES", {}),
        ("none", {"use_preconditioner": 0}),
        ("inner FCG, point space", {"use_preconditioner": 1, "preconditioner_type": 0, "inner": "fcg", "assembled_outer_solve": 0}),
    ]),
    # ---- the operator's terms: shift, kappa, a level's table and the affine arithmetic, set, changed, stacked and cleared
    "operator_terms_n7": dict(mesh=BOX_N7, family="operator", oracle=True, base={"amg": "host", "sub_use_preconditioner": 1, "max_iterations": 5, "sub_num_vectors": 2, "sub_max_iterations": 2}, steps=[
        ("Poisson", {}),
        ("lambda constant", {"helmholtz": 10.0}),
        ("lambda field", {"helmholtz": "field"}),
        ("kappa smooth on top of lambda", {"diffusivity": "smooth"}),
        ("kappa jump", {"diffusivity": "jump"}),
        ("kappa jump set again, streamed scaled arrays", {"coefficient_in_kernel": 0}),
        ("kappa cleared, lambda stays", {"diffusivity": None, "coefficient_in_kernel": 1}),
        ("all cleared, identity in the inner solve: the oracle's configuration", {"helmholtz": None, "sub_use_preconditioner": 0, "sub_num_vectors": 4, "sub_max_iterations": 4}),
    ]),
    "operator_terms_attached": dict(mesh=BOX_SMALL, family="operator", base={"amg": "attached", "sub_use_preconditioner": 1, "max_iterations": 5}, steps=[
        ("lambda on", {"helmholtz": 2.0}),
        ("kappa on", {"diffusivity": "smooth"}),
        ("both off, cap 4", {"helmholtz": None, "diffusivity": None, "max_iterations": 4}),
    ]),
    "operator_terms_first_use": dict(mesh=BOX_SMALL, family="operator", base={"amg": "first_use", "sub_use_preconditioner": 1, "max_iterations": 5}, steps=[
        ("kappa smooth, set before anything is built", {"diffusivity": "smooth"}),
        ("a solve more, cap 4", {"max_iterations": 4}),
        ("kappa jump", {"diffusivity": "jump"}),
        ("lambda on", {"helmholtz": 3.0}),
        ("affine on", {"affine_geometry": 1}),
        ("all off", {"diffusivity": None, "helmholtz": None, "affine_geometry": 0}),
    ]),
    # point-Jacobi in the inner GMRES reads the exact diagonal, which the shift sits on (the Chebyshev walks below leave the shift out)
    "operator_terms_jacobi": dict(mesh=BOX_SMALL, family="operator", base={"sub_use_preconditioner": 2, "max_iterations": 5}, steps=[
        ("Poisson", {}),
        ("lambda constant", {"helmholtz": 10.0}),
        ("lambda field", {"helmholtz": "field"}),
        ("lambda cleared, cap 4", {"helmholtz": None, "max_iterations": 4}),
    ]),
}
# the Chebyshev-Jacobi inner solve keeps cheby.lambda, the Jacobi inverses and the first step's scaling (w_generation) across
# solves: each kind of change but the shift (the fused gather epilogue steps aside under one), in both precisions
for _name, _precision in (("operator_terms_chebyshev", 64), ("operator_terms_chebyshev_f32", 32)):
    WALKS[_name] = dict(mesh=BOX_N7, family="operator", base={"inner_solver": 1, "preconditioner_precision": _precision, "max_iterations": 5}, steps=[
        ("Poisson", {}),
        ("D_hat perturbed", {"D_hat": "perturbed"}),
        ("D_hat back", {"D_hat": None}),
        ("kappa on", {"diffusivity": "smooth"}),
        ("affine on with kappa", {"affine_geometry": 1}),
        ("kappa off", {"diffusivity": None}),
        ("affine off, no kappa set", {"affine_geometry": 0, "max_iterations": 4}),
    ])
# Neumann and Robin faces: the Robin term is the shift's second source (rebuild_shift), on boundary dofs only -- the indexed
# shift kernel -- and on the diagonal of the level-0 matrix; with the hierarchy built on first use, and under the float
# Chebyshev-Jacobi inner solve, whose Jacobi inverses and eigenvalue bound carry it
_ROBIN_STEPS = [
    ("alpha set", {"robin": {1: 2.0, 3: 0.5}}),
    ("alpha changed", {"robin": {1: 0.25, 5: 4.0}}),
    ("lambda stacked on alpha", {"helmholtz": 10.0}),
    ("kappa stacked on both", {"diffusivity": "smooth"}),
    ("alpha cleared, lambda and kappa stay", {"robin": None}),
]
# after "all cleared" the oracle has every term that is left: the V-cycle of the hierarchy as the rebuilds left it is held to
# the oracle's on the mesh with its natural faces (check_vcycle_against_oracle, 1e-11)
WALKS["operator_terms_natural_faces_first_use"] = dict(mesh=BOX_N7_NATURAL, family="operator", oracle_vcycle_step=len(_ROBIN_STEPS), base={"amg": "first_use", "sub_use_preconditioner": 1, "max_iterations": 5}, steps=_ROBIN_STEPS + [
    ("all cleared, cap 4", {"helmholtz": None, "diffusivity": None, "max_iterations": 4}),
])
WALKS["operator_terms_natural_faces_chebyshev_f32"] = dict(mesh=BOX_N7_NATURAL, family="operator", base={"inner_solver": 1, "preconditioner_precision": 32, "max_iterations": 5}, steps=_ROBIN_STEPS + [
    ("all cleared, cap 4", {"helmholtz": None, "diffusivity": None, "max_iterations": 4}),
])
FAMILIES = ("outer", "inner", "vcycle", "kernels", "caps", "precond", "operator")


def walk_names(cpu):
    return [n for n, w in WALKS.items() if not (cpu and w.get("base", {}).get("amg") in CPU_LEFT_OUT["amg"])]


def configurations(walk, name=None, cpu=False):
    """The complete configuration of every step as (requested, in force): they differ in the options the library refuses at
    that step (REFUSED), which keep their value; the next step starts from what is in force.  cpu: as the CPU build runs it
    (on_cpu)."""
    c = dict(BASE)
    c.update(walk.get("base", {}))
    out = []
    for label, changes in walk["steps"]:
        assert set(changes) <= set(BASE), set(changes) - set(BASE)
        assert "D_hat" not in changes or not {"affine_geometry", "helmholtz", "diffusivity"} & set(changes), "a step changes the table alone: the call would empty what the other change owes"
        requested = dict(c)
        requested.update(changes)
        assert requested["helmholtz"] is None or requested["inner"] == "gmres", "the inner FCG is refused under a shift"
        if cpu:
            requested = on_cpu(requested)
        in_force = dict(requested)
        for w, at, option in REFUSED:
            if w == name and at == label:
                assert requested[option] != c[option], "a refusal is a change"
                in_force[option] = c[option]
        out.append((requested, in_force))
        c = in_force
    assert all(out[-1][1] != earlier[1] for earlier in out[:-1]), "a walk ends on a configuration of its own"
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Driver:
    """H: host_api, S: support, lib: the package's lib module (all bound to the library under test by the caller)"""

    def __init__(self, H, S, lib, cpu=False):
        self.H, self.S, self.lib, self.cpu = H, S, lib, cpu

    def build(self, mesh):
        kind, E, N, red = mesh[:4]
        faces = mesh[4] if len(mesh) > 4 else "DDDDDD"
        H, S = self.H, self.S
        if kind == "kershaw":
            p = H.Problem.kershaw(E, (1, 1, 1), N, red, 0.3, True, faces=faces)
        else:
            p = H.Problem.box(E, (1, 1, 1), N, red, True, force_composite=(kind == "composite"), faces=faces)
        p.natural_faces = "N" in faces  # only then is fddh_boundary_robin_set called at all
        for lvl in range(p.info["num_levels"]):
            p.set_D_hat(lvl, S.gll(p.level_degree(lvl))[2])
        p.takes_terms = kind != "composite"  # a composite refuses fddh_helmholtz_set and fddh_diffusivity_set whatever the value (capi_refusals.py)
        return p

    def apply(self, p, c, state, refusals=()):
        """Set every key of c.  state: what this problem's hierarchy is (None before it exists).  refusals: the options the
        library is expected to refuse at this step; returns the configuration in force afterwards."""
        in_force = dict(c)
        p.set_options(**{k: c[k] for k in OPTION_KEYS})
        for k in FLAG_KEYS:
            if k in SET_ON_CHANGE and c[k] == state.get("in_force", BASE)[k]:
                continue
            try:
                p.set_flag(k, c[k])
            except self.lib.FddError as exc:
                assert k in refusals, "set_flag(%r, %r) was refused and is not on the list of refusals: %s" % (k, c[k], exc)
                assert k in str(exc), "the refusal does not name the option %r: %s" % (k, exc)
                in_force[k] = state["in_force"][k]
            else:
                assert k not in refusals, "set_flag(%r, %r) is on the list of refusals and was accepted" % (k, c[k])
        if c["amg"] in ("host", "device") and state.get("amg") is None:
            p.amg_build(device=(c["amg"] == "device"))
            if c["amg"] == "device":
                assert p.amg_setup_info()["levels_built_on_device"] >= 1
            state["amg"] = c["amg"]
        elif c["amg"] == "attached" and state.get("amg") is None:
            m = self.S.ArrayMesh.from_problem(p)
            p.amg_attach(self.S.low_order_hierarchy(m, p.sub_point_dofs(), p.info["sub_num_dofs"]))
            state["amg"] = "attached"
        self.set_operator_terms(p, c, state)
        state["in_force"] = in_force
        return in_force

    def set_operator_terms(self, p, c, state):
        """state["D_hat"]: the table this problem holds (absent: the GLL table `build` set)"""
        S = self.S
        assert c["D_hat"] in (None, "perturbed")
        if c["D_hat"] != state.get("D_hat"):  # only a change: the call empties everything (the module's docstring)
            D = S.gll(p.level_degree(0))[2].copy()
            if c["D_hat"] == "perturbed":
                D.flat[1] *= 1.0 + 2.0**-10  # entry 62 is no longer the negation of entry 1
            p.set_D_hat(0, D)
            state["D_hat"] = c["D_hat"]
        if not p.takes_terms:
            assert c["helmholtz"] is None and c["diffusivity"] is None
            return
        if not self.cpu:  # the stand-in's fddh_helmholtz_set answers "does not export" for any value
            lam = c["helmholtz"]
            if lam == "field":
                lam = np.where(S.seeded_uniform(p.n, 78) < 0.25, 0.0, 50.0 * S.seeded_uniform(p.n, 77))
            p.helmholtz(0.0 if lam is None else lam)
        else:
            assert c["helmholtz"] is None
        if p.natural_faces and not self.cpu:  # the stand-in's fddh_boundary_robin_set answers "does not export"
            p.robin(c["robin"])
        else:
            assert c["robin"] is None
        kappa = c["diffusivity"]
        if kappa == "smooth":
            kappa = K.kappa_smooth(*(p.mesh_array(a) for a in "xyz"))
        elif kappa == "jump":
            kappa = K.kappa_jump(p.mesh_array("x"), (p.level_degree(0) + 1) ** 3, 1000.0)
        else:
            assert kappa is None
        p.diffusivity(kappa)

    def workload(self, p, c, step):
        """The inputs depend on the step: state kept from the step before (a cached basis, a history, a right-hand side on the
        device) then holds values the new step would NOT compute, and shows.  fresh(ci) is given the same i."""
        S = self.S
        r = S.seeded_uniform(p.n, 15 + step) - 0.5
        _, f = p.make_rhs_from(S.seeded_uniform(p.n, 1234 + step))
        out = {}
        out["precond.z"], out["precond.history"] = p.precond_apply(r, c["inner"])
        for method in ("fcg", "gmres"):
            u, its, hist = p.solve(f, method)
            out[method + ".u"], out[method + ".iterations"], out[method + ".history"] = u, its, hist
        if c["amg"] is not None:
            out["amg_apply.z"] = p.amg_apply(r)
        if c["pcg_steps"]:
            p.pcg_begin(f)
            out["pcg_steps.residual"] = np.array([p.pcg_steps(c["pcg_steps"])])
            out["pcg_steps.u"] = p.pcg_solution()
        return out

    def fresh(self, mesh, c, step):
        p = self.build(mesh)
        try:
            self.apply(p, c, {})
            return self.workload(p, c, step)
        finally:
            p.close()


def differences(a, b):
    """names of the outputs that are not the same bits (or counts, or lengths)"""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    bad = []
    for k in a:
        if isinstance(a[k], (int, np.integer)):
            if a[k] != b[k]:
                bad.append("%s: %d != %d" % (k, a[k], b[k]))
        elif a[k].shape != b[k].shape:
            bad.append("%s: %d entries != %d" % (k, a[k].size, b[k].size))
        elif not np.array_equal(bits(a[k]), bits(b[k])):
            bad.append("%s: max |difference| %.3e of %.3e" % (k, np.nanmax(np.abs(a[k] - b[k])), np.nanmax(np.abs(b[k]))))
    return bad


def check_against_oracle(driver, p, c, mesh):
    """The last step of a walk held to the oracle itself (test_gpu_host.py::test_inner_gmres_restarts_and_stops_inside_a_cycle,
    its 1e-9 bars): the inner GMRES without the V-cycle, in double, on this very problem after everything it went through."""
    S = driver.S
    assert c["inner"] == "gmres" and c["sub_use_preconditioner"] == 0 and c["preconditioner_precision"] == 64, "a walk marked oracle=True ends on the oracle's configuration"
    _, _, N, red = mesh[:4]
    meshes = [S.ArrayMesh.from_problem(p, lvl) for lvl in range(p.info["num_levels"])]
    sd = S.OracleSubdomain(None, N, red, meshes=meshes)
    try:
        r = S.seeded_uniform(p.n, 15) - 0.5
        z, hist = p.precond_apply(r, "gmres")
        oz, _, ohist = sd.solve(r, "gmres", num_vectors=c["sub_num_vectors"], max_iterations=c["sub_max_iterations"])
        assert len(hist) == len(ohist), (len(hist), len(ohist))
        print("    oracle: history %.2e, solution %.2e (relative)" % (np.abs(hist - ohist).max() / ohist[0], np.abs(z - oz).max() / np.abs(oz).max()))
        assert np.abs(hist - ohist).max() <= 1e-9 * ohist[0]
        assert np.abs(z - oz).max() <= 1e-9 * np.abs(oz).max()
    finally:
        sd.close()


def check_vcycle_against_oracle(driver, p, c, mesh):
    """The V-cycle of a walked problem held to the oracle's (amg_checks.check_amg, its 1e-11 bar: the product applies the
    polynomial as A (D w) and a precomputed inverse on the coarsest level, the oracle val D w and an elimination): the
    hierarchy as it stands after the rebuilds of the walk is read back, handed to the oracle with level 0 renumbered to the
    oracle's dofs, and one application compared."""
    import scipy.sparse as sp

    S = driver.S
    assert c["amg_precision"] == 64 and c["preconditioner_precision"] == 64 and c["amg"] in ("host", "first_use")
    _, _, N, red = mesh[:4]
    meshes = [S.ArrayMesh.from_problem(p, lvl) for lvl in range(p.info["num_levels"])]
    sd = S.OracleSubdomain(None, N, red, meshes=meshes)
    try:
        dof, odof, nd = p.sub_point_dofs(), sd.point_dofs(), p.info["sub_num_dofs"]
        assert np.array_equal(dof >= 0, odof >= 0)
        pair = {}
        for a, b in zip(dof[dof >= 0], odof[odof >= 0]):
            assert pair.setdefault(int(a), int(b)) == int(b)
        levels = p.amg_levels(c["amg_cheby_order"])
        assert len(levels) >= 2 and levels[0]["A"].shape[0] == nd and len(levels[0]["coefs"]) == c["amg_cheby_order"]
        Pm = sp.csr_matrix((np.ones(nd), (np.array([pair[a] for a in range(nd)]), np.arange(nd))), shape=(nd, nd))
        fine = dict(levels[0])
        fine["A"] = (Pm @ levels[0]["A"] @ Pm.T).tocsr()
        fine["D"] = np.asarray(Pm @ levels[0]["D"])
        fine["P"] = (Pm @ levels[0]["P"]).tocsr()
        sd.attach_amg([fine] + levels[1:], cheby_order=c["amg_cheby_order"], num_vcycles=c["amg_num_vcycles"])
        r = S.seeded_uniform(p.n, 5) - 0.5
        z, oz = p.amg_apply(r), sd.low_order_preconditioner(r)
        print("    oracle V-cycle (order %d, %d cycles): %.2e (relative)" % (c["amg_cheby_order"], c["amg_num_vcycles"], np.abs(z - oz).max() / np.abs(oz).max()))
        assert np.abs(oz).max() > 0 and np.abs(z - oz).max() <= 1e-11 * np.abs(oz).max()
    finally:
        sd.close()


def run_walk(driver, name):
    """walked(c0, ..., ck) on one problem against fresh(ci) at every step; the control first.  Raises AssertionError naming
    every transition whose outputs differ."""
    walk = WALKS[name]
    mesh = walk["mesh"]
    configs = configurations(walk, name, driver.cpu)
    labels = [cpu_label(*s) if driver.cpu else s[0] for s in walk["steps"]]
    last = configs[-1][1]

    k = len(configs) - 1
    control = differences(driver.fresh(mesh, last, k), driver.fresh(mesh, last, k))
    assert not control, "%s: two fresh problems at the last configuration differ: %s" % (name, control)

    failures = []
    p = driver.build(mesh)
    try:
        state = {}
        for i, (requested, expected) in enumerate(configs):
            refusals = [k for k in requested if requested[k] != expected[k]]
            in_force = driver.apply(p, requested, state, refusals)
            assert in_force == expected
            got = driver.workload(p, in_force, i)
            bad = differences(got, driver.fresh(mesh, in_force, i))
            print("  %s step %d (%s)%s: %s" % (name, i, labels[i], " [refused: %s]" % ", ".join(refusals) if refusals else "", "same bits as a fresh problem" if not bad else bad))
            if bad:
                failures.append("step %d, '%s' -> '%s': %s" % (i, labels[i - 1] if i else "(new problem)", labels[i], "; ".join(bad)))
            if walk.get("oracle_vcycle_step") == i:
                check_vcycle_against_oracle(driver, p, in_force, mesh)
        assert not failures, "%s: a reconfigured problem differs from a fresh one:\n  " % name + "\n  ".join(failures)
        if walk.get("oracle"):
            check_against_oracle(driver, p, last, mesh)
    finally:
        p.close()


# ---- a stepwise run abandoned while it is live: an order no walk runs (their pcg_begin / pcg_steps always end in pcg_solution
# and nothing follows inside the step).  The two one-rank boxes whose dof slice ends at an odd and at an even node
# (test_gpu_fused_passes.py), with the V-cycle inside the inner solve.
ABANDONED = {
    "abandoned_stepwise_odd_slice_end": ("box", (4, 4, 4), 3, 2),
    "abandoned_stepwise_even_slice_end": ("box", (4, 3, 3), 5, 4),
}


def run_abandoned_stepwise(driver, name):
    """pcg_begin, pcg_steps(2) and no pcg_solution -- the inner solve's lazy history is still on the device and the outer
    solver's run state is that of iteration 2 -- then solve(fcg), solve(gmres) and precond_apply(gmres) with another
    right-hand side: the bits (vectors, histories, iteration counts) of a fresh problem given the same three calls."""
    S = driver.S
    mesh = ABANDONED[name]
    c = dict(BASE, amg="host", sub_use_preconditioner=1)
    if driver.cpu:
        c = on_cpu(c)

    def three_calls(p):
        r = S.seeded_uniform(p.n, 16) - 0.5
        _, f2 = p.make_rhs_from(S.seeded_uniform(p.n, 1235))
        out = {}
        for method in ("fcg", "gmres"):
            out[method + ".u"], out[method + ".iterations"], out[method + ".history"] = p.solve(f2, method)
        out["precond.z"], out["precond.history"] = p.precond_apply(r, "gmres")
        return out

    outs = []
    for abandon in (True, False):
        p = driver.build(mesh)
        try:
            driver.apply(p, c, {})
            if abandon:
                _, f1 = p.make_rhs_from(S.seeded_uniform(p.n, 1234))
                p.pcg_begin(f1)
                assert np.isfinite(p.pcg_steps(2))
            outs.append(three_calls(p))
        finally:
            p.close()
    bad = differences(outs[0], outs[1])
    print("  %s: %s" % (name, "same bits as a fresh problem" if not bad else bad))
    assert outs[1]["fcg.iterations"] > 2 and outs[1]["gmres.iterations"] > 2 and len(outs[1]["precond.history"]) > 1
    assert not bad, "%s: after an abandoned stepwise run the problem differs from a fresh one: %s" % (name, "; ".join(bad))


def families_have_an_oracle_walk():
    return {f: [n for n, w in WALKS.items() if w["family"] == f and w.get("oracle")] for f in FAMILIES}


if __name__ == "__main__":
    import os

    host_so, walk = sys.argv[1], sys.argv[2]
    here = os.path.dirname(os.path.abspath(__file__))
    for d in (os.path.dirname(here), here):
        if d not in sys.path:
            sys.path.insert(0, d)
    import support as S
    from polynomial_reduction_with_full_domain_decomposition_preconditioner_amd import host_api as H, lib

    lib._host = lib._Lib(host_so, os.path.join(lib.INCLUDE_DIR, "fdd_host.h"), "fddh_last_error")  # test-only: the CPU build of the host layer
    H.init(0, use_torch_stream=False)
    H.comm_single()
    H.set_print(False)
    (run_abandoned_stepwise if walk in ABANDONED else run_walk)(Driver(H, S, lib, cpu=True), walk)
    print("ok")
