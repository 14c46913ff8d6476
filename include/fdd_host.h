/*
 * fdd_host.h -- C-ABI of libfdd_host.so: the C++ host classes
 * (CSR_Matrix / Math / Domain / Subdomain, mirrors of the reference's
 * csr_matrix.hpp / math.hpp / domain.hpp / subdomain.hpp) and what the
 * reference's driver does with them (poisson.cpp:150-251: one Domain per
 * polynomial level, a Subdomain preconditioner, manufactured right-hand side,
 * outer flexible CG / GMRES), exposed with plain pointers so that tests,
 * bench.py and foreign-language hosts can drive it.
 *
 * Vectors cross this boundary as HOST arrays of num_local_points doubles
 * (element-major, the layout of the mesh files); the solver works on device
 * copies.  Every entry returns 0 on success; fddh_last_error() has the text.
 */
#ifndef FDD_HOST_H
#define FDD_HOST_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *fddh_last_error(void);

/* Device and stream of this rank (OCCA_Initialize, poisson.cpp:127-148).
 * own_stream != 0 creates a private non-blocking stream (stream is ignored);
 * otherwise every kernel runs on `stream` exactly as given -- NULL is the
 * default stream.  Pass torch's current stream to share ordering with
 * torch.distributed collectives. */
int fddh_init(int device, void *stream, int own_stream);
int fddh_set_print(int on); /* rank-0 residual history lines (rstdout) */
int fddh_set_timer(int on); /* named timing regions (timer.hpp); off by default */
int fddh_timer_total(const char *key, double *seconds);
/* the same aggregated over the ranks, "max" (the reference's table, poisson.cpp:256, timer.tpp:67) or "sum": collective */
int fddh_timer_total_over_ranks(const char *key, const char *aggregation, double *seconds);

/* Communicator (MPI_Initialize, poisson.cpp:84-89).  Exactly one of: */
int fddh_comm_single(void);
int fddh_comm_rccl_unique_id(char *out128);                        /* rank 0; ship the 128 bytes to all ranks */
int fddh_comm_rccl_init(const char *id128, int rank, int size);    /* RCCL over xGMI, called directly */
typedef int (*fddh_allreduce_fn)(void *ctx, void *buf, long long n);
typedef int (*fddh_allgather_fn)(void *ctx, const void *send, void *recv, long long bytes);
typedef int (*fddh_barrier_fn)(void *ctx);
int fddh_comm_callbacks(int rank, int size, void *ctx, fddh_allreduce_fn allreduce_sum_f64, fddh_allreduce_fn allreduce_max_f64, fddh_allgather_fn allgather_bytes, fddh_barrier_fn barrier);
/* The same with the point-to-point exchange the composite region needs (the reference's gslib pull of neighbour
 * elements, subdomain.tpp:601-642, 4626): one grouped call, n peers; send_bytes[i] from send[i] go to peers[i] and
 * recv_bytes[i] from peers[i] arrive in recv[i] (device buffers of this rank; either side may be 0). */
typedef int (*fddh_exchange_fn)(void *ctx, int n, const int *peers, const void *const *send, const long long *send_bytes, void *const *recv, const long long *recv_bytes);
int fddh_comm_callbacks_ex(int rank, int size, void *ctx, fddh_allreduce_fn allreduce_sum_f64, fddh_allreduce_fn allreduce_max_f64, fddh_allgather_fn allgather_bytes, fddh_barrier_fn barrier, fddh_exchange_fn exchange_bytes);
/* Several ranks inside ONE process, each on its own host thread (every fddh_* entry acts on the calling thread's rank:
 * device stream, communicator, timer and print switches are per thread), sharing one GPU: collectives are device-to-device
 * copies and rank-ordered sums between the ranks' buffers.  For rehearsing the N-rank path where RCCL cannot be used (it
 * admits one rank per device): create the world once, then every rank thread calls fddh_init (own stream) and
 * fddh_comm_local with its rank. */
int fddh_local_world_create(void **world, int size);
int fddh_local_world_destroy(void *world);
/* a rank of the world failed outside a collective (its thread raised): wake the peers waiting for it with an error now */
int fddh_local_world_fail(void *world);
/* end of a rank thread: release what fddh_init(own_stream) / fddh_comm_* gave the calling thread (stream, communicator) */
int fddh_rank_finalize(void);
int fddh_comm_local(void *world, int rank);
int fddh_comm_info(int *rank, int *size, char *name, size_t name_len);
/* run every collective of the active communicator once on n doubles and verify the results */
int fddh_comm_selftest(int n);

/* A "problem" = what run_simulation builds (poisson.cpp:176-206): Domains for
 * the levels N, N-r, ..., 1 of this rank and, optionally, the Subdomain
 * preconditioner over them. */
typedef struct fddh_problem fddh_problem;

/* synthetic box mesh: E global elements, P rank blocks per direction */
int fddh_problem_create_box(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int with_subdomain);
/* Nek5000-export directory, the reference's input (poisson.cpp:61-68, domain.tpp:45-224) */
int fddh_problem_create_dir(fddh_problem **out, const char *directory, int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int with_subdomain);
/* The same with the reference's overlap arguments (poisson.cpp:61-68) and construction flags:
 *   FDDH_WITH_SUBDOMAIN    build the Subdomain preconditioner
 *   FDDH_BLOCK_LOCAL       more than one rank: keep every rank's own elements only (no neighbour rings, no
 *                          superdomain): block-Jacobi, the comparison point of the full-domain-decomposition method
 *   FDDH_FORCE_COMPOSITE   build the region through the composite setup even on one rank (test hook) */
enum
{
    FDDH_WITH_SUBDOMAIN = 1,
    FDDH_BLOCK_LOCAL = 2,
    FDDH_FORCE_COMPOSITE = 4
};
int fddh_problem_create_box_ex(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags);
int fddh_problem_create_dir_ex(fddh_problem **out, const char *directory, int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags);
/* frees every device block, plan and captured graph the problem took; refused (and then nothing is freed) from a thread that
 * is not the rank that built it, or after that rank's fddh_rank_finalize */
int fddh_problem_destroy(fddh_problem *p);
/* write the box mesh of this rank as the reference's file set under `directory` */
int fddh_write_box_mesh_files(const char *directory, const int E[3], const int P[3], int poly_degree, int rank);
/* The box mesh under the generalized Kershaw map (eps_y, eps_z in (0, 1]; 1 = the uniform box): the geometry of every
 * experiment of the reference (run.py:25-47, run.sh:30: Nek5000 "Kershaw" exports with eps = 0.3, which are not in the
 * repository).  GLL points moved by the map, the six geometric factors isoparametric at each level's own degree, all six
 * non-zero (host/box_mesh.hpp). */
int fddh_problem_create_kershaw_ex(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags, double eps_y, double eps_z);
int fddh_write_kershaw_mesh_files(const char *directory, const int E[3], const int P[3], int poly_degree, int rank, double eps_y, double eps_z);
/* The same meshes with a boundary condition per face of the cube (an option of this build; the block "Neumann and Robin
 * faces" below): faces = six characters for x-, x+, y-, y+, z-, z+, 'D' Dirichlet (the points of the face are masked) or 'N'
 * natural (they are unknowns).  A point is masked iff it lies on at least one 'D' face: an edge between a 'D' and an 'N' face
 * is Dirichlet.  The same codes at every level's degree; the Kershaw map keeps the faces; eps 1.0 is the uniform box.  Mesh
 * data, accepted for any rank grid.  Another character or length is refused.  The entries above are these with "DDDDDD". */
int fddh_problem_create_box_faces(fddh_problem **out, const int E[3], const int P[3], int poly_degree, int poly_reduction, int subdomain_overlap, int superdomain_overlap, int flags, double eps_y, double eps_z, const char *faces);
int fddh_write_box_faces_mesh_files(const char *directory, const int E[3], const int P[3], int poly_degree, int rank, double eps_y, double eps_z, const char *faces);

enum
{
    FDDH_INFO_NUM_LOCAL_POINTS = 0,
    FDDH_INFO_NUM_LOCAL_NODES,
    FDDH_INFO_NUM_BDARY_NODES,
    FDDH_INFO_NUM_INTERFACE_SLOTS,
    FDDH_INFO_NUM_TOTAL_NODES,
    FDDH_INFO_NUM_TOTAL_ELEMENTS,
    FDDH_INFO_NUM_LOCAL_ELEMENTS,
    FDDH_INFO_NUM_LEVELS,
    FDDH_INFO_SUB_NUM_VALUES,
    FDDH_INFO_SUB_NUM_DOFS,
    FDDH_INFO_NUM_ITERATIONS,
    FDDH_INFO_DIM, /* 2 or 3: set by the mesh (domain.tpp:47) */
    FDDH_INFO_COUNT
};
int fddh_problem_info(const fddh_problem *p, long long *info, int n);
int fddh_problem_level_degree(const fddh_problem *p, int level, int *poly_degree);

/* The composite region of this rank (subdomain.tpp:455-579, 2581-2583) */
enum
{
    FDDH_SUB_IS_COMPOSITE = 0,   /* 1: rings + superdomain (more than one rank), 0: the rank's own conforming elements */
    FDDH_SUB_NUM_ELEMS,          /* own + ring elements */
    FDDH_SUB_NUM_EXT_ELEMS,      /* + the extended ring */
    FDDH_SUB_NUM_POINTS,         /* points of all of them = head of a composite vector */
    FDDH_SUB_NUM_SUB_DOFS,       /* subdomain dofs: regular + interface */
    FDDH_SUB_NUM_SUB_EXT_DOFS,   /* + extended */
    FDDH_SUB_NUM_INTERFACE_DOFS,
    FDDH_SUB_NUM_SUP_DOFS,       /* superdomain dofs: interface + regular */
    FDDH_SUB_NUM_SUP_EXT_DOFS,   /* + extended = tail of a composite vector */
    FDDH_SUB_NUM_UNIQUE_DOFS,    /* Subdomain::num_dofs */
    FDDH_SUB_NUM_COARSE_DOFS,    /* degree-1 dofs of the whole domain */
    FDDH_SUB_NUM_VALUES,
    FDDH_SUB_OWN_POINTS,
    FDDH_SUB_NUM_PEERS,          /* ranks this one exchanges ring data with */
    FDDH_SUB_INFO_COUNT
};
int fddh_problem_sub_info(const fddh_problem *p, long long *info, int n);
/* global element id and polynomial level of every region element (FDDH_SUB_NUM_EXT_ELEMS entries) */
int fddh_problem_sub_region(const fddh_problem *p, int *element, int *level, int n);
/* composite dofs kept per coarsening level of the superdomain (at most n values; *num_levels receives the count) */
int fddh_problem_sub_composite_levels(const fddh_problem *p, int *kept, int n, int *num_levels);

/* mesh arrays of a level as Domain::initialize holds them: name in
 * {"x","y","z","glo_num"(int64),"node_degree"(int32),"p_mask","g_1".."g_6"} */
int fddh_problem_mesh_array(const fddh_problem *p, int level, const char *name, void *out, size_t bytes);
/* CSR of the fine level's gather matrix Qt / scatter matrix Q (host copies) */
int fddh_problem_csr(const fddh_problem *p, int which /*0 = Q, 1 = Qt*/, int *num_rows, int *num_cols, int *num_nnz, int *ptr, int *col, double *val);
int fddh_problem_assembled_weight(const fddh_problem *p, double *out, int n);

/* Replace the GLL tables (D_hat of a level, J_cf between two levels) -- tests
 * feed the reference's own tables so parity does not hinge on the last bit of
 * the GLL nodes. */
int fddh_problem_set_D_hat(fddh_problem *p, int level, const double *D_hat, int n);
int fddh_problem_get_D_hat(const fddh_problem *p, int level, double *D_hat, int n);

/* Solver options: domain.hpp:112-118 and subdomain.hpp:228-238.  Negative
 * values (and NaN tolerance) leave a field unchanged. */
int fddh_problem_set_options(fddh_problem *p, int max_iterations, double tolerance, int num_vectors, int use_preconditioner, int preconditioner_type, int sub_num_vectors, int sub_max_iterations, int sub_build_tree);

/* Implementation switches (results are identical either way; the reference-shaped
 * launch sequences stay available for comparison):
 *   "fused_dssum"              1: one gather-scatter kernel per dssum (default), 0: the Qt / Q SpMV pair
 *   "restructured_inner_solve" 1: inner GMRES with cached assembled vectors, multi-dot / multi-axpy (default),
 *                              0: the reference's launch-by-launch sequence (subdomain.tpp:4309-4489)
 *   "assembled_outer_solve"    1: flexible CG on node vectors (one value per assembled node): Q fused into the stiffness
 *                              load, no dssum pass, the inner solve entered and left in dof numbering (default when the
 *                              inner solve is the assembled GMRES or there is no preconditioner); 0: point vectors
 *   "lazy_steps"               1: fddh_problem_pcg_steps(K) runs its K iterations with ONE host synchronisation, at the end
 *                              (norms kept in a device-side history, inner solves without their end-of-cycle read; default)
 *   "device_bookkeeping"       1: Givens rotations / stopping tests of the inner GMRES in one-thread kernels and alpha, beta
 *                              of the node-space PCG read from device memory: two host synchronisations per PCG step
 *                              (default); 0: the host computes them between launches, as the reference does
 *   "assembled_inner_solve"    1: inner GMRES on vectors over the dofs, Q fused into the stiffness load, one host
 *                              synchronisation per step (default); 0: the point-space forms above
 *   "mfma_stiffness"           1: degrees 11..15 apply the stiffness on the fp64 matrix cores (default;
 *                              agrees with the bit-exact kernel to ~1e-15, not bit for bit), 0: scalar fused kernel
 *   "sub_use_preconditioner"   1: the inner solver preconditions with the low-order AMG V-cycle
 *                              (Subdomain::use_preconditioner, subdomain.hpp:231; the reference's and this build's default),
 *                              0: the identity on assembled data (dssum, subdomain.tpp:4379-4382),
 *                              2: point-Jacobi, the exact diagonal of the inner iteration's operator -- a labelled option of
 *                              this build, not in the reference (host/subdomain.hpp)
 *   "amg_graph"                1: the V-cycle is replayed as one hipGraph when the stream allows capture (default)
 *   "amg_fused_smoother"       1: the smoother's element-wise kernels run as SpMV epilogues, bit-identical (default); 0: the reference's launch sequence 
 *   "amg_precision"            64 (default) or 32: the reference's `Float` (AMG/config.hpp:4): the V-cycle in double or in float
 *   "amg_device_setup"         0 (default): the low-order AMG hierarchy is built on the host threads; 1: the FEM matrix and
 *                              every level coarsened on the lattice are built on the device and stay in HBM (the first level
 *                              that is not comes back to the host loop), bit-identical to the host build.  Applies to
 *                              fddh_problem_amg_build and to the build on first use; a composite region builds on the host
 *                              and says so.  Fails, naming the entry, when the kernel library lacks an fdd_amg_setup_* entry.
 *   "fused_projection"         1 (default where the kernel library has the fdd_projection_* entries): the passes of the
 *                              projection (below) are single launches of csrc/fdd_projection.hip; 0: they are composed from
 *                              the multi-vector entries (the only form on a library without them; setting 1 there fails,
 *                              naming the entry).  Same sums, same element-wise bits; the basis stays.
 *   "inner_solver"             0 (default): the inner FCG / GMRES(m); 1: the Chebyshev-Jacobi iteration (an option of this
 *                              build, see fddh_problem_inner_chebyshev_configure below), which takes the place of either.
 *   "inner_chebyshev_order"    1..16 (default 4): diagonal scalings per application; one operator application fewer
 *   "inner_chebyshev_lower_permille" 1..999 (default 100): the lower end of the interval in thousandths of lambda
 *   "chebyshev_kernels"        1 (default where the kernel library has fdd_cheby_step / _f32): a step of that iteration is one
 *                              launch; 0: composed from vector_vector_addition and vector_diagonal_scaling_dev.  Same bits.
 *   "fused_chebyshev"          1 (default where the library has fdd_csr_plan_gather_cheby / _f32): in a conforming region of unit
 *                              norm weight the step is the epilogue of the gather Qt in front of it; 0: gather, then the step.
 *                              Same bits.  Either flag set to 1 on a library without the entries fails, naming the entry.
 *   "amg_num_vcycles" 1..16, "amg_cheby_order" 1..4 (subdomain.hpp:236-237), "amg_matrix_free_transfer",
 *   "preconditioner_precision" 64 / 32 (the whole inner solve)
 *
 * Changing options and flags on a live problem.  The settings above may be changed between two calls of a problem that
 * has already solved something; tests/reconfigure_walks.py walks one-rank problems (box, Kershaw, forced composite)
 * through lists of them, setting the flags in the order of that file, and requires at every step the bits of a problem
 * built anew with the same settings.  That, not more, is what is covered: several ranks are not, nor is every order of
 * setting the flags.  Buffers follow the sizes, captured graphs are dropped with the setting they were captured under,
 * and the V-cycle's switches outlive a (re)build of the hierarchy.  "amg_cheby_order" on a hierarchy of
 * fddh_problem_amg_build's own (explicit or on first use) builds it again with the options of that build and the current
 * "amg_device_setup" -- the whole setup is paid again (one line on stdout says how long it took).
 * Where the order of setting matters:
 *   "preconditioner_precision" 32 is checked against "device_bookkeeping" / "assembled_inner_solve" when it is set (both
 *                              must be on); switching one of them off afterwards is accepted, while a problem built anew
 *                              that sets them in that other order is refused: not covered by the walks
 *   "preconditioner_precision" sets the V-cycle's precision too once a hierarchy exists: set "amg_precision" after it
 *   "amg_precision" / "preconditioner_precision" 32 need a Chebyshev order of at least 2 at the time they are set
 * What changes the operator of a live problem: fddh_problem_set_D_hat (any level), the flag "affine_geometry",
 * fddh_helmholtz_set and fddh_diffusivity_set (below).  All four end in one place, operator_changed in
 * host/fdd_host_capi.cpp, which says what each reaches.  Every one of them empties a live projection basis
 * (fddh_problem_projection_configure), since its stored images A X would no longer be the operator's, and drops the
 * point-Jacobi diagonal, its inverses, the Chebyshev-Jacobi eigenvalue bound and the first step's scaling, which are made
 * again at next use; a table also replaces the inner solve's host and float copies of it and their lean verdicts; the
 * shift and kappa also rebuild a hierarchy that fddh_problem_amg_build made (one that was handed in is the caller's and
 * stays).  A shift of zero on a problem that has none changes nothing and empties nothing.  Solver options and the other
 * flags leave all of it alone.
 * Refused on a live problem, with an error that names the option, the option keeping its value (the closed list of
 * refused transitions; tests/reconfigure_walks.py REFUSED matches it line for line):
 *   "amg_cheby_order"          a new value once a hierarchy has been handed in (fddh_problem_amg_add_level): its
 *                              coefficients are the caller's
 *   "amg_cheby_order"          a value below 2 while "amg_precision" or "preconditioner_precision" is 32
 */
/* Flag "affine_geometry" (an option of this build, off by default; the reference always streams the six factor
 * arrays): after fddh_problem_set_flag(p, "affine_geometry", 1), which of the operators run on the kernel that forms the
 * factors from six numbers per element (fdd_hip.h: fdd_stiffness_matrix_affine) -- the fine Domain's node-space operator,
 * and how many of the Subdomain's level lists -- and the largest relative deviation of the mesh's own factor arrays
 * from that form (-1 before the flag was ever set).  Any argument may be NULL. */
int fddh_problem_affine_info(fddh_problem *p, int *fine_domain_affine, int *sub_lists_affine, int *sub_lists, double *max_deviation);
/* Flag "skip_zero_factors" (default 1 where the kernel library exports fdd_stiffness_matrix_diag, _diag_f32 and
 * fdd_stiffness_offdiag_zero; setting it to 1 on a library without them is refused, naming the missing entry): a 3-D element
 * list of degree <= 15 whose three off-diagonal factor arrays are 0.0 at every point -- checked once on the device when the
 * list's factor pointers are set; every box and rectilinear mesh -- runs the stiffness kernel that streams three factor arrays
 * instead of six, unless "affine_geometry" has switched it over; a list on the matrix cores (degree 11..15, "mfma_stiffness")
 * takes their three-array instance under "mfma_skip_zero_factors" below and is not counted here.  Unlike "affine_geometry" this
 * leaves the operator's values as they are (the addition of exact zeros is all that is dropped; the sign of a zero may
 * differ), so nothing that hangs on the operator is emptied.  0: six arrays everywhere.
 * The info entry: is the flag on, does the fine Domain's list run that kernel, how many of the Subdomain's level lists do (in
 * the precision in use), of how many.  Any argument may be NULL. */
int fddh_problem_zero_factor_info(fddh_problem *p, int *enabled, int *fine_domain_diag, int *sub_lists_diag, int *sub_lists);
/* Flag "mfma_skip_zero_factors" (default 1 where the kernel library exports fdd_stiffness_matrix_mfma_diag besides the entries
 * above; setting it to 1 on a library without it is refused, naming the missing entry): a list whose off-diagonal factor
 * arrays are zero (the same check) and that runs on the matrix cores runs their three-array instance.  It takes effect only
 * while "skip_zero_factors" and "mfma_stiffness" are both on -- "skip_zero_factors" = 0 goes on meaning six arrays everywhere --
 * and "affine_geometry" keeps precedence.  The values are those of the six-array matrix-core kernel (the sign of a zero may
 * differ), so nothing that hangs on the operator is emptied.  The info entry: is the flag on, does the fine Domain's list run
 * that instance, how many of the Subdomain's level lists do (in the precision in use: none in a float inner solve, which has
 * no matrix-core kernel), of how many.  Any argument may be NULL. */
int fddh_problem_mfma_zero_factor_info(fddh_problem *p, int *enabled, int *fine_domain_mfma_diag, int *sub_lists_mfma_diag, int *sub_lists);
/* Flag "line_stiffness" (default 1 where the kernel library exports fdd_stiffness_matrix_lines and _lines_f32; setting it to 1
 * on a library without them is refused, naming the missing entry): a 3-D list of degree 7 that runs the three-array kernel
 * (see "skip_zero_factors") runs its line form, in both precisions, in the local and the gather form.  The line form gives
 * the bits of the slab form, so histories and iterates do not change with the flag.  Lists that stream six arrays keep the
 * slab form: their line form was built and measured no faster, and is not compiled in.  0: the slab form everywhere.
 * The info entry: is the flag on, does the fine Domain's list run the line form, how many of the Subdomain's level lists do
 * (in the precision in use), of how many.  Any argument may be NULL. */
int fddh_problem_line_stiffness_info(fddh_problem *p, int *enabled, int *fine_domain_lines, int *sub_lists_lines, int *sub_lists);
/* Flag "shared_factor_blocks" (default 1 where the kernel library exports fdd_stiffness_matrix_lines_shared, _lines_shared_f32,
 * fdd_stiffness_factor_block_hash and _factor_block_verify; setting it to 1 on a library without them is refused, naming the
 * missing entry): a list that runs the line form (see "line_stiffness") and whose elements hold, bit for bit, the G[0..2] blocks
 * of a few of them -- a uniform box, a piecewise-uniform grid; established once from the list's own arrays on the device, by
 * hash and then by comparison of every bit; at most 1 MiB of distinct blocks and at most half as many as elements -- reads
 * those few blocks instead of streaming every element's copy, in both precisions, in the local and the gather form.  The
 * words read are the mesh's own, so histories and iterates do not change with the flag.  It takes effect only where the line
 * form runs: "line_stiffness" = 0, "skip_zero_factors" = 0, "affine_geometry" = 1, six-array lists and other degrees keep
 * their meaning.  A deformed mesh shares nothing and keeps the streamed instance.  0: every element streams its own block.
 * The info entry: is the flag on, does the fine Domain's list run the shared instance, how many distinct blocks its check
 * found (0: not looked for), how many of the Subdomain's level lists run it (in the precision in use), of how many.  Any
 * argument may be NULL. */
int fddh_problem_shared_factor_info(fddh_problem *p, int *enabled, int *fine_domain_shared, int *fine_domain_classes, int *sub_lists_shared, int *sub_lists);
/* Flag "lean_line_stiffness" (default 1 where the kernel library exports fdd_stiffness_matrix_lines_lean and _lines_lean_f32;
 * setting it to 1 on a library without them is refused, naming the missing entry): a list that runs the line form (see
 * "line_stiffness"), shared or streamed, runs its lean instance where the derivative table the list uploads has an interior
 * diagonal of +-0.0 and is off that diagonal bit for bit its own negated mirror image (D_hat[63 - m] = -D_hat[m]) -- checked on the host on the
 * very array that is uploaded, at set-up and at every fddh_problem_set_D_hat, the float copy of the single-precision inner
 * solve on its own.  The table of this library's GLL nodes passes in both precisions.  A table that fails keeps the parent
 * instance, silently.  The lean instance leaves out the addition of exact zeros and nothing else (fdd_hip.h): the operator's
 * values are the parent's, to the sign of a zero, so nothing that hangs on the operator is emptied.  It takes effect only
 * where the line form runs.  0: the parent instances everywhere.
 * The info entry: is the flag on, does the fine Domain's table pass the check, does its list run the lean instance, how many
 * of the Subdomain's level lists run it (in the precision in use), of how many.  Any argument may be NULL. */
int fddh_problem_lean_line_info(fddh_problem *p, int *enabled, int *fine_domain_table_ok, int *fine_domain_lean, int *sub_lists_lean, int *sub_lists);
/* Flag "assemble_in_stiffness" (default 1 where the kernel library exports fdd_stiffness_matrix_lines_direct and
 * fdd_csr_plan_gather_mapped; setting it to 1 on a library without them is refused, naming the missing entry): in the
 * Subdomain's operator on dof vectors (Qt A_L Q), the degree-7 line kernel stores the rows of Qt that have one entry, or two
 * from x-neighbours of one workgroup of that kernel, straight into the dof vector, and only the other rows go through the
 * point buffer and a gather of their own.  Which rows those are is read off Qt's own arrays after every set-up.  The sums
 * are the gather's own statements in its order, so histories and iterates do not change with the flag, to the last bit.  It
 * takes effect in a double-precision inner solve on a conforming region with unit norm weights all of whose lists run the line
 * form (shared or streamed, lean or not); everything else keeps its kernels.  0: the point buffer and the whole gather.
 * The info entry: is the flag on; is it in effect now and, if not, why (why_not, a C string of at most why_not_len bytes,
 * empty when in effect); rows[3] = Qt's rows that are general, single, pair; points[5] = the region's points that are
 * general, single, pair-low, pair-high, without a dof; the row blocks of the general rows' plan (0 until that plan is made,
 * which happens where everything else holds).  Any argument may be NULL.  Needs a Subdomain.
 * The arrays entry: the classes themselves, for checks -- point_class_dof (num_points ints: point_dof with the class 0..3
 * in bits 29..30 of the non-negative entries, in the order above) and the general rows as a CSR of their own (ptr:
 * num_rows + 1, col: num_nnz point indices, row_map: num_rows dofs).  Call once for the sizes, again with the arrays. */
int fddh_problem_assembly_info(fddh_problem *p, int *enabled, int *in_effect, long long *rows, long long *points, int *reduced_row_blocks, char *why_not, size_t why_not_len);
int fddh_problem_assembly_arrays(fddh_problem *p, int *num_points, int *num_rows, int *num_nnz, int *point_class_dof, int *ptr, int *col, int *row_map);
int fddh_problem_set_flag(fddh_problem *p, const char *name, int value);

/* Low-order AMG preconditioner of the inner solve (Subdomain::low_order_preconditioner,
 * subdomain.tpp:3987-4159).  The reference builds the hierarchy with HYPRE BoomerAMG
 * (subdomain.tpp:3383-3549); here the caller hands it in, finest level first:
 * A (CSR), the Chebyshev diagonal scaling D_val and coefficients (hypre ds / coefs), and
 * the prolongation P to the next level (null + n_coarse 0 on the coarsest level).  Level 0
 * is numbered by the subdomain's dofs: fddh_problem_sub_point_dofs gives the dof of every
 * level-0 point (-1 on Dirichlet points). */
int fddh_problem_sub_point_dofs(const fddh_problem *p, int *dof, int n);
int fddh_problem_amg_add_level(fddh_problem *p, int n, const int *A_ptr, const int *A_col, const double *A_val, const double *D_val, const double *coefs, int num_coefs, int n_coarse, const int *P_ptr, const int *P_col, const double *P_val);
int fddh_problem_amg_finalize(fddh_problem *p);
int fddh_problem_amg_apply(fddh_problem *p, const double *r, double *z);
/* Or let the host layer build both the low-order FEM matrix (P1 on the 6 tetrahedra of every GLL sub-cell,
 * subdomain.tpp:2823-3060) and this build's own smoothed-aggregation hierarchy for it (HYPRE BoomerAMG's stand-in,
 * subdomain.tpp:3383-3549), and attach it.  coarsest_size / strength <= 0 take the defaults (400 rows, 0.08). */
int fddh_problem_amg_build(fddh_problem *p, int coarsest_size, double strength, int smooth_prolongator, int verbose, int *num_levels);
int fddh_problem_amg_level_info(const fddh_problem *p, int level, int *n, int *nnz_A, int *n_coarse, int *nnz_P);
/* the last hierarchy build (explicit or on first use): on how many of its levels the matrix A was computed on the device
 * ("amg_device_setup": the FEM matrix, the Galerkin products of the lattice levels, the hand-off level's included; 0 for a
 * host build) and its wall time in seconds (0 and 0 before any build).  Either argument may be NULL. */
int fddh_problem_amg_setup_info(const fddh_problem *p, int *levels_built_on_device, double *setup_seconds);
/* 1 where the interpolator of `level` (to level + 1) is applied matrix-free: a geometric level of fddh_problem_amg_build's own
 * hierarchy on a conforming 3-D region with 8 or 16 lattice nodes per direction (fdd_lattice_prolong / _restrict,
 * include/fdd_hip.h), and the flag "amg_matrix_free_transfer" (default 1) on; 0: two SpMVs with the CSR interpolator */
int fddh_problem_amg_level_transfer(const fddh_problem *p, int level, int *matrix_free);
int fddh_problem_amg_level_arrays(const fddh_problem *p, int level, int *A_ptr, int *A_col, double *A_val, double *D_val, double *coefs, int *P_ptr, int *P_col, double *P_val);

/* Domain operations on host vectors of num_local_points */
int fddh_problem_dssum(fddh_problem *p, double *out, const double *in, int apply_mask, int apply_weight);          /* Domain::direct_stiffness_summation */
int fddh_problem_stiffness(fddh_problem *p, double *out, const double *in, int apply_dssum);                       /* Domain::stiffness_matrix */
int fddh_problem_residual_norm(fddh_problem *p, const double *r, double *norm);                                    /* Domain::residual_norm */
int fddh_problem_make_rhs(fddh_problem *p, int function_id, unsigned long long seed, double *u_star, double *f);   /* poisson.cpp:211-219 */
/* u* given on the host (e.g. a seeded vector): u* <- weighted dssum(u*), f = A_L u* */
int fddh_problem_make_rhs_from(fddh_problem *p, double *u_star_inout, double *f);

/* Mass, gradient and weak divergence of fields on the problem's fine mesh (an option of this build; fdd_hip.h: fdd_field_*,
 * where the formulas are): what a caller who solves -laplace(u) = s, or the pressure step of a flow code, needs around the
 * solve.  Host vectors of num_local_points, element-local like every vector of this header; 3-D problems of degree <= 15 (a
 * 2-D problem is refused and stays usable); refused, naming the missing entry, on a kernel library without the fdd_field_*
 * entries.  The opening is that of the fddh_problem_* entries: the calling thread must be the problem's rank.
 *   mass             the diagonal mass matrix B = w_i w_j w_k det J, unassembled: f = B s (point by point) is the right-hand
 *                    side of -laplace(u) = s for fddh_problem_solve
 *   gradient         of u, per element.  average != 0: every component is replaced by its multiplicity-weighted mean over the
 *                    copies of a node (Domain::direct_stiffness_summation without the mask, with the weight), which is
 *                    continuous; collective on several ranks
 *   weak_divergence  out_i = integral of grad(phi_i) . v, unassembled like the f of fddh_problem_make_rhs and handed to
 *                    fddh_problem_solve as it is; weak_divergence(gradient(u)) = fddh_problem_stiffness(u)
 * They read the level's current D_hat (fddh_problem_set_D_hat is followed) and a device copy of the coordinates made at the
 * first call (24 B per point) and freed with the problem.  A non-positive Jacobian is not detected: the generated meshes are
 * checked when they are made; for a mesh read from files, min(mass) > 0 is the caller's check. */
int fddh_field_mass(fddh_problem *p, double *mass);
int fddh_field_gradient(fddh_problem *p, const double *u, double *gx, double *gy, double *gz, int average);
int fddh_field_weak_divergence(fddh_problem *p, const double *vx, const double *vy, const double *vz, double *out);

/* The convection term c . grad u of a velocity c = (cx, cy, cz) and a field u on the same mesh (an option of this build;
 * fdd_hip.h: fdd_field_convect and fdd_field_weak_convect, where the formulas are): the one term of an advection-diffusion
 * or flow step that mass, gradient and weak divergence do not give.  Host vectors of num_local_points as above, the same
 * opening, the same refusals (a 2-D problem, a degree above 15; the problem stays usable), and on a kernel library without
 * the two kernel entries both refuse, naming the first missing one.  A diffusivity that is set is not applied: like
 * fddh_field_*, these are geometry.  They stand outside the fddh_field_* names because that set is the three entries above,
 * every one of which needs the fdd_field_mass family; fddh_convect_quadrature needs no kernel at all.
 *   convect       out = c . grad u at every point (collocated, strong form)
 *   weak_convect  out_i = integral of phi_i (c . grad u) on (3n+1)/2 Gauss-Legendre points per direction, n = N+1 (the 3/2
 *                 rule, which does not alias the product on an affine element), element-local and unassembled like
 *                 weak_divergence and the f of fddh_problem_make_rhs.  Every degree 1..15 has a kernel instance
 *   quadrature    the host tables of that rule: *num_quad = M = (3n+1)/2, z and w (M Gauss-Legendre points and weights), P
 *                 (M x n, P[i + q n] = l_i(z_q): the interpolation from the GLL points) and Pd = P D_hat (the derivative of
 *                 the interpolant at z_q).  Any of the pointers may be NULL (not written); ask for num_quad first.
 * Pd is made from the fine level's current D_hat and made again after fddh_problem_set_D_hat, so both operators follow a
 * changed table as the gradient does. */
int fddh_convect(fddh_problem *p, const double *cx, const double *cy, const double *cz, const double *u, double *out);
int fddh_weak_convect(fddh_problem *p, const double *cx, const double *cy, const double *cz, const double *u, double *out);
int fddh_convect_quadrature(fddh_problem *p, int *num_quad, double *z, double *w, double *P, double *Pd);

/* The inner GMRES's last Arnoldi step of a cycle (flag "last_norm_from_projections", on by default where the kernel library has
 * the entries and refused at 1 where it lacks them; double inner solves with sub_num_vectors < 8 on the dof-space forms): the
 * norm of the step's vector, which nobody reads, is taken as <q, q> - sum h_k^2 where that difference keeps at least 2^-10 of
 * <q, q> (include/fdd_norm_estimate.h), and from the exact pass otherwise.  Counted over the life of the problem's Subdomain:
 * *estimated steps took the difference, *exact fell back, *min_ratio is the smallest difference / <q, q> among them (0 before
 * the first).  Any pointer may be NULL.  A problem without a Subdomain is refused.  One blocking read of the device state. */
int fddh_inner_norm_counters(fddh_problem *p, long long *estimated, long long *exact, double *min_ratio);

/* ---- Helmholtz solves: (-laplace + lambda) u = f (an option of this build; the reference solves the Poisson problem) ----
 * A shift is a constant lambda >= 0 or, lambda_points != NULL, a value >= 0 per point of the fine level (all finite).  It is
 * kept as one node vector, cbar[n] = sum over the copies p of node n of lambda_p * B_p (B: fddh_field_mass; the products in
 * double on the host, summed in the column order of the row of the gather matrix, fddh_problem_csr(1)), which the outer
 * solve adds behind its operator application (q^ += cbar .* p~) and the inner solve, renumbered to its dofs, behind its
 * own; what hangs on the operator follows as said once at fddh_problem_set_flag (operator_changed): a hierarchy built by
 * fddh_problem_amg_build is built again, on the host, with cbar on the diagonal of its level-0 matrix, one that was handed
 * in is not.  An all-zero shift switches the term off: every solve then has the bits it had before a shift was ever set.
 * fddh_problem_solve / _solve_timed / _pcg_* / _precond_apply / _sub_dof_op / _sub_jacobi_diagonal / _sub_dof_solve follow a
 * set shift; the right-hand side of a manufactured solution is stiffness(u*) + lambda B u*, formed by the caller.
 * Refused, the problem staying usable: more than one rank, a composite Subdomain, a 2-D problem, poly_degree > 15, a kernel
 * library without fdd_shift_add / _f32 / _inner_product or fdd_field_mass (naming the entry); and, when it starts, a solve
 * that would not run the node-space outer loops and the dof-space inner operator (point-space outer forms, the inner FCG,
 * assembled_inner_solve = 0, device_bookkeeping = 0), and fddh_problem_solve_projected.
 *   info           whether a shift is set, and the smallest and largest lambda it was made from
 *   shift          cbar on the rank's nodes (zeros when none is set)
 *   node_operator  q^ = (Qt A_L Q + diag(cbar)) v~ on node vectors and vq = <v~, q^>: the launches of the outer flexible CG's
 *                  operator application and of the dot behind it (gather-form stiffness, gather, fused shift-and-dot) */
int fddh_helmholtz_set(fddh_problem *p, double lambda, const double *lambda_points /* NULL: the constant */);
int fddh_helmholtz_info(fddh_problem *p, int *active, double *min, double *max);
int fddh_helmholtz_shift(fddh_problem *p, double *cbar_nodes, int n);
int fddh_helmholtz_node_operator(fddh_problem *p, const double *v_nodes, double *q_nodes, int n, double *vq);

/* ---- Neumann and Robin faces (an option of this build; every problem of the reference is homogeneous Dirichlet) ----
 * A problem made by fddh_problem_create_box_faces knows its faces: the face list is every face of the rank's elements that
 * lies on the surface of the box, sorted by (side, element), side = 2 axis + upper; face f has (N+1)^2 points, point (a, b) at
 * f (N+1)^2 + a + (N+1) b with (a, b) = (j, k) on x-faces, (i, k) on y-faces, (i, j) on z-faces (fdd_hip.h: fdd_field_surface,
 * where the formulas are).  A problem made from mesh files has no face list: faces, surface and robin_set refuse it and say
 * so (which covers every 2-D problem); info answers with empty codes and num_faces = -1.
 *   info       the six codes (faces_out: 7 chars, NUL-terminated), the length of the face list, whether a Robin coefficient
 *              is set and the smallest and largest alpha it was made from, the number of non-zero entries of the node shift
 *              cbar (0 when none is set), the flag "indexed_shift", and in bit 0 / bit 1 whether the outer / the inner
 *              operator adds cbar by fdd_shift_add_indexed as things stand.  Any pointer may be NULL
 *   faces      the list: element (local) and side of every face, m = num_faces
 *   surface    area = w_a w_b |Nvec|, the weight of the surface integral at every face point, and the unit outward normal
 *              (nx, ny, nz all NULL: not computed); count = num_faces (N+1)^2.  Degree <= 15; refused, naming the entry, on
 *              a kernel library without fdd_field_surface.  Works on any rank grid (each rank its own faces)
 *   robin_set  the condition kappa du/dn + alpha u = g on natural faces: alpha per face point, finite and >= 0, and 0 on every
 *              masked point (a positive alpha on a point of a 'D' face is refused, naming the first such point); NULL clears.
 *              The term is diagonal: r[q] = sum of alpha * area over the face entries at point q, in face-list order from
 *              0.0, joins the products of a Helmholtz shift per point -- lambda_q B_q where a lambda is set, else 0.0, then
 *              + r[q] -- and the sums over the copies of a node are cbar as described at fddh_helmholtz_set, with everything
 *              that follows a set shift there (the outer and inner operators, the exact diagonal, the level-0 matrix of a
 *              hierarchy built here, the refusal of fddh_problem_solve_projected).  fddh_helmholtz_info keeps reporting
 *              lambda's range and whether a lambda is set; fddh_helmholtz_shift returns the whole cbar.  The refusals are
 *              those of fddh_helmholtz_set (one rank, a conforming region, 3-D, degree <= 15, the kernel entries); the
 *              problem stays usable.  An all-zero alpha is no coefficient.
 * The data of the conditions go into the right-hand side, formed by the caller (host_api.py: Problem.boundary_rhs):
 * f - A_L u_D - lambda B u_D + scatter(area * flux), the solution being solve(f') + u_D.
 * Flag "indexed_shift" (fddh_problem_set_flag; refused where the kernel library lacks fdd_shift_add_indexed[_f32]): where at
 * most 1/16 of the entries of cbar are non-zero -- a Robin term alone -- the passes that only add the term run over its
 * support; the same values.  Default 1 where the entries are (measured faster: DESIGN section 15).  The fused shift-and-dot of
 * the outer CG step reads both vectors anyway and stays dense.
 * A problem whose faces are all 'N' and that has no zeroth-order term is singular (the constants): it can be created, since a
 * shift may follow, but fddh_problem_solve / _solve_timed / _solve_projected / _pcg_begin / _precond_apply refuse it, naming
 * the remedies. */
int fddh_boundary_info(fddh_problem *p, char *faces_out, int *num_faces, int *robin_active, double *alpha_min, double *alpha_max, long long *shift_support, int *indexed_shift, int *indexed_in_use);
int fddh_boundary_faces(fddh_problem *p, int *elem, int *side, int m);
int fddh_boundary_surface(fddh_problem *p, double *area, double *nx, double *ny, double *nz, long long count);
int fddh_boundary_robin_set(fddh_problem *p, const double *alpha_face_points /* NULL clears */);

/* ---- Variable diffusivity: -div(kappa grad u) + lambda u = f (an option of this build; the reference solves the Poisson problem) ----
 * kappa_points: one double per point of the fine level, element-major like fddh_problem_mesh_array("x"), every value
 * finite and > 0; continuity across elements is not asked for (a jump along element faces is legal).  The local operator
 * becomes D^T [kappa G] D: the scaled factor arrays G'[g][p] = mesh g[g][p] * kappa[p] (one IEEE double product per entry,
 * on the host, all six g) replace the mesh's in the device buffers every stiffness kernel reads; the mesh's own arrays are
 * not written (fddh_problem_mesh_array("g_1".."g_6") keeps returning them), and setting again or clearing (NULL) starts
 * from them.  What is derived from the factor arrays is derived again: the zero-factor, shared-block and (where that option
 * is on) affine verdicts and the float copies where the arrays are rewritten; the rest of what hangs on the operator as said
 * once at fddh_problem_set_flag (operator_changed): a hierarchy built by fddh_problem_amg_build is built again on the host,
 * each tetrahedron of the low-order matrix scaled by the mean of kappa at its four vertices; a hierarchy that was handed in
 * stays.  The projection basis is cleared by every accepted call that sets kappa or clears one that was set;
 * fddh_problem_solve_projected stays allowed.  A Helmholtz shift is independent and keeps the unscaled mass.
 * fddh_problem_stiffness / _make_rhs_from / _solve* / _pcg_* / _precond_apply / _sub_dof_op / _sub_jacobi_diagonal /
 * _sub_dof_solve / _amg_build and fddh_helmholtz_node_operator follow a set kappa; fddh_field_* are geometry and do not.
 * Flag "coefficient_in_kernel" (fddh_problem_set_flag; refused where the kernel library lacks
 * fdd_stiffness_matrix_lines_coef[_f32|_direct]): a 3-D degree-7 list whose UNSCALED factor blocks repeat runs the
 * coefficient instance of the line kernel, which reads the shared unscaled block and kappa and forms the product itself
 * instead of streaming G'; the same bits either way.  Default 1 where the entries are (measured faster: DESIGN section 14).
 * Refused, nothing touched and the problem staying usable: more than one rank, a composite Subdomain, a 2-D problem, n other
 * than the number of fine-level points, a value that is not finite or not > 0 (the first such point is named).
 *   info   whether a kappa is set, its smallest and largest value, and -- as the other fddh_problem_*_info entries count --
 *          whether the fine Domain's list and how many of the Subdomain's lists run the coefficient instance */
int fddh_diffusivity_set(fddh_problem *p, const double *kappa_points /* NULL clears */, int n);
int fddh_diffusivity_info(fddh_problem *p, int *active, double *min, double *max, int *fine_domain_in_kernel, int *sub_lists_in_kernel, int *sub_lists);

/* Outer solve: solver_id 0 = flexible_conjugate_gradient, 1 = generalized_minimum_residual
 * (poisson.cpp:224-231).  history receives the residual norms the reference
 * prints (iteration 0 first). */
int fddh_problem_solve(fddh_problem *p, int solver_id, const double *f, double *u, double *history, int history_cap, int *num_history, int *num_iterations);

/* The same solve with the right-hand side already uploaded and the clock around the device work only (stream
 * synchronised before and after): what bench.py reports as time to tolerance.  u may be NULL. */
int fddh_problem_solve_timed(fddh_problem *p, int solver_id, const double *f, double *u, double *history, int history_cap, int *num_history, int *num_iterations, double *seconds);

/* Successive-right-hand-side projection (an addition of this build; the reference starts every solve from u = 0): a few
 * earlier solutions are kept as an A-orthonormal basis X with their images A_L X, the next solve starts from the A-norm best
 * approximation x0 = X (X^T f), the Krylov solver removes only what is left, and the correction is folded back into the
 * basis (host/projection.hpp).  Opt-in: with capacity 0, the default, nothing changes anywhere.
 *   configure  capacity 0: off, the slabs are freed; 1..16 (FDD_PROJECTION_MAX): slabs allocated, the basis empty.  Another
 *              value is an error naming the argument, and nothing changes.
 *   clear      empties the basis (capacity and slabs stay)
 *   info       capacity, vectors in the basis, restarts so far (a full basis restarts from the solution alone)
 *   basis      host copies of X_k and A_L X_k, k < size (either may be NULL)
 * fddh_problem_solve_projected is fddh_problem_solve from that start value: it stops at the same |r| <= tolerance |f|, a start
 * value that already meets it takes 0 iterations (history = { |f - A x0| }), f = 0 gives u = 0 and stores nothing, and with
 * capacity 0 it is the plain solve.  Every solver option and flag of the plain solve applies.  Collective on several ranks.
 * projection[4] = { |f|, |f - A x0|, basis size used, basis size afterwards } (may be NULL); seconds (may be NULL): the device
 * time as fddh_problem_solve_timed takes it, the projection's own passes included. */
int fddh_problem_projection_configure(fddh_problem *p, int capacity);
int fddh_problem_projection_clear(fddh_problem *p);
int fddh_problem_projection_info(const fddh_problem *p, int *capacity, int *size, long long *restarts);
int fddh_problem_projection_basis(const fddh_problem *p, int k, double *x, double *Ax);
int fddh_problem_solve_projected(fddh_problem *p, int solver_id, const double *f, double *u, double *history, int history_cap, int *num_history, int *num_iterations, double *projection, double *seconds);

/* Subdomain (preconditioner) operations; type 0 = flexible_conjugate_gradient,
 * 1 = generalized_minimum_residual */
int fddh_problem_precond_apply(fddh_problem *p, int type, const double *r, double *z, double *history, int history_cap, int *num_history);
/* op 0 = tree_operator (in: an outer vector of num_local_points; collective on a composite region),
 * 1 = stiffness_matrix, 2 = direct_stiffness_summation; in/out of sub_num_values = [region points | superdomain dofs] */
int fddh_problem_sub_op(fddh_problem *p, int op, const double *in, double *out);
int fddh_problem_sub_residual_norm(fddh_problem *p, const double *r, double *norm);
/* The inner iteration in its dof-space form (host/subdomain.hpp: GMRES on Qt A_L Q over the unique dofs
 * [subdomain regular | interface | superdomain regular], n = FDDH_SUB_NUM_UNIQUE_DOFS):
 * op 0: out = operator(in), both n dofs; op 1: out (n dofs) = the right-hand side the inner solve sees for the outer
 * vector `in` (num_local_points; runs tree_operator: collective on a composite region).  Analysis and tests. */
int fddh_problem_sub_dof_op(fddh_problem *p, int op, const double *in, double *out, int n);
/* the diagonal of that operator over the n unique dofs, as the point-Jacobi option ("sub_use_preconditioner" = 2) uses it */
int fddh_problem_sub_jacobi_diagonal(fddh_problem *p, double *out, int n);
/* out (n dofs) = the configured inner solve (GMRES(m) with the current options, or Chebyshev-Jacobi) applied to the dof-space
 * right-hand side fa, from a zero start.  Analysis and tests, like fddh_problem_sub_dof_op. */
int fddh_problem_sub_dof_solve(fddh_problem *p, const double *fa, double *ua, int n);

/* Chebyshev-Jacobi inner solve (flag "inner_solver" = 1; an addition of this build, off by default): the local
 * problems are answered by the Chebyshev polynomial of order m in D^-1 A for the interval [lower, upper] * lambda, with D the
 * exact diagonal of fddh_problem_sub_jacobi_diagonal and lambda the Rayleigh quotient of D^-1/2 A D^-1/2 after
 * power_iterations steps of the power iteration (each rank on its own region: no communication).  m diagonal scalings and
 * m - 1 operator applications per application, no inner product, no synchronisation; a fixed, linear, symmetric operator.
 * The outer solver's preconditioner_type (set_options) is not looked at while it is on; "preconditioner_precision" 32 runs
 * it on float vectors.  lambda is computed at first use and kept; fddh_problem_set_D_hat and the flag "affine_geometry"
 * drop it together with the diagonal.
 *   configure  order 1..16, 0 < lower < upper, power_iterations 1..10000; defaults 4, 0.1, 1.1, 25.  A new lower or upper keeps
 *              lambda, a new power_iterations drops it.  A bad value is an error and nothing changes.
 *   info       the settings and lambda, which is computed now if it is not there (lambda NULL: not computed)
 * Refused when a solve starts (error return, the problem stays usable): "sub_use_preconditioner" = 1 (Chebyshev around the
 * V-cycle is not built), and a problem whose inner iteration does not run in dof space (2-D, "assembled_inner_solve" = 0). */
int fddh_problem_inner_chebyshev_configure(fddh_problem *p, int order, double lower, double upper, int power_iterations);
int fddh_problem_inner_chebyshev_info(fddh_problem *p, int *order, double *lower, double *upper, double *lambda, int *power_iterations);

/* Average launch time (HIP events on the stream) and algorithmic bytes (12 B per non-zero,
 * 12 B per row, 8 B per column) of the assembly SpMVs of csr_matrix.okl on the problem's matrices:
 * which = 0: Q x (scatter), 1: Qt x (gather). */
int fddh_problem_spmv_time(fddh_problem *p, int which, int iterations, double *avg_us, double *algorithmic_bytes);
/* The solve path's exchanges alone, with the sizes and buffers the solve uses: avg_us[FDDH_COMM_TIME_COUNT],
 * bytes[FDDH_COMM_TIME_COUNT] = { all-reduce of 3 scalars, interface exchange of two prefixes as a dense all-reduce, coarse-level
 * all-gather (total bytes gathered), ring pull (bytes this rank sends), the same interface exchange as grouped sends / receives
 * between the ranks that share nodes (bytes this rank sends: the default path, flag "neighbour_interface_exchange"), ring pull
 * and coarse blocks in one group (bytes this rank sends: the default path, flag "fold_coarse_exchange") }; host wall clock around
 * device synchronisation, after a barrier.  Collective: every rank calls it.  Zeros on one rank / without a composite. */
#define FDDH_COMM_TIME_COUNT 6
int fddh_problem_comm_time(fddh_problem *p, int iterations, double *avg_us, double *bytes);
/* The general CSR case of the same metric: the 27-point trilinear stencil on an m^3 node grid
 * ((3m - 2)^3 non-zeros; m = 225 is the C2 node grid), values and x seeded, y = A x through CSR_Matrix::multiply. */
int fddh_spmv_stencil_time(int m, int iterations, double *avg_us, double *algorithmic_bytes, long long *num_nnz);

/* Stepwise PCG with vectors resident in HBM (what bench.py times): begin sets
 * u = 0, r = f, z = M^-1 r, p = z; each step is one full outer iteration with
 * no stopping test.  last_residual receives ||r|| of the last step. */
int fddh_problem_pcg_begin(fddh_problem *p, const double *f);
int fddh_problem_pcg_steps(fddh_problem *p, int steps, double *last_residual);
int fddh_problem_pcg_solution(fddh_problem *p, double *u);
/* Per-kernel timing with HIP events on the rank's stream (bench.py's roofline
 * object).  collect() synchronises and writes a JSON object
 * {"<kernel family>": {"count": n, "ms": total, "bytes": algorithmic total}}. */
int fddh_profile_enable(int on);
int fddh_profile_only(const char *kernel_key); /* after enable: time only this kernel family (NULL / "": all); two event records per launch cost a few microseconds */
int fddh_profile_collect(char *json, size_t json_len);

int fddh_sync(void);   /* stream synchronise */
int fddh_barrier(void); /* communicator barrier (stream-ordered, then synchronised) */

#ifdef __cplusplus
}
#endif

#endif /* FDD_HOST_H */
