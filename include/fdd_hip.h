/*
 * fdd_hip.h -- C-ABI of libfdd_hip.so: the MI355X (gfx950) kernels of the
 * preconditioned-CG hot path of the SEM Poisson solve, replacing the OCCA
 * launch layer (occa::device / occa::memory / occa::kernel::operator()) of the
 * reference.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - every entry returns int: 0 = ok, >0 = hipError_t, <0 = FDD_ERR_*;
 *     fdd_last_error() gives the text of the last failure on this thread;
 *   - all pointers named like reference kernel arguments are DEVICE pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     kernel entry is asynchronous on it.  Only fdd_memcpy_h2d / _d2h,
 *     fdd_stream_sync and fdd_device_sync block (occa::memory::copyFrom/copyTo
 *     and occa::device::finish semantics);
 *   - the caller owns all buffers, kernels never allocate;
 *   - argument order follows the OKL kernel it replaces, then workspaces,
 *     then `stream`;
 *   - arithmetic is fp64 with int32 indices (csr_matrix.tpp:132-134), compiled
 *     with -ffp-contract=off: element-wise kernels, thread-per-row and
 *     LDS-staged SpMV and the tensor-product kernels keep the reference's
 *     per-output operation order and are bit-identical to the OCCA-Serial
 *     arithmetic; reductions use a different summation tree (tolerance stated
 *     in tests/), and the fp64-MFMA kernels fuse multiply-add.
 *
 * Each entry cites the reference interface it replaces (file:line relative to
 * the reference repository root).
 */
#ifndef FDD_HIP_H
#define FDD_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDD_ERR_INVALID_ARGUMENT (-1)
#define FDD_ERR_UNSUPPORTED (-2)
#define FDD_ERR_NOT_INITIALIZED (-3)

#define FDD_NUM_GEOM_FACTS 6      /* element.hpp:10-12 */
#define FDD_REDUCE_MAX_BLOCKS 2048 /* partial sums any reduction entry may write into its workspace */

/* ------------------------------------------------------------------ */
/* runtime: replaces occa::device / occa::memory (config.hpp:52;        */
/* usage inventory SURVEY.md section 8(b))                              */
/* ------------------------------------------------------------------ */
const char *fdd_version(void);
const char *fdd_last_error(void);
int fdd_device_count(int *count);
int fdd_set_device(int device);                 /* occa::device::setup, poisson.cpp:137 */
int fdd_get_device(int *device);
int fdd_device_name(char *buf, size_t buf_len);
int fdd_malloc(void **ptr, size_t bytes);       /* occa::device::malloc<T>(n) */
int fdd_free(void *ptr);                        /* occa::memory::free() */
/* What the library has handed out and not got back, for tests of ownership (the card's free memory is other processes'
 * too).  Fills the first n of: live fdd_malloc blocks, their bytes, the high-water mark of those bytes since
 * fdd_live_objects_reset_peak, live plans (fdd_csr_plan_create / _f32), live captured graphs (fdd_graph_end_capture), the
 * count of fdd_malloc calls that returned a block, ever.  Process-wide: ranks are threads. */
int fdd_live_objects(long long *out, int n);
int fdd_live_objects_reset_peak(void);
int fdd_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream); /* occa::memory::copyFrom(host): blocking */
int fdd_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream); /* occa::memory::copyTo(host): blocking */
int fdd_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream); /* occa::memory::copyFrom/To(mem): async */
int fdd_fetch_scalars(void *dst, const void *src, size_t bytes, void *stream); /* blocking D2H of <= 4 KiB of reduction results via a pinned staging buffer */
int fdd_memset(void *dst, int value, size_t bytes, void *stream);
int fdd_stream_create(void **stream);           /* cudaStreamCreate, subdomain.tpp:3475 */
int fdd_stream_destroy(void *stream);
int fdd_stream_sync(void *stream);
int fdd_device_sync(void);                      /* occa::device::finish(), timer.tpp:50,59 */
/* hipGraph capture / replay of a launch sequence (cudaGraph of the V-cycle legs,
 * subdomain.tpp:3644-3704, 4021, 4113).  Capture needs a non-default stream. */
int fdd_graph_begin_capture(void *stream);
int fdd_graph_end_capture(void *stream, void **graph_exec);
int fdd_graph_launch(void *graph_exec, void *stream);
int fdd_graph_destroy(void *graph_exec);
int fdd_event_create(void **event);
int fdd_event_destroy(void *event);
int fdd_event_record(void *event, void *stream);
int fdd_event_elapsed_ms(float *ms, void *start, void *stop); /* synchronises on `stop` */

/* ------------------------------------------------------------------ */
/* csr_matrix.okl -- CSR y = A x                                        */
/* ------------------------------------------------------------------ */
/* csr_matrix.okl:5-18  multiply(Au, A_ptr, A_col, A_val, u, n); launched from csr_matrix.tpp:310 */
int fdd_csr_multiply(double *Au, const int *A_ptr, const int *A_col, const double *A_val, const double *u, int n, void *stream);
/* csr_matrix.okl:20-33 multiply_range(..., row_start, row_end) -- row_end INCLUSIVE; csr_matrix.tpp:328 */
int fdd_csr_multiply_range(double *Au, const int *A_ptr, const int *A_col, const double *A_val, const double *u, int row_start, int row_end, void *stream);
/* csr_matrix.okl:35-48 multiply_weight(..., weight, n); csr_matrix.tpp:340 */
int fdd_csr_multiply_weight(double *Au, const int *A_ptr, const int *A_col, const double *A_val, const double *u, const double *weight, int n, void *stream);

/* Planned SpMV: the row partition CSR_Matrix::assemble (csr_matrix.tpp:94-180)
 * can compute once while it still holds the host `ptr` array.  Rows are grouped
 * into blocks of <= FDD_CSR_BLOCK_NNZ non-zeros that one workgroup streams
 * coalesced through LDS; each row is then summed in column order by one lane,
 * which keeps the reference's summation order.  Rows longer than a block are
 * reduced by a whole workgroup (order differs; tolerance in tests/). */
#define FDD_CSR_BLOCK_NNZ 2048
typedef struct fdd_csr_plan fdd_csr_plan;
int fdd_csr_plan_create(fdd_csr_plan **plan, const int *A_ptr_host, int num_rows, int num_cols, int num_nnz);
int fdd_csr_plan_destroy(fdd_csr_plan *plan);
int fdd_csr_plan_num_blocks(const fdd_csr_plan *plan, int *num_blocks);
int fdd_csr_plan_kind(const fdd_csr_plan *plan, int *kind); /* 0 = thread-per-row, 1 = LDS-staged row blocks */
int fdd_csr_plan_pipelined(const fdd_csr_plan *plan, int *pipelined); /* 1: a short-row plan whose SpMV / gather entries run on the persistent, software-pipelined kernel (profile labels) */
/* Tell the plan that every stored value is exactly 1.0 (the boolean gather / scatter matrices Q, Qt,
 * Q_int, ...; CSR_Matrix::assemble checks its host values): the kernels then skip the val array --
 * 1.0*x is x, so results are unchanged and 8 of the 12 bytes per non-zero are not moved.  A plan of either
 * precision (fdd_csr_plan_create_f32: what fdd_csr_plan_gather_cheby_f32 runs on). */
int fdd_csr_plan_set_unit_values(fdd_csr_plan *plan, int unit_values);
/* Give the plan a sliced-ELL copy of the matrix (slices of 64 rows, column-major, padded to the slice's longest row)
 * when that costs at most max_padding times the stored entries and no row exceeds 64 entries: the form for the
 * short, even rows of the AMG levels.  *attached = 1: fdd_csr_plan_multiply / _matvec[_to] / fdd_amg_smooth_* of this
 * plan run on it from now on, same row sums in the same order.  A_ptr_host: host copy of the row pointers; A_ptr,
 * A_col, A_val: the device arrays (A_val double, or float on a plan of fdd_csr_plan_create_f32). */
int fdd_csr_plan_attach_sell(fdd_csr_plan *plan, const int *A_ptr_host, const int *A_ptr, const int *A_col, const void *A_val, double max_padding, int *attached, void *stream);
/* What the attach made: slices of 64 rows (0: none) and how many of them store their columns in the compact form -- entry k of
 * a slice's 64 rows as one base (the smallest of the 64 columns) + a 16-bit offset per row, possible wherever the 64 columns
 * of every slot lie within 65535 of each other (on the lattice-numbered AMG levels they lie within 63): 10 instead of 12
 * bytes per entry, 6 instead of 8 in single precision; the same columns, values and order. */
int fdd_csr_plan_sell_info(const fdd_csr_plan *plan, int *slices, int *compact_slices);
/* weight may be NULL (multiply) or a device vector of num_rows (multiply_weight) */
int fdd_csr_plan_multiply(const fdd_csr_plan *plan, double *Au, const int *A_ptr, const int *A_col, const double *A_val, const double *u, const double *weight, void *stream);

/* ------------------------------------------------------------------ */
/* math.okl -- BLAS-1                                                    */
/* ------------------------------------------------------------------ */
int fdd_set_to_value(double *u, double alpha, int n, int offset, void *stream);                                              /* math.okl:5-11,  math.tpp:48 */
int fdd_invert_vector_elements(double *u, int n, void *stream);                                                              /* math.okl:13-19, math.tpp:54 */
int fdd_vector_vector_addition(double *uv, double alpha, const double *u, double beta, const double *v, int n, void *stream); /* math.okl:21-27, math.tpp:60; uv may alias u or v */
int fdd_vector_scaling(double *au, double alpha, const double *u, int n, void *stream);                                      /* math.okl:29-35, math.tpp:66 */

/* ------------------------------------------------------------------ */
/* domain.okl -- outer solver kernels                                   */
/* ------------------------------------------------------------------ */
/* Reference two-kernel form, one thread per GLL point, global scratch GDu.
 * G / GDu are HOST arrays of device pointers (the reference keeps device
 * pointer tables, domain.tpp:65-67, 221-224).  dim = 2 or 3. */
int fdd_dom_stiffness_matrix_1(double *const GDu[3], const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], int num_points, int poly_degree, int dim, void *stream); /* domain.okl:5-52,  domain.tpp:605 */
int fdd_dom_stiffness_matrix_2(double *Au, const double *const GDu[3], const double *D_hat, int num_points, int poly_degree, int dim, void *stream);                                           /* domain.okl:54-98, domain.tpp:606 */
/* Fused Au = D^T G D u (both passes in one launch, slabs staged in LDS, no
 * global scratch): 64 B/point.  3-D, poly_degree 1..15.  Replaces the pair of
 * launches in Domain::stiffness_matrix (domain.tpp:602-607). */
int fdd_dom_stiffness_matrix(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], int num_elements, int poly_degree, void *stream);

/* The same fused operator on the fp64 matrix cores (v_mfma_f64_16x16x4_f64) for poly_degree 8..15:
 * the six contractions of an element are 16x16x16 products on LDS-staged views, one persistent
 * 1024-lane workgroup per CU, next element prefetched.  MFMA fuses multiply-add, so this entry is
 * NOT bit-identical to the reference arithmetic (agrees to ~1e-15 * max|Au|).  elem_offset as in
 * fdd_sub_stiffness_matrix (NULL => contiguous elements).  Au must not alias u. */
int fdd_stiffness_matrix_mfma(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
int fdd_stiffness_matrix_mfma_gather(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream); /* u[p] = (*v_scale_dev) * v[point_dof[p]] on load (scale may be NULL) */
/* The matrix-core kernel where the three off-diagonal factor arrays G[3..5] are 0.0 at every point of the list (see
 * fdd_stiffness_matrix_diag below, whose argument list this is): they are not read -- entries 3..5 of G are never
 * dereferenced and may be NULL -- and GDu_d = G[d] Du_d.  40 B per point instead of 64 in the local form (point_dof NULL:
 * u = v point by point), 36 instead of 60 in the gather form.  Every output is the IEEE value of fdd_stiffness_matrix_mfma /
 * _mfma_gather on the same input for finite v, bit for bit up to the sign of a zero: only additions of exact zero products
 * are dropped.  v_scale_dev and elem_offset may each be NULL.  poly_degree 8..15, FDD_ERR_UNSUPPORTED otherwise; Au must
 * not alias v. */
int fdd_stiffness_matrix_mfma_diag(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);

int fdd_dom_initialize_arrays(double *u_k, double *r_k, const double *f, int num_points, void *stream); /* domain.okl:100-107, domain.tpp:618,734 */

/* Reductions.  The reference kernels write one partial per 128-thread block
 * and the host sums them after a D2H copy (domain.tpp:916-996).  Here `out`
 * (device) receives the FINAL scalar(s); `ws` is a device workspace of
 * fdd_reduce_workspace_doubles() doubles. */
size_t fdd_reduce_workspace_doubles(void);
int fdd_dom_residual_norm(double *out, double *ws, const double *r_k, const double *QQt_r_k, const double *dirichlet_mask, int num_points, void *stream);                  /* domain.okl:109-138; out[0] = sum r*QQt_r*mask (no sqrt) */
int fdd_dom_projection_inner_products(double *out2, double *ws, const double *z_k, const double *r_k, const double *p_k, const double *q_k, int num_points, void *stream); /* domain.okl:140-184; out2 = {gamma, theta} */
int fdd_dom_inner_product_flexible(double *out, double *ws, const double *r_k, const double *r_kp1, const double *z_k, int num_points, void *stream);                      /* domain.okl:195-224 */
/* The same sum and, from the same three vectors, the NEXT iteration's gamma = <z_k, r_kp1> (the first sum of
 * domain.okl:140-184 one iteration early; fdd_sub_inner_product(p, q) is what is left of that kernel):
 * out2 = {gamma_next, theta}.  Same bits as the two separate entries. */
int fdd_dom_inner_product_flexible_gamma(double *out2, double *ws, const double *r_k, const double *r_kp1, const double *z_k, int num_points, void *stream);
/* fdd_multi_lincomb_limited_dev on z_k's slice [slice_begin, slice_begin + slice_size) (v[k][d] belongs to node slice_begin + d;
 * z_is_zero: the slice is not read) and fdd_dom_inner_product_flexible_gamma over all num_points, in ONE pass: the slice of
 * z_k is formed, stored and entered into the two sums without being read back, and a v[0] that is r_kp1's own slice is read
 * once.  z_k and out2 have the bits of the two separate entries. */
int fdd_dom_lincomb_flexible_gamma(double *out2, double *ws, const double *r_k, const double *r_kp1, double *z_k, int num_points, int slice_begin, int slice_size, int z_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, const double *last_dev, int m, void *stream);
int fdd_dom_inner_product(double *out, double *ws, const double *u_k, const double *v_k, const double *dirichlet_mask, int num_points, void *stream);                      /* domain.okl:235-264 */

int fdd_dom_solution_and_residual_update(double *u_k, double *r_kp1, const double *r_k, const double *p_k, const double *q_k, double alpha_k, int num_points, void *stream); /* domain.okl:186-193, domain.tpp:978 */
int fdd_dom_residual_and_search_update(double *p_k, double *r_k, const double *z_k, const double *r_kp1, double beta_k, int num_points, void *stream);                      /* domain.okl:226-233, domain.tpp:720 */
/* Same updates with the step length taken from device scalars (no host
 * round trip between the dot products and the update):
 *   alpha = num[0] / den[0];   beta = num[0] / den[0]. */
int fdd_dom_solution_and_residual_update_dev(double *u_k, double *r_kp1, const double *r_k, const double *p_k, const double *q_k, const double *alpha_num, const double *alpha_den, int num_points, void *stream);
int fdd_dom_residual_and_search_update_dev(double *p_k, double *r_k, const double *z_k, const double *r_kp1, const double *beta_num, const double *beta_den, int num_points, void *stream);
/* The residual half of fdd_dom_solution_and_residual_update_dev alone, r_kp1 = r_k - alpha q_k over all num_points, and of
 * the values it stores the sum of squares over the slice [slice_begin, slice_begin + slice_size), in ONE pass: out[0] has
 * the bits of fdd_multi_weighted_inner_product_scaled(out, ws, r_kp1 + slice_begin, {r_kp1 + slice_begin}, NULL, 1, NULL,
 * slice_size) run afterwards (its grid, its choice of path by the alignment of r_kp1 + slice_begin, its lanes counted
 * from the slice start), without r_kp1 being read back.  r_kp1 may be r_k. */
int fdd_dom_residual_update_norm2_dev(double *out, double *ws, double *r_kp1, const double *r_k, const double *q_k, const double *alpha_num, const double *alpha_den, int num_points, int slice_begin, int slice_size, void *stream);
/* The solution half of fdd_dom_solution_and_residual_update_dev and fdd_xpby_ratio_dev(p_k, z_k, beta_num, beta_den, p_k)
 * with p_k loaded once: u_k += alpha p_k, then p_k = z_k + beta p_k, both from the old p_k.  Same bits as the two entries.
 * u_k, p_k and z_k are distinct vectors. */
int fdd_dom_solution_direction_update_dev(double *u_k, double *p_k, const double *z_k, const double *alpha_num, const double *alpha_den, const double *beta_num, const double *beta_den, int num_points, void *stream);

/* ------------------------------------------------------------------ */
/* subdomain.okl -- FDD local-solve kernels                             */
/* ------------------------------------------------------------------ */
/* Reference form with per-point indirection (offset / vert / level int arrays,
 * subdomain.tpp:1603-1630).  D_hat_ptr is a HOST array of num_levels device
 * pointers; poly_degree is the HOST table injected as the JIT macro
 * POLY_DEGREE (subdomain.tpp:3886-3890), num_levels <= 16. */
int fdd_sub_stiffness_matrix_1(double *const GDu[3], const double *u, const double *const *D_hat_ptr, const int *offset, const int *vert, const int *level, const int *poly_degree, int num_levels, const double *const G[FDD_NUM_GEOM_FACTS], int num_points, int dim, void *stream); /* subdomain.okl:4-53,   subdomain.tpp:3953 */
int fdd_sub_stiffness_matrix_2(double *Au, const double *const GDu[3], const double *const *D_hat_ptr, const int *offset, const int *vert, const int *level, const int *poly_degree, int num_levels, int num_points, int dim, void *stream);                                           /* subdomain.okl:55-101, subdomain.tpp:3961 */
/* Fused, level-sorted form: one launch per polynomial level over the list of
 * that level's elements; elem_offset[e] (device) is the first point of element
 * e in u / Au / G (NULL => e * (N+1)^3). */
int fdd_sub_stiffness_matrix(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* 2-D form of the fused kernel (the DIM == 2 branches of domain.okl:20-33 and :69-80 in one launch, 40 B/point):
 * elements of (poly_degree+1)^2 points, G[0] = G11, G[1] = G22, G[2] = G12 (the other three are not read);
 * elem_offset as in fdd_sub_stiffness_matrix (nullptr: element e starts at e*(poly_degree+1)^2).  Au may alias u.
 * Bit-identical to fdd_dom_stiffness_matrix_1 + _2 with dim = 2. */
int fdd_stiffness_matrix_2d(double *Au, const double *u, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* The same with the boolean scatter Q of the subdomain fused into the load: u[p] = v[point_dof[p]]
 * (0 where point_dof[p] < 0), v a vector over the subdomain's dofs (Q v then A, subdomain.tpp:3977-3981 + 3942-3967). */
int fdd_sub_stiffness_matrix_gather(double *Au, const double *v, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);

int fdd_sub_inner_product(double *out, double *ws, const double *u, const double *v, int num_values, void *stream);                                                                                  /* subdomain.okl:103-132 */
int fdd_sub_weighted_inner_product(double *out, double *ws, const double *u, const double *v, const double *w, int num_values, void *stream);                                                       /* subdomain.okl:134-163, subdomain.tpp:4302,4508 */
int fdd_sub_projection_inner_products(double *out2, double *ws, const double *z_k, const double *r_k, const double *p_k, const double *q_k, const double *weight, int num_values, void *stream);    /* subdomain.okl:165-209, subdomain.tpp:4526 */
int fdd_sub_search_update_inner_product(double *out, double *ws, const double *r_k, const double *r_kp1, const double *z_k, const double *weight, int num_points, void *stream);                    /* subdomain.okl:229-258, subdomain.tpp:4552 */
int fdd_sub_initialize_arrays(double *u_k, double *r_k, const double *f, int num_values, void *stream);                                                                                             /* subdomain.okl:211-218, subdomain.tpp:4274 */
int fdd_sub_solution_and_residual_update(double *u_k, double *r_kp1, const double *r_k, const double *p_k, const double *q_k, double alpha_k, int num_values, void *stream);                        /* subdomain.okl:220-227, subdomain.tpp:4541 */
int fdd_sub_residual_and_search_update(double *p_k, double *r_k, const double *z_k, const double *r_kp1, double beta_k, int num_values, void *stream);                                              /* subdomain.okl:259-266, subdomain.tpp:4563 */
/* precision-cast copies between outer (EType) and preconditioner (DType) data */
int fdd_sub_copy_f64_f64(double *u, const double *v, int num_points, void *stream); /* subdomain.okl:268-282 with DType=EType=double */
int fdd_sub_copy_f32_f64(float *u, const double *v, int num_points, void *stream);  /* subdomain.okl:268-274, DType=float */
int fdd_sub_copy_f64_f32(double *u, const float *v, int num_points, void *stream);  /* subdomain.okl:276-282, DType=float */
/* degree-tree restriction, reference three-launch form with global intermediates */
int fdd_sub_restriction_1(double *Ju, const double *J_cf, const double *u, int num_points, int n_f, int n_c, int dim, void *stream); /* subdomain.okl:284-313, subdomain.tpp:4593,4601 */
int fdd_sub_restriction_2(double *Ju, const double *J_cf, const double *u, int num_points, int n_f, int n_c, int dim, void *stream); /* subdomain.okl:315-344, subdomain.tpp:4596,4604 */
int fdd_sub_restriction_3(double *Ju, const double *J_cf, const double *u, int num_points, int n_f, int n_c, void *stream);          /* subdomain.okl:346-366, subdomain.tpp:4607 */
/* Fused J^T (x) J^T (x) J^T per element through LDS, 3-D: 8*(n_f^3+n_c^3) B/element */
int fdd_sub_restriction(double *u_c, const double *J_cf, const double *u_f, int num_elements, int n_f, int n_c, void *stream);
/* the `dim == 2` branches of restriction_1 and _2 (subdomain.okl:284-344) in one launch, bit-identical to the pair */
int fdd_sub_restriction_2d(double *u_c, const double *J_cf, const double *u_f, int num_elements, int n_f, int n_c, void *stream);

/* ------------------------------------------------------------------ */
/* AMG/kernels.cu + AMG/csr_matrix.cpp -- Chebyshev-smoothed V-cycle     */
/* ------------------------------------------------------------------ */
int fdd_amg_vector_set_to_value(double *data, double value, int size, void *stream);                                                   /* AMG/kernels.cu:11-23 */
int fdd_amg_main_scaled_residual(double *Sr, double *w, const double *f_m_Au, const double *S, double alpha, int size, void *stream);   /* AMG/kernels.cu:25-41 */
int fdd_amg_main_polynomial_evaluation(double *w, double *v, const double *r, const double *D_val, double alpha, int size, void *stream); /* AMG/kernels.cu:43-59 */
int fdd_amg_main_update_field(double *u, const double *w, const double *D_val, int size, void *stream);                                /* AMG/kernels.cu:61-76 */
int fdd_amg_vector_multiplication(double *uv, const double *u, const double *v, int size, void *stream);                               /* AMG/kernels.cu:79-94 */
/* y = alpha*A*x + beta*y (cusparseSpMV CSR_ALG1 at AMG/csr_matrix.cpp:129-131); y must not alias x */
int fdd_amg_matvec(double *y, const int *ptr, const int *col, const double *val, const double *x, double alpha, double beta, int num_rows, void *stream);
/* the same on a plan (LDS row staging for the ~27 non-zeros per row of the AMG levels) */
int fdd_csr_plan_matvec(const fdd_csr_plan *plan, double *y, const int *A_ptr, const int *A_col, const double *A_val, const double *x, double alpha, double beta, void *stream);
int fdd_csr_plan_matvec_to(const fdd_csr_plan *plan, double *y, const double *y_in, const int *A_ptr, const int *A_col, const double *A_val, const double *x, double alpha, double beta, void *stream); /* y = alpha*A*x + beta*y_in (y_in NULL: y itself): f - A u without first copying f */
/* The Chebyshev smoother (subdomain.tpp:19-83) with its element-wise kernels (AMG/kernels.cu:25-94) fused into the
 * SpMV in front of them, statement for statement the same arithmetic:
 *   residual:    Sr = D*(f - A u);  work = D*(coef*Sr)          [matvec(-1,1) + scaled_residual + vector_multiplication]
 *   polynomial:  work_out = D*(coef*Sr + D*(A work_in))         [matvec(1,0) + polynomial_evaluation + vector_multiplication]
 *   update:      u += D*(coef*Sr + D*(A work_in))               [matvec(1,0) + polynomial_evaluation + update_field]
 *   start:       Sr = D*f;  work = D*(coef*Sr)                  [scaled_residual from u = 0 + vector_multiplication] */
int fdd_amg_smooth_residual_matvec(const fdd_csr_plan *plan, double *work, double *Sr, const int *A_ptr, const int *A_col, const double *A_val, const double *u, const double *f, const double *D_val, double coef, void *stream);
int fdd_amg_smooth_polynomial_matvec(const fdd_csr_plan *plan, double *work_out, const int *A_ptr, const int *A_col, const double *A_val, const double *work_in, const double *Sr, const double *D_val, double coef, void *stream);
int fdd_amg_smooth_update_matvec(const fdd_csr_plan *plan, double *u, const int *A_ptr, const int *A_col, const double *A_val, const double *work_in, const double *Sr, const double *D_val, double coef, void *stream);
int fdd_amg_smooth_start(double *work, double *Sr, const double *f, const double *D_val, double coef, int size, void *stream);

/* ---- matrix-free grid transfer of a geometric AMG level (csrc/fdd_transfer.hip) ------------------------------------
 * Replaces the two SpMVs with the interpolator of a level whose coarse grid is a coarsened GLL lattice (u += P e and
 * f_c = P^T v: the role of P_fem / R_fem, subdomain.tpp:3526-3545, 4064-4068, 4097-4101) where that interpolator is
 * multi-linear in the elements' reference coordinates: the same n x m table of 1-D weights in every element and direction
 * (host/low_order.hpp: geometric_level).  n lattice nodes per direction and element, m kept ones; fine node i sits between
 * kept nodes lo[i] <= hi[i] with weights wl[i] and 1 - wl[i] (lo == hi: a kept node).  lo, hi, wl: HOST arrays of n.
 *   owner_dof[num_elements * n^3]   the fine dof of a lattice point where the point is the first of its dof, -1 elsewhere
 *   coarse_dof[num_elements * m^3]  the coarse dof of an element's kept node (x fastest), -1 on a Dirichlet node
 * prolong: u[dof] += interpolated coarse value, every fine dof once.  restrict: partial[e * m^3 + t] = the element's own
 * weighted sum for its kept node t; the caller adds the partial sums of a coarse dof (a boolean gather over coarse_dof's
 * transpose: fdd_csr_plan_multiply).  The CSR interpolator's operator with its sums in another order: equal to rounding.
 * 3-D; n = 8 and n = 16 are built (fdd_lattice_supported), others are refused. */
int fdd_lattice_supported(int n, int m, int *supported);
int fdd_lattice_prolong(double *u, const double *coarse, const int *owner_dof, const int *coarse_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long num_elements, void *stream);
int fdd_lattice_prolong_f32(float *u, const float *coarse, const int *owner_dof, const int *coarse_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long num_elements, void *stream);
int fdd_lattice_restrict(double *partial, const double *fine, const int *owner_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long num_elements, void *stream);
int fdd_lattice_restrict_f32(float *partial, const float *fine, const int *owner_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long num_elements, void *stream);
/* Float = float (AMG/config.hpp:4, run.py:157): the V-cycle on f32 values and vectors.  Only the fused sequence is
 * provided (SpMV + fused smoother + set/start); casts at the V-cycle's ends: fdd_sub_copy_f32_f64 / _f64_f32.
 * Plans for these entries come from fdd_csr_plan_create_f32 (row blocks whatever the row lengths); the fp64
 * entries refuse such a plan and these refuse an fp64 one. */
int fdd_csr_plan_create_f32(fdd_csr_plan **plan, const int *A_ptr_host, int num_rows, int num_cols, int num_nnz);
int fdd_csr_plan_matvec_to_f32(const fdd_csr_plan *plan, float *y, const float *y_in, const int *A_ptr, const int *A_col, const float *A_val, const float *x, float alpha, float beta, void *stream);
int fdd_amg_smooth_residual_matvec_f32(const fdd_csr_plan *plan, float *work, float *Sr, const int *A_ptr, const int *A_col, const float *A_val, const float *u, const float *f, const float *D_val, float coef, void *stream);
int fdd_amg_smooth_polynomial_matvec_f32(const fdd_csr_plan *plan, float *work_out, const int *A_ptr, const int *A_col, const float *A_val, const float *work_in, const float *Sr, const float *D_val, float coef, void *stream);
/* the update from u = 0 (pre-smoothing): u = 0 + D*(coef*Sr + D*(A work_in)), u not read -- the bits of the update on a zeroed u */
int fdd_amg_smooth_update_matvec_from_zero(const fdd_csr_plan *plan, double *u, const int *A_ptr, const int *A_col, const double *A_val, const double *work_in, const double *Sr, const double *D_val, double coef, void *stream);
int fdd_amg_smooth_update_matvec_from_zero_f32(const fdd_csr_plan *plan, float *u, const int *A_ptr, const int *A_col, const float *A_val, const float *work_in, const float *Sr, const float *D_val, float coef, void *stream);
int fdd_amg_smooth_update_matvec_f32(const fdd_csr_plan *plan, float *u, const int *A_ptr, const int *A_col, const float *A_val, const float *work_in, const float *Sr, const float *D_val, float coef, void *stream);
int fdd_amg_smooth_start_f32(float *work, float *Sr, const float *f, const float *D_val, float coef, int size, void *stream);
int fdd_amg_vector_set_to_value_f32(float *data, float value, int size, void *stream);
/* cublasDdot replacement (AMG/vector.cpp:100,129): out[0] = sum x*y */
int fdd_amg_dot(double *out, double *ws, const double *x, const double *y, int size, void *stream);

/* ------------------------------------------------------------------ */
/* multi-vector forms of the Gram-Schmidt sweep of the Krylov solvers   */
/* (same per-element arithmetic as the launch-per-vector reference       */
/* sequence; vectors are read once)                                      */
/* ------------------------------------------------------------------ */
#define FDD_MULTI_MAX 8
/* doubles per result slot of one Arnoldi step on the device: (j + 1) projections and the norm behind them, j < FDD_MULTI_MAX
 * (the inner solve runs up to FDD_MULTI_MAX steps per cycle: run.py:151-152 sweeps 1, 2, 4, 8) */
#define FDD_GMRES_SLOT (FDD_MULTI_MAX + 2)
/* out[i] = sum a*b[i]*w, i < m <= 8: the (j+1) weighted_inner_product launches of one
 * Arnoldi step (subdomain.tpp:4389-4394).  b is a HOST array of m device pointers. */
int fdd_multi_weighted_inner_product(double *out, double *ws, const double *a, const double *const *b, int m, const double *w, int n, void *stream);
/* q = 1.0*q + coeffs[0]*v[0]; q = 1.0*q + coeffs[1]*v[1]; ... (m <= 8) in one pass: the successive
 * vector_vector_addition launches of domain.tpp:817-822,902-907 / subdomain.tpp:4396-4401,4473-4478.
 * coeffs is a HOST array, v a HOST array of device pointers (none may alias q). */
int fdd_multi_axpy(double *q, const double *coeffs, const double *const *v, int m, int n, void *stream);
/* y += sign * sum_k coeffs_dev[k] * x_k and out[0] = sum y*y*w of the result, one pass, coefficients read
 * from device memory (the output of fdd_multi_weighted_inner_product): Gram-Schmidt update + norm with no
 * host round trip in between (subdomain.tpp:4396-4416). */
int fdd_multi_axpy_norm2_dev(double *out, double *ws, double *y, const double *coeffs_dev, double sign, const double *const *x, int m, const double *w, int n, void *stream);
/* au = (1 / sqrt(*norm2_dev)) * u (subdomain.tpp:4457 with the norm still on the device) */
int fdd_vector_scaling_rsqrt_dev(double *au, const double *norm2_dev, const double *u, int n, void *stream);
int fdd_multi_axpy_dev(double *q, const double *coeffs_dev, const double *const *v, int m, int n, void *stream); /* fdd_multi_axpy, coefficients in device memory */

/* ---- successive-right-hand-side projection (csrc/fdd_projection.hip; an addition of this build, the reference has no
 * counterpart): the passes around an outer solve that starts from the best approximation in the span of earlier solutions
 * (host/projection.hpp).  The basis X and its images AX are one slab each: rows of `ld` doubles, ld even and >= n, base
 * 16-byte aligned; the entries take (base, ld, K) with K <= FDD_PROJECTION_MAX rows in use.  `ws` is the common reduction
 * workspace (fdd_reduce_workspace_doubles()).  Sums are deterministic for given n and K; their order is the kernels' own.
 *   dots   out[k] = sum_i X[k][i] * f[i], k < K, one pass over f.  K == 0 writes nothing, n == 0 writes zeros.
 *   apply  x = x_in + sign_x * sum_k c_k X[k],  b = b_in + sign_b * sum_k c_k AX[k]  (each sum in the order k = 0 .. K - 1,
 *          as fdd_multi_axpy_dev forms it), coefficients read from device memory, one pass: 2K + 2 streams read, 2 written.
 *          nu2_out != NULL: *nu2_out = sum_i x[i] * b[i] of the values just formed.  x_in == NULL: taken as 0 and not read.
 *          x_in == x and b_in == b are allowed (in place).  The start of a solve uses sign_x = +1, sign_b = -1
 *          (x0 = X alpha, f' = f - AX alpha); the basis update uses -1, -1 on (delta, A delta) with the dot.
 *   store  Xk = x / sqrt(*nu2_dev), AXk = b / sqrt(*nu2_dev)  (the factor of fdd_vector_scaling_rsqrt_dev) */
#define FDD_PROJECTION_MAX 16
int fdd_projection_dots(double *out, double *ws, const double *X, int ld, int K, const double *f, int n, void *stream);
int fdd_projection_apply(double *x, double *b, double *nu2_out, double *ws, const double *x_in, const double *b_in, const double *X, const double *AX, int ld, int K, const double *coeffs_dev, double sign_x, double sign_b, int n, void *stream);
int fdd_projection_store(double *Xk, double *AXk, const double *x, const double *b, const double *nu2_dev, int n, void *stream);

/* ---- Chebyshev-Jacobi inner solve (an addition of this build, host/subdomain.hpp chebyshev_dofs): one step of
 * the recurrence as ONE element-wise pass, coefficients by value.
 *   first : t = dinv .* r_in;  d = c_r*t + 0*t;  x = d                                       (q, r_out, c_d not used)
 *   later : r = 1*r_in + (-1)*q;  t = dinv .* r;  d = c_d*d + c_r*t;  x = 1*x + 1*d;  r_out = r   (r_out may be r_in)
 *   last  : d and r_out are not stored (may be NULL where they are not read either).
 * The statements are those of fdd_vector_vector_addition and fdd_vector_diagonal_scaling_dev in that order, so a step
 * composed from those entries has the same bits.  Any n, any alignment (16 bytes per lane where every pointer allows it).
 * fdd_csr_plan_gather_cheby: a later step with q = Qt u formed by the kernel itself, u the point vector and Qt a boolean
 * gather matrix whose plan runs on the persistent pipelined kernel (fdd_csr_plan_pipelined; any other plan is an error):
 * q never goes through memory.  Rows are summed in column order, as fdd_csr_plan_dssum mode 1 sums them: same bits as the
 * gather followed by fdd_cheby_step.  u must not alias x, d or r_out.  Each entry takes a plan of its own precision, as the
 * SpMV entries do: fdd_csr_plan_gather_cheby refuses a plan of fdd_csr_plan_create_f32 and fdd_csr_plan_gather_cheby_f32
 * refuses any other (no value is read; the row blocks of the two plans of one short-row matrix are the same). */
int fdd_cheby_step(double *x, double *d, double *r_out, const double *r_in, const double *q, const double *dinv, double c_d, double c_r, int first, int last, int n, void *stream);
int fdd_cheby_step_f32(float *x, float *d, float *r_out, const float *r_in, const float *q, const float *dinv, float c_d, float c_r, int first, int last, int n, void *stream);
int fdd_csr_plan_gather_cheby(const fdd_csr_plan *plan, double *x, double *d, double *r_out, const int *Qt_ptr, const int *Qt_col, const double *u, const double *r_in, const double *dinv, double c_d, double c_r, int last, void *stream);
int fdd_csr_plan_gather_cheby_f32(const fdd_csr_plan *plan, float *x, float *d, float *r_out, const int *Qt_ptr, const int *Qt_col, const float *u, const float *r_in, const float *dinv, float c_d, float c_r, int last, void *stream);
/* The boolean gather on a selection of Qt's rows: the plan, ptr and col are those of a matrix that holds rows of Qt one after
 * the other (columns still point indices), and row r's sum is stored at y[row_map[r]] (row_map: num_rows ints in device
 * memory); the other words of y are not touched.  The sums are those of fdd_csr_plan_dssum (mode 1), bit for bit.  On the
 * persistent pipelined kernel only, like fdd_csr_plan_gather_cheby: any other plan is FDD_ERR_INVALID_ARGUMENT.  Used with
 * fdd_stiffness_matrix_lines_direct, which completes the rows left out. */
int fdd_csr_plan_gather_mapped(const fdd_csr_plan *plan, double *y, const int *row_map, const int *ptr, const int *col, const double *u, void *stream);

/* Scalar bookkeeping of one restart cycle of the inner flexible GMRES(m) (subdomain.tpp:4396-4477) on the device:
 * Hessenberg column + Givens rotations + residual recurrence + stopping tests per step, back-substitution at the
 * end, so that a cycle is enqueued without a host round trip per step.  `state` = fdd_gmres_state_bytes() bytes of
 * device memory.  A stop is recorded, not acted on: later steps of the cycle run on vectors nobody uses, and
 * fdd_gmres_fetch reports the columns 0..j_last the reference would have used.
 *   begin : gamma[0] = sqrt(*norm2_dev) (also the relative-test norm when first_cycle)
 *   step j: dots_dev[0..j] = <q, v_i>, dots_dev[j+1] = ||q - sum_i h_i v_i||^2
 *   finish: y = H^-1 gamma on columns 0..j_last; fdd_gmres_coefficients gives the device pointer to y[FDD_MULTI_MAX] */
size_t fdd_gmres_state_bytes(void);
int fdd_gmres_begin_dev(void *state, const double *norm2_dev, int first_cycle, void *stream);
int fdd_gmres_step_dev(void *state, const double *dots_dev, int j, int iterations_before, int max_iterations, double tolerance, int use_relative, void *stream);
int fdd_gmres_finish_dev(void *state, int m, void *stream);
int fdd_gmres_fetch(void *state, double *y, double *hist, int *num_hist, int *j_last, int *steps, int *converged, void *stream);
int fdd_gmres_coefficients(void *state, const double **y_dev);
/* the basis may stay unnormalised: inv[0] = 1/gamma_0, inv[j+1] = 1/||q_j|| are kept in the state (the factors
 * vector_scaling would have applied, subdomain.tpp:4358, 4457) for the *_scaled entries below to apply on load */
int fdd_gmres_scales(void *state, const double **inv_dev);
int fdd_gmres_last_column(void *state, const double **j_last_dev); /* device address of j_last (a double), for fdd_multi_lincomb_limited_dev */
int fdd_sub_stiffness_matrix_gather_scaled(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* in the multi-vector reductions below w == NULL means unit weights: nothing is read, and x * 1.0 is x bit for bit */
int fdd_multi_weighted_inner_product_scaled(double *out, double *ws, const double *a, const double *const *b, const double *b_scale_dev, int m, const double *w, int n, void *stream);
int fdd_multi_axpy_norm2_scaled_dev(double *out, double *ws, double *dst, const double *y, const double *coeffs_dev, double sign, const double *const *x, const double *x_scale_dev, int m, const double *w, int n, void *stream); /* dst == NULL (also in the _f32 form): the updated vector is not stored, only its norm is formed -- the last Arnoldi step of a cycle, whose basis vector nobody reads */
/* The last Arnoldi step of a cycle, whose vector nobody reads, with its norm taken from the projections where rounding allows
 * (include/fdd_norm_estimate.h states the function and its bound; double precision only -- a float basis is orthogonal to
 * about 1e-7 and the float entries keep their pass).  m <= FDD_MULTI_MAX - 1 in all three.
 *   _self : out[0..m-1] as fdd_multi_weighted_inner_product_scaled gives them, bit for bit, and out[m] = sum a*a*w (no scale),
 *           from the values the dots load anyway: one launch, one fold
 *   _gated: fdd_multi_axpy_norm2_scaled_dev behind a gate.  dots_dev: the m + 1 sums of _self.  Where the function says the
 *           norm may be taken from them, both launches return at once and out, dst and ws are not written; where it does not,
 *           out and dst have the ungated entry's bits
 *   step  : fdd_gmres_step_dev with dots_dev[0..j] = <q, v_i>, dots_dev[j+1] = <q, q>, dots_dev[j+2] = what _gated wrote if it
 *           ran; asks the same function of the same numbers and takes the norm from the estimate or from dots_dev[j+2].
 *           It counts both outcomes in the state; fdd_gmres_fetch_norm_counters reads the counts and the smallest
 *           est / <q, q> seen (the owner of the state clears its block once, when allocating it) */
int fdd_multi_weighted_inner_product_self(double *out, double *ws, const double *a, const double *const *b, const double *b_scale_dev, int m, const double *w, int n, void *stream);
int fdd_multi_axpy_norm2_scaled_gated_dev(double *out, double *ws, double *dst, const double *y, const double *coeffs_dev, double sign, const double *const *x, const double *x_scale_dev, int m, const double *w, int n, const double *dots_dev, void *stream);
int fdd_gmres_step_last_dev(void *state, const double *dots_dev, int j, int iterations_before, int max_iterations, double tolerance, int use_relative, void *stream);
int fdd_gmres_fetch_norm_counters(void *state, long long *estimated, long long *exact, double *min_ratio, void *stream);
int fdd_multi_axpy_scaled_dev(double *q, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, int m, int n, void *stream);
int fdd_vector_scaling_dev(double *au, const double *scale_dev, const double *u, int n, void *stream); /* au = (*scale_dev) * u */
int fdd_multi_lincomb_scaled_dev(double *q, int q_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, int m, int n, void *stream); /* fdd_multi_axpy_scaled_dev; q_is_zero: q is taken to be 0 and is not read (it need not have been cleared) */
int fdd_multi_lincomb_limited_dev(double *q, int q_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, const double *last_dev, int m, int n, void *stream); /* only vectors 0..(int)*last_dev enter (NULL: all m) */
int fdd_sqrt_sum_dev(double *out, const double *parts_dev, int nparts, void *stream); /* out[0] = sqrt(sum parts): a residual norm appended to a device-side history */
/* ---- single-precision preconditioner (the reference's PTYPE = Float = float, config.hpp:19-20, poisson.cpp:206): the
 * kernels of the dof-space inner solve on float vectors.  Device-resident scalars and reduction accumulators stay double. ---- */
/* The same operator on elements that are AFFINE images of the reference cube (every element of a box mesh), an option of
 * this build: the six factors of a point are formed from six numbers per element and the GLL weights,
 *   G_f(e; i, j, k) = elem_factors[6 e + f] * (w_i w_j) w_k,     gll_weights[0 .. poly_degree],
 * instead of being streamed (48 of the 64 bytes per point of domain.okl:5-98 are not read).  point_dof == NULL: u = v
 * point by point (Domain); otherwise gathered and scaled as above (v_scale_dev may be NULL).  The host layer uses it only
 * where the mesh's own factor arrays have that form to rounding (Stiffness_Operator::affine); results agree with the
 * streamed form to a few ulp of the factors, not bit for bit. */
int fdd_stiffness_matrix_affine(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *elem_factors, const double *gll_weights, const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* the same on the matrix-core kernel (poly_degree 8..15; Au != v) */
int fdd_stiffness_matrix_mfma_affine(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *elem_factors, const double *gll_weights, const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* Do the factor arrays have that form?  Per element e of the list: elem_factors[6 e + f] = G_f / W at the element's middle
 * point, deviation[e] = max over points and factors of |G_f(p) - elem_factors[6 e + f] W(p)| / (max_f |elem_factors| W(p)),
 * W(p) = (w_i w_j) w_k.  3-D elements. */
int fdd_stiffness_affine_detect(double *elem_factors, double *deviation, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const double *gll_weights, int num_elements, int poly_degree, void *stream);
/* The fused kernel where the three off-diagonal factor arrays G[3..5] are 0.0 at every point of the list (every mesh whose
 * elements have orthogonal axes: boxes, rectilinear grids): they are not read -- G is still the six-pointer array, entries
 * 3..5 are never dereferenced -- and GDu_d = G[d] Du_d.  36 B per point instead of 60 in the gather form (20 instead of 32
 * in float), 40 instead of 64 in the local form.  What is dropped is the addition of exact zeros: every output is the IEEE
 * value of the six-array entries for finite v, bit for bit up to the sign of a zero.  v_scale_dev, point_dof and elem_offset
 * may each be NULL, as for fdd_stiffness_matrix_affine.  poly_degree 1..15, FDD_ERR_UNSUPPORTED above. */
int fdd_stiffness_matrix_diag(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
int fdd_stiffness_matrix_diag_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* The line form of the same kernel for poly_degree 7 (an element is one wavefront; a lane owns a whole x-row, y-column and
 * z-column of it in turn and contracts each in registers, LDS only transposes between the three): the argument list of
 * fdd_stiffness_matrix_diag plus diag.  diag = 1: three factor arrays, G[3..5] never dereferenced, every output bit for bit
 * that of fdd_stiffness_matrix_diag[_f32] (signs of zeros included).  diag = 0 (six arrays): that form measured no faster
 * than fdd_sub_stiffness_matrix_gather_scaled[_f32] and is not compiled in: FDD_ERR_UNSUPPORTED, as for every poly_degree
 * other than 7; the output is not touched then. */
int fdd_stiffness_matrix_lines(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, int diag, void *stream);
int fdd_stiffness_matrix_lines_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, int diag, void *stream);
/* Are they?  One pass over G[3], G[4], G[5] on the points of the list (3-D elements): flags_out (three ints in device
 * memory) [f] = 0 exactly when every value of G[3 + f] there compares == 0.0 (-0.0 does; a denormal or a NaN does not),
 * 1 otherwise. */
int fdd_stiffness_offdiag_zero(int *flags_out, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* The line form where factor blocks repeat from element to element (a uniform box: every element's (N+1)^3 values of each
 * array are bit for bit those of element 0): the argument list of fdd_stiffness_matrix_lines plus factor_elem, num_elements
 * ints in device memory, each in 0..num_elements-1.  Element e reads its three factor lines from the block of element
 * factor_elem[e] of the same arrays (at elem_offset[factor_elem[e]], or factor_elem[e] (N+1)^3 where elem_offset is NULL), with
 * plain loads, so that the few blocks named stay in cache: 12 B per point + the gathered values instead of 36 (8 instead of
 * 20 in float; 16 instead of 40 in the local form).  v, point_dof and Au keep the element's own offset.  Where the block
 * named holds the element's own words -- fdd_stiffness_factor_block_verify says whether it does -- every output bit is that
 * of fdd_stiffness_matrix_lines[_f32].  poly_degree 7 and diag = 1 only: FDD_ERR_UNSUPPORTED otherwise, output untouched. */
int fdd_stiffness_matrix_lines_shared(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream);
int fdd_stiffness_matrix_lines_shared_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream);
/* The lean instances of the line form, for a D_hat of which the CALLER guarantees, bit for bit: D_hat[i + 8 i] is +-0.0 for
 * i = 1..6 (the interior diagonal, either sign), and D_hat[63 - m] has the bits of -D_hat[m] for every other m in 0..63 (the
 * table of GLL nodes that mirror exactly; the entry does not check).  The argument list of fdd_stiffness_matrix_lines_shared, with factor_elem allowed
 * to be NULL: NULL means streamed factors (every element reads its own block), otherwise the shared instance as above.  The
 * kernel leaves out the products with the interior diagonal and starts every partial sum from its first product instead of
 * 0 +; the double entry also reads D_hat once per wavefront (the 29 entries of rows 0..3 off the diagonal; the others are used
 * as the negation of their mirror image, D_hat[32..63] and the diagonal are never read), the float entry reads the rows as
 * the parent does and relies on the first condition only.
 * The order of the remaining terms is that of the parent.  What is dropped is only the addition of
 * exact zeros, the caveat fdd_stiffness_matrix_diag carries: for finite inputs every output is the value of
 * fdd_stiffness_matrix_lines[_shared][_f32], bit for bit up to the sign of a zero.  poly_degree 7 and diag = 1 only:
 * FDD_ERR_UNSUPPORTED otherwise, output untouched. */
int fdd_stiffness_matrix_lines_lean(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream);
int fdd_stiffness_matrix_lines_lean_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, int diag, void *stream);
/* The line form that also assembles: y = Qt Au for most rows of the boolean gather Qt (points -> dofs) without the round trip
 * through the point buffer.  point_class_dof is point_dof with the class of the point in bits 29..30 of every non-negative
 * entry (so dofs below 2^29; a negative entry is a point without a dof, as in point_dof), the class being what Qt's own
 * arrays say about the row of the point's dof:
 *   0 general    the value goes to the point buffer Au as in fdd_stiffness_matrix_lines, for a gather of those rows
 *                (fdd_csr_plan_gather_mapped on the compacted rows);
 *   1 single     the row's only entry: y[dof] = 0 + value;
 *   2 pair-low   point (7, j, k) of list element e, the first of the row's two entries;
 *   3 pair-high  point (0, j, k) of list element e + 1, the second, with e / 4 == (e + 1) / 4 (the two elements are waves of
 *                one workgroup): y[dof] = (0 + value of the pair-low point) + value.
 * These are the gather's own statements in column order, so every word of y written here has the bits fdd_csr_plan_dssum
 * (mode 1) writes after fdd_stiffness_matrix_lines[_shared|_lean] on the same inputs; the points of class 0 hold the same
 * bits in Au, the other points of Au are not written.  The CALLER guarantees the classes (the entry cannot check them) and
 * that every row of y is completed exactly once by this entry and the gather of the general rows together.  Which instance:
 * lean != 0: that of fdd_stiffness_matrix_lines_lean (with its condition on D_hat; factor_elem may be NULL), else that of
 * fdd_stiffness_matrix_lines_shared where factor_elem is given and of fdd_stiffness_matrix_lines where it is NULL.  Double
 * only.  Refuses what those entries refuse (poly_degree other than 7, diag other than 1: FDD_ERR_UNSUPPORTED), before any
 * output is touched.  FDD_TUNE_ASSEMBLE_NT_STORE=1: non-temporal stores of y (default 0). */
int fdd_stiffness_matrix_lines_direct(double *Au, double *y, const double *v, const double *v_scale_dev, const int *point_class_dof, const double *D_hat, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int lean, int num_elements, int poly_degree, int diag, void *stream);
/* The coefficient instances of the line form: the operator D^T [kappa G] D on a list whose UNSCALED factor blocks repeat,
 * kappa one double per point, without streaming the scaled arrays kappa G.  blocks: a HOST array of three device pointers
 * to the distinct unscaled blocks of G[0], G[1], G[2] in compact form (block c starts at c * 512 doubles);
 * block_of_elem[e] (device ints): the block of element e, in any order; coef: one double per point, read at the element's
 * own offset (elem_offset[e], or e * 512 where elem_offset is NULL), three times per element -- once in each role of the
 * lane -- of which the second and third are expected to come from cache: 8 B per point beside the 12 of the shared instance
 * (derived, not measured).  Per point and array the kernel forms g = coef * block as one IEEE double product, the
 * statement G'[g][p] = G[g][p] * kappa[p] of the caller that makes the scaled arrays; coef and blocks are double in both
 * precisions and the float entry rounds the double product once, to the float cast of G'.  Everything else is the body of
 * fdd_stiffness_matrix_lines[_f32]: every output bit is that entry's on G' (lean != 0: fdd_stiffness_matrix_lines_lean's,
 * with its condition on D_hat and up to the sign of a zero).  point_dof NULL: the local form.  _direct: the arguments and
 * the classes of fdd_stiffness_matrix_lines_direct.  Refused before anything is touched, the degree first: poly_degree
 * other than 7 and diag other than 1 (FDD_ERR_UNSUPPORTED); a NULL coef, blocks, blocks[g] or block_of_elem; an output
 * (Au, y) that is one of the inputs, or an input that starts inside the points of Au where elem_offset is NULL
 * (FDD_ERR_INVALID_ARGUMENT): Au may NOT alias v here. */
int fdd_stiffness_matrix_lines_coef(double *Au, const double *v, const double *v_scale_dev, const int *point_dof, const double *D_hat, const double *coef, const double *const blocks[3], const int *block_of_elem, const int *elem_offset, int lean, int num_elements, int poly_degree, int diag, void *stream);
int fdd_stiffness_matrix_lines_coef_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const double *coef, const double *const blocks[3], const int *block_of_elem, const int *elem_offset, int lean, int num_elements, int poly_degree, int diag, void *stream);
int fdd_stiffness_matrix_lines_coef_direct(double *Au, double *y, const double *v, const double *v_scale_dev, const int *point_class_dof, const double *D_hat, const double *coef, const double *const blocks[3], const int *block_of_elem, const int *elem_offset, int lean, int num_elements, int poly_degree, int diag, void *stream);
/* Which blocks repeat?  out[e] (num_elements 64-bit words in device memory) = a hash of the bit patterns of element e's block
 * of G[0], G[1], G[2] that depends on the position of every word: equal blocks give equal hashes, and two blocks that differ
 * in a single word give different ones.  3-D elements, poly_degree 1..15. */
int fdd_stiffness_factor_block_hash(unsigned long long *out, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
/* *mismatches (one int in device memory, cleared by the entry) = the number of elements e whose block differs from the block
 * of element factor_elem[e] in any bit of any of the three arrays (-0.0 differs from 0.0, NaN payloads count), or whose
 * factor_elem[e] lies outside 0..num_elements-1.  0: the map is safe to hand to fdd_stiffness_matrix_lines_shared[_f32]. */
int fdd_stiffness_factor_block_verify(int *mismatches, const double *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, const int *factor_elem, int num_elements, int poly_degree, void *stream);
/* The halves the stiffness operator is made of, as entries of their own (an option of this build; csrc/fdd_field.hip), and the
 * diagonal mass matrix.  3-D, double, elements contiguous (element e starts at e (N+1)^3); xyz, grad and v are HOST arrays
 * of three device pointers (the coordinates of the points; the components).  With D[i][p] = D_hat[p + i n], per point:
 *   J[a][b] = dX_a / dr_b   D_hat applied to x, y, z along r, s, t;  I = J^-1 by cofactors over det J
 *   mass    = w_i w_j w_k det J                                      (gll_weights: the n weights)
 *   grad_a  = sum_b du/dr_b I[b][a]
 *   out     = D_r^T F_r + D_s^T F_s + D_t^T F_t,  F_b = mass sum_a I[b][a] v_a:  the weak divergence, integral of
 *             grad(phi) . v against every basis function phi, element-local and unassembled like mass and grad, so that
 *             weak_divergence(gradient(u)) is the stiffness operator's Au
 * The metric is formed in the kernel, no array holds it: 32 (mass), 56 (gradient) and 56 (weak divergence) B per point.
 * A non-positive det J is not detected.  poly_degree 1..15, FDD_ERR_UNSUPPORTED otherwise; num_elements < 2^31 / (N+1)^3;
 * no output may be one of the inputs or another output (equal pointers: FDD_ERR_INVALID_ARGUMENT).  A call that is refused
 * touches no output; num_elements = 0 does nothing. */
int fdd_field_mass(double *mass, const double *const xyz[3], const double *D_hat, const double *gll_weights, int num_elements, int poly_degree, void *stream);
int fdd_field_gradient(double *const grad[3], const double *u, const double *const xyz[3], const double *D_hat, int num_elements, int poly_degree, void *stream);
int fdd_field_weak_divergence(double *out, const double *const v[3], const double *const xyz[3], const double *D_hat, const double *gll_weights, int num_elements, int poly_degree, void *stream);
/* The convection term c . grad u on the same mesh, pointwise and as an over-integrated weak form (an option of this build;
 * csrc/fdd_field.hip).  c is a HOST array of three device pointers (the components of the velocity at the points); the
 * notation is that of the block above, C = adj J.  Per point of the GLL grid:
 *   chat_b  = sum_a C[b][a] c_a                        the velocity in reference space times det J; no division
 *   convect       out = (sum_b chat_b du/dr_b) / det J     = c . grad u at the point: the strong form, one division a point
 * The weak form integrates on M = (3n + 1) / 2 (integer division) Gauss-Legendre points zeta_q per direction with weights
 * omega_q (gl_weights), the 3/2 rule: P[q][i] = P[i + q n] = l_i(zeta_q) interpolates from the GLL points to them (M x n),
 * Pd = P D is the derivative of the interpolant there.  Per fine point q = (q_r, q_s, q_t):
 *   chat_b(q) = (P x P x P) chat_b                     the GLL-point values of chat_b, interpolated
 *   u,_r(q)   = (P_t x P_s x Pd_r) u,  u,_s and u,_t likewise with Pd in the s / t slot
 *   s(q)      = omega_qr omega_qs omega_qt sum_b chat_b(q) u,_b(q)
 *   weak_convect  out = (P^T x P^T x P^T) s            element-local and unassembled like the weak divergence
 * det J cancels: the weak form divides nowhere.  On an element with an affine map this is the integral of phi_i (c_h . grad
 * u_h) exactly for c_h, u_h of degree N (the integrand has degree 3N per direction, the rule is exact to 2M - 1 >= 3N).  On
 * a deformed element chat_b has degree 3N and is represented by its GLL interpolant: the aliasing of the geometry that
 * Nek5000's set_convect_new accepts too.  A non-positive det J is not detected.  56 B read and 8 B written per point.
 * poly_degree 1..15, checked first (FDD_ERR_UNSUPPORTED otherwise); num_quad must be (3n + 1) / 2; num_elements <
 * 2^31 / (N+1)^3; out may be none of the inputs; a call that is refused touches nothing; num_elements = 0 does nothing. */
int fdd_field_convect(double *out, const double *const c[3], const double *u, const double *const xyz[3], const double *D_hat, int num_elements, int poly_degree, void *stream);
int fdd_field_weak_convect(double *out, const double *const c[3], const double *u, const double *const xyz[3], const double *D_hat, const double *P, const double *Pd, const double *gl_weights, int num_quad, int num_elements, int poly_degree, void *stream);
/* The zeroth-order term of -laplace(u) + lambda u on assembled vectors (an option of this build; csrc/fdd_helmholtz.hip):
 *   y[i] = y[i] + c[i] * x[i]          x[i] standing for (*scale_dev) * x[i] where scale_dev is given (the _f32 entry rounds
 *                                      the factor to float first, as fdd_vector_scaling_dev_f32 does)
 * behind the operator application that formed y; multiply, then add, at every width.  The inner-product entry stores the
 * same update and returns sum x[i] * y_new[i] through the reduction workspace (fdd_reduce_workspace_doubles): what
 * fdd_sub_inner_product(x, y) would read back.  16-byte lanes where y, c and x are all 16-byte aligned, one element per
 * lane otherwise; deterministic for given n and alignment.  y must overlap neither c nor x (FDD_ERR_INVALID_ARGUMENT);
 * a call that is refused touches no output; n = 0 stores nothing (the sum is 0). */
int fdd_shift_add(double *y, const double *c, const double *scale_dev, const double *x, int n, void *stream);
int fdd_shift_add_f32(float *y, const float *c, const double *scale_dev, const float *x, int n, void *stream);
int fdd_shift_add_inner_product(double *out, double *ws, double *y, const double *c, const double *x, int n, void *stream);
/* The same statement on the support of a c that is zero on most of the vector (a Robin term lives on the boundary nodes):
 *   y[index[k]] = y[index[k]] + c_values[k] * x[index[k]],  k < m        x standing for (*scale_dev) * x as above
 * index: m distinct, ascending ints in 0..n-1 (device memory); nothing else of y is touched, so where the dense entry's
 * y + 0 * x turns a -0.0 into +0.0 this one leaves it.  On the support the bits are the dense entry's.  An index outside
 * 0..n-1 is skipped.  m <= n; y must overlap neither c_values, index nor x (FDD_ERR_INVALID_ARGUMENT); a call that is
 * refused touches no output; m = 0 does nothing. */
int fdd_shift_add_indexed(double *y, const double *c_values, const int *index, int m, const double *scale_dev, const double *x, int n, void *stream);
int fdd_shift_add_indexed_f32(float *y, const float *c_values, const int *index, int m, const double *scale_dev, const float *x, int n, void *stream);
/* Surface weights and unit normals of listed element faces (an option of this build; csrc/fdd_field.hip).  Face f of the list
 * is side face_side[f] = 2 axis + upper (0..5: r-, r+, s-, s+, t-, t+) of element face_elem[f] (device arrays of num_faces
 * ints, which the CALLER validates: a face whose element or side is out of range is skipped, its outputs stay).  Its n^2
 * points are stored at f n^2 + a + n b with (a, b) = (j, k) on r-faces, (i, k) on s-faces, (i, j) on t-faces.  With X_r, X_s,
 * X_t the derivatives of (x, y, z) along the in-face directions (D_hat applied to the face's own points):
 *   Nvec   = X_s x X_t on r-faces, X_t x X_r on s-faces, X_r x X_s on t-faces
 *   area   = w_a w_b |Nvec|                         the quadrature weight of the surface integral over the face
 *   normal = +- Nvec / |Nvec|, + on the upper side  outward where det J > 0; normal may be NULL (not computed)
 * area and normal[0..2] have num_faces n^2 entries; xyz and normal are HOST arrays of three device pointers.
 * poly_degree 1..15 (checked first), FDD_ERR_UNSUPPORTED otherwise; num_elements < 2^31 / (N+1)^3, num_faces < 2^31 / (N+1)^2;
 * no output may be an input or another output; a refused call touches nothing; num_faces = 0 does nothing. */
int fdd_field_surface(double *area, double *const normal[3], const double *const xyz[3], const double *D_hat, const double *gll_weights, const int *face_elem, const int *face_side, int num_faces, int num_elements, int poly_degree, void *stream);
int fdd_stiffness_matrix_affine_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *elem_factors, const float *gll_weights, const int *elem_offset, int num_elements, int poly_degree, void *stream);
int fdd_sub_stiffness_matrix_gather_scaled_f32(float *Au, const float *v, const double *v_scale_dev, const int *point_dof, const float *D_hat, const float *const G[FDD_NUM_GEOM_FACTS], const int *elem_offset, int num_elements, int poly_degree, void *stream);
int fdd_multi_inner_product_scaled_f32(double *out, double *ws, const float *a, const float *const *b, const double *b_scale_dev, int m, int n, void *stream); /* out[k] = sum a * (s_k b_k), k < m <= 8 */
int fdd_multi_axpy_norm2_scaled_dev_f32(double *out, double *ws, float *dst, const float *y, const double *coeffs_dev, double sign, const float *const *x, const double *x_scale_dev, int m, int n, void *stream); /* dst = y + sign sum c_k (s_k x_k); out = |dst|^2 */
int fdd_vector_scaling_dev_f32(float *au, const double *scale_dev, const float *u, int n, void *stream);
/* z = d .* ((*scale_dev) * u), scale_dev NULL: z = d .* u.  The point-Jacobi preconditioner of the inner solve (a labelled
 * option of this build, host/subdomain.hpp) on a Krylov vector kept unnormalised: math.okl:29-35, then
 * AMG/kernels.cu:64-73 (vector_multiplication), in that order */
int fdd_vector_diagonal_scaling_dev(double *z, const double *d, const double *scale_dev, const double *u, int n, void *stream);
int fdd_vector_diagonal_scaling_dev_f32(float *z, const float *d, const double *scale_dev, const float *u, int n, void *stream);
int fdd_vector_vector_addition_f32(float *uv, float alpha, const float *u, float beta, const float *v, int n, void *stream);
int fdd_multi_lincomb_limited_dev_f32(float *q, int q_is_zero, const double *coeffs_dev, const float *const *v, const double *v_scale_dev, const double *last_dev, int m, int n, void *stream); /* q (+)= sum_{k <= *last} c_k (s_k v_k); last_dev NULL: all m */
int fdd_gather_rows_f32(float *t, const int *ptr, const int *col, const float *u, int row_lo, int row_hi, void *stream); /* t[row] = sum of u over the row's entries (boolean gather) */
/* fdd_gather_rows_f32 on the row blocks of a plan (LDS-staged, coalesced index stream): same sums in the same order */
int fdd_csr_plan_gather_f32(const fdd_csr_plan *plan, float *t, const int *ptr, const int *col, const float *u, int row_lo, int row_hi, void *stream);
int fdd_gather_indexed_f32(float *out, const float *in, const int *index, int n, void *stream);         /* out[i] = in[index[i]], 0 where index[i] < 0 */
int fdd_gather_indexed_f32_f64(double *out, const float *in, const int *index, int n, void *stream);    /* the same, cast up (subdomain.okl:276-282 at the solve's exit) */
int fdd_xmay_ratio_dev(double *out, const double *x, const double *num_dev, const double *den_dev, const double *y, int n, void *stream); /* out = x - (*num / *den) * y (domain.okl:191: r+ = r - alpha q with alpha on the device; out may be x) */
int fdd_xpby_ratio_dev(double *out, const double *x, const double *num_dev, const double *den_dev, const double *y, int n, void *stream); /* out = x + (*num / *den) * y (domain.okl:226: p = z + beta p; out may be y) */
/* out[0] = sum_nodes s*s*w with s = (Qt u)[node]*w[node]: Subdomain::residual_norm
 * (subdomain.tpp:4491-4515: multiply_weight + weighted_inner_product) without the dof vector */
int fdd_gather_weighted_norm2(double *out, double *ws, const int *Qt_ptr, const int *Qt_col, const double *u, const double *node_weight, int num_nodes, void *stream);

/* ------------------------------------------------------------------ */
/* fused direct-stiffness summation (gather-scatter)                    */
/* ------------------------------------------------------------------ */
/* direct_stiffness_summation (domain.tpp:582-600, subdomain.tpp:3969-3985) is
 *   t = (Qt u) .* node_weight ; [gs_add on the boundary prefix] ; out = (Q t) .* point_mask
 * with boolean Qt (all values 1.0) and Q = Qt^T.  One lane per assembled node
 * gathers its points and scatters the sum back: ~36 B/point instead of two
 * SpMVs (66-74 B/point), same arithmetic, bit-identical.  node_weight /
 * point_mask / t may be NULL.  QQtu may alias u.  Nodes [node_start, node_end). */
int fdd_dssum_fused(double *QQtu, double *t, const int *Qt_ptr, const int *Qt_col, const double *u, const double *node_weight, const double *point_mask, int node_start, int node_end, void *stream);
int fdd_dssum_gather(double *t, const int *Qt_ptr, const int *Qt_col, const double *u, const double *node_weight, int node_start, int node_end, void *stream);      /* t = (Qt u) .* w on a node range */
int fdd_dssum_scatter(double *QQtu, const double *t, const int *Qt_ptr, const int *Qt_col, const double *point_mask, int node_start, int node_end, void *stream);  /* out = (Q t) .* mask on a node range */
int fdd_fill_indexed(double *out, const int *idx, double value, int n, void *stream); /* out[idx[i]] = value (points without a dof) */
int fdd_gather_indexed(double *out, const double *in, const int *index, const double *scale, int n, void *stream); /* out[i] = in[index[i]] * scale[i] (0 where index[i] < 0; scale may be NULL) */
/* The same (no scale) from a vector whose head [0, split) lives in `lo` and whose tail lives in `hi` (indexed by the
 * same, unshifted index): out[i] = (index[i] < split ? lo : hi)[index[i]].  Packs the ring data of tree_operator's
 * pull (subdomain.tpp:4626) from the caller's level-0 vector and the restricted levels without copying the former. */
int fdd_gather_indexed_split(double *out, const double *lo, const double *hi, int split, const int *index, int n, void *stream);
/* y[index[i]] += t[i], distinct indices: the result of a transposed SpMV whose non-empty rows are few, added into the
 * full vector (the hanging-point rows S^T of the composite region, subdomain.tpp:1522-1578 transposed). */
int fdd_scatter_add_indexed(double *y, const int *index, const double *t, int n, void *stream);
int fdd_scatter_add_indexed_f32(float *y, const int *index, const float *t, int n, void *stream);
/* The same three operations on the row blocks of Qt's SpMV plan (unit-value plans only): entries are
 * staged through LDS so that no global access depends on a row length.  mode 0 = gather + scatter,
 * 1 = gather only (t out), 2 = scatter only (t in); nodes [row_lo, row_hi).  Same bits as above. */
int fdd_csr_plan_dssum(const fdd_csr_plan *plan, double *QQtu, double *t, const int *Qt_ptr, const int *Qt_col, const double *u, const double *node_weight, const double *point_mask, int row_lo, int row_hi, int mode, void *stream);
int fdd_csr_plan_gather_weighted_norm2(const fdd_csr_plan *plan, double *out, double *ws, const int *Qt_ptr, const int *Qt_col, const double *u, const double *node_weight, void *stream);

/* ------------------------------------------------------------------ */
/* interface exchange helpers: gslib gs(gs_add) on the boundary-node    */
/* prefix (domain.tpp:590-594) becomes pack -> all-reduce -> unpack on a */
/* dense interface-slot vector                                           */
/* ------------------------------------------------------------------ */
int fdd_interface_pack(double *slots, const int *slot_of, const double *prefix, int n, void *stream);   /* slots[slot_of[i]] = prefix[i]; slot_of is injective */
int fdd_interface_unpack(double *prefix, const double *slots, const int *slot_of, int n, void *stream); /* prefix[i] = slots[slot_of[i]] */
/* neighbour form of gs(gs_add) (domain.tpp:590-594) for point-to-point links: buf[i*nc + c] = {a, b}[c][index[i]] (nc = b ? 2 : 1) fills the
 * own copies and the parts sent to the peers; after the grouped send / receive, {a, b}[c][r] = sum_k buf[col[k]*nc + c] over ptr[r] <= k < ptr[r+1],
 * in the order of col (ascending rank of the contributor) */
int fdd_interface_gather(double *buf, const int *index, int n, const double *a, const double *b, void *stream);
int fdd_interface_sum(double *a, double *b, const int *ptr, const int *col, int rows, const double *buf, void *stream);

/* ------------------------------------------------------------------ */
/* AMG setup on the device (csrc/fdd_amg_setup.hip): the leading levels */
/* of the low-order hierarchy, bit-identical to host/low_order.hpp      */
/* ------------------------------------------------------------------ */
/* Every sparse result is built count -> row pointers -> fill.  Matrices are CSR with int indices in device memory.
 * row_pointers: ptr_host[0] = 0, ptr_host[i + 1] = ptr_host[i] + row_len[i], scanned on the host in 64-bit arithmetic
 * (FDD_ERR_INVALID_ARGUMENT when the total leaves the int range; nothing wraps), and copied to ptr (device, rows + 1).
 * Blocking. */
int fdd_amg_setup_row_pointers(int *ptr, int *ptr_host, const int *row_len, int rows, void *stream);
/* C = A B in the order of low_order::multiply (Gustavson: acc[j] starts at 0.0 and takes a_ik * b_kj in the order of A's
 * row, then of B's row); output columns ascending.  B's rows must be sorted by column.  cursor_ws: nnz(A) ints.  The col /
 * val arrays of a matrix without entries may be NULL. */
int fdd_amg_setup_spgemm_count(int *row_len, int *cursor_ws, const int *A_ptr, const int *A_col, const int *B_ptr, const int *B_col, int a_rows, int b_rows, void *stream);
int fdd_amg_setup_spgemm_fill(int *C_col, double *C_val, int *cursor_ws, const int *C_ptr, const int *A_ptr, const int *A_col, const double *A_val, const int *B_ptr, const int *B_col, const double *B_val, int a_rows, int b_rows, void *stream);
/* T = A^T, the stable counting sort of low_order::transpose: every row of T in A's row order, values only move.
 * drop_tol >= 0 keeps the entries with |a| > drop_tol only (CSR_Matrix::transpose); < 0 keeps all.  A_val / T_val may be
 * NULL (pattern only).  row_len: a_cols ints (zeroed here); cursor_ws: a_cols ints; src_ws: nnz_t ints. */
int fdd_amg_setup_transpose_count(int *row_len, const int *A_ptr, const int *A_col, const double *A_val, int a_rows, int a_cols, double drop_tol, void *stream);
int fdd_amg_setup_transpose_fill(int *T_col, double *T_val, int *cursor_ws, int *src_ws, const int *T_ptr, const int *A_ptr, const int *A_col, const double *A_val, int a_rows, int a_cols, int nnz_t, double drop_tol, void *stream);
/* low_order::assemble_fem: the P1 stiffness of the 6 tetrahedra of every GLL sub-cell.  stencils: per element point
 * (element-major, x fastest) its row's 27 neighbour slots K[27 * point + s] and their `touched` bits mask[point], summed in
 * the host's order (sz, sy, sx, t).  count / fill: the rows of the dofs from the stencils of their points (dof_ptr /
 * dof_points: the ascending points of every dof, the transpose of point_dof), as from_triplets merges them. */
int fdd_amg_setup_fem_stencils(double *K, unsigned int *mask, const double *x, const double *y, const double *z, const int *point_dof, int poly_degree, int num_elements, double epsilon, void *stream);
int fdd_amg_setup_fem_count(int *row_len, const int *dof_ptr, const int *dof_points, const unsigned int *mask, const int *point_dof, int poly_degree, int num_dofs, void *stream);
int fdd_amg_setup_fem_fill(int *A_col, double *A_val, const int *A_ptr, const int *dof_ptr, const int *dof_points, const unsigned int *mask, const double *K, const int *point_dof, int poly_degree, int num_dofs, void *stream);
/* D[i] = 1 / sqrt(a_ii) (a_ii = 0.0 where row i has no diagonal entry), as low_order::build computes it */
int fdd_amg_setup_inv_sqrt_diagonal(double *D, const int *A_ptr, const int *A_col, const double *A_val, int rows, void *stream);
/* flag (device int) = 1 if every one of the nnz values is exactly 1.0, else 0 */
int fdd_amg_setup_unit_values(int *flag, const double *val, long long nnz, void *stream);
/* One geometric level (low_order::geometric_level) of a conforming 3-D lattice given as its point -> dof array point_dof
 * (num_elements * n^3 points, -1: no dof).  keep (m), lo, hi, wl (n each) are HOST arrays: the nodes the coarser lattice
 * keeps and the 1-D interpolation of every node (n <= 32).  In order:
 *   lattice_dofs          first[d] = the first point of dof d (INT_MAX: none), kept[d] = 1 where a point of d is kept in
 *                         every direction; num_points < 2^31
 *   lattice_coarse_flags  flag[d] = 1 for the dofs that stay (no point, or kept) -> fdd_amg_setup_row_pointers -> cstart
 *   lattice_cmap          cmap[d] = cstart[d] for those, -1 otherwise; owner_dof[first[d]] = d (-1 elsewhere, num_points
 *                         entries); *unplaced (device int) = 1 if some dof has no point
 *   lattice_interp_count / _fill   the rows of P (num_dofs x coarse dofs): row lengths (-1 where a kept node's dof is not
 *                         kept, refused by row_pointers), then columns and values
 *   lattice_coarse_points the coarser lattice's point -> coarse dof array (num_elements * m^3 points) */
int fdd_amg_setup_lattice_dofs(int *first, int *kept, const int *point_dof, long long num_elements, int num_dofs, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream);
int fdd_amg_setup_lattice_coarse_flags(int *flag, const int *first, const int *kept, int num_dofs, void *stream);
int fdd_amg_setup_lattice_cmap(int *cmap, int *owner_dof, int *unplaced, const int *cstart, const int *first, const int *kept, long long num_points, int num_dofs, void *stream);
int fdd_amg_setup_lattice_interp_count(int *row_len, const int *cmap, const int *first, const int *point_dof, int num_dofs, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream);
int fdd_amg_setup_lattice_interp_fill(int *P_col, double *P_val, const int *P_ptr, const int *cmap, const int *first, const int *point_dof, int num_dofs, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream);
int fdd_amg_setup_lattice_coarse_points(int *coarse_point_dof, const int *point_dof, const int *cmap, long long num_elements, int n, int m, const int *keep, const int *lo, const int *hi, const double *wl, void *stream);
/* free and total device memory (hipMemGetInfo): the setup's peak HBM under FDD_SETUP_TIMING */
int fdd_amg_setup_memory_info(size_t *free_bytes, size_t *total_bytes);

#ifdef __cplusplus
}
#endif

#endif /* FDD_HIP_H */
