/*
 * precision_ops.hpp -- the kernel entries that exist once per precision (fdd_x on double, fdd_x_f32 on float vectors),
 * named once: inline overloads on the pointer type, so that the inner GMRES (subdomain.hpp) and the V-cycle (amg.hpp)
 * are written once over `Real`.  Where the two precisions differ in more than the suffix the difference is spelled
 * out here and nowhere else.  Scalars on the device (scales, coefficients, reduction results) are double in both.
 * The profile labels are the ones bench.py's kernel table keys on.
 */
#ifndef FDD_PRECISION_OPS_HPP
#define FDD_PRECISION_OPS_HPP

#include "config.hpp"

namespace fdd
{
namespace ops
{

// ---- element-wise ----
inline void scaling_dev(double *au, const double *scale_dev, const double *u, int n, void *s) { FDD_CALL(fdd_vector_scaling_dev(au, scale_dev, u, n, s)); }
inline void scaling_dev(float *au, const double *scale_dev, const float *u, int n, void *s) { FDD_CALL(fdd_vector_scaling_dev_f32(au, scale_dev, u, n, s)); }
inline void diagonal_scaling_dev(double *z, const double *d, const double *scale_dev, const double *u, int n, void *s) { FDD_CALL(fdd_vector_diagonal_scaling_dev(z, d, scale_dev, u, n, s)); }
inline void diagonal_scaling_dev(float *z, const float *d, const double *scale_dev, const float *u, int n, void *s) { FDD_CALL(fdd_vector_diagonal_scaling_dev_f32(z, d, scale_dev, u, n, s)); }
inline void vector_vector_addition(double *uv, double a, const double *u, double b, const double *v, int n, void *s) { FDD_CALL(fdd_vector_vector_addition(uv, a, u, b, v, n, s)); }
inline void vector_vector_addition(float *uv, float a, const float *u, float b, const float *v, int n, void *s) { FDD_CALL(fdd_vector_vector_addition_f32(uv, a, u, b, v, n, s)); }
inline void set_to_zero(double *u, int n, void *s) { FDD_CALL(fdd_set_to_value(u, 0.0, n, 0, s)); }
inline void set_to_zero(float *u, int n, void *s) { FDD_CALL(fdd_amg_vector_set_to_value_f32(u, 0.0f, n, s)); }
inline void gather_indexed(double *out, const double *in, const int *index, int n, void *s) { FDD_CALL(fdd_gather_indexed(out, in, index, nullptr, n, s)); }
inline void gather_indexed(float *out, const float *in, const int *index, int n, void *s) { FDD_CALL(fdd_gather_indexed_f32(out, in, index, n, s)); }
inline void scatter_add_indexed(double *y, const int *index, const double *t, int n, void *s) { FDD_CALL(fdd_scatter_add_indexed(y, index, t, n, s)); }
inline void scatter_add_indexed(float *y, const int *index, const float *t, int n, void *s) { FDD_CALL(fdd_scatter_add_indexed_f32(y, index, t, n, s)); }
inline void copy(double *u, const double *v, int n, void *s) { FDD_CALL(fdd_memcpy_d2d(u, v, (size_t)n * sizeof(double), s)); }
inline void copy(float *u, const float *v, int n, void *s) { FDD_CALL(fdd_memcpy_d2d(u, v, (size_t)n * sizeof(float), s)); }
// one step of the Chebyshev-Jacobi inner solve as one pass (Subdomain::chebyshev_dofs)
inline void cheby_step(double *x, double *d, double *r_out, const double *r_in, const double *q, const double *dinv, double c_d, double c_r, bool first, bool last, int n, void *s)
{
    ProfileScope prof("ew_vec2_kernel<ChebyStep>", 8.0 * n * (first ? 4 : (last ? 6 : 8)));
    FDD_CALL(fdd_cheby_step(x, d, r_out, r_in, q, dinv, c_d, c_r, first ? 1 : 0, last ? 1 : 0, n, s));
}
inline void cheby_step(float *x, float *d, float *r_out, const float *r_in, const float *q, const float *dinv, double c_d, double c_r, bool first, bool last, int n, void *s)
{
    ProfileScope prof("cheby_step_f32_kernel", 4.0 * n * (first ? 4 : (last ? 6 : 8)));
    FDD_CALL(fdd_cheby_step_f32(x, d, r_out, r_in, q, dinv, (float)c_d, (float)c_r, first ? 1 : 0, last ? 1 : 0, n, s));
}
// y += c .* (scale x): the zeroth-order term of a Helmholtz operator behind the operator application that formed y
inline void shift_add(double *y, const double *c, const double *scale_dev, const double *x, int n, void *s)
{
    ProfileScope prof("shift_add_kernel<f64>", 8.0 * n * 4);
    FDD_CALL(fdd_shift_add(y, c, scale_dev, x, n, s));
}
inline void shift_add(float *y, const float *c, const double *scale_dev, const float *x, int n, void *s)
{
    ProfileScope prof("shift_add_kernel<f32>", 4.0 * n * 4);
    FDD_CALL(fdd_shift_add_f32(y, c, scale_dev, x, n, s));
}

// the same on the m entries of c's support (host/boundary.hpp: ShiftSupport); an entry moves two values of y, one of x, one of
// c and its index, each scattered access a line of its own at worst
inline void shift_add_indexed(double *y, const double *c_values, const int *index, int m, const double *scale_dev, const double *x, int n, void *s)
{
    ProfileScope prof("shift_add_indexed_kernel<f64>", (8.0 * 4 + 4.0) * m);
    FDD_CALL(fdd_shift_add_indexed(y, c_values, index, m, scale_dev, x, n, s));
}
inline void shift_add_indexed(float *y, const float *c_values, const int *index, int m, const double *scale_dev, const float *x, int n, void *s)
{
    ProfileScope prof("shift_add_indexed_kernel<f32>", (4.0 * 4 + 4.0) * m);
    FDD_CALL(fdd_shift_add_indexed_f32(y, c_values, index, m, scale_dev, x, n, s));
}

// ---- the Arnoldi step's reductions: out[k] = <a, s_k b_k>, and dst = y + sign sum c_k (s_k x_k) with |dst|^2 ----
// w: the norm weight of the dofs (null: 1 everywhere, not read).  The float entries take none.
inline void multi_dot(double *out, double *ws, const double *a, const double *const *b, const double *b_scale, int m, const double *w, int n, void *s)
{
    ProfileScope prof("reduce_vec2_kernel<MultiDotW>", 8.0 * n * (m + 1 + (w ? 1 : 0)));
    FDD_CALL(fdd_multi_weighted_inner_product_scaled(out, ws, a, b, b_scale, m, w, n, s));
}
inline void multi_dot(double *out, double *ws, const float *a, const float *const *b, const double *b_scale, int m, const double *, int n, void *s)
{
    ProfileScope prof("reduce_vec2_kernel<MultiDotF32>", 4.0 * n * (m + 1));
    FDD_CALL(fdd_multi_inner_product_scaled_f32(out, ws, a, b, b_scale, m, n, s));
}
inline void multi_axpy_norm2(double *out, double *ws, double *dst, const double *y, const double *coeffs_dev, double sign, const double *const *x, const double *x_scale, int m, const double *w, int n, void *s)
{
    ProfileScope prof("reduce_vec2_kernel<MultiAxpyNorm>", 8.0 * n * (m + 2 + (w ? 1 : 0)));
    FDD_CALL(fdd_multi_axpy_norm2_scaled_dev(out, ws, dst, y, coeffs_dev, sign, x, x_scale, m, w, n, s));
}
inline void multi_axpy_norm2(double *out, double *ws, float *dst, const float *y, const double *coeffs_dev, double sign, const float *const *x, const double *x_scale, int m, const double *, int n, void *s)
{
    ProfileScope prof("reduce_vec2_kernel<MultiAxpyNormF32>", 4.0 * n * (m + 2));
    FDD_CALL(fdd_multi_axpy_norm2_scaled_dev_f32(out, ws, dst, y, coeffs_dev, sign, x, x_scale, m, n, s));
}
// the last step of a cycle, double only (include/fdd_norm_estimate.h): the dots with out[m] = <a, a> behind them -- the same
// streams, so the same label and bytes -- and the norm pass gated on those m + 1 sums.  The gated pass is recorded under a
// label of its own with no bytes: it moves m + 2 vectors where the gate is open and nothing where it is closed.
inline void multi_dot_self(double *out, double *ws, const double *a, const double *const *b, const double *b_scale, int m, const double *w, int n, void *s)
{
    ProfileScope prof("reduce_vec2_kernel<MultiDotW>", 8.0 * n * (m + 1 + (w ? 1 : 0)));
    FDD_CALL(fdd_multi_weighted_inner_product_self(out, ws, a, b, b_scale, m, w, n, s));
}
inline void multi_axpy_norm2_gated(double *out, double *ws, double *dst, const double *y, const double *coeffs_dev, double sign, const double *const *x, const double *x_scale, int m, const double *w, int n, const double *dots_dev, void *s)
{
    ProfileScope prof("reduce_vec2_gated_kernel<MultiAxpyNorm>", 0.0);
    FDD_CALL(fdd_multi_axpy_norm2_scaled_gated_dev(out, ws, dst, y, coeffs_dev, sign, x, x_scale, m, w, n, dots_dev, s));
}

// ---- the solution update q (+)= sum_k c_k (s_k v_k); q_is_zero: q is not read ----
// all m vectors (the host knows the column count).  Float has the limited entry only and runs it without a limit.
inline void lincomb(double *q, int q_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale, int m, int n, void *s)
{
    ProfileScope prof("ew_vec2_kernel<MultiAxpy>", 8.0 * n * (m + (q_is_zero ? 1 : 2)));
    FDD_CALL(fdd_multi_lincomb_scaled_dev(q, q_is_zero, coeffs_dev, v, v_scale, m, n, s));
}
inline void lincomb(float *q, int q_is_zero, const double *coeffs_dev, const float *const *v, const double *v_scale, int m, int n, void *s) { FDD_CALL(fdd_multi_lincomb_limited_dev_f32(q, q_is_zero, coeffs_dev, v, v_scale, nullptr, m, n, s)); }
// vectors 0 .. (int)*last_dev only (the column count stays on the device: the lazy history)
inline void lincomb_limited(double *q, int q_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale, const double *last_dev, int m, int n, void *s)
{
    ProfileScope prof("ew_vec2_kernel<MultiAxpy>", 8.0 * n * (m + 2));
    FDD_CALL(fdd_multi_lincomb_limited_dev(q, q_is_zero, coeffs_dev, v, v_scale, last_dev, m, n, s));
}
inline void lincomb_limited(float *q, int q_is_zero, const double *coeffs_dev, const float *const *v, const double *v_scale, const double *last_dev, int m, int n, void *s) { FDD_CALL(fdd_multi_lincomb_limited_dev_f32(q, q_is_zero, coeffs_dev, v, v_scale, last_dev, m, n, s)); }

// ---- V-cycle (amg.hpp) ----
inline void amg_set_to_value(double *u, double value, int n, void *s) { FDD_CALL(fdd_amg_vector_set_to_value(u, value, n, s)); }
inline void amg_set_to_value(float *u, float value, int n, void *s) { FDD_CALL(fdd_amg_vector_set_to_value_f32(u, value, n, s)); }
inline void amg_smooth_start(double *work, double *Sr, const double *f, const double *D, double coef, int n, void *s) { FDD_CALL(fdd_amg_smooth_start(work, Sr, f, D, coef, n, s)); }
inline void amg_smooth_start(float *work, float *Sr, const float *f, const float *D, float coef, int n, void *s) { FDD_CALL(fdd_amg_smooth_start_f32(work, Sr, f, D, coef, n, s)); }
inline void lattice_restrict(double *partial, const double *fine, const int *owner_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long ne, void *s) { FDD_CALL(fdd_lattice_restrict(partial, fine, owner_dof, n, m, lo, hi, wl, ne, s)); }
inline void lattice_restrict(float *partial, const float *fine, const int *owner_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long ne, void *s) { FDD_CALL(fdd_lattice_restrict_f32(partial, fine, owner_dof, n, m, lo, hi, wl, ne, s)); }
inline void lattice_prolong(double *u, const double *coarse, const int *owner_dof, const int *coarse_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long ne, void *s) { FDD_CALL(fdd_lattice_prolong(u, coarse, owner_dof, coarse_dof, n, m, lo, hi, wl, ne, s)); }
inline void lattice_prolong(float *u, const float *coarse, const int *owner_dof, const int *coarse_dof, int n, int m, const int *lo, const int *hi, const double *wl, long long ne, void *s) { FDD_CALL(fdd_lattice_prolong_f32(u, coarse, owner_dof, coarse_dof, n, m, lo, hi, wl, ne, s)); }

} // namespace ops
} // namespace fdd

#endif
