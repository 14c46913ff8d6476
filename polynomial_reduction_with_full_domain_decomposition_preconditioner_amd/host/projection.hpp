/*
 * projection.hpp -- successive-right-hand-side projection for the outer solve (an addition of this build: the
 * reference starts every solve from u = 0 and has no counterpart; the practice is Fischer's, standard in Nek5000).
 *
 * A few earlier solutions are kept as an A-orthonormal basis X together with AX = A_L X (unassembled, as make_rhs
 * applies the operator).  The next solve starts from the A-norm best approximation x0 = X (X^T f), the Krylov solver
 * removes what is left, f' = f - AX (X^T f), and the correction is folded back into the basis
 * (Domain::solve_projected drives it).  This class holds the storage and the three passes:
 *
 *   dots   c_k = <X_k, v>                                      (this rank's sums; the caller all-reduces)
 *   apply  x = x_in + sign_x X c, b = b_in + sign_b AX c, optionally <x, b>
 *   store  row k = (x, b) / sqrt(nu2)
 *
 * each either as ONE launch of csrc/fdd_projection.hip (X and AX are one slab each, up to 16 rows) or, where the
 * kernel library lacks those entries or the flag "fused_projection" is 0, composed from entries that were there
 * before: the multi-dot and multi-axpy forms in groups of FDD_MULTI_MAX, fdd_sub_inner_product and
 * fdd_vector_scaling_rsqrt_dev.  Both compute the same sums; the element-wise results have the same bits.
 *
 * Bytes outside the Krylov solve, V = one point vector, K rows in use: start 3K + 4 (dots K + 1, apply 2K + 3), update
 * 3K + 7 (e0 2, dots K + 1, apply 2K + 4), store 4, u = x0 + delta 3: about (6K + 18) V plus one operator application
 * and the two residual norms.
 */
#ifndef FDD_PROJECTION_HPP
#define FDD_PROJECTION_HPP

#include <algorithm>
#include <vector>

#include "fdd_device.hpp"

namespace fdd
{

// the first projection entry the loaded kernel library does not export, or nullptr
inline const char *missing_projection_entry()
{
    if (&fdd_projection_dots == nullptr) return "fdd_projection_dots";
    if (&fdd_projection_apply == nullptr) return "fdd_projection_apply";
    if (&fdd_projection_store == nullptr) return "fdd_projection_store";
    return nullptr;
}

class Projection
{
  public:
    int capacity = 0; // rows allocated (0: off)
    int size = 0;     // rows in use
    int n = 0;        // values per vector
    int ld = 0;       // doubles per row: n rounded up to even, so that every row is 16-byte aligned
    long long restarts = 0;
    bool fused = true; // flag "fused_projection": the kernels of fdd_projection.hip where the library has them

    memory X, AX;      // the slabs
    memory x0, d, w;   // start value, correction and its image
    memory c;          // device scalars: [0, 16) coefficients, then e0 and nu2 behind the K in use; [32, 64) their signed copies

    bool use_fused() const { return fused and missing_projection_entry() == nullptr; }
    double *row(memory &slab, int k) const { return slab.as<double>() + (size_t)k * ld; }

    void release()
    {
        X = AX = x0 = d = w = c = memory();
        capacity = size = n = ld = 0;
        restarts = 0;
    }

    // 0: off, the slabs are freed; the basis starts empty either way
    void configure(int capacity_, int n_)
    {
        release();
        if (capacity_ <= 0) return;
        capacity = capacity_;
        n = n_;
        ld = n + (n & 1);
        X = dev().malloc<double>((size_t)capacity * std::max(ld, 2));
        AX = dev().malloc<double>((size_t)capacity * std::max(ld, 2));
        for (memory *m : {&x0, &d, &w}) *m = dev().malloc<double>(std::max(n, 1));
        c = dev().malloc<double>(64);
    }

    void clear() { size = 0; }

    // out[k] = <X_k, v> (or AX_k with images), k < size: this rank's sums
    void dots(double *out, double *ws, const double *v)
    {
        const int K = size;
        void *stream = dev().stream;
        if (K == 0) return;
        if (use_fused())
        {
            ProfileScope prof("projection_dots_kernel", 8.0 * (K + 1.0) * n);
            FDD_CALL(fdd_projection_dots(out, ws, X.as<double>(), ld, K, v, n, stream));
            return;
        }
        const double *rows[FDD_MULTI_MAX];
        for (int g0 = 0; g0 < K; g0 += FDD_MULTI_MAX)
        {
            const int cnt = std::min(FDD_MULTI_MAX, K - g0);
            for (int i = 0; i < cnt; i++) rows[i] = row(X, g0 + i);
            FDD_CALL(fdd_multi_weighted_inner_product(out + g0, ws, v, rows, cnt, nullptr, n, stream));
        }
    }

    // x = (x_in or 0) + sign_x X coeffs, b = b_in + sign_b AX coeffs over the rows in use; nu2_out: <x, b> (this rank's sum)
    void apply(double *x, double *b, double *nu2_out, double *ws, const double *x_in, const double *b_in, const double *coeffs, double sign_x, double sign_b)
    {
        const int K = size;
        void *stream = dev().stream;
        if (use_fused())
        {
            ProfileScope prof("projection_apply_kernel", 8.0 * (2.0 * K + (x_in ? 4.0 : 3.0)) * n);
            FDD_CALL(fdd_projection_apply(x, b, nu2_out, ws, x_in, b_in, X.as<double>(), AX.as<double>(), ld, K, coeffs, sign_x, sign_b, n, stream));
            return;
        }
        double *sx = c.as<double>() + 32, *sb = sx + FDD_PROJECTION_MAX;
        if (K > 0)
        {
            FDD_CALL(fdd_vector_scaling(sx, sign_x, coeffs, K, stream));
            FDD_CALL(fdd_vector_scaling(sb, sign_b, coeffs, K, stream));
        }
        if (x_in == nullptr)
            FDD_CALL(fdd_set_to_value(x, 0.0, n, 0, stream));
        else if (x_in != x)
            FDD_CALL(fdd_memcpy_d2d(x, x_in, (size_t)n * sizeof(double), stream));
        if (b_in != b) FDD_CALL(fdd_memcpy_d2d(b, b_in, (size_t)n * sizeof(double), stream));
        const double *rows[FDD_MULTI_MAX];
        for (int g0 = 0; g0 < K; g0 += FDD_MULTI_MAX)
        {
            const int cnt = std::min(FDD_MULTI_MAX, K - g0);
            for (int i = 0; i < cnt; i++) rows[i] = row(X, g0 + i);
            FDD_CALL(fdd_multi_axpy_dev(x, sx + g0, rows, cnt, n, stream));
            for (int i = 0; i < cnt; i++) rows[i] = row(AX, g0 + i);
            FDD_CALL(fdd_multi_axpy_dev(b, sb + g0, rows, cnt, n, stream));
        }
        if (nu2_out) FDD_CALL(fdd_sub_inner_product(nu2_out, ws, x, b, n, stream));
    }

    // row k = (x, b) / sqrt(*nu2_dev)
    void store(int k, const double *x, const double *b, const double *nu2_dev)
    {
        void *stream = dev().stream;
        if (use_fused())
        {
            ProfileScope prof("projection_store_kernel", 8.0 * 4.0 * n);
            FDD_CALL(fdd_projection_store(row(X, k), row(AX, k), x, b, nu2_dev, n, stream));
            return;
        }
        FDD_CALL(fdd_vector_scaling_rsqrt_dev(row(X, k), nu2_dev, x, n, stream));
        FDD_CALL(fdd_vector_scaling_rsqrt_dev(row(AX, k), nu2_dev, b, n, stream));
    }
};

} // namespace fdd

#endif
