/*
 * fdd_norm_estimate.h -- the norm of the last Arnoldi vector of a cycle from the projections, stated once for the device
 * kernels (csrc/fdd_reduce.hip, csrc/fdd_krylov.hip) and for the host recurrence (host/subdomain.hpp).
 *
 * With an orthonormal basis v_0..v_{m-1}, h_k = <q, v_k> and aa = <q, q>,
 *     |q - sum_k h_k v_k|^2 = aa - sum_k h_k^2
 * up to rounding, so the pass that forms the left side from the vectors can be left out where its vector is not read.
 *
 * The subtraction cancels: it loses log2(aa / est) of the 53 bits of a double.  The estimate is used only while
 * est >= aa * 2^-10: ten lost bits leave a relative error near 2^-43 ~ 1e-13, below the 1e-12 this project holds its
 * operators to.  That bound is a design bound, not a tuned value.  Below it, for a negative difference (an Arnoldi
 * breakdown) and for anything that is not finite the answer is 0 and the caller runs the exact pass.
 *
 * Double precision only: a float basis is orthogonal to about 1e-7, so the identity does not hold to double rounding there.
 */
#ifndef FDD_NORM_ESTIMATE_H
#define FDD_NORM_ESTIMATE_H

#if defined(__HIPCC__)
#define FDD_NORM_ESTIMATE_FN __host__ __device__ static inline
#elif defined(__GNUC__) && !defined(__clang__)
#define FDD_NORM_ESTIMATE_FN __attribute__((optimize("fp-contract=off"))) static inline
#else
#define FDD_NORM_ESTIMATE_FN static inline
#endif

#define FDD_NORM_ESTIMATE_BOUND 0.0009765625 /* 2^-10 */

/* est = aa - h[0]^2 - h[1]^2 - ... - h[m-1]^2, subtracted in ascending order, every product rounded before it is
 * subtracted (no contraction).  Returns 1 where *est may stand for the directly summed norm, 0 where it may not. */
FDD_NORM_ESTIMATE_FN int fdd_norm2_from_projections(double aa, const double *h, int m, double *est)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double e = aa;
    for (int k = 0; k < m; k++)
    {
        const double hh = h[k] * h[k];
        e = e - hh;
    }
    *est = e;
    /* x - x is 0 for a finite x and NaN for an infinite one or a NaN; a NaN among the h makes e a NaN */
    const int finite = (aa - aa == 0.0) && (e - e == 0.0);
    return finite && e >= aa * FDD_NORM_ESTIMATE_BOUND;
}

#endif
