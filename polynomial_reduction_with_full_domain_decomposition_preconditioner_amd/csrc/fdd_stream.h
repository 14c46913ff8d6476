// How a lane of a streaming (HBM-bound, read-once) kernel reaches its element or elements of a vector, and the few
// statements more than one of those kernels makes (fdd_blas1.hip, fdd_reduce.hip, fdd_f32.hip, fdd_projection.hip).
#ifndef FDD_STREAM_H
#define FDD_STREAM_H

#include "fdd_common.h"

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = FDD_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, FDD_WAVE);
    return v;
}

// 16-byte streaming loads are non-temporal: these kernels read every byte once per launch
// and the operands are far larger than the caches (measured +10-15 % on the multi-stream ops)
typedef double fdd_v2f64 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 ld2(const double *p, long long i)
{
    const fdd_v2f64 v = __builtin_nontemporal_load(reinterpret_cast<const fdd_v2f64 *>(p) + i);
    return make_double2(v.x, v.y);
}

// W elements of a vector; the arithmetic is per component, between two of them or a scalar on the left and one.
// A struct and not an ext_vector_type: with clang's vector arithmetic the scalar set-up in front of the loops grows
// (ew_vec2_kernel<MultiAxpyOp<8>>: 74 -> 104 SGPRs, 8 -> 7 waves per SIMD); with this most pair kernels compile to the
// text they had when each op spelt .x and .y out (profiles/r18_stream_ops/device_code.md).
template <typename T, int W>
struct alignas(W * sizeof(T)) fdd_vec
{
    T c[W];
};
#define FDD_VEC_OP(OP)                                                                                                         \
    template <typename T, int W>                                                                                               \
    __device__ __forceinline__ fdd_vec<T, W> operator OP(const fdd_vec<T, W> &a, const fdd_vec<T, W> &b)                        \
    {                                                                                                                          \
        fdd_vec<T, W> r;                                                                                                       \
        for (int k = 0; k < W; k++) r.c[k] = a.c[k] OP b.c[k];                                                                 \
        return r;                                                                                                              \
    }                                                                                                                          \
    template <typename T, int W>                                                                                               \
    __device__ __forceinline__ fdd_vec<T, W> operator OP(typename std::common_type<T>::type s, const fdd_vec<T, W> &b)          \
    {                                                                                                                          \
        fdd_vec<T, W> r;                                                                                                       \
        for (int k = 0; k < W; k++) r.c[k] = s OP b.c[k];                                                                      \
        return r;                                                                                                              \
    }
FDD_VEC_OP(+)
FDD_VEC_OP(-)
FDD_VEC_OP(*)
FDD_VEC_OP(/)
#undef FDD_VEC_OP

template <typename T, int W>
struct fdd_lane_value
{
    typedef fdd_vec<T, W> type;
};
template <typename T>
struct fdd_lane_value<T, 1>
{
    typedef T type;
};

// W consecutive elements per lane: element i of a lane is elements W*i .. W*i + W-1 of the vector.  An operation written
// over an accessor A holds its loads, arithmetic and stores once; the arithmetic on value<T> is per component, in the
// order written (-ffp-contract=off), so every width gives every element the same bits.
//   W = 1  plain loads and stores, any pointer (slice offsets, the odd last element)
//   W = 2  doubles: one 16-byte non-temporal load (ld2 above); floats: one plain 8-byte load
//   W = 4  floats: one plain 16-byte load
// Stores are plain everywhere: the next kernel usually reads what this one wrote.
template <int W>
struct fdd_lanes
{
    template <typename T>
    using value = typename fdd_lane_value<T, W>::type;

    // what a pointer to T must be aligned to
    template <typename T>
    static constexpr int bytes = W == 1 ? 1 : W * (int)sizeof(T);

    template <typename T>
    static __device__ __forceinline__ value<T> ld(const T *p, long long i)
    {
        if constexpr (W == 2 && std::is_same<T, double>::value)
        {
            const double2 v = ld2(p, i);
            return {v.x, v.y};
        }
        else
            return reinterpret_cast<const value<T> *>(p)[i];
    }

    template <typename T>
    static __device__ __forceinline__ void st(T *p, long long i, value<T> v)
    {
        reinterpret_cast<value<T> *>(p)[i] = v;
    }

    // x in every component
    template <typename T>
    static __device__ __forceinline__ value<T> all(T x)
    {
        if constexpr (W == 1)
            return x;
        else
        {
            value<T> v;
            for (int k = 0; k < W; k++) v.c[k] = x;
            return v;
        }
    }

    // every component converted to To
    template <typename To, typename V>
    static __device__ __forceinline__ value<To> to(V v)
    {
        if constexpr (W == 1)
            return (To)v;
        else
        {
            value<To> r;
            for (int k = 0; k < W; k++) r.c[k] = (To)v.c[k];
            return r;
        }
    }

    // s += the components of t, first to last: the order of a reduction's private sum
    static __device__ __forceinline__ void add(double &s, value<double> t)
    {
        if constexpr (W == 1)
            s += t;
        else
            for (int k = 0; k < W; k++) s += t.c[k];
    }
};

static inline bool fdd_aligned(const void *p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

// Whether every vector `op` touches may be walked with accessor A.  op.pointers(f) names them: f(p), or f(p, bytes) for
// a pointer the entry has always held to more than A asks.  NULL (an optional vector that is absent) counts as aligned.
template <typename A, typename Op>
static inline bool fdd_lanes_fit(const Op &op)
{
    bool fit = true;
    op.pointers([&fit](auto *p, int bytes = 1) {
        constexpr int need = A::template bytes<std::remove_cv_t<std::remove_pointer_t<decltype(p)>>>;
        fit = fit && fdd_aligned(p, bytes > need ? bytes : need);
    });
    return fit;
}

// x <- (...((1.0*x + c_0 v_0) + c_1 v_1)...) + c_kmax v_kmax, v_k standing for vs[k] * v_k where vs is given: M successive
// vector_vector_addition(q, 1.0, q, c_k, v_k) (math.okl:21-27) on the values of one lane, coefficients in device memory.
// v(k) loads v_k's values.
template <int M, typename V, typename Load>
__device__ __forceinline__ V fdd_lincomb(V x, int kmax, const double *c, const double *vs, Load v)
{
#pragma unroll
    for (int k = 0; k < M; k++)
    {
        if (k > kmax) break;
        const double ck = c[k];
        V b = v(k);
        if (vs) b = vs[k] * b;
        x = 1.0 * x + ck * b;
    }
    return x;
}

// One step of the Chebyshev-Jacobi inner solve (host/subdomain.hpp, chebyshev_dofs) on the elements of one lane, T = double
// or float.  The statements are those of the entries the step can also be composed from, in their order --
// vector_vector_addition (AxpbyOp, axpby_f32_kernel) and vector_diagonal_scaling_dev (DiagScaleDevOp,
// diag_scale_dev_f32_kernel) -- so the bits are the same either way:
//   first : t = dinv .* r_in;  d = c_r*t + 0*t;                                x = d
//   later : r = 1*r_in + (-1)*q;  t = dinv .* r;  d = c_d*d + c_r*t;            x = 1*x + 1*d
// r_in is the right-hand side at the second step (never written) and r_out itself afterwards; the last step stores x only.
// f64 bytes per dof: first 32, middle 64, last 48.
template <typename A, typename T>
__device__ __forceinline__ void fdd_cheby_step_at(A a, long long i, T *x, T *d, T *r_out, const T *r_in, const T *q, const T *dinv, T c_d, T c_r, int first, int last)
{
    const auto di = a.ld(dinv, i);
    auto r = a.ld(r_in, i), dv = a.all(T(0.0)), xv = dv;
    if (!first)
    {
        const auto qv = a.ld(q, i);
        dv = a.ld(d, i);
        xv = a.ld(x, i);
        r = T(1.0) * r + T(-1.0) * qv;
    }
    const auto t = di * r;
    dv = first ? c_r * t + T(0.0) * t : c_d * dv + c_r * t;
    a.st(x, i, first ? dv : T(1.0) * xv + T(1.0) * dv);
    if (last) return;
    a.st(d, i, dv);
    if (!first) a.st(r_out, i, r);
}

#endif
