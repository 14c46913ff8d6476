// Element-wise streaming kernels (HBM-bound): math.okl, the fused vector
// updates of domain.okl / subdomain.okl, the precision-cast copies and the
// element-wise AMG smoother kernels of AMG/kernels.cu.
//
// One template drives them all: every op states its loads, arithmetic and stores
// once, in at(), over a lane accessor (fdd_stream.h).  Where every pointer the op
// names allows it, a lane moves a pair (16 B of doubles) per access; the grid is
// capped and strides over the vector, so a 134 MB vector is fully coalesced 1 KiB
// wave-accesses.  Pointers that are not aligned for pairs (occa::memory::slice
// offsets, math.okl's `offset`) and the odd last element take one element per lane.
//
// Compiled with -ffp-contract=off: a*x + b*y is two multiplies and one add in
// source order, bit-identical to the OCCA-Serial arithmetic.
#include "fdd_stream.h"

namespace
{

constexpr int kBlock = 256;
using Single = fdd_lanes<1>;
using Pair = fdd_lanes<2>;

template <typename Op>
__global__ __launch_bounds__(kBlock) void ew_vec2_kernel(Op op, long long n2, long long n)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) op.at(Pair{}, i);
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) op.at(Single{}, n - 1);
}

template <typename Op>
__global__ __launch_bounds__(kBlock) void ew_scalar_kernel(Op op, long long n)
{
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) op.at(Single{}, i);
}

// Element-wise kernels have no per-workgroup epilogue: at C2 sizes a grid of one pair of doubles per lane (21 k workgroups)
// streams 5 % faster than 2048 workgroups walking the vector (6.7 against 6.3 TB/s on the axpy forms); the reductions,
// whose workgroups end in a fold, are best at the 2048 of FDD_REDUCE_MAX_BLOCKS (16384: 4.0-5.1 instead of 5.9 TB/s).
constexpr int kEwMaxBlocks = 32768;

template <typename Op>
int launch_ew(const Op &op, long long n, void *stream)
{
    if (n <= 0) return 0;
    if (fdd_lanes_fit<Pair>(op) && n >= 2)
    {
        long long n2 = n / 2;
        int grid = fdd_stream_grid(n2, kBlock, kEwMaxBlocks);
        hipLaunchKernelGGL(ew_vec2_kernel<Op>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), op, n2, n);
    }
    else
    {
        int grid = fdd_stream_grid(n, kBlock, kEwMaxBlocks);
        hipLaunchKernelGGL(ew_scalar_kernel<Op>, dim3(grid), dim3(kBlock), 0, fdd_stream(stream), op, n);
    }
    FDD_LAUNCH_CHECK();
    return 0;
}

// Every op: at(a, i) is the operation on element i of accessor a (all loads before the first store: the vectors may be
// one another), pointers(f) names the vectors it touches.

// ---------------------------------------------------------------- math.okl
struct SetOp // math.okl:5-11
{
    double *u;
    double alpha;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(u, i, a.all(alpha)); }
    template <typename F>
    void pointers(F f) const { f(u); }
};

struct InvertOp // math.okl:13-19
{
    double *u;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(u, i, 1.0 / a.ld(u, i)); }
    template <typename F>
    void pointers(F f) const { f(u); }
};

struct AxpbyOp // math.okl:21-27
{
    double *uv;
    const double *u;
    const double *v;
    double alpha, beta;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(uv, i, alpha * a.ld(u, i) + beta * a.ld(v, i)); }
    template <typename F>
    void pointers(F f) const { f(uv), f(u), f(v); }
};

// x = (1 / sqrt(*s2)) * u with the squared norm still on the device
// (host sequence: alpha = sqrt(s2); vector_scaling(x, 1.0 / alpha, u), subdomain.tpp:4457)
struct ScaleRsqrtDevOp
{
    double *au;
    const double *u;
    const double *s2;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(au, i, (1.0 / sqrt(*s2)) * a.ld(u, i)); }
    template <typename F>
    void pointers(F f) const { f(au), f(u); }
};

// au = (*scale) * u: math.okl:29-35 with the factor read from device memory
struct ScaleDevOp
{
    double *au;
    const double *u;
    const double *scale;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(au, i, (*scale) * a.ld(u, i)); }
    template <typename F>
    void pointers(F f) const { f(au), f(u); }
};

// z = d .* ((*scale) * u): the point-Jacobi preconditioner of the inner solve applied to a Krylov vector kept
// unnormalised (vector_scaling, math.okl:29-35, then AMG/kernels.cu:64-73 vector_multiplication, in that order)
struct DiagScaleDevOp
{
    double *z;
    const double *d;
    const double *u;
    const double *scale; // may be null: z = d .* u
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const auto uu = a.ld(u, i), dd = a.ld(d, i);
        a.st(z, i, scale ? dd * ((*scale) * uu) : dd * uu);
    }
    template <typename F>
    void pointers(F f) const { f(z), f(u), f(d); }
};

// out = x + (*num / *den) * y: the p = z + beta*p half of residual_and_search_update (domain.okl:218-233)
// when r = r+ is a buffer swap instead of a copy
struct XpbyRatioDevOp
{
    double *out;
    const double *x, *y, *num, *den;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(out, i, a.ld(x, i) + (*num / *den) * a.ld(y, i)); }
    template <typename F>
    void pointers(F f) const { f(out), f(x), f(y); }
};

// out = x - (*num / *den) * y: the r+ = r - alpha*q half of solution_and_residual_update (domain.okl:186-193) on
// a vector the node-space solve keeps beside its node vectors (the point-space residual the degree tree is fed with)
struct XmayRatioDevOp
{
    double *out;
    const double *x, *y, *num, *den;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(out, i, a.ld(x, i) - (*num / *den) * a.ld(y, i)); }
    template <typename F>
    void pointers(F f) const { f(out), f(x), f(y); }
};

// u = u + (*a_num / *a_den) * p and p = z + (*b_num / *b_den) * p with p loaded once: the solution update of UpdateUROp
// (domain.okl:186-193), which nothing reads before the end of a solve, carried by the direction update that reads p anyway
// (XpbyRatioDevOp above, out == y == p).  Both expressions are those ops' own, so u and p keep their bits.
struct SolutionDirectionDevOp
{
    double *u, *p;
    const double *z, *a_num, *a_den, *b_num, *b_den;
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const double al = a_num[0] / a_den[0];
        const auto uu = a.ld(u, i), pp = a.ld(p, i), zz = a.ld(z, i);
        a.st(u, i, uu + al * pp);
        a.st(p, i, zz + (*b_num / *b_den) * pp);
    }
    template <typename F>
    void pointers(F f) const { f(u), f(p), f(z); }
};

struct ChebyStepOp // fdd_cheby_step_at (fdd_stream.h)
{
    double *x, *d, *r_out;
    const double *r_in, *q, *dinv;
    double c_d, c_r;
    int first, last;
    template <typename A>
    __device__ void at(A a, long long i) const { fdd_cheby_step_at(a, i, x, d, r_out, r_in, q, dinv, c_d, c_r, first, last); }
    template <typename F>
    void pointers(F f) const // the vectors this step touches: a pointer it leaves alone may be anything
    {
        f(x), f(r_in), f(dinv);
        if (!last) f(d);
        if (!first) f(q), f(d);
        if (!first && !last) f(r_out);
    }
};

} // namespace
__global__ void fdd_sqrt_sum_kernel(double *out, const double *parts, int nparts)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < nparts; k++) s += parts[k];
    *out = sqrt(s);
}
namespace
{
struct ScaleOp // math.okl:29-35
{
    double *au;
    const double *u;
    double alpha;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(au, i, alpha * a.ld(u, i)); }
    template <typename F>
    void pointers(F f) const { f(au), f(u); }
};

// ------------------------------------------------- domain.okl / subdomain.okl
struct InitOp // domain.okl:100-107, subdomain.okl:211-218
{
    double *u_k;
    double *r_k;
    const double *f;
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const auto fv = a.ld(f, i);
        a.st(u_k, i, a.all(0.0));
        a.st(r_k, i, fv);
    }
    template <typename F>
    void pointers(F fn) const { fn(u_k), fn(r_k), fn(f); }
};

// alpha either by value or as num/den read from device memory
struct ScalarByValue
{
    double v;
    __device__ double get() const { return v; }
};
struct ScalarRatioDev
{
    const double *num;
    const double *den;
    __device__ double get() const { return num[0] / den[0]; }
};

template <typename S>
struct UpdateUROp // domain.okl:186-193, subdomain.okl:220-227
{
    double *u_k;
    double *r_kp1;
    const double *r_k;
    const double *p_k;
    const double *q_k;
    S alpha;
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const double al = alpha.get();
        const auto u = a.ld(u_k, i), r = a.ld(r_k, i), p = a.ld(p_k, i), q = a.ld(q_k, i);
        a.st(u_k, i, u + al * p);
        a.st(r_kp1, i, r - al * q);
    }
    template <typename F>
    void pointers(F f) const { f(u_k), f(r_kp1), f(r_k), f(p_k), f(q_k); }
};

template <typename S>
struct UpdatePROp // domain.okl:226-233, subdomain.okl:259-266
{
    double *p_k;
    double *r_k;
    const double *z_k;
    const double *r_kp1;
    S beta;
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const double b = beta.get();
        const auto z = a.ld(z_k, i), p = a.ld(p_k, i), r = a.ld(r_kp1, i);
        a.st(p_k, i, z + b * p);
        a.st(r_k, i, r);
    }
    template <typename F>
    void pointers(F f) const { f(p_k), f(r_k), f(z_k), f(r_kp1); }
};

template <typename TO, typename FROM>
struct CopyAs // subdomain.okl:268-282: DType = EType = double, and the two casts of DType = float
{
    TO *u;
    const FROM *v;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(u, i, A::template to<TO>(a.ld(v, i))); }
    template <typename F>
    void pointers(F f) const { f(u), f(v); }
};
struct CopyOp : CopyAs<double, double> // subdomain.okl:268-282 with DType = EType = double
{
};
struct CopyF32F64Op : CopyAs<float, double> // subdomain.okl:268-274, DType = float
{
};
struct CopyF64F32Op : CopyAs<double, float> // subdomain.okl:276-282, DType = float
{
};

// q <- (...((1.0*q + c_0 v_0) + c_1 v_1)...) + c_{M-1} v_{M-1}: the M successive
// vector_vector_addition(q, 1.0, q, c_i, v_i) launches of a Gram-Schmidt
// sweep (domain.tpp:817-822, subdomain.tpp:4396-4401) or of the solution
// update (domain.tpp:902-907) in one pass: q is read and written once, each
// element goes through the same operations in the same order.
template <int M>
struct MultiAxpyOp
{
    double *q;
    const double *v[M];
    double c[M];
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        auto x = a.ld(q, i);
#pragma unroll
        for (int k = 0; k < M; k++) x = 1.0 * x + c[k] * a.ld(v[k], i);
        a.st(q, i, x);
    }
    template <typename F>
    void pointers(F f) const
    {
        f(q);
        for (int k = 0; k < M; k++) f(v[k]);
    }
};

template <int M>
int launch_multi_axpy(double *q, const double *coeffs, const double *const *v, int n, void *stream)
{
    MultiAxpyOp<M> op;
    op.q = q;
    for (int k = 0; k < M; k++)
    {
        op.v[k] = v[k];
        op.c[k] = coeffs[k];
    }
    return launch_ew(op, n, stream);
}

// the same with the coefficients read from device memory (the output of fdd_gmres_finish_dev): fdd_lincomb (fdd_stream.h)
template <int M>
struct MultiAxpyDevOp
{
    double *q;
    const double *v[M];
    const double *c;
    const double *vs; // optional per-vector scales: v_k stands for vs[k] * v_k
    bool from_zero;   // q is known to be 0 (it was just cleared): it is not read, 1.0*0 + c*v is c*v all the same
    const double *last; // optional: only vectors 0..(int)*last enter (a count that never left the device)
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const auto x = from_zero ? a.all(0.0) : a.ld(q, i);
        a.st(q, i, fdd_lincomb<M>(x, last ? (int)*last : M - 1, c, vs, [&](int k) { return a.ld(v[k], i); }));
    }
    template <typename F>
    void pointers(F f) const
    {
        f(q);
        for (int k = 0; k < M; k++) f(v[k]);
    }
};

template <int M>
int launch_multi_axpy_dev(double *q, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, bool from_zero, const double *last_dev, int n, void *stream)
{
    MultiAxpyDevOp<M> op;
    op.q = q;
    op.c = coeffs_dev;
    op.vs = v_scale_dev;
    op.from_zero = from_zero;
    op.last = last_dev;
    for (int k = 0; k < M; k++) op.v[k] = v[k];
    return launch_ew(op, n, stream);
}

// ------------------------------------------------------------ AMG/kernels.cu
struct ScaledResidualOp // AMG/kernels.cu:25-41
{
    double *Sr;
    double *w;
    const double *f_m_Au;
    const double *S;
    double alpha;
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const auto sr = a.ld(S, i) * a.ld(f_m_Au, i);
        a.st(Sr, i, sr);
        a.st(w, i, alpha * sr);
    }
    template <typename F>
    void pointers(F f) const { f(Sr), f(w), f(f_m_Au), f(S); }
};

// scaled_residual from u = 0 (f - A u is f) followed by vector_multiplication: Sr = S*f, work = D*(alpha*Sr); T = double or float
template <typename A, typename T>
__device__ __forceinline__ void smooth_start_at(A a, long long i, T *work, T *Sr, const T *f, const T *S, T alpha)
{
    const auto s = a.ld(S, i), sr = s * a.ld(f, i);
    a.st(Sr, i, sr);
    a.st(work, i, s * (alpha * sr));
}

struct SmoothStartOp
{
    double *work;
    double *Sr;
    const double *f;
    const double *S;
    double alpha;
    template <typename A>
    __device__ void at(A a, long long i) const { smooth_start_at(a, i, work, Sr, f, S, alpha); }
    template <typename F>
    void pointers(F fn) const { fn(work), fn(Sr), fn(f), fn(S); }
};

// ---- Float = float (AMG/config.hpp:4): the two element-wise kernels the fused f32 V-cycle launches.  Their pairs are
// 8 bytes, but the entries have always asked 16 of their pointers before they walk them in pairs, and still do ----
struct SetF32Op // AMG/kernels.cu:11-23
{
    float *data;
    float value;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(data, i, a.all(value)); }
    template <typename F>
    void pointers(F f) const { f(data, 16); }
};

struct SmoothStartF32Op // SmoothStartOp in f32
{
    float *work;
    float *Sr;
    const float *f;
    const float *S;
    float alpha;
    template <typename A>
    __device__ void at(A a, long long i) const { smooth_start_at(a, i, work, Sr, f, S, alpha); }
    template <typename F>
    void pointers(F fn) const { fn(work, 16), fn(Sr, 16), fn(f, 16), fn(S, 16); }
};

struct PolyEvalOp // AMG/kernels.cu:43-59
{
    double *w;
    double *v;
    const double *r;
    const double *D_val;
    double alpha;
    template <typename A>
    __device__ void at(A a, long long i) const
    {
        const auto vv = a.ld(v, i) * a.ld(D_val, i), rr = a.ld(r, i);
        a.st(v, i, vv);
        a.st(w, i, alpha * rr + vv);
    }
    template <typename F>
    void pointers(F f) const { f(w), f(v), f(r), f(D_val); }
};

struct UpdateFieldOp // AMG/kernels.cu:61-76
{
    double *u;
    const double *w;
    const double *D_val;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(u, i, a.ld(u, i) + a.ld(D_val, i) * a.ld(w, i)); }
    template <typename F>
    void pointers(F f) const { f(u), f(w), f(D_val); }
};

struct VMulOp // AMG/kernels.cu:79-94
{
    double *uv;
    const double *u;
    const double *v;
    template <typename A>
    __device__ void at(A a, long long i) const { a.st(uv, i, a.ld(u, i) * a.ld(v, i)); }
    template <typename F>
    void pointers(F f) const { f(uv), f(u), f(v); }
};

static int initialize_arrays(double *u_k, double *r_k, const double *f, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(u_k != nullptr && r_k != nullptr && f != nullptr);
    return launch_ew(InitOp{u_k, r_k, f}, n, stream);
}

template <typename S>
static int update_ur(double *u_k, double *r_kp1, const double *r_k, const double *p_k, const double *q_k, S alpha, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(u_k != nullptr && r_kp1 != nullptr && r_k != nullptr && p_k != nullptr && q_k != nullptr);
    return launch_ew(UpdateUROp<S>{u_k, r_kp1, r_k, p_k, q_k, alpha}, n, stream);
}

template <typename S>
static int update_pr(double *p_k, double *r_k, const double *z_k, const double *r_kp1, S beta, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(p_k != nullptr && r_k != nullptr && z_k != nullptr && r_kp1 != nullptr);
    return launch_ew(UpdatePROp<S>{p_k, r_k, z_k, r_kp1, beta}, n, stream);
}

} // namespace

extern "C" {

int fdd_set_to_value(double *u, double alpha, int n, int offset, void *stream)
{
    FDD_REQUIRE(n >= 0 && offset >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(u != nullptr);
    double *p = u + offset;
    return launch_ew(SetOp{p, alpha}, n, stream);
}

int fdd_invert_vector_elements(double *u, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(u != nullptr);
    return launch_ew(InvertOp{u}, n, stream);
}

int fdd_vector_vector_addition(double *uv, double alpha, const double *u, double beta, const double *v, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(uv != nullptr && u != nullptr && v != nullptr);
    return launch_ew(AxpbyOp{uv, u, v, alpha, beta}, n, stream);
}

int fdd_vector_scaling(double *au, double alpha, const double *u, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(au != nullptr && u != nullptr);
    return launch_ew(ScaleOp{au, u, alpha}, n, stream);
}

int fdd_sqrt_sum_dev(double *out, const double *parts_dev, int nparts, void *stream)
{
    FDD_REQUIRE(out != nullptr && parts_dev != nullptr && nparts >= 1);
    hipLaunchKernelGGL(fdd_sqrt_sum_kernel, dim3(1), dim3(64), 0, fdd_stream(stream), out, parts_dev, nparts);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_xpby_ratio_dev(double *out, const double *x, const double *num_dev, const double *den_dev, const double *y, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(out != nullptr && x != nullptr && y != nullptr && num_dev != nullptr && den_dev != nullptr);
    return launch_ew(XpbyRatioDevOp{out, x, y, num_dev, den_dev}, n, stream);
}

int fdd_xmay_ratio_dev(double *out, const double *x, const double *num_dev, const double *den_dev, const double *y, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(out != nullptr && x != nullptr && y != nullptr && num_dev != nullptr && den_dev != nullptr);
    return launch_ew(XmayRatioDevOp{out, x, y, num_dev, den_dev}, n, stream);
}

int fdd_dom_solution_direction_update_dev(double *u_k, double *p_k, const double *z_k, const double *alpha_num, const double *alpha_den, const double *beta_num, const double *beta_den, int num_points, void *stream)
{
    FDD_REQUIRE(num_points >= 0);
    if (num_points == 0) return 0;
    FDD_REQUIRE(u_k != nullptr && p_k != nullptr && z_k != nullptr && u_k != p_k && alpha_num != nullptr && alpha_den != nullptr && beta_num != nullptr && beta_den != nullptr);
    return launch_ew(SolutionDirectionDevOp{u_k, p_k, z_k, alpha_num, alpha_den, beta_num, beta_den}, num_points, stream);
}

int fdd_vector_scaling_dev(double *au, const double *scale_dev, const double *u, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(au != nullptr && u != nullptr && scale_dev != nullptr);
    return launch_ew(ScaleDevOp{au, u, scale_dev}, n, stream);
}

int fdd_vector_diagonal_scaling_dev(double *z, const double *d, const double *scale_dev, const double *u, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(z != nullptr && u != nullptr && d != nullptr);
    return launch_ew(DiagScaleDevOp{z, d, u, scale_dev}, n, stream);
}

int fdd_cheby_step(double *x, double *d, double *r_out, const double *r_in, const double *q, const double *dinv, double c_d, double c_r, int first, int last, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(x != nullptr && r_in != nullptr && dinv != nullptr);
    FDD_REQUIRE(last || d != nullptr);
    FDD_REQUIRE(first || (q != nullptr && d != nullptr && (last || r_out != nullptr)));
    return launch_ew(ChebyStepOp{x, d, r_out, r_in, q, dinv, c_d, c_r, first ? 1 : 0, last ? 1 : 0}, n, stream);
}

int fdd_vector_scaling_rsqrt_dev(double *au, const double *norm2_dev, const double *u, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(au != nullptr && u != nullptr && norm2_dev != nullptr);
    return launch_ew(ScaleRsqrtDevOp{au, u, norm2_dev}, n, stream);
}

int fdd_dom_initialize_arrays(double *u_k, double *r_k, const double *f, int num_points, void *stream)
{
    return initialize_arrays(u_k, r_k, f, num_points, stream);
}

int fdd_sub_initialize_arrays(double *u_k, double *r_k, const double *f, int num_values, void *stream)
{
    return initialize_arrays(u_k, r_k, f, num_values, stream);
}

int fdd_dom_solution_and_residual_update(double *u_k, double *r_kp1, const double *r_k, const double *p_k, const double *q_k, double alpha_k, int num_points, void *stream)
{
    return update_ur(u_k, r_kp1, r_k, p_k, q_k, ScalarByValue{alpha_k}, num_points, stream);
}

int fdd_sub_solution_and_residual_update(double *u_k, double *r_kp1, const double *r_k, const double *p_k, const double *q_k, double alpha_k, int num_values, void *stream)
{
    return update_ur(u_k, r_kp1, r_k, p_k, q_k, ScalarByValue{alpha_k}, num_values, stream);
}

int fdd_dom_solution_and_residual_update_dev(double *u_k, double *r_kp1, const double *r_k, const double *p_k, const double *q_k, const double *alpha_num, const double *alpha_den, int num_points, void *stream)
{
    FDD_REQUIRE(alpha_num != nullptr && alpha_den != nullptr);
    return update_ur(u_k, r_kp1, r_k, p_k, q_k, ScalarRatioDev{alpha_num, alpha_den}, num_points, stream);
}

int fdd_dom_residual_and_search_update(double *p_k, double *r_k, const double *z_k, const double *r_kp1, double beta_k, int num_points, void *stream)
{
    return update_pr(p_k, r_k, z_k, r_kp1, ScalarByValue{beta_k}, num_points, stream);
}

int fdd_sub_residual_and_search_update(double *p_k, double *r_k, const double *z_k, const double *r_kp1, double beta_k, int num_values, void *stream)
{
    return update_pr(p_k, r_k, z_k, r_kp1, ScalarByValue{beta_k}, num_values, stream);
}

int fdd_dom_residual_and_search_update_dev(double *p_k, double *r_k, const double *z_k, const double *r_kp1, const double *beta_num, const double *beta_den, int num_points, void *stream)
{
    FDD_REQUIRE(beta_num != nullptr && beta_den != nullptr);
    return update_pr(p_k, r_k, z_k, r_kp1, ScalarRatioDev{beta_num, beta_den}, num_points, stream);
}

int fdd_sub_copy_f64_f64(double *u, const double *v, int num_points, void *stream)
{
    FDD_REQUIRE(num_points >= 0);
    if (num_points == 0) return 0;
    FDD_REQUIRE(u != nullptr && v != nullptr);
    return launch_ew(CopyOp{u, v}, num_points, stream);
}

int fdd_sub_copy_f32_f64(float *u, const double *v, int num_points, void *stream)
{
    FDD_REQUIRE(num_points >= 0);
    if (num_points == 0) return 0;
    FDD_REQUIRE(u != nullptr && v != nullptr);
    return launch_ew(CopyF32F64Op{u, v}, num_points, stream);
}

int fdd_sub_copy_f64_f32(double *u, const float *v, int num_points, void *stream)
{
    FDD_REQUIRE(num_points >= 0);
    if (num_points == 0) return 0;
    FDD_REQUIRE(u != nullptr && v != nullptr);
    return launch_ew(CopyF64F32Op{u, v}, num_points, stream);
}

int fdd_multi_axpy(double *q, const double *coeffs, const double *const *v, int m, int n, void *stream)
{
    FDD_REQUIRE(n >= 0 && m >= 1 && m <= FDD_MULTI_MAX);
    if (n == 0) return 0;
    FDD_REQUIRE(q != nullptr && coeffs != nullptr && v != nullptr);
    for (int k = 0; k < m; k++) FDD_REQUIRE(v[k] != nullptr && v[k] != q);
    switch (m)
    {
    case 1: return launch_multi_axpy<1>(q, coeffs, v, n, stream);
    case 2: return launch_multi_axpy<2>(q, coeffs, v, n, stream);
    case 3: return launch_multi_axpy<3>(q, coeffs, v, n, stream);
    case 4: return launch_multi_axpy<4>(q, coeffs, v, n, stream);
    case 5: return launch_multi_axpy<5>(q, coeffs, v, n, stream);
    case 6: return launch_multi_axpy<6>(q, coeffs, v, n, stream);
    case 7: return launch_multi_axpy<7>(q, coeffs, v, n, stream);
    default: return launch_multi_axpy<8>(q, coeffs, v, n, stream);
    }
}

int fdd_multi_axpy_dev(double *q, const double *coeffs_dev, const double *const *v, int m, int n, void *stream)
{
    return fdd_multi_axpy_scaled_dev(q, coeffs_dev, v, nullptr, m, n, stream);
}

int fdd_multi_axpy_scaled_dev(double *q, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, int m, int n, void *stream)
{
    return fdd_multi_lincomb_scaled_dev(q, 0, coeffs_dev, v, v_scale_dev, m, n, stream);
}

int fdd_multi_lincomb_scaled_dev(double *q, int q_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, int m, int n, void *stream)
{
    return fdd_multi_lincomb_limited_dev(q, q_is_zero, coeffs_dev, v, v_scale_dev, nullptr, m, n, stream);
}

int fdd_multi_lincomb_limited_dev(double *q, int q_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, const double *last_dev, int m, int n, void *stream)
{
    const bool from_zero = q_is_zero != 0;
    FDD_REQUIRE(n >= 0 && m >= 1 && m <= FDD_MULTI_MAX);
    if (n == 0) return 0;
    FDD_REQUIRE(q != nullptr && coeffs_dev != nullptr && v != nullptr);
    for (int k = 0; k < m; k++) FDD_REQUIRE(v[k] != nullptr && v[k] != q);
    switch (m)
    {
    case 1: return launch_multi_axpy_dev<1>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    case 2: return launch_multi_axpy_dev<2>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    case 3: return launch_multi_axpy_dev<3>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    case 4: return launch_multi_axpy_dev<4>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    case 5: return launch_multi_axpy_dev<5>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    case 6: return launch_multi_axpy_dev<6>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    case 7: return launch_multi_axpy_dev<7>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    default: return launch_multi_axpy_dev<8>(q, coeffs_dev, v, v_scale_dev, from_zero, last_dev, n, stream);
    }
}

int fdd_amg_vector_set_to_value(double *data, double value, int size, void *stream)
{
    return fdd_set_to_value(data, value, size, 0, stream);
}

int fdd_amg_main_scaled_residual(double *Sr, double *w, const double *f_m_Au, const double *S, double alpha, int size, void *stream)
{
    FDD_REQUIRE(size >= 0);
    if (size == 0) return 0;
    FDD_REQUIRE(Sr != nullptr && w != nullptr && f_m_Au != nullptr && S != nullptr);
    return launch_ew(ScaledResidualOp{Sr, w, f_m_Au, S, alpha}, size, stream);
}

int fdd_amg_smooth_start(double *work, double *Sr, const double *f, const double *D_val, double coef, int size, void *stream)
{
    FDD_REQUIRE(size >= 0);
    if (size == 0) return 0;
    FDD_REQUIRE(work != nullptr && Sr != nullptr && f != nullptr && D_val != nullptr);
    return launch_ew(SmoothStartOp{work, Sr, f, D_val, coef}, size, stream);
}

int fdd_amg_vector_set_to_value_f32(float *data, float value, int size, void *stream)
{
    FDD_REQUIRE(size >= 0);
    if (size == 0) return 0;
    FDD_REQUIRE(data != nullptr);
    return launch_ew(SetF32Op{data, value}, size, stream);
}

int fdd_amg_smooth_start_f32(float *work, float *Sr, const float *f, const float *D_val, float coef, int size, void *stream)
{
    FDD_REQUIRE(size >= 0);
    if (size == 0) return 0;
    FDD_REQUIRE(work != nullptr && Sr != nullptr && f != nullptr && D_val != nullptr);
    return launch_ew(SmoothStartF32Op{work, Sr, f, D_val, coef}, size, stream);
}

int fdd_amg_main_polynomial_evaluation(double *w, double *v, const double *r, const double *D_val, double alpha, int size, void *stream)
{
    FDD_REQUIRE(size >= 0);
    if (size == 0) return 0;
    FDD_REQUIRE(w != nullptr && v != nullptr && r != nullptr && D_val != nullptr);
    return launch_ew(PolyEvalOp{w, v, r, D_val, alpha}, size, stream);
}

int fdd_amg_main_update_field(double *u, const double *w, const double *D_val, int size, void *stream)
{
    FDD_REQUIRE(size >= 0);
    if (size == 0) return 0;
    FDD_REQUIRE(u != nullptr && w != nullptr && D_val != nullptr);
    return launch_ew(UpdateFieldOp{u, w, D_val}, size, stream);
}

int fdd_amg_vector_multiplication(double *uv, const double *u, const double *v, int size, void *stream)
{
    FDD_REQUIRE(size >= 0);
    if (size == 0) return 0;
    FDD_REQUIRE(uv != nullptr && u != nullptr && v != nullptr);
    return launch_ew(VMulOp{uv, u, v}, size, stream);
}

} // extern "C"
